// inflate_kernels.hip.inc -- BGZF blocks inflated on the device (cs_inflate_bgzf), and the k-th newline of a text that
// is already there (cs_dtext_after_kth_newline).
//
// The decoder is include/cutseq_inflate.h: bit reader, header parsing, table construction, symbol decode and every
// bounds decision are the code the host check runs under the sanitizers.  This file adds how a wavefront shares the
// work: one wave per block; all 64 lanes run the symbol loop on the same values (bit buffer and control flow are
// wave-uniform), the tables are built cooperatively in LDS, and the bytes are moved by all lanes --
//   literals   wait in a register, lane i holding the i-th one, and leave 64 at a time (or in front of a match);
//   matches    are copied by the lanes side by side, the distance < length case replicated modulo the distance (every
//              source byte then lies in front of the match);
//   stored     blocks are copied straight from the payload.
// The text goes to global memory, not to a 64 KB LDS window (two waves per CU would be left): a match reads bytes other
// lanes stored, so a workgroup-scope fence and a wait for the stores stand between.  When the stream has ended, every
// lane runs the CRC of its slice of the text and counts the line ends in it; log steps join the slices.
#include "../../include/cutseq_inflate.h"

namespace csinflate {

struct WaveSink {
  uint8_t *out;
  uint32_t lane;
  uint32_t held = 0;   // this lane's waiting literal
  uint32_t nheld = 0;  // literals waiting in the wave: those of out[end - nheld .. end)

  __device__ static void stores_visible() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __device__ void flush(uint32_t end) {
    if (nheld) {
      if (lane < nheld) out[end - nheld + lane] = (uint8_t)held;
      nheld = 0;
    }
  }
  __device__ void lit(uint32_t pos, uint32_t byte) {
    if (nheld == lane) held = byte;
    if (++nheld == 64) flush(pos + 1);
  }
  __device__ void match(uint32_t pos, uint32_t len, uint32_t dist) {
    flush(pos);
    stores_visible();
    const uint8_t *src = out + pos - dist;
    if (dist >= len) {
      for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[i];
    } else {
      for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[i % dist];
    }
  }
  __device__ void stored(uint32_t pos, const uint8_t *src, uint32_t len) {
    flush(pos);
    for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[i];
  }
  __device__ void finish(uint32_t pos) {
    flush(pos);
    stores_visible();
  }
};

// One wave per table entry.  verdict[b]: CSI_*; lines[b]: '\n' in the block's text (0 for a refused block).
__global__ __launch_bounds__(64) void inflate_bgzf(const uint8_t *__restrict__ comp, const cs_inflate_block *__restrict__ blocks,
                                                   uint32_t n_blocks, uint8_t *text, uint32_t *__restrict__ verdict,
                                                   uint32_t *__restrict__ lines) {
  __shared__ csi_shared sh;
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  if (b >= n_blocks) return;
  const cs_inflate_block blk = blocks[b];
  uint8_t *out = text + blk.out_off;
  WaveSink sink;
  sink.out = out;
  sink.lane = lane;
  csi_crc_table(sh.crc_tab, lane, 64);
  uint32_t produced = 0;
  uint32_t err = csi_inflate_stream(sh, comp + blk.comp_off, blk.comp_len, blk.out_len, sink, lane, 64u, &produced);
  err = CSI_UNIFORM(err);
  uint32_t n_lines = 0;
  if (err == CSI_OK) {
    __syncthreads();  // (the CRC table)
    uint32_t crc = csi_crc_slice(out, blk.out_len, sh.crc_tab, lane, 64, &n_lines);
    uint32_t shift = csi_xpow8((blk.out_len + 63u) / 64u);
    for (uint32_t step = 1; step < 64; step <<= 1) {  // lane 0 ends up with slices 0 .. 63 joined
      crc = csi_crc_join(crc, (uint32_t)__shfl_down((int)crc, step), shift);
      shift = csi_mulmod(shift, shift);
      n_lines += (uint32_t)__shfl_down((int)n_lines, step);
    }
    if (csi_crc_final(CSI_UNIFORM(crc), blk.out_len) != blk.crc32) err = CSI_ERR_CRC;
  }
  if (lane == 0) {
    verdict[b] = err;
    lines[b] = err == CSI_OK ? n_lines : 0u;
  }
}

// The offset behind newline number k (k >= 1) of text[0 .. n), or -1 when the text has fewer: one workgroup walks the
// text in pieces of 16 KB, 16 bytes a thread, until the piece that holds it.
constexpr uint32_t kNlThreads = 1024, kNlBytes = 16;

__global__ __launch_bounds__(1024) void after_kth_newline(const uint8_t *__restrict__ text, uint64_t n, uint64_t k,
                                                          long long *__restrict__ result) {
  __shared__ uint32_t wave_sum[kNlThreads / 64];
  __shared__ long long found;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  if (t == 0) found = -1;
  uint64_t seen = 0;  // newlines in front of the piece
  for (uint64_t piece = 0; piece < n; piece += (uint64_t)kNlThreads * kNlBytes) {
    const uint64_t lo = piece + (uint64_t)t * kNlBytes, hi = lo + kNlBytes < n ? lo + kNlBytes : n;
    uint32_t mine = 0;
    for (uint64_t i = lo; i < hi; ++i) mine += text[i] == '\n';
    uint32_t incl = mine;  // inclusive scan over the wave, then over the waves
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    __syncthreads();  // (the previous piece's readers of wave_sum)
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kNlThreads / 64; ++w) {
      if (w < wave) before += wave_sum[w];
      total += wave_sum[w];
    }
    const uint64_t first = seen + before + incl - mine;  // newlines in front of this thread's bytes
    if (mine && first < k && k <= first + mine) {
      uint64_t left = k - first;
      for (uint64_t i = lo; i < hi; ++i)
        if (text[i] == '\n' && --left == 0) {
          found = (long long)(i + 1);
          break;
        }
    }
    seen += total;
    if (seen >= k) break;  // (uniform: every thread has the same `seen`)
  }
  __syncthreads();
  if (t == 0) *result = found;
}

}  // namespace csinflate
