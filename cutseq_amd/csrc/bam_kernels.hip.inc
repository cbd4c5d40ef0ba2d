// bam_kernels.hip.inc -- unaligned BAM records -> the four-line FASTQ text the text path parses (cs_text_submit_bam).
//
// The front step of the text path for a BAM input: the host has walked the length-prefixed chain (csh_bam_walk) and
// uploads the raw record bytes with their offsets; three launches per text put the FASTQ text into the slot's text
// buffer, where text_count_nl and everything behind it find it as if it had been uploaded:
//
//   bam_sizes         one thread per record: the fixed fields, every refusal of include/cutseq_bam.h (csb_shape, then
//                     csb_check: name, flag, qualities), the record's text length, in-block prefix and per-block sums
//   text_scan_blocks  (text_kernels.hip.inc, as it is) the blocks' sums -> their text offsets
//   bam_expand        32 lanes per record, format_copy's shape: '@' name '\n' | letters, eight per four packed bytes
//                     through the 16-entry table (two register pairs) | "\n+\n" | qual + 33, a packed add | '\n'
//
// A refused record lands in TextMeta.err as the smallest (record, code) key like every other reader error; bam_expand and
// every later kernel return on it.  The key is kept in a word of the front step's own as well (BamArgs.err): the newline
// passes behind it do not look at TextMeta.err, find no lines in a text nobody wrote, and put their line-count key on
// record 0 in front of it.  cs_text_wait reports the front step's key when there is one.
//
// For ANY record bytes the kernels read only rec[off[r] .. off[r + 1]) and write only text[0 .. cap): csb_shape vouches
// for the lengths before name, bases or qualities are touched, and a record whose text would leave `cap` (the size the
// host derived from the same fields) is not written.
#include "../../include/cutseq_bam.h"

namespace csbam {

struct BamArgs {
  const uint8_t *rec;    // the records of one text, back to back
  const uint32_t *off;   // n + 1 ascending offsets into rec, every record at least CSB_FIXED bytes (the host checked)
  uint32_t n;
  uint32_t *toff;        // per record: its text's offset inside its block of 256 records
  uint32_t *blk;         // per block: text bytes; behind text_scan_blocks the block's text offset
  uint8_t *text;         // the slot's text buffer
  uint32_t cap;          // bytes of text the host announced: nothing is written beyond
  uint32_t mate_flag;    // CS_TEXT_ERR_BAM_MATE2 on mate 2's text
  unsigned long long *err;  // the smallest (record << 8 | code) key of a refused record over the batch's texts; ~0: none
  cstext::TextMeta *meta;
};

__global__ void __launch_bounds__(256) bam_sizes(BamArgs a) {
  __shared__ uint32_t sh[8];
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  uint32_t len = 0;
  if (r < a.n) {
    const uint32_t at = a.off[r], avail = a.off[r + 1u] - at;
    const uint8_t *rec = a.rec + at;
    csb_shape_t s;
    int code = csb_shape(rec, avail, &s);
    if (code == CSB_OK) {
      len = s.text_len;
      code = csb_check(rec, &s);
    }
    if (code != CSB_OK) {
      atomicMin(a.err, ((unsigned long long)r << 8) | (uint32_t)code | a.mate_flag);
      cstext::report(a.meta, r, (uint32_t)code | a.mate_flag);
    }
  }
  uint32_t total;
  const uint32_t before = cstext::block_scan_256(len, total, sh);
  if (r < a.n) a.toff[r] = before;
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// stretch_store (text_kernels.hip.inc) with 33 added to every byte.  No byte carries into its neighbour: bam_sizes let
// no quality above 93 pass (and whatever the bytes, a carry stays inside the dword that is stored).
__device__ __forceinline__ void stretch_store_phred(uint32_t lane, uint8_t *dst, const uint8_t *src, uint32_t n,
                                                    const cstext::Held &h) {
  constexpr uint32_t kAdd = 0x21212121u;
  const uint32_t i0 = 4u * lane, i1 = i0 + 128u, r = n & 3u;
  uint32_t v;
  if (i0 + 4u <= n) {
    v = h.v0 + kAdd;
    __builtin_memcpy(dst + i0, &v, 4);
  }
  if (i1 + 4u <= n) {
    v = h.v1 + kAdd;
    __builtin_memcpy(dst + i1, &v, 4);
  }
  if (lane < r) dst[n - r + lane] = (uint8_t)(h.tail + 33u);
  for (uint32_t i = i0 + 256u; i + 4u <= n; i += 128u) {
    __builtin_memcpy(&v, src + i, 4);
    v += kAdd;
    __builtin_memcpy(dst + i, &v, 4);
  }
}

__global__ void __launch_bounds__(256) bam_expand(BamArgs a) {
  if (a.meta->err != ~0ull) return;
  const uint32_t lane = threadIdx.x & 31u;
  for (uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 5; r < a.n; r += (gridDim.x * 256u) >> 5) {
    const uint32_t at = a.off[r], avail = a.off[r + 1u] - at;
    const uint8_t *rec = a.rec + at;
    csb_shape_t s;
    if (csb_shape(rec, avail, &s) != CSB_OK) continue;  // (bam_sizes has reported it; uniform over the record's lanes)
    const uint32_t dst = a.blk[r >> 8] + a.toff[r];
    if ((unsigned long long)dst + s.text_len > a.cap) {  // the fields are not the ones the host sized the text by
      if (lane == 0) cstext::report(a.meta, 0, cstext::ERR_LINE_COUNT);
      continue;
    }
    uint8_t *out = a.text + dst;
    const uint32_t nm = s.l_name - 1u, L = s.l_seq;  // (csb_check: l_name >= 1)
    const uint8_t *name = rec + s.name_at, *seq = rec + s.seq_at, *qual = rec + s.qual_at;
    // segment ends: '@' | name | '\n' | letters | "\n+\n" | qualities | '\n'
    const uint32_t e_name = 1u + nm, e_seq = e_name + 1u + L, e_plus = e_seq + 3u;
    // every stretch's loads in front of the first store, as in format_copy
    const cstext::Held h_name = cstext::stretch_load(lane, name, nm);
    const cstext::Held h_qual = cstext::stretch_load(lane, qual, L);
    const uint32_t groups = L >> 3, rest = L & 7u;  // a group: four packed bytes, eight letters
    uint32_t packed = 0, last = 0;
    if (lane < groups) __builtin_memcpy(&packed, seq + 4u * lane, 4);
    if (lane < rest) last = seq[4u * groups + (lane >> 1)];
    if (lane == 0) out[0] = '@';
    cstext::stretch_store(lane, out + 1u, name, nm, h_name);
    if (lane == 1) out[e_name] = '\n';
    uint8_t *bases = out + e_name + 1u;
    uint32_t lo, hi;
    if (lane < groups) {
      csb_letters8(packed, &lo, &hi);
      __builtin_memcpy(bases + 8u * lane, &lo, 4);
      __builtin_memcpy(bases + 8u * lane + 4u, &hi, 4);
    }
    for (uint32_t g = lane + 32u; g < groups; g += 32u) {
      __builtin_memcpy(&packed, seq + 4u * g, 4);
      csb_letters8(packed, &lo, &hi);
      __builtin_memcpy(bases + 8u * g, &lo, 4);
      __builtin_memcpy(bases + 8u * g + 4u, &hi, 4);
    }
    // (an odd l_seq: the last byte's low nibble is no base and is not written)
    if (lane < rest) bases[8u * groups + lane] = (uint8_t)csb_letter((lane & 1u) ? last & 15u : last >> 4);
    if (lane >= 2 && lane <= 4) out[e_seq + lane - 2u] = lane == 3 ? (uint8_t)'+' : (uint8_t)'\n';
    stretch_store_phred(lane, out + e_plus, qual, L, h_qual);
    if (lane == 5) out[e_plus + L] = '\n';
  }
}

}  // namespace csbam
