// deflate_kernels.hip.inc -- gzip members of the output streams, written on the device (device code only).
// Included by cutseq_hip.hip behind text_kernels.hip.inc.  gfx950 / wave64 only.
//
// The reference writes its .fastq.gz outputs through xopen at compression level 1 (cutadapt's default; cutseq/run.py
// 434-441, 751-758 via OutputFiles).  On the host that deflate is the most expensive thing left once the device parses
// and formats (CUTSEQ_PROFILE=1 at the time: ~12 CPU-seconds per 8 M pairs against ~6 for the inflate), so for ".gz"
// outputs the text path compresses on the device: every 32 KB chunk of an output stream becomes one deflate block with
// its own dynamic Huffman codes, ended by an empty stored block so that chunks are byte-aligned and can be laid out
// by byte copies (the pigz trick), CRC-32 per chunk from 128-byte slices combined with GF(2) polynomial arithmetic.
// The LZ77 stage is the cheap part of what level 1 finds in FASTQ text, and every thread finds it on its own 128 bytes:
//   * runs (distance 1): quality strings are runs of a few values, homopolymers are runs of a base;
//   * the record name against the PREVIOUS record's name (the line four -- FASTA: two -- line ends back): neighbouring
//     names share everything but a coordinate.
// Bases stay literals: two bits of information each whatever a matcher does.  Round 3's literal-only blocks came out
// 23 % larger than zlib level 1 on the bench reads (ratio 2.65 against 3.26); profiles/r04_gzip_ratio.json has both.  A chunk that does not shrink is stored.  The layout kernel
// wraps the chunks of a stream into ONE gzip member (header, blocks, final empty block, CRC-32, ISIZE): the host
// writes the bytes it downloads, nothing else.  Any inflater reads the result; what parity is defined on -- the
// decompressed bytes -- is unchanged.
// BGZF (cs_text_params.compress = 2, the CLI's --bgzf): the same chunks, each a gzip member of its own with htslib's
// 'BC' extra field -- deflate_chunks<true> and bgzf_layout in place of deflate_chunks<false>, deflate_layout and
// deflate_compact; see bgzf_layout.

namespace csdefl {

constexpr uint32_t kChunk = 32768;   // raw bytes per deflate block
constexpr uint32_t kSlice = 128;     // raw bytes per thread (256 threads)
constexpr uint32_t kOutWords = 5120; // LDS bit buffer: 20 KB (a chunk that does not shrink below 5/8 is stored instead; round 4
                                     // kept 36 KB and with it three blocks per CU instead of five)
constexpr uint32_t kSlot = kChunk + 64;  // staging bytes per chunk
constexpr uint32_t kPoly = 0xedb88320u;

struct ChunkInfo {  // per chunk, written by deflate_chunks
  uint32_t comp_len, raw_len, crc, route;
};

__constant__ uint32_t c_x2n[32];       // x^(2^n) mod p (zlib's x2n_table), uploaded by the host
__constant__ uint32_t c_shift128[256];  // x^(8 * 128 * i) mod p

// multmodp / x2nmodp: polynomial multiplication and x^(n * 2^k) modulo the CRC-32 polynomial, after the routines of the
// same names in zlib's crc32.c (Mark Adler; zlib licence: "This software is provided 'as-is' ... Permission is granted
// to anyone to use this software for any purpose, including commercial applications, and to alter it and redistribute
// it freely" with the origin not misrepresented -- it is zlib's, restated here for the device).  c_x2n is zlib's
// x2n_table, built by the host at start-up.
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1u)) == 0u) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}
__device__ __forceinline__ uint32_t x2nmodp(uint32_t n, uint32_t k) {  // x^(n * 2^k)
  uint32_t p = 1u << 31;
  while (n) {
    if (n & 1u) p = multmodp(c_x2n[k & 31u], p);
    n >>= 1;
    ++k;
  }
  return p;
}

// Huffman code (lengths limited to `maxlen`, canonical codes of RFC 1951 3.2.2 bit-reversed for LSB-first packing) for
// `nsym` <= 288 symbols with frequencies freq[] -> len[], tab[s] = code | len << 16.  The WHOLE BLOCK (256 threads) builds
// it (round 5; one thread walking 286 symbols five times over, with its counters in scratch memory, was most of a
// chunk's time): used symbols compacted by a scan, sorted by rank counting, ONE thread merges the two queues (the only
// serial part, one step per used symbol: a few dozen in FASTQ text), the length limit is enforced on the length
// histogram miniz-style, codes are assigned from per-wave ballots.  Every thread must call it; barriers inside.
struct HuffScratch {
  uint16_t usym[288];    // used symbols in symbol order, then (order[]) by ascending (frequency, symbol)
  uint16_t order[288];
  uint32_t ufreq[288];
  uint32_t weight[576];  // leaves in order[], then internal nodes
  uint16_t parent[576];
  uint8_t depth[576];
  uint32_t count[64];    // codes per length
  uint32_t wave_cnt[5][16];  // canonical codes: symbols per (wave round, length)
  uint32_t next[16];
  uint32_t n_used;
};

__device__ void huff_build(const uint32_t *freq, int nsym, int maxlen, uint8_t *len, uint32_t *tab, HuffScratch &w, uint32_t *sh) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // ---- used symbols, in symbol order (two per thread: tid and 256 + tid)
  const uint32_t s1 = 256u + tid;
  const uint32_t f0 = tid < (uint32_t)nsym ? freq[tid] : 0u, f1 = s1 < (uint32_t)nsym ? freq[s1] : 0u;
  uint32_t tot0, tot1;
  const uint32_t at0 = cstext::block_scan_256(f0 ? 1u : 0u, tot0, sh);
  const uint32_t at1 = tot0 + cstext::block_scan_256(f1 ? 1u : 0u, tot1, sh);
  const uint32_t n = tot0 + tot1;
  if (f0) {
    w.usym[at0] = (uint16_t)tid;
    w.ufreq[at0] = f0;
  }
  if (f1) {
    w.usym[at1] = (uint16_t)s1;
    w.ufreq[at1] = f1;
  }
  if (tid < (uint32_t)nsym) {
    len[tid] = 0;
    tab[tid] = 0;
  }
  if (s1 < (uint32_t)nsym) {
    len[s1] = 0;
    tab[s1] = 0;
  }
  if (tid < 64u) w.count[tid] = 0;
  if (tid < 80u) (&w.wave_cnt[0][0])[tid] = 0;
  __syncthreads();
  if (n == 0u) return;  // (block-uniform)
  if (n == 1u) {
    if (tid == 0) {
      len[w.usym[0]] = 1;
      tab[w.usym[0]] = 1u << 16;  // code 0, one bit
    }
    __syncthreads();
    return;
  }
  // ---- ascending (frequency, symbol): every entry counts the entries in front of it (n reads of the same address by
  // all threads: broadcasts)
  for (uint32_t e = tid; e < n; e += 256u) {
    const uint32_t f = w.ufreq[e], sy = w.usym[e];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t fj = w.ufreq[j];
      rank += (fj < f || (fj == f && (uint32_t)w.usym[j] < sy)) ? 1u : 0u;
    }
    w.order[rank] = (uint16_t)sy;
    w.weight[rank] = f;
  }
  __syncthreads();
  // ---- two-queue merge (leaves 0..n-1 ascending, internal nodes n.. in creation order: ascending too)
  if (tid == 0) {
    uint32_t leaf = 0, inode = n, next = n;
    for (uint32_t k = 0; k + 1u < n; ++k) {
      uint32_t pick[2];
      for (int q = 0; q < 2; ++q) {
        if (leaf < n && (inode >= next || w.weight[leaf] <= w.weight[inode]))
          pick[q] = leaf++;
        else
          pick[q] = inode++;
      }
      w.weight[next] = w.weight[pick[0]] + w.weight[pick[1]];
      w.parent[pick[0]] = w.parent[pick[1]] = (uint16_t)next;
      ++next;
    }
    const uint32_t root = next - 1u;
    w.depth[root] = 0;
    for (uint32_t v = root; v-- > n;) w.depth[v] = (uint8_t)min((uint32_t)w.depth[w.parent[v]] + 1u, 63u);
  }
  __syncthreads();
  for (uint32_t e = tid; e < n; e += 256u) atomicAdd(&w.count[min((uint32_t)w.depth[w.parent[e]] + 1u, 63u)], 1u);
  __syncthreads();
  // ---- the length limit on the histogram, then lengths by rank: the rarest symbols get the longest codes
  if (tid == 0) {
    for (int l = maxlen + 1; l < 64; ++l) {
      w.count[maxlen] += w.count[l];
      w.count[l] = 0;
    }
    unsigned long long total = 0;
    for (int l = maxlen; l >= 1; --l) total += (unsigned long long)w.count[l] << (maxlen - l);
    while (total > (1ull << maxlen)) {
      w.count[maxlen]--;
      for (int l = maxlen - 1; l >= 1; --l)
        if (w.count[l]) {
          w.count[l]--;
          w.count[l + 1] += 2;
          break;
        }
      total--;
    }
  }
  __syncthreads();
  for (uint32_t e = tid; e < n; e += 256u) {  // entry e of the ascending order: e codes of at least its length come first
    uint32_t acc = 0, l = (uint32_t)maxlen;
    for (; l >= 1u; --l) {
      acc += w.count[l];
      if (e < acc) break;
    }
    len[w.order[e]] = (uint8_t)l;
  }
  __syncthreads();
  // ---- canonical codes: a symbol's code is next[l] + the number of smaller symbols of the same length.  Round r holds
  // symbols 64 r .. 64 r + 63 (rounds 0..3: this thread's first symbol, round 4: symbols 256..287 in wave 0).
  uint32_t within[2] = {0, 0};
  const uint32_t l0 = tid < (uint32_t)nsym ? len[tid] : 0u, l1 = (wave == 0 && s1 < (uint32_t)nsym) ? len[s1] : 0u;
  for (uint32_t L = 1; L <= (uint32_t)maxlen; ++L) {  // (uniform)
    const unsigned long long m0 = __ballot(l0 == L), m1 = __ballot(l1 == L);
    const uint32_t below0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
    const uint32_t below1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
    if (l0 == L) within[0] = below0;
    if (l1 == L) within[1] = below1;
    if (lane == 0) {
      w.wave_cnt[wave][L] = (uint32_t)__popcll(m0);
      if (wave == 0) w.wave_cnt[4][L] = (uint32_t)__popcll(m1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t code = 0, prev = 0;
    for (uint32_t L = 1; L <= 15u; ++L) {
      code = (code + prev) << 1;
      w.next[L] = code;
      prev = L <= (uint32_t)maxlen ? w.wave_cnt[0][L] + w.wave_cnt[1][L] + w.wave_cnt[2][L] + w.wave_cnt[3][L] + w.wave_cnt[4][L] : 0u;
    }
  }
  __syncthreads();
  if (l0) {
    uint32_t before = 0;
    for (uint32_t r = 0; r < wave; ++r) before += w.wave_cnt[r][l0];
    tab[tid] = (__brev(w.next[l0] + before + within[0]) >> (32u - l0)) | (l0 << 16);
  }
  if (l1) {
    const uint32_t before = w.wave_cnt[0][l1] + w.wave_cnt[1][l1] + w.wave_cnt[2][l1] + w.wave_cnt[3][l1];
    tab[s1] = (__brev(w.next[l1] + before + within[1]) >> (32u - l1)) | (l1 << 16);
  }
  __syncthreads();
}

// ---- the token alphabet of RFC 1951
__device__ __forceinline__ uint32_t length_symbol(uint32_t len, uint32_t &nbits, uint32_t &extra) {  // 3 <= len <= 257
  const uint32_t l = len - 3u;
  if (l < 8u) {
    nbits = extra = 0;
    return 257u + l;
  }
  nbits = (31u - (uint32_t)__clz((int)l)) - 2u;
  extra = l & ((1u << nbits) - 1u);
  return 257u + 4u * nbits + 4u + ((l >> nbits) - 4u);
}
__device__ __forceinline__ uint32_t distance_symbol(uint32_t dist, uint32_t &nbits, uint32_t &extra) {  // 1 <= dist <= 32768
  const uint32_t d = dist - 1u;
  if (d < 4u) {
    nbits = extra = 0;
    return d;
  }
  nbits = (31u - (uint32_t)__clz((int)d)) - 1u;
  extra = d & ((1u << nbits) - 1u);
  return 2u * nbits + 2u + ((d >> nbits) & 1u);
}

constexpr uint32_t kMinRun = 4, kMinNameMatch = 4, kMaxLines = 2304;

// ---- 128-bit position masks of a thread's slice (bit i: byte i), as two 64-bit halves
struct Mask128 {
  unsigned long long lo, hi;
};
__device__ __forceinline__ uint32_t m128_next_set(Mask128 m, uint32_t from) {  // lowest set bit >= from, 128: none
  if (from < 64u) {
    const unsigned long long x = m.lo & (~0ull << from);
    if (x) return (uint32_t)__builtin_ctzll(x);
    from = 64u;
  }
  if (from < 128u) {
    const unsigned long long x = m.hi & (~0ull << (from - 64u));
    if (x) return 64u + (uint32_t)__builtin_ctzll(x);
  }
  return 128u;
}
__device__ __forceinline__ uint32_t m128_next_clear(Mask128 m, uint32_t from) {
  const Mask128 inv = {~m.lo, ~m.hi};
  return m128_next_set(inv, from);
}
__device__ __forceinline__ uint32_t m128_count_below(Mask128 m, uint32_t i) {
  if (i == 0u) return 0u;
  if (i < 64u) return (uint32_t)__popcll(m.lo & ((1ull << i) - 1ull));
  if (i == 64u) return (uint32_t)__popcll(m.lo);
  return (uint32_t)__popcll(m.lo) + (uint32_t)__popcll(i >= 128u ? m.hi : (m.hi & ((1ull << (i - 64u)) - 1ull)));
}
// bytes of `w` equal to the byte `c` replicated in `rep`: one flag bit per byte, gathered into the low nibble
__device__ __forceinline__ uint32_t eq_nibble(uint32_t w, uint32_t rep) {
  const uint32_t x = w ^ rep;
  const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;  // exact zero-byte test
  return (((z >> 7) * 0x01020408u) >> 24) & 0xfu;
}

// One thread's slice as matches, found ONCE on the slice's 32 dwords in registers -- no byte-at-a-time loop whose next
// step waits for a load:
//   runs    bytes equal to the byte in front of them (one XOR against the dword shifted by a byte); a stretch of at
//           least kMinRun such bytes is a match of distance 1
//   names   a record starts where the marker byte follows a line end; the record in front of it starts `lines` line
//           ends back -- the chunk's line ends are indexed in LDS (nl_pos), so that is one look-up -- and the common
//           prefix of the two names is the match (compared four bytes at a time).  A record whose predecessor starts in
//           the chunk in front goes without: one or two names per chunk.
// The matches -- at most 32 of four bytes and more in 128 bytes -- wait in the chunk's staging slot (nothing else uses
// it before the block's last step), everything between them is a literal.
//   match word: position in the slice | (length - 3) << 7 | (distance - 1) << 15
struct SliceMasks {
  Mask128 eq, nl, mark;
};
__device__ __forceinline__ SliceMasks slice_masks(const uint32_t (&w)[32], uint32_t prev_byte, uint32_t n_valid, uint32_t marker) {
  SliceMasks m = {{0, 0}, {0, 0}, {0, 0}};
  const uint32_t mrep = marker * 0x01010101u;
#pragma unroll
  for (int d = 0; d < 32; ++d) {
    const uint32_t before = d == 0 ? prev_byte : (w[d - 1] >> 24);
    const unsigned long long e = eq_nibble(w[d], (w[d] << 8) | before);
    const unsigned long long n = eq_nibble(w[d], 0x0a0a0a0au), k = eq_nibble(w[d], mrep);
    if (d < 16) {
      m.eq.lo |= e << (4 * d);
      m.nl.lo |= n << (4 * d);
      m.mark.lo |= k << (4 * d);
    } else {
      m.eq.hi |= e << (4 * (d - 16));
      m.nl.hi |= n << (4 * (d - 16));
      m.mark.hi |= k << (4 * (d - 16));
    }
  }
  if (n_valid < 128u) {  // the stream's last slice: bytes behind its end are nobody's
    const Mask128 keep = {n_valid >= 64u ? ~0ull : ((1ull << n_valid) - 1ull),
                          n_valid > 64u ? ((1ull << (n_valid - 64u)) - 1ull) : 0ull};
    m.eq.lo &= keep.lo, m.eq.hi &= keep.hi;
    m.nl.lo &= keep.lo, m.nl.hi &= keep.hi;
    m.mark.lo &= keep.lo, m.mark.hi &= keep.hi;
  }
  return m;
}

template <typename Match>
__device__ __forceinline__ void find_matches(const uint8_t *chunk, uint32_t lo, uint32_t n_valid, const SliceMasks &m,
                                              bool line_starts_here, uint32_t lines_before, const uint16_t *nl_pos,
                                              uint32_t lines, bool chunk_starts_line, Match match) {
  // record starts: the marker right behind a line end
  Mask128 starts = {m.mark.lo & ((m.nl.lo << 1) | (line_starts_here ? 1ull : 0ull)), m.mark.hi & ((m.nl.hi << 1) | (m.nl.lo >> 63))};
  uint32_t cur = 0;
  while (cur < n_valid) {
    const uint32_t ns = m128_next_set(starts, cur), rs = m128_next_set(m.eq, cur);
    if (ns >= n_valid && rs >= n_valid) break;
    if (ns <= rs) {
      // line index of this record start = line ends in front of it; its predecessor is `lines` lines back
      const uint32_t q = lines_before + m128_count_below(m.nl, ns);
      uint32_t len = 0, dist = 0;
      if (q >= lines && q - lines < kMaxLines && (q > lines || chunk_starts_line)) {
        const uint32_t p = q == lines ? 0u : (uint32_t)nl_pos[q - lines - 1u] + 1u;  // chunk position of the predecessor
        const uint32_t here = lo + ns, cap = n_valid - ns;
        dist = here - p;
        while (len + 4u <= cap) {  // four bytes at a time (byte loads: the addresses are as they come)
          uint32_t a4, b4;
          __builtin_memcpy(&a4, chunk + p + len, 4);
          __builtin_memcpy(&b4, chunk + here + len, 4);
          if (a4 != b4) {
            len += (uint32_t)__builtin_ctz(a4 ^ b4) >> 3;
            break;
          }
          len += 4u;
        }
        if (len + 4u > cap)
          while (len < cap && chunk[p + len] == chunk[here + len]) ++len;
      }
      if (len >= kMinNameMatch) {
        match(ns, len, dist);
        cur = ns + len;
        continue;
      }
      if (ns < 64u) starts.lo &= ~(1ull << ns); else starts.hi &= ~(1ull << (ns - 64u));
      continue;  // (a run may start at the same place)
    }
    const uint32_t re = min(m128_next_clear(m.eq, rs), n_valid);
    if (re - rs >= kMinRun) match(rs, re - rs, 1u);
    cur = re;
  }
}

// The slice as tokens, in position order, from the slice's dwords IN REGISTERS and its match list: lit(byte) /
// match(length, distance).  Fully unrolled over the 128 positions, so every byte is a compile-time field of a register
// (round 4 walked the slice three times with a byte load from global memory per literal, each behind the previous
// one's atomic: the three walks were most of a block's time).  `covered`: bit i set = byte i belongs to a match.
template <typename Lit, typename Match>
__device__ __forceinline__ void walk_tokens(const uint32_t (&w)[32], uint32_t n_valid, Mask128 covered, const uint32_t *list,
                                             uint32_t n_matches, Lit lit, Match match) {
  uint32_t q = 0;
  uint32_t next_at = n_matches ? (list[0] & 127u) : 128u;
#pragma unroll
  for (int d = 0; d < 32; ++d) {
    if ((uint32_t)(4 * d) >= n_valid) break;
    const uint32_t cov = (uint32_t)((d < 16 ? covered.lo >> (4 * d) : covered.hi >> (4 * (d - 16))) & 0xfull);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t p = (uint32_t)(4 * d + k);
      if (p < n_valid) {
        if (p == next_at) {
          const uint32_t e = list[q];
          match(((e >> 7) & 255u) + 3u, (e >> 15) + 1u);
          ++q;
          next_at = q < n_matches ? (list[q] & 127u) : 128u;
        } else if (!((cov >> k) & 1u)) {
          lit((w[d] >> (8 * k)) & 0xffu);
        }
      }
    }
  }
}

struct DeflateArgs {
  const uint8_t *text;                 // one mate's output text: the route streams back to back
  const unsigned long long *route_bytes;  // [route][mate] for this mate, stride 2
  uint32_t n_routes;                   // 3, or 3 + barcodes for a demultiplexing plan
  uint8_t *stage;                      // kSlot bytes per chunk
  ChunkInfo *info;
  uint32_t max_chunks;
  const unsigned long long *gate;
  uint32_t fasta_classes;              // bit c: the streams of route class c (0 .. 2, 3 = every barcode's) are FASTA.  It
                                       // says where a record starts and how far back its predecessor's name lies:
                                       // '>' and 2 lines, else '@' and 4 (every chunk belongs to one route)
  uint32_t literal_only;               // 1: no LZ77 stage (CUTSEQ_GPU_LZ=0: round 3's blocks)
};

__device__ __forceinline__ void put_bits(uint32_t *obuf, uint32_t &pos, uint32_t bits, uint32_t nbits) {
  // (LDS bit buffer, zeroed; neighbouring threads share boundary words: atomic OR)
  const uint32_t w = pos >> 5, sh = pos & 31u;
  atomicOr(&obuf[w], bits << sh);
  if (sh + nbits > 32u) atomicOr(&obuf[w + 1], bits >> (32u - sh));
  pos += nbits;
}

__device__ __forceinline__ Mask128 m128_range(uint32_t at, uint32_t len) {  // bits [at, at + len), at + len <= 128
  const unsigned long long ones = ~0ull;
  Mask128 m = {0, 0};
  const uint32_t end = at + len;
  if (at < 64u) m.lo = (ones << at) & (end >= 64u ? ones : ((1ull << end) - 1ull));
  if (end > 64u) m.hi = (at >= 64u ? (ones << (at - 64u)) : ones) & (end >= 128u ? ones : ((1ull << (end - 64u)) - 1ull));
  return m;
}

// CRC-32 of a thread's slice: four byte-wise chains over its quarters side by side (a chain's next step waits for an LDS
// look-up: one chain of 128 steps was a block's longest dependent sequence), then the quarters combined -- the CRC of a
// message is its polynomial times x^32 reduced, so crc(A B) = crc'(A) x^(8 |B|) + crc'(B) on the raw registers.
__device__ __forceinline__ uint32_t crc_step(const uint32_t *crc_tab, uint32_t crc, uint32_t byte) {
  return crc_tab[(crc ^ byte) & 0xffu] ^ (crc >> 8);
}

// kBgzf (cs_text_params.compress = 2): the chunk is a stream of its own -- its first byte has no byte in front of it
// and starts a line -- so that its block inflates alone.  A template parameter: the kernel is register-critical.
template <bool kBgzf>
__global__ void __launch_bounds__(256) deflate_chunks(DeflateArgs a) {
  if (a.gate && *a.gate != ~0ull) return;
  __shared__ uint32_t obuf[kOutWords];
  __shared__ uint32_t freq[288], dfreq[32];
  __shared__ uint32_t ctab[288], dtab[32];  // literal/length and distance codes: code | len << 16
  __shared__ uint32_t crc_tab[256];
  __shared__ uint8_t clen[288], dlen[32];
  __shared__ uint32_t cl_freq[19], cl_tab[19];
  __shared__ uint8_t cl_len[19];
  // the chunk's line index is done with when the code construction starts: they share their LDS
  __shared__ union {
    HuffScratch scratch;
    uint16_t nl_pos[kMaxLines];  // chunk positions of the chunk's first line ends (find_matches)
  } u;
  __shared__ uint32_t sh[8];
  __shared__ uint32_t s_header_bits, s_stored;
  const uint32_t tid = threadIdx.x;
  // which chunk of which route stream is this block's?
  constexpr uint32_t kNone = 0xffffffffu;
  uint32_t b = blockIdx.x, route = kNone;
  unsigned long long base = 0, rbytes = 0;
  for (uint32_t r = 0; r < a.n_routes; ++r) {
    const unsigned long long bytes = a.route_bytes[r * 2];
    const uint32_t nch = (uint32_t)((bytes + kChunk - 1) / kChunk);
    if (route == kNone && b < nch) {
      route = r;
      rbytes = bytes;
    }
    if (route == kNone) {
      b -= nch;
      base += bytes;
    }
  }
  if (route == kNone) return;  // beyond the last chunk
  const bool fasta = (a.fasta_classes >> min(route, 3u)) & 1u;
  const uint32_t marker = fasta ? '>' : '@', lines = fasta ? 2u : 4u;
  const uint32_t raw_len = (uint32_t)min((unsigned long long)kChunk, rbytes - (unsigned long long)b * kChunk);
  const uint8_t *stream = a.text + base;  // the route's stream: matches may reach back into the chunk in front
  const long long chunk0 = (long long)b * kChunk;
  const uint8_t *src = stream + chunk0;
  uint8_t *dst = a.stage + (size_t)blockIdx.x * kSlot;

  for (uint32_t i = tid; i < kOutWords; i += 256) obuf[i] = 0;
  for (uint32_t i = tid; i < 288; i += 256) freq[i] = 0;
  if (tid < 32) dfreq[tid] = 0;
  {  // byte-wise CRC table
    uint32_t c = tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
    crc_tab[tid] = c;
  }
  __syncthreads();
  // this thread's slice, in registers: 32 dwords cut out of the (arbitrarily aligned) stream with funnel shifts, and
  // the byte in front of it
  const uint32_t lo = tid * kSlice, hi = min(lo + kSlice, raw_len);
  const uint32_t n_valid = hi > lo ? hi - lo : 0u;
  uint32_t w[32];
  uint32_t prev_byte = 0x100u;  // (no byte in front: the stream starts here)
  {
    const uint8_t *at = src + lo;
    const uint32_t *al = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(at) & ~(uintptr_t)3);
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(at) & 3u);
    const uint32_t words = n_valid ? (n_valid + shift + 3u) / 4u : 0u;  // aligned dwords that hold the slice
    uint32_t raw[33];
#pragma unroll
    for (int d = 0; d < 33; ++d) raw[d] = (uint32_t)d < words ? al[d] : 0u;
#pragma unroll
    for (int d = 0; d < 32; ++d) w[d] = __builtin_amdgcn_alignbyte(raw[d + 1], raw[d], shift);
    if (n_valid && (kBgzf ? (long long)lo : chunk0 + lo) > 0) prev_byte = src[(long long)lo - 1];
  }
  // CRC-32 of the slice, moved to the chunk's front by the bytes behind it (see crc_step)
  uint32_t crc_moved = 0;
  if (n_valid) {
    uint32_t c4[4] = {0xffffffffu, 0u, 0u, 0u};  // (the pre-set ones belong to the message's first bytes only)
#pragma unroll
    for (int d = 0; d < 8; ++d) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t p = (uint32_t)(32 * q + 4 * d + k);
          if (p < n_valid) c4[q] = crc_step(crc_tab, c4[q], (w[8 * q + d] >> (8 * k)) & 0xffu);
        }
      }
    }
    // quarter q is followed by `rest` bytes of the slice: its register moves by x^(8 rest)
    uint32_t crc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t end_q = min((uint32_t)(32 * q + 32), n_valid);
      if ((uint32_t)(32 * q) < n_valid) {
        const uint32_t rest = n_valid - end_q;
        crc ^= rest ? multmodp(x2nmodp(rest, 3), c4[q]) : c4[q];
      }
    }
    crc = ~crc;
    const uint32_t after = raw_len - hi;
    const uint32_t mul = (after % kSlice == 0 && after / kSlice < 256u) ? c_shift128[after / kSlice] : x2nmodp(after, 3);
    crc_moved = multmodp(mul, crc);
  }
  const bool lz = a.literal_only == 0;
  uint32_t *my_matches = reinterpret_cast<uint32_t *>(dst) + tid * 32u;  // (the slot is 4-byte aligned, 32 KB + 64)
  uint32_t n_matches = 0;
  Mask128 covered = {0, 0};
  if (lz) {
    // (block-uniform branch: the line index needs every thread at its barriers)
    const SliceMasks m = slice_masks(w, prev_byte == 0x100u ? (~w[0] & 0xffu) : prev_byte, n_valid, marker);
    uint32_t all_lines;
    const uint32_t lines_before = cstext::block_scan_256((uint32_t)__popcll(m.nl.lo) + (uint32_t)__popcll(m.nl.hi), all_lines, sh);
    {
      uint32_t at = lines_before;
      for (uint32_t i = m128_next_set(m.nl, 0u); i < 128u && at < kMaxLines; i = m128_next_set(m.nl, i + 1u)) u.nl_pos[at++] = (uint16_t)(lo + i);
    }
    __syncthreads();
    const bool chunk_starts_line = kBgzf || chunk0 == 0 || src[-1] == '\n';
    if (n_valid)
      find_matches(src, lo, n_valid, m, prev_byte == 0x100u || prev_byte == '\n', lines_before, u.nl_pos, lines, chunk_starts_line,
                   [&](uint32_t at, uint32_t len, uint32_t dist) {
                     my_matches[n_matches++] = at | ((len - 3u) << 7) | ((dist - 1u) << 15);
                     const Mask128 r = m128_range(at, len);
                     covered.lo |= r.lo;
                     covered.hi |= r.hi;
                   });
  }
  if (n_valid)
    walk_tokens(w, n_valid, covered, my_matches, n_matches, [&](uint32_t byte) { atomicAdd(&freq[byte], 1u); },
                [&](uint32_t len, uint32_t dist) {
                  uint32_t nb, ex;
                  atomicAdd(&freq[length_symbol(len, nb, ex)], 1u);
                  atomicAdd(&dfreq[distance_symbol(dist, nb, ex)], 1u);
                });
  if (tid == 0) {
    atomicAdd(&freq[256], 1u);  // end of block
    atomicAdd(&dfreq[0], 1u);   // (a block without a match still names one distance code: one bit, never used)
  }
  // CRC of the chunk: the XOR of the moved slices
  {
    uint32_t v = crc_moved;
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
    __syncthreads();  // (freq complete as well, and nobody reads the line index any more)
    if ((tid & 63u) == 0) sh[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) a.info[blockIdx.x].crc = sh[0] ^ sh[1] ^ sh[2] ^ sh[3];
  }
  // literal/length code, distance code, then the code of the code lengths (no run-length symbols: plain lengths) --
  // the whole block builds each of them (huff_build)
  huff_build(freq, 286, 15, clen, ctab, u.scratch, sh);
  huff_build(dfreq, 30, 15, dlen, dtab, u.scratch, sh);
  if (tid < 19) cl_freq[tid] = 0;
  __syncthreads();
  atomicAdd(&cl_freq[clen[tid]], 1u);
  if (tid < 30u) atomicAdd(&cl_freq[clen[256u + tid]], 1u);
  if (tid < 30u) atomicAdd(&cl_freq[dlen[tid]], 1u);
  __syncthreads();
  huff_build(cl_freq, 19, 7, cl_len, cl_tab, u.scratch, sh);
  if (tid == 0) {
    // block header: BFINAL 0, BTYPE 10, HLIT 29 (286 codes), HDIST 29 (30 codes), HCLEN 15 (all 19 lengths)
    uint32_t pos = 0;
    put_bits(obuf, pos, 0u, 1);
    put_bits(obuf, pos, 2u, 2);
    put_bits(obuf, pos, 29u, 5);
    put_bits(obuf, pos, 29u, 5);
    put_bits(obuf, pos, 15u, 4);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) put_bits(obuf, pos, cl_len[order[i]], 3);
    s_header_bits = pos;  // (the 316 code lengths follow, every thread its own: below)
  }
  __syncthreads();
  // the code lengths of the 286 + 30 symbols in the code of the code lengths: thread t writes symbol t (and 256 + t)
  {
    const uint32_t e0 = cl_tab[clen[tid]];
    const uint32_t s1 = 256u + tid;
    const uint32_t e1 = s1 < 286u ? cl_tab[clen[s1]] : (s1 < 316u ? cl_tab[dlen[s1 - 286u]] : 0u);
    uint32_t tot0, tot1;
    const uint32_t before0 = cstext::block_scan_256(e0 >> 16, tot0, sh);
    const uint32_t before1 = cstext::block_scan_256(e1 >> 16, tot1, sh);
    uint32_t p0 = s_header_bits + before0, p1 = s_header_bits + tot0 + before1;
    put_bits(obuf, p0, e0 & 0xffffu, e0 >> 16);
    if (e1 >> 16) put_bits(obuf, p1, e1 & 0xffffu, e1 >> 16);
    __syncthreads();
    if (tid == 0) s_header_bits += tot0 + tot1;
    __syncthreads();
  }
  // bits of this thread's tokens, then where they go
  uint32_t my_bits = 0;
  if (n_valid)
    walk_tokens(w, n_valid, covered, my_matches, n_matches, [&](uint32_t byte) { my_bits += ctab[byte] >> 16; },
                [&](uint32_t len, uint32_t dist) {
                  uint32_t nb, ex, nb2;
                  my_bits += ctab[length_symbol(len, nb, ex)] >> 16;
                  my_bits += dtab[distance_symbol(dist, nb2, ex)] >> 16;
                  my_bits += nb + nb2;
                });
  uint32_t total_bits;
  uint32_t pos = s_header_bits + cstext::block_scan_256(my_bits, total_bits, sh);
  const uint32_t eob_bits = ctab[256] >> 16;
  // header + data + end of block + empty stored block (3 bits, pad, LEN, NLEN)
  const uint32_t all_bits = s_header_bits + total_bits + eob_bits;
  const uint32_t comp_bytes = (all_bits + 3u + 7u) / 8u + 4u;
  if (tid == 0) s_stored = (comp_bytes >= raw_len + 5u || comp_bytes > kOutWords * 4u - 8u) ? 1u : 0u;
  __syncthreads();
  if (s_stored) {
    // stored block: 0 0 0 (BFINAL, BTYPE 00), pad, LEN, NLEN, raw bytes -- byte-aligned by construction
    // (every thread is past its match list: the scan above had barriers behind the last read of it)
    if (tid == 0) {
      dst[0] = 0;
      dst[1] = (uint8_t)(raw_len & 0xffu);
      dst[2] = (uint8_t)(raw_len >> 8);
      dst[3] = (uint8_t)(~raw_len & 0xffu);
      dst[4] = (uint8_t)((~raw_len >> 8) & 0xffu);
      ChunkInfo &ci = a.info[blockIdx.x];
      ci.comp_len = raw_len + 5u;
      ci.raw_len = raw_len;
      ci.route = route;
    }
    for (uint32_t i = tid; i < raw_len; i += 256) dst[5 + i] = src[i];
    return;
  }
  if (n_valid)
    walk_tokens(w, n_valid, covered, my_matches, n_matches,
                [&](uint32_t byte) {
                  const uint32_t e = ctab[byte];
                  put_bits(obuf, pos, e & 0xffffu, e >> 16);
                },
                [&](uint32_t len, uint32_t dist) {
                  uint32_t nb, ex;
                  const uint32_t e = ctab[length_symbol(len, nb, ex)];
                  put_bits(obuf, pos, e & 0xffffu, e >> 16);
                  if (nb) put_bits(obuf, pos, ex, nb);
                  const uint32_t f = dtab[distance_symbol(dist, nb, ex)];
                  put_bits(obuf, pos, f & 0xffffu, f >> 16);
                  if (nb) put_bits(obuf, pos, ex, nb);
                });
  __syncthreads();
  if (tid == 0) {
    uint32_t p = s_header_bits + total_bits;
    put_bits(obuf, p, ctab[256] & 0xffffu, eob_bits);
    put_bits(obuf, p, 0u, 3);      // empty stored block, not final
    p = (p + 7u) & ~7u;            // to the byte boundary
    put_bits(obuf, p, 0u, 16);     // LEN 0
    put_bits(obuf, p, 0xffffu, 16);  // NLEN
    ChunkInfo &ci = a.info[blockIdx.x];
    ci.comp_len = p / 8u;
    ci.raw_len = raw_len;
    ci.route = route;
  }
  __syncthreads();
  uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst);  // (slots are 4-byte aligned)
  for (uint32_t i = tid; i < (comp_bytes + 3u) / 4u; i += 256) dst32[i] = obuf[i];
}

struct LayoutArgs {
  const ChunkInfo *info;
  const unsigned long long *route_bytes;  // [route * 2]: raw bytes of the stream
  uint32_t n_routes;
  uint32_t *chunk_dst;                    // per chunk: byte offset inside the mate's gzip buffer
  uint8_t *gz;                            // the mate's gzip buffer
  unsigned long long *gz_route_bytes;     // out [route * 2]: bytes of the route's gzip member (0: nothing to write)
  unsigned long long *gz_total;           // out: sum
  const unsigned long long *gate;
};

// One block: members laid out back to back; per member 10-byte header, the chunks, final empty block, CRC-32, ISIZE.
// Every thread takes a RUN of consecutive chunks of the route (round 5; round 4 dealt the chunks out one per thread and
// round, and every chunk paid x^(8 * bytes behind it) by square-and-multiply over 26 bits -- fourteen polynomial
// products per chunk, 0.31 ms per mate and batch on ONE compute unit).  A chunk's place is the prefix sum of the
// compressed lengths in front of it: serial inside the run, one block scan over the runs.  The member's CRC: crc32_combine
// is linear over GF(2), crc(A B C) = crc(A) x^(8 |B C|) + crc(B) x^(8 |C|) + crc(C) (mod p); all chunks but the last are
// 32 KB, so with Q = x^(8 * 32768) a run is Horner's rule in Q (one product per chunk), moved to its place by
// Q^(full chunks behind the run) (square-and-multiply over 12 bits) and by x^(8 * length of the last chunk).
__global__ void __launch_bounds__(256) deflate_layout(LayoutArgs a) {
  if (a.gate && *a.gate != ~0ull) return;
  __shared__ uint32_t s_crc[4];
  __shared__ uint32_t sh[8];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t Q = c_x2n[18];  // x^(2^18) = x^(8 * 32768)
  static_assert(kChunk == 32768, "Q");
  unsigned long long at = 0;  // (block-uniform)
  uint32_t first = 0;
  for (uint32_t r = 0; r < a.n_routes; ++r) {
    const unsigned long long raw = a.route_bytes[r * 2];
    const uint32_t nch = (uint32_t)((raw + kChunk - 1) / kChunk);
    if (raw == 0) {
      if (tid == 0) a.gz_route_bytes[r * 2] = 0;
      continue;
    }
    const unsigned long long start = at;
    const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    if (tid < 10) a.gz[at + tid] = head[tid];
    at += 10;
    const uint32_t run = (nch + 255u) / 256u;
    const uint32_t c0 = min(tid * run, nch), c1 = min(c0 + run, nch);
    const uint32_t full_end = min(c1, nch - 1u);  // chunks [c0, full_end) of the run are full ones followed by more
    uint32_t run_bytes = 0, acc = 0, crc_part = 0;
    for (uint32_t c = c0; c < c1; ++c) {
      const ChunkInfo ci = a.info[first + c];
      run_bytes += ci.comp_len;
      if (c < full_end)
        acc = (c > c0 ? multmodp(Q, acc) : 0u) ^ ci.crc;  // sum of crc_c * Q^(full_end - 1 - c)
      else
        crc_part ^= ci.crc;  // the route's last chunk: nothing behind it
    }
    if (full_end > c0) {
      // behind chunk full_end - 1: (nch - 1 - full_end) full chunks and the last one
      const uint32_t last_len = (uint32_t)(raw - (unsigned long long)(nch - 1u) * kChunk);
      uint32_t mul = x2nmodp(last_len, 3);
      const uint32_t fulls = nch - 1u - full_end;
      if (fulls) mul = multmodp(x2nmodp(fulls, 18), mul);
      crc_part ^= multmodp(mul, acc);
    }
    uint32_t total;
    const uint32_t before = cstext::block_scan_256(run_bytes, total, sh);
    {
      unsigned long long pos = at + before;
      for (uint32_t c = c0; c < c1; ++c) {
        a.chunk_dst[first + c] = (uint32_t)pos;
        pos += a.info[first + c].comp_len;
      }
    }
    at += total;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) crc_part ^= (uint32_t)__shfl_xor((int)crc_part, d, 64);
    if (lane == 0u) s_crc[wv] = crc_part;
    __syncthreads();
    const uint32_t crc = s_crc[0] ^ s_crc[1] ^ s_crc[2] ^ s_crc[3];
    if (tid == 0) {
      unsigned long long w = at;
      a.gz[w++] = 0x03;  // final block: fixed Huffman, end of block
      a.gz[w++] = 0x00;
      for (int i = 0; i < 4; ++i) a.gz[w++] = (uint8_t)(crc >> (8 * i));
      for (int i = 0; i < 4; ++i) a.gz[w++] = (uint8_t)((raw & 0xffffffffull) >> (8 * i));
    }
    at += 10;
    if (tid == 0) a.gz_route_bytes[r * 2] = at - start;
    first += nch;
    __syncthreads();  // s_crc is written again for the next route
  }
  if (tid == 0) *a.gz_total = at;
}

struct CompactArgs {
  const ChunkInfo *info;
  const uint32_t *chunk_dst;
  const uint8_t *stage;
  uint8_t *gz;
  const unsigned long long *route_bytes;
  uint32_t n_routes;
  const unsigned long long *gate;
};

__global__ void __launch_bounds__(256) deflate_compact(CompactArgs a) {
  if (a.gate && *a.gate != ~0ull) return;
  uint32_t total = 0;
  for (uint32_t r = 0; r < a.n_routes; ++r) total += (uint32_t)((a.route_bytes[r * 2] + kChunk - 1) / kChunk);
  if (blockIdx.x >= total) return;
  const uint32_t n = a.info[blockIdx.x].comp_len;
  const uint8_t *src = a.stage + (size_t)blockIdx.x * kSlot;
  uint8_t *dst = a.gz + a.chunk_dst[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

// ---- BGZF (cs_text_params.compress = 2): every chunk is a gzip member of its own, a BGZF block (SAM specification 4.1):
// 18 header bytes -- FEXTRA with the subfield 'B' 'C', whose value BSIZE is the block's size less one --, the chunk as
// deflate_chunks<true> staged it, the final empty fixed block, the CHUNK's CRC-32 and length.  Nothing is combined and no
// route is walked serially: a chunk's place is the sum of comp_len + kBgzfWrap over the chunks in front of it, routes
// back to back, and the block that copies a chunk finds that sum itself (a few thousand chunks a batch at most: a dozen
// loads a thread), writes the header and the trailer around the copy, and the route's and the mate's sizes where its
// chunk is the route's or the mate's last.  The EOF marker is the file's, not the stream's: the host appends it.
constexpr uint32_t kBgzfHead = 18, kBgzfTail = 10, kBgzfWrap = kBgzfHead + kBgzfTail;
static_assert(kBgzfWrap + kChunk + 5u <= 65536u, "BSIZE: a stored chunk's block has to fit 16 bits");
static_assert(kBgzfWrap + kChunk + 5u <= kSlot, "a block takes no more of the gz buffer than its chunk's staging slot");
static_assert(kOutWords * 4u <= kChunk + 5u, "a dynamic chunk is no larger than a stored one");

struct BgzfArgs {
  const ChunkInfo *info;
  const uint8_t *stage;
  const unsigned long long *route_bytes;  // [route * 2]: raw bytes of the stream
  uint32_t n_routes;
  uint32_t *chunk_dst;                    // per chunk: byte offset of its block inside the mate's gzip buffer
  uint8_t *gz;
  unsigned long long *gz_route_bytes;     // out [route * 2]: bytes of the route's blocks (0: nothing to write)
  unsigned long long *gz_total;           // out: sum
  const unsigned long long *gate;
};

__global__ void __launch_bounds__(256) bgzf_layout(BgzfArgs a) {
  if (a.gate && *a.gate != ~0ull) return;
  __shared__ uint32_t s_sum[2][4];
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  // this block's chunk: its route's first chunk and chunk count, and the chunks of the mate
  constexpr uint32_t kNone = 0xffffffffu;
  uint32_t total = 0, first = kNone, nch_route = 0, route = 0;
  for (uint32_t r = 0; r < a.n_routes; ++r) {
    const uint32_t nch = (uint32_t)((a.route_bytes[r * 2] + kChunk - 1) / kChunk);
    if (first == kNone && c < total + nch) {
      first = total;
      nch_route = nch;
      route = r;
    }
    if (c == 0 && tid == 0 && nch == 0) a.gz_route_bytes[r * 2] = 0;
    total += nch;
  }
  if (c == 0 && tid == 0 && total == 0) *a.gz_total = 0;
  if (first == kNone) return;  // beyond the last chunk (block-uniform)
  // bytes in front of the route and, from there, in front of the chunk
  uint32_t before_route = 0, in_route = 0;
  for (uint32_t j = tid; j < c; j += 256) {
    const uint32_t n = a.info[j].comp_len + kBgzfWrap;
    if (j < first) before_route += n; else in_route += n;
  }
  for (int o = 32; o > 0; o >>= 1) {
    before_route += __shfl_xor(before_route, o, 64);
    in_route += __shfl_xor(in_route, o, 64);
  }
  if ((tid & 63u) == 0) {
    s_sum[0][tid >> 6] = before_route;
    s_sum[1][tid >> 6] = in_route;
  }
  __syncthreads();
  before_route = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
  in_route = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
  const ChunkInfo ci = a.info[c];
  const uint32_t at = before_route + in_route, size = ci.comp_len + kBgzfWrap;
  uint8_t *dst = a.gz + at;
  if (tid < kBgzfHead) {
    // 1f 8b 08 04 (FEXTRA), MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C', SLEN 2, BSIZE
    const unsigned long long h0 = 0x0000000004088b1full, h1 = 0x000243420006ff00ull;
    dst[tid] = (uint8_t)(tid < 8u ? h0 >> (8u * tid) : tid < 16u ? h1 >> (8u * (tid - 8u)) : (size - 1u) >> (8u * (tid - 16u)));
  } else if (tid >= 32u && tid < 32u + kBgzfTail) {
    // 03 00 (final block, fixed Huffman, end of block), the chunk's CRC-32, its length
    const uint32_t k = tid - 32u;
    dst[kBgzfHead + ci.comp_len + k] = (uint8_t)(k < 2u ? 0x0003u >> (8u * k) : k < 6u ? ci.crc >> (8u * (k - 2u)) : ci.raw_len >> (8u * (k - 6u)));
  }
  const uint8_t *src = a.stage + (size_t)c * kSlot;
  for (uint32_t i = tid; i < ci.comp_len; i += 256) dst[kBgzfHead + i] = src[i];
  if (tid == 0) {
    a.chunk_dst[c] = at;
    if (c + 1u == first + nch_route) a.gz_route_bytes[route * 2] = (unsigned long long)in_route + size;
    if (c + 1u == total) *a.gz_total = (unsigned long long)at + size;
  }
}

}  // namespace csdefl
