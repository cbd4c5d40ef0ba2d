// text_kernels.hip.inc -- FASTQ text in, finished FASTQ text out, on the device (device code only).
// Included by cutseq_hip.hip.  gfx950 / wave64 only.
//
// The host side of the reference's hot path is dnaio's record parser and writer as cutadapt drives them
// (cutseq/run.py:434-441, 751-758, 785-794).  With the trimming kernels at billions of reads per second that
// string work IS the end-to-end bottleneck, so the text path moves it here: the host uploads raw, record-aligned
// FASTQ text (what the inflate threads produce) and downloads finished output text (what the deflate / write
// threads consume).  HBM-bound byte work, nothing else:
//
//   text_count_nl / text_scan_blocks / text_write_nl   positions of every '\n' (two passes over the text: counts per
//                                                      16 KB segment, exclusive scan, positions)
//   text_parse_records    one lane per record: the four lines' extents, '@' / '+' / equal-length checks, read
//                         length, SuffixRemover literals, Renamer's id field (name.split(maxsplit=1)[0])
//   text_restride         sequence and quality lines -> the [n][stride] rows the trimming kernels take (one lane per
//                         destination dword: two aligned source dwords, one funnel shift)
//   (scan + resolve kernels: trim_kernel.hip.inc, unchanged)
//   format_sizes / format_scan / format_offsets   route of every record (TooShort -> TooLong -> TooManyN ->
//                         TooManyExpectedErrors -> IsUntrimmedAny -> sink, pair filter "any"; the three in the middle
//                         discard the pair: no route, no bytes) and the byte offset of its output record inside the route's stream: block
//                         sums, exclusive scan, block-local scans -- output order = input order.  <3>: the three routes;
//                         <4>: cs_text_params.too_long_route, the pairs TooLong catches are a fourth route, not discarded
//   format_copy           32 lanes per output record: '@' id ['_' UMI] '\n' seq[start:stop] "\n+\n" qual[start:stop] '\n'
//   text_parse_records_woven / format_sizes_woven / format_offsets_woven   cutadapt's --interleaved (cs_text_create_interleaved):
//                         both mates' records in ONE text, alternating, and / or ONE output stream per route, the
//                         record of one mate followed by its partner's.  Kernels of their own: a cs_text without the
//                         bits launches what it launched before
//   name_len / emit_name  cutadapt's --rename (cs_text_set_rename): the record name from a template's segments.  The
//                         format kernels (and the info table's) take the RenameTable as one more argument; without it
//                         they are the kernels they were, instantiations of their own with it
//
// Everything a kernel rejects (malformed record, read longer than the row stride, mate ids that differ) lands in
// TextMeta.err as the smallest (record index, code) key; the host raises what the reference's reader would.

namespace cstext {

constexpr uint32_t kSeg = 16384;       // text bytes per block of the newline passes
constexpr uint32_t kSegThreads = 256;  // 64 bytes per thread
constexpr uint32_t kSuffixMax = 8;

enum { ERR_NONE = 0, ERR_MALFORMED = 1, ERR_TOO_LONG = 2, ERR_IDS_DIFFER = 3, ERR_LINE_COUNT = 4 };

struct Rec {           // one input record of one mate (16 bytes)
  uint32_t seq_off;    // byte offset of the sequence line
  uint32_t qual_off;   // ... of the quality line
  uint32_t hdr_off;    // ... of the header behind '@'
  uint16_t hdr_len;    // header bytes after the SuffixRemover chain (line end stripped)
  uint16_t len;        // read length
};

struct TextMeta {                    // what the host reads back per batch (one 128-byte block)
  unsigned long long err;            // smallest (record << 8 | code) over everything that went wrong; ~0 = fine
  unsigned long long out_bytes[2];   // per mate: bytes of the three route streams, back to back
  unsigned long long route_bytes[3][2];
  uint32_t route_count[3];
  uint32_t n_lines[2];
  uint32_t max_len;                  // longest read seen (the host grows the row stride when it exceeds it)
  uint32_t no_index;                 // bit m: mate m's text has the wrong line count, its newline index was not written
  // pairs the discarding filters took, each under the FIRST of TooLong -> TooManyN -> TooManyExpectedErrors that
  // caught it (cs_plan_set_max_length / _max_n / _max_ee); n_too_many_ee fills what was padding
  uint32_t n_too_many_n, n_too_long, n_too_many_ee;
  alignas(8) unsigned long long written_bp[2];  // bases of the records that reach the final sink (route 0), per mate
  uint32_t n_long[2];                // per mate: reads longer than the rows (long_kernel.hip.inc walks their chains)
  unsigned long long gz_route_bytes[3][2];  // compressed output (deflate_kernels.hip.inc): bytes of each gzip member
  unsigned long long gz_bytes[2];           // ... per mate
};
static_assert(offsetof(TextMeta, written_bp) == 112 && sizeof(TextMeta) == 200, "TextMeta layout");

constexpr uint32_t kMaxRoutes = 3 + 255;  // trimmed / short / untrimmed + one route per barcode of a demultiplexing plan
constexpr uint32_t kRouteDiscard = 0x1feu;  // a discarding filter: the pair goes nowhere (below the 0x1ff of the lanes past the end)
constexpr uint32_t kDiscarded = ~0u;        // FormatArgs.dst of a discarded record (no output offset is ever that)

struct TextParams {  // constant per engine
  uint8_t paired, has_umi, untrimmed_filter, reverse_complement;
  uint8_t flag_too_short, flag_untrimmed;
  uint16_t n_bins;  // demultiplexing plans: the trimmed records of barcode b go to route 3 + b (route 0 stays empty)
  uint8_t suffix[2][2][kSuffixMax];  // [mate][which]: SuffixRemover literals, applied in order
  uint8_t suffix_len[2][2];
  uint8_t demux_mate;                // n_bins > 0: the mate (0 / 1) whose chain holds the demultiplexing op
  uint8_t fasta_routes;              // bit 2 * class + mate: that stream's records are ">id\nseq\n" (class = route, 3 for
                                     // every barcode's route).  cs_text_create folds cs_text_params.fasta_out into it
  uint8_t filters;                   // the plan has some of TooLong / TooManyN / TooManyExpectedErrors (CS_X_* bits):
                                     // FormatArgs.xf holds the per-read flags
  uint8_t too_long_route;            // cs_text_params.too_long_route: a pair TooLong catches forms route 3 (no bins then)
};

__device__ __forceinline__ void report(TextMeta *meta, uint32_t record, uint32_t code) {
  atomicMin(&meta->err, ((unsigned long long)record << 8) | code);
}

// flags of the bytes equal to '\n' in a dword: bit 7 of each such byte
__device__ __forceinline__ uint32_t nl_flags(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;  // exact zero-byte test
}

// exclusive scan over the 256 threads of a block (4 waves); total in every thread
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t &total, uint32_t *sh /* >= 8 dwords */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();  // sh may still be read by the previous call
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s = sh[w];
    if (w < wave) before += s;
    all += s;
  }
  total = all;
  return before + inc - v;
}

// ---- newline index -----------------------------------------------------------------------------------------
// text is padded to a multiple of 16 bytes in its allocation (bytes beyond `bytes` are ignored)

__device__ __forceinline__ uint32_t count_thread_nl(const uint8_t *text, uint32_t bytes, uint32_t off, uint4 w[4]) {
  uint32_t c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t o = off + 16u * q;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o < bytes) v = *reinterpret_cast<const uint4 *>(text + o);
    // bytes at or beyond `bytes` do not count
    uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t p = o + 4u * k;
      if (p + 4 > bytes) {
        const uint32_t keep = p >= bytes ? 0u : (0xffffffffu >> (8u * (p + 4 - bytes)));
        d[k] = (d[k] & keep) | (~keep & 0x20202020u);  // pad with spaces
      }
    }
    w[q] = make_uint4(d[0], d[1], d[2], d[3]);
    c += __popc(nl_flags(d[0])) + __popc(nl_flags(d[1])) + __popc(nl_flags(d[2])) + __popc(nl_flags(d[3]));
  }
  return c;
}

__global__ void __launch_bounds__(kSegThreads) text_count_nl(const uint8_t *text, uint32_t bytes, uint32_t *blk_cnt) {
  __shared__ uint32_t sh[8];
  uint4 w[4];
  const uint32_t off = blockIdx.x * kSeg + threadIdx.x * 64u;
  const uint32_t c = count_thread_nl(text, bytes, off, w);
  uint32_t total;
  (void)block_scan_256(c, total, sh);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// exclusive scan of `cols` interleaved columns over `n` rows, in place; totals[c] receives the column sums
__global__ void __launch_bounds__(1024) text_scan_blocks(uint32_t *v, uint32_t n, uint32_t cols, unsigned long long *totals) {
  __shared__ unsigned long long sh[16];
  __shared__ unsigned long long carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t c = blockIdx.x; c < cols; c += gridDim.x) {  // (one block: every column; more: columns dealt out)
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
      const uint32_t i = base + threadIdx.x;
      const unsigned long long x = i < n ? v[(size_t)i * cols + c] : 0;
      unsigned long long inc = x;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) sh[wave] = inc;
      __syncthreads();
      unsigned long long before = carry_s, all = 0;
      for (int w = 0; w < 16; ++w) {
        if (w < wave) before += sh[w];
        all += sh[w];
      }
      // offsets inside one batch stay below 2^32 (cs_text_create checks the capacities)
      if (i < n) v[(size_t)i * cols + c] = (uint32_t)(before + inc - x);
      __syncthreads();
      if (threadIdx.x == 0) carry_s += all;
      __syncthreads();
    }
    if (threadIdx.x == 0) totals[c] = carry_s;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kSegThreads) text_write_nl(const uint8_t *text, uint32_t bytes, const uint32_t *blk_base,
                                                             const unsigned long long *total_lines, uint32_t expect_lines,
                                                             uint32_t *nl, TextMeta *meta, int mate) {
  __shared__ uint32_t sh[8];
  uint4 w[4];
  const uint32_t off = blockIdx.x * kSeg + threadIdx.x * 64u;
  const uint32_t c = count_thread_nl(text, bytes, off, w);
  uint32_t total;
  uint32_t at = blk_base[blockIdx.x] + block_scan_256(c, total, sh);
  // a text whose last line lacks its '\n' is one newline short: the end of the text stands in for it
  const uint32_t lines = (uint32_t)*total_lines;
  const bool ok = lines == expect_lines || (lines + 1 == expect_lines && bytes > 0 && text[bytes - 1] != '\n');
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    meta->n_lines[mate] = lines;
    if (!ok) {
      report(meta, 0, ERR_LINE_COUNT);
      atomicOr(&meta->no_index, 1u << mate);
    }
    if (ok && lines + 1 == expect_lines) nl[expect_lines - 1] = bytes;
  }
  if (!ok) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t d[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t f = nl_flags(d[k]);
      while (f) {
        const uint32_t b = (uint32_t)__builtin_ctz(f) >> 3;
        f &= f - 1u;
        nl[at++] = off + 16u * q + 4u * k + b;
      }
    }
  }
}

// ---- records ---------------------------------------------------------------------------------------------------

// str.split()'s white space on 7-bit input (the reference splits a str, not bytes): " \t\n\v\f\r" and \x1c .. \x1f
__device__ __forceinline__ bool is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

constexpr uint32_t kNotLong = 0xffffffffu;

__global__ void __launch_bounds__(256) text_parse_records(const uint8_t *text, const uint32_t *nl, uint32_t n, uint32_t stride,
                                                          TextParams tp, int mate, Rec *rec, uint32_t *idr, uint16_t *len,
                                                          cslong::LongRec *lrec, uint32_t *long_of, TextMeta *meta) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  // No index to go by (text_write_nl): recorded per mate, NOT read off the low byte of meta->err -- that is the
  // smallest (record, code) key over both mates, and another error on record 0 replaces the line-count key.  The
  // records are written as empty ones, so that text_restride never follows offsets nobody computed.
  if (meta->no_index & (1u << mate)) {
    const Rec none = {0, 0, 0, 0, 0};
    rec[r] = none;
    idr[r] = 0;
    len[r] = 0;
    long_of[r] = kNotLong;
    return;
  }
  uint32_t start[4], end[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const uint32_t line = 4u * r + (uint32_t)l;
    start[l] = line == 0 ? 0u : nl[line - 1] + 1u;
    end[l] = nl[line];
    if (end[l] > start[l] && text[end[l] - 1] == '\r') --end[l];
  }
  Rec out = {0, 0, 0, 0, 0};
  bool bad = end[0] <= start[0] || text[start[0]] != '@' || end[2] <= start[2] || text[start[2]] != '+';
  const uint32_t sl = end[1] - start[1], ql = end[3] - start[3];
  bad = bad || sl != ql || end[0] - start[0] - 1u > 65535u;
  uint32_t long_slot = kNotLong;
  if (bad) {
    report(meta, r, ERR_MALFORMED);
  } else {
    atomicMax(&meta->max_len, sl);
    if (sl > CS_MAX_READ) report(meta, r, ERR_TOO_LONG);
    if (sl > stride || sl >= (uint32_t)CS_LEN_SKIP) {
      // does not fit the rows: out of the tile kernels' way (CS_LEN_SKIP), onto the list of the long-read kernel
      long_slot = atomicAdd(&meta->n_long[mate], 1u);  // (at most n of them: the list has n entries)
      cslong::LongRec lr;
      lr.rec = r;
      lr.seq_off = start[1];
      lr.qual_off = start[3];
      lr.len = sl;
      lrec[long_slot] = lr;
    }
    out.seq_off = start[1];
    out.qual_off = start[3];
    out.hdr_off = start[0] + 1u;
    uint32_t hl = end[0] - start[0] - 1u;
    const uint8_t *name = text + out.hdr_off;
    // SuffixRemover chain (cutseq/run.py:330, 537-542): literals removed from the END of the whole header, in order
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint32_t k = tp.suffix_len[mate][s];
      if (k && hl >= k) {
        bool same = true;
        for (uint32_t i = 0; i < k; ++i) same = same && name[hl - k + i] == tp.suffix[mate][s][i];
        if (same) hl -= k;
      }
    }
    out.hdr_len = (uint16_t)hl;
    out.len = long_slot == kNotLong ? (uint16_t)sl : (uint16_t)0;  // (a long read leaves an empty row)
    // Renamer.parse_name: the first of two whitespace-separated fields, else the whole name
    uint32_t a = 0;
    while (a < hl && is_space(name[a])) ++a;
    uint32_t b = a;
    while (b < hl && !is_space(name[b])) ++b;
    uint32_t c = b;
    while (c < hl && is_space(name[c])) ++c;
    idr[r] = (b > a && c < hl) ? (a | ((b - a) << 16)) : (hl << 16);
  }
  rec[r] = out;
  len[r] = long_slot == kNotLong ? out.len : (uint16_t)CS_LEN_SKIP;
  long_of[r] = long_slot;
}

// The same for an interleaved text (cs_text_create_interleaved, CS_INTERLEAVE_IN): the one text holds both mates'
// records, alternating, under one newline index -- record r of mate `mate` stands at lines 4 * (2r + mate) .. + 3.  One
// launch per mate, like text_parse_records; everything else is that kernel's, line for line.  A kernel of its own and
// not a shared body: text_parse_records has to stay the code it was (profiles/interleaved_ab.log), and it does not when
// its body moves into a function the two are inlined from (two more SGPRs, another block order).
__global__ void __launch_bounds__(256) text_parse_records_woven(const uint8_t *text, const uint32_t *nl, uint32_t n,
                                                                uint32_t stride, TextParams tp, int mate, Rec *rec,
                                                                uint32_t *idr, uint16_t *len, cslong::LongRec *lrec,
                                                                uint32_t *long_of, TextMeta *meta) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  // (no index to go by: the one text's bit, mate 1's, for both launches)
  if (meta->no_index & 1u) {
    const Rec none = {0, 0, 0, 0, 0};
    rec[r] = none;
    idr[r] = 0;
    len[r] = 0;
    long_of[r] = kNotLong;
    return;
  }
  uint32_t start[4], end[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const uint32_t line = 4u * (2u * r + (uint32_t)mate) + (uint32_t)l;
    start[l] = line == 0 ? 0u : nl[line - 1] + 1u;
    end[l] = nl[line];
    if (end[l] > start[l] && text[end[l] - 1] == '\r') --end[l];
  }
  Rec out = {0, 0, 0, 0, 0};
  bool bad = end[0] <= start[0] || text[start[0]] != '@' || end[2] <= start[2] || text[start[2]] != '+';
  const uint32_t sl = end[1] - start[1], ql = end[3] - start[3];
  bad = bad || sl != ql || end[0] - start[0] - 1u > 65535u;
  uint32_t long_slot = kNotLong;
  if (bad) {
    report(meta, r, ERR_MALFORMED);
  } else {
    atomicMax(&meta->max_len, sl);
    if (sl > CS_MAX_READ) report(meta, r, ERR_TOO_LONG);
    if (sl > stride || sl >= (uint32_t)CS_LEN_SKIP) {
      long_slot = atomicAdd(&meta->n_long[mate], 1u);  // (at most n of them: the list has n entries)
      cslong::LongRec lr;
      lr.rec = r;
      lr.seq_off = start[1];
      lr.qual_off = start[3];
      lr.len = sl;
      lrec[long_slot] = lr;
    }
    out.seq_off = start[1];
    out.qual_off = start[3];
    out.hdr_off = start[0] + 1u;
    uint32_t hl = end[0] - start[0] - 1u;
    const uint8_t *name = text + out.hdr_off;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint32_t k = tp.suffix_len[mate][s];
      if (k && hl >= k) {
        bool same = true;
        for (uint32_t i = 0; i < k; ++i) same = same && name[hl - k + i] == tp.suffix[mate][s][i];
        if (same) hl -= k;
      }
    }
    out.hdr_len = (uint16_t)hl;
    out.len = long_slot == kNotLong ? (uint16_t)sl : (uint16_t)0;  // (a long read leaves an empty row)
    uint32_t a = 0;
    while (a < hl && is_space(name[a])) ++a;
    uint32_t b = a;
    while (b < hl && !is_space(name[b])) ++b;
    uint32_t c = b;
    while (c < hl && is_space(name[c])) ++c;
    idr[r] = (b > a && c < hl) ? (a | ((b - a) << 16)) : (hl << 16);
  }
  rec[r] = out;
  len[r] = long_slot == kNotLong ? out.len : (uint16_t)CS_LEN_SKIP;
  long_of[r] = long_slot;
}

// dnaio.record_names_match: ids up to the first space / tab, one trailing 1 / 2 / 3 ignored in both
__global__ void __launch_bounds__(256) text_check_pairs(const uint8_t *text1, const Rec *rec1, const uint8_t *text2,
                                                        const Rec *rec2, uint32_t n, TextMeta *meta) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  // Leave only for a key of a record at or in front of this one (a malformed record of the parse kernels, the line-count
  // key on record 0, whose records are empty): the word is also written by the other blocks of THIS launch, and a
  // later record's key seen there must not keep this record's smaller one from being reported.  (~0 >> 8 is beyond
  // every record.)
  if (r >= n || (meta->err >> 8) <= r) return;
  const uint8_t *n1 = text1 + rec1[r].hdr_off, *n2 = text2 + rec2[r].hdr_off;
  const uint32_t l1 = rec1[r].hdr_len, l2 = rec2[r].hdr_len;
  uint32_t a = 0, b = 0;
  while (a < l1 && n1[a] != ' ' && n1[a] != '\t') ++a;
  while (b < l2 && n2[b] != ' ' && n2[b] != '\t') ++b;
  if (a && b && n1[a - 1] >= '1' && n1[a - 1] <= '3' && n2[b - 1] >= '1' && n2[b - 1] <= '3') {
    --a;
    --b;
  }
  bool same = a == b;
  for (uint32_t i = 0; same && i < a; ++i) same = n1[i] == n2[i];
  if (!same) report(meta, r, ERR_IDS_DIFFER);
}

// one lane per destination dword of the [n][stride] rows (both arrays): two aligned source dwords, one funnel shift
__global__ void __launch_bounds__(256) text_restride(const uint8_t *text, const Rec *rec, uint32_t n, uint32_t stride_dw,
                                                     uint32_t *seq_rows, uint32_t *qual_rows) {
  const unsigned long long total = (unsigned long long)n * stride_dw * 2ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total;
       i += (unsigned long long)gridDim.x * 256ull) {
    const uint32_t which = (uint32_t)(i >= total / 2);  // 0 sequence, 1 quality
    const unsigned long long j = which ? i - total / 2 : i;
    const uint32_t r = (uint32_t)(j / stride_dw), d = (uint32_t)(j - (unsigned long long)r * stride_dw);
    const Rec rc = rec[r];
    const uint32_t len = rc.len, first = 4u * d;
    // behind the read: 'N' in the sequence rows (the scan kernel's fast re-coding vouches for A, C, G, T and N:
    // trim_kernel.hip.inc, encode4_pairs_fast), 0 in the quality rows
    const uint32_t fill = which ? 0u : 0x4E4E4E4Eu;
    uint32_t w = fill;
    if (first < len) {
      const uint32_t src = (which ? rc.qual_off : rc.seq_off) + first;
      const uint32_t *p = reinterpret_cast<const uint32_t *>(text + (src & ~3u));
      const uint32_t lo = p[0], hi = (src & 3u) ? p[1] : 0u;  // (the text allocation is padded: p[1] exists)
      w = __builtin_amdgcn_alignbyte(hi, lo, src & 3u);
      if (first + 4u > len) {
        const uint32_t keep = 0xffffffffu >> (8u * (first + 4u - len));
        w = (w & keep) | (fill & ~keep);
      }
    }
    (which ? qual_rows : seq_rows)[(size_t)r * stride_dw + d] = w;
  }
}

// ---- output --------------------------------------------------------------------------------------------------

struct FormatArgs {
  const uint8_t *text[2];
  const Rec *rec[2];
  const uint32_t *idr[2];
  const uint8_t *seq[2];   // [n][stride] rows
  const uint8_t *qual[2];
  const cs_result *res[2];
  const cs_cap2 *cap2;     // single-end plans with two captures, else null
  const uint32_t *long_of[2];        // per record: index into lrec / lres, or kNotLong
  const cslong::LongRec *lrec[2];
  const cslong::LongRes *lres[2];
  const uint8_t *xf[2];    // TextParams.filters: cs_reads.xflags of the tile kernels (long reads: LongRes.xflags)
  uint32_t n, stride;
  uint32_t *blk;           // [n_blocks][6] block sums (8 with a too-long route), then their exclusive scan (column = route * 2 + mate)
  unsigned long long *totals;  // [6] column sums (8 with a too-long route)
  uint32_t *dst[2];        // per mate: byte offset of every record's output inside the mate's buffer | route class << 30
  uint8_t *out[2];
  TextMeta *meta;
  // demultiplexing plans (TextParams.n_bins > 0): routes 0 .. 2 + n_bins; too-long plans (TextParams.too_long_route):
  // routes 0 .. 3, no bc
  const uint8_t *bc;                  // per record: barcode index (CS_DEMUX_NONE: none)
  unsigned long long *route_bytes;    // out [route][mate]: bytes of every route stream
  uint32_t *route_count;              // out [route]: records (pairs) per route
};

struct RecordShape {
  uint32_t route, len[2];
  uint32_t why;  // route == kRouteDiscard: 1 << 10 * k for the k-th of TooLong, TooManyN, TooManyExpectedErrors (the
                 // first that caught the pair); 0 otherwise.  Three ten-bit counters sum in one word over a block.
};

// One mate's read as the formatter sees it, wherever its result came from: the rows and 8-byte results of the tile
// kernels, or the text and the 32-bit results of the long-read kernel.
struct ReadView {
  const uint8_t *seq, *qual;
  uint32_t start, stop, cap_off, cap_len, cap2_off, cap2_len, flags;
};

__device__ __forceinline__ ReadView read_view(const FormatArgs &a, uint32_t m, uint32_t r) {
  ReadView v;
  const uint32_t slot = a.long_of[m][r];
  if (slot != kNotLong) {
    const cslong::LongRec lr = a.lrec[m][slot];
    const cslong::LongRes x = a.lres[m][slot];
    v.seq = a.text[m] + lr.seq_off;
    v.qual = a.text[m] + lr.qual_off;
    v.start = x.start;
    v.stop = x.stop;
    v.cap_off = x.cap_off;
    v.cap_len = x.cap_len;
    v.cap2_off = x.cap2_off;
    v.cap2_len = x.cap2_len;
    v.flags = x.flags;
    return v;
  }
  const cs_result x = a.res[m][r];
  v.seq = a.seq[m] + (size_t)r * a.stride;
  v.qual = a.qual[m] + (size_t)r * a.stride;
  v.start = x.start;
  v.stop = x.stop;
  v.cap_off = x.cap_off;
  v.cap_len = x.cap_len;
  v.flags = x.flags;
  v.cap2_off = v.cap2_len = 0;
  if (m == 0 && a.cap2) {
    v.cap2_off = a.cap2[r].off;
    v.cap2_len = a.cap2[r].len;
  }
  return v;
}

__device__ __forceinline__ uint32_t xflags_of(const FormatArgs &a, uint32_t m, uint32_t r) {
  const uint32_t slot = a.long_of[m][r];
  return slot != kNotLong ? a.lres[m][slot].xflags : a.xf[m][r];
}

// the class of a route as TextParams.fasta_routes counts them
__device__ __forceinline__ uint32_t route_class(uint32_t route) { return route < 3u ? route : 3u; }

__device__ __forceinline__ bool fasta_stream(const TextParams &tp, uint32_t cls, uint32_t m) {
  return (tp.fasta_routes >> (2u * cls + m)) & 1u;
}

// ---- record names ------------------------------------------------------------------------------------------------
// The name of an output record is the run's default -- id ['_' UMI], what the reference's (PairedEnd)Renamer writes
// (cutseq/run.py:377-380, 642-645) -- or, with cs_text_set_rename, what a template makes of the header and the captures.
// A kernel that takes a RenameTable behind its other arguments formats by the template; every such kernel is declared
// with a trailing pack that is empty for the default name, so that one body serves both and the default's instantiation
// is the code it was.

constexpr uint32_t kRenameSegs = CS_RENAME_MAX_SEGMENTS, kRenameLiteral = CS_RENAME_MAX_LITERAL;

struct RenameTable {  // by value, behind TextParams
  uint32_t n;
  cs_rename_seg seg[kRenameSegs];
  uint8_t lit[kRenameLiteral + 1u];
};

struct NameParts {  // Renamer.parse_name on the header behind the SuffixRemover chain
  const uint8_t *hdr;
  uint32_t hdr_len, id_off, id_len, com_off, com_len;
};

__device__ __forceinline__ NameParts name_parts(const FormatArgs &a, uint32_t m, uint32_t r) {
  NameParts p;
  const uint32_t idr = a.idr[m][r];
  p.hdr = a.text[m] + a.rec[m][r].hdr_off;
  p.hdr_len = a.rec[m][r].hdr_len;
  p.id_off = idr & 0xffffu;
  p.id_len = idr >> 16;
  // two fields (text_parse_records): the comment begins behind the blank run that follows the id, its own trailing
  // blanks stay; one field: the id is the whole header and there is no comment
  uint32_t c = p.id_off + p.id_len;
  while (c < p.hdr_len && is_space(p.hdr[c])) ++c;
  p.com_off = c;
  p.com_len = p.hdr_len - c;
  return p;
}

// The capture a segment names: the first or second of mate 1, of mate 2 or of the written mate (a single-end r2 is r1).
// (From copies of the fields: `c ? r1.x : r2.x` is an lvalue, a choice between two addresses, and put both views into
// scratch.)
struct Capture {
  const uint8_t *at;
  uint32_t len;
};

__device__ __forceinline__ Capture capture_of(const cs_rename_seg &s, uint32_t m, const ReadView &r1, const ReadView &r2) {
  const bool mate2 = (s.mate == CS_RENAME_OWN ? m : (uint32_t)s.mate) != 0u, second = s.kind == CS_RENAME_CAPTURE2;
  const uint8_t *const seq1 = r1.seq, *const seq2 = r2.seq;
  const uint32_t off1a = r1.cap_off, off1b = r1.cap2_off, off2a = r2.cap_off, off2b = r2.cap2_off;
  const uint32_t len1a = r1.cap_len, len1b = r1.cap2_len, len2a = r2.cap_len, len2b = r2.cap2_len;
  Capture c;
  c.at = mate2 ? seq2 + (second ? off2b : off2a) : seq1 + (second ? off1b : off1a);
  c.len = mate2 ? (second ? len2b : len2a) : (second ? len1b : len1a);
  return c;
}

__device__ __forceinline__ uint32_t segment_len(const cs_rename_seg &s, const NameParts &p, uint32_t m, const ReadView &r1,
                                                const ReadView &r2) {
  switch (s.kind) {
    case CS_RENAME_LITERAL: return s.lit_len;
    case CS_RENAME_HEADER: return p.hdr_len;
    case CS_RENAME_ID: return p.id_len;
    case CS_RENAME_COMMENT: return p.com_len;
    case CS_RENAME_CAPTURE:
    case CS_RENAME_CAPTURE2: return capture_of(s, m, r1, r2).len;
    default: return 1u;  // CS_RENAME_MATE
  }
}

// bytes of mate m's name: the default template's (`tag`: '_' and the captures, 0 without a UMI) ...
__device__ __forceinline__ uint32_t name_len(const FormatArgs &a, uint32_t m, uint32_t r, uint32_t tag, const ReadView &,
                                             const ReadView &) {
  return (a.idr[m][r] >> 16) + tag;
}

// ... or a --rename template's
__device__ __forceinline__ uint32_t name_len(const FormatArgs &a, uint32_t m, uint32_t r, uint32_t, const ReadView &r1,
                                             const ReadView &r2, const RenameTable &rn) {
  const NameParts p = name_parts(a, m, r);
  uint32_t n = 0;
  for (uint32_t i = 0; i < rn.n; ++i) n += segment_len(rn.seg[i], p, m, r1, r2);
  return n;
}

// The stretch copy of format_copy (there: why), 32 lanes per stretch: a lane holds its dwords of the first 256 bytes,
// so that a caller can issue the loads of several stretches before the first store; longer stretches finish in a loop
// behind the stores.
struct Held {
  uint32_t v0, v1, tail;
};

__device__ __forceinline__ Held stretch_load(uint32_t lane, const uint8_t *src, uint32_t n) {
  Held h{0u, 0u, 0u};
  const uint32_t i0 = 4u * lane, i1 = i0 + 128u, r = n & 3u;
  if (i0 + 4u <= n) __builtin_memcpy(&h.v0, src + i0, 4);
  if (i1 + 4u <= n) __builtin_memcpy(&h.v1, src + i1, 4);
  if (lane < r) h.tail = src[n - r + lane];
  return h;
}

__device__ __forceinline__ void stretch_store(uint32_t lane, uint8_t *dst, const uint8_t *src, uint32_t n, const Held &h) {
  const uint32_t i0 = 4u * lane, i1 = i0 + 128u, r = n & 3u;
  if (i0 + 4u <= n) __builtin_memcpy(dst + i0, &h.v0, 4);
  if (i1 + 4u <= n) __builtin_memcpy(dst + i1, &h.v1, 4);
  if (lane < r) dst[n - r + lane] = (uint8_t)h.tail;
  for (uint32_t i = i0 + 256u; i + 4u <= n; i += 128u) {
    uint32_t v;
    __builtin_memcpy(&v, src + i, 4);
    __builtin_memcpy(dst + i, &v, 4);
  }
}

// Mate m's name by the template, written by the record's 32 lanes; `out` stands behind the '@'.  The segments one after
// the other, control flow uniform over the lanes: the header's pieces by the stretch copy, literals and captures a byte
// per lane (with the loop for those beyond 32 bytes), the mate's digit by lane 0.
__device__ __forceinline__ void emit_name(const FormatArgs &a, const RenameTable &rn, uint32_t m, uint32_t r, const ReadView &r1,
                                          const ReadView &r2, uint8_t *out, uint32_t lane) {
  const NameParts p = name_parts(a, m, r);
  for (uint32_t i = 0; i < rn.n; ++i) {
    const cs_rename_seg s = rn.seg[i];
    const uint32_t n = segment_len(s, p, m, r1, r2);
    if (s.kind == CS_RENAME_HEADER || s.kind == CS_RENAME_ID || s.kind == CS_RENAME_COMMENT) {
      const uint8_t *src = p.hdr + (s.kind == CS_RENAME_ID ? p.id_off : (s.kind == CS_RENAME_COMMENT ? p.com_off : 0u));
      const Held h = stretch_load(lane, src, n);
      stretch_store(lane, out, src, n, h);
    } else if (s.kind == CS_RENAME_LITERAL) {
      for (uint32_t t = lane; t < n; t += 32u) out[t] = rn.lit[s.lit_off + t];
    } else if (s.kind == CS_RENAME_CAPTURE || s.kind == CS_RENAME_CAPTURE2) {
      const uint8_t *src = capture_of(s, m, r1, r2).at;
      for (uint32_t t = lane; t < n; t += 32u) out[t] = src[t];
    } else if (lane == 0) {
      out[0] = (uint8_t)('1' + m);
    }
    out += n;
  }
}

// kTooLong (TextParams.too_long_route; the four-route kernels): the pair TooLong catches is written, as route 3
template <bool kTooLong = false, class... Rename>
__device__ __forceinline__ RecordShape record_shape(const FormatArgs &a, const TextParams &tp, uint32_t r, const Rename &... rn) {
  RecordShape s;
  const ReadView r1 = read_view(a, 0, r);
  uint32_t flags = r1.flags, tag = 0;
  ReadView r2 = r1;
  if (tp.paired) {
    r2 = read_view(a, 1, r);
    flags |= r2.flags;
  }
  if (tp.has_umi) tag = 1u + r1.cap_len + (tp.paired ? r2.cap_len : r1.cap2_len);
  s.route = (flags & tp.flag_too_short) ? 1u : ((tp.untrimmed_filter && (flags & tp.flag_untrimmed)) ? 2u : 0u);
  // TooLong -> TooManyN -> TooManyExpectedErrors (pair filter "any": the OR of the mates' bits), behind TooShort and
  // in front of IsUntrimmedAny: no file for any of them (kTooLong: route 3 for the first), the pair counts under the
  // first that catches it
  s.why = 0;
  if (tp.filters && s.route != 1u) {
    const uint32_t xf = (xflags_of(a, 0, r) | (tp.paired ? xflags_of(a, 1, r) : 0u)) & tp.filters;
    if (xf) {
      s.route = (kTooLong && (xf & CS_X_TOO_LONG)) ? 3u : kRouteDiscard;  // (why counts the pair either way)
      s.why = (xf & CS_X_TOO_LONG) ? 1u : ((xf & CS_X_TOO_MANY_N) ? 1u << 10 : 1u << 20);
    }
  }
  if (tp.n_bins && s.route == 0u) {
    const uint32_t slot = a.long_of[tp.demux_mate][r];  // (a read longer than the rows: its barcode is in the long kernel's result)
    const uint32_t bc = slot != kNotLong ? a.lres[tp.demux_mate][slot].bc : a.bc[r];
    if (bc != CS_DEMUX_NONE) s.route = 3u + bc;
  }
  // '@' name '\n' seq "\n+\n" qual '\n'   or, without qualities,   '>' name '\n' seq '\n'
  // -- which of the two goes by the file the (route, mate) stream is written to
  const uint32_t cls = route_class(s.route);  // (kRouteDiscard counts as 3 here: nobody looks at its sizes)
  const bool fa1 = fasta_stream(tp, cls, 0), fa2 = fasta_stream(tp, cls, 1);
  s.len[0] = name_len(a, 0, r, tag, r1, r2, rn...) + (fa1 ? 1u : 2u) * (r1.stop - r1.start) + (fa1 ? 3u : 6u);
  s.len[1] = tp.paired ? name_len(a, 1, r, tag, r1, r2, rn...) + (fa2 ? 1u : 2u) * (r2.stop - r2.start) + (fa2 ? 3u : 6u) : 0u;
  return s;
}

// a block's discards (RecordShape.why summed over its 256 records) -> the batch's three counts
__device__ __forceinline__ void add_discards(TextMeta *meta, uint32_t packed) {
  if (packed & 0x3ffu) atomicAdd(&meta->n_too_long, packed & 0x3ffu);
  if ((packed >> 10) & 0x3ffu) atomicAdd(&meta->n_too_many_n, (packed >> 10) & 0x3ffu);
  if (packed >> 20) atomicAdd(&meta->n_too_many_ee, packed >> 20);
}

// (a rejected batch is not formatted: sizes derived from half-parsed records could exceed the output buffers)
// kRoutes = 3: the plain plan.  kRoutes = 4: a too-long plan (TextParams.too_long_route), route 3 = the pairs TooLong
// caught; 2 * kRoutes columns in blk / totals.  A lane behind the last record holds route kRoutes: in no column.
// No plan but a too-long plan launches the <4> pair.
template <uint32_t kRoutes, class... Rename>
__global__ void __launch_bounds__(256) format_sizes(FormatArgs a, TextParams tp, Rename... rn) {
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  RecordShape s = {kRoutes, {0u, 0u}, 0u};
  if (r < a.n) s = record_shape<kRoutes == 4u>(a, tp, r, rn...);
#pragma unroll
  for (uint32_t c = 0; c < 2u * kRoutes; ++c) {
    uint32_t total;
    (void)block_scan_256(s.route == (c >> 1) ? s.len[c & 1] : 0u, total, sh);
    if (threadIdx.x == 0) a.blk[blockIdx.x * (2u * kRoutes) + c] = total;
  }
}

template <uint32_t kRoutes, class... Rename>
__global__ void __launch_bounds__(256) format_offsets(FormatArgs a, TextParams tp, Rename... rn) {
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  RecordShape s = {kRoutes, {0u, 0u}, 0u};
  if (r < a.n) s = record_shape<kRoutes == 4u>(a, tp, r, rn...);
  // where a route's stream starts inside the mate's buffer: behind the routes in front of it
  unsigned long long base[kRoutes][2];
  for (int m = 0; m < 2; ++m) {
    base[0][m] = 0;
    base[1][m] = a.totals[0 * 2 + m];
    base[2][m] = base[1][m] + a.totals[1 * 2 + m];
    if (kRoutes == 4u) base[kRoutes - 1u][m] = base[2][m] + a.totals[2 * 2 + m];
  }
  uint32_t mine[2] = {0, 0};
#pragma unroll
  for (uint32_t c = 0; c < 2u * kRoutes; ++c) {
    uint32_t total;
    const uint32_t local = block_scan_256(s.route == (c >> 1) ? s.len[c & 1] : 0u, total, sh);
    if (s.route == (c >> 1)) mine[c & 1] = (uint32_t)base[c >> 1][c & 1] + a.blk[blockIdx.x * (2u * kRoutes) + c] + local;
  }
  uint32_t counts[kRoutes];
#pragma unroll
  for (uint32_t q = 0; q < kRoutes; ++q) {
    uint32_t total;
    (void)block_scan_256(s.route == q ? 1u : 0u, total, sh);
    counts[q] = total;
  }
  uint32_t discarded = 0;
  if (tp.filters) (void)block_scan_256(r < a.n ? s.why : 0u, discarded, sh);
  // cutadapt's written_bp: what reaches the final sink (report.account_chunk)
  uint32_t kept_bp[2] = {0, 0};
#pragma unroll
  for (uint32_t m = 0; m < 2; ++m) {
    uint32_t bp = 0;
    if (r < a.n && s.route == 0u && (m == 0 || tp.paired)) {
      const ReadView v = read_view(a, m, r);
      bp = v.stop - v.start;
    }
    (void)block_scan_256(bp, kept_bp[m], sh);
  }
  if (r < a.n) {
    const bool gone = s.route == kRouteDiscard;
    a.dst[0][r] = gone ? kDiscarded : mine[0] | (s.route << 30);
    if (tp.paired) a.dst[1][r] = gone ? kDiscarded : mine[1] | (s.route << 30);
  }
  if (threadIdx.x == 0) {
    for (uint32_t q = 0; q < 3; ++q)
      if (counts[q]) atomicAdd(&a.meta->route_count[q], counts[q]);
    if (kRoutes == 4u)  // (the summary keeps its three routes; the fourth is in the route block alone)
      for (uint32_t q = 0; q < kRoutes; ++q)
        if (counts[q]) atomicAdd(&a.route_count[q], counts[q]);
    add_discards(a.meta, discarded);
    for (uint32_t m = 0; m < 2; ++m)
      if (kept_bp[m]) atomicAdd(&a.meta->written_bp[m], (unsigned long long)kept_bp[m]);
    if (blockIdx.x == 0) {
      for (int m = 0; m < 2; ++m) {
        a.meta->out_bytes[m] = a.totals[m] + a.totals[2 + m] + a.totals[4 + m] + (kRoutes == 4u ? a.totals[2u * (kRoutes - 1u) + m] : 0ull);
        for (int q = 0; q < 3; ++q) a.meta->route_bytes[q][m] = a.totals[q * 2 + m];
        if (kRoutes == 4u)
          for (uint32_t q = 0; q < kRoutes; ++q) a.route_bytes[q * 2u + m] = a.totals[q * 2u + m];
      }
    }
  }
}

// ---- the same two steps for interleaved output (cs_text_create_interleaved, CS_INTERLEAVE_OUT): a route's two mate
// streams are ONE stream in mate 1's buffer, record of mate 1, record of mate 2, pair after pair.  One column per route
// (blk / totals hold kRoutes of them), a pair contributes len[0] + len[1]; the first mate's record stands at the pair's
// offset and the second's behind it.  dst[0] and dst[1] are offsets into the one buffer (FormatArgs.out[1] == out[0]),
// so format_copy runs as it is.  `second_first` (CS_INTERLEAVE_OUT_MATE2_FIRST): mate 2's record leads.
template <uint32_t kRoutes, class... Rename>
__global__ void __launch_bounds__(256) format_sizes_woven(FormatArgs a, TextParams tp, Rename... rn) {
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  RecordShape s = {kRoutes, {0u, 0u}, 0u};
  if (r < a.n) s = record_shape<kRoutes == 4u>(a, tp, r, rn...);
#pragma unroll
  for (uint32_t c = 0; c < kRoutes; ++c) {
    uint32_t total;
    (void)block_scan_256(s.route == c ? s.len[0] + s.len[1] : 0u, total, sh);
    if (threadIdx.x == 0) a.blk[blockIdx.x * kRoutes + c] = total;
  }
}

template <uint32_t kRoutes, class... Rename>
__global__ void __launch_bounds__(256) format_offsets_woven(FormatArgs a, TextParams tp, uint32_t second_first, Rename... rn) {
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  RecordShape s = {kRoutes, {0u, 0u}, 0u};
  if (r < a.n) s = record_shape<kRoutes == 4u>(a, tp, r, rn...);
  // where a route's stream starts inside the buffer: behind the routes in front of it
  unsigned long long base[kRoutes];
  base[0] = 0;
  for (uint32_t q = 1; q < kRoutes; ++q) base[q] = base[q - 1u] + a.totals[q - 1u];
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t c = 0; c < kRoutes; ++c) {
    uint32_t total;
    const uint32_t local = block_scan_256(s.route == c ? s.len[0] + s.len[1] : 0u, total, sh);
    if (s.route == c) mine = (uint32_t)base[c] + a.blk[blockIdx.x * kRoutes + c] + local;
  }
  uint32_t counts[kRoutes];
#pragma unroll
  for (uint32_t q = 0; q < kRoutes; ++q) {
    uint32_t total;
    (void)block_scan_256(s.route == q ? 1u : 0u, total, sh);
    counts[q] = total;
  }
  uint32_t discarded = 0;
  if (tp.filters) (void)block_scan_256(r < a.n ? s.why : 0u, discarded, sh);
  uint32_t kept_bp[2] = {0, 0};
#pragma unroll
  for (uint32_t m = 0; m < 2; ++m) {
    uint32_t bp = 0;
    if (r < a.n && s.route == 0u) {
      const ReadView v = read_view(a, m, r);
      bp = v.stop - v.start;
    }
    (void)block_scan_256(bp, kept_bp[m], sh);
  }
  if (r < a.n) {
    const bool gone = s.route == kRouteDiscard;
    const uint32_t lead = second_first ? 1u : 0u;
    a.dst[lead][r] = gone ? kDiscarded : mine | (s.route << 30);
    a.dst[lead ^ 1u][r] = gone ? kDiscarded : (mine + s.len[lead]) | (s.route << 30);
  }
  if (threadIdx.x == 0) {
    for (uint32_t q = 0; q < 3; ++q)
      if (counts[q]) atomicAdd(&a.meta->route_count[q], counts[q]);
    if (kRoutes == 4u)
      for (uint32_t q = 0; q < kRoutes; ++q)
        if (counts[q]) atomicAdd(&a.route_count[q], counts[q]);
    add_discards(a.meta, discarded);
    for (uint32_t m = 0; m < 2; ++m)
      if (kept_bp[m]) atomicAdd(&a.meta->written_bp[m], (unsigned long long)kept_bp[m]);
    if (blockIdx.x == 0) {  // (mate 2's sizes stay the zeros text_init_meta and the route block's memset wrote)
      unsigned long long all = 0;
      for (uint32_t q = 0; q < kRoutes; ++q) all += a.totals[q];
      a.meta->out_bytes[0] = all;
      for (int q = 0; q < 3; ++q) a.meta->route_bytes[q][0] = a.totals[q];
      if (kRoutes == 4u)
        for (uint32_t q = 0; q < kRoutes; ++q) a.route_bytes[q * 2u] = a.totals[q];
    }
  }
}

// ---- the same two steps for demultiplexing plans: 3 + n_bins routes.  A block scan per route would be 500 scans; here
// the block keeps per-route sums in LDS, and a record's place among the records of ITS route inside the block comes
// from the lanes of its wave that share the route (nine ballots make the peer mask) plus the waves in front.
__global__ void __launch_bounds__(256) format_sizes_bins(FormatArgs a, TextParams tp) {
  __shared__ uint32_t acc[kMaxRoutes * 2];
  if (a.meta->err != ~0ull) return;
  const uint32_t cols = (3u + tp.n_bins) * 2u;
  for (uint32_t i = threadIdx.x; i < cols; i += 256u) acc[i] = 0;
  __syncthreads();
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < a.n) {
    const RecordShape s = record_shape(a, tp, r);
    if (s.route != kRouteDiscard) {
      atomicAdd(&acc[s.route * 2u], s.len[0]);
      if (tp.paired) atomicAdd(&acc[s.route * 2u + 1u], s.len[1]);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cols; i += 256u) a.blk[(size_t)blockIdx.x * cols + i] = acc[i];
}

__global__ void __launch_bounds__(256) format_offsets_bins(FormatArgs a, TextParams tp) {
  __shared__ uint32_t base[kMaxRoutes * 2];     // where this block's records of a route start in the mate's buffer
  __shared__ uint32_t wsum[4][kMaxRoutes * 2];  // bytes per wave and route
  __shared__ uint32_t rcount[kMaxRoutes];
  __shared__ uint32_t sz[256][2];
  __shared__ uint32_t n_gone;
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t routes = 3u + tp.n_bins, cols = routes * 2u;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i < cols; i += 256u) wsum[0][i] = wsum[1][i] = wsum[2][i] = wsum[3][i] = 0;
  for (uint32_t i = tid; i < routes; i += 256u) rcount[i] = 0;
  if (tid == 0) n_gone = 0;
  if (tid < 2u) {  // the routes' streams lie back to back in route order: a running sum over the column totals
    unsigned long long run = 0;
    for (uint32_t q = 0; q < routes; ++q) {
      base[q * 2u + tid] = (uint32_t)run + a.blk[(size_t)blockIdx.x * cols + q * 2u + tid];
      run += a.totals[q * 2u + tid];
    }
  }
  __syncthreads();
  const uint32_t r = blockIdx.x * 256u + tid;
  RecordShape s = {0x1ffu, {0u, 0u}, 0u};  // (lanes behind the last record: a route of their own)
  if (r < a.n) {
    s = record_shape(a, tp, r);
    if (s.route == kRouteDiscard) {
      s.len[0] = s.len[1] = 0;
      atomicAdd(&n_gone, s.why);
    } else {
      atomicAdd(&wsum[wave][s.route * 2u], s.len[0]);
      if (tp.paired) atomicAdd(&wsum[wave][s.route * 2u + 1u], s.len[1]);
      atomicAdd(&rcount[s.route], 1u);
    }
  }
  sz[tid][0] = s.len[0];
  sz[tid][1] = s.len[1];
  __syncthreads();
  // the lanes of this wave with the same route, and what the ones in front of this lane take
  unsigned long long peers = ~0ull;
#pragma unroll
  for (uint32_t bit = 0; bit < 9u; ++bit) {
    const bool one = (s.route >> bit) & 1u;
    const unsigned long long b = __ballot(one);
    peers &= one ? b : ~b;
  }
  unsigned long long front = peers & ((1ull << lane) - 1ull);
  uint32_t mine[2] = {0, 0};
  while (front) {
    const uint32_t j = (uint32_t)__builtin_ctzll(front);
    front &= front - 1ull;
    mine[0] += sz[wave * 64u + j][0];
    mine[1] += sz[wave * 64u + j][1];
  }
  if (r < a.n && s.route == kRouteDiscard) {
    a.dst[0][r] = kDiscarded;
    if (tp.paired) a.dst[1][r] = kDiscarded;
  } else if (r < a.n) {
#pragma unroll
    for (uint32_t m = 0; m < 2u; ++m) {
      uint32_t at = base[s.route * 2u + m] + mine[m];
      for (uint32_t w = 0; w < wave; ++w) at += wsum[w][s.route * 2u + m];
      if (m == 0 || tp.paired) a.dst[m][r] = at | (route_class(s.route) << 30);  // (cs_text_create keeps a mate's output below 1 GiB)
    }
  }
  uint32_t kept_bp[2] = {0, 0};
#pragma unroll
  for (uint32_t m = 0; m < 2; ++m) {
    uint32_t bp = 0;
    if (r < a.n && (s.route == 0u || (s.route >= 3u && s.route != kRouteDiscard)) && (m == 0 || tp.paired)) {
      const ReadView v = read_view(a, m, r);
      bp = v.stop - v.start;
    }
    (void)block_scan_256(bp, kept_bp[m], sh);
  }
  for (uint32_t q = tid; q < routes; q += 256u)
    if (rcount[q]) {
      atomicAdd(&a.route_count[q], rcount[q]);
      atomicAdd(&a.meta->route_count[q < 3u ? q : 0u], rcount[q]);  // (the summary keeps three routes: every barcode's reads are "trimmed")
    }
  if (tid == 0) {
    for (uint32_t m = 0; m < 2; ++m)
      if (kept_bp[m]) atomicAdd(&a.meta->written_bp[m], (unsigned long long)kept_bp[m]);
    add_discards(a.meta, n_gone);
  }
  if (blockIdx.x == 0) {
    for (uint32_t i = tid; i < cols; i += 256u) a.route_bytes[i] = a.totals[i];
    if (tid < 2u) {
      unsigned long long all = 0, binned = 0;
      for (uint32_t q = 0; q < routes; ++q) {
        all += a.totals[q * 2u + tid];
        if (q == 0u || q >= 3u) binned += a.totals[q * 2u + tid];
      }
      a.meta->out_bytes[tid] = all;
      a.meta->route_bytes[0][tid] = binned;
      a.meta->route_bytes[1][tid] = a.totals[2u + tid];
      a.meta->route_bytes[2][tid] = a.totals[4u + tid];
    }
  }
}

__device__ __forceinline__ uint8_t complement(uint8_t c) {
  // cutseq/run.py:164-196 (ReverseComplementConverter through common.reverse_complement): ATGCatgc only
  switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'G': return 'C';
    case 'C': return 'G';
    case 'a': return 't';
    case 't': return 'a';
    case 'g': return 'c';
    case 'c': return 'g';
    default: return c;
  }
}

// 32 lanes per output record: byte j of the record -> the source byte it copies.  kMixed: the output files name
// different formats, so FASTA or FASTQ is a property of the record (its route class, from the top bits of its dst,
// and its mate); otherwise the one format of the whole grid, a scalar as before streams had formats of their own.
template <bool kMixed, class... Rename>
__global__ void __launch_bounds__(256) format_copy(FormatArgs a, TextParams tp, Rename... rn) {
  constexpr bool kRenamed = sizeof...(Rename) != 0;  // the name by a template (emit_name), not id ['_' UMI]
  if (a.meta->err != ~0ull) return;
  const uint32_t lane = threadIdx.x & 31u;
  const uint32_t mates = tp.paired ? 2u : 1u;
  const unsigned long long items = (unsigned long long)a.n * mates;
  for (unsigned long long it = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) >> 5; it < items;
       it += ((unsigned long long)gridDim.x * 256ull) >> 5) {
    const uint32_t m = tp.paired ? (uint32_t)(it & 1ull) : 0u, r = (uint32_t)(tp.paired ? it >> 1 : it);
    if (tp.filters && a.dst[m][r] == kDiscarded) continue;  // (a discarded pair; uniform over the record's 32 lanes)
    const ReadView me = read_view(a, m, r);
    const ReadView r1 = m == 0 ? me : read_view(a, 0, r);
    const uint8_t *id = nullptr, *tag1 = nullptr, *tag2 = nullptr;
    uint32_t id_len = 0, t1 = 0, t2 = 0, tag = 0;
    ReadView r2 = r1;
    if constexpr (kRenamed) {
      if (tp.paired) r2 = m == 1 ? me : read_view(a, 1, r);
      id_len = name_len(a, m, r, 0u, r1, r2, rn...);  // (the whole name stands where the id does)
    } else {
      const uint32_t idr = a.idr[m][r];
      id_len = idr >> 16;
      id = a.text[m] + a.rec[m][r].hdr_off + (idr & 0xffffu);
      tag1 = r1.seq + r1.cap_off;
      if (tp.has_umi) {
        t1 = r1.cap_len;
        if (tp.paired) {
          r2 = m == 1 ? me : read_view(a, 1, r);
          tag2 = r2.seq + r2.cap_off;
          t2 = r2.cap_len;
        } else {
          tag2 = r1.seq + r1.cap2_off;
          t2 = r1.cap2_len;
        }
      }
      tag = tp.has_umi ? 1u + t1 + t2 : 0u;
    }
    const uint32_t L = me.stop - me.start;
    const uint8_t *seq = me.seq, *qual = me.qual;
    const bool rc = tp.reverse_complement && !tp.paired;
    const uint32_t dst = a.dst[m][r];
    const bool fasta = kMixed ? fasta_stream(tp, dst >> 30, m) : tp.fasta_routes != 0;
    uint8_t *out = a.out[m] + (dst & 0x3fffffffu);
    // segment ends: '@' | id | tag | '\n' | seq | "\n+\n" | qual | '\n'
    // (FASTA output: the record ends with the line end behind the sequence -- byte e_seq, which the '+' branch below
    // writes as '\n')
    const uint32_t e_id = 1u + id_len, e_tag = e_id + tag, e_seq = e_tag + 1u + L, e_plus = e_seq + 3u;
    const uint32_t total = fasta ? e_seq + 1u : e_plus + L + 1u;
    // Stretch by stretch (round 5): the id, the bases and the qualities are copied four bytes per lane and step --
    // unaligned dword loads and stores, uniform control flow --, the UMI tag and the fixed bytes by single lanes.  (A byte
    // per lane and step, every byte picked by an eight-way chain of comparisons, moved 134 MB per batch of 262 144 pairs
    // in 0.43 ms: the text path's largest kernel.  Quads across the whole record with a byte-wise path for the ones that
    // straddle a stretch were slower still, 0.65 ms: every step of every wave has such a quad.)
    // ... and every stretch's loads are issued before the first store (the stores of one stretch used to stand between
    // the loads of the next: uint8_t pointers may alias, so each stretch paid its own trip to memory): stretch_load /
    // stretch_store.
    auto load = [&](const uint8_t *src, uint32_t n) -> Held { return stretch_load(lane, src, n); };
    auto store = [&](uint8_t *dst, const uint8_t *src, uint32_t n, const Held &h) { stretch_store(lane, dst, src, n, h); };
    Held h_id{0u, 0u, 0u};
    if constexpr (!kRenamed) h_id = load(id, id_len);
    Held h_seq{0u, 0u, 0u}, h_qual{0u, 0u, 0u};
    if (!rc) {
      h_seq = load(seq + me.start, L);
      if (!fasta) h_qual = load(qual + me.start, L);
    }
    if constexpr (kRenamed) {
      if (lane == 0) out[0] = fasta ? '>' : '@';
      emit_name(a, rn..., m, r, r1, r2, out + 1u, lane);
    } else {
      uint8_t tag_byte = (uint8_t)'_';  // (tags of up to 32 bytes: one per lane; longer ones finish in the loop below)
      if (lane > 0 && lane < tag) tag_byte = lane <= t1 ? tag1[lane - 1u] : tag2[lane - 1u - t1];
      if (lane == 0) out[0] = fasta ? '>' : '@';
      store(out + 1u, id, id_len, h_id);
      if (lane < tag) out[e_id + lane] = tag_byte;
      for (uint32_t t = lane + 32u; t < tag; t += 32u) out[e_id + t] = t <= t1 ? tag1[t - 1u] : tag2[t - 1u - t1];
    }
    if (lane == 1) out[e_tag] = '\n';
    if (!rc) {
      store(out + e_tag + 1u, seq + me.start, L, h_seq);
    } else {
      for (uint32_t t = lane; t < L; t += 32u) out[e_tag + 1u + t] = complement(seq[me.stop - 1u - t]);
    }
    if (fasta) {
      if (lane == 2) out[e_seq] = '\n';
    } else {
      if (lane >= 2 && lane <= 4) out[e_seq + lane - 2u] = lane == 3 ? (uint8_t)'+' : (uint8_t)'\n';
      if (!rc) {
        store(out + e_plus, qual + me.start, L, h_qual);
      } else {
        for (uint32_t t = lane; t < L; t += 32u) out[e_plus + t] = qual[me.stop - 1u - t];
      }
      if (lane == 5) out[total - 1u] = '\n';
    }
  }
}

}  // namespace cstext
