// info_kernels.hip.inc -- cutadapt's --info-file on the device: which adapter matched where, read by read (device code
// only).  Included by cutseq_hip.hip behind text_kernels.hip.inc.  gfx950 / wave64 only.
//
// The reference marks the table as a TODO in front of its TooShort step (cutseq/run.py: "# TODO: report info",
// PairedSingleEndStep(InfoFileWriter(...))): one row per adapter match of read 1, one "-1" row for a read without a
// match, every input record, input order.  The trimming kernels keep the surviving interval and eight flag bits per
// read; where an op matched and with how many errors is lost.  Nothing here runs unless cs_text_params.info asks:
//
//   info_record    one lane per record of mate 1: the long-read kernel's walk of the op chain (cslong::walk_chain),
//                  straight from the uploaded text (any read length) -- the aligner's columns sized by the plan's
//                  longest adapter -- with every match written down: (adapter ordinal, rstart, rstop, errors, interval
//                  at match time).  An adapter op whose flag bit no other op of the chain sets, and which the trimming
//                  kernels' result shows unset, did not match: its alignment is skipped.  The walk's final interval
//                  and flags must be what the trimming kernels produced for the record; anything else is reported as
//                  ERR_INFO_MISMATCH and the batch is not formatted.  (For an op skipped that way the flag half of
//                  the comparison holds by construction; the interval half still checks the walk around it.)
//   info_sizes / (text_scan_blocks) / info_offsets   bytes of every record's rows, their place in the stream
//   info_copy      32 lanes per record write the rows
//
// The stream then takes the deflate kernels like a route's stream when the file is a .gz.

namespace csinfo {

using csdev::DevOp;
using csdev::DevPlan;
using cstext::FormatArgs;
using cstext::ReadView;
using cstext::TextParams;

constexpr uint32_t ERR_INFO_MISMATCH = 5;  // CS_TEXT_ERR_INFO_MISMATCH
constexpr uint32_t ERR_INFO_OVERFLOW = 6;  // CS_TEXT_ERR_INFO_OVERFLOW

struct InfoMatch {  // one AdapterCutter match (20 bytes)
  uint32_t s, e;           // the interval of the original read the op searched
  uint32_t rstart, rstop;  // Match.rstart / rstop, relative to s
  uint16_t errors;
  uint8_t name;            // 1-based position of the op among the adapter ops of the chain
  uint8_t _pad;
};

struct InfoRec {
  uint32_t start, stop;  // the walk's final interval
  uint32_t n_matches;
  uint32_t bytes;        // of the record's rows
};

struct InfoMeta {  // what the host reads back per batch
  unsigned long long bytes;     // the table's text
  unsigned long long gz_bytes;  // its gzip member (deflate_layout), 0 for a plain stream
  unsigned long long gz_total;
  unsigned long long rows;
};

struct InfoArgs {
  InfoMatch *match;  // [n][n_adapters]
  InfoRec *rec;      // [n]
  uint32_t *blk;     // block sums of the row bytes, then their exclusive scan
  unsigned long long *total;
  uint32_t *dst;     // [n] byte offset of the record's rows
  uint8_t *out;
  InfoMeta *imeta;
  uint32_t n_adapters;  // adapter ops in mate 1's chain (>= 1 slots per record)
  uint32_t plan_slot;
  uint32_t uniq_flags;  // CS_F_* bits that exactly one adapter op of mate 1's chain sets
  uint32_t no_qual;     // the input has no qualities (FASTA): the quality columns stay empty
  unsigned long long cap;  // bytes `out` holds
};

__device__ __forceinline__ uint32_t dec_width(uint32_t x) {
  uint32_t w = 1;
  while (x >= 10u) {
    x /= 10u;
    ++w;
  }
  return w;
}

// The record's name as the output files carry it -- format_copy's rule: SuffixRemover applied (Rec.hdr_len), the id
// field, '_' and the captured bases when the scheme has a UMI.  With a --rename template (cs_text_set_rename: the
// kernels' trailing RenameTable, as in text_kernels.hip.inc) it is mate 1's name by cstext::name_len / emit_name.
struct NameView {
  const uint8_t *id, *tag1, *tag2;
  uint32_t id_len, t1, t2, tag;
  __device__ __forceinline__ uint32_t len() const { return id_len + tag; }
};

__device__ __forceinline__ NameView name_view(const FormatArgs &a, const TextParams &tp, uint32_t r, const ReadView &r1) {
  NameView n;
  const uint32_t idr = a.idr[0][r];
  n.id_len = idr >> 16;
  n.id = a.text[0] + a.rec[0][r].hdr_off + (idr & 0xffffu);
  n.tag1 = r1.seq + r1.cap_off;
  n.tag2 = nullptr;
  n.t1 = n.t2 = 0;
  if (tp.has_umi) {
    n.t1 = r1.cap_len;
    if (tp.paired) {
      const ReadView r2 = cstext::read_view(a, 1, r);
      n.tag2 = r2.seq + r2.cap_off;
      n.t2 = r2.cap_len;
    } else {
      n.tag2 = r1.seq + r1.cap2_off;
      n.t2 = r1.cap2_len;
    }
  }
  n.tag = tp.has_umi ? 1u + n.t1 + n.t2 : 0u;
  return n;
}

struct Recorder {  // what info_record keeps of a walk: every match, and the bytes of the rows they make
  static constexpr bool kDemux = false;  // (cs_text_create refuses info on a plan with a CS_OP_DEMUX op)
  InfoMatch *mine;
  uint32_t n_adapters, uniq_flags, trimmed_flags, per_base;
  int max_m;  // the adapter length the walk's columns are sized for
  uint32_t ordinal = 0, row_bytes = 0;

  __device__ __forceinline__ bool adapter_runs(const cs_op &op) {
    ++ordinal;
    // the trimming kernels say "this op did not match" where the flag is the op's alone
    const bool known_miss = (op.match_flag & uniq_flags) && !(trimmed_flags & op.match_flag);
    return !known_miss && (int)op.m <= max_m;  // (info_max_m selects the instantiation: the host never lets m exceed it)
  }
  __device__ __forceinline__ void adapter_matched(const cs_op &, const cslong::Walk &w, int rstart, int rstop, int errors) {
    if ((uint32_t)w.n_matches < n_adapters) {
      InfoMatch m;
      m.s = (uint32_t)w.s;
      m.e = (uint32_t)w.e;
      m.rstart = (uint32_t)rstart;
      m.rstop = (uint32_t)rstop;
      m.errors = (uint16_t)errors;
      m.name = (uint8_t)ordinal;
      m._pad = 0;
      mine[w.n_matches] = m;
    }
    row_bytes += 12u + dec_width((uint32_t)errors) + dec_width((uint32_t)rstart) + dec_width((uint32_t)rstop) +
                 dec_width(ordinal) + per_base * (uint32_t)(w.e - w.s);
  }
  __device__ __forceinline__ void cut(const cs_op &, int, int) {}
  __device__ __forceinline__ void quality_trimmed(int) {}
  __device__ __forceinline__ void polya_trimmed(int) {}  // (cutadapt's PolyATrimmer writes no row: the final read narrows)
};

template <int kMaxM, bool ENDS, bool POLYA, class... Rename>
__device__ __forceinline__ void info_record_body(FormatArgs a, TextParams tp, InfoArgs ia, Rename... rn) {
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 64u + threadIdx.x;
  if (r >= a.n) return;
  const DevPlan *plan = &csdev::c_plans[ia.plan_slot];
  const cslong::Env env(plan);
  const cstext::Rec rc = a.rec[0][r];
  const uint32_t slot = a.long_of[0][r];
  const ReadView v = cstext::read_view(a, 0, r);  // what the trimming kernels made of the record
  const uint32_t per_base = ia.no_qual ? 1u : 2u;
  Recorder ev{ia.match + (size_t)r * ia.n_adapters, ia.n_adapters, ia.uniq_flags, v.flags, per_base, kMaxM};
  const cslong::Walk w = cslong::walk_chain<kMaxM, ENDS, POLYA>(plan, 0, env, a.text[0] + rc.seq_off, a.text[0] + rc.qual_off,
                                                   (int)(slot != cstext::kNotLong ? a.lrec[0][slot].len : (uint32_t)rc.len), ev);
  // the table must not disagree with the records next to it
  if ((uint32_t)w.s != v.start || (uint32_t)w.e != v.stop || w.flags != v.flags) cstext::report(a.meta, r, ERR_INFO_MISMATCH);
  uint32_t name_bytes;
  if constexpr (sizeof...(Rename) != 0)
    name_bytes = cstext::name_len(a, 0, r, 0u, v, tp.paired ? cstext::read_view(a, 1, r) : v, rn...);
  else
    name_bytes = name_view(a, tp, r, v).len();
  uint32_t row_bytes = ev.row_bytes;
  if (w.n_matches == 0)
    row_bytes = 7u + per_base * (uint32_t)(w.e - w.s);  // name "\t-1\t" seq '\t' qual "\t\n"
  row_bytes += (uint32_t)max(w.n_matches, 1) * name_bytes;
  InfoRec out;
  out.start = (uint32_t)w.s;
  out.stop = (uint32_t)w.e;
  out.n_matches = (uint32_t)w.n_matches;
  out.bytes = row_bytes;
  ia.rec[r] = out;
}

template <int kMaxM, bool ENDS = false, class... Rename>
__global__ void __launch_bounds__(64) info_record(FormatArgs a, TextParams tp, InfoArgs ia, Rename... rn) {
  info_record_body<kMaxM, ENDS, false>(a, tp, ia, rn...);
}
// the instantiations for plans with a CS_OP_POLYA op (cslong::walk_chain's POLYA walk)
template <int kMaxM, class... Rename>
__global__ void __launch_bounds__(64) info_record_polya(FormatArgs a, TextParams tp, InfoArgs ia, Rename... rn) {
  info_record_body<kMaxM, true, true>(a, tp, ia, rn...);
}

__global__ void __launch_bounds__(256) info_sizes(FormatArgs a, InfoArgs ia) {
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  uint32_t bytes = 0, rows = 0;
  if (r < a.n) {
    const InfoRec ir = ia.rec[r];
    bytes = ir.bytes;
    rows = max(ir.n_matches, 1u);
  }
  uint32_t total, total_rows;
  (void)cstext::block_scan_256(bytes, total, sh);
  (void)cstext::block_scan_256(rows, total_rows, sh);
  if (threadIdx.x == 0) {
    ia.blk[blockIdx.x] = total;
    atomicAdd(&ia.imeta->rows, (unsigned long long)total_rows);
  }
}

__global__ void __launch_bounds__(256) info_offsets(FormatArgs a, InfoArgs ia) {
  __shared__ uint32_t sh[8];
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const uint32_t bytes = r < a.n ? ia.rec[r].bytes : 0u;
  uint32_t total;
  const uint32_t local = cstext::block_scan_256(bytes, total, sh);
  if (r < a.n) ia.dst[r] = ia.blk[blockIdx.x] + local;
  if (blockIdx.x == 0 && threadIdx.x == 0) ia.imeta->bytes = *ia.total;
  // (cs_text_create sizes the stream from the text and the adapter ops; a table beyond it is not written)
  if (threadIdx.x == 0 && *ia.total > ia.cap) cstext::report(a.meta, 0, ERR_INFO_OVERFLOW);
}

template <class... Rename>
__global__ void __launch_bounds__(256) info_copy(FormatArgs a, TextParams tp, InfoArgs ia, Rename... rn) {
  if (a.meta->err != ~0ull) return;
  const uint32_t lane = threadIdx.x & 31u;
  const bool with_qual = ia.no_qual == 0;
  for (unsigned long long it = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) >> 5; it < a.n;
       it += ((unsigned long long)gridDim.x * 256ull) >> 5) {
    const uint32_t r = (uint32_t)it;
    const InfoRec ir = ia.rec[r];
    const cstext::Rec rc = a.rec[0][r];
    const uint8_t *seq = a.text[0] + rc.seq_off, *qual = a.text[0] + rc.qual_off;
    const ReadView v = cstext::read_view(a, 0, r);
    const NameView nm = name_view(a, tp, r, v);
    uint8_t *out = ia.out + ia.dst[r];
    uint32_t pos = 0;
    auto copy = [&](const uint8_t *src, uint32_t n) {
      for (uint32_t i = lane; i < n; i += 32u) out[pos + i] = src[i];
      pos += n;
    };
    auto byte = [&](uint8_t c) {
      if (lane == 0) out[pos] = c;
      ++pos;
    };
    auto dec = [&](uint32_t x) {
      const uint32_t w = dec_width(x);
      if (lane < w) {
        uint32_t y = x;
        for (uint32_t i = lane + 1u; i < w; ++i) y /= 10u;
        out[pos + lane] = (uint8_t)('0' + y % 10u);
      }
      pos += w;
    };
    auto name = [&]() {
      if constexpr (sizeof...(Rename) != 0) {
        const ReadView r2 = tp.paired ? cstext::read_view(a, 1, r) : v;
        cstext::emit_name(a, rn..., 0, r, v, r2, out + pos, lane);
        pos += cstext::name_len(a, 0, r, 0u, v, r2, rn...);
      } else {
        copy(nm.id, nm.id_len);
        if (nm.tag) {
          byte('_');
          copy(nm.tag1, nm.t1);
          copy(nm.tag2, nm.t2);
        }
      }
    };
    if (ir.n_matches == 0) {
      // name, -1, the final sequence, the final qualities, an empty column
      const uint32_t L = ir.stop - ir.start;
      const bool rcomp = tp.reverse_complement && !tp.paired;
      name();
      byte('\t');
      byte('-');
      byte('1');
      byte('\t');
      if (!rcomp) {
        copy(seq + ir.start, L);
      } else {
        for (uint32_t i = lane; i < L; i += 32u) out[pos + i] = cstext::complement(seq[ir.stop - 1u - i]);
        pos += L;
      }
      byte('\t');
      if (with_qual) {
        if (!rcomp) {
          copy(qual + ir.start, L);
        } else {
          for (uint32_t i = lane; i < L; i += 32u) out[pos + i] = qual[ir.stop - 1u - i];
          pos += L;
        }
      }
      byte('\t');
      byte('\n');
      continue;
    }
    const InfoMatch *mine = ia.match + (size_t)r * ia.n_adapters;
    for (uint32_t k = 0; k < min(ir.n_matches, ia.n_adapters); ++k) {
      const InfoMatch m = mine[k];
      const uint32_t n = m.e - m.s;
      name();
      byte('\t');
      dec(m.errors);
      byte('\t');
      dec(m.rstart);
      byte('\t');
      dec(m.rstop);
      byte('\t');
      copy(seq + m.s, m.rstart);
      byte('\t');
      copy(seq + m.s + m.rstart, m.rstop - m.rstart);
      byte('\t');
      copy(seq + m.s + m.rstop, n - m.rstop);
      byte('\t');
      dec(m.name);
      byte('\t');
      if (with_qual) copy(qual + m.s, m.rstart);
      byte('\t');
      if (with_qual) copy(qual + m.s + m.rstart, m.rstop - m.rstart);
      byte('\t');
      if (with_qual) copy(qual + m.s + m.rstop, n - m.rstop);
      byte('\t');
      byte('\n');
    }
  }
}

}  // namespace csinfo
