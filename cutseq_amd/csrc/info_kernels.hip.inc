// info_kernels.hip.inc -- cutadapt's --info-file on the device: which adapter matched where, read by read (device code
// only).  Included by cutseq_hip.hip behind text_kernels.hip.inc.  gfx950 / wave64 only.
//
// The reference marks the table as a TODO in front of its TooShort step (cutseq/run.py: "# TODO: report info",
// PairedSingleEndStep(InfoFileWriter(...))): one row per adapter match of read 1, one "-1" row for a read without a
// match, every input record, input order.  The trimming kernels keep the surviving interval and eight flag bits per
// read; where an op matched and with how many errors is lost.  Nothing here runs unless cs_text_params.info asks:
//
//   info_record    one lane per record of mate 1: the op chain once more, straight from the uploaded text (any read
//                  length), with Aligner.locate as the long-read kernel restates it -- its columns sized by the plan's
//                  longest adapter -- and every match written down: (adapter ordinal, rstart, rstop, errors, interval
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
// field, '_' and the captured bases when the scheme has a UMI.
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

template <int kMaxM>
__global__ void __launch_bounds__(64) info_record(FormatArgs a, TextParams tp, InfoArgs ia) {
  if (a.meta->err != ~0ull) return;
  const uint32_t r = blockIdx.x * 64u + threadIdx.x;
  if (r >= a.n) return;
  const DevPlan *plan = &csdev::c_plans[ia.plan_slot];
  const int n_ops = plan->n_ops[0];
  const int rule = plan->params.select_rule;
  const bool tie_ins = plan->params.indel_tie == CS_TIE_INSERTION;
  const bool fold = plan->params.case_rule == CS_CASE_FOLD;
  const bool coded = plan->coded != 0;
  const cstext::Rec rc = a.rec[0][r];
  const uint32_t slot = a.long_of[0][r];
  const uint8_t *seq = a.text[0] + rc.seq_off, *qual = a.text[0] + rc.qual_off;
  const ReadView v = cstext::read_view(a, 0, r);  // what the trimming kernels made of the record
  InfoMatch *mine = ia.match + (size_t)r * ia.n_adapters;
  int s = 0, e = (int)(slot != cstext::kNotLong ? a.lrec[0][slot].len : (uint32_t)rc.len), n_matches = 0;
  uint32_t flags = 0, ordinal = 0, row_bytes = 0;
  const uint32_t per_base = ia.no_qual ? 1u : 2u;
  for (int t = 0; t < n_ops; ++t) {
    const DevOp &d = plan->ops[0][t];
    const cs_op &op = d.op;
    const int n = e - s;
    if (op.kind == CS_OP_ADAPTER) {
      ++ordinal;
      int qs = 0, qe = 0, errors = 0;
      bool hit = false;
      // the trimming kernels say "this op did not match" where the flag is the op's alone
      const bool known_miss = (op.match_flag & ia.uniq_flags) && !(v.flags & op.match_flag);
      if (!known_miss && (int)op.m <= kMaxM) {
        if (op.shortcut == CS_SHORTCUT_FIND) {
          for (int p = 0; p + (int)op.m <= n && !hit; ++p) {
            int i = 0;
            for (; i < (int)op.m; ++i)
              if (cslong::query_code(seq[s + (op.reversed ? n - 1 - (p + i) : p + i)], coded, fold) != (uint32_t)op.seq[i]) break;
            if (i == (int)op.m) {
              hit = true;
              qs = p;
              qe = p + op.m;
            }
          }
        }
        if (!hit) hit = cslong::locate_sized<kMaxM>(d, coded, fold, rule, tie_ins, seq + s, n, qs, qe, errors);
      }
      if (hit) {
        int rstart = qs, rstop = qe;
        if (op.reversed) {  // RightmostFrontAdapter.match_to: back to forward coordinates
          rstart = n - qe;
          rstop = n - qs;
        }
        if ((uint32_t)n_matches < ia.n_adapters) {
          InfoMatch m;
          m.s = (uint32_t)s;
          m.e = (uint32_t)e;
          m.rstart = (uint32_t)rstart;
          m.rstop = (uint32_t)rstop;
          m.errors = (uint16_t)errors;
          m.name = (uint8_t)ordinal;
          m._pad = 0;
          mine[n_matches] = m;
        }
        row_bytes += 12u + dec_width((uint32_t)errors) + dec_width((uint32_t)rstart) + dec_width((uint32_t)rstop) +
                     dec_width(ordinal) + per_base * (uint32_t)n;
        ++n_matches;
        flags |= op.match_flag;
        if (op.remove == CS_REMOVE_BEFORE)
          s += rstop;
        else
          e = s + rstart;
      } else if (op.required) {
        flags |= CS_F_UNTRIMMED;
      }
    } else if (op.kind == CS_OP_CUT) {
      if (op.conditional && n_matches == 0 && n < (int)op.force_min_len) continue;
      if (op.cut_len > 0)
        s += min((int)op.cut_len, n);
      else if (op.cut_len < 0)
        e -= min(-(int)op.cut_len, n);
    } else if (op.kind == CS_OP_QTRIM) {
      int sum = 0, best = 0, stop = n;
      for (int i = n - 1; i >= 0; --i) {
        sum += (int)op.q_cutoff - ((int)qual[s + i] - (int)op.q_base);
        if (sum < 0) break;
        if (sum > best) {
          best = sum;
          stop = i;
        }
      }
      if (stop < n) flags |= CS_F_QTRIMMED;
      e = s + stop;
    }
    // (CS_OP_DEMUX: cs_text_create refuses info on such a plan)
  }
  if (e - s < (int)plan->params.min_length) flags |= CS_F_TOO_SHORT;
  // the table must not disagree with the records next to it
  if ((uint32_t)s != v.start || (uint32_t)e != v.stop || flags != v.flags) cstext::report(a.meta, r, ERR_INFO_MISMATCH);
  const NameView nm = name_view(a, tp, r, v);
  if (n_matches == 0)
    row_bytes = 7u + per_base * (uint32_t)(e - s);  // name "\t-1\t" seq '\t' qual "\t\n"
  row_bytes += (uint32_t)max(n_matches, 1) * nm.len();
  InfoRec out;
  out.start = (uint32_t)s;
  out.stop = (uint32_t)e;
  out.n_matches = (uint32_t)n_matches;
  out.bytes = row_bytes;
  ia.rec[r] = out;
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

__global__ void __launch_bounds__(256) info_copy(FormatArgs a, TextParams tp, InfoArgs ia) {
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
      copy(nm.id, nm.id_len);
      if (nm.tag) {
        byte('_');
        copy(nm.tag1, nm.t1);
        copy(nm.tag2, nm.t2);
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
