// long_kernel.hip.inc -- the op chain for reads that do not fit the rows of the tile kernels (device code only).
// Included by cutseq_hip.hip behind trim_kernel.hip.inc.  gfx950 / wave64 only.
//
// The reference streams records of any length through dnaio and cutadapt (cutseq/run.py:434-441, 751-758); the tile
// kernels stage 64 reads of at most CS_MAX_STRIDE bases in LDS.  In the text path a read longer than the batch's row
// stride is therefore taken out of the rows (its length slot holds CS_LEN_SKIP, the tile kernels pass over it) and
// walks the whole chain here, straight from the uploaded text: one lane per long read, cutadapt's Aligner.locate
// column by column with three-int cells (costs, scores and origins of a 100 kb read do not fit the packed cells of
// the tile kernels), Ukkonen's cut-off, candidate selection in column order, then the rows of the last column --
// SURVEY.md appendix B.2 statement for statement; cutters, demultiplexing, quality trimming and the filters as in
// trim_kernel.  Long reads are rare in the libraries cutseq is used on: this kernel is exact, not fast
// (a 20 kb read costs its lane a few million instructions per adapter op).
//
// walk_chain is that scalar walk, once: long_kernel calls it for the long reads of either mate, info_record
// (info_kernels.hip.inc) for every record of mate 1.  What a caller does beyond the interval and the flags -- statistics,
// captures and demultiplexing here, the match table there -- lives in the events object it passes in.

namespace cslong {

using csdev::DevOp;
using csdev::DevPlan;

struct LongRec {  // one long read of one mate
  uint32_t rec;       // record index inside the batch
  uint32_t seq_off;   // byte offsets into the batch's text
  uint32_t qual_off;
  uint32_t len;
};

struct LongRes {  // its result: cs_result + cs_cap2 with 32-bit positions
  uint32_t start, stop, cap_off, cap2_off;
  uint8_t cap_len, cap2_len, flags, bc;
  uint8_t xflags, _pad[3];  // CS_X_* (TooLong, TooManyN, TooManyExpectedErrors)
};

struct Env {  // the plan's aligner settings
  int rule;
  bool tie_ins, fold, coded;
  __device__ explicit Env(const DevPlan *plan)
      : rule(plan->params.select_rule), tie_ins(plan->params.indel_tie == CS_TIE_INSERTION),
        fold(plan->params.case_rule == CS_CASE_FOLD), coded(plan->coded != 0) {}
};

__device__ __forceinline__ uint32_t query_code(uint8_t c, bool coded, bool fold) {
  if (fold && c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
  return coded ? csdev::base_code(c) : (uint32_t)c;
}

// cutadapt Aligner.locate on query = text[q0 + s, q0 + e) (walked backwards for the rightmost variant).  kMaxM bounds
// the adapter length the three columns are sized for (the caller vouches for op.m <= kMaxM); `errors` receives the
// cost of the selected candidate (Match.errors).
template <int kMaxM>
__device__ __forceinline__ bool locate_sized(const DevOp &d, const Env &v, const uint8_t *q, int n, int &qs, int &qe,
                                             int &errors) {
  const cs_op &op = d.op;
  const int rule = v.rule;
  const bool tie_ins = v.tie_ins;
  const int m = op.m, k = op.k, flags = op.align_flags, min_overlap = op.min_overlap;
  const bool RS = flags & CS_REF_START, QS = flags & CS_QUERY_START;
  const bool RE = flags & CS_REF_END, QSTOP = flags & CS_QUERY_STOP;
  const bool reversed = op.reversed;
  int ccost[kMaxM + 1], cscore[kMaxM + 1], corigin[kMaxM + 1];
  int min_n, max_n;
  csdev::column_range(flags, m, k, n, min_n, max_n);
  for (int i = 0; i <= m; ++i) {
    cscore[i] = 0;
    if (!RS && !QS) {
      ccost[i] = max(i, min_n);
      corigin[i] = 0;
    } else if (RS && !QS) {
      ccost[i] = min_n;
      corigin[i] = min(0, min_n - i);
    } else if (!RS && QS) {
      ccost[i] = i;
      corigin[i] = max(0, min_n - i);
    } else {
      ccost[i] = min(i, min_n);
      corigin[i] = min_n - i;
    }
  }
  bool have = false;
  int b_origin = 0, b_cost = 0, b_score = 0, b_refstop = m, b_qstop = n;
  int last = RS ? m : min(m, k + 1);
  for (int j = min_n + 1; j <= max_n; ++j) {
    int dcost = ccost[0], dscore = cscore[0], dorigin = corigin[0];
    if (QS)
      corigin[0] = j;
    else
      ccost[0] = j;
    const uint32_t qc = query_code(q[reversed ? n - j : j - 1], v.coded, v.fold);
    for (int i = 1; i <= last; ++i) {
      int cost, score, origin;
      if ((uint32_t)op.seq[i - 1] == qc) {
        cost = dcost;
        origin = dorigin;
        score = dscore + 1;
      } else {
        const int cd = dcost + 1, cdel = ccost[i] + 1, cins = ccost[i - 1] + 1;
        if (cd <= cdel && cd <= cins) {
          cost = cd;
          origin = dorigin;
          score = dscore - 1;
        } else if (tie_ins ? cins <= cdel : cins < cdel) {
          cost = cins;
          origin = corigin[i - 1];
          score = cscore[i - 1] - 2;
        } else {
          cost = cdel;
          origin = corigin[i];
          score = cscore[i] - 2;
        }
      }
      dcost = ccost[i];
      dscore = cscore[i];
      dorigin = corigin[i];
      ccost[i] = cost;
      cscore[i] = score;
      corigin[i] = origin;
    }
    while (last >= 0 && ccost[last] > k) --last;
    if (last < m) {
      ++last;
    } else if (QSTOP) {
      const int cost = ccost[m], score = cscore[m], origin = corigin[m];
      const int length = m + min(origin, 0);
      const bool ok = length >= min_overlap && cost <= (int)op.thr[max(length, 0)];
      const int b_length = m + min(b_origin, 0);
      if (ok && csdev::better_candidate(rule, m, have, b_origin, b_cost, b_score, b_length, cost, score, origin, length)) {
        have = true;
        b_origin = origin;
        b_cost = cost;
        b_score = score;
        b_refstop = m;
        b_qstop = j;
        if (cost == 0 && origin >= 0) break;
      }
    }
  }
  if (max_n == n) {
    const int first_i = RE ? 0 : m;
    // (after an early break this loop still runs in cutadapt, on the column the break left behind; an exact
    // full-length hit scores m and no row can replace it -- kept literal all the same)
    for (int i = m; i >= first_i; --i) {
      const int cost = ccost[i], score = cscore[i], origin = corigin[i];
      const int length = i + min(origin, 0);
      const bool ok = length >= min_overlap && length >= 0 && cost <= (int)op.thr[max(length, 0)];
      const int b_length = b_refstop + min(b_origin, 0);
      if (ok && csdev::better_candidate(rule, m, have, b_origin, b_cost, b_score, b_length, cost, score, origin, length)) {
        have = true;
        b_origin = origin;
        b_cost = cost;
        b_score = score;
        b_refstop = i;
        b_qstop = n;
      }
    }
  }
  if (!have) return false;
  qs = b_origin >= 0 ? b_origin : 0;
  qe = b_qstop;
  errors = b_cost;
  return true;
}

// cutadapt <= 2.x (CS_SHORTCUT_FIND): str.find on the query as the aligner sees it
__device__ __forceinline__ bool find_exact(const cs_op &op, const Env &v, const uint8_t *q, int n, int &qs, int &qe) {
  for (int p = 0; p + (int)op.m <= n; ++p) {
    int i = 0;
    for (; i < (int)op.m; ++i)
      if (query_code(q[op.reversed ? n - 1 - (p + i) : p + i], v.coded, v.fold) != (uint32_t)op.seq[i]) break;
    if (i == (int)op.m) {
      qs = p;
      qe = p + op.m;
      return true;
    }
  }
  return false;
}

// cutadapt quality_trim_index, the 3' walk on qual[0, n): BWA running sum from the 3' end, first strict maximum.
// A term is at most 256 in size (cs_plan_create clamps the cutoff), a read at most CS_MAX_READ = 2^24 bases: the sum
// reaches 2^32, so it is a 64-bit sum.
__device__ __forceinline__ int quality_stop(const cs_op &op, const uint8_t *qual, int n) {
  long long sum = 0, best = 0;
  int stop = n;
  for (int i = n - 1; i >= 0; --i) {
    sum += (int)op.q_cutoff - ((int)qual[i] - (int)op.q_base);
    if (sum < 0) break;
    if (sum > best) {
      best = sum;
      stop = i;
    }
  }
  return stop;
}

// ... and its 5' walk (cs_op.q_cutoff_front != 0 only): forward over the same qual[0, n), whatever the 3' walk decided;
// start = one behind the first strict maximum.  The same terms, the same 64-bit sum.
__device__ __forceinline__ int quality_start(const cs_op &op, const uint8_t *qual, int n) {
  long long sum = 0, best = 0;
  int start = 0;
  for (int i = 0; i < n; ++i) {
    sum += (int)op.q_cutoff_front - ((int)qual[i] - (int)op.q_base);
    if (sum < 0) break;
    if (sum > best) {
      best = sum;
      start = i + 1;
    }
  }
  return start;
}

// cutadapt nextseq_trim_index (CS_OP_NEXTSEQ) on seq[0, n) / qual[0, n): quality_stop's walk in which a 'G' (upper case
// only) adds 1 whatever its quality byte says.  The terms are within the same bound (cs_plan_create refuses a cutoff
// outside the range it clamps CS_OP_QTRIM's to), the sum is the same 64-bit sum.
__device__ __forceinline__ int quality_stop_nextseq(const cs_op &op, const uint8_t *seq, const uint8_t *qual, int n) {
  long long sum = 0, best = 0;
  int stop = n;
  for (int i = n - 1; i >= 0; --i) {
    sum += seq[i] == 0x47u ? 1 : (int)op.q_cutoff - ((int)qual[i] - (int)op.q_base);
    if (sum < 0) break;
    if (sum > best) {
      best = sum;
      stop = i;
    }
  }
  return stop;
}

// cutadapt poly_a_trim_index (CS_OP_POLYA) on seq[0, n): how many bases stay -- of the front for the tail form, of the
// back for the head form (`head`: poly-T, walked from the 5' end).  The loop of include/cutseq_hip.h with the error
// count folded into the score (errors * 5 <= l  <=>  5 * score >= 2 * l) and its two exits: no later position can beat
// the best score, or qualify.  |score| <= 2 * CS_MAX_READ = 2^25: an int.
__device__ __forceinline__ int polya_keep(const uint8_t *seq, int n, bool head) {
  static_assert(5ll * 3 * CS_MAX_READ < (1ll << 31), "polya_keep: 5 * (score + bases left) in an int");
  const uint8_t match = head ? 0x54u : 0x41u;
  int score = 0, best = 0, index = n;
  for (int l = 1; l <= n; ++l) {  // l: the candidate's length
    score += seq[head ? l - 1 : n - l] == match ? 1 : -2;
    if (score > best && 5 * score >= 2 * l) {
      best = score;
      index = n - l;
    }
    const int reach = score + (n - l);  // the score of the whole rest matching
    if (reach <= best || 5 * reach < 2 * n) break;
  }
  return index > n - 3 ? n : index;  // tails shorter than 3 are ignored
}

// Where a demultiplexing table keeps the first `depth` bases of q[0, n) -- read from the 5' end, or backwards from the
// 3' end -- : the block of the prefixes of min(n, depth) bases, then the prefix in base 5 (A, C, G, T, anything else).
__device__ __forceinline__ uint32_t prefix_index(const uint8_t *q, int n, int depth, bool from_end, bool fold) {
  const int take = min(n, depth);
  uint32_t idx = 0, pw = 1, block = 0;
  for (int u = 0; u < depth; ++u) {
    if (u < take) {
      uint8_t ch = q[from_end ? n - 1 - u : u];
      if (fold && ch >= 'a' && ch <= 'z') ch = (uint8_t)(ch - 32);
      const uint32_t digit = (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') ? (((uint32_t)ch >> 1) & 3u) : 4u;
      idx += digit * pw;
      block += pw;
    }
    pw *= 5u;
  }
  return block + idx;
}

struct Walk {  // a read on its way through the chain
  int s, e;  // the interval that is left of it
  uint32_t flags;
  int n_matches;
};

// One mate's op chain on one read, straight from its text.  kMaxM sizes the aligner's columns.  `ev` is the caller's:
//   bool adapter_runs(op)      in front of an adapter op; false: the caller knows it does not match, nothing is aligned
//   adapter_matched(op, w, rstart, rstop, errors)   the match, `w` still as the op found it
//   cut(op, off, c)            a cutter took c bases at off
//   quality_trimmed(k)         the quality trimmer took k bases
//   demux(d, v, seq, w)        a CS_OP_DEMUX op, the caller's to apply (Events::kDemux; compiled out where false)
//   polya_trimmed(k)           a CS_OP_POLYA op took k bases (POLYA instantiations only)
// ENDS: the instantiation for plans with a front cutoff, a CS_OP_NTRIM, CS_OP_NEXTSEQ or CS_OP_SHORTEN op (cs_engine::ends), the only
// one that holds their code; every other plan runs the walk it ran before they came.  POLYA: likewise for plans with a
// CS_OP_POLYA op (cs_engine::polya); it comes with ENDS, whose walk is the one that knows every op.
template <int kMaxM, bool ENDS, bool POLYA = false, class Events>
__device__ __forceinline__ Walk walk_chain(const DevPlan *plan, int mate, const Env &v, const uint8_t *seq, const uint8_t *qual,
                                           int len, Events &ev) {
  Walk w = {0, len, 0u, 0};
  const int n_ops = plan->n_ops[mate];
  for (int t = 0; t < n_ops; ++t) {
    const DevOp &d = plan->ops[mate][t];
    const cs_op &op = d.op;
    const int n = w.e - w.s;
    if (op.kind == CS_OP_ADAPTER) {
      int qs = 0, qe = 0, errors = 0;
      bool hit = false;
      if (ev.adapter_runs(op)) {
        hit = op.shortcut == CS_SHORTCUT_FIND && find_exact(op, v, seq + w.s, n, qs, qe);
        if (!hit) hit = locate_sized<kMaxM>(d, v, seq + w.s, n, qs, qe, errors);
      }
      if (hit) {
        int rstart = qs, rstop = qe;
        if (op.reversed) {  // RightmostFrontAdapter.match_to: back to forward coordinates
          rstart = n - qe;
          rstop = n - qs;
        }
        ev.adapter_matched(op, w, rstart, rstop, errors);
        ++w.n_matches;
        w.flags |= op.match_flag;
        if (op.remove == CS_REMOVE_BEFORE)
          w.s += rstop;
        else
          w.e = w.s + rstart;
      } else if (op.required) {
        w.flags |= CS_F_UNTRIMMED;
      }
    } else if (op.kind == CS_OP_CUT) {
      if (op.conditional && w.n_matches == 0 && n < (int)op.force_min_len) continue;
      if (op.cut_len == 0) continue;
      int c, off;
      if (op.cut_len > 0) {
        c = min((int)op.cut_len, n);
        off = w.s;
        w.s += c;
      } else {
        c = min(-(int)op.cut_len, n);
        off = w.e - c;
        w.e -= c;
      }
      ev.cut(op, off, c);
    } else if (op.kind == CS_OP_DEMUX) {
      if constexpr (Events::kDemux) ev.demux(d, v, seq, w);
    } else if (op.kind == CS_OP_QTRIM) {
      int stop = quality_stop(op, qual + w.s, n), start = 0;
      if constexpr (ENDS) {
        if (op.q_cutoff_front != 0) {  // cutadapt -q FRONT,BACK; 0: the reference's op, no front walk
          start = quality_start(op, qual + w.s, n);
          if (start >= stop) start = stop = 0;  // the two walks crossed: nothing is left, reported as [s, s)
        }
      }
      if (stop - start < n) w.flags |= CS_F_QTRIMMED;
      ev.quality_trimmed(n - (stop - start));
      w.e = w.s + stop;
      w.s += start;
    } else if (op.kind == CS_OP_NEXTSEQ) {  // cutadapt's NextseqQualityTrimmer: the 3' walk that sees through 'G'
      if constexpr (ENDS) {
        const int stop = quality_stop_nextseq(op, seq + w.s, qual + w.s, n);
        if (stop < n) w.flags |= CS_F_QTRIMMED;
        ev.quality_trimmed(n - stop);
        w.e = w.s + stop;
      }
    } else if (op.kind == CS_OP_POLYA) {  // cutadapt's PolyATrimmer: the tail (reversed: the poly-T head) goes
      if constexpr (POLYA) {
        const int keep = polya_keep(seq + w.s, n, op.reversed != 0);
        ev.polya_trimmed(n - keep);
        if (op.reversed)
          w.s = w.e - keep;
        else
          w.e = w.s + keep;
      }
    } else if (op.kind == CS_OP_SHORTEN) {  // cutadapt's Shortener: min(n, |length|) bases stay, first or (< 0) last ones
      if constexpr (ENDS) {
        // 32 bits against 32 bits: intervals here exceed 16 bits, and |INT32_MIN| exists as an unsigned value only
        const int32_t length = op.length;
        const int keep = (int)min((uint32_t)n, length < 0 ? 0u - (uint32_t)length : (uint32_t)length);
        if (length >= 0)
          w.e = w.s + keep;
        else
          w.s = w.e - keep;
      }
    } else if (op.kind == CS_OP_NTRIM) {  // cutadapt's NEndTrimmer: the runs of 'N' (upper case only) at both ends
      if constexpr (ENDS) {
        int lead = 0;
        while (lead < n && seq[w.s + lead] == 0x4Eu) ++lead;
        if (lead == n) {
          w.e = w.s;
        } else {
          while (seq[w.e - 1] == 0x4Eu) --w.e;
          w.s += lead;
        }
      }
    }
  }
  if (w.e - w.s < (int)plan->params.min_length) w.flags |= CS_F_TOO_SHORT;
  return w;
}

struct LongArgs {
  const uint8_t *text;
  const LongRec *rec;
  LongRes *res;
  const uint32_t *n_long;      // how many of them (device side: the record kernel counts)
  uint32_t cap;                // capacity of rec / res
  unsigned long long *stats;   // this mate's cs_stats block (u64 words)
  unsigned long long *xstats;  // this mate's csdev::XST_* words behind the two cs_stats
  uint32_t plan_slot;
  int mate;
  const unsigned long long *gate;
};

struct LongEvents {  // what long_kernel keeps of a walk besides the interval and the flags
  static constexpr bool kDemux = true;
  unsigned long long *stats;
  uint32_t bc = CS_DEMUX_NONE, cap_off = 0, cap_len = 0, cap2_off = 0, cap2_len = 0, qtrimmed = 0;
  uint32_t polya = 0;  // (POLYA instantiation only; no other walk calls polya_trimmed)

  __device__ __forceinline__ bool adapter_runs(const cs_op &) const { return true; }
  __device__ __forceinline__ void adapter_matched(const cs_op &op, const Walk &, int, int, int) {
    atomicAdd(&stats[csdev::ST_OPS + op.stat_slot], 1ull);
  }
  __device__ __forceinline__ void cut(const cs_op &op, int off, int c) {
    // (selects, not branches: stores to one capture or the other become one store through a selected address, and
    // that keeps all four words in scratch)
    const bool one = op.capture == 1, two = op.capture == 2;
    cap_off = one ? (uint32_t)off : cap_off;
    cap_len = one ? (uint32_t)c : cap_len;
    cap2_off = two ? (uint32_t)off : cap2_off;
    cap2_len = two ? (uint32_t)c : cap2_len;
  }
  __device__ __forceinline__ void quality_trimmed(int k) { qtrimmed += (uint32_t)k; }
  __device__ __forceinline__ void polya_trimmed(int k) { polya += (uint32_t)k; }

  __device__ __forceinline__ void demux(const DevOp &d, const Env &v, const uint8_t *seq, Walk &w) {
    const cs_op &op = d.op;
    const int s = w.s, n = w.e - w.s;
    const bool at_end = d.filter_mode && op.reversed != 0;  // barcodes at the 3' end: SuffixAdapter ops
    uint32_t id = CS_DEMUX_NONE;
    int cut = 0;
    bool ambiguous = false;
    if (d.filter_mode) {
      // the barcodes' own ops (cs_plan_set_demux_ops): candidates from the table over the first bases, each one's
      // PrefixAdapter located on the read, the outcomes merged as in trim_kernel
      const uint32_t *first = reinterpret_cast<const uint32_t *>((uintptr_t)d.peq[0]);
      const uint8_t *pool = reinterpret_cast<const uint8_t *>((uintptr_t)d.peq[1]);
      const DevOp *bops = reinterpret_cast<const DevOp *>((uintptr_t)d.peq[2]);
      const uint32_t ent = first[prefix_index(seq + s, n, (int)d.peq[3], at_end, v.fold)];
      const uint32_t cnt = ent & 0xffu, off = ent >> 8;
      uint32_t hits = 0;
      bool exact_taken = false;
      const int mb = (int)op.m;
      for (uint32_t ci = 0; ci < cnt; ++ci) {
        const uint32_t b = pool[off + ci];
        const DevOp &bd = bops[b];
        int qs = 0, qe = 0, errors;
        if (!locate_sized<CS_MAX_ADAPTER>(bd, v, seq + s, n, qs, qe, errors)) continue;
        bool exact = n >= mb && (at_end ? qs == n - mb : qe == mb);
        for (int i = 0; exact && i < mb; ++i)
          exact = query_code(seq[at_end ? s + n - mb + i : s + i], v.coded, v.fold) == (uint32_t)bd.op.seq[i];
        if (id == CS_DEMUX_NONE || (exact && !exact_taken)) {
          id = b;
          cut = at_end ? qs : qe;
        }
        exact_taken = exact_taken || exact;
        ++hits;
      }
      ambiguous = hits > 1u;
    } else {  // the table over every prefix of m + k bases: barcode, bases to remove, "several barcodes claim it"
      const uint16_t *table = reinterpret_cast<const uint16_t *>((uintptr_t)d.peq[0]);
      const uint32_t entry = table[prefix_index(seq + s, n, (int)op.m + (int)op.k, false, v.fold)];
      if ((entry & 0xffu) != CS_DEMUX_NONE) id = entry & 0xffu;
      cut = (int)((entry >> 8) & 0xfu);
      ambiguous = (entry & 0x4000u) != 0;
    }
    if (id != CS_DEMUX_NONE) {
      if (at_end)
        w.e = s + cut;  // SuffixAdapter: RemoveAfterMatch
      else
        w.s += cut;
      ++w.n_matches;
      w.flags |= op.match_flag;
      atomicAdd(&stats[csdev::ST_OPS + op.stat_slot], 1ull);
      if (ambiguous) w.flags |= CS_F_AMBIGUOUS;
      bc = id;
    } else if (op.required) {
      w.flags |= CS_F_UNTRIMMED;
    }
  }
};

// MORE: the instantiation that also decides TooLong and TooManyExpectedErrors (plans with cs_plan_set_max_length or
// cs_plan_set_max_ee); every other plan runs the kernel it ran before those filters came.
// POLYA: the walk that knows CS_OP_POLYA, and its counter.
template <bool MORE, bool ENDS, bool POLYA>
__device__ __forceinline__ void long_body(LongArgs a) {
  if (a.gate && *a.gate != ~0ull) return;
  const DevPlan *plan = &csdev::c_plans[a.plan_slot];
  const Env v(plan);
  const uint32_t total = min(*a.n_long, a.cap);
  for (uint32_t it = blockIdx.x * 64u + threadIdx.x; it < total; it += gridDim.x * 64u) {
    const LongRec lr = a.rec[it];
    const uint8_t *seq = a.text + lr.seq_off;
    LongEvents ev{a.stats};
    const Walk w = walk_chain<CS_MAX_ADAPTER, ENDS, POLYA>(plan, a.mate, v, seq, a.text + lr.qual_off, (int)lr.len, ev);
    uint32_t xflags = 0;
    if (plan->max_n_on) {  // TooManyN on the final interval: the read's own bytes, up to CS_MAX_READ of them
      uint32_t nn = 0;
      for (int i = w.s; i < w.e; ++i) nn += (seq[i] | 0x20u) == 'n' ? 1u : 0u;
      if (csdev::too_many_n(nn, w.e - w.s, plan->max_n)) {
        xflags = CS_X_TOO_MANY_N;
        atomicAdd(&a.stats[csdev::ST_TOO_MANY_N], 1ull);
      }
    }
    if constexpr (MORE) {
      if (plan->max_length_on && w.e > w.s && (uint32_t)(w.e - w.s) > plan->max_length) {  // TooLong
        xflags |= CS_X_TOO_LONG;
        atomicAdd(&a.xstats[csdev::XST_TOO_LONG], 1ull);
      }
      if (plan->max_ee_on) {  // TooManyExpectedErrors: the same left-to-right double sum as csdev::expected_errors
        const uint8_t *qual = a.text + lr.qual_off;
        double ee = 0.0;
        if (!plan->ee_reversed)
          for (int i = w.s; i < w.e; ++i) ee += plan->ee_table[qual[i]];
        else  // (cs_plan_set_ee_reversed)
          for (int i = w.e - 1; i >= w.s; --i) ee += plan->ee_table[qual[i]];
        if (ee > plan->max_ee) {
          xflags |= CS_X_TOO_MANY_EE;
          atomicAdd(&a.xstats[csdev::XST_TOO_MANY_EE], 1ull);
        }
      }
    }
    LongRes r;
    r.start = (uint32_t)w.s;
    r.stop = (uint32_t)w.e;
    r.cap_off = ev.cap_off;
    r.cap2_off = ev.cap2_off;
    r.cap_len = (uint8_t)ev.cap_len;
    r.cap2_len = (uint8_t)ev.cap2_len;
    r.flags = (uint8_t)w.flags;
    r.bc = (uint8_t)ev.bc;
    r.xflags = (uint8_t)xflags;
    r._pad[0] = r._pad[1] = r._pad[2] = 0;
    a.res[it] = r;
    atomicAdd(&a.stats[csdev::ST_READS], 1ull);
    atomicAdd(&a.stats[csdev::ST_IN_BP], (unsigned long long)lr.len);
    atomicAdd(&a.stats[csdev::ST_OUT_BP], (unsigned long long)(w.e - w.s));
    atomicAdd(&a.stats[csdev::ST_QTRIM_BP], (unsigned long long)ev.qtrimmed);
    if (w.flags & CS_F_TOO_SHORT) atomicAdd(&a.stats[csdev::ST_TOO_SHORT], 1ull);
    if (w.flags & CS_F_UNTRIMMED) atomicAdd(&a.stats[csdev::ST_UNTRIMMED], 1ull);
    if constexpr (POLYA) {  // (the mate's word behind both mates' XST_* words, reached from this mate's)
      unsigned long long *polya = a.xstats + (2 - a.mate) * csdev::kXStatWords + a.mate;
      if (ev.polya) atomicAdd(polya, (unsigned long long)ev.polya);
    }
  }
}

template <bool MORE, bool ENDS = false>
__global__ void __launch_bounds__(64) long_kernel(LongArgs a) {
  long_body<MORE, ENDS, false>(a);
}
// the instantiation for plans with a CS_OP_POLYA op: every filter, every read-end op, and that op
__global__ void __launch_bounds__(64) long_kernel_polya(LongArgs a) { long_body<true, true, true>(a); }

}  // namespace cslong
