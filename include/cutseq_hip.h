/*
 * cutseq_hip.h -- C ABI of the MI355X-native trimming engine (libcutseq_hip.so).
 *
 * The reference (y9c/cutseq) has no FFI: its hot path sits behind cutadapt's Python
 * operator API.  This header is the boundary a maintainer binds
 * with ctypes instead; every entry point names the reference interface it replaces
 * (paths relative to the reference tree).  Plain pointers and sizes only, no
 * exceptions, no Python/torch types.  Return value: 0 = ok, negative = cs_status;
 * cs_last_error() gives the thread-local message.
 *
 * Data contract
 *   A batch is a structure-of-arrays of reads: `seq` and `qual` are row-major byte
 *   matrices [n_reads][stride] (ASCII as in the FASTQ record, stride a multiple of 4,
 *   bytes past len[i] are ignored for the results), `len` holds the read lengths.  Speed note: the scan kernel re-codes
 *   a tile of 64 rows with a fast form that vouches for the bytes A, C, G, T and N and falls back to the exact form,
 *   for good, in a wave that meets any other byte ANYWHERE in its rows (IUPAC codes, lower case, the padding): rows
 *   padded with 'N' behind the read -- what cutseq_amd's own producers write -- run about 2 % faster than rows padded
 *   with zeros.  Results are the same for any padding.  len[i] <= stride is the
 *   caller's contract; the kernel clamps a longer value to stride instead of reading past the row.
 *   Headers never cross the boundary: the device returns, per read, the surviving
 *   interval of the ORIGINAL record plus the location of the captured UMI, and the
 *   host renames/formats (cutadapt's Renamer is string work).
 */
#ifndef CUTSEQ_HIP_H
#define CUTSEQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_ABI_VERSION 7
#define CS_MAX_ADAPTER 128 /* longest adapter sequence an op can carry          */
#define CS_MAX_OPS 24      /* longest per-mate op chain                           */
#define CS_MAX_STRIDE 1536 /* longest row the LDS tile can stage (64 rows/block) */
#define CS_LEN_SKIP 0xFFFF /* cs_reads.len[i]: the kernels pass over this read (no result, not counted); the text path
                              marks reads longer than the rows this way and walks their chain in a kernel of their own */
#define CS_MAX_READ (1u << 24) /* longest read the text path takes (cs_text_*): positions are 32-bit there */

typedef enum cs_status {
  CS_OK = 0,
  CS_ERR_ARG = -1,     /* bad argument (null pointer, stride, op table)      */
  CS_ERR_HIP = -2,     /* HIP runtime error, message in cs_last_error()       */
  CS_ERR_NO_GPU = -3,  /* no usable gfx950 device: there is NO CPU fallback   */
  CS_ERR_NOMEM = -4,
  CS_ERR_STATE = -5
} cs_status;

/* ---- op table: what cutseq/run.py:305-433 (single) and :493-731 (paired) compile -- */

enum {
  CS_OP_ADAPTER = 1, CS_OP_CUT = 2, CS_OP_QTRIM = 3, CS_OP_DEMUX = 4, CS_OP_NTRIM = 5, CS_OP_NEXTSEQ = 6, CS_OP_SHORTEN = 7,
  CS_OP_POLYA = 8
};

/* CS_OP_QTRIM -- cutadapt's QualityTrimmer(cutoff_front, cutoff_back, base), quality_trim_index on the interval [s, e)
 * the op sees (n = e - s, qualities q[0..n)):
 *     back:   sum = best = 0, stop = n;  for i = n - 1 down to 0: sum += q_cutoff - (q[i] - q_base); break if sum < 0;
 *             if sum > best: best = sum, stop = i
 *     front:  sum = best = 0, start = 0; for i = 0 .. n - 1: sum += q_cutoff_front - (q[i] - q_base); break if sum < 0;
 *             if sum > best: best = sum, start = i + 1
 * Both walks run over the WHOLE interval, independently.  start >= stop: the read is empty, reported as [s, s);
 * otherwise [s + start, s + stop) is left.  cs_stats.qualtrim_bp gains n - (stop - start), CS_F_QTRIMMED says that it is
 * more than 0.  q_cutoff_front == 0 is the reference's op (cutseq installs cutoff_front = 0): the front walk does not run
 * at all -- its result would be start = 0 for every quality byte >= q_base -- and the kernels launched are those of a
 * plan without it.  cs_plan_create clamps both cutoffs to cutoff + q_base in [-1, 256] (outside, every term has one sign:
 * no result changes).
 *
 * CS_OP_NTRIM -- cutadapt's NEndTrimmer (--trim-n), no fields: the leading run a and the trailing run b of the byte 'N'
 * (0x4E; upper case only: cutadapt's patterns are ^N+ and N+$ without IGNORECASE -- TooManyN counts 'n' too) of
 * seq[s:e) go: a == e - s leaves [s, s), anything else [s + a, e - b).  No counter and no flag of its own: out_bp,
 * TooShort and the filters see the result.  A plan with a non-zero q_cutoff_front or a CS_OP_NTRIM op runs kernels of
 * its own; every other plan the kernels it ran before these came.
 *
 * CS_OP_NEXTSEQ -- cutadapt's NextseqQualityTrimmer(cutoff, base) (--nextseq-trim), nextseq_trim_index on the interval
 * [s, e) the op sees (n = e - s, bases b[0..n), qualities q[0..n)); fields q_cutoff and q_base:
 *     sum = best = 0, stop = n;  for i = n - 1 down to 0:
 *         sum += (b[i] == 'G') ? 1 : q_cutoff - (q[i] - q_base);  break if sum < 0;  if sum > best: best = sum, stop = i
 * [s, s + stop) is left: CS_OP_QTRIM's back walk in which a 'G' (0x47; upper case only, 'g' is an ordinary base) is a
 * base of quality q_cutoff - 1 whatever its quality byte says -- the dark cycles of two-colour instruments read as G
 * of high quality.  cs_stats.qualtrim_bp gains n - stop, CS_F_QTRIMMED says that it is more than 0 (cutadapt counts both
 * trimmers under quality_trimmed).  The cutoff is NOT clamped: a G's term is +1 whatever the cutoff, so the walk over
 * 100 x 'G', one 'A' of quality 'I', 300 x 'G' breaks at the 'A' under cutoff -5000 (stop 101) and goes past it under
 * -34 (stop 0).  cs_plan_create refuses an op with q_cutoff + q_base outside [-1, 256] (CS_ERR_ARG); inside, every term
 * is within the bound CS_OP_QTRIM's sums are built for.  A plan with the op runs the read-end instantiations of the
 * long-read and info kernels and tile kernels that hold the read-end modifiers' code and this op's; every other plan
 * the kernels it ran before (cutadapt's order: this op in front of the chain's CS_OP_QTRIM).
 *
 * CS_OP_SHORTEN -- cutadapt's Shortener(length) (-l / --length, -L for read 2); one field, `length` (int32), on the
 * interval [s, e) the op sees (n = e - s):
 *     length >= 0:  e = s + min(n, length)        read[:length]; length 0 leaves [s, s)
 *     length <  0:  s = e - min(n, |length|)      read[length:]: the last |length| bases stay
 * Every int32 is a valid length, INT32_MIN included: |length| is formed as an unsigned 32-bit value and compared with n
 * as such, never negated as an int.  No counter and no flag of its own (cutadapt has none): out_bp, TooShort, the
 * filters and the info table's final read see the result; qualtrim_bp and CS_F_QTRIMMED do not change.  cutadapt's order:
 * behind the chain's CS_OP_QTRIM, in front of its CS_OP_NTRIM.  A plan with the op runs the read-end instantiations of the
 * long-read and info kernels and tile kernels of its own, which hold all the read-end ops' code and this op's; every
 * other plan the kernels it ran before.
 *
 * CS_OP_POLYA -- cutadapt's PolyATrimmer (--poly-a; cutadapt >= 4.4), poly_a_trim_index on the interval [s, e) the op
 * sees (n = e - s, bases b[0..n)); one field, `reversed` (1 = the head form, PolyATrimmer(revcomp=True)).  Bytes are
 * compared exactly: only 'A' (0x41; head form: 'T', 0x54) is a match -- 'a', 'N' and everything else is an error.
 *     tail (reversed = 0):  score = errors = best = 0; index = n
 *         for i = n - 1 down to 0:
 *             if b[i] == 'A': score += 1   else: score -= 2; errors += 1
 *             if score > best and errors * 5 <= n - i:   best = score; index = i
 *         if index > n - 3: index = n              tails shorter than 3 are ignored
 *         [s, s + index) is left                   the counter gains n - index
 *     head (reversed = 1):  the mirror image: 'T', i = 0 .. n - 1, condition errors * 5 <= i + 1, index = i + 1;
 *         if index < 3: index = 0;  [s + index, e) is left;  the counter gains index
 * Equivalent facts (held to the loop by enumeration, tests/test_polya_cpu.py): a candidate of length l with e errors has
 * score l - 3e, so errors * 5 <= l  <=>  5 * score >= 2 * l; the result is the FIRST position in walk order that attains
 * the maximum score among the qualifying positions with score > 0 -- a maximum over (score, position) keys, the shape of
 * CS_OP_QTRIM's key; a walk that stands at length l with score sc is settled as soon as sc + (n - l) <= best or
 * 5 * (sc + n - l) < 2 * n (no later position can beat the best one, or qualify).  |score| <= 2 * n.
 * No flag (cs_result.flags has no free bit, and cutadapt records nothing per read); the counter
 * PolyATrimmer.trimmed_bases per mate comes through cs_polya_bp_fetch.  out_bp, TooShort, the filters and the info
 * table's final read see the result.  cutadapt's order: behind the adapter cutters, in front of the quality trimmers.  A
 * plan with the op runs tile, long-read and info kernels of its own (instantiations that hold this op's code); every
 * other plan the kernels it ran before. */

/* CS_OP_DEMUX -- extension, not a reference capability (BASELINE.json config 5): ONE pass
 * decides which of up to 255 equally long inline barcodes starts the read, where the reference would
 * need one `--ensure-inline-barcode` run per barcode, each with AdapterCutter([PrefixAdapter(barcode, 0.2)])
 * (run.py:357-362, 592-597).  A PrefixAdapter match depends on nothing but the first m + k bases of the
 * interval, so the op is a table look-up: entry = outcome of all those PrefixAdapter ops on that prefix,
 * built by running them (cutseq_amd/demux.py drives the device's own adapter op over every possible
 * prefix) and attached with cs_plan_set_demux.  Alphabet {A, C, G, T, other}; prefixes of every length
 * 0 .. m + k (reads shorter than m + k) are covered.  The matched barcode's index goes to cs_reads.bc. */
#define CS_DEMUX_NONE 0xFF      /* cs_reads.bc: no barcode matched                                   */
#define CS_DEMUX_MAX_PREFIX 11  /* m + k <= 11: at most 5^11 + ... table entries (2 bytes each)       */
#define CS_DEMUX_MAX_LONG 24    /* m + k <= 24 with cs_plan_set_demux_ops (no table of every prefix)  */
#define CS_DEMUX_BY_OPS 1       /* cs_op.shortcut of a CS_OP_DEMUX op: take cs_plan_set_demux_ops whatever m + k is
                                   (how cutseq_amd/demux.py builds the TABLES: one pass over every prefix)  */
/* table entry (uint16): [7:0] barcode index or CS_DEMUX_NONE, [11:8] bases the match removes,
 * [14] more than one barcode matched (reported: an exact copy if there is one, else the lowest index) */
#define CS_DEMUX_ENTRY(id, rstop, ambiguous) ((uint16_t)((id) | ((rstop) << 8) | ((ambiguous) ? 0x4000 : 0)))

/* cutadapt aligner flags (cutadapt.align.EndSkip) */
enum { CS_REF_START = 1, CS_QUERY_START = 2, CS_REF_END = 4, CS_QUERY_STOP = 8 };
enum {
  CS_WHERE_BACK = 14,               /* BackAdapter (run.py:346,569,580)              */
  CS_WHERE_FRONT = 11,
  CS_WHERE_PREFIX = 8,              /* PrefixAdapter (run.py:358,593,605)            */
  CS_WHERE_SUFFIX = 2,              /* SuffixAdapter (run.py:365)                    */
  CS_WHERE_FRONT_NOT_INTERNAL = 9,  /* NonInternalFrontAdapter (run.py:400,686,695)  */
  CS_WHERE_BACK_NOT_INTERNAL = 6,   /* NonInternalBackAdapter (run.py:393,679,702)   */
  CS_WHERE_ANYWHERE = 15            /* BackAdapter(force_anywhere=True)              */
};
enum { CS_REMOVE_BEFORE = 0, CS_REMOVE_AFTER = 1 };
/* Exact-substring short cut taken before the aligner.  CS_SHORTCUT_NONE (the default of every
 * op cutseq_amd/plan.py compiles) follows cutadapt >= 3: <Adapter>.match_to goes straight to
 * Aligner.locate (behind a result-neutral k-mer filter).  CS_SHORTCUT_FIND restates cutadapt <= 2.x
 * (str.find / str.rfind first) and is kept as an opt-in so its exposure can be measured
 * (tools/parity_exposure.py). */
enum { CS_SHORTCUT_NONE = 0, CS_SHORTCUT_FIND = 1 };
/* which candidate wins inside Aligner.locate */
enum {
  CS_SELECT_LEFTMOST = 0, /* cutadapt >= 4.0: first hit, replaced only by an overlapping/longer hit of higher score */
  CS_SELECT_SCORE = 1     /* cutadapt 3.x / SURVEY.md appendix B.2: highest score, then fewest errors           */
};

/* read bases as the aligner sees them: <Adapter>.match_to aligns sequence.upper() while the
 * output keeps the original bytes */
enum { CS_CASE_FOLD = 0, CS_CASE_SENSITIVE = 1 };
/* Aligner.locate on a mismatching cell whose insertion (same column, row above) and deletion (same
 * row, previous column) cost the same and less than the diagonal: which one supplies origin/score */
enum {
  CS_TIE_INSERTION = 0, /* `elif cost_insertion <= cost_deletion` first */
  CS_TIE_DELETION = 1   /* the other order */
};

/* per-read result flag bits */
enum {
  CS_F_ADAPTER5 = 0x01,  /* step-2 5' adapter matched (run.py:332-341, 544-563)   */
  CS_F_ADAPTER3 = 0x02,  /* step-3 3' adapter matched (run.py:343-355, 565-590)   */
  CS_F_INLINE = 0x04,    /* inline-barcode adapter matched (run.py:357-370)       */
  CS_F_POLY = 0x08,      /* a poly-A/T adapter matched (run.py:388-413, 673-716)  */
  CS_F_QTRIMMED = 0x10,  /* QualityTrimmer removed >= 1 base                      */
  CS_F_TOO_SHORT = 0x20, /* TooShort(min_length) is true for this mate (run.py:446-451) */
  CS_F_UNTRIMMED = 0x40, /* IsUntrimmedAny is true for this mate (run.py:97-110)  */
  CS_F_AMBIGUOUS = 0x80  /* CS_OP_DEMUX: more than one barcode matched this read   */
};

/* per-read extra flag bits (cs_reads.xflags; cs_result.flags has no free bit) */
enum {
  CS_X_TOO_MANY_N = 0x01, /* TooManyN(count) of cs_plan_set_max_n is true for this mate (cutadapt --max-n) */
  CS_X_TOO_LONG = 0x02,   /* TooLong(length) of cs_plan_set_max_length is true for this mate (cutadapt -M)  */
  CS_X_TOO_MANY_EE = 0x04 /* TooManyExpectedErrors(errors) of cs_plan_set_max_ee is true for this mate (cutadapt --max-ee) */
};
#define CS_X_COUNTS 3 /* CS_X_* bits: cs_xflag_counts_fetch returns one count per bit, bit 0 first */

typedef struct cs_op {
  uint8_t kind;          /* CS_OP_*                                                   */
  uint8_t align_flags;   /* ADAPTER: CS_WHERE_*                                       */
  uint8_t reversed;      /* ADAPTER: 1 = RightmostFrontAdapter: `seq` holds the reversed
                            adapter, the aligner walks the read right-to-left;
                            POLYA: 1 = the head form (poly-T at the 5' end);
                            DEMUX: 1 = the barcodes end the read (SuffixAdapter ops through
                            cs_plan_set_demux_ops: CS_WHERE_SUFFIX, CS_REMOVE_AFTER)     */
  uint8_t remove;        /* ADAPTER: CS_REMOVE_BEFORE (read[rstop:]) / _AFTER (read[:rstart]) */
  uint8_t shortcut;      /* ADAPTER: CS_SHORTCUT_*; DEMUX: CS_DEMUX_BY_OPS = the barcodes' own ops even where a table would fit */
  uint8_t match_flag;    /* ADAPTER: CS_F_* bit OR-ed into the result when it matched */
  uint8_t required;      /* ADAPTER: listed in IsUntrimmedAny -> CS_F_UNTRIMMED if it did not match */
  uint8_t conditional;   /* CUT: ConditionalCutter semantics (run.py:145-161)         */
  uint8_t capture;       /* CUT: 0 none, 1 = cs_result.cap_*, 2 = cs_cap2             */
  uint8_t homopolymer;   /* ADAPTER: filled by cs_plan_create (all bases equal)       */
  uint8_t q_base;        /* QTRIM: quality base (33)                                  */
  uint8_t stat_slot;     /* index into cs_stats.op_matched                            */
  uint16_t m;            /* ADAPTER: sequence length; DEMUX: barcode length           */
  uint16_t k;            /* ADAPTER / DEMUX: int(max_error_rate * m), computed in double on the host */
  uint16_t min_overlap;  /* ADAPTER: already capped to m                              */
  int16_t cut_len;       /* CUT: >0 from the 5' end, <0 from the 3' end               */
  uint16_t force_min_len;/* CUT (conditional): force_trim_min_length                  */
  int16_t q_cutoff;      /* QTRIM: cutoff_back (3' end); cutoff_front: q_cutoff_front below */
  union {                          /* (offset 24: the int32 shares the first bytes of a field only adapters use) */
    uint8_t seq[CS_MAX_ADAPTER];   /* ADAPTER: upper-cased bases                      */
    int32_t length;                /* SHORTEN: >= 0 keep the first `length` bases, < 0 the last |length| */
  };
  uint8_t thr[CS_MAX_ADAPTER + 1]; /* ADAPTER: thr[L] = floor(L * max_error_rate) in IEEE double */
  uint8_t _pad[1];
  int16_t q_cutoff_front; /* QTRIM: cutoff_front (5' end); 0 = the reference's op, no front walk (carved out of the
                             padding: a table written before the field existed holds 0 here) */
} cs_op;

typedef struct cs_params {
  uint32_t abi_version;  /* CS_ABI_VERSION                                   */
  uint16_t min_length;   /* TooShort threshold (-m, run.py:943-948)           */
  uint8_t select_rule;   /* CS_SELECT_*                                       */
  uint8_t use_filter;    /* 1 = bit-parallel pre-filter + windowed DP (result-neutral), 0 = full DP */
  uint8_t case_rule;     /* CS_CASE_*  (0 = fold, the cutadapt behaviour)         */
  uint8_t indel_tie;     /* CS_TIE_*                                          */
  uint8_t reserved8[2];
  uint32_t reserved[5];
} cs_params;

/* 8 bytes per read: [start, stop) of the ORIGINAL record survives; cap_* locates the
 * bases a capturing cut removed (the UMI that cutseq's Renamer appends, run.py:378,643). */
typedef struct cs_result {
  uint16_t start;
  uint16_t stop;
  uint16_t cap_off;
  uint8_t cap_len;
  uint8_t flags;
} cs_result;

/* second capture, single-end schemes with a 5' AND a 3' UMI only (run.py:373-378) */
typedef struct cs_cap2 {
  uint16_t off;
  uint8_t len;
  uint8_t _pad;
} cs_cap2;

typedef struct cs_stats {
  uint64_t n_reads;
  uint64_t in_bp;
  uint64_t out_bp;       /* sum of (stop - start) over all reads of the mate   */
  uint64_t qualtrim_bp;  /* QualityTrimmer.trimmed_bases                       */
  uint64_t n_too_short;
  uint64_t n_untrimmed;
  uint64_t n_exact_dp;   /* reads that needed the exact DP (diagnostic)        */
  uint64_t n_refiltered; /* reads the existence-only scan of a rare adapter op could not clear (diagnostic)   */
  uint64_t op_matched[CS_MAX_OPS]; /* AdapterCutter.with_adapters per op         */
  uint64_t n_too_many_n; /* reads of this mate with CS_X_TOO_MANY_N (a per-mate count, not a pair count) */
} cs_stats;

/* one mate's device- or host-resident arrays */
typedef struct cs_reads {
  const uint8_t *seq;
  const uint8_t *qual;
  const uint16_t *len;
  cs_result *out;
  cs_cap2 *cap2; /* may be NULL */
  uint8_t *bc;   /* may be NULL; CS_OP_DEMUX: index of the barcode that matched, CS_DEMUX_NONE otherwise */
  uint8_t *xflags; /* may be NULL; CS_X_* bits per read (0 where none applies); not written by a plan without any of
                      cs_plan_set_max_n / _max_length / _max_ee (its kernels are the ones without the filters) */
} cs_reads;

typedef struct cs_plan cs_plan;
typedef struct cs_engine cs_engine;

int cs_abi_version(void);
const char *cs_last_error(void);
int cs_device_count(void); /* number of visible HIP devices, <0 on error */

/* Replaces the modifier-list assembly of pipeline_single / pipeline_paired
 * (cutseq/run.py:326-426, 533-731): the caller hands over the compiled chain per mate.
 * n2 == 0 -> single-end.  The plan is immutable and device independent. */
int cs_plan_create(const cs_op *ops_r1, int n1, const cs_op *ops_r2, int n2, const cs_params *params,
                   cs_plan **out);
void cs_plan_destroy(cs_plan *plan);

/* Attach the look-up table of a CS_OP_DEMUX op (mate 1 or 2, op index).  `table` holds one uint16 entry per
 * prefix: first the single entry of the empty prefix, then the 5 prefixes of length 1, ... up to length
 * m + k, each block indexed by sum(digit[t] * 5^t) with digit = 0, 1, 2, 3 for A, C, T, G (bits 2:1 of the
 * ASCII code) and 4 for anything else; `entries` must be (5^(m+k+1) - 1) / 4.  The plan copies the table. */
int cs_plan_set_demux(cs_plan *plan, int mate, int op_index, const uint16_t *table, size_t entries);

/* CS_OP_DEMUX with longer barcodes (CS_DEMUX_MAX_PREFIX < m + k <= CS_DEMUX_MAX_LONG; 10- to 20-base barcodes at the
 * reference's rate of 0.2): a table of every prefix no longer fits, so the op carries the barcodes' own ops instead --
 * (also for shorter ones when the op says CS_DEMUX_BY_OPS)
 * `ops[b]` is the CS_OP_ADAPTER op of barcode b exactly as a single-barcode plan would hold it (CS_WHERE_PREFIX,
 * CS_REMOVE_BEFORE, min_overlap = m, its thr[] table; A/C/G/T only).  The library derives a look-up table over the
 * first min(m + k, 9) bases that names the barcodes which can still match (a superset, from plain edit distance), and
 * the device runs the ops of those candidates on the read and merges the outcomes by the rule of the table entries
 * above.  Reads of such a plan all pass through the resolve kernel: slower than the table form, same results. */
int cs_plan_set_demux_ops(cs_plan *plan, int mate, int op_index, const cs_op *ops, int n_ops);

/* The candidate table that cs_plan_set_demux_ops derived, read-only; for tests and tools, no caller needs it.  *depth:
 * how many bases the table looks at (min(m + k, 9), fewer where the lists outgrew the format).  first[0 .. n_first): one
 * entry per prefix of length 0 .. depth in the layout of cs_plan_set_demux (a read shorter than depth has the slot of its
 * own length's block; a 3' op indexes the read's LAST bases, last base first): offset into `pool` << 8 | candidates, 0
 * where no barcode can match.  pool[0 .. n_pool): the lists, barcode indices in ascending order -- the order the device
 * tries them in, which is what makes "the lowest index claims the read" hold.  The pointers go into the plan's own
 * storage: valid until cs_plan_destroy or the next cs_plan_set_demux_ops on that op.  CS_ERR_ARG for an op that is not a
 * CS_OP_DEMUX op with its barcode ops attached. */
int cs_plan_demux_view(const cs_plan *plan, int mate, int op_index, int *depth, const uint32_t **first, size_t *n_first,
                       const uint8_t **pool, size_t *n_pool);

/* cutadapt's --max-n filter, TooManyN(count), on both mates (reference TODO, cutseq/run.py:452, 770): a read whose
 * final interval seq[start:stop] holds too many 'N' / 'n' bases gets CS_X_TOO_MANY_N.  count < 1 is a proportion:
 * stop > start and n / (stop - start) > count (IEEE double); count >= 1 is a number: n > count.  INFINITY never fires.
 * The text path discards such a pair (pair filter "any") after TooShort and before IsUntrimmedAny.  Called before
 * cs_engine_create, like cs_plan_set_demux; never called: no filter.  CS_ERR_ARG for a negative or NaN count. */
int cs_plan_set_max_n(cs_plan *plan, double count);

/* cutadapt's -M / --max-length filter, TooLong(length), on both mates: a read whose final interval is longer than
 * `length` bases (stop - start > length, 32 bits) gets CS_X_TOO_LONG.  Called like cs_plan_set_max_n. */
int cs_plan_set_max_length(cs_plan *plan, uint32_t length);

/* cutadapt's --max-ee / --max-expected-errors filter, TooManyExpectedErrors(errors), on both mates: a read gets
 * CS_X_TOO_MANY_EE when expected_errors(qual[start:stop]) > errors, where
 *     e = 0.0; for every quality byte b, left to right: e += T[b];   T[b] = pow(10, -(b - 33) / 10.0)
 * in IEEE double.  The device adds in exactly that order, one lane per read, so the sum equals the loop's to the bit
 * (T is computed once on the host and uploaded with the plan; indexed by the raw byte, 0..255).  The comparison is
 * strict, an empty interval has 0 expected errors, INFINITY never fires.  A mate without qualities (cs_reads.qual ==
 * NULL) never gets the bit.  Called like cs_plan_set_max_n; CS_ERR_ARG for a negative or NaN bound.
 *
 * Order of the filter steps on the text path and in the host formatter (pair filter "any" throughout): TooShort ->
 * TooLong -> TooManyN -> TooManyExpectedErrors -> IsUntrimmedAny -> sink.  The three in the middle discard the pair:
 * it is written nowhere, counted in no route, and counted under the first of them that catches it. */
int cs_plan_set_max_ee(cs_plan *plan, double errors);

/* For a caller that writes the reads reverse-complemented (cs_text_params.reverse_complement, csh_format_chunk; the
 * reference's ReverseComplementConverter is a modifier, so cutadapt's filters see the read turned round): reversed != 0
 * makes the expected-error sum run over qual[stop - 1] down to qual[start], the left-to-right order of the read as it
 * is written.  The other two filters do not depend on the orientation.  Default 0. */
int cs_plan_set_ee_reversed(cs_plan *plan, int reversed);

/* What the scan kernel's leading walk was compiled to for a mate (1 or 2); for tests and tools, no caller needs it.
 * info[0]: 0 no leading walk, 1 the forward op that opens the chain walks alone, 2 the existence-only 5' op and the 3'
 * op behind it walk together; info[1]: leading groups of eight columns that can hold no candidate of either op and run
 * without scores and tests; info[2..5]: the 5' op's T(j) + 1 of columns 1..32, four bits each (0: no candidate can end
 * there). */
int cs_plan_walk_info(const cs_plan *plan, int mate, uint32_t info[6]);

/* One engine per GPU (one per process in the multi-GPU layout; replaces
 * make_runner(inpaths, cores=threads), run.py:436,753). Uploads the op tables, owns a
 * stream, the device statistics block and `n_slots` staging slots of `max_reads` reads
 * x `max_stride` bytes for cs_trim_batch (0 slots: device-pointer API only). */
int cs_engine_create(const cs_plan *plan, int device, uint32_t n_slots, uint32_t max_reads,
                     uint32_t max_stride, cs_engine **out);
void cs_engine_destroy(cs_engine *eng);

/* The hot path, inputs already resident in HBM: two kernel launches over both mates -- the scan kernel
 * (staging, bit-parallel filters, closed forms, cuts, quality trimming; reads that need the exact DP go
 * to a queue in HBM) and the resolve kernel (strip DP on that queue, then the rest of those reads'
 * chains) -- replacing the per-read modifier loop inside runner.run(pipeline, ...), run.py:473,794.
 * `stream` is a hipStream_t (NULL = the engine's own stream); asynchronous: the results are complete
 * in `stream` order.  r2 == NULL for single-end.  Calls may come on different streams: each call takes
 * one of the engine's lanes (hand-out counters, queue) and first waits for that lane's previous user. */
int cs_trim_device(cs_engine *eng, void *stream, const cs_reads *r1, const cs_reads *r2,
                   uint32_t n_reads, uint32_t stride);

/* The same two launches, pipelined across calls: the scan kernel runs on `stream`, the resolve kernel on
 * the engine's resolve stream behind it, so the NEXT call's scan kernel overlaps THIS call's resolve
 * kernel (a few latency-bound waves that fit beside the scan kernel's).  The results of a pipelined call
 * are complete in `stream` order only after cs_join(eng, stream); keep the result arrays of up to three
 * calls apart (a call waits for the call three before it).  This is how a runner keeps batches in flight
 * (make_runner(cores=N), run.py:436,753) and what bench.py times. */
int cs_trim_device_pipelined(cs_engine *eng, void *stream, const cs_reads *r1, const cs_reads *r2,
                             uint32_t n_reads, uint32_t stride);
/* makes `stream` (NULL = the engine's own) wait for every resolve kernel issued so far */
int cs_join(cs_engine *eng, void *stream);

/* Same path for host buffers (pinned via cs_alloc_pinned for true overlap), pipelined the same way:
 * hipMemcpyAsync H2D -> scan kernel on the engine stream, resolve kernel -> hipMemcpyAsync D2H on the
 * resolve stream, using staging slot `slot`; returns immediately, cs_sync(eng, slot) waits for the
 * results.  With two slots in flight one slot's upload and scan overlap the other's resolve and download. */
int cs_trim_batch(cs_engine *eng, uint32_t slot, const cs_reads *r1, const cs_reads *r2,
                  uint32_t n_reads, uint32_t stride);
int cs_sync(cs_engine *eng, uint32_t slot);

/* Device-side counters (counterpart of cutadapt's Statistics, run.py:473,794).
 * stats[0] = mate 1, stats[1] = mate 2.  Ordered behind every launch the engine has issued so far (on
 * any stream) and synchronous. */
int cs_stats_fetch(cs_engine *eng, cs_stats stats[2], int reset);

/* How many reads of each mate got each CS_X_* bit: counts[mate][k] for bit 1 << k (TooManyN, TooLong,
 * TooManyExpectedErrors).  Per mate and per bit: not pair counts, and no precedence between the filters.  Ordered and
 * synchronous like cs_stats_fetch.  counts[m][0] is cs_stats.n_too_many_n; `reset` zeroes all six counters (that word
 * of cs_stats included), and cs_stats_fetch's reset leaves the other four alone. */
int cs_xflag_counts_fetch(cs_engine *eng, uint64_t counts[2][CS_X_COUNTS], int reset);

/* cutadapt's PolyATrimmer.trimmed_bases: bp[mate] = the bases every CS_OP_POLYA op of that mate's chain removed (0 for a
 * plan without the op).  Ordered and synchronous like cs_stats_fetch; `reset` zeroes both counters, and neither
 * cs_stats_fetch's nor cs_xflag_counts_fetch's reset touches them. */
int cs_polya_bp_fetch(cs_engine *eng, uint64_t bp[2], int reset);

/* Timing of the last cs_trim_device / cs_trim_device_pipelined call, measured with HIP events recorded
 * around each kernel on the stream it ran on (ms, the two kernels added).  Synchronises on the stop event. */
int cs_last_kernel_ms(cs_engine *eng, float *ms);
/* the same launch split into its two kernels: ms[0] = scan kernel, ms[1] = resolve kernel */
int cs_last_kernel_split_ms(cs_engine *eng, float ms[2]);
/* Sums of those event-measured durations over every cs_trim_device / cs_trim_device_pipelined call since
 * the last reset (*calls of them): the per-kernel averages bench.py reports.  Waits for the calls in flight. */
int cs_kernel_time_totals(cs_engine *eng, uint32_t *calls, float ms[2], int reset);

/* ---- text path: raw FASTQ text in, finished FASTQ text out -------------------------------
 * Replaces what dnaio / cutadapt.files do around the modifier loop for the reference (record parsing in
 * runner.run's reader, cutseq/run.py:434-441, 751-758; SuffixRemover / Renamer / PairedEndRenamer string work,
 * run.py:330, 378, 537-542, 642-645; TooShort -> IsUntrimmedAny -> sink routing and record formatting,
 * run.py:446-471, 760-793): the host hands over record-aligned text blocks exactly as they come out of the file
 * or the inflate threads, the device finds the records, runs the trimming kernels on them and writes the output
 * records of the three routes; the host only reads / inflates and deflates / writes.
 *
 * A batch is `n_records` complete 4-line records per mate ('\n' or '\r\n' line ends; the last line may lack
 * its line end).  Output per mate: the records of route 0 (trimmed), 1 (too short), 2 (untrimmed) back to back,
 * each route in input order, each record as  @<id>[_<captured bases>]\n<seq[start:stop]>\n+\n<qual[start:stop]>\n.
 * Errors are reported the way the reference's reader would raise them (cs_text_result.error), never ignored. */
enum {
  CS_TEXT_OK = 0,
  CS_TEXT_ERR_MALFORMED = 1,   /* no '@' / '+' line, sequence and quality lengths differ: record `error_record` */
  CS_TEXT_ERR_TOO_LONG = 2,    /* a read is longer than CS_MAX_READ                                            */
  CS_TEXT_ERR_IDS_DIFFER = 3,  /* PairedEndRenamer: "Input read IDs not identical" at record `error_record`    */
  CS_TEXT_ERR_LINE_COUNT = 4,  /* the text does not hold 4 * n_records lines                                   */
  CS_TEXT_ERR_INFO_MISMATCH = 5, /* cs_text_params.info: the match recorder's final interval or flags of record
                                   `error_record` differ from what the trimming kernels produced: an engine fault,
                                   reported instead of a table that contradicts the records                          */
  CS_TEXT_ERR_INFO_OVERFLOW = 6, /* cs_text_params.info: the table of the batch is larger than the bound cs_text_create
                                   derived for it (an engine fault too: the bound covers every possible table); nothing
                                   of it was written                                                                 */
  /* cs_text_submit_bam: BAM record `error_record` (counted in its text; an interleaved engine: 2r + m) is refused.
   * The values are the CSB_ERR_* of include/cutseq_bam.h, tested in this order; CS_TEXT_ERR_BAM_MATE2 is set on top
   * when the record is one of bam2's. */
  CS_TEXT_ERR_BAM_BLOCK_SIZE = 16,    /* block_size below 32, or beyond the bytes its offsets give the record          */
  CS_TEXT_ERR_BAM_OVERRUN = 17,       /* fixed part, name, cigar, bases and qualities exceed block_size                */
  CS_TEXT_ERR_BAM_NAME = 18,          /* l_read_name == 0 or no NUL at the name's end                                  */
  CS_TEXT_ERR_BAM_ALIGNED = 19,       /* flag bit 0x4 not set: an aligned record                                       */
  CS_TEXT_ERR_BAM_NAME_LINE_END = 20, /* '\n' or '\r' inside the name                                                  */
  CS_TEXT_ERR_BAM_NO_QUAL = 21,       /* l_seq > 0 and qual[0] == 0xFF                                                 */
  CS_TEXT_ERR_BAM_QUAL_RANGE = 22,    /* a quality above 93                                                            */
  CS_TEXT_ERR_BAM_MATE2 = 0x40
};

/* cs_text_params.info: cutadapt's --info-file for read 1 (a TODO of the reference, cutseq/run.py "report info"):
 * per batch one more stream, the tab-separated table of every adapter match in input order.  A read with k >= 1
 * matches has k rows of 12 columns, in chain order -- name as the record outputs carry it, errors, rstart, rstop,
 * sequence left of / in / right of the match (together: the read as that op saw it), the 1-based position of the op
 * among the adapter ops of mate 1's chain, the qualities cut the same way, an empty column --, a read without one a
 * row of 5: name, -1, final sequence, final qualities, an empty column.  Every record has rows, whatever its route. */
enum {
  CS_INFO_ON = 1,      /* record the matches and format the table                                               */
  CS_INFO_GZIP = 2,    /* the table leaves the device as ONE gzip member per batch (like a route with compress)  */
  CS_INFO_NO_QUAL = 4  /* the input had no qualities (FASTA): the quality columns stay empty                    */
};

typedef struct cs_text_params {
  uint8_t has_umi;            /* Renamer template carries the captures: {id}_{cut_prefix}{cut_suffix}           */
  uint8_t untrimmed_filter;   /* IsUntrimmedAny filter installed (run.py:453-467, 771-784)                      */
  uint8_t reverse_complement; /* single-end --auto-rc on a '-' library (run.py:420-426)                         */
  uint8_t compress;           /* 1: every route's output leaves the device as ONE gzip member (32 KB deflate blocks with
                                 their own dynamic Huffman codes behind an LZ77 stage -- byte runs and the previous
                                 record's name as matches, bases as literals; the counterpart of xopen's level-1 writer
                                 the reference's OutputFiles use): route_bytes / out_bytes then count compressed bytes.
                                 2: BGZF -- every 32 KB chunk of every stream the handle compresses (the info table's
                                 with CS_INFO_GZIP) is a gzip member of its own with the 'BC' extra field: 18 header
                                 bytes, the chunk's blocks, 03 00, the chunk's CRC-32 and length; at most 32 801 bytes;
                                 no run reaches in front of its chunk.  A route's bytes are its blocks back to back,
                                 WITHOUT the 28-byte EOF marker: that ends a file, and the host appends it.
                                 Other values: CS_ERR_ARG                                                              */
  uint32_t max_tag;           /* most bytes a record name can gain: 1 + the plan's capture lengths (0 = no UMI) */
  const char *suffix1[2];     /* SuffixRemover literals of mate 1, applied in order (NULL = none)               */
  const char *suffix2[2];
  uint32_t n_bins;            /* plans with a CS_OP_DEMUX op (table form): the number of barcodes.  The trimmed
                                 records of barcode b then form route 3 + b (route 0 stays empty): 3 + n_bins streams
                                 per mate, back to back in route order; sizes through cs_text_routes.  0: no bins */
  uint8_t fasta_out;          /* records leave as FASTA (">id\nsequence\n"): the input had no qualities -- what
                                 runner.input_file_format().has_qualities() tells OutputFiles, cutseq/run.py:437-441,
                                 754-758 -- or the output files are named .fasta / .fa                              */
  uint8_t fasta_routes;       /* per-stream form of fasta_out, for output files that name different formats: bit
                                 2 * class + mate (mate 0 / 1) set = that stream's records leave as FASTA.  class 0 =
                                 trimmed, 1 = too short, 2 = untrimmed, 3 = the routes of all barcodes (n_bins > 0) or the
                                 too-long route (too_long_route; the two never meet).  A
                                 stream is FASTA when fasta_out is set or its bit is; 0 = fasta_out alone decides.  A
                                 bit of a stream the plan does not have (mate 2 of a single-end plan, class 3 without
                                 bins or a too-long route) is CS_ERR_ARG                                                                 */
  uint8_t info;               /* CS_INFO_* bits; 0 = no table (the kernels launched are then exactly those of a
                                 cs_text without the member).  CS_ERR_ARG on a plan with a CS_OP_DEMUX op            */
  uint8_t too_long_route;     /* cutadapt's --too-long-output: a pair TooLong (cs_plan_set_max_length) catches behind
                                 TooShort is written, not discarded -- as trimmed, to route 3: four streams per mate,
                                 back to back in route order (0 trimmed, 1 too short, 2 untrimmed, 3 too long), sizes
                                 through cs_text_routes; fasta_routes class 3 and a gzip member of its own (compress)
                                 are that stream's.  The other two discarding filters still discard.  0 (what the byte
                                 held while it was reserved): TooLong discards, three streams, the kernels launched are
                                 those of a cs_text without the member.  CS_ERR_ARG on a plan without
                                 cs_plan_set_max_length, and together with n_bins (class 3 is the barcodes' there)   */
} cs_text_params;

typedef struct cs_text_result {
  int32_t error;              /* CS_TEXT_*                                                                      */
  uint32_t error_record;      /* first offending record of the batch                                            */
  uint32_t max_len;           /* longest read of the batch                                                      */
  uint32_t n_records;
  uint32_t route_count[3];    /* records (pairs) per route (n_bins > 0: [0] = all barcodes together; likewise below).
                                 too_long_route: these, route_bytes and text_bytes keep describing routes 0 .. 2 --
                                 the fourth stream's sizes come from cs_text_routes -- while out_bytes sums all four */
  uint32_t n_too_many_n;      /* pairs discarded by TooManyN (cs_plan_set_max_n), in no route; cs_text_discards has
                                 this and the other two discarding filters' counts                                */
  uint64_t route_bytes[3][2]; /* [route][mate]                                                                  */
  uint64_t out_bytes[2];      /* per mate: sum over the routes = what cs_text_fetch copies                      */
  uint64_t written_bp[2];     /* per mate: bases of the records of route 0 (cutadapt's written_bp)              */
  uint32_t n_lines[2];        /* per mate: line ends found in the text (diagnostic for CS_TEXT_ERR_LINE_COUNT)  */
  uint32_t n_long[2];         /* per mate: reads longer than the rows (they took the slow, exact kernel)         */
  uint64_t text_bytes[3][2];  /* compress = 1: uncompressed size of every stream (route_bytes holds the gzip sizes) */
} cs_text_result;

typedef struct cs_text cs_text;

/* `n_slots` batches in flight, each up to `max_text_bytes` of text per mate and `max_records` records, rows of
 * `stride` bytes (multiple of 4, <= CS_MAX_STRIDE).  Uses the engine's plan, streams and statistics block. */
int cs_text_create(cs_engine *eng, const cs_text_params *params, uint32_t n_slots, uint64_t max_text_bytes,
                   uint32_t max_records, uint32_t stride, cs_text **out);
/* cutadapt's --interleaved: the mates of a paired plan in ONE text and / or ONE stream per route.  cs_text_create is
 * this function with interleave = 0 (and launches exactly the kernels it launched before this one existed).
 *
 * CS_INTERLEAVE_IN: cs_text_submit takes one text of 2 * n_records records -- mate 1 of pair 0, mate 2 of pair 0, mate 1
 * of pair 1, ... --, text2 must be NULL and bytes2 0; max_text_bytes bounds that one text.  n_records, max_records,
 * error_record and every count keep meaning pairs: a malformed record of either mate of pair r reports record r, mates
 * whose ids differ CS_TEXT_ERR_IDS_DIFFER at r, a text without 8 * n_records lines CS_TEXT_ERR_LINE_COUNT
 * (cs_text_result.n_lines[0] has the lines found, n_lines[1] is 0).
 *
 * CS_INTERLEAVE_OUT: each route's two mate streams are one stream in mate 1's buffer -- the record of mate 1, then the
 * record of mate 2, pair after pair in input order; with CS_INTERLEAVE_OUT_MATE2_FIRST mate 2's record leads (what
 * paired --auto-rc on a '-' library asks for, where two files would swap names).  route_bytes[q][1], text_bytes[q][1],
 * out_bytes[1] and the [q][1] entries of cs_text_routes are 0, the [q][0] entries describe the woven stream, and
 * cs_text_fetch takes dst2 == NULL.  With compress each route is one gzip member holding both mates.  route_count,
 * written_bp[2], cs_text_discards and the info table are what they are without the bit.
 *
 * CS_ERR_ARG: any bit on a single-end plan; an unknown bit; MATE2_FIRST without OUT; params->n_bins != 0 (the kernels of
 * demultiplexing plans are not extended); with OUT, fasta_routes bits of one class that differ between the mates (one
 * stream has one format), and a woven buffer of 1 GiB or more (the bound cs_text_create applies per mate applies to the
 * sum: output offsets keep 30 bits). */
enum { CS_INTERLEAVE_IN = 1, CS_INTERLEAVE_OUT = 2, CS_INTERLEAVE_OUT_MATE2_FIRST = 4 };
int cs_text_create_interleaved(cs_engine *eng, const cs_text_params *params, uint32_t interleave,
                               uint32_t n_slots, uint64_t max_text_bytes, uint32_t max_records,
                               uint32_t stride, cs_text **out);
/* cutadapt's --rename: the name of every output record from a template, in place of the default the reference's
 * (PairedEnd)Renamer writes (id, and '_' and the captures with cs_text_params.has_umi).  The template arrives compiled:
 * up to CS_RENAME_MAX_SEGMENTS segments, written one behind the other; the literal segments index `literals`
 * (n_bytes of them, no terminator needed; the lit_len of all literal segments sum to CS_RENAME_MAX_LITERAL at most).
 * One template serves both mates of a paired plan, each with its own header.
 *
 *   CS_RENAME_LITERAL   literals[lit_off .. lit_off + lit_len)
 *   CS_RENAME_HEADER    the header behind the SuffixRemover chain
 *   CS_RENAME_ID        Renamer.parse_name's id: the first of two blank-separated fields, else the whole header
 *   CS_RENAME_COMMENT   ... its comment: the second field with its trailing blanks, empty without one
 *   CS_RENAME_CAPTURE   the bases the first capturing CS_OP_CUT of `mate`'s chain took (0 mate 1, 1 mate 2,
 *                       CS_RENAME_OWN the mate being written); CS_RENAME_CAPTURE2: the second one's (single-end plans)
 *   CS_RENAME_MATE      '1' or '2': the mate being written
 *
 * At most CS_RENAME_MAX_HEADER segments of the three header kinds.  n = 0 is legal: every name is empty.  Call it on a
 * created cs_text before its first cs_text_submit (CS_ERR_ARG afterwards, and for a malformed table, mate 2 on a
 * single-end plan, a cs_text with n_bins): the output buffers are sized again, since max_tag no longer bounds what a
 * name gains -- per record the literals, every captured segment and the mate digits, plus the text once more per header
 * segment; the info table's bound likewise, its column 1 is mate 1's name by the template.  CS_ERR_ARG too when that
 * takes a mate's output to 1 GiB or the info table to 4 GiB.  A cs_text without the call launches the kernels it
 * launched before this function existed; one with it, instantiations of their own. */
enum { CS_RENAME_LITERAL = 0, CS_RENAME_HEADER = 1, CS_RENAME_ID = 2, CS_RENAME_COMMENT = 3, CS_RENAME_CAPTURE = 4,
       CS_RENAME_CAPTURE2 = 5, CS_RENAME_MATE = 6 };
enum { CS_RENAME_OWN = 2 };
#define CS_RENAME_MAX_SEGMENTS 16
#define CS_RENAME_MAX_LITERAL 255
#define CS_RENAME_MAX_HEADER 4
typedef struct cs_rename_seg {
  uint8_t kind;    /* CS_RENAME_*                                          */
  uint8_t mate;    /* CS_RENAME_CAPTURE / _CAPTURE2: whose capture         */
  uint8_t lit_off; /* CS_RENAME_LITERAL: where in `literals`, how many     */
  uint8_t lit_len;
} cs_rename_seg;
int cs_text_set_rename(cs_text *t, const cs_rename_seg *segments, uint32_t n, const char *literals, uint32_t n_bytes);
void cs_text_destroy(cs_text *t);
/* Asynchronous: upload (text1 / text2: host memory, pinned for true overlap; they must stay untouched until
 * cs_text_wait returns), record index, trimming kernels, output formatting.  text2 == NULL for single-end. */
int cs_text_submit(cs_text *t, uint32_t slot, const void *text1, uint64_t bytes1, const void *text2, uint64_t bytes2,
                   uint32_t n_records);
/* Blocks until the slot's batch is formatted on the device; sizes and errors in *res. */
int cs_text_wait(cs_text *t, uint32_t slot, cs_text_result *res);
/* Behind cs_text_wait: the sizes of every route stream, 3 + n_bins of them (4 with too_long_route): bytes[route][mate] as cs_text_fetch
 * delivers them (gzip members if compress), text_bytes[route][mate] uncompressed, count[route] records.  The streams of
 * a mate lie in route order in the fetched buffer.  Any of the three pointers may be NULL. */
int cs_text_routes(cs_text *t, uint32_t slot, uint64_t *bytes, uint64_t *text_bytes, uint32_t *count);
/* Behind cs_text_wait: the pairs (single-end: reads) of the slot's batch that the discarding filters took, by
 * precedence: pairs[0] TooLong, pairs[1] TooManyN (= cs_text_result.n_too_many_n), pairs[2] TooManyExpectedErrors.
 * A pair that several of them catch counts once, under the first in that order; one that TooShort catches in none.
 * With cs_text_params.too_long_route the pairs TooLong caught are written, not discarded: pairs[0] keeps counting them
 * (it equals count[3] of cs_text_routes), and stays where a report takes its too_long figure from. */
int cs_text_discards(cs_text *t, uint32_t slot, uint32_t pairs[3]);
/* Copies the output text (res->out_bytes[m] bytes per mate) into the caller's buffers and blocks until it is
 * there; the slot is free for the next cs_text_submit afterwards.  dst2 == NULL for single-end. */
int cs_text_fetch(cs_text *t, uint32_t slot, void *dst1, void *dst2);
/* The info table of the slot's batch (cs_text_params.info): *bytes as cs_text_fetch_info delivers it (the gzip member
 * with CS_INFO_GZIP), *text_bytes uncompressed, *rows table rows.  Any pointer may be NULL.  Both calls are valid between
 * cs_text_wait and cs_text_fetch; cs_text_fetch frees the slot, cs_text_fetch_info does not.  CS_ERR_STATE on a cs_text
 * created without info. */
int cs_text_info(cs_text *t, uint32_t slot, uint64_t *bytes, uint64_t *text_bytes, uint64_t *rows);
/* Copies the table (*bytes of cs_text_info) into dst and blocks until it is there. */
int cs_text_fetch_info(cs_text *t, uint32_t slot, void *dst);

void *cs_alloc_pinned(size_t bytes);
/* The same on transparent huge pages (an anonymous mapping, touched, hipHostRegister-ed): 2-3x quicker to get --
 * what a short run feels --, same copy bandwidth; falls back to cs_alloc_pinned.  Freed by cs_free_pinned too. */
void *cs_alloc_pinned_huge(size_t bytes);
void cs_free_pinned(void *p);
void *cs_alloc_device(int device, size_t bytes);
void cs_free_device(int device, void *p);
int cs_copy_to_device(int device, void *dst, const void *src, size_t bytes);
int cs_copy_to_host(int device, void *dst, const void *src, size_t bytes);
/* device to device, both pointers on `device`; the ranges must not overlap.  Blocks until the copy is done. */
int cs_copy_on_device(int device, void *dst, const void *src, size_t bytes);

/* ---- text that is already on the device -------------------------------------------------------------------------
 * cs_text_submit without the upload: dtext1 / dtext2 are device pointers on the cs_text's device that hold complete
 * text when the call is made (cs_inflate_bgzf and the cs_copy_* calls block, so what they wrote is).  Everything else
 * is cs_text_submit's: the same arguments, checks and errors, the same lifetime rule -- the texts stay untouched until
 * cs_text_wait returns --, the same kernels behind it, and interleave, rename, info, compress and the too-long route
 * work as they do there.  (The texts are copied into the slot's own buffers on the device, where cs_text_submit
 * uploads them to; the copy goes by where each pointer lives, so the one mate of a pair that still is in host memory
 * may be passed as it is.) */
int cs_text_submit_device(cs_text *t, uint32_t slot, const void *dtext1, uint64_t bytes1, const void *dtext2,
                          uint64_t bytes2, uint32_t n_records);

/* ---- unaligned BAM records, expanded to FASTQ text on the device ---------------------------------------------------
 * cs_text_submit for record bytes: bamM holds whole BAM records (block_size and block, include/cutseq_bam.h) back to
 * back, offM[r] is where record r starts and offM[n] where the last one ends -- n_records + 1 entries, ascending; for an
 * interleaved engine, CS_INTERLEAVE_IN, 2 * n_records + 1 entries in bam1 / off1, mate 1 and mate 2 alternating, and
 * bam2 / off2 NULL.  Both are host memory (pinned for speed) and stay untouched until cs_text_wait returns.  The call
 * uploads them, three launches per text (bam_sizes, text_scan_blocks, bam_expand: bam_kernels.hip.inc) write
 *     @<read_name>\n<l_seq letters of "=ACMGRSVTWYHKDBN">\n+\n<qual + 33>\n
 * per record into the slot's text buffer, and from there on it is cs_text_submit: the same kernels, results, errors,
 * slots and lifetime rules, interleave, rename, info, compress and the too-long route included.  Tags, cigar, mapq, bin
 * and positions are not read.  A record the device refuses (CS_TEXT_ERR_BAM_*) ends the batch like any reader error.
 * CS_ERR_ARG, with nothing launched: offsets that descend or leave bytesM, a record of less than 36 bytes, records that
 * expand to more text than max_text_bytes.  The device staging for records and offsets is allocated by the first such
 * call on a slot (and again when a batch brings more bytes than it holds); a cs_text that never gets one has none. */
int cs_text_submit_bam(cs_text *t, uint32_t slot, const void *bam1, uint64_t bytes1, const uint32_t *off1, const void *bam2,
                       uint64_t bytes2, const uint32_t *off2, uint32_t n_records);

/* The device twin of the host library's csh_after_kth_newline: *offset = the offset behind newline number k of
 * dtext[0 .. nbytes) (device memory on `device`), 0 for k < 1, -1 when the text holds fewer than k.  Blocks. */
int cs_dtext_after_kth_newline(int device, const void *dtext, uint64_t nbytes, int64_t k, int64_t *offset);

/* ---- BGZF input inflated on the device ---------------------------------------------------------------------------
 * A BGZF file (the htslib toolchain's .gz: `bgzip`) is a series of gzip members of at most 64 KiB of text, each with
 * its compressed size in the header and CRC-32 and ISIZE in the trailer: the host knows every input and output offset
 * before a bit is decoded.  It parses headers and trailers and hands over a table of blocks; one launch decodes them,
 * one wavefront per block (RFC 1951 complete: stored, fixed and dynamic blocks, several per member), checks ISIZE and
 * CRC-32 of every block on the device and counts its line ends in the same pass.
 *
 * A block describes the DEFLATE PAYLOAD only.  The decoder reads nothing outside comp[comp_off .. comp_off + comp_len)
 * and writes nothing outside dtext[out_off .. out_off + out_len), whatever the bytes are; no alignment is asked of
 * either offset.  A block that fails gets a verdict and leaves the other blocks of the call alone (its own output
 * range holds unspecified bytes). */
enum {
  CS_INFLATE_OK = 0,
  CS_INFLATE_ERR_BTYPE = 1,     /* block type 3                                                               */
  CS_INFLATE_ERR_STORED = 2,    /* stored block: LEN / NLEN mismatch                                          */
  CS_INFLATE_ERR_CODE = 3,      /* over-subscribed code, or an incomplete one where zlib refuses it; too many codes */
  CS_INFLATE_ERR_REPEAT = 4,    /* code-length repeat without a predecessor (or past the last code)           */
  CS_INFLATE_ERR_NO_EOB = 5,    /* no end-of-block code                                                       */
  CS_INFLATE_ERR_SYMBOL = 6,    /* invalid symbol                                                             */
  CS_INFLATE_ERR_INPUT = 7,     /* input exhausted                                                            */
  CS_INFLATE_ERR_OUTPUT = 8,    /* output overrun: more text than out_len                                     */
  CS_INFLATE_ERR_DISTANCE = 9,  /* distance too far: in front of the block's own text                         */
  CS_INFLATE_ERR_ISIZE = 10,    /* less text than out_len                                                     */
  CS_INFLATE_ERR_CRC = 11,      /* CRC-32 mismatch                                                            */
  CS_INFLATE_ERR_TRAILING = 12  /* payload bytes left behind the final deflate block                          */
};
typedef struct cs_inflate_block {
  uint64_t comp_off; /* the deflate payload: comp[comp_off .. comp_off + comp_len)                           */
  uint64_t out_off;  /* its text: dtext[out_off .. out_off + out_len)                                        */
  uint32_t comp_len;
  uint32_t out_len;  /* ISIZE                                                                                 */
  uint32_t crc32;    /* the trailer's                                                                         */
  uint32_t reserved; /* 0                                                                                     */
} cs_inflate_block;
typedef struct cs_inflate_result {
  int32_t verdict; /* CS_INFLATE_OK, or the verdict of the first block that failed */
  uint32_t block;  /* ... and its index                                             */
} cs_inflate_result;
typedef struct cs_inflate cs_inflate;

/* Device buffers for calls of up to max_comp_bytes compressed bytes and max_blocks blocks, and a stream. */
int cs_inflate_create(int device, uint64_t max_comp_bytes, uint32_t max_blocks, cs_inflate **out);
void cs_inflate_destroy(cs_inflate *h);
/* Uploads comp[0 .. comp_bytes) (host memory, pinned for speed) and the table, decodes into dtext (device memory on the
 * handle's device, dtext_cap bytes) and blocks until that is done.  lines_out[n_blocks]: '\n' per block's text (0 for a
 * failed block); verdicts_out[n_blocks]: CS_INFLATE_* per block, may be NULL; *res: the first failing block, or OK.
 * n_blocks == 0 is legal.  CS_ERR_ARG -- and nothing launched -- for a table entry that leaves comp[0 .. comp_bytes) or
 * dtext[0 .. dtext_cap), and for more bytes or blocks than the handle was made for.  A failing block is NOT an error
 * of the call (CS_OK, the verdict in *res).  One call at a time per handle. */
int cs_inflate_bgzf(cs_inflate *h, const void *comp, uint64_t comp_bytes, const cs_inflate_block *blocks, uint32_t n_blocks,
                    void *dtext, uint64_t dtext_cap, uint32_t *lines_out, int32_t *verdicts_out, cs_inflate_result *res);

#ifdef __cplusplus
}
#endif
#endif /* CUTSEQ_HIP_H */
