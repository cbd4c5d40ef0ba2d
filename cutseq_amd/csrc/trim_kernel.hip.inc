// trim_kernel.hip.inc -- the per-read trimming kernels: one body, two modes (device code only).
// Included by cutseq_hip.hip.  gfx950 / wave64 only.
//
// Two launches per batch: a scan kernel (everything that needs no DP) and a resolve kernel (the
// exact DP on full strip passes for the reads the scan kernel deferred, then the rest of their chain).
// Blocks are ONE wave (64 reads) and persistent: tiles of 64 reads are handed out dynamically.
// A tile is staged from HBM into LDS with coalesced 16-byte loads, every base re-coded to a 4-bit
// table offset (8 bases per LDS dword), then each lane owns one read and walks the whole op chain
// (cutseq/run.py:326-426 / 533-731):
//
//   ADAPTER  phase A (all lanes, both kernels):  lossless pre-filter in registers
//              - general adapters (m <= 64): Myers/Hyyro bit-vector edit distance; the
//                per-base match mask comes from an 8-entry LDS table indexed by the base
//                code, eight bases per tile dword, software-pipelined.  D[m][j] exact for
//                every column -> no candidate / exact hit / substitution-only hit settled by one
//                Hamming comparison / the column window and row limit that can hold a candidate
//              - homopolymer poly-A tail / poly-T head: the DP collapses to mismatch counts
//                (closed form, see DESIGN.md): per-lane classification of the 32 bases next to the
//                anchored end, then bitmap + scalar closed form for the wave's few maybe-lanes
//            scan kernel: a read that needs the DP goes to the queue (32-byte record), its lane drops out
//            phase B (resolve kernel: queue records and later ops of their chains): survivors
//            compacted with __ballot / mbcnt inside the wave;
//              - m <= 32: four lanes per survivor, strips of rows in registers, anti-diagonal
//                sweep with one DPP row shift per step, 16 survivors per pass
//              - otherwise: one lane per survivor, column in LDS
//              both compute cutadapt's exact (cost, score, origin) cells inside the window
//   CUT / conditional CUT: interval arithmetic on [s, e);  DEMUX: table look-up on the first m + k bases
//   QTRIM: BWA running sum on packed (sum, position) keys; with a front cutoff (FILT_ENDS kernels only) a second,
//          forward walk from the 5' end.  NTRIM (FILT_ENDS kernels only): the runs of 'N' at both ends of [s, e)
//   SHORTEN (FILT_SHORTEN kernels only): min(n, |length|) bases stay, from the 5' end or, length < 0, from the 3' end
//   NEXTSEQ (FILT_NEXTSEQ kernels and above only): QTRIM's 3' walk with the read's bases beside its qualities, a 'G' adds 1
//   POLYA (FILT_POLYA kernels only): cutadapt's poly-A walk, a running score with a rate condition, as a maximum over
//          (score, position) keys; the wave walks: the first 64 bases of 16 reads a turn, tails four reads a turn
//
// No block-wide barrier is needed after staging.  Result: 8 bytes per read.  Integer work: no MFMA.

#include <type_traits>

namespace csdev {

// Phase timers (diagnostic build only: hipcc -DCS_PHASE_TIMERS, tools/phase_timers.py): wall-clock
// cycles per wave and phase, reported through the unused tail of the op_matched[] counters.
#ifdef CS_PHASE_TIMERS
struct PhaseTimer {
  uint64_t last;
  uint32_t acc[8];
  uint32_t passes, steps, items;  // strip-DP passes, their wave-level step counts, survivors
};
#define CS_T_MARK(T, PHASE)                                   \
  {                                                           \
    const uint64_t cs_now = clock64();                        \
    (T).acc[PHASE] += (uint32_t)(cs_now - (T).last);          \
    (T).last = cs_now;                                        \
  }
#else
#define CS_T_MARK(T, PHASE)
#endif


constexpr int kWave = 64;

// packed DP cell: [31:24] cost (saturated at k+1) | [23:13] score + 1024 | [12:0] origin + 4096
constexpr uint32_t kScoreBias = 1024u, kOriginBias = 4096u;
constexpr uint32_t kCostShift = 24, kScoreShift = 13;
constexpr uint32_t kCellZero = (kScoreBias << kScoreShift) | kOriginBias;  // cost 0, score 0, origin 0
constexpr uint32_t kDeltaMatch = 1u << kScoreShift;                        // score + 1
constexpr uint32_t kDeltaMismatch = (1u << kCostShift) - (1u << kScoreShift);  // cost + 1, score - 1
constexpr uint32_t kDeltaIndel = (1u << kCostShift) - (2u << kScoreShift);     // cost + 1, score - 2

enum { FILTER_NONE = 0, FILTER_MYERS32 = 1, FILTER_MYERS64 = 2, FILTER_POLY_TAIL = 3, FILTER_POLY_HEAD = 4 };

// Base codes of the coded tile: byte = sel << 3 | invalid << 5 with sel = (ascii >> 1) & 3
// (A 0, C 1, T 2, G 3).  The code is the byte offset into an op's 8 x 8-byte match-mask table;
// entries 4..7 (anything that is not exactly A, C, G or T) are zero.
__host__ __device__ constexpr uint32_t base_code(uint32_t ascii) {
  const uint32_t sel = (ascii >> 1) & 3u;
  const bool ok = ascii == 'A' || ascii == 'C' || ascii == 'G' || ascii == 'T';
  return (sel << 3) | (ok ? 0u : 32u);
}
constexpr int kEqTableBytes = 64;
constexpr int kWaveItemDwords = 4;  // queue entry per survivor: row|j0, j1|do_end|rmax, s|e, result
constexpr int kCutRun = 4;          // most CUT ops walked in one turn of the op loop (DevOp::cut_pack)
// QTRIM: cutoff + base as cs_plan_create clamps it (build_dev_op: outside [-1, 256] every term has one sign, the result
// is that of the nearest end), and the largest |term| = |cutoff + base - quality byte| that leaves
constexpr int kQCutoffLow = -1, kQCutoffHigh = 256, kQTermMax = 256;

// The scalar fields of a cs_op as dwords (filled when the engine uploads the plan): a wave-uniform dword comes through
// the scalar cache, a byte or a halfword through a VECTOR load with a wait for everything the wave has in flight --
// some twenty of those per tile stood in the scan kernel's chain walk.
struct DevFields {
  uint32_t kind, align_flags, reversed, remove, shortcut, match_flag, required, conditional, capture, homopolymer,
      q_base, stat_slot, m, k, min_overlap, force_min_len;
  int32_t cut_len, q_cutoff;
  int32_t length;  // CS_OP_SHORTEN (0 for every other kind); takes the four bytes DevOp padded in front of peq
};

struct DevOp {
  cs_op op;         // in a coded plan op.seq holds base codes instead of ASCII (device code reads seq / thr here,
                    // every scalar field through f)
  DevFields f;
  uint64_t peq[4];  // match masks of the (possibly reversed) adapter for A, C, G, T
  uint32_t filter_mode;
  uint32_t base_char;  // homopolymer base (code in a coded plan)
  uint32_t acgt_only;  // peq[] describes the adapter completely (m <= 64, ACGT only)
  uint32_t thr_mul;    // != 0: thr[L] == (L * thr_mul) >> 16 for every L <= m (checked on the host)
  uint64_t thr_step[2];  // bit i-1 set <=> thr[i] == thr[i-1] + 1  (thr[] is a unit-step table)
  // what a block copies into LDS when it starts (built on the host, cs_plan_create):
  // match masks, entry sel (A, C, T, G, then zeros) at [sel * 2 .. + 1]: low dword = rows 1..32 from bit 0 (what
  // the DP engines index), high dword = the same mask LEFT-aligned for adapters of up to 32 bases (32-bit filter),
  // rows 33..64 otherwise
  uint32_t eq_tab[kEqTableBytes / 4];
  // coded plans: adapter bases in READ orientation (un-reversed for the rightmost variant), 4 bits per base
  uint32_t fnib[6];
  // scan kernel: matches of this op are expected to be rare (the 5' template-switch artefact, cutseq/run.py:332-341,
  // 544-563): an existence-only column scan proves "no match" for nearly every read at 12 instead of 20 instructions
  // per column, the few others go to the resolve kernel and are filtered there exactly (myers_none below)
  uint32_t exists_only;
  // scan kernel: this (existence-only) op and the adapter op behind it run as ONE forward walk (myers_pair below)
  uint32_t pair_next;
  uint32_t solo_first;  // ... or: this forward op opens the chain on its own and takes the same walk (myers_pair<false>)
  uint32_t pair_tn[4];  // forward existence test: T(j) + 1 of columns j = 1..32, four bits each (myers_pair)
  uint32_t eq_fwd[4];   // match masks of the adapter in READ orientation, left-aligned, entries A, C, T, G (sel order)
  // CUT ops: a run of consecutive cuts is walked in ONE turn of the op loop, from the run's first op (the turn itself --
  // op fields fetched from constant memory, the dispatch on the kind -- costs more than a cut: the three cuts of a
  // TAKARAV3 mate were 6 % of the scan kernel).  cut_run = cuts in the run that starts here (0 / 1: just this one);
  // cut_pack[i] = cut_len (16 bits, signed) | conditional << 16 | capture << 17 | force_min_len << 19 of its i-th cut
  uint32_t cut_run;
  uint32_t cut_pack[kCutRun];
  // scan kernel, on the op that opens the chain (pair_next or solo_first): the walk's first quiet_groups groups of eight
  // columns hold no candidate of the exact op (quiet_columns below) and no column in FRONT of their last one has
  // T(j) >= 0; they run without scores, tests and log (myers_pair)
  uint32_t quiet_groups;
};

// The leading walk's quiet columns: the largest multiple of eight Q such that the exact op (m rows, k errors) has no
// candidate in a column <= Q -- row m costs at least m - j in column j unless the reference start is free, the columns
// Aligner.locate visits apart (column_range: all of them, the op's query ends are free) -- and, where an existence-only
// op walks along (tn: its T(j) + 1 of columns 1..32, DevOp::pair_tn; null: none), T(j) = -1 for every j < Q.
__host__ __device__ inline int quiet_columns(int flags, int m, int k, const uint32_t *tn) {
  if (flags & CS_REF_START) return 0;
  int q = 0;
  while (q + 8 < m - k && q + 8 <= 32) {
    bool clear = true;
    for (int j = q > 0 ? q : 1; j < q + 8 && tn; ++j)  // (column q closed the groups so far: now it lies in front of the last one)
      clear = clear && ((tn[(j - 1) >> 3] >> (4 * ((j - 1) & 7))) & 15u) == 0u;
    if (!clear) break;
    q += 8;
  }
  return q;
}

struct DevPlan {
  cs_params params;
  int32_t n_ops[2];
  int32_t coded;  // every adapter base is A/C/G/T: the tile is re-coded at staging
  int32_t max_n_on;  // cs_plan_set_max_n was called: TooManyN(max_n) on the final interval of every read
  DevOp ops[2][CS_MAX_OPS];
  double max_n;
  // the other two filters of the final interval (kernels with FILT == 2; new fields behind the old ones, so that the
  // other kernels' loads keep their offsets)
  uint32_t max_length_on, max_length;  // cs_plan_set_max_length: TooLong(max_length)
  uint32_t max_ee_on, ee_reversed;     // cs_plan_set_max_ee: TooManyExpectedErrors(max_ee); cs_plan_set_ee_reversed
  double max_ee;
  double ee_table[256];                // 10 ** (-(byte - 33) / 10), the host's pow(), indexed by the raw quality byte
};

// Plans live in constant memory (scalar loads for everything wave-uniform); one slot per
// live engine of the process.
constexpr int kMaxPlanSlots = 8;
__constant__ DevPlan c_plans[kMaxPlanSlots];

struct MateArgs {
  const uint32_t *seq;  // [n][stride] bytes viewed as dwords
  const uint8_t *qual;
  const uint16_t *len;
  cs_result *out;
  cs_cap2 *cap2;
  uint8_t *bc;
  uint8_t *xflags;
};

// dynamic tile hand-out: counters per mate (one address sustains ~88 atomics/us; light plans need more)
constexpr uint32_t kTileCounters = 8, kTileCounterStride = 32;  // stride in dwords

struct KArgs {
  MateArgs mate[2];
  unsigned long long *stats;  // cs_stats[2] viewed as u64 words
  uint32_t n_reads;
  uint32_t stride_dw;      // global row stride in dwords
  uint32_t lds_stride_dw;  // LDS row stride in dwords (odd: conflict-free column walks)
  uint32_t col_dwords;     // LDS dwords reserved for exact-DP columns, per wave
  uint32_t plan_slot;      // index into c_plans
  uint32_t *tile_counter;  // [2][kTileCounters] unit counters, 128 bytes apart, zeroed before the launch
  uint32_t n_table_ops;    // match-mask tables kept in LDS (max op count of the two mates)
  uint32_t big_tiles;      // tiles handed out in big units (a multiple of the big unit); the rest goes in small units
  uint32_t big_shift, small_shift;  // log2 of the two unit sizes
  uint32_t static_units;   // blocks below this index own unit blockIdx.x as their first one
  uint4 *defer[2];         // per mate: queue of deferred reads, n_reads records of two uint4
  uint32_t batch_knob;     // resolve kernel: smaller batches below this many batches per wave (0 = always 64 records)
  uint32_t *defer_count;   // 128 bytes apart: [mate] records written (scan kernel), [2 + mate] batches claimed (resolve
                           // kernel), [4 + mate] records of the existence-only scan, written from the TOP of the queue down
  uint32_t defer_cap;      // records per queue
  // text path: a batch the record kernels rejected (TextMeta.err != ~0) is not trimmed -- its rows are half-built and
  // its reads must not show up in the statistics; null for every other caller
  const unsigned long long *gate;
  uint32_t item_slots;     // scan kernel: 8-byte items per lane in the wave's item log (myers_pair, ItemLog)
  uint32_t fast_recode;    // scan kernel: start with the fast form of the re-coding (CUTSEQ_FAST_RECODE=0: never; 2, tests only:
                           // always, whatever its check says)
};

__device__ __forceinline__ uint32_t cell_pack(int cost, int score, int origin) {
  return ((uint32_t)cost << kCostShift) | ((uint32_t)(score + (int)kScoreBias) << kScoreShift) |
         (uint32_t)(origin + (int)kOriginBias);
}
__device__ __forceinline__ int cell_cost(uint32_t c) { return (int)(c >> kCostShift); }
__device__ __forceinline__ int cell_score(uint32_t c) { return (int)((c >> kScoreShift) & 0x7ffu) - (int)kScoreBias; }
__device__ __forceinline__ int cell_origin(uint32_t c) { return (int)(c & 0x1fffu) - (int)kOriginBias; }
// The strips' cells (strip_dp_pass, adapters of at most 32 bases: |score| <= 2 (k + 2) + m < 256): the score takes nine
// bits and leaves two between it and the cost, zero in every stored cell, for the rank of a candidate among equals.
constexpr uint32_t kStripScoreBias = 256u, kStripPrioShift = 22;
constexpr uint32_t kStripZero = (kStripScoreBias << kScoreShift) | kOriginBias;
__device__ __forceinline__ uint32_t strip_pack(int cost, int score, int origin) {
  return ((uint32_t)cost << kCostShift) | ((uint32_t)(score + (int)kStripScoreBias) << kScoreShift) |
         (uint32_t)(origin + (int)kOriginBias);
}
__device__ __forceinline__ int strip_score(uint32_t c) {
  return (int)((c >> kScoreShift) & 0x1ffu) - (int)kStripScoreBias;
}

// thr[L] = floor(L * max_error_rate) rebuilt from the step mask (no memory access)
__device__ __forceinline__ int thr_of(const DevOp &d, int L) {
  if (d.thr_mul) return (int)(__umul24((uint32_t)max(L, 0), d.thr_mul) >> 16);  // L < 2^8, mul < 2^16: full-rate 24-bit multiply
  if (L <= 0) return 0;
  if (L <= 64) return __popcll(d.thr_step[0] & (~0ull >> (64 - L)));
  return __popcll(d.thr_step[0]) + __popcll(d.thr_step[1] & (~0ull >> (128 - L)));
}
__device__ __forceinline__ int thr_step_bit(const DevOp &d, int i) {  // thr[i] - thr[i-1], i >= 1
  return (int)(((i <= 64) ? (d.thr_step[0] >> (i - 1)) : (d.thr_step[1] >> (i - 65))) & 1ull);
}

// ASCII dword -> four 4-bit codes packed in 16 bits (SWAR): sel = (c >> 1) & 3 per byte, v_perm
// rebuilds the letter that sel stands for, any byte that differs from it is flagged invalid
// (nibble = sel | invalid << 2).  The table offset of a base is its nibble << 3, the same code
// space op.seq / base_char use.
__device__ __forceinline__ uint32_t encode4_nib(uint32_t w) {
  const uint32_t sel = (w >> 1) & 0x03030303u;
  const uint32_t expect = __builtin_amdgcn_perm(0u, 0x47544341u /* "ACTG" */, sel);
  const uint32_t diff = expect ^ w;
  const uint32_t nz = (((diff & 0x7f7f7f7fu) + 0x7f7f7f7fu) | diff) & 0x80808080u;
  const uint32_t x = sel | (nz >> 5);                // bytes hold the nibbles b3 b2 b1 b0
  const uint32_t y = x | (x >> 4);                   // byte0 = b0 | b1 << 4, byte2 = b2 | b3 << 4
  return (y & 0xffu) | ((y >> 8) & 0xff00u);
}

// The same re-coding with every constant held in a VGPR and the three-input terms spelled as
// v_bitop3: on gfx950 a VALU op with a literal or SGPR operand issues at half rate
// (tools/micro/valu_ops.hip), and the tile staging runs this once per four bases.
// Case folding (cs_params.case_rule == CS_CASE_FOLD, cutadapt's sequence.upper()) costs nothing here:
// the difference mask simply leaves out bit 5, so 'a' compares equal to the 'A' that sel stands for
// (no other byte differs from A/C/G/T in bit 5 only).
struct EncodeConsts {
  uint32_t k03, k7f, k04, actg, kff, kff00, kdiff, pick;
};
__device__ __forceinline__ EncodeConsts encode_consts(bool fold) {
  EncodeConsts c = {0x03030303u, 0x7f7f7f7fu, 0x04040404u, 0x47544341u /* "ACTG" */, 0xffu, 0xff00u,
                    fold ? 0x5f5f5f5fu : 0x7f7f7f7fu, 0x06040200u /* v_perm: bytes 0, 2 of the low source, 0, 2 of the high one */};
  asm volatile("" : "+v"(c.k03), "+v"(c.k7f), "+v"(c.k04), "+v"(c.actg), "+v"(c.kff), "+v"(c.kff00), "+v"(c.kdiff), "+v"(c.pick));
  return c;
}
// four ASCII bases -> byte 0 = nibbles of bases 0, 1; byte 2 = nibbles of bases 2, 3 (bytes 1, 3: don't care)
__device__ __forceinline__ uint32_t encode4_pairs_v(uint32_t w, const EncodeConsts &c) {
  constexpr uint32_t A = 0xF0u, B = 0xCCu, C = 0xAAu;
  const uint32_t sel = (w >> 1) & c.k03;
  const uint32_t expect = __builtin_amdgcn_perm(0u, c.actg, sel);
  const uint32_t t = __builtin_amdgcn_bitop3_b32(expect, w, c.kdiff, ((A ^ B) & C) & 0xFFu) + c.k7f;
  const uint32_t nz = __builtin_amdgcn_bitop3_b32(t, expect, w, (A | (B ^ C)) & 0xFFu);  // bit 7 of a byte: it differs
  const uint32_t x = __builtin_amdgcn_bitop3_b32(nz >> 5, c.k04, sel, ((A & B) | C) & 0xFFu);
  return x | (x >> 4);
}
__device__ __forceinline__ uint32_t encode4_nib_v(uint32_t w, const EncodeConsts &c) {
  constexpr uint32_t A = 0xF0u, B = 0xCCu, C = 0xAAu;
  const uint32_t y = encode4_pairs_v(w, c);
  return __builtin_amdgcn_bitop3_b32(y >> 8, c.kff00, y & c.kff, ((A & B) | C) & 0xFFu);
}
// eight ASCII bases (two dwords) -> one dword of the coded tile: one v_perm gathers the four pair bytes
__device__ __forceinline__ uint32_t encode8_nib_v(uint32_t w0, uint32_t w1, const EncodeConsts &c) {
  return __builtin_amdgcn_perm(encode4_pairs_v(w1, c), encode4_pairs_v(w0, c), c.pick);
}

// The FAST form of the re-coding (round 5).  For the five bytes a read is made of the code is already IN the byte:
// (ascii >> 1) & 7 is 0, 1, 2, 3 for A, C, T, G and 7 for N -- sel | invalid << 2, the code space above; and for ANY byte
// whose bits 1..3 read 4..7 it equals what the exact form assigns (sel | 4).  Only a byte that reads 0..3 WITHOUT being that
// letter (IUPAC codes, lower case, the zero bytes some callers pad rows with) would come out wrong, so the fast form checks:
// one v_perm looks up the letter the code stands for ('N' for 7, 0xff -- never equal -- for 4..6), one v_bitop3 ORs the
// difference into an accumulator that the caller looks at ONCE per tile; a wave that finds a difference stages that tile
// again with the exact form and stays with it.  Six instead of ten instructions per four bases (the staging was 6.5 % of
// the scan kernel's instructions, six of ten spent on finding bytes that are not there).  Rows padded with 'N' -- what
// this package's own producers write -- take the fast form; zero padding is as correct as ever and as fast as before.
struct FastEncodeConsts {
  uint32_t k07, lut_lo, lut_hi, pick;
};
__device__ __forceinline__ FastEncodeConsts fast_encode_consts() {
  FastEncodeConsts c = {0x07070707u, 0x47544341u /* "ACTG": codes 0..3 */, 0x4effffffu /* codes 4..6: no byte; 7: 'N' */, 0x06040200u};
  asm volatile("" : "+v"(c.k07), "+v"(c.lut_lo), "+v"(c.lut_hi), "+v"(c.pick));
  return c;
}
// four ASCII bases -> byte 0 = nibbles of bases 0, 1; byte 2 = nibbles of bases 2, 3; `bad` collects expected ^ seen
__device__ __forceinline__ uint32_t encode4_pairs_fast(uint32_t w, uint32_t &bad, const FastEncodeConsts &c) {
  constexpr uint32_t A = 0xF0u, B = 0xCCu, C = 0xAAu;
  const uint32_t x = (w >> 1) & c.k07;
  const uint32_t expect = __builtin_amdgcn_perm(c.lut_hi, c.lut_lo, x);
  bad = __builtin_amdgcn_bitop3_b32(bad, expect, w, (A | (B ^ C)) & 0xFFu);
  return x | (x >> 4);
}
__device__ __forceinline__ uint32_t encode4_nib_fast(uint32_t w, uint32_t &bad, const FastEncodeConsts &c) {
  const uint32_t y = encode4_pairs_fast(w, bad, c);
  return (y & 0xffu) | ((y >> 8) & 0xff00u);
}
__device__ __forceinline__ uint32_t encode8_nib_fast(uint32_t w0, uint32_t w1, uint32_t &bad, const FastEncodeConsts &c) {
  const uint32_t lo = encode4_pairs_fast(w0, bad, c), hi = encode4_pairs_fast(w1, bad, c);
  return __builtin_amdgcn_perm(hi, lo, c.pick);
}

// raw (ASCII) tiles: str.upper() on four bytes at once -- bytes in 'a'..'z' lose bit 5
__device__ __forceinline__ uint32_t upper4(uint32_t w) {
  const uint32_t x = w & 0x7f7f7f7fu;
  const uint32_t ge_a = x + 0x1f1f1f1fu, gt_z = x + 0x05050505u;  // bit 7: x >= 'a' / x > 'z'
  const uint32_t lower = ge_a & ~gt_z & ~w & 0x80808080u;
  return w - (lower >> 2);
}

// 16-bit LDS store at byte address `addr + imm` (imm folds into the instruction's offset field)
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
__device__ __forceinline__ void lds_write_u16(uint32_t addr, uint32_t imm, uint32_t value) {
  *(lds_u16 *)(uintptr_t)(addr + imm) = (uint16_t)value;
}

// code of the base at read position pos: coded tile = 8 bases per dword -> table offset,
// raw tile = 4 ASCII bytes per dword
template <bool CODED>
__device__ __forceinline__ uint32_t row_code(const uint32_t *row, int pos) {
  if (CODED) return ((row[pos >> 3] >> ((pos & 7) << 2)) & 7u) << 3;
  return (row[pos >> 2] >> ((pos & 3) << 3)) & 0xffu;
}
template <bool CODED>
__device__ __forceinline__ uint32_t word_code(uint32_t w, int idx) {  // idx-th base of a tile dword
  if (CODED) return (idx == 0) ? ((w << 3) & 0x38u) : ((w >> (4 * idx - 3)) & 0x38u);
  return (idx == 3) ? (w >> 24) : ((w >> (8 * idx)) & 0xffu);
}

struct Verdict {
  int found;  // 1: match decided, (qs, qe) valid (query coordinates of the aligner)
  int qs, qe;
#ifdef CS_EXP_REASON
  int reason;  // diagnostic: why the filter could not settle the read (myers_verdict)
#endif
  int need;  // 1: exact DP required on columns (j0, j1], rows 0..rmax
  int j0, j1, do_end, rmax;
  uint32_t rows;  // rows 1..32 that can be accepted in the last column (bit i - 1); all ones = unknown
};

__device__ __forceinline__ Verdict verdict_none(int m) {
  Verdict v;
  v.found = v.qs = v.qe = v.need = v.j0 = v.j1 = v.do_end = 0;
  v.rmax = m;
  v.rows = 0xffffffffu;
  return v;
}

// One DP cell, branch-free (selects only).  cutadapt's order of preference on a mismatch:
// diagonal if cost_diag <= cost_deletion and <= cost_insertion, else insertion (same column, row
// above) or deletion (same row, previous column), whichever is cheaper; cs_params.indel_tie says
// who wins when they cost the same.  The cost sits in the
// top byte of the packed cell, so comparing whole cells shifted right compares costs.
__device__ __forceinline__ uint32_t dp_cell(uint32_t diag, uint32_t left, uint32_t up, bool eq, uint32_t live_limit,
                                            uint32_t dead, bool tie_ins) {
  const uint32_t cd = diag >> kCostShift, cl = left >> kCostShift, cu = up >> kCostShift;
  // insertion = from the row above (up), deletion = from the previous column (left); cs_params.indel_tie
  const bool take_up = tie_ins ? (cu <= cl) : (cu < cl);
  const uint32_t indel = (take_up ? up : left) + kDeltaIndel;
  const bool use_diag = (cd <= cl) & (cd <= cu);
  uint32_t r = use_diag ? (diag + kDeltaMismatch) : indel;
  r = eq ? (diag + kDeltaMatch) : r;
  return (r >= live_limit) ? dead : r;
}

// mask ? a : b for an all-ones / all-zeros mask, one full-rate v_bitop3
__device__ __forceinline__ uint32_t sel_mask(uint32_t mask, uint32_t a, uint32_t b) {
  return __builtin_amdgcn_bitop3_b32(mask, a, b, 0xCAu);
}

// cutadapt Aligner.locate: column range the DP visits
__device__ __forceinline__ void column_range(int flags, int m, int k, int n, int &min_n, int &max_n) {
  max_n = n;
  min_n = 0;
  if (!(flags & CS_QUERY_START)) max_n = min(n, m + k);
  if (!(flags & CS_QUERY_STOP)) min_n = max(0, n - m - k);
}

// str.find on the query as the aligner sees it (forward or reversed walk) -- slow path for
// adapters the bit-parallel filter cannot take.  op.seq is in the tile's alphabet.
template <bool CODED>
__device__ int naive_find(const DevOp &d, const uint32_t *row, int s, int e) {
  const cs_op &op = d.op;
  const int n = e - s, m = op.m;
  for (int p = 0; p + m <= n; ++p) {
    int i = 0;
    for (; i < m; ++i) {
      const int pos = op.reversed ? (e - 1 - (p + i)) : (s + p + i);
      if (row_code<CODED>(row, pos) != op.seq[i]) break;
    }
    if (i == m) return p;
  }
  return -1;
}

// cutadapt Aligner.locate "update best" predicate: CS_SELECT_LEFTMOST = cutadapt >= 4.0,
// CS_SELECT_SCORE = cutadapt 3.x (include/cutseq_hip.h)
__device__ __forceinline__ bool better_candidate(int rule, int m, bool have_best, int b_origin, int b_cost,
                                                 int b_score, int b_length, int cost, int score, int origin,
                                                 int length) {
  if (!have_best) return true;
  if (rule == CS_SELECT_SCORE) return score > b_score || (score == b_score && cost < b_cost);
  if (origin <= b_origin + m / 2 && score > b_score) return true;
  if (length > b_length && score > b_score) return true;
  return false;
}

// ---------------------------------------------------------------------------------
// Phase A, general adapters with m <= 32 / 64: Myers' bit-vector edit distance with
// Hyyro's start conditions.  Gives D[m][j] for every column exactly, which is all the
// selection logic needs to know about reads WITHOUT a hit; reads with a possible hit get
// the column window (m+k columns in front of the first candidate) for phase B.
// ---------------------------------------------------------------------------------
template <typename W>
struct MyersState {
  W Pv, Mv;
  int score;
};

// per-base match mask: coded tile -> one LDS read from the op's table, raw tile -> selects
template <typename W, bool CODED>
__device__ __forceinline__ W eq_lookup(uint32_t c, const char *tab, W pA, W pC, W pG, W pT) {
  if (CODED) return *reinterpret_cast<const W *>(tab + c);
  const W eA = (c == 'A') ? pA : W(0), eC = (c == 'C') ? pC : W(0);
  const W eG = (c == 'G') ? pG : W(0), eT = (c == 'T') ? pT : W(0);
  return (eA | eC) | (eG | eT);
}

template <typename W>
__device__ __forceinline__ void myers_step(MyersState<W> &st, W Eq, W hin, int top_shift) {
  const W Pv = st.Pv, Mv = st.Mv;
  const W Xv = Eq | Mv;
  const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  W Ph = Mv | ~(Xh | Pv);
  W Mh = Pv & Xh;
  st.score += (int)((Ph >> top_shift) & 1) - (int)((Mh >> top_shift) & 1);
  Ph = (Ph << 1) | hin;
  Mh = Mh << 1;
  st.Pv = Mh | ~(Xv | Ph);
  st.Mv = Ph & Xv;
}

// 32-bit variant on LEFT-ALIGNED vectors (adapter row i at bit 32 - m + i - 1, so the last row is the
// sign bit), written for gfx950's issue rates (tools/micro/valu_ops.hip): and/or/xor/add/sub,
// right shifts and v_bitop3 with VGPR operands issue every ~2.3 cycles per wave, while left
// shifts, v_bfe, v_lshl_or, v_and_or, min/max, compares and anything with an SGPR or literal
// operand take twice as long.  Hence x + x for x << 1, explicit bitop3 for the three-input
// terms, the top row read with a plain >> 31, and hin / the table base kept in VGPRs.
// The 32 - m bits below the adapter carry Pv = 1, Mv = 0 and Eq = 0: they generate no carry into
// the adapter rows, produce Ph = Mh = 0 (so zeros shift into row 1 and hin_bit supplies the row-0
// delta), and reproduce themselves every column.
__device__ __forceinline__ uint32_t shl1_full_rate(uint32_t x) {
  uint32_t r;  // x + x in C++ is canonicalised back into the (half-rate) shift
  asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x));
  return r;
}
constexpr uint32_t kTtA = 0xF0u, kTtB = 0xCCu, kTtC = 0xAAu;  // bitop3 truth-table columns of operands 0, 1, 2
template <bool HIN>
__device__ __forceinline__ void myers_step_la(MyersState<uint32_t> &st, uint32_t Eq, uint32_t hin_bit) {
  const uint32_t Pv = st.Pv, Mv = st.Mv;
  const uint32_t Xv = Eq | Mv;
  const uint32_t t = (Eq & Pv) + Pv;
  const uint32_t Xh = __builtin_amdgcn_bitop3_b32(t, Pv, Eq, ((kTtA ^ kTtB) | kTtC) & 0xFFu);
  const uint32_t Ph = __builtin_amdgcn_bitop3_b32(Mv, Xh, Pv, (kTtA | ~(kTtB | kTtC)) & 0xFFu);
  const uint32_t Mh = Pv & Xh;
  st.score += (int)(Ph >> 31) - (int)(Mh >> 31);
  uint32_t Ph2 = shl1_full_rate(Ph);
  if (HIN) Ph2 |= hin_bit;  // anchored query start: +1 enters row 1 every column
  const uint32_t Mh2 = shl1_full_rate(Mh);
  st.Pv = __builtin_amdgcn_bitop3_b32(Mh2, Xv, Ph2, (kTtA | ~(kTtB | kTtC)) & 0xFFu);
  st.Mv = Ph2 & Xv;
}

// LDS byte address of a pointer into shared memory / dword read at such an address.  Doing the
// table arithmetic on a laundered 32-bit VGPR value keeps the per-base address add at full rate
// (the compiler would otherwise add the wave-uniform table base as an SGPR operand).
typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
__device__ __forceinline__ uint32_t lds_addr_of(const void *p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}
__device__ __forceinline__ uint32_t lds_read_u32(uint32_t addr) { return *(lds_cu32 *)(uintptr_t)addr; }

// Adapter bases in READ orientation (un-reversed for the rightmost variant), 4 bits per base like the
// coded tile, kFnibDwords dwords per op in LDS (32 bases + zero padding for the funnel shifts).
constexpr int kFnibDwords = 6;
#ifndef PRIO_LOOP
#define PRIO_LOOP 0
#define PRIO_REST 3
#define PRIO_RESOLVE 3
#endif
// scan kernel: queue records of a tile wait in LDS (kRingRecords x 32 bytes per wave) until the answer of their
// queue reservation is there -- one tile later; a tile that defers more reads than that reserves and writes at once
constexpr int kRingRecords = 16;

// Mismatching bases between read[p0, p0 + L) and adapter bases [f0, f0 + L) (read orientation), L <= 32,
// coded tile: both windows are cut out with funnel shifts, compared eight bases per XOR.
__device__ __forceinline__ int hamming_coded(const uint32_t *row, int p0, const uint32_t *fnib, int f0, int L, int m) {
  const int rw = p0 >> 3, fw = f0 >> 3;
  const uint32_t rsh = (uint32_t)(p0 & 7) * 4u, fsh = (uint32_t)(f0 & 7) * 4u;
  // every dword both windows can touch is asked for up front (one LDS round trip, not one per eight bases); reads
  // beyond a window stay inside the tile row's / the table's padding and are masked out below
  uint32_t rd[5], fd[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    if (8 * (q - 1) >= m) break;  // wave-uniform: L <= m
    rd[q] = row[rw + q];
    fd[q] = fnib[fw + q];
  }
  int diff = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (8 * q >= m) break;  // wave-uniform
    const uint32_t r = __builtin_amdgcn_alignbit(rd[q + 1], rd[q], rsh);
    const uint32_t f = __builtin_amdgcn_alignbit(fd[q + 1], fd[q], fsh);
    uint32_t x = r ^ f;
    x |= x >> 1;
    x |= x >> 2;
    x &= 0x11111111u;
    const int left = L - 8 * q;  // bases of this dword inside the window
    x = left >= 8 ? x : left <= 0 ? 0u : (x & ((1u << (4 * left)) - 1u));
    diff += __popc(x);
  }
  return diff;
}

// What the column scan of myers_filter / myers_pair leaves behind -> the op's verdict: no candidate, a hit that
// settles without the DP, or the DP window.  st: the Myers state behind the last column; jfirst / jlast: first and
// last column with D[m][j] <= k; (cmin, jmin): lowest D[m][j] and the first column that reaches it; exact_end: the
// first column with an exact full-length occurrence (where the flags make one recognisable), else -1.
// ROWS4: the scan kernel's form of the end-row test (four rows per step, see below); the resolve kernel -- one wave per
// SIMD, registers scarce -- keeps the row-by-row loop (with the four-row form: eight more spilled registers, 12 % slower).
template <typename W, int DIR, bool CODED, bool ROWS4 = false>
__device__ __forceinline__ Verdict myers_verdict(const DevOp &d, int rule, const uint32_t *fnib, const uint32_t *row, int s,
                                                  int e, const MyersState<W> &st, int jfirst, int jlast, int exact_end,
                                                  int cmin, int jmin, bool tie_next = false) {
  Verdict v = verdict_none(d.f.m);
  constexpr int BITS = (int)sizeof(W) * 8;
  constexpr bool LA = sizeof(W) == 4;
  const int m = d.f.m, k = d.f.k, flags = d.f.align_flags, min_overlap = d.f.min_overlap;
  const bool RS = flags & CS_REF_START, QS = flags & CS_QUERY_START;
  const bool RE = flags & CS_REF_END, QSTOP = flags & CS_QUERY_STOP;
  const int n = e - s;
  int min_n, max_n;
  column_range(flags, m, k, n, min_n, max_n);
  const int sh = LA ? BITS - m : 0;
  const bool find = d.f.shortcut == CS_SHORTCUT_FIND;
  const bool exact_by_shiftand = find && QS && QSTOP && RS;
  if (exact_end >= 0) {  // free query ends: min_n == 0 && max_n == n, the scan saw everything up to here
    // Without the short cut the exact hit still has to win Aligner.locate's selection.  It scores m,
    // more than any inexact candidate, so under the score rule it is taken and the loop breaks.
    // Under the leftmost rule it replaces the running best only if it starts within m/2 of it; every
    // candidate seen so far ended in [jfirst, exact_end) and so starts at or after jfirst - (m + k):
    // exact_end - jfirst <= m/2 - k guarantees the overlap (the usual case: the candidates right in
    // front of an exact hit are its own run, k columns long).  Otherwise an older, far-away inexact
    // hit may keep the title: the DP decides, and stops at this column as locate() does.
    // (anchored query start: every alignment starts at the first base, so the overlap is a given)
    if (exact_by_shiftand || find || rule == CS_SELECT_SCORE || !QS || exact_end - jfirst <= m / 2 - k) {
      v.found = 1;
      v.qs = exact_end - m;
      v.qe = exact_end;
      return v;
    }
#ifdef CS_EXP_REASON
    v.reason = 0;
#endif
    v.need = 1;
    v.do_end = 0;
    v.j1 = exact_end;
    v.rmax = m;
    v.j0 = max(min_n, jfirst - (m + k));
    return v;
  }
  const bool any_main = QSTOP && jfirst >= 0;
  int imax_end = -1;
  // Candidates that end at the read end, from the last column's vertical deltas.  Besides the
  // highest acceptable row this tracks the EXACT prefix hit (cost 0 at row lstar: cell
  // (0, lstar, n - lstar), pure diagonal) and whether any acceptable row above it could beat it:
  // a row i with cost c scores at most i - 2c, and it overlaps lstar's start when
  // (i - lstar) + c <= m/2.  If every such row stays below score lstar, cutadapt's selection
  // (either rule) ends on row lstar and no DP is needed.
  int lstar = -1, above_score = -0x7fffffff, above_span = 0;
  int span_all = 0;  // largest i + cost over the acceptable rows: none of them starts before n - span_all
  // best score any acceptable row can have (i - 2 cost: every error a substitution), the LONGEST row that
  // reaches it, its cost, and how many shorter rows reach it too
  int best_u = -0x7fffffff, istar = 0, cstar = 0, u_ties = 0;
  uint32_t rows = 0;
  if (max_n == n && n > 0) {
    const int first_i = RE ? 0 : m;
    const int lo = max(first_i, min_overlap);
    const int cost0 = QS ? 0 : n;  // cost of row 0 in the last column
    const W pv0 = st.Pv >> sh, mv0 = st.Mv >> sh;
    // Pass 1, branch-free: which rows are acceptable.  cost_i = cost0 + #P - #M over rows 1..i; rows below
    // `lo` cannot be accepted, their deltas are summed in one go.
    const int skip = min(max(lo - 1, 0), m);
    int cost = cost0, thr_i = 0;  // thr_i: wave-uniform, like i (the threshold steps come from the plan)
    W pv = pv0, mv = mv0;
    if (skip > 0) {
      const W below = (skip >= BITS) ? ~W(0) : ((W(1) << skip) - 1);
      cost += (sizeof(W) == 4 ? __popc((uint32_t)(pv & below)) - __popc((uint32_t)(mv & below))
                              : __popcll((unsigned long long)(pv & below)) - __popcll((unsigned long long)(mv & below)));
      pv = (skip >= BITS) ? W(0) : (pv >> skip);
      mv = (skip >= BITS) ? W(0) : (mv >> skip);
      thr_i = thr_of(d, skip);
    }
    unsigned long long acc = 0;  // bit i - 1: row i is acceptable
    if constexpr (sizeof(W) == 4 && ROWS4) {
      // 32-bit flavour, FOUR rows per step: byte b of a dword walks rows skip + 8 b + 1 .. + 8 (the bits of byte b
      // of the deltas), so eight steps cover 32 rows where the row-by-row loop took one step per row (18 for the
      // bench's 3' adapter: ~160 VALU instructions per tile and mate).  X holds the four running costs (each byte's
      // start from two popcounts), T the four thresholds + 128 (wave-uniform: scalar unit), bit 7 of a byte of
      // T - X says cost <= thr (no borrow between bytes: costs are clamped far below 128), and the flags are
      // shifted in from the top of each byte like the single flag was -- after eight steps bit t of byte b is row
      // skip + 8 b + t + 1, the mask's own order.
      const int R = m - skip;  // rows to test: 0 .. 32
      if (R > 0) {
        uint32_t ones = 0x01010101u, c80 = 0x80808080u;
        asm volatile("" : "+v"(ones), "+v"(c80));  // (VGPR operands: literals halve the issue rate)
        const uint32_t w = (uint32_t)(d.thr_step[0] >> skip);  // bit b: thr steps up INTO row skip + b + 1
        // a cost beyond every threshold stays beyond it for 32 rows (one down per row at most): clamped, so that
        // an anchored query start (cost0 = n) fits a byte
        const uint32_t c0 = (uint32_t)min(cost, 80);
        uint32_t X = c0, T = (uint32_t)(thr_i + (int)(w & 1u)) + 128u;
        if (R > 8) {
          X |= (c0 + (uint32_t)__popc(pv & 0xffu) - (uint32_t)__popc(mv & 0xffu)) << 8;
          T |= ((uint32_t)(thr_i + __popc(w & 0x1ffu)) + 128u) << 8;
        }
        if (R > 16) {
          X |= (c0 + (uint32_t)__popc(pv & 0xffffu) - (uint32_t)__popc(mv & 0xffffu)) << 16;
          T |= ((uint32_t)(thr_i + __popc(w & 0x1ffffu)) + 128u) << 16;
        }
        if (R > 24) {
          X |= (c0 + (uint32_t)__popc(pv & 0xffffffu) - (uint32_t)__popc(mv & 0xffffffu)) << 24;
          T |= ((uint32_t)(thr_i + __popc(w & 0x1ffffffu)) + 128u) << 24;
        }
        const int steps = min(R, 8);
        uint32_t flags = 0, pp = pv, mm = mv, ws = w;
        for (int t = 0; t < steps; ++t) {  // (wave-uniform)
          X += pp & ones;
          X -= mm & ones;
          pp >>= 1;
          mm >>= 1;
          flags = __builtin_amdgcn_bitop3_b32(flags >> 1, T - X, c80, 0xF8 /* a | (b & c) */);
          ws >>= 1;
          T += ws & 0x01010101u;
        }
        if (steps < 8) flags >>= (8 - steps);
        const uint32_t keep = R >= 32 ? ~0u : ((1u << R) - 1u);
        acc = (unsigned long long)(flags & keep) << skip;
      }
    } else if constexpr (sizeof(W) == 4) {
      // 32-bit flavour, row by row: the sign of cost - thr - 1 is shifted in at the top (one shift and one v_bitop3
      // instead of a 64-bit select and or per row); after row m the flags sit m bits from the top
      uint32_t top_first = 0;
      for (int i = skip + 1; i <= m; ++i) {
        cost += (int)(pv & 1) - (int)(mv & 1);
        pv >>= 1;
        mv >>= 1;
        thr_i += thr_step_bit(d, i);
        const uint32_t neg = (uint32_t)(cost - thr_i - 1);  // sign bit set: cost <= thr
        top_first = __builtin_amdgcn_bitop3_b32(top_first >> 1, neg, 0x80000000u, 0xF8 /* a | (b & c) */);
      }
      acc = m > skip ? (unsigned long long)(top_first >> (32 - m)) : 0ull;
    } else {
      for (int i = skip + 1; i <= m; ++i) {
        cost += (int)(pv & 1) - (int)(mv & 1);
        pv >>= 1;
        mv >>= 1;
        thr_i += thr_step_bit(d, i);
        acc |= (cost <= thr_i) ? (1ull << (i - 1)) : 0ull;
      }
    }
    if (m <= 32) rows = (uint32_t)acc;
    // Pass 2: the acceptable rows one by one, shortest first (a lane has a handful at most); the row's cost
    // comes back from two popcounts
    while (acc) {
      const int i = __builtin_ctzll(acc) + 1;
      acc &= acc - 1ull;
      const W upto = (i >= BITS) ? ~W(0) : ((W(1) << i) - 1);
      const int ci = cost0 + (sizeof(W) == 4 ? __popc((uint32_t)(pv0 & upto)) - __popc((uint32_t)(mv0 & upto))
                                             : __popcll((unsigned long long)(pv0 & upto)) - __popcll((unsigned long long)(mv0 & upto)));
      imax_end = i;
      span_all = max(span_all, i + ci);
      // (with a free query stop, row m of the last column is the full-length candidate of column n)
      const int u_i = (i < m || !QSTOP) ? i - 2 * ci : -0x7fffffff;
      if (u_i > best_u) {
        best_u = u_i;
        u_ties = 0;
        istar = i;
        cstar = ci;
      } else if (u_i == best_u) {
        u_ties++;
        istar = i;
        cstar = ci;
      }
      if (ci == 0) {
        lstar = i;
        above_score = -0x7fffffff;
        above_span = 0;
      } else {
        above_score = max(above_score, i - 2 * ci);
        above_span = max(above_span, i + ci);
      }
    }
  }
  if (!any_main && lstar >= 0 && QS && !RS && RE && n >= m + k && above_score < lstar &&
      above_span - lstar <= m / 2) {  // (n >= m + k: no row's alignment starts in the first column, see below)
    v.found = 1;
    v.qs = n - lstar;
    v.qe = n;
    return v;
  }
  bool any_end = imax_end >= 0;
  // Full-length hit inside the read AND a (usually accidental) partial hit at its end, far apart:
  // under the leftmost rule the partial one can never win.  Some full-length candidate is taken
  // first (the first one always is) and every such candidate starts at or before jlast - m + k;
  // a row of the last column replaces the best only if it starts within m/2 of it (it is never
  // longer), and it cannot start before n - span_all.  Dropping the end rows keeps the DP window
  // at the hit instead of stretching it to the read end.
  if (any_main && any_end && rule == CS_SELECT_LEFTMOST && QS && !RS && n - span_all > (jlast - m + k) + m / 2) {
    any_end = false;
    rows = 0;
  }
  if (!(any_main || any_end)) return v;
  // ---- substitution-only hits settle without the DP.  If the pure diagonal ending in a candidate cell
  // costs exactly what the cell costs (Hamming distance == edit distance), the recurrence walked that
  // diagonal: every cell on it holds its prefix mismatch count (a cheaper prefix would make the
  // candidate cheaper), so at each mismatch the diagonal predecessor is at least as cheap as the other
  // two and wins the tie, and matches always take the diagonal.  The cell is then (cost c, score
  // length - 2c, origin = start of the diagonal); any other candidate with cost c' scores at most
  // length' - 2c'.  What is left to show is that Aligner.locate's selection ends on that cell.
  // One exception to "a candidate with cost c' scores at most length' - 2c'": the first column holds
  // (cost i, score 0), so an alignment that starts there on row i0 > 0 has paid i0 errors without losing
  // score for them.  Such an alignment ends at a full-length column j <= m + k - 2 or, for a row of the
  // last column, needs n <= i + k - 2: with n >= m + k and (if there are full-length candidates)
  // jfirst >= m + k - 1 none exists, everything else goes to the DP.
#ifdef CS_EXP_REASON
  int why = 1 + 6 * ((any_main ? 1 : 0) + 2 * (any_end ? 1 : 0));
#endif
  if (LA && CODED && QS && !RS && n >= m + k && (!any_main || jfirst >= m + k - 1)) {
#ifdef CS_EXP_REASON
    why = 2 + 6 * ((any_main ? 1 : 0) + 2 * (any_end ? 1 : 0));
#endif
    // Full-length candidates: jmin is the first column with the lowest cost cmin.  Every earlier
    // candidate scores less (cost > cmin) and -- leftmost rule -- starts within m/2 of the cell (it ended
    // at or after jfirst, so it starts at or after jfirst - m - k): the cell replaces the running best;
    // every later candidate costs >= cmin, scores <= m - 2 cmin and cannot replace it under either rule.
    const bool main_ok = any_main && jmin >= m && (rule == CS_SELECT_SCORE || jmin - jfirst <= m / 2 - k);
    const int main_bound = any_main ? m - 2 * cmin : -0x7fffffff;  // no full-length candidate scores more
    // Candidates at the read end (rows below m when the query stop is free: row m of the last column IS
    // the full-length candidate of column n), visited from the longest row down after the columns.  Row istar is the longest one whose
    // bound i - 2 cost is the highest (best_u).  Longer rows and -- when best_u > main_bound -- all
    // full-length candidates score less; it starts within m/2 of each of them (leftmost rule: no row
    // starts before n - span_all, no full-length candidate before jfirst - m - k), so it replaces the
    // running best when its turn comes; shorter rows score at most the same and never replace it under
    // the leftmost rule -- under the score rule a shorter row with the same bound and fewer errors
    // could, hence no ties there.
    int reach = n - span_all;
    if (any_main) reach = min(reach, jfirst - m - k);
    // (without REF_END -- SuffixAdapter -- row m is the only row there is)
    const bool end_ok = any_end && istar > 0 && istar <= n &&  // (a row longer than the read has no diagonal)
                        (rule == CS_SELECT_SCORE ? u_ties == 0 : (n - istar) - reach <= m / 2);
    // one comparison per lane: the end row if it can beat every full-length candidate, else the full-length cell
    const bool try_end = end_ok && best_u > main_bound;
    const bool try_main = !try_end && main_ok &&
                          (!any_end || (rule == CS_SELECT_SCORE ? best_u < main_bound : best_u <= main_bound));
    if (try_end || try_main) {
#ifdef CS_EXP_REASON
      why = (try_end ? 3 : 4) + 6 * ((any_main ? 1 : 0) + 2 * (any_end ? 1 : 0));
#endif
      int p0, f0, len, want;
      if (try_end) {
        p0 = (DIR > 0) ? (e - istar) : s;
        f0 = (DIR > 0) ? 0 : (m - istar);
        len = istar;
        want = cstar;
      } else {  // the full-length cell wins the columns, and no end row can score more than it does
        p0 = (DIR > 0) ? (s + jmin - m) : (e - jmin);
        f0 = 0;
        len = m;
        want = cmin;
      }
      if (hamming_coded(row, p0, fnib, f0, len, m) == want) {
        v.found = 1;
        v.qs = try_end ? n - istar : jmin - m;
        v.qe = try_end ? n : jmin;
        return v;
      }
      // The hit ONE column on (second session of round 4).  A substitution-only occurrence whose last adapter base is
      // one of the substitutions costs c in its own column j* and in the column before it (the last base skipped
      // instead), so jmin = j* - 1 and the comparison above fails.  tie_next: D[m][jmin + 1] == cmin (the walk knows).
      // Cell A = (m, jmin), when the read's base in column jmin differs from the adapter's last base: its
      // query-skipping predecessor costs D[m][jmin - 1] + 1 >= c + 2 (jmin is the FIRST column with the lowest cost),
      // its diagonal one D[m - 1][jmin - 1] + 1 >= D[m][jmin - 1] >= c + 1, so the recurrence took the reference-
      // skipping step from a cell of cost c - 1 whatever its tie order: score(A) <= (m - 1) - 2 (c - 1) - 2 = m - 2c - 1.
      // Cell B = (m, jmin + 1) with a diagonal of Hamming distance c is (c, m - 2c, its diagonal's start) as above.
      // Every candidate before A costs more than c and scores at most m - 2c - 2; all of them start at or after
      // jfirst - m - k, within m/2 of B under the condition below, so B replaces whichever of them is the running best;
      // every later candidate scores at most m - 2c and replaces nothing; end rows: the same bound as for jmin's cell.
      if (DIR > 0 && try_main && tie_next && jmin + 1 <= n && (rule == CS_SELECT_SCORE || jmin + 1 - jfirst <= m / 2 - k)) {
#ifdef CS_EXP_REASON
        why = 5 + 6 * ((any_main ? 1 : 0) + 2 * (any_end ? 1 : 0));
#endif
        const uint32_t read_base = row_code<CODED>(row, s + jmin - 1);
        const uint32_t last_base = ((fnib[(m - 1) >> 3] >> (((m - 1) & 7) * 4)) & 7u) << 3;
        if (read_base != last_base && hamming_coded(row, s + jmin + 1 - m, fnib, 0, m, m) == cmin) {
          v.found = 1;
          v.qs = jmin + 1 - m;
          v.qe = jmin + 1;
          return v;
        }
      }
    }
  }
  // ---- anchored start (PrefixAdapter: the inline barcode of cutseq/run.py:357-362, 592-597): a substitution-only hit
  // that is the ONLY candidate settles here as well.  Every alignment starts in cell (0, 0), only row m holds candidates
  // (no REF_END), and the read is longer than m + k, so the last column plays no part.  If column m is the one column
  // with D[m][j] <= k and the diagonal's Hamming distance equals its cost c, the cell is (c, m - 2c, origin 0) by the
  // argument above, and Aligner.locate has nothing else to choose from.  (Not "the cheapest of several": leading
  // query-skipping steps run along row 0, whose cells hold score 0 whatever they cost, so a copy of the barcode ONE base
  // further right -- a homopolymer barcode behind a foreign first base -- costs the same and scores two more.  A test
  // with such barcodes caught the wider rule.)
  if (DIR > 0 && LA && CODED && !QS && !RS && QSTOP && !RE && any_main && !any_end && max_n < n && jfirst == m && jlast == m &&
      hamming_coded(row, s, fnib, 0, m, m) == cmin) {
    v.found = 1;
    v.qs = 0;
    v.qe = m;
    return v;
  }
#ifdef CS_EXP_REASON
  v.reason = why;
#endif
  v.need = 1;
  v.do_end = any_end ? 1 : 0;
  v.j1 = any_end ? n : jlast;
  v.rmax = m;
  // without a free reference start the aligned length of row i is i, so the rows the exact DP can
  // accept in the last column are exactly the ones found here
  if (!RS && m <= 32) v.rows = rows;
  int start;
  if (any_main) {
    start = jfirst - (m + k);
  } else {
    // only candidates at the read end: nothing above row imax_end can be accepted, and an
    // accepted row i spans at most i + thr[i] columns
    start = n - (imax_end + thr_of(d, imax_end));
    if (RE) v.rmax = imax_end;
  }
  if (!QS) start = min_n;  // anchored starts: the true first column is always inside reach
  v.j0 = max(min_n, start);
  return v;
}

template <typename W, int DIR, bool CODED, bool ROWS4>
#ifdef CS_PHASE_TIMERS
#define CS_T_PARAM , PhaseTimer &pt
#define CS_T_ARG , pt
#else
#define CS_T_PARAM
#define CS_T_ARG
#endif
__device__ __forceinline__ Verdict myers_filter(const DevOp &d, int rule, const char *tab, const uint32_t *fnib,
                                                 const uint32_t *row, int s, int e CS_T_PARAM) {
  constexpr int BITS = (int)sizeof(W) * 8;
  constexpr bool LA = sizeof(W) == 4;  // left-aligned vectors (32-bit variant)
  const int m = d.f.m, k = d.f.k, flags = d.f.align_flags;
  const bool RS = flags & CS_REF_START, QS = flags & CS_QUERY_START;
  const bool QSTOP = flags & CS_QUERY_STOP;
  const int n = e - s;
  int min_n, max_n;
  column_range(flags, m, k, n, min_n, max_n);
  const int sh = LA ? BITS - m : 0;  // bit of adapter row 1
  const W ones = (m >= BITS) ? ~W(0) : ((W(1) << m) - 1);
  const int t = min(min_n, m);
  const W low = (t >= BITS) ? ~W(0) : ((W(1) << t) - 1);
  MyersState<W> st;
  st.Mv = 0;
  if (!RS && !QS) {
    st.Pv = ones & ~low;
    st.score = max(m, min_n);
  } else if (RS && !QS) {
    st.Pv = 0;
    st.score = min_n;
  } else if (!RS && QS) {
    st.Pv = ones;
    st.score = m;
  } else {
    st.Pv = low & ones;
    st.score = min(m, min_n);
  }
  if (LA) st.Pv = (W)((st.Pv << sh) | ((W(1) << sh) - 1));  // filler bits below the adapter: Pv = 1
  const W hin = QS ? W(0) : W(1);
  uint32_t hin_bit = (uint32_t)hin << sh;
  asm volatile("" : "+v"(hin_bit));
  const W pA = (W)d.peq[0] << sh, pC = (W)d.peq[1] << sh, pG = (W)d.peq[2] << sh, pT = (W)d.peq[3] << sh;
  const int top_shift = m - 1 + sh;
  // the 32-bit filter reads the op's left-aligned masks from the block's private copy at the very
  // start of LDS (filled by the caller): the table offset of a base IS the address, no add
  // (the kernel has no static LDS, so the dynamic block -- and with it the private table -- starts at
  // LDS address 0; the kernel entry traps if that ever changes)
  auto lookup = [&](uint32_t code) -> W {
    if (LA && CODED) return (W)lds_read_u32(code);
    return eq_lookup<W, CODED>(code, tab, pA, pC, pG, pT);
  };
  auto step = [&](W Eq) {  // peel / tail columns
    if constexpr (LA) {
      myers_step_la<true>(st, Eq, hin_bit);
    } else {
      myers_step<W>(st, Eq, hin, top_shift);
    }
  };
  // the exact short cut (str.find) needs "full adapter, no error, not a skipped prefix":
  // with free query start and no free reference start that is D[m][j] == 0; otherwise a
  // shift-and automaton runs beside the Myers recurrences.
  // With free query ends and no free reference start, D[m][j] == 0 marks the exact full-length
  // occurrence: the column str.find reports (CS_SHORTCUT_FIND) and the column at which
  // Aligner.locate stops looking (`if cost == 0 and origin >= 0: break`), so the scan can stop there
  // under either setting.  With a free reference start only the short cut looks for it.
  const bool find = d.f.shortcut == CS_SHORTCUT_FIND;  // other flag sets: the caller ran naive_find
  const bool exact_by_score = QSTOP && !RS;  // (anchored query start too: PrefixAdapter, columns up to m + k)
  const bool exact_by_shiftand = find && QS && QSTOP && RS;
  W R = 0;
  const W top = W(1) << top_shift, row1 = W(1) << sh;
  int jfirst = -1, jlast = -1, exact_end = -1;
  int cmin = 0x7fff, jmin = -1;  // cheapest full-length candidate: its cost and the FIRST column that reaches it

  int j = min_n + 1;                                    // next column (1-based)
  int pos = (DIR > 0) ? (s + min_n) : (e - 1 - min_n);  // its read position
  // one column with full book-keeping (peel / tail / shift-and variant)
#define CS_MYERS_COLUMN(CH) CS_MYERS_COLUMN_EQ(lookup(CH))
#define CS_MYERS_COLUMN_EQ(EQ)                                                   \
  {                                                                              \
    const W Eq = (EQ);                                                           \
    step(Eq);                                                                    \
    if (exact_by_shiftand) {                                                     \
      R = ((R << 1) | row1) & Eq;                                                \
      if ((R & top) && exact_end < 0) exact_end = j;                             \
    }                                                                            \
    if (st.score <= k) {                                                         \
      if (jfirst < 0) jfirst = j;                                                \
      jlast = j;                                                                 \
      if (st.score < cmin) {                                                     \
        cmin = st.score;                                                         \
        jmin = j;                                                                \
      }                                                                          \
      if (exact_by_score && st.score == 0 && exact_end < 0) exact_end = j;       \
    }                                                                            \
    ++j;                                                                         \
  }
  constexpr int NB = CODED ? 8 : 4;  // bases per tile dword
  constexpr int SH = CODED ? 3 : 2;
  constexpr uint32_t BASE_BITS = CODED ? 4 : 8;
  // Groups of NB columns, software-pipelined: while the NB steps of one group run, the match masks
  // of the next group and the tile dword after that are already in flight.  A group starts at
  // the current read position, wherever that falls inside a tile dword: its NB bases are cut out
  // of two neighbouring dwords with one v_alignbit (no per-base peel loop up to a dword boundary).
  // One set of mask registers, refilled a group ahead.  Scores move by at most one per column, so three
  // of the eight columns decide whether the group can hold a candidate at all.
  W q[NB];               // ONE set of match-mask registers, refilled on the fly (see group below)
  bool grouped = false;  // wave-uniform in effect: the group loop ran, q[] holds the masks of the columns behind it
  if (!exact_by_shiftand && j + NB - 1 <= max_n && exact_end < 0) {
    grouped = true;
    // forward: the group is positions pos .. pos+NB-1 (bits `shift` up of {hi, lo} = row[wi+1], row[wi]);
    // backward: positions pos-NB+1 .. pos, consumed from the top (bits of {row[wi], row[wi-1]}).
    // One dword before the row / after it is still inside the LDS allocation.
    const int edge = (DIR > 0) ? pos : pos + 1;
    int wi = edge >> SH;
    const uint32_t shift = (uint32_t)(edge & (NB - 1)) * BASE_BITS;
    uint32_t lo = (DIR > 0) ? row[wi] : row[max(wi - 1, 0)];
    uint32_t hi = (DIR > 0) ? row[wi + 1] : row[wi];
    auto take = [&]() -> uint32_t { return __builtin_amdgcn_alignbit(hi, lo, shift); };
    auto advance = [&]() {
      wi += DIR;
      if (DIR > 0) {
        lo = hi;
        hi = row[wi + 1];
      } else {
        hi = lo;
        lo = row[max(wi - 1, 0)];
      }
    };
    // byte constants of the candidate book-keeping, in VGPRs (operands from there keep the ops at full rate)
    uint32_t kb = (0x80u | (uint32_t)k) * 0x01010101u, m80 = 0x80808080u, ones = 0x01010101u;
    asm volatile("" : "+v"(kb), "+v"(m80), "+v"(ones));
    // the mask of column u of the next group leaves for its register as soon as column u of this group has used
    // it (seven columns ahead of its use)
    auto group = [&](auto hin_tag) {
      constexpr bool HIN = decltype(hin_tag)::value;
      const uint32_t word = take();  // the bases of the NEXT group
      advance();
      int sc[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        // (the refill is asked for BEHIND the step: asked for in front of it, the old mask would have to be copied
        // out of the register the LDS read is about to overwrite -- one v_mov per column)
        if constexpr (LA) {
          myers_step_la<HIN>(st, q[u], hin_bit);
        } else {
          myers_step<W>(st, q[u], hin, top_shift);
        }
        sc[u] = st.score;
        q[u] = lookup(word_code<CODED>(word, DIR > 0 ? u : NB - 1 - u));
      }
      int lowest;
      if constexpr (NB == 8) {
        lowest = min(sc[1], min(sc[4], sc[7])) - 1;
      } else {
        lowest = min(min(sc[0], sc[1]), min(sc[2], sc[3]));
      }
      if (lowest <= k) {  // some column may hold a candidate (in most groups of a 3' adapter scan SOME lane gets here)
        __builtin_amdgcn_s_setprio(PRIO_REST);  // a few lanes, a short dependent chain: not behind the other waves' columns
        // The group's scores as bytes (they stay below 128: m + k <= 127 for every op that takes this filter).
        // Byte u of kb - packed has its top bit set exactly when sc[u] <= k: first / last candidate column from
        // the flag bits.  The lowest score of the group and the FIRST column that holds it (zero-byte search in
        // packed ^ broadcast(min)) serve both the running minimum and the exact hit (score 0).
        uint32_t plo = (uint32_t)sc[0], phi = 0;
#pragma unroll
        for (int u = 1; u < 4; ++u) plo |= (uint32_t)sc[u] << (8 * u);
        if constexpr (NB == 8) {
          phi = (uint32_t)sc[4];
#pragma unroll
          for (int u = 5; u < 8; ++u) phi |= (uint32_t)sc[u] << (8 * (u - 4));
        }
        const uint32_t clo = (kb - plo) & m80;
        const uint32_t chi = NB == 8 ? ((kb - phi) & m80) : 0u;
        if (clo | chi) {
          const unsigned long long c64 = ((unsigned long long)chi << 32) | clo;
          if (jfirst < 0) jfirst = j + (__builtin_ctzll(c64) >> 3);
          jlast = j + ((63 - __builtin_clzll(c64)) >> 3);
          int gm;
          if constexpr (NB == 8)
            gm = min(min(min(sc[0], sc[1]), min(sc[2], sc[3])), min(min(sc[4], sc[5]), min(sc[6], sc[7])));
          else
            gm = min(min(sc[0], sc[1]), min(sc[2], sc[3]));
          if (gm < cmin || (exact_by_score && gm == 0 && exact_end < 0)) {
            const uint32_t gb = __builtin_amdgcn_perm(0u, (uint32_t)gm, 0u);  // the minimum in every byte
            const uint32_t xlo = plo ^ gb, xhi = phi ^ gb;
            const uint32_t zlo = (xlo - ones) & ~xlo & m80;  // lowest flagged byte: the first zero byte, exactly
            const uint32_t zhi = NB == 8 ? ((xhi - ones) & ~xhi & m80) : 0u;
            const int gu = __builtin_ctzll(((unsigned long long)zhi << 32) | zlo) >> 3;
            if (exact_by_score && gm == 0 && exact_end < 0) exact_end = j + gu;
            if (gm < cmin) {  // strict: the first column that reaches the minimum
              cmin = gm;
              jmin = j + gu;
            }
          }
        }
        __builtin_amdgcn_s_setprio(PRIO_LOOP);
      }
      j += NB;
      pos += NB * DIR;
    };
    {
      const uint32_t word = take();
#pragma unroll
      for (int u = 0; u < NB; ++u) q[u] = lookup(word_code<CODED>(word, DIR > 0 ? u : NB - 1 - u));
      advance();
    }
    auto run = [&](auto hin_tag) {
      do {
        group(hin_tag);
      } while (j + NB - 1 <= max_n && exact_end < 0);
    };
    // Issue priority: LOW inside the column loop, high everywhere else.  A wave in the loop has an instruction
    // ready nearly every cycle and takes whatever issue slots are left; a wave between loops (staging, verdicts,
    // quality trimming, hand-out) is a chain of short dependent steps and memory round trips, and every cycle
    // it waits for an issue slot is a cycle added to that chain.
    __builtin_amdgcn_s_setprio(PRIO_LOOP);
    if (LA && QS)  // wave-uniform: free query start, nothing enters row 1
      run(std::false_type{});
    else
      run(std::true_type{});
    __builtin_amdgcn_s_setprio(PRIO_REST);
  }
  if (grouped) {
    // the up to NB - 1 columns behind the last whole group: their masks are in q[] already
#pragma unroll
    for (int u = 0; u < NB - 1; ++u) {
      if (j <= max_n && exact_end < 0) {
        CS_MYERS_COLUMN_EQ(q[u]);
        pos += DIR;
      }
    }
  }
  while (j <= max_n && exact_end < 0) {  // windows shorter than a group, the shift-and variant
    const uint32_t c = row_code<CODED>(row, pos);
    CS_MYERS_COLUMN(c);
    pos += DIR;
  }
#undef CS_MYERS_COLUMN
#undef CS_MYERS_COLUMN_EQ
  CS_T_MARK(pt, 1);
  return myers_verdict<W, DIR, CODED, ROWS4>(d, rule, fnib, row, s, e, st, jfirst, jlast, exact_end, cmin, jmin);
}

// ---------------------------------------------------------------------------------
// Phase A for ops whose matches are rare: existence only.  The same Myers recurrences as myers_filter, column for
// column, but WITHOUT the running score of the last row (4 of the 20 instructions of a column): D[m][j] is read off the
// vertical deltas every fourth column instead, popc(Pv) - popc(Mv) over the adapter rows (free query start: row 0
// costs nothing).  Scores move by at most one per column, so a column between two samples a and c that lie L columns
// apart can reach cost <= k only if a + c <= 2k + L: on random sequence a 20-nt adapter scores 9..12 and the test
// fires for one read in four hundred.  The rows of the last column are judged from the final deltas exactly as in
// myers_filter.  Returns true when Aligner.locate provably finds nothing; false sends the read to the exact filter.
// Only for the 32-bit left-aligned form on coded tiles, free query ends, no free reference start (BackAdapter flags:
// what RightmostFrontAdapter is built on, SURVEY.md appendix B.1).
// ---------------------------------------------------------------------------------
template <bool HIN>
__device__ __forceinline__ void myers_step_noscore(MyersState<uint32_t> &st, uint32_t Eq, uint32_t hin_bit) {
  const uint32_t Pv = st.Pv, Mv = st.Mv;
  const uint32_t Xv = Eq | Mv;
  const uint32_t t = (Eq & Pv) + Pv;
  const uint32_t Xh = __builtin_amdgcn_bitop3_b32(t, Pv, Eq, ((kTtA ^ kTtB) | kTtC) & 0xFFu);
  const uint32_t Ph = __builtin_amdgcn_bitop3_b32(Mv, Xh, Pv, (kTtA | ~(kTtB | kTtC)) & 0xFFu);
  const uint32_t Mh = Pv & Xh;
  uint32_t Ph2 = shl1_full_rate(Ph);
  if (HIN) Ph2 |= hin_bit;
  const uint32_t Mh2 = shl1_full_rate(Mh);
  st.Pv = __builtin_amdgcn_bitop3_b32(Mh2, Xv, Ph2, (kTtA | ~(kTtB | kTtC)) & 0xFFu);
  st.Mv = Ph2 & Xv;
}

template <int DIR>
__device__ __forceinline__ bool myers_none(const DevOp &d, const uint32_t *row, int s, int e CS_T_PARAM) {
  const int m = d.f.m, k = d.f.k, min_overlap = d.f.min_overlap;
  const bool RE = d.f.align_flags & CS_REF_END;
  const int n = e - s;
  const int sh = 32 - m;
  MyersState<uint32_t> st;
  st.Mv = 0;
  st.Pv = 0xffffffffu;  // adapter rows: cost i in the first column; filler bits below them: Pv = 1 as well
  st.score = 0;
  uint32_t fill_c = (uint32_t)(32 - m), zero = 0u;  // (operands from VGPRs keep v_bcnt's neighbours at full rate)
  asm volatile("" : "+v"(fill_c), "+v"(zero));
  int prev = m;      // D[m][0]
  int lowest = 0x7fff;  // min over the sample pairs of a + c - L
  auto sample = [&](int L) {
    const int cur = (int)__builtin_popcount(st.Pv) - (int)(__builtin_popcount(st.Mv) + fill_c);
    lowest = min(lowest, prev + cur - L);
    prev = cur;
  };
  auto lookup = [&](uint32_t code) -> uint32_t { return lds_read_u32(code); };  // the op's private table at LDS address 0
  constexpr int NB = 8;
  int j = 1;
  int pos = (DIR > 0) ? s : (e - 1);
  uint32_t q[NB];
  if (n >= NB) {
    const int edge = (DIR > 0) ? pos : pos + 1;
    int wi = edge >> 3;
    const uint32_t shift = (uint32_t)(edge & (NB - 1)) * 4u;
    uint32_t lo = (DIR > 0) ? row[wi] : row[max(wi - 1, 0)];
    uint32_t hi = (DIR > 0) ? row[wi + 1] : row[wi];
    auto take = [&]() -> uint32_t { return __builtin_amdgcn_alignbit(hi, lo, shift); };
    auto advance = [&]() {
      wi += DIR;
      if (DIR > 0) {
        lo = hi;
        hi = row[wi + 1];
      } else {
        hi = lo;
        lo = row[max(wi - 1, 0)];
      }
    };
    {
      const uint32_t word = take();
#pragma unroll
      for (int u = 0; u < NB; ++u) q[u] = lookup(word_code<true>(word, DIR > 0 ? u : NB - 1 - u));
      advance();
    }
    __builtin_amdgcn_s_setprio(PRIO_LOOP);
    do {
      const uint32_t word = take();  // the bases of the NEXT group
      advance();
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        myers_step_noscore<false>(st, q[u], 0u);
        q[u] = lookup(word_code<true>(word, DIR > 0 ? u : NB - 1 - u));
        if (u == 3 || u == 7) sample(4);
      }
      j += NB;
    } while (j + NB - 1 <= n);
    __builtin_amdgcn_s_setprio(PRIO_REST);
    // the up to NB - 1 columns behind the last whole group: their masks are in q[] already
    int since = 0;
#pragma unroll
    for (int u = 0; u < NB - 1; ++u) {
      if (j <= n) {
        myers_step_noscore<false>(st, q[u], 0u);
        ++j;
        ++since;
        if (since == 4) {
          sample(4);
          since = 0;
        }
      }
    }
    if (since) sample(since);
  } else {
    for (; j <= n; ++j) {  // reads shorter than a group
      myers_step_noscore<false>(st, lookup(row_code<true>(row, pos)), 0u);
      pos += DIR;
    }
    if (n > 0) sample(n);
  }
  CS_T_MARK(pt, 1);
  bool none = lowest > 2 * k;  // no column can hold a full-length candidate
  // rows of the last column (candidates that end at the read end): exact costs from the final deltas
  if (n > 0) {
    const int first_i = RE ? 0 : m;
    const int lo_i = max(first_i, min_overlap);
    const uint32_t pv0 = st.Pv >> sh, mv0 = st.Mv >> sh;
    const int skip = min(max(lo_i - 1, 0), m);
    int cost = 0, thr_i = 0;
    uint32_t pv = pv0, mv = mv0;
    if (skip > 0) {
      const uint32_t below = (skip >= 32) ? ~0u : ((1u << skip) - 1u);
      cost += __popc(pv & below) - __popc(mv & below);
      pv = (skip >= 32) ? 0u : (pv >> skip);
      mv = (skip >= 32) ? 0u : (mv >> skip);
      thr_i = thr_of(d, skip);
    }
    bool any = false;
    for (int i = skip + 1; i <= m; ++i) {
      cost += (int)(pv & 1u) - (int)(mv & 1u);
      pv >>= 1;
      mv >>= 1;
      thr_i += thr_step_bit(d, i);
      any = any || cost <= thr_i;
    }
    none = none && !any;
  }
  return none;
}

// ---------------------------------------------------------------------------------
// Phase A for the PAIR of ops that opens every chain the reference compiles (cutseq/run.py:332-355, 544-590): the 5' op
// (RightmostFrontAdapter -- existence only, see myers_none) and the 3' op right behind it (BackAdapter -- the exact
// filter of myers_filter), in ONE forward walk over the read.  Both recurrences share the base extraction, ONE
// 64-bit LDS look-up per base (private table: low dword = the 3' op's mask, high dword = the 5' adapter's mask in READ
// orientation), the tile walk and the loop; two independent dependency chains per lane fill each other's gaps.
//
// Why the 5' op may walk forward although Aligner.locate sees the reversed read: the test only has to be a SUPERSET
// of "locate finds something" (a read it cannot clear goes to the resolve kernel, which runs the op's exact filter).
//   * A full-length occurrence (cost <= k) is the same substring whichever way it is read: D[m][j] <= k at its end.
//   * A partial occurrence is the adapter's last i bases (i >= min_overlap) against a PREFIX read[0:x] with cost
//     c <= thr[i].  The forward walk lets the first m - min_overlap adapter rows be skipped for nothing (column 0 costs
//     0 up to that row, then +1 per row: the rest of a longer skip are deletions, which such an alignment may contain
//     anyway), so cell (m, x) <= c.  |i - x| <= c bounds the length: T(x) = max thr[i] over i in [min_overlap, m] with
//     |i - x| <= thr[i] (-1: none; computed on the host, DevOp::pair_tn) and D[m][x] <= T(x) must hold.
// The first columns (up to m + k: T varies) are tested column by column with a running score; behind them T = k and
// the score is sampled from the vertical deltas every fourth column as in myers_none.  On the bench reads the test
// cannot clear 0.9 % of the reads (the reversed walk with its exact row thresholds: 0.7 %; tools/pair_scan_sim.py).
//
// Both ops see the interval [s, e) the chain starts with: a read whose 5' op may match leaves for the resolve
// kernel at that op and the 3' verdict computed here is dropped with it.
// Returns the 3' op's verdict; a_none: Aligner.locate provably finds nothing for the 5' op.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long lds_read_u64(uint32_t addr) { return *(const lds_u64 *)(uintptr_t)addr; }
typedef __attribute__((address_space(3))) uint8_t lds_u8;
__device__ __forceinline__ void lds_write_u8(uint32_t addr, uint32_t imm, uint32_t value) {
  *(lds_u8 *)(uintptr_t)(addr + imm) = (uint8_t)value;
}
__device__ __forceinline__ uint32_t lds_read_u8(uint32_t addr) { return *(const lds_u8 *)(uintptr_t)addr; }
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// The 3' op's candidate book-keeping is DEFERRED (round 4).  Some lane of a wave holds a candidate (D[m][j] <= k) in 94 %
// of the groups -- a third of the reads carry the adapter -- so the ~47 instructions that turn a group's eight scores
// into (jfirst, jlast, cmin, jmin) ran in nearly every group for 4 % of the (lane, group) pairs.  Now a lane with a
// candidate in the group only LOGS the group: eight byte stores of the scores and one of the group's index into the
// lane's slots of the wave's item log in LDS (no VALU work), and the book-keeping runs once behind the loops, item by
// item in column order -- two to three rounds per tile instead of eighteen.  A lane with more flagged groups than
// slots (adapter concatemers, low-complexity reads) is not decided here: it reports "unknown" and the caller sends the
// read to the top region of the deferral queue, where the resolve kernel filters the chain's first op exactly.
struct ItemLog {
  uint32_t slot0;    // LDS byte address of this lane's first item (8 bytes each: the group's scores)
  uint32_t bytes;    // bytes of items per lane (slots * 8)
  uint32_t tag_off;  // the item at byte address A has its group index at byte (A >> 3) + tag_off
};

// HAS_A = false: the same walk for a chain that opens with the forward op alone (a plain 3' adapter, BASELINE config 2):
// no second recurrence, everything else as it is -- groups on dword boundaries, two look-ups in flight.
template <bool HAS_A>
__device__ __forceinline__ Verdict myers_pair(const DevOp &da, const DevOp &db, int rule, const uint32_t *fnib_b,
                                               const uint32_t *row, int e, bool &a_none, const ItemLog &il CS_T_PARAM) {
  constexpr int NB = 8;
  constexpr int s = 0;  // the pair opens the chain: nothing has moved the interval's start yet (the caller checks)
  const int n = e - s;
  // ---- the 3' op: myers_filter's 32-bit left-aligned form, free query ends
  const int m = db.f.m, k = db.f.k;
  const bool RS = db.f.align_flags & CS_REF_START;
  const int sh = 32 - m;
  MyersState<uint32_t> st;
  st.Mv = 0;
  st.Pv = RS ? 0u : (m >= 32 ? ~0u : ((1u << m) - 1u));
  // The walk keeps D[m][j] - (k + 1): a column is a candidate exactly when the value is negative, so "some column of the
  // group holds one" is the sign of the OR of its eight values (four full-rate instructions; the minimum of eight took
  // four half-rate ones) and a logged item marks its candidates with bit 7 of their bytes.
  const int k1 = k + 1;
  st.score = (RS ? 0 : m) - k1;
  st.Pv = (st.Pv << sh) | ((1u << sh) - 1u);  // filler bits below the adapter: Pv = 1
  const bool exact_by_score = !RS;
  // (the exact full-length occurrence, where the flags make one recognisable, is the first column that reaches cost 0:
  // jmin when cmin == 0; the walk goes on behind it for the 5' op's sake, which changes none of the four)
  int jfirst = -1, jlast = -1;
  int cmin = 0x7fff, jmin = -1;
  bool tie_next = false;     // D[m][jmin + 1] == cmin (myers_verdict: the hit one column on)
  uint32_t slot = il.slot0;  // the lane's next free item of the log
  const uint32_t slot_end = il.slot0 + il.bytes;
  bool log_full = false;     // more flagged groups than slots: the read is not decided here
  // ---- the 5' op, forward: rows up to m - min_overlap cost nothing in column 0
  const int ma = da.f.m, ka = da.f.k;
  const int sha = 32 - ma, free_a = ma - (int)da.f.min_overlap;
  MyersState<uint32_t> sa;
  sa.Mv = 0;
  sa.Pv = (((ma >= 32 ? ~0u : ((1u << ma) - 1u)) & ~((1u << free_a) - 1u)) << sha) | ((1u << sha) - 1u);
  sa.score = ma - free_a;  // D[m][0]; exact behind every column of the first groups, at the samples later on
  int flag = 0;            // sign bit: some column may hold a candidate of the 5' op
  const uint32_t tn0 = da.pair_tn[0], tn1 = da.pair_tn[1], tn2 = da.pair_tn[2], tn3 = da.pair_tn[3];  // T + 1 of columns 1..32
  const uint32_t fill_a = (uint32_t)sha, cst4 = (uint32_t)(4 + 2 * ka + 1);
  auto sample_a = [&](uint32_t cst) {  // cst = L + 2k + 1, L columns since the last exact value
    const int cur = (int)__builtin_popcount(sa.Pv) - (int)(__builtin_popcount(sa.Mv) + fill_a);
    flag |= sa.score + cur - (int)cst;
    sa.score = cur;
  };
  // T(j) + 1 for a per-lane column (tail columns only; by value: a lambda that captures the four words by reference
  // ends up as an array of pointers on the stack)
  const unsigned long long tn_lo = ((unsigned long long)tn1 << 32) | tn0, tn_hi = ((unsigned long long)tn3 << 32) | tn2;
  auto tn_of = [tn_lo, tn_hi, ka](int j) -> int {
    int t1 = ka + 1;
    if (__ballot(j <= 32)) {  // (a real branch: reads of ordinary length have left the table behind)
      const unsigned long long w = j <= 16 ? tn_lo : tn_hi;
      const int tj = (int)((uint32_t)(w >> (((uint32_t)(j - 1) & 15u) * 4u)) & 15u);
      t1 = j > 32 ? t1 : tj;
    }
    return t1;
  };
  // one column with full book-keeping for both ops (tail columns, reads shorter than a group)
  auto column = [&](uint32_t eb, uint32_t ea, int j) {
    myers_step_la<false>(st, eb, 0u);
    if constexpr (HAS_A) {
      myers_step_la<false>(sa, ea, 0u);
      flag |= sa.score - tn_of(j);
    }
    if (st.score < 0) {  // (biased: D[m][j] <= k)
      if (jfirst < 0) jfirst = j;
      jlast = j;
      if (j == jmin + 1 && st.score + k1 == cmin) tie_next = true;
      if (st.score + k1 < cmin) {
        cmin = st.score + k1;
        jmin = j;
        tie_next = false;
      }
    }
  };
  int j = 1;
  if (n >= NB) {
    int wi = 0;  // the group's tile dword (groups start on dword boundaries: s == 0)
    auto take = [&]() -> uint32_t { return row[wi]; };
    auto advance = [&]() { wi += 1; };
    // masks of QD columns in flight (two ops: 2 QD registers); the bases of the group's later columns and of the next
    // group's first ones wait in `wcur` / `wnext`
#ifndef CS_PAIR_DEPTH
#define CS_PAIR_DEPTH 2  // (1 / 2 / 4 / 8 measured: 3588 / 3603 / 3591 / 3563 M pairs/s, profiles/r04_pair_depth_ab.log)
#endif
    constexpr int QD = CS_PAIR_DEPTH;  // look-ups in flight per lane, each two columns ahead of its use
    static_assert(NB % QD == 0, "a group's columns must map onto the slots the same way in every group");
    uint32_t qb[QD], qa[QD];
    auto refill = [&](int slot, uint32_t code) {
      const unsigned long long pr = lds_read_u64(code);
      qb[slot] = (uint32_t)pr;
      qa[slot] = (uint32_t)(pr >> 32);
    };
    uint32_t wcur = take();
    advance();
#pragma unroll
    for (int u = 0; u < QD; ++u) refill(u, word_code<true>(wcur, u));
    constexpr int STEADY = 0, EARLY_G = 1, QUIET = 2;
    auto group = [&](auto body_tag, uint32_t tw) {
      constexpr bool EARLY = decltype(body_tag)::value == EARLY_G;
      const uint32_t wnext = take();  // the bases of the NEXT group
      advance();
      if constexpr (decltype(body_tag)::value == QUIET) {
        // no column of the group can hold a candidate of either op (DevOp::quiet_groups): the bare recurrences
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          myers_step_noscore<false>(st, qb[u % QD], 0u);
          if constexpr (HAS_A) myers_step_noscore<false>(sa, qa[u % QD], 0u);
          refill(u % QD, u + QD < NB ? word_code<true>(wcur, u + QD) : word_code<true>(wnext, u + QD - NB));
        }
        wcur = wnext;
        j += NB;
        return;
      }
      int sc[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        myers_step_la<false>(st, qb[u % QD], 0u);
        sc[u] = st.score;
        if constexpr (HAS_A && EARLY) {
          myers_step_la<false>(sa, qa[u % QD], 0u);
          flag |= sa.score - (int)((tw >> (4 * u)) & 15u);
        } else if constexpr (HAS_A) {
          myers_step_noscore<false>(sa, qa[u % QD], 0u);
          if (u == 3 || u == 7) sample_a(cst4);
        }
        refill(u % QD, u + QD < NB ? word_code<true>(wcur, u + QD) : word_code<true>(wnext, u + QD - NB));
      }
      wcur = wnext;
      // a candidate of the 3' op in this group?  The lane logs the group and walks on (see ItemLog)
      constexpr uint32_t kOr3 = 0xFEu;  // bitop3 truth table of a | b | c
      uint32_t any = __builtin_amdgcn_bitop3_b32((uint32_t)sc[0], (uint32_t)sc[1], (uint32_t)sc[2], kOr3);
      any = __builtin_amdgcn_bitop3_b32(any, (uint32_t)sc[3], (uint32_t)sc[4], kOr3);
      any = __builtin_amdgcn_bitop3_b32(any, (uint32_t)sc[5], (uint32_t)sc[6], kOr3);
      any |= (uint32_t)sc[7];
      if ((int)any < 0) {
        if (slot < slot_end) {
#pragma unroll
          for (int u = 0; u < NB; ++u) lds_write_u8(slot, (uint32_t)u, (uint32_t)sc[u]);
          lds_write_u8((slot >> 3) + il.tag_off, 0u, (uint32_t)(j >> 3));  // j = 8 g + 1
        }
        slot += 8u;  // (beyond the lane's slots: "too many", see below)
      }
      j += NB;
    };
    __builtin_amdgcn_s_setprio(PRIO_LOOP);
    const int early_groups = (ma + ka + NB - 1) >> 3;
    // two loops, not one with a switch inside: the two group bodies leave the five state registers in different
    // places, and a common loop head pays ten register moves per group to reconcile them
    // the quiet groups; behind them both scores come from the vertical deltas -- exact values, not bounds -- and the
    // last quiet column, the only one of them that T may admit, gets its 5' test
    const int quiet_j = (int)da.quiet_groups * NB + 1;  // the first column behind them
    if (quiet_j > 1) {
      do group(std::integral_constant<int, QUIET>{}, 0u);
      while (j < quiet_j && j + NB - 1 <= n);
      st.score = (int)__builtin_popcount(st.Pv) - (int)(__builtin_popcount(st.Mv) + (uint32_t)sh) - k1;
      if constexpr (HAS_A) {
        sa.score = (int)__builtin_popcount(sa.Pv) - (int)(__builtin_popcount(sa.Mv) + fill_a);
        const int tq = (int)(da.pair_tn[da.quiet_groups - 1u] >> 28);  // T + 1 of the last quiet column
        flag |= sa.score - (j == quiet_j ? tq : 0);  // (a read that ends before: T = -1 where it stopped)
      }
    }
    if constexpr (HAS_A) {
      // (g counts from the plan's constant, not from where a lane's quiet groups stopped: a lane that stopped early has
      // no whole group left, and a wave-uniform g keeps the group's T word and its nibbles on the scalar unit)
      int g = (int)da.quiet_groups;
      while (g < early_groups && j + NB - 1 <= n) {
        group(std::integral_constant<int, EARLY_G>{}, g == 0 ? tn0 : g == 1 ? tn1 : g == 2 ? tn2 : tn3);
        ++g;
      }
    }
    while (j + NB - 1 <= n) group(std::integral_constant<int, STEADY>{}, 0u);
    __builtin_amdgcn_s_setprio(PRIO_REST);
    // the up to NB - 1 columns behind the last whole group, as one more group of the lanes that have them (their
    // columns sit where each lane's walk stopped): the steps of both ops with exact scores, the 5' test per column,
    // and the 3' scores LOGGED like any other group's -- the book-keeping behind the loops takes them in column
    // order with the rest (it used to run here, column by column, in nearly every wave).  Columns beyond the
    // read's end log 0x7f: no candidate, never the lowest.  The masks of the first QD columns are in flight.
    if (j <= n) {
      int sc[NB];
#pragma unroll
      for (int u = 0; u < NB - 1; ++u) {
        sc[u] = 0x7f;
        if (j + u <= n) {
          uint32_t eb, ea;
          if (u < QD) {
            eb = qb[u];
            ea = qa[u];
          } else {
            const unsigned long long pr = lds_read_u64(word_code<true>(wcur, u));
            eb = (uint32_t)pr;
            ea = (uint32_t)(pr >> 32);
          }
          myers_step_la<false>(st, eb, 0u);
          sc[u] = st.score;
          if constexpr (HAS_A) {
            myers_step_la<false>(sa, ea, 0u);
            flag |= sa.score - tn_of(j + u);
          }
        }
      }
      sc[NB - 1] = 0x7f;
      int any = sc[0];
#pragma unroll
      for (int u = 1; u < NB - 1; ++u) any |= sc[u];  // (0x7f leaves the sign alone)
      if (any < 0) {
        if (slot < slot_end) {
#pragma unroll
          for (int u = 0; u < NB; ++u) lds_write_u8(slot, (uint32_t)u, (uint32_t)sc[u]);
          lds_write_u8((slot >> 3) + il.tag_off, 0u, (uint32_t)(j >> 3));
        }
        slot += 8u;
      }
      j = n + 1;
    }
    // ---- the logged groups, in column order: what the walk used to do inside every group
    {
      const uint32_t m80 = 0x80808080u, ones = 0x01010101u;
      const uint32_t stop_at = min(slot, slot_end);
      uint32_t rd = il.slot0;
      while (__ballot(rd < stop_at)) {
        if (rd < stop_at) {
          const unsigned long long sc8 = lds_read_u64(rd);
          const int jg = (int)lds_read_u8((rd >> 3) + il.tag_off) * 8 + 1;
          rd += 8u;
          // bytes hold D - (k + 1): candidates carry bit 7; flipped, every byte is D - (k + 1) + 128 >= 0, in order
          const uint32_t clo = (uint32_t)sc8 & m80, chi = (uint32_t)(sc8 >> 32) & m80;  // (never both zero: the lane logged a candidate)
          const uint32_t plo = (uint32_t)sc8 ^ m80, phi = (uint32_t)(sc8 >> 32) ^ m80;
          const unsigned long long c64 = ((unsigned long long)chi << 32) | clo;
          if (jfirst < 0) jfirst = jg + (__builtin_ctzll(c64) >> 3);
          jlast = jg + ((63 - __builtin_clzll(c64)) >> 3);
          // lowest score of the group: bytes -> 16-bit halves, packed minima
          const uint32_t h00ff = 0x00ff00ffu;
          const uint32_t a0 = plo & h00ff, a1 = (plo >> 8) & h00ff, b0 = phi & h00ff, b1 = (phi >> 8) & h00ff;
          const uint32_t m4 = pk_min_u16(pk_min_u16(a0, a1), pk_min_u16(b0, b1));
          const uint32_t gbyte = min(m4 & 0xffffu, m4 >> 16);  // lowest D - (k + 1) + 128 of the group
          const int gmin = (int)gbyte - 128 + k1;
          // (the column behind jmin, when jmin closed the group before this one)
          if (jmin == jg - 1 && (int)(plo & 0xffu) - 128 + k1 == cmin) tie_next = true;
          if (gmin < cmin) {  // strict: the first column that reaches the minimum
            const uint32_t gb = __builtin_amdgcn_perm(0u, gbyte, 0u);  // the minimum in every byte
            const uint32_t xlo = plo ^ gb, xhi = phi ^ gb;
            const uint32_t zlo = (xlo - ones) & ~xlo & m80, zhi = (xhi - ones) & ~xhi & m80;
            const int pos = __builtin_ctzll(((unsigned long long)zhi << 32) | zlo) >> 3;
            cmin = gmin;
            jmin = jg + pos;
            // the column behind it, inside this item (exact byte compare: the zero-byte masks above are only exact
            // for the lowest zero byte)
            const unsigned long long flipped = ((unsigned long long)phi << 32) | plo;
            tie_next = pos < 7 && (uint32_t)((flipped >> (8 * (pos + 1))) & 0xffull) == gbyte;
          }
        }
      }
      log_full = slot > slot_end;
    }
  } else {
    for (int pos = s; j <= n; ++j, ++pos) {  // reads shorter than a group
      const unsigned long long pr = lds_read_u64(row_code<true>(row, pos));
      column((uint32_t)pr, (uint32_t)(pr >> 32), j);
    }
  }
  CS_T_MARK(pt, 1);
  a_none = flag >= 0 && !log_full;  // (a full log: the caller treats the read like one the 5' test could not clear)
  st.score += k1;  // (back to D[m][n])
  const int exact_end = (exact_by_score && cmin == 0) ? jmin : -1;
  return myers_verdict<uint32_t, +1, true, true>(db, rule, fnib_b, row, s, e, st, jfirst, jlast, exact_end, cmin, jmin, tie_next);
}

// ---------------------------------------------------------------------------------
// Phase A == the whole answer for homopolymer adapters (cutseq/run.py:388-413, 673-716).
//
// poly-A TAIL (NonInternalBackAdapter: QUERY_START|REF_END, reference X^m).  Only cells of the
// last column are candidates.  With every reference base equal, a column either matches all
// rows (pure diagonal copy) or none, and on a non-matching column the recurrence always
// prefers the diagonal (cost_diag <= cost_deletion and <= cost_insertion hold with equality
// at worst, and ties go to the mismatch).  Hence cell (i, n) = (cost b_i, score i - 2 b_i,
// origin n - i), b_i = number of foreign bases among the last i; for i > n (reads shorter than
// the row) the diagonal ends in the first column: cost (i - n) + b_n, score n - 2 b_n, origin 0.
// ---------------------------------------------------------------------------------
// Foreign-base flags of one coded tile dword: bit 4b is set when base 8*di + b differs from the
// homopolymer base and lies inside [lo, hi).
__device__ __forceinline__ uint32_t foreign_flags(const uint32_t *row, int di, uint32_t xrep, int lo, int hi) {
  const uint32_t x = row[di] ^ xrep;
  const uint32_t t = (x | (x >> 1) | (x >> 2)) & 0x11111111u;
  const int first = max(lo - 8 * di, 0), last = min(hi - 8 * di, 8);
  const uint32_t upto = (last >= 8) ? 0xffffffffu : ((1u << (4 * last)) - 1u);
  return t & upto & ~((1u << (4 * first)) - 1u);
}

struct PolyBest {
  bool have;
  int origin, cost, score, len, where;
};

template <bool CODED>
__device__ __forceinline__ Verdict poly_tail(const DevOp &d, int rule, const uint32_t *row, int s, int e) {
  Verdict v = verdict_none(d.f.m);
  const int n = e - s, m = d.f.m, k = d.f.k, min_overlap = d.f.min_overlap;
  const uint32_t X = d.base_char;
  const int lim = min(n, m);
  PolyBest best = {false, 0, 0, 0, 0, 0};
  auto consider = [&](int i, int cost, int score, int origin) {
    if (i >= min_overlap && cost <= thr_of(d, i) &&
        better_candidate(rule, m, best.have, best.origin, best.cost, best.score, best.len, cost, score, origin, i)) {
      best.have = true;
      best.origin = origin;
      best.cost = cost;
      best.score = score;
      best.len = i;
    }
  };
  int b = 0, i_hi = 0;
  if (!CODED) {
    // raw tile: one base at a time
    for (int i = 1; i <= lim; ++i) {
      const int nb = b + ((row_code<CODED>(row, e - i) != X) ? 1 : 0);
      if (nb > k) break;
      b = nb;
      i_hi = i;
    }
  } else {
    // coded tile: eight bases per step with a popcount; the dword in which the budget k runs out is
    // walked base by base
    const uint32_t xrep = (X >> 3) * 0x11111111u;
    const int lo = e - lim;
    for (int di = (e - 1) >> 3; di >= (lo >> 3); --di) {
      const uint32_t f = foreign_flags(row, di, xrep, lo, e);
      const int c = __popc(f);
      const int seg_lo = max(lo, 8 * di);
      if (b + c <= k) {
        b += c;
        i_hi = e - seg_lo;
        continue;
      }
      for (int pos = min(e, 8 * di + 8) - 1; pos >= seg_lo; --pos) {
        const int nb = b + (int)((f >> (4 * (pos - 8 * di))) & 1u);
        if (nb > k) break;
        b = nb;
        i_hi = e - pos;
      }
      break;
    }
  }
  // rows longer than the read (only when the whole read is inside the budget)
  if (i_hi == n && n < m) {
    for (int i = m; i > n; --i) {
      const int cost = (i - n) + b;
      if (cost <= k) consider(i, cost, n - 2 * b, 0);
    }
  }
  // descending over the rows that fit into the read: i_hi, i_hi - 1, ..., 1
  if (!CODED) {
    for (int i = i_hi; i >= 1; --i) {
      consider(i, b, i - 2 * b, n - i);
      b -= (row_code<CODED>(row, e - i) != X) ? 1 : 0;
    }
  } else if (i_hi > 0) {
    // Rows are visited from the longest (i_hi) down, as cutadapt does, but only where a visit can
    // change the outcome: a row whose next-longer row merely adds a MATCHING base is never taken
    // (the longer row has the same cost, one more point and a threshold at least as high, and was
    // visited first; whether that one was taken, lost on score or lost on the overlap window, this
    // one loses too -- under either selection rule).  What remains are row i_hi and the rows that
    // start right after a foreign base: a real poly-A tail costs a handful of visits, not one per A.
    const uint32_t xrep = (X >> 3) * 0x11111111u;
    const int lo = e - i_hi;
    uint32_t carry = 0;  // the base just left of this dword's first base is foreign
    for (int di = lo >> 3; di <= ((e - 1) >> 3); ++di) {
      const uint32_t f = foreign_flags(row, di, xrep, lo, e);
      const int c = __popc(f);
      const int seg_lo = max(lo, 8 * di), seg_hi = min(e, 8 * di + 8);
      const int i_left = e - seg_lo;  // largest i of this dword (the most permissive threshold)
      // fewest foreign bases any row of this dword can have: the row that keeps only its last base
      const int b_min = b - c + (int)((f >> (4 * (seg_hi - 1 - 8 * di))) & 1u);
      if (i_left >= min_overlap && b_min <= thr_of(d, i_left)) {
        uint32_t visit = (f << 4) | carry;                     // left neighbour foreign
        if (seg_lo == lo) visit |= 1u << (4 * (lo - 8 * di));  // row i_hi itself
        const int nlo = seg_lo - 8 * di, nhi = seg_hi - 8 * di;
        visit &= 0x11111111u & (nhi >= 8 ? 0xffffffffu : ((1u << (4 * nhi)) - 1u)) & ~((1u << (4 * nlo)) - 1u);
        while (visit) {
          const int t = __builtin_ctz(visit);  // 4 * (pos - 8 di)
          visit &= visit - 1u;
          const int pos = 8 * di + (t >> 2);
          const int bi = b - __popc(f & ((1u << t) - 1u));  // foreign bases left of pos are not in the row
          const int i = e - pos;
          consider(i, bi, i - 2 * bi, n - i);
        }
      }
      b -= c;
      carry = (seg_hi == 8 * di + 8) ? ((f >> 28) & 1u) : 0u;
    }
  }
  if (best.have) {
    v.found = 1;
    v.qs = best.origin;
    v.qe = n;
  }
  return v;
}

// poly-T HEAD (NonInternalFrontAdapter: REF_START|QUERY_STOP, reference X^m).  Candidates are the
// cells (m, j).  For j <= m every row i >= j holds the same "deep" value (cost b_j, score
// j - 2 b_j, origin -(i - j)), b_j = foreign bases among the first j: the diagonal from the free
// first column wins every tie and the insertion from the row above can never be cheaper because
// every foreign base costs at least one.  Columns j > m (reads that start with >= m-k X's) leave
// the closed form: those reads go to the exact DP.
template <bool CODED>
__device__ __forceinline__ Verdict poly_head(const DevOp &d, int rule, const uint32_t *row, int s, int e) {
  Verdict v = verdict_none(d.f.m);
  const int n = e - s, m = d.f.m, k = d.f.k, min_overlap = d.f.min_overlap;
  const uint32_t X = d.base_char;
  const int lim = min(n, m);
  PolyBest best = {false, 0, 0, 0, 0, 0};
  auto consider = [&](int j, int cost) {
    const int score = j - 2 * cost, origin = j - m;
    if (j >= min_overlap && cost <= thr_of(d, j) &&
        better_candidate(rule, m, best.have, best.origin, best.cost, best.score, best.len, cost, score, origin, j)) {
      best.have = true;
      best.origin = origin;
      best.cost = cost;
      best.score = score;
      best.len = j;
      best.where = j;
    }
  };
  int b = 0;
  bool alive = true;
  if (!CODED) {
    for (int j = 1; j <= lim; ++j) {
      b += (row_code<CODED>(row, s + j - 1) != X) ? 1 : 0;
      if (b > k) {
        alive = false;
        break;
      }
      consider(j, b);
    }
  } else {
    // Columns are visited in cutadapt's order (ascending), skipping those that cannot matter: when
    // the NEXT base matches and is still inside the budget, column j + 1 has the same cost, one more
    // point, a threshold at least as high and is longer, so it is taken whenever j was (and judged
    // against the same previous best when j was not) -- the state after j + 1 is the same with or
    // without the visit to j, under either rule.  Left: columns followed by a foreign base, and
    // the last column inside the budget.
    const uint32_t xrep = (X >> 3) * 0x11111111u;
    const int hi = s + lim;
    for (int di = s >> 3; di <= ((hi - 1) >> 3) && alive; ++di) {
      const uint32_t f = foreign_flags(row, di, xrep, s, hi);
      const int c = __popc(f);
      const int seg_lo = max(s, 8 * di), seg_hi = min(hi, 8 * di + 8);
      const int j_hi = seg_hi - s;  // largest j of this dword (the most permissive threshold)
      const int b_min = b + (int)((f >> (4 * (seg_lo - 8 * di))) & 1u);  // fewest foreign bases of any j in here
      // first position of this dword at which the budget is exceeded (if any): nothing at or after it counts
      int pos_dead = seg_hi;
      if (b + c > k) {
        uint32_t g = f;
        for (int over = k - b; over > 0; --over) g &= g - 1u;  // drop the foreign bases still inside the budget
        pos_dead = 8 * di + (__builtin_ctz(g) >> 2);
      }
      if (j_hi >= min_overlap && b_min <= thr_of(d, j_hi) && b_min <= k) {
        // next base foreign: the flags of this dword shifted down one base, plus the first flag of the next dword
        uint32_t next_first = 0;
        if (seg_hi == 8 * di + 8 && seg_hi < hi) next_first = foreign_flags(row, di + 1, xrep, s, hi) & 1u;
        uint32_t visit = (f >> 4) | (next_first << 28);
        const int last = min(pos_dead, seg_hi) - 1;  // last column of this dword that is still alive
        if (last >= seg_lo && (pos_dead < seg_hi || seg_hi == hi)) visit |= 1u << (4 * (last - 8 * di));
        const int nlo = seg_lo - 8 * di, nhi = last + 1 - 8 * di;
        visit &= 0x11111111u & (nhi >= 8 ? 0xffffffffu : (nhi <= 0 ? 0u : ((1u << (4 * nhi)) - 1u))) & ~((1u << (4 * nlo)) - 1u);
        while (visit) {
          const int t = __builtin_ctz(visit);
          visit &= visit - 1u;
          const int pos = 8 * di + (t >> 2);
          const int bj = b + __popc(f & ((2u << t) - 1u));  // foreign bases up to and including pos
          consider(pos - s + 1, bj);
        }
      }
      b += c;
      if (b > k) alive = false;
    }
  }
  if (alive && n > m) {  // columns beyond m are reachable: not covered by the closed form
    int min_n, max_n;
    column_range(d.f.align_flags, m, k, n, min_n, max_n);
    v.need = 1;
    v.j0 = min_n;
    v.j1 = max_n;
    v.do_end = (max_n == n) ? 1 : 0;
    v.rmax = m;
    return v;
  }
  if (best.have) {
    v.found = 1;
    v.qs = 0;  // origin < 0 (or == 0 when j == m): the match starts at the first base
    v.qe = best.where;
  }
  return v;
}

// ---------------------------------------------------------------------------------
// Homopolymer ops on coded tiles, the fast way.  Hardly any read carries a poly-A/T stretch, but a wave
// pays for its slowest lane, so the closed forms above (kept for raw tiles) cost every wave the
// price of a real tail.  Instead:
//   1. every lane classifies its read from the 32 bases next to the anchored end -- straight-line code,
//      exact on those bases: "no row/column can be accepted and the error budget is spent" (the usual
//      case) settles the op; anything else is a maybe;
//   2. the wave serves its maybe-lanes one at a time: the 64 lanes fetch 64 bases of THAT read each,
//      one __ballot turns them into a bitmap of foreign bases, and the closed form runs on the bitmap
//      with wave-uniform values, i.e. on the scalar unit, beside the other waves' vector work.
// ---------------------------------------------------------------------------------
template <bool HEAD>
__device__ __forceinline__ bool poly_maybe(const DevOp &d, const uint32_t *row, int s, int e) {
  const int n = e - s, m = d.f.m, k = d.f.k, mo = d.f.min_overlap;
  const int lim = min(n, m);
  const uint32_t xrep = (d.base_char >> 3) * 0x11111111u;
  // four dwords = 32 bases from the anchored end; base number i (1-based from that end) sits in dword
  // (i - 1) >> 3, counted from the low nibble (head) or from the top nibble (tail)
  uint32_t F[4];
  int C[5];
  C[0] = 0;
  const int edge = HEAD ? s : e;
  const int w0 = edge >> 3;
  const uint32_t sh = (uint32_t)(edge & 7) * 4u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t w;
    if (HEAD)
      w = __builtin_amdgcn_alignbit(row[w0 + q + 1], row[w0 + q], sh);  // bases s + 8q ..
    else
      w = __builtin_amdgcn_alignbit(row[w0 - q], row[max(w0 - q - 1, -4)], sh);  // bases e - 8q - 8 .. e - 8q - 1
    const uint32_t x = w ^ xrep;
    uint32_t f = (x | (x >> 1) | (x >> 2)) & 0x11111111u;
    const int inside = lim - 8 * q;  // bases of this dword that exist
    if (inside < 8) {
      const uint32_t keep = inside <= 0 ? 0u : (HEAD ? ((1u << (4 * inside)) - 1u) : (~0u << (32 - 4 * inside)));
      f &= keep;
    }
    F[q] = f;
    C[q + 1] = C[q] + __popc(f);
  }
  bool maybe = C[4] <= k;  // budget not spent within 32 bases (or within the read): look closer
  // a row / column p can be accepted only if b_p <= thr[p]; b never falls and thr only moves at its step
  // positions, so the minimum of b - thr over any stretch sits at min_overlap or right at a step
  int pcheck = mo;
  const unsigned long long steps = d.thr_step[0];
  while (pcheck <= 32) {  // wave-uniform loop
    const int q = (pcheck - 1) >> 3, nib = ((pcheck - 1) & 7) + 1;
    const uint32_t fq = q == 0 ? F[0] : q == 1 ? F[1] : q == 2 ? F[2] : F[3];
    const int cq = q == 0 ? C[0] : q == 1 ? C[1] : q == 2 ? C[2] : C[3];
    const uint32_t upto = nib >= 8 ? ~0u : (HEAD ? ((1u << (4 * nib)) - 1u) : (~0u << (32 - 4 * nib)));
    const int b = cq + __popc(fq & upto);
    if (pcheck <= lim && b <= thr_of(d, pcheck)) maybe = true;
    const unsigned long long rest = pcheck < 64 ? (steps >> pcheck) : 0ull;  // bit i - 1 - pcheck: a step at i > pcheck
    if (!rest) break;
    pcheck += 1 + __builtin_ctzll(rest);
  }
  return maybe;
}

struct Mask128 {
  unsigned long long lo, hi;
};
__device__ __forceinline__ int m128_count_below(Mask128 a, int i) {  // set bits among [0, i)
  if (i <= 0) return 0;
  if (i < 64) return __popcll(a.lo & ((1ull << i) - 1ull));
  if (i == 64) return __popcll(a.lo);
  if (i < 128) return __popcll(a.lo) + __popcll(a.hi & ((1ull << (i - 64)) - 1ull));
  return __popcll(a.lo) + __popcll(a.hi);
}
__device__ __forceinline__ int m128_next(Mask128 a, int from) {  // lowest set bit >= from, 128 if none
  if (from < 64) {
    const unsigned long long x = a.lo & (~0ull << from);
    if (x) return __builtin_ctzll(x);
    from = 64;
  }
  if (from < 128) {
    const unsigned long long x = a.hi & (~0ull << (from - 64));
    if (x) return 64 + __builtin_ctzll(x);
  }
  return 128;
}
__device__ __forceinline__ int m128_prev(Mask128 a, int below) {  // highest set bit < below, -1 if none
  if (below > 64) {
    const unsigned long long x = below >= 128 ? a.hi : (a.hi & ((1ull << (below - 64)) - 1ull));
    if (x) return 127 - __builtin_clzll(x);
    below = 64;
  }
  if (below > 0) {
    const unsigned long long x = below >= 64 ? a.lo : (a.lo & ((1ull << below) - 1ull));
    if (x) return 63 - __builtin_clzll(x);
  }
  return -1;
}

// One read's homopolymer op, served by the whole wave (coded tiles).  Lane q looks at base number q from the
// anchored end (two rounds for adapters longer than 64): is it foreign, how many foreign bases sit in front of it
// (its rank), and could the row / column that stops right in front of it be accepted (q >= min_overlap and
// rank <= thr[q])?  Two ballots per round leave the foreign bitmap `fm` and the bitmap `am` of acceptable stops.
// Only stops in front of a foreign base and the longest stop inside the budget can change the outcome
// (poly_tail / poly_head above), and of those only the acceptable ones -- usually one or two -- are then
// visited in cutadapt's order with wave-uniform values, i.e. on the scalar unit.
struct PolyMaps {
  Mask128 fm, am;
  int total;  // foreign bases among the first lim (exact while <= k; counting stops once the budget is spent)
};
__device__ __forceinline__ PolyMaps poly_maps(const DevOp &d, const uint32_t *lrow, bool head, int ls, int le, int lane) {
  const int lim = min(le - ls, (int)d.f.m), mo = d.f.min_overlap;
  const uint32_t xnib = d.base_char >> 3;
  PolyMaps pm = {{0ull, 0ull}, {0ull, 0ull}, 0};
  // (a stop behind more than k foreign bases is never acceptable: no second round once the budget is spent)
  for (int half = 0; half * 64 < lim && pm.total <= (int)d.f.k; ++half) {
    const int q = half * 64 + lane;
    const int pos = head ? (ls + q) : (le - 1 - q);
    bool foreign = false;
    if (q < lim) foreign = ((lrow[pos >> 3] >> ((pos & 7) * 4)) & 7u) != xnib;
    const unsigned long long bits = __ballot(foreign);
    const int rank = pm.total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bits, 0u));
    const unsigned long long acc = __ballot(foreign && q >= mo && rank <= thr_of(d, q));
    if (half == 0) {
      pm.fm.lo = bits;
      pm.am.lo = acc;
    } else {
      pm.fm.hi = bits;
      pm.am.hi = acc;
    }
    pm.total += __popcll(bits);
  }
  return pm;
}

// poly-T head (bit q of fm: base s + q is foreign, q < lim).  Columns are visited in ascending order, so a
// later candidate is always longer: it replaces the best exactly when it scores more, under either selection
// rule.  Candidates: the column in front of every foreign base, then the last column if the budget lasts.
__device__ __forceinline__ Verdict poly_head_wave(const DevOp &d, const PolyMaps &pm, int n) {
  Verdict v = verdict_none(d.f.m);
  const int m = d.f.m, k = d.f.k, mo = d.f.min_overlap;
  const int lim = min(n, m);
  bool have = false;
  int best_score = 0, best_j = 0;
  for (int j = m128_next(pm.am, 0); j < 128; j = m128_next(pm.am, j + 1)) {
    const int score = j - 2 * m128_count_below(pm.fm, j);
    if (!have || score > best_score) {
      have = true;
      best_score = score;
      best_j = j;
    }
  }
  const bool alive = pm.total <= k;  // the scan reaches the last column without running out of budget
  if (alive && lim >= mo && pm.total <= thr_of(d, lim)) {
    const int score = lim - 2 * pm.total;
    if (!have || score > best_score) {
      have = true;
      best_score = score;
      best_j = lim;
    }
  }
  if (alive && n > m) {  // columns beyond m are reachable: not covered by the closed form
    int min_n, max_n;
    column_range(d.f.align_flags, m, k, n, min_n, max_n);
    v.need = 1;
    v.j0 = min_n;
    v.j1 = max_n;
    v.do_end = (max_n == n) ? 1 : 0;
    v.rmax = m;
    return v;
  }
  if (have) {
    v.found = 1;
    v.qs = 0;
    v.qe = best_j;
  }
  return v;
}

// poly-A tail (bit q of fm: base e - 1 - q is foreign, q < lim).  Rows are visited from the longest one inside
// the budget down, as cutadapt does: rows longer than the read, the whole stretch if the budget lasts, then
// the acceptable rows that start right behind a foreign base.
__device__ __forceinline__ Verdict poly_tail_wave(const DevOp &d, int rule, const PolyMaps &pm, int n) {
  Verdict v = verdict_none(d.f.m);
  const int m = d.f.m, k = d.f.k, mo = d.f.min_overlap;
  const int lim = min(n, m);
  PolyBest best = {false, 0, 0, 0, 0, 0};
  auto consider = [&](int i, int cost, int score, int origin) {
    if (i >= mo && cost <= thr_of(d, i) &&
        better_candidate(rule, m, best.have, best.origin, best.cost, best.score, best.len, cost, score, origin, i)) {
      best.have = true;
      best.origin = origin;
      best.cost = cost;
      best.score = score;
      best.len = i;
    }
  };
  const int b = pm.total;
  if (b <= k) {  // the whole stretch is inside the budget
    if (n < m)   // rows longer than the read
      for (int i = min(m, n + k - b); i > n; --i) consider(i, (i - n) + b, n - 2 * b, 0);
    consider(lim, b, lim - 2 * b, n - lim);
  }
  for (int i = m128_prev(pm.am, 128); i >= 0; i = m128_prev(pm.am, i)) {
    const int bi = m128_count_below(pm.fm, i);
    consider(i, bi, i - 2 * bi, n - i);
  }
  if (best.have) {
    v.found = 1;
    v.qs = best.origin;
    v.qe = n;
  }
  return v;
}

// ---------------------------------------------------------------------------------
// Phase B: exact (cost, score, origin) DP over query columns (j0, j1], reference rows
// 0..rmax, column in LDS (c0[i * cstride]), cells saturated to DEAD above k errors.
// A window that starts after the aligner's first column is seeded with "row 0 alive,
// everything else dead": every cell with true cost <= k whose alignment starts inside the
// window comes out bit-identical (costs can only grow, ties break the same way), and the
// filter guarantees all candidate cells have their whole alignment inside the window.
// EQ: 0 = adapter bases from memory, 1 = 32-bit match masks, 2 = 64-bit match masks.
// Returns found << 31 | query_start << 16 | query_stop.
// ---------------------------------------------------------------------------------
template <int EQ, bool CODED>
__device__ uint32_t exact_dp(const DevOp &d, const char *tab, int rule, bool tie_ins, const uint32_t *row, int s,
                             int e, int j0, int j1, int do_end, int rmax, uint32_t *c0, int cstride) {
  const DevFields &op = d.f;
  const int m = op.m, k = op.k, flags = op.align_flags, min_overlap = op.min_overlap;
  const bool RS = flags & CS_REF_START, QS = flags & CS_QUERY_START;
  const bool RE = flags & CS_REF_END, QSTOP = flags & CS_QUERY_STOP;
  const bool reversed = op.reversed;
  const int n = e - s;
  int min_n, max_n;
  column_range(flags, m, k, n, min_n, max_n);
  const uint32_t dead = ((uint32_t)(k + 1) << kCostShift) | kCellZero;
  const uint32_t live_limit = (uint32_t)(k + 1) << kCostShift;  // cell < live_limit  <=>  cost <= k
  const uint64_t pA = d.peq[0], pC = d.peq[1], pG = d.peq[2], pT = d.peq[3];

  // ---- first column
  int last;  // rows 1..last are computed per column (Ukkonen), rows above hold DEAD
  if (j0 == min_n) {
    int lastlive = -1;
    for (int i = 0; i <= rmax; ++i) {
      int cost, origin;
      if (!RS && !QS) {
        cost = max(i, min_n);
        origin = 0;
      } else if (RS && !QS) {
        cost = min_n;
        origin = min(0, min_n - i);
      } else if (!RS && QS) {
        cost = i;
        origin = max(0, min_n - i);
      } else {
        cost = min(i, min_n);
        origin = min_n - i;
      }
      const bool alive = cost <= k;
      c0[i * cstride] = alive ? cell_pack(cost, 0, origin) : dead;
      if (alive) lastlive = i;
    }
    last = min(rmax, lastlive + 1);
  } else {
    c0[0] = cell_pack(0, 0, j0);  // only reachable with QUERY_START
    for (int i = 1; i <= rmax; ++i) c0[i * cstride] = dead;
    last = min(rmax, 1);
  }

  bool have = false;
  int b_origin = 0, b_cost = 0, b_score = 0, b_refstop = m, b_qstop = n;
  bool broke = false;

  for (int j = j0 + 1; j <= j1; ++j) {
    const int pos = reversed ? (e - j) : (s + j - 1);
    const uint32_t qc = row_code<CODED>(row, pos);
    uint64_t eqmask = 0;
    if (EQ == 1)
      eqmask = eq_lookup<uint32_t, CODED>(qc, tab, (uint32_t)pA, (uint32_t)pC, (uint32_t)pG, (uint32_t)pT);
    else if (EQ == 2)
      eqmask = eq_lookup<uint64_t, CODED>(qc, tab, pA, pC, pG, pT);
    uint32_t diag = c0[0];
    uint32_t up;
    if (QS) {
      up = cell_pack(0, 0, j);
    } else {
      up = (j <= k) ? ((diag & ~(0xffu << kCostShift)) | ((uint32_t)j << kCostShift)) : dead;
    }
    c0[0] = up;
    int lastlive = (up < live_limit) ? 0 : -1;
    uint32_t left = (last >= 1) ? c0[cstride] : dead;
    for (int i = 1; i <= last; ++i) {
      // next row's cell of the previous column is requested before this row's arithmetic
      const uint32_t left_next = c0[min(i + 1, rmax) * cstride];
      bool eq;
      if (EQ == 1)
        eq = ((uint32_t)eqmask >> (i - 1)) & 1u;
      else if (EQ == 2)
        eq = (eqmask >> (i - 1)) & 1ull;
      else
        eq = (uint32_t)d.op.seq[i - 1] == qc;
      const uint32_t r = dp_cell(diag, left, up, eq, live_limit, dead, tie_ins);
      c0[i * cstride] = r;
      diag = left;
      up = r;
      left = left_next;
      if (r < live_limit) lastlive = i;
    }
    const bool at_full_row = (last == m) && (lastlive == m);
    last = min(rmax, lastlive + 1);
    if (at_full_row && QSTOP) {
      const int cost = cell_cost(up), score = cell_score(up), origin = cell_origin(up);
      const int length = m + min(origin, 0);
      const bool ok = length >= min_overlap && cost <= thr_of(d, length);
      const int b_length = m + min(b_origin, 0);
      if (ok && better_candidate(rule, m, have, b_origin, b_cost, b_score, b_length, cost, score, origin, length)) {
        have = true;
        b_origin = origin;
        b_cost = cost;
        b_score = score;
        b_refstop = m;
        b_qstop = j;
        if (cost == 0 && origin >= 0) {
          broke = true;
          break;
        }
      }
    }
  }

  if (do_end && !broke && j1 == n && max_n == n) {
    const int first_i = RE ? 0 : m;
    for (int i = min(m, rmax); i >= first_i; --i) {
      const uint32_t c = c0[i * cstride];
      if (c >= live_limit) continue;
      const int cost = cell_cost(c), score = cell_score(c), origin = cell_origin(c);
      const int length = i + min(origin, 0);
      if (length < min_overlap || length < 0) continue;
      if (cost > thr_of(d, length)) continue;
      const int b_length = b_refstop + min(b_origin, 0);
      if (better_candidate(rule, m, have, b_origin, b_cost, b_score, b_length, cost, score, origin, length)) {
        have = true;
        b_origin = origin;
        b_cost = cost;
        b_score = score;
        b_refstop = i;
        b_qstop = n;
      }
    }
  }
  const uint32_t qs = (uint32_t)(b_origin >= 0 ? b_origin : 0);
  return ((have ? 1u : 0u) << 31) | (qs << 16) | (uint32_t)b_qstop;
}

// LDS traffic between lanes of ONE wave: the LDS executes a wave's instructions in order, so
// only the compiler has to be kept from moving accesses across this point.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------
// Phase B, cooperative form for adapters with m <= 32 (the common case): FOUR lanes share
// one survivor.  Lane g of the group owns the strip of H reference rows g*H+1 .. g*H+H and
// keeps its cells in registers; the groups sweep the window along anti-diagonals (lane g is
// g columns behind lane g-1) and pass the strip's bottom cell to the next lane with one DPP
// row shift per step.  Sixteen survivors run side by side in a wave, no LDS column, no
// Ukkonen bookkeeping (every cell is computed, DEAD saturation keeps the arithmetic the same).
// The lane that owns the last row runs cutadapt's candidate selection in column order, then
// the end-of-read scan over the final column (parked in LDS).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t dpp_row_shr1(uint32_t v) {
  // (bound_ctrl: lane 0 of a row reads 0 -- no register to pre-load; it is a top strip and ignores what it receives)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
}

template <int G, int H, bool CODED, bool TIE_INS>
__device__ void strip_dp_pass(const DevOp &d, const char *tab, int rule, const uint32_t *wave_rows,
                              uint32_t lds_stride_dw, uint32_t *wq, uint32_t *fin, int fin_stride, int base, int qn,
                              int lane CS_T_PARAM) {
  static_assert(G == 4 || G == 8 || G == 16, "lanes per survivor: a power of two inside a 16-lane DPP row");
  constexpr int GSHIFT = (G == 4) ? 2 : (G == 8) ? 3 : 4;
  const DevFields &op = d.f;
  const int m = op.m, k = op.k, flags = op.align_flags, min_overlap = op.min_overlap;
  const bool RS = flags & CS_REF_START, QS = flags & CS_QUERY_START;
  const bool RE = flags & CS_REF_END, QSTOP = flags & CS_QUERY_STOP;
  const bool reversed = op.reversed;
  const uint32_t dead = ((uint32_t)(k + 1) << kCostShift) | kStripZero;
  const uint32_t live_limit = (uint32_t)(k + 1) << kCostShift;
  const uint32_t pA = (uint32_t)d.peq[0], pC = (uint32_t)d.peq[1], pG = (uint32_t)d.peq[2], pT = (uint32_t)d.peq[3];

  const int g = lane & (G - 1), slot = lane >> GSHIFT, idx = base + slot;
  const bool active = idx < qn;
  uint32_t i0 = 0, i1 = 0, i2 = 0, i3 = 0;
  if (active) {
    const uint32_t *it = wq + idx * kWaveItemDwords;
    i0 = it[0];
    i1 = it[1];
    i2 = it[2];
    i3 = it[3];
  }
  const int r = (int)(i0 & 0xffffu), j0 = (int)(i0 >> 16);
  const int j1 = (int)(i1 & 0x7fffu), do_end = (int)((i1 >> 15) & 1u), rmax = (int)(i1 >> 16);
  const int s = (int)(i2 & 0xffffu), e = (int)(i2 >> 16);
  const int n = e - s;
  int min_n, max_n;
  column_range(flags, m, k, n, min_n, max_n);
  const uint32_t *rrow = wave_rows + (size_t)r * lds_stride_dw;
  const int rb = g * H;                           // rows rb+1 .. rb+H live in this lane
  const int top = min(m, rmax);                   // last row that matters
  const int owner = (top - 1) / H;                // lane that sees row `top` (and row m when rmax == m)
  const int hm = (m - 1) - owner * H;             // register index of row m inside the owner strip
  const bool works = active && rb < top;
  const int ncols = works ? (j1 - j0) : 0;

  // first column of the window
  const bool true_init = (j0 == min_n);
  uint32_t L[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const int i = rb + h + 1;
    int cost, origin;
    if (!RS && !QS) {
      cost = max(i, min_n);
      origin = 0;
    } else if (RS && !QS) {
      cost = min_n;
      origin = min(0, min_n - i);
    } else if (!RS && QS) {
      cost = i;
      origin = max(0, min_n - i);
    } else {
      cost = min(i, min_n);
      origin = min_n - i;
    }
    L[h] = (true_init && cost <= k && i <= rmax) ? strip_pack(cost, 0, origin) : dead;
  }
  // cell (rb, j0): what this strip sees diagonally above its first row at the first column
  uint32_t prev_recv;
  {
    const int i = rb;
    int cost, origin;
    if (!RS && !QS) {
      cost = max(i, min_n);
      origin = 0;
    } else if (RS && !QS) {
      cost = min_n;
      origin = min(0, min_n - i);
    } else if (!RS && QS) {
      cost = i;
      origin = max(0, min_n - i);
    } else {
      cost = min(i, min_n);
      origin = min_n - i;
    }
    prev_recv = (true_init && cost <= k) ? strip_pack(cost, 0, origin) : dead;
  }
  uint32_t bottom = dead;

  bool have = false, broke = false;
  int b_origin = 0, b_cost = 0, b_score = 0, b_refstop = m, b_qstop = n;

  const int steps = ncols > 0 ? ncols + owner : 0;  // lane `owner` is the last one that matters
  // row 0 in closed form: free query start -> (0, 0, j); anchored -> (j, 0, 0) while j <= k
  auto row0 = [&](int j) -> uint32_t {
    if (QS) return kStripZero + (uint32_t)j;  // wave-uniform branch
    return (j <= k) ? (((uint32_t)j << kCostShift) | kStripZero) : dead;
  };
  const bool is_top = (g == 0);
  const bool is_owner = (g == owner) && (rmax == m) && QSTOP;
  // the match mask of a lane's next column is fetched one step ahead (two dependent LDS reads);
  // the lane's read position advances by one base per step
  const int pstep = reversed ? -1 : 1;
  int pnext = reversed ? (e - (j0 + 1 - g)) : (s + (j0 + 1 - g) - 1);
  // no clamping: a lane's position leaves [s, e) only while its column is outside the window (at
  // most G - 1 bases either side), the mask fetched there is never used, and the read stays inside
  // the block's LDS (the tile starts 16 bytes into it, rows are contiguous, scratch follows)
  auto fetch_eq = [&]() -> uint32_t {
    const int pos = pnext;
    pnext += pstep;
    return eq_lookup<uint32_t, CODED>(row_code<CODED>(rrow, pos), tab, pA, pC, pG, pT) >> rb;
  };
  // insertion (from the row above) against deletion (from the column before): TIE_INS = the insertion wins a tie
  // (cs_params.indel_tie); the diagonal wins every tie (priority 0)
  uint32_t v_match = kDeltaMatch, v_mis = kDeltaMismatch;
  uint32_t v_up = kDeltaIndel + ((TIE_INS ? 1u : 2u) << kStripPrioShift);
  uint32_t v_left = kDeltaIndel + ((TIE_INS ? 2u : 1u) << kStripPrioShift);
  uint32_t v_clear = ~(3u << kStripPrioShift);
  asm volatile("" : "+v"(v_match), "+v"(v_mis), "+v"(v_up), "+v"(v_left), "+v"(v_clear));
  uint32_t eq_next = (steps > 0) ? fetch_eq() : 0u;
  // what this lane saw above its first row one column ago: row 0 for the top strip, the
  // neighbour's bottom cell otherwise
  uint32_t prev_up = is_top ? row0(j0) : prev_recv;
  // full-adapter candidates can only sit in columns the filter flagged: the window starts m + k
  // columns before the first of them whenever it does not start at the aligner's first column
  const int j_cand = true_init ? 0 : j0 + m + k;
  int c = -g, j = j0 + 1 - g;
  CS_T_MARK(pt, 3);
#ifdef CS_PHASE_TIMERS
  {
    int smax = steps;
    for (int o = 32; o > 0; o >>= 1) smax = max(smax, __shfl_xor(smax, o, 64));
    pt.steps += (uint32_t)smax;
    pt.passes += 1;
    pt.items += (uint32_t)min(qn - base, 64 / G);
  }
#endif
  for (int t = 0; t < steps; ++t, ++c, ++j) {
    const uint32_t recv = dpp_row_shr1(bottom);
    const uint32_t eqs = eq_next;
    eq_next = fetch_eq();
    if ((uint32_t)c < (uint32_t)ncols) {
      uint32_t up = is_top ? row0(j) : recv;
      uint32_t diag = prev_up;
      prev_up = up;
      // H cells, each the unsigned minimum of its three candidates: the cost sits in the top byte, and the two
      // bits under it rank the candidates of EQUAL cost the way cutadapt's recurrence does (diagonal first, then
      // the indel cs_params.indel_tie prefers) before score or origin can have a say.  A match cell goes through the
      // same minimum, where cutadapt takes its diagonal + 0 outright.  That is not because the diagonal is never dearer
      // than an indel everywhere: beside the first column of a window that starts late (true_init false, j0 > min_n:
      // row 0 is 0 there, rows >= 1 are held dead at k + 1) the neighbours are only upper bounds, and a match cell can
      // take up + 1 and stay live where cutadapt would take the dead diagonal.  The argument is this: every cell on a
      // path of cost at most k to a candidate the window reports has exact neighbours, and there the diagonal + 0 is
      // the minimum and wins the ties; every other cell only needs to be an upper bound of its true cost, which a
      // minimum of upper bounds is.  Dead cells (cost > k) are NOT clamped to a canonical one: a cell at most
      // k is the minimum over candidates from cells at most k (costs never fall along a path), so what the dead
      // ones hold changes no live cell, aliveness is always tested as "< live_limit", and the fields cannot overflow:
      // cost <= row 0's cost + i <= k + 1 + 32 (the insertion from above is always a candidate), so score >= -2 cost
      // stays inside its nine bits.
      // What hangs on the previous column only comes first (no chain between the cells), then the chain down the
      // strip: add, minimum, and per cell -- and the new cells can take the old ones' registers.
      uint32_t ca[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const uint32_t eqm = (uint32_t)__builtin_amdgcn_sbfe((int)eqs, h, 1);
        ca[h] = (h == 0 ? diag : L[h - 1]) + sel_mask(eqm, v_match, v_mis);
      }
      // (the rest written out so that a new cell lands in the register of the old one: the compiler's own choice
      // put it elsewhere and copied H + 1 registers back at the end of every step)
#pragma unroll
      for (int h = 0; h < H; ++h) asm("v_add_u32_e32 %0, %0, %1" : "+v"(L[h]) : "v"(v_left));
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const uint32_t cb = up + v_up;
        asm("v_min3_u32 %0, %1, %2, %0\n\tv_and_b32_e32 %0, %0, %3" : "+v"(L[h]) : "v"(ca[h]), "v"(cb), "v"(v_clear));
        up = L[h];
      }
      bottom = up;
      if (is_owner && !broke && j >= j_cand) {
        uint32_t cand = L[H - 1];
        if (hm != H - 1) {  // wave-uniform
          cand = L[0];
#pragma unroll
          for (int h = 1; h < H; ++h) cand = (h == hm) ? L[h] : cand;
        }
        if (cand < live_limit) {
          const int cost = cell_cost(cand), score = strip_score(cand), origin = cell_origin(cand);
          bool take;
          if (!RS) {
            // origin >= 0: the aligned length is m, "cost <= thr[m]" is "cell alive", and the
            // longer-match clause of the selection rule can never fire
            take = !have || ((rule == CS_SELECT_SCORE) ? (score > b_score || (score == b_score && cost < b_cost))
                                                       : (origin <= b_origin + m / 2 && score > b_score));
          } else {
            const int length = m + min(origin, 0);
            const bool ok = length >= min_overlap && cost <= thr_of(d, length);
            const int b_length = m + min(b_origin, 0);
            take = ok && better_candidate(rule, m, have, b_origin, b_cost, b_score, b_length, cost, score, origin, length);
          }
          if (take) {
            have = true;
            b_origin = origin;
            b_cost = cost;
            b_score = score;
            b_refstop = m;
            b_qstop = j;
            if (cost == 0 && origin >= 0) broke = true;
          }
        }
      }
    }
  }

  CS_T_MARK(pt, 7);
  // final column -> LDS, then the owner lane walks it from the last row upwards
  const bool scan = do_end && j1 == n && max_n == n;
  if (works && scan) {
#pragma unroll
    for (int h = 0; h < H; ++h)
      if (rb + h + 1 <= top) fin[slot * fin_stride + rb + h + 1] = L[h];
  }
  wave_lds_fence();
  if (works && g == owner) {
    if (scan && !broke) {
      const int first_i = RE ? 1 : m;  // row 0 has length 0 and can never be accepted
      // rows first_i..top, from the top, restricted to the ones the filter found acceptable (i3)
      uint32_t todo = i3 & (top >= 32 ? 0xffffffffu : ((1u << top) - 1u)) & ~((1u << (first_i - 1)) - 1u);
      while (todo) {
        const int i = 32 - __builtin_clz(todo);
        todo &= ~(1u << (i - 1));
        const uint32_t c = fin[slot * fin_stride + i];
        if (c >= live_limit) continue;
        const int cost = cell_cost(c), score = strip_score(c), origin = cell_origin(c);
        const int length = i + min(origin, 0);
        if (length < min_overlap || length < 0) continue;
        if (cost > thr_of(d, length)) continue;
        const int b_length = b_refstop + min(b_origin, 0);
        if (better_candidate(rule, m, have, b_origin, b_cost, b_score, b_length, cost, score, origin, length)) {
          have = true;
          b_origin = origin;
          b_cost = cost;
          b_score = score;
          b_refstop = i;
          b_qstop = n;
        }
      }
    }
    const uint32_t qs = (uint32_t)(b_origin >= 0 ? b_origin : 0);
    wq[idx * kWaveItemDwords + 3] = ((have ? 1u : 0u) << 31) | (qs << 16) | (uint32_t)b_qstop;
  }
  wave_lds_fence();
}

// Sum over the wave, in every lane's SGPR: four row_shr steps leave each row of 16 lanes' sum in its last
// lane, row_bcast15 / row_bcast31 carry the row sums up to lane 63 -- six DPP adds, no LDS round trips.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x112 /* row_shr:2 */, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114 /* row_shr:4 */, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118 /* row_shr:8 */, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142 /* row_bcast:15 */, 0xa, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143 /* row_bcast:31 */, 0xc, 0xf, true);
  return (uint32_t)__builtin_amdgcn_readlane(x, 63);
}
// The lane's index in a block of one wave, computed where it is needed: two instructions on the execution-mask
// counters (their start value hidden from the optimiser, or the result is hoisted and lives on).  The scan kernel
// uses it instead of threadIdx.x, which would occupy a register from the first tile to the last.
__device__ __forceinline__ uint32_t wave_lane_fresh() {
  uint32_t zero = 0u;
  asm volatile("" : "+v"(zero));
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
}
__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// One lane's atomicAdd on a wave-uniform address whose answer is looked at LATER (the tile and queue reservations).
// On a uniform address the compiler's atomic optimiser rewrites the call for "any number of lanes": one lane adds the
// wave's total and the old value is broadcast with v_readfirstlane right behind the atomic -- a wait for the whole
// round trip to L2 (a microsecond or two) where the design meant none.  An address the optimiser cannot prove uniform
// stays a plain atomic; the wait lands where the answer is used.
__device__ __forceinline__ uint32_t atomic_add_later(uint32_t *p, uint32_t v) {
  uint32_t zero = 0;
  asm volatile("" : "+v"(zero));
  return atomicAdd(p + zero, v);
}


// stats slots inside one mate's cs_stats (u64 words)
enum { ST_READS = 0, ST_IN_BP, ST_OUT_BP, ST_QTRIM_BP, ST_TOO_SHORT, ST_UNTRIMMED, ST_EXACT_DP, ST_RESERVED, ST_OPS };
constexpr int ST_TOO_MANY_N = ST_OPS + CS_MAX_OPS;  // cs_stats.n_too_many_n, behind op_matched[]
constexpr int kStatWords = ST_TOO_MANY_N + 1;
static_assert(sizeof(cs_stats) == kStatWords * 8, "cs_stats layout");
// The per-mate counts of the other CS_X_* bits lie behind the two cs_stats (cs_stats itself and the LDS accumulators
// keep their size): word kXStatBase + mate * kXStatWords + XST_*; cs_xflag_counts_fetch reads them.
enum { XST_TOO_LONG = 0, XST_TOO_MANY_EE, kXStatWords };
constexpr int kXStatBase = 2 * kStatWords;
// ... and behind those the bases CS_OP_POLYA ops removed, one word per mate (cs_polya_bp_fetch)
constexpr int kPolyABase = kXStatBase + 2 * kXStatWords;
constexpr int kStatsBlockWords = kPolyABase + 2;

// ---- TooManyN (cs_plan_set_max_n, cutadapt --max-n): 'N' / 'n' bases in [s, e) of a row, and the filter's rule.
// Raw bytes (ASCII rows in HBM, or a raw tile: its case folding only turns 'n' into 'N'): exact zero-byte test on
// byte ^ 'N' with bit 5 cleared.
__device__ __forceinline__ uint32_t count_n_bytes(const uint32_t *row, int s, int e) {
  uint32_t n = 0;
  if (e <= s) return 0;
  const int d0 = s >> 2, d1 = (e - 1) >> 2;
  for (int d = d0; d <= d1; ++d) {
    uint32_t keep = 0x80808080u;
    if (d == d0) keep &= 0x80808080u << ((s & 3) * 8);
    if (d == d1) keep &= 0x80808080u >> ((3 - ((e - 1) & 3)) * 8);
    const uint32_t x = (row[d] & 0xdfdfdfdfu) ^ 0x4e4e4e4eu;
    n += (uint32_t)__popc(~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & keep);
  }
  return n;
}
// A coded tile of the FAST form (every byte vouched to be A, C, G, T or N): code 7 is 'N' and nothing else, eight
// three-bit codes per dword -- the bits of a nibble ANDed together, one popcount.  (Not on exact-form tiles: IUPAC codes
// and 'n' under CS_CASE_SENSITIVE land in 4..7 there.)
__device__ __forceinline__ uint32_t count_n_nibbles(const uint32_t *row, int s, int e) {
  uint32_t n = 0;
  if (e <= s) return 0;
  const int d0 = s >> 3, d1 = (e - 1) >> 3;
  for (int d = d0; d <= d1; ++d) {
    uint32_t keep = 0x11111111u;
    if (d == d0) keep &= 0x11111111u << ((s & 7) * 4);
    if (d == d1) keep &= 0x11111111u >> ((7 - ((e - 1) & 7)) * 4);
    const uint32_t w = row[d];
    n += (uint32_t)__popc(w & (w >> 1) & (w >> 2) & keep);
  }
  return n;
}
// cutadapt TooManyN: a count below 1 is a proportion of the read's length (IEEE double division, strict >; an empty
// read is kept), any other count a number of bases
__device__ __forceinline__ bool too_many_n(uint32_t n, int len, double count) {
  if (count < 1.0) return len > 0 && (double)n / (double)len > count;
  return (double)n > count;
}
// cutadapt TooManyExpectedErrors: e = 0.0; for every quality byte of [s, e), left to right: e += table[byte].  One lane
// per read and one IEEE double add per base, in index order: the filter compares this sum with strict >, so a tree or
// a wave reduction (another rounding order) would decide reads at the threshold differently.  There is nothing to fuse
// (no multiply) and the build has no fast-math, so the adds stay as written; a byte outside [s, e) of the first or
// last dword adds nothing (not +0.0 either).  qrow: the read's quality row in HBM, dword-aligned.  reversed
// (wave-uniform, cs_plan_set_ee_reversed): the caller writes the read reverse-complemented, so "left to right" in the
// read cutadapt's filter sees is e - 1 down to s here.
__device__ __forceinline__ double expected_errors(const uint32_t *qrow, int s, int e, const double *table, bool reversed) {
  double ee = 0.0;
  if (e <= s) return ee;
  const int d0 = s >> 2, d1 = (e - 1) >> 2;
  if (!reversed) {
    for (int d = d0; d <= d1; ++d) {
      const uint32_t w = qrow[d];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int p = 4 * d + b;
        if (p >= s && p < e) ee += table[(w >> (8 * b)) & 0xffu];
      }
    }
  } else {
    for (int d = d1; d >= d0; --d) {
      const uint32_t w = qrow[d];
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        const int p = 4 * d + b;
        if (p >= s && p < e) ee += table[(w >> (8 * b)) & 0xffu];
      }
    }
  }
  return ee;
}

// ---------------------------------------------------------------------------------
// Two kernels, one body.
//
//   MODE_SCAN     persistent waves over tiles of 64 consecutive reads: stage, pre-filters, closed
//                 forms, cuts, quality trimming.  A read whose adapter op needs the exact DP is
//                 DEFERRED: its chain state and the DP window go into a 32-byte record of the mate's
//                 queue in HBM (one atomic per tile) and the lane drops out of the tile.  No DP code,
//                 no DP scratch in LDS.
//   MODE_RESOLVE  persistent waves over batches of 64 queue records: gather those reads' rows into
//                 the LDS tile, run the strip DP on FULL passes (16 survivors x 4 lanes, every lane
//                 busy; a scan tile on its own fills half a pass on average and still pays for a
//                 whole one), then every lane resumes its read's chain behind the deferring op.
//                 Later ops of the chain that need the DP again are served inside the wave.
//
// The resolve kernel is launched behind the scan kernel on the same stream and reads the record
// count the scan kernel left in memory.
// ---------------------------------------------------------------------------------
enum { MODE_SCAN = 0, MODE_RESOLVE = 1 };

// WIDE: the plan has an ACGT adapter of 33..64 bases (64-bit bit-vectors); plans without one get
// a kernel without that code, which needs far fewer registers.
// Scan kernel at 5 waves/SIMD (96 VGPRs, 13 spilled).  6 waves/SIMD (80 VGPRs) measured 2 % faster but
// spills ~45 VGPRs to scratch and nearly doubles the kernel's HBM traffic (DESIGN.md section 2).
#ifndef CS_SCAN_WAVES
#define CS_SCAN_WAVES 5  // diagnostic builds: -DCS_SCAN_WAVES=6 / 7 (tools/lean_probe.sh)
#endif
// FILT: the filters of the final interval this instantiation decides.  0: none (the code every plan without a filter
// runs); 1: TooManyN alone (what a plan with cs_plan_set_max_n and nothing else runs); 2: any set of TooLong, TooManyN
// and TooManyExpectedErrors, chosen at run time from the plan; 3: the same, plus the two read-end modifiers of
// include/cutseq_hip.h -- the quality trimmer's front walk (CS_OP_QTRIM with a q_cutoff_front) and CS_OP_NTRIM -- for the
// plans that hold one (cutadapt -q FRONT,BACK and --trim-n): their code exists in these instantiations alone; 4: FILT 3's
// code plus CS_OP_NEXTSEQ (cutadapt --nextseq-trim), for the plans that hold that op.  It has a value of its own because
// inside FILT 3 its walk cost the -q 20,20 --trim-n plan 1.1 % of its throughput, three times the spread of the parent's
// own runs (profiles/nextseq_ab.log); 5: FILT 4's code plus CS_OP_SHORTEN (cutadapt -l / -L), for the plans that hold that
// op.  A value of its own although the op is four integer instructions: inside FILT 3 it changed the spill counts of 10
// of the 16 FILT 3 / FILT 4 kernels (the coded wide scan kernel: 9 -> 11 spilled VGPRs; profiles/length_ab.log), and
// the same kind of change cost the -q 20,20 --trim-n plan 1.1 % when CS_OP_NEXTSEQ was tried there.  Here every kernel a
// plan without the op runs is the parent's, figure for figure.
//
// FILT_POLYA is no rung but a bit on top of one: the instantiations that hold CS_OP_POLYA (cutadapt --poly-a).  On the
// ladder the op would sit above FILT_SHORTEN, and a plain --poly-a plan -- the common one: the RNA presets with nothing
// else switched on -- would run the read-end ops' and the filters' code, 17-20 % of the trimming kernels' throughput
// (README), for an op that needs none of it.  So the bit exists on two rungs only: FILT_NONE | FILT_POLYA for plans
// whose only addition is the op, FILT_SHORTEN | FILT_POLYA for plans that have it next to any filter or read-end op.
// Sixteen instantiations; the kernels of a plan without the op are the ones it ran before, figure for figure
// (profiles/poly_a_ab.log).  Inside the kernel FILT means the rung.
enum { FILT_NONE = 0, FILT_MAXN = 1, FILT_ALL = 2, FILT_ENDS = 3, FILT_NEXTSEQ = 4, FILT_SHORTEN = 5, FILT_POLYA = 8 };
template <bool CODED, bool WIDE, int MODE, int FILT_ARG>
__global__ void __launch_bounds__(64, MODE == MODE_RESOLVE ? 4 : CS_SCAN_WAVES) trim_kernel(KArgs a) {
  if (a.gate && *a.gate != ~0ull) return;  // (wave-uniform: one wave per block)
  const DevPlan *plan = &c_plans[a.plan_slot];
  extern __shared__ uint32_t smem[];
  constexpr int TILE = kWave;  // blocks are one wave (the host launches 64 threads, __launch_bounds__ says so)
  constexpr bool SCAN = MODE != MODE_RESOLVE;
  constexpr int FILT = FILT_ARG & (FILT_POLYA - 1);      // the rung of the ladder
  constexpr bool POLYA = (FILT_ARG & FILT_POLYA) != 0;   // ... and whether CS_OP_POLYA's code is here
  uint32_t polya_bp = 0;  // bases this lane's CS_OP_POLYA ops removed, all tiles (POLYA only; dead code elsewhere)
  const int tid = threadIdx.x;
  const int mate = blockIdx.y;
  const MateArgs &ma = a.mate[mate];
  const int n_ops = plan->n_ops[mate];
  // (byte fields come through vector loads: readfirstlane moves them to the scalar unit once, or everything derived
  // from them -- the staging constants, for one -- lives in VGPRs across the tile loop, is spilled, and its reload
  // orders the next tile's first loads behind the last tile's result stores)
  const uint32_t pw0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const uint32_t *>(&plan->params)[1]);
  const uint32_t pw1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const uint32_t *>(&plan->params)[2]);
  static_assert(offsetof(cs_params, min_length) == 4 && offsetof(cs_params, select_rule) == 6 && offsetof(cs_params, use_filter) == 7 &&
                offsetof(cs_params, case_rule) == 8 && offsetof(cs_params, indel_tie) == 9, "cs_params layout");
  const int min_length = (int)(pw0 & 0xffffu);
  const int rule = (int)((pw0 >> 16) & 0xffu);
  const bool use_filter = ((pw0 >> 24) & 0xffu) != 0;
  const bool fold_case = (pw1 & 0xffu) == CS_CASE_FOLD;
  const bool tie_ins = ((pw1 >> 8) & 0xffu) == CS_TIE_INSERTION;
#ifdef CS_PHASE_TIMERS
  const int lane = tid;
#endif

  // LDS carve-up (dwords): private mask table + slack | tile | DP scratch | queue | match-mask tables | stats
  // (the scan kernel has neither DP scratch nor queue: col_dwords == 0, no items)
  if (lds_addr_of(smem) != 0u) __builtin_trap();  // myers_filter addresses the private table absolutely
  __builtin_amdgcn_s_setprio(SCAN ? PRIO_REST : PRIO_RESOLVE);  // (see myers_filter)
  uint32_t *cur_tab = smem;  // 64 bytes: the running op's match masks for the 32-bit filter (blocks are one wave)
  uint32_t *tile = smem + 20;  // + 16 bytes of slack: look-behind reads of the first row stay inside the allocation
  uint32_t *col = tile + (size_t)TILE * a.lds_stride_dw;
  uint32_t *wq = col + a.col_dwords;
  uint32_t *tables = wq + (SCAN ? 0 : kWave * kWaveItemDwords);
  uint32_t *fnibs = tables + a.n_table_ops * (kEqTableBytes / 4);  // adapter bases in read orientation, 4 bits each
  uint32_t *sacc = fnibs + a.n_table_ops * kFnibDwords;            // kStatWords block partial sums
  (void)col;
  (void)wq;

  // match-mask tables and read-orientation adapter nibbles (once per block): plain copies of what the host
  // laid out in the plan (DevOp::eq_tab, DevOp::fnib)
  for (int i = tid; i < (int)a.n_table_ops * (kEqTableBytes / 4); i += TILE) {
    const int t = i >> 4;
    tables[i] = t < n_ops ? plan->ops[mate][t].eq_tab[i & 15] : 0u;
  }
  for (int i = tid; i < (int)a.n_table_ops * kFnibDwords; i += TILE) {
    const int t = i / kFnibDwords, w = i - t * kFnibDwords;
    fnibs[i] = (CODED && t < n_ops) ? plan->ops[mate][t].fnib[w] : 0u;
  }
  for (int i = tid; i < kStatWords; i += TILE) sacc[i] = 0;
  // the leading pair of adapter ops (myers_pair): the 5' adapter's forward masks wait in the four slack dwords in
  // front of the tile (whatever they hold is fine for the look-behind reads they are there for)
  if (SCAN && CODED && tid < 4) smem[16 + tid] = (n_ops > 0 && plan->ops[mate][0].pair_next) ? plan->ops[mate][0].eq_fwd[tid] : 0u;

  // ---- work hand-out
  // Scan kernel.  Tiles are handed out in units of consecutive tiles: big units for the first part
  // of the batch (few atomics while every block is busy anyway -- plans without a scan finish a tile
  // in ~1 us and would otherwise hit the counter's ~88 ops/us limit), small units for the rest, so
  // that the blocks drain within a tile-time or two of each other (the host picks the sizes from
  // the plan's weight and the tiles per block, cutseq_hip.hip launch()).  The blocks that are resident
  // from the start (index < static_units) own unit blockIdx.x as their first one -- no atomic storm
  // at kernel start; everything else comes from the counter, so blocks that only become resident
  // late (the grid is twice the resident set) find small units or none.  The index of the next
  // tile is fetched one tile ahead.
  // Resolve kernel.  Batches of 64 records, one atomic each, the next one fetched a batch ahead.
  const uint32_t n_records = SCAN ? 0u : a.defer_count[mate * kTileCounterStride];
  // Resolve kernel: when there are fewer 64-record batches than waves, half of the waves would idle while the
  // others walk four strip passes in a row; batches of 32 or 16 records (two or one pass) spread the same
  // work over all of them.  (With more batches than waves the size does not matter: a wave's serial latency
  // per record is what bounds the kernel.)
  uint32_t batch_rows = TILE;
  if (!SCAN) {
    if (n_records < a.batch_knob * 64u * (uint32_t)gridDim.x) batch_rows = 32;
    if (n_records < a.batch_knob * 32u * (uint32_t)gridDim.x) batch_rows = 16;
  }
  // Resolve kernel: the queue holds two kinds of records, apart: from the bottom up the reads whose filter left a DP
  // window, from the top down the reads the existence-only scan could not clear (they need the whole exact filter of
  // their op: a wave full of them pays for it once, a wave with one of them among window records would pay it too)
  const uint32_t n_refl = SCAN ? 0u : a.defer_count[(4u + (uint32_t)mate) * kTileCounterStride];
  const uint32_t tiles_a = (n_records + batch_rows - 1) / batch_rows;
  const uint32_t n_tiles = SCAN ? (a.n_reads + (uint32_t)TILE - 1) / (uint32_t)TILE : tiles_a + (n_refl + (uint32_t)TILE - 1) / (uint32_t)TILE;
  const uint32_t big_tiles = a.big_tiles, big_units = big_tiles >> a.big_shift;
  const uint32_t big_mask = (1u << a.big_shift) - 1u, small_mask = (1u << a.small_shift) - 1u;
  auto unit_start = [&](uint32_t u) -> uint32_t {
    return (u < big_units) ? (u << a.big_shift) : big_tiles + ((u - big_units) << a.small_shift);
  };
  auto unit_end = [&](uint32_t tile) -> uint32_t {  // end of the unit that holds `tile`
    return (tile < big_tiles) ? ((tile | big_mask) + 1u) : big_tiles + (((tile - big_tiles) | small_mask) + 1u);
  };
  uint32_t *next_slot = sacc + kStatWords;  // one LDS dword to broadcast the fetched index
  // counter c hands out units static_units + c, + c + kTileCounters, ...: the counters advance together
  const uint32_t n_counters = min(kTileCounters, (uint32_t)gridDim.x);  // every counter needs a block that drains it
  const uint32_t my_counter = blockIdx.x % n_counters;
  uint32_t *counter = a.tile_counter + ((uint32_t)mate * kTileCounters + my_counter) * kTileCounterStride;
  uint32_t *claim = a.defer_count + (2u + (uint32_t)mate) * kTileCounterStride;
  auto next_unit = [&]() -> uint32_t { return a.static_units + my_counter + n_counters * atomicAdd(counter, 1u); };
  if (SCAN) {
    if (tid == 0) *next_slot = unit_start(blockIdx.x < a.static_units ? blockIdx.x : next_unit());
  } else {
    if (tid == 0) *next_slot = atomicAdd(claim, 1u);
  }
  __syncthreads();
  uint32_t tile_id = *next_slot, next_id = 0;
#ifdef CS_PHASE_TIMERS
  PhaseTimer pt;
  pt.last = clock64();
  for (int i = 0; i < 8; ++i) pt.acc[i] = 0;
  pt.passes = pt.steps = pt.items = 0;
#endif

  // scan kernel: the records of the previous tile's deferred reads, parked in LDS, and their queue reservation
  uint4 *ring = reinterpret_cast<uint4 *>((reinterpret_cast<uintptr_t>(sacc + kStatWords + 4) + 15u) & ~(uintptr_t)15u);
  uint32_t pend_count = 0;  // wave-uniform: records parked
  bool pend_asked = false;  // wave-uniform: their queue reservation left behind this tile's staging
  uint32_t pend_q = 0;      // lane 0: the queue position the counter answered
  auto flush_ring = [&]() {  // parked records -> queue
    const uint32_t qb = (uint32_t)__builtin_amdgcn_readfirstlane((int)pend_q);
    const uint32_t lane = wave_lane_fresh();
    if (lane < pend_count) {
      uint4 *rec = a.defer[mate] + (size_t)(qb + lane) * 2u;
      rec[0] = ring[lane * 2];
      rec[1] = ring[lane * 2 + 1];
    }
    pend_count = 0;
    pend_asked = false;
  };
  bool fast_ok = SCAN && CODED && a.fast_recode != 0u, fast_failed = false;  // wave-uniform: see the staging below
  for (; tile_id < n_tiles; tile_id = next_id) {
  // The lane index is "new" in every tile (an empty asm the optimiser cannot see through): addresses and offsets
  // derived from it are recomputed per tile -- a handful of adds and shifts -- instead of living in registers across
  // the tile loop.  Hoisted, four of them were spilled, and their reloads -- scratch loads, answered in order behind the
  // previous tile's result stores -- made the next tile's first instructions wait for those stores.
  // (scan kernel: not even threadIdx.x itself stays in a register across the loop, see wave_lane_fresh)
  uint32_t lane_fresh = SCAN ? wave_lane_fresh() : threadIdx.x;
  asm volatile("" : "+v"(lane_fresh));
  const int tid = (int)lane_fresh, lane = tid;
  const bool top = !SCAN && tile_id >= tiles_a;  // a batch of the queue's top region
  const uint32_t row0 = top ? (tile_id - tiles_a) * (uint32_t)TILE : tile_id * batch_rows;
  const uint32_t rows_here = top ? min((uint32_t)TILE, n_refl - row0) : min(batch_rows, (SCAN ? a.n_reads : n_records) - row0);
  const bool valid = (uint32_t)tid < rows_here;

  // ---- per-lane chain state: fresh (scan) or from the queue record (resolve)
  uint32_t gr = row0 + tid;
  int s = 0, e = 0, t0 = 0;
  // small fields share registers (the chain state is what gets spilled around the adapter ops):
  //   fm   = result flags (bits 0..7) | ops that matched (bit 8 + t)
  //   meta = matches so far | exact-DP requests << 8 | barcode index << 16 | deferring op << 24
  //   capo = offset of capture 1 | offset of capture 2 << 16 (UMIs; the layout of record dword rb.z)
  //   qc   = quality-trimmed bases | length of capture 1 << 16 | length of capture 2 << 24
  uint32_t fm = 0, capo = 0, qc = 0;
  uint32_t meta = (uint32_t)CS_DEMUX_NONE << 16;
  uint32_t rec_win = 0, rec_rows = 0, rec_rmax = 0;  // the deferring op's DP window
  if (!SCAN) {
    uint4 ra = make_uint4(0, 0, 0, 0), rb = make_uint4(0, 0, 0, 0);
    if (valid) {
      const uint4 *rec = a.defer[mate] + (size_t)(top ? a.defer_cap - 1u - gr : gr) * 2u;
      ra = rec[0];
      rb = rec[1];
    }
    gr = ra.x;
    s = (int)(ra.y & 0xffffu);
    e = (int)(ra.y >> 16);
    rec_win = ra.z;
    rec_rows = ra.w;
    t0 = (int)(rb.x >> 24);
    fm = (rb.y & 0xffu) | ((rb.x & 0xffffffu) << 8);
    meta = ((rb.y >> 8) & 0xffu) | ((rb.w >> 24) << 16);  // matches so far, barcode index
    rec_rmax = (rb.y >> 16) & 0xffu;
    capo = rb.z;
    qc = ((rb.w >> 8) & 0xffffu) | ((rb.y >> 24) << 16) | (rb.w << 24);
  }

  // len[i] <= stride is the caller's contract (cutseq_hip.h); a longer value is clamped, never followed
  // (asked for in front of the staging loads: nothing waits for it)
  const uint32_t len_raw = valid ? (uint32_t)ma.len[gr] : 0u;
  // CS_LEN_SKIP: a read that is handled elsewhere (text path: longer than the rows, long_kernel.hip.inc walks its chain)
  const bool here = SCAN ? (valid && len_raw != (uint32_t)CS_LEN_SKIP) : valid;
  const int len = here ? min((int)len_raw, (int)(a.stride_dw * 4u)) : 0;

  // ---- stage the tile: bases re-coded (coded plans: 4 bits per base, 8 per LDS dword), rows re-strided
  // to an odd dword count.
  {
    const uint32_t S = a.stride_dw;
    const uint32_t tile_b = lds_addr_of(tile);
    if (SCAN) {
      // coalesced 16-byte loads over the tile's contiguous byte range.  A source dword D (4 bases) of row r
      // lands in 16-bit slot D + r * pad of the coded tile (pad = LDS row length in 16-bit units minus
      // source row length in dwords), so the destination follows from the linear index and one running
      // row number -- no division, no multiply.
      const uint32_t total = rows_here * S;
      const uint32_t *src = ma.seq + (size_t)row0 * S;
      if (CODED) {
        const uint32_t pad2 = (a.lds_stride_dw * 2u - S) * 2u;  // pad in bytes
        // (FAST: the re-coding that trusts the bytes and checks them, see encode4_pairs_fast; -> the lanes' differences)
        // (LINEAR: the coded tile is linear in the source -- no pad, 16-byte aligned rows of at least a quad -- see below)
        const bool linear = pad2 == 0 && (((uintptr_t)src) & 15u) == 0 && S >= 4;  // wave-uniform
        auto stage_coded = [&](auto fast_tag, auto linear_tag) -> uint32_t {
        constexpr bool FAST = decltype(fast_tag)::value, LINEAR = decltype(linear_tag)::value;
        uint32_t bad = 0, done = 0;
        EncodeConsts ec;
        FastEncodeConsts fc;
        if constexpr (FAST) fc = fast_encode_consts(); else ec = encode_consts(fold_case);
        auto enc8 = [&](uint32_t w0, uint32_t w1) -> uint32_t {
          if constexpr (FAST) return encode8_nib_fast(w0, w1, bad, fc); else return encode8_nib_v(w0, w1, ec);
        };
        auto enc4 = [&](uint32_t w) -> uint32_t {
          if constexpr (FAST) return encode4_nib_fast(w, bad, fc); else return encode4_nib_v(w, ec);
        };
        constexpr int kBatch = 4;  // loads in flight per lane before the first one is consumed (three rounds per 150-base tile; five in flight are no faster any more and spill five registers more)
        constexpr uint32_t kRound = (uint32_t)TILE * kBatch;
        if constexpr (LINEAR) {
          // quad q of the tile lands at byte 8 q of the coded tile whatever row it lies in: one 8-byte store per quad
          // at a constant offset from the lane's slot of the round, no row / column to keep.  The loads roll as below.
          const uint32_t quads = total >> 2, last_q = quads - 1u;
          const uint4 *src4 = reinterpret_cast<const uint4 *>(src);
          uint32_t dst = tile_b + ((uint32_t)tid << 3);
          uint4 w[kBatch];
#pragma unroll
          for (int u = 0; u < kBatch; ++u) w[u] = src4[min((uint32_t)tid + (uint32_t)u * TILE, last_q)];
          auto put = [&](const uint4 &v, uint32_t off) {
            *(lds_u64 *)(uintptr_t)(dst + off) = (unsigned long long)enc8(v.x, v.y) | ((unsigned long long)enc8(v.z, v.w) << 32);
          };
          uint32_t qb = 0;  // (wave-uniform)
          for (; qb + kRound < quads; qb += kRound) {
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
              put(w[u], (uint32_t)u * TILE * 8u);
              w[u] = src4[min(qb + kRound + (uint32_t)u * TILE + (uint32_t)tid, last_q)];
            }
            dst += kRound * 8u;
          }
#pragma unroll
          for (int u = 0; u < kBatch; ++u)
            if (qb + (uint32_t)u * TILE + (uint32_t)tid < quads) put(w[u], (uint32_t)u * TILE * 8u);
          done = quads << 2;
        } else if ((((uintptr_t)src) & 15u) == 0 && S >= 4) {  // a quad then touches at most two rows
          const uint32_t quads = total >> 2;
          const uint4 *src4 = reinterpret_cast<const uint4 *>(src);
          // row / column of this lane's first dword by one division, then advanced by the constant
          // lane stride (TILE quads) with a wrap test
          // (no integer division per tile: (x + 0.5) / S in float is further from an integer than its rounding error
          // for x < 256, S <= CS_MAX_STRIDE / 4)
          uint32_t r = (uint32_t)(((float)((uint32_t)tid << 2) + 0.5f) * (1.0f / (float)S)), c = ((uint32_t)tid << 2) - r * S;
          const uint32_t step_r = ((uint32_t)TILE << 2) / S, step_c = ((uint32_t)TILE << 2) - step_r * S;
          uint32_t dst = tile_b + ((uint32_t)tid << 3) + r * pad2;  // byte address of the quad's first slot
          const uint32_t step_dst = ((uint32_t)TILE << 3) + step_r * pad2;
          // The loads ROLL: a slot's next load leaves as soon as the slot has been consumed, so the tile pays one memory
          // round trip and not one per round of kBatch loads.  Every round but the last is whole (all its quads exist):
          // loads and stores in straight-line code, the wait in front of a slot leaves the three younger loads in flight.
          // A load beyond the tile's last quad (the last round is partial as a rule) re-reads that quad and is dropped.
          const uint32_t last_q = quads - 1u;  // (quads >= 1: a tile has at least one row of at least four dwords)
          (void)enc8;
          uint4 w[kBatch];
#pragma unroll
          for (int u = 0; u < kBatch; ++u) w[u] = src4[min((uint32_t)tid + (uint32_t)u * TILE, last_q)];
          auto put = [&](const uint4 &v) {  // (pad2 != 0 here: the linear tile has its own form above)
            const uint32_t n0 = enc4(v.x), n1 = enc4(v.y);
            const uint32_t n2 = enc4(v.z), n3 = enc4(v.w);
            // the quad may run over the end of its row: later slots move by one pad
            lds_write_u16(dst, 0, n0);
            lds_write_u16(dst + ((c + 1 >= S) ? pad2 : 0u), 2, n1);
            lds_write_u16(dst + ((c + 2 >= S) ? pad2 : 0u), 4, n2);
            lds_write_u16(dst + ((c + 3 >= S) ? pad2 : 0u), 6, n3);
          };
          auto step = [&]() {
            c += step_c;
            dst += step_dst;
            if (c >= S) {
              c -= S;
              dst += pad2;
            }
          };
          uint32_t qb = 0;  // (wave-uniform)
          for (; qb + kRound < quads; qb += kRound) {  // whole rounds with another round behind them
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
              put(w[u]);
              step();
              w[u] = src4[min(qb + kRound + (uint32_t)u * TILE + (uint32_t)tid, last_q)];
            }
          }
#pragma unroll
          for (int u = 0; u < kBatch; ++u) {  // the last round
            if (qb + (uint32_t)u * TILE + (uint32_t)tid < quads) put(w[u]);
            step();
          }
          done = quads << 2;
        }
        for (uint32_t dw = done + tid; dw < total; dw += TILE) {
          const uint32_t r = dw / S;
          lds_write_u16(tile_b + dw * 2u + r * pad2, 0, enc4(src[dw]));
        }
        return bad;
        };  // stage_coded
        auto stage = [&](auto fast_tag) -> uint32_t {
          return linear ? stage_coded(fast_tag, std::true_type{}) : stage_coded(fast_tag, std::false_type{});
        };
        // a wave keeps the fast form until a tile holds a byte it cannot vouch for (wave-uniform, sticky)
        bool redo = !fast_ok;
        if (fast_ok) {
          const uint32_t bad = stage(std::true_type{});
          if (a.fast_recode != 2u && __ballot(bad != 0u)) {  // (2: tests only -- never fall back)
            redo = true;
            fast_ok = !fast_failed;  // one odd byte now and then costs its tile a second staging; two tiles in a row
          }                          // (zero padding, soft-masked reads): the wave stays with the exact form
          fast_failed = redo;
        }
        if (redo) (void)stage(std::false_type{});
      } else {
        for (uint32_t dw = tid; dw < total; dw += TILE) {
          const uint32_t r = dw / S;
          tile[r * a.lds_stride_dw + (dw - r * S)] = fold_case ? upper4(src[dw]) : src[dw];
        }
      }
    } else {
      // gather: the rows of the batch's records, dword by dword in linear order over the batch (lane i takes
      // dword i, i + 64, ...: a row's dwords are read by consecutive lanes), eight loads in flight per lane
      wq[tid] = gr;
      wave_lds_fence();
      const uint32_t total = rows_here * S;
      EncodeConsts ec = encode_consts(fold_case);
      uint32_t r = (uint32_t)tid / S, c = (uint32_t)tid - r * S;
      const uint32_t step_r = (uint32_t)TILE / S, step_c = (uint32_t)TILE - step_r * S;
      constexpr int kBatch = 8;
      for (uint32_t i0 = tid; i0 < total; i0 += (uint32_t)TILE * kBatch) {
        uint32_t w[kBatch], dst[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const uint32_t i = i0 + (uint32_t)u * TILE;
          if (i < total) {
            w[u] = ma.seq[(size_t)wq[r] * S + c];
            dst[u] = CODED ? (tile_b + r * a.lds_stride_dw * 4u + c * 2u) : (r * a.lds_stride_dw + c);
          }
          r += step_r;
          c += step_c;
          if (c >= S) {
            c -= S;
            r += 1;
          }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const uint32_t i = i0 + (uint32_t)u * TILE;
          if (i < total) {
            if (CODED)
              lds_write_u16(dst[u], 0, encode4_nib_v(w[u], ec));
            else
              tile[dst[u]] = fold_case ? upper4(w[u]) : w[u];
          }
        }
      }
      wave_lds_fence();  // wq is the survivor queue again from here on
    }
  }
  __syncthreads();
  CS_T_MARK(pt, 0);
  // The index of the next tile.  When this unit / batch is used up the counter is asked HERE, behind the staging
  // loads (memory operations return in order: an atomic in front of them would hold their data back), and the
  // answer is looked at when the tile is done.
  const bool same_unit = SCAN && tile_id + 1 < unit_end(tile_id);
  uint32_t fetched = 0;
  if (tid == 0 && !same_unit) fetched = SCAN ? atomic_add_later(counter, 1u) : atomic_add_later(claim, 1u);
  // (the counter is one address for the whole device: records of several tiles share a reservation)
  if (SCAN && pend_count >= (uint32_t)kRingRecords / 2) {
    if (tid == 0) pend_q = atomic_add_later(&a.defer_count[mate * kTileCounterStride], pend_count);
    pend_asked = true;
  }
  const uint32_t *wave_rows = tile;
  const uint32_t *myrow = wave_rows + (size_t)lane * a.lds_stride_dw;
  bool deferred = false;  // scan kernel: this lane's read went to the queue
  bool refl = false;      // ... to its top region (existence-only scan: the resolve kernel filters the op exactly)
  bool refl_any = false;  // wave-uniform: some lane of this tile did
  uint32_t refl_q = 0, refl_rank = 0;

  if (SCAN) e = len;
  // ---- scan kernel: the pair of adapter ops that opens the chain, in one forward walk (myers_pair).  It runs IN
  // FRONT of the op loop, before the chain state exists: none of it occupies a register while the columns are walked.
  int t_first = 0;
  if constexpr (SCAN && CODED) {
    const bool pair = use_filter && n_ops >= 2 && plan->ops[mate][0].pair_next;  // wave-uniform (plan constants)
    const bool solo = use_filter && n_ops >= 1 && plan->ops[mate][0].solo_first;
    if (pair || solo) {
      const int tb = pair ? 1 : 0;  // the op whose exact filter the walk is
      const DevOp &da = plan->ops[mate][0], &db = plan->ops[mate][tb];
      if (lane < 8) {  // private table, low dword: the 3' op's masks, high dword: the 5' adapter in read orientation
        cur_tab[lane * 2] = tables[tb * (kEqTableBytes / 4) + lane * 2 + 1];
        cur_tab[lane * 2 + 1] = (pair && lane < 4) ? smem[16 + lane] : 0u;
      }
      wave_lds_fence();
      bool none = true;
      Verdict vb = verdict_none(db.f.m);
      if (here && len > 0) {
        // the wave's item log (myers_pair, ItemLog): a.item_slots 8-byte items per lane behind the ring, then their tags
        ItemLog il;
        il.bytes = a.item_slots * 8u;
        il.slot0 = lds_addr_of(ring + kRingRecords * 2) + (uint32_t)lane * il.bytes;
        il.tag_off = (lds_addr_of(ring + kRingRecords * 2) + (uint32_t)TILE * il.bytes) - (lds_addr_of(ring + kRingRecords * 2) >> 3);
        if (pair)
          vb = myers_pair<true>(da, db, rule, fnibs + kFnibDwords, myrow, len, none, il CS_T_ARG);
        else
          vb = myers_pair<false>(da, db, rule, fnibs, myrow, len, none, il CS_T_ARG);
      }
      CS_T_MARK(pt, 2);
      // op 0 of a pair: a read the walk could not clear goes to the TOP region of the queue, the resolve kernel filters
      // it exactly
      refl = !none;  // (a lone forward op: only a full item log gets here)
      const unsigned long long rm = __ballot(refl);
      if (rm) {
        if (lane == 0) refl_q = atomic_add_later(&a.defer_count[(4u + (uint32_t)mate) * kTileCounterStride], (uint32_t)__popcll(rm));
        refl_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rm, 0u));
        refl_any = true;
      }
      if (refl) {
        deferred = true;
        rec_win = 0;
        rec_rows = 0xffffffffu;
        rec_rmax = 0xffu;  // "no window yet": the resolve kernel runs the exact filter on op 0 itself
      } else if (here) {
        if (pair && da.f.required) fm |= CS_F_UNTRIMMED;  // (op 0 did not match)
        // the forward op: its verdict, as the op loop would apply it
#ifdef CS_EXP_REASON
        for (int q = 0; q < 24; ++q) {  // diagnostic: deferred reads by reason -> statistics slots (two counters per word)
          const unsigned long long bm = __ballot(vb.need && vb.reason == q);
          if (bm && lane == 0) atomicAdd(&a.stats[(size_t)mate * kStatWords + ST_OPS + 8 + (q % 12)], (unsigned long long)__popcll(bm) << (q >= 12 ? 32 : 0));
        }
#endif
        if (vb.need) {
          meta += 0x100u;
          deferred = true;
          meta = (meta & 0x00ffffffu) | ((uint32_t)tb << 24);
          rec_win = (uint32_t)vb.j0 | ((uint32_t)vb.j1 << 16) | ((uint32_t)vb.do_end << 31);
          rec_rows = vb.rows;
          rec_rmax = (uint32_t)vb.rmax;
        } else if (vb.found) {  // (not reversed: query coordinates are read coordinates; s == 0)
          meta += 1u;
          fm |= (uint32_t)db.f.match_flag | (0x100u << tb);
          if (db.f.remove == CS_REMOVE_BEFORE)
            s = vb.qe;
          else
            e = vb.qs;
        } else if (db.f.required) {
          fm |= CS_F_UNTRIMMED;
        }
      }
      t_first = tb + 1;
    }
  }

  for (int t = t_first; t < n_ops; ++t) {
    const DevOp &d = plan->ops[mate][t];
    const DevFields &op = d.f;
    const bool on = here && !deferred && t >= t0;  // this lane's read is at this op
    if (!SCAN && !__ballot(on)) continue;           // every record of the batch was deferred further down
    const int n = e - s;
    const int kind = op.kind;
    if (kind == CS_OP_ADAPTER) {
      const int m = op.m;
      const char *tab = reinterpret_cast<const char *>(tables + t * (kEqTableBytes / 4));
      if (SCAN && (d.filter_mode == FILTER_POLY_TAIL || d.filter_mode == FILTER_POLY_HEAD)) CS_T_MARK(pt, 7);
      Verdict v = verdict_none(m);
      bool poly_lane = false;  // homopolymer op on a coded tile: this lane's read may match (see poly_maybe)
      const uint32_t mode = use_filter ? d.filter_mode : (uint32_t)FILTER_NONE;
      if (CODED && mode == FILTER_MYERS32) {  // uniform: this op's left-aligned masks -> private table
        if (lane < 8) cur_tab[lane * 2] = tables[t * (kEqTableBytes / 4) + lane * 2 + 1];
        wave_lds_fence();
      }
      const bool refilter = !SCAN && on && t == t0 && rec_rmax == 0xffu;  // deferred by the existence-only scan
      if (!SCAN && on && t == t0 && !refilter) {
        // the op that sent this read to the queue: its filter already ran, the record holds the window
        v.need = 1;
        v.j0 = (int)(rec_win & 0xffffu);
        v.j1 = (int)((rec_win >> 16) & 0x7fffu);
        v.do_end = (int)(rec_win >> 31);
        v.rmax = (int)rec_rmax;
        v.rows = rec_rows;
      } else if (on && n > 0) {
        const int aflags = op.align_flags;
        const bool free_ends = (aflags & (CS_QUERY_START | CS_QUERY_STOP)) == (CS_QUERY_START | CS_QUERY_STOP);
        if (op.shortcut == CS_SHORTCUT_FIND && (!free_ends || mode == FILTER_NONE)) {
          // str.find looks at the whole read; settle it separately where the filter cannot
          const int p = naive_find<CODED>(d, myrow, s, e);
          if (p >= 0) {
            v.found = 1;
            v.qs = p;
            v.qe = p + m;
          }
        }
        if (v.found) {
          // decided by the exact short cut
        } else if (SCAN && CODED && mode == FILTER_MYERS32 && d.exists_only) {
          // matches of this op are rare: prove that there is none, or let the resolve kernel look closely
          const bool none = op.reversed ? myers_none<-1>(d, myrow, s, e CS_T_ARG) : myers_none<+1>(d, myrow, s, e CS_T_ARG);
          if (!none) {
            v.need = 1;
            v.rmax = 0xff;  // "no window yet": the resolve kernel runs the exact filter on this op itself
            refl = true;
          }
        } else if (mode == FILTER_MYERS32) {
          if (op.reversed)
            v = myers_filter<uint32_t, -1, CODED, SCAN>(d, rule, tab, fnibs + t * kFnibDwords, myrow, s, e CS_T_ARG);
          else
            v = myers_filter<uint32_t, +1, CODED, SCAN>(d, rule, tab, fnibs + t * kFnibDwords, myrow, s, e CS_T_ARG);
        } else if (WIDE && mode == FILTER_MYERS64) {
          if (op.reversed)
            v = myers_filter<uint64_t, -1, CODED, SCAN>(d, rule, tab, fnibs + t * kFnibDwords, myrow, s, e CS_T_ARG);
          else
            v = myers_filter<uint64_t, +1, CODED, SCAN>(d, rule, tab, fnibs + t * kFnibDwords, myrow, s, e CS_T_ARG);
        } else if (mode == FILTER_POLY_TAIL) {
          if (CODED)
            poly_lane = poly_maybe<false>(d, myrow, s, e);
          else
            v = poly_tail<CODED>(d, rule, myrow, s, e);
        } else if (mode == FILTER_POLY_HEAD) {
          if (CODED)
            poly_lane = poly_maybe<true>(d, myrow, s, e);
          else
            v = poly_head<CODED>(d, rule, myrow, s, e);
        } else {
          int min_n, max_n;
          column_range(aflags, m, op.k, n, min_n, max_n);
          v.need = 1;
          v.j0 = min_n;
          v.j1 = max_n;
          v.do_end = (max_n == n) ? 1 : 0;
        }
      }
      if (SCAN && (mode == FILTER_POLY_TAIL || mode == FILTER_POLY_HEAD)) CS_T_MARK(pt, 3);
      if (CODED && (mode == FILTER_POLY_TAIL || mode == FILTER_POLY_HEAD)) {
        // the wave serves its maybe-lanes one by one (wave-uniform from here: bitmap by ballot, closed form on
        // the scalar unit)
        unsigned long long todo = __ballot(poly_lane);
#ifdef CS_PHASE_TIMERS
        if (SCAN) {  // diagnostic: maybe-lanes served (items) and tiles that had any (passes)
          pt.items += (uint32_t)__popcll(todo);
          pt.passes += todo ? 1u : 0u;
        }
#endif
        const bool head = mode == FILTER_POLY_HEAD;
        while (todo) {
          const int src = __builtin_ctzll(todo);
          todo &= todo - 1ull;
          const int ls = __builtin_amdgcn_readlane(s, src), le = __builtin_amdgcn_readlane(e, src);
          const int ln = le - ls;
          const uint32_t *lrow = wave_rows + (size_t)src * a.lds_stride_dw;
          const PolyMaps pm = poly_maps(d, lrow, head, ls, le, lane);
          const Verdict uv = head ? poly_head_wave(d, pm, ln) : poly_tail_wave(d, rule, pm, ln);
          if (lane == src) v = uv;
        }
      }
      if (v.need && !(!SCAN && on && t == t0 && !refilter) && !(SCAN && v.rmax == 0xff)) meta += 0x100u;
      CS_T_MARK(pt, (mode == FILTER_POLY_TAIL || mode == FILTER_POLY_HEAD) ? 4 : 2);
      if constexpr (SCAN) {
        // reads the existence-only scan could not clear go to the TOP region of the queue; the reservation leaves
        // now, its answer is looked at when the tile is done
        if (CODED && d.exists_only) {
          const unsigned long long rm = __ballot(refl && !deferred);
          if (rm) {
            if (lane == 0) refl_q = atomic_add_later(&a.defer_count[(4u + (uint32_t)mate) * kTileCounterStride], (uint32_t)__popcll(rm));
            refl_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rm, 0u));
            refl_any = true;
          }
        }
        // ---- the exact DP is the resolve kernel's business: freeze this lane's chain state
        if (v.need) {
          deferred = true;
          meta = (meta & 0x00ffffffu) | ((uint32_t)t << 24);
          rec_win = (uint32_t)v.j0 | ((uint32_t)v.j1 << 16) | ((uint32_t)v.do_end << 31);
          rec_rows = v.rows;
          rec_rmax = (uint32_t)v.rmax;
        }
      } else {
        // ---- phase B inside the wave: survivors compacted to the low lanes
        const unsigned long long need_mask = __ballot(v.need != 0);
        if (need_mask) {
          const int qn = __popcll(need_mask);
          // queue order = window length class: a strip pass (16 survivors) costs what its longest window costs,
          // so the short windows (partial hits at the read end) go through passes of their own
          const int wclass = min((v.j1 - v.j0) >> 3, 3);
          int my_slot = 0, before = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const unsigned long long cm = __ballot(v.need != 0 && wclass == c);
            if (wclass == c)
              my_slot = before + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(cm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cm, 0u));
            before += __popcll(cm);
          }
          if (v.need) {
            uint32_t *it = wq + my_slot * kWaveItemDwords;
            it[0] = (uint32_t)lane | ((uint32_t)v.j0 << 16);
            it[1] = (uint32_t)v.j1 | ((uint32_t)v.do_end << 15) | ((uint32_t)v.rmax << 16);
            it[2] = (uint32_t)s | ((uint32_t)e << 16);
            it[3] = v.rows;
          }
          wave_lds_fence();
          const int eqm = (d.acgt_only && m <= 32) ? 1 : (d.acgt_only ? 2 : 0);
          if (eqm == 1 && (int)a.col_dwords >= 16 * (m + 1)) {
            // cooperative strips: 4 lanes per survivor (16 survivors per pass) normally; with at most 8
            // survivors and a short adapter 8 lanes of 3 rows each -- fewer cells per step for a few more steps
            auto strips = [&](auto tie_tag) {
              constexpr bool TI = decltype(tie_tag)::value;
              if (qn <= 8 && m <= 24) {
                strip_dp_pass<8, 3, CODED, TI>(d, tab, rule, wave_rows, a.lds_stride_dw, wq, col, m + 1, 0, qn, lane CS_T_ARG);
              } else {
                for (int base = 0; base < qn; base += 16) {
                  if (m <= 20)
                    strip_dp_pass<4, 5, CODED, TI>(d, tab, rule, wave_rows, a.lds_stride_dw, wq, col, m + 1, base, qn, lane CS_T_ARG);
                  else
                    strip_dp_pass<4, 8, CODED, TI>(d, tab, rule, wave_rows, a.lds_stride_dw, wq, col, m + 1, base, qn, lane CS_T_ARG);
                }
              }
            };
            if (tie_ins)  // wave-uniform (plan constant)
              strips(std::true_type{});
            else
              strips(std::false_type{});
          } else {
            // one lane per survivor, column in LDS (long or non-ACGT adapters)
            const int cap = min(kWave, (int)(a.col_dwords / (uint32_t)(m + 1)));
            for (int base = 0; base < qn; base += cap) {
              const int idx = base + lane;
              if (lane < cap && idx < qn) {
                uint32_t *it = wq + idx * kWaveItemDwords;
                const uint32_t i0 = it[0], i1 = it[1], i2 = it[2];
                const int r = (int)(i0 & 0xffffu), j0 = (int)(i0 >> 16);
                const int j1 = (int)(i1 & 0x7fffu), do_end = (int)((i1 >> 15) & 1u), rmax = (int)(i1 >> 16);
                const int rs = (int)(i2 & 0xffffu), re = (int)(i2 >> 16);
                const uint32_t *rrow = wave_rows + (size_t)r * a.lds_stride_dw;
                uint32_t res;
                if (eqm == 1)
                  res = exact_dp<1, CODED>(d, tab, rule, tie_ins, rrow, rs, re, j0, j1, do_end, rmax, col + lane, cap);
                else if (WIDE && eqm == 2)
                  res = exact_dp<2, CODED>(d, tab, rule, tie_ins, rrow, rs, re, j0, j1, do_end, rmax, col + lane, cap);
                else
                  res = exact_dp<0, CODED>(d, tab, rule, tie_ins, rrow, rs, re, j0, j1, do_end, rmax, col + lane, cap);
                it[3] = res;
              }
            }
          }
          wave_lds_fence();
          if (v.need) {
            const uint32_t r = wq[my_slot * kWaveItemDwords + 3];
            v.found = (int)(r >> 31);
            v.qs = (int)((r >> 16) & 0x7fffu);
            v.qe = (int)(r & 0xffffu);
          }
          wave_lds_fence();  // queue entries are reused by the next adapter op
        }
        CS_T_MARK(pt, 3);
      }
      if (on && !deferred) {
        if (v.found) {
          int rstart = v.qs, rstop = v.qe;
          if (op.reversed) {
            rstart = n - v.qe;
            rstop = n - v.qs;
          }
          meta += 1u;
          fm |= (uint32_t)op.match_flag | (0x100u << t);
          if (op.remove == CS_REMOVE_BEFORE)
            s += rstop;
          else
            e = s + rstart;
        } else if (op.required) {
          fm |= CS_F_UNTRIMMED;
        }
      }
    } else if (kind == CS_OP_CUT) {
      // (a run of cuts in one turn: the chain resumes in the resolve kernel at an adapter or demultiplexing op only,
      // never inside a run)
      const int run = max(1, min((int)d.cut_run, kCutRun));
#pragma unroll
      for (int q = 0; q < kCutRun; ++q) {
        if (q >= run) break;  // wave-uniform
        const uint32_t pk = d.cut_pack[q];
        const int cut_len = (int)(int16_t)(pk & 0xffffu);
        const bool conditional = (pk >> 16) & 1u;
        const uint32_t capture = (pk >> 17) & 3u;
        const int force_min_len = (int)(pk >> 19);
        const int nq = e - s;
        const bool skip = conditional && (meta & 0xffu) == 0u && nq < force_min_len;
        if (on && !skip && cut_len != 0) {
          int c, off;
          if (cut_len > 0) {
            c = min(cut_len, nq);
            off = s;
            s += c;
          } else {
            c = min(-cut_len, nq);
            off = e - c;
            e -= c;
          }
          if (capture == 1) {
            capo = (capo & 0xffff0000u) | (uint32_t)off;
            qc = (qc & 0xff00ffffu) | ((uint32_t)c << 16);
          } else if (capture == 2) {
            capo = (capo & 0x0000ffffu) | ((uint32_t)off << 16);
            qc = (qc & 0x00ffffffu) | ((uint32_t)c << 24);
          }
        }
      }
      t += run - 1;
    } else if (kind == CS_OP_DEMUX) {
      // Which of the plan's inline barcodes starts the interval?  Every PrefixAdapter outcome on the first
      // m + k bases is in the table (cutseq_hip.h, CS_OP_DEMUX): index the bases in base 5, one load.
      const int span = (int)op.m + (int)op.k;
      if (d.filter_mode) {  // (uniform) the barcodes' own ops, no table of every prefix (cs_plan_set_demux_ops)
        if constexpr (SCAN) {
          // the resolve kernel's business, for every read: it has the DP and its scratch columns
          if (on) {
            deferred = true;
            meta = (meta & 0x00ffffffu) | ((uint32_t)t << 24);
            rec_win = rec_rows = rec_rmax = 0;
          }
        } else {
          // A table over the first bases names the barcodes that can still match; each candidate's own PrefixAdapter
          // op then runs on the read (the exact DP, as a single-barcode plan without a filter would run it), and the
          // outcomes merge as in a table entry: an exact copy of a barcode first, else the lowest index; more than one
          // match is flagged.
          const uint32_t *first = reinterpret_cast<const uint32_t *>((uintptr_t)d.peq[0]);
          const uint8_t *pool = reinterpret_cast<const uint8_t *>((uintptr_t)d.peq[1]);
          const DevOp *bops = reinterpret_cast<const DevOp *>((uintptr_t)d.peq[2]);
          const int depth = (int)d.peq[3];
          const bool at_end = op.reversed != 0;  // the barcodes sit at the 3' end of the interval (SuffixAdapter ops)
          uint32_t cnt = 0, off = 0;
          if (on) {
            const int take = min(n, depth);
            uint32_t idx = 0, pw = 1, block = 0;
            for (int u = 0; u < depth; ++u) {  // uniform
              if (u < take) {
                const uint32_t c = row_code<CODED>(myrow, at_end ? e - 1 - u : s + u);
                uint32_t digit;
                if (CODED)
                  digit = (c & 0x20u) ? 4u : (c >> 3);
                else
                  digit = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? ((c >> 1) & 3u) : 4u;
                idx += digit * pw;
                block += pw;
              }
              pw *= 5u;
            }
            const uint32_t ent = first[block + idx];
            cnt = ent & 0xffu;
            off = ent >> 8;
          }
          uint32_t id = CS_DEMUX_NONE, hits = 0;
          int cut = 0;
          bool exact_taken = false;
          const int mb = (int)op.m;
          for (uint32_t ci = 0; __ballot(ci < cnt); ++ci) {
            if (ci < cnt) {
              const uint32_t b = pool[off + ci];
              const DevOp &bd = bops[b];
              int min_n, max_n;
              column_range((int)bd.f.align_flags, mb, (int)bd.f.k, n, min_n, max_n);
              const uint32_t r = exact_dp<0, CODED>(bd, nullptr, rule, tie_ins, myrow, s, e, min_n, max_n,
                                                    max_n == n ? 1 : 0, mb, col + lane, kWave);
              if (r >> 31) {
                const int qs = (int)((r >> 16) & 0x7fffu), qe = (int)(r & 0xffffu);
                // an exact copy of the barcode at the anchored end
                bool exact = n >= mb && (at_end ? qs == n - mb : qe == mb);
                for (int i = 0; exact && i < mb; ++i)
                  exact = row_code<CODED>(myrow, at_end ? e - mb + i : s + i) == (uint32_t)bd.op.seq[i];
                if (id == CS_DEMUX_NONE || (exact && !exact_taken)) {
                  id = b;
                  cut = at_end ? qs : qe;
                }
                exact_taken = exact_taken || exact;
                ++hits;
              }
            }
          }
          if (on) {
            if (id != CS_DEMUX_NONE) {
              if (at_end)
                e = s + cut;  // SuffixAdapter: RemoveAfterMatch
              else
                s += cut;     // PrefixAdapter: RemoveBeforeMatch
              meta += 1u;
              fm |= (uint32_t)op.match_flag | (0x100u << t);
              if (hits > 1u) fm |= CS_F_AMBIGUOUS;
              meta = (meta & 0xff00ffffu) | (id << 16);
            } else if (op.required) {
              fm |= CS_F_UNTRIMMED;
            }
          }
        }
      } else {
        const uint16_t *table = reinterpret_cast<const uint16_t *>((uintptr_t)d.peq[0]);
        if (on) {
          const int take = min(n, span);
          uint32_t idx = 0, pw = 1, block = 0;  // block: where the prefixes of length `take` start
          for (int u = 0; u < span; ++u) {      // uniform
            if (u < take) {
              const uint32_t c = row_code<CODED>(myrow, s + u);
              uint32_t digit;
              if (CODED)
                digit = (c & 0x20u) ? 4u : (c >> 3);
              else
                digit = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? ((c >> 1) & 3u) : 4u;
              idx += digit * pw;
              block += pw;
            }
            pw *= 5u;
          }
          const uint32_t entry = table[block + idx];
          const uint32_t id = entry & 0xffu;
          if (id != CS_DEMUX_NONE) {
            s += (int)((entry >> 8) & 0xfu);  // PrefixAdapter: RemoveBeforeMatch
            meta += 1u;
            fm |= (uint32_t)op.match_flag | (0x100u << t);
            if (entry & 0x4000u) fm |= CS_F_AMBIGUOUS;
            meta = (meta & 0xff00ffffu) | (id << 16);
          } else if (op.required) {
            fm |= CS_F_UNTRIMMED;
          }
        }
      }
    } else if (kind == CS_OP_QTRIM) {
      // BWA running sum from the 3' end (cutadapt quality_trim_index), quality bytes straight from HBM.
      // The reference walks i = n-1 .. 0: sum += cutoff - (q[i] - base); stop at the first negative sum; the
      // answer is the position of the first strict maximum.  (sum, position) packed into one key -- sum
      // in the high bits, position below -- turns "first strict maximum" into a plain running max: a later
      // (lower) position wins only with a larger sum.  The dword that holds the read's last base and the
      // dword in which a lane's sum first turns negative (or the partial dword at the start of the interval)
      // go through the exact per-base routine; everything in between is whole dwords of a lane that is
      // still alive: four prefix sums, one sign test, one max.
      const uint32_t *q = reinterpret_cast<const uint32_t *>(ma.qual + (size_t)gr * a.stride_dw * 4u);
      const int cq = (int)op.q_cutoff + (int)op.q_base;  // what a base adds: cq - quality byte
      int stop = n;
      {
        const bool live = on && n > 0;
        const int p_last = s + n - 1;
        constexpr int kPosBits = 11;  // positions < 2048 (CS_MAX_STRIDE = 1536)
        // the key is an int: position below the start key's 2047, running sum (at most kQTermMax a base over a row,
        // the cutoff clamped by cs_plan_create) in the 31 - kPosBits bits above it
        static_assert(CS_MAX_STRIDE < (1 << kPosBits) - 1 && kQCutoffHigh <= kQTermMax && 255 - kQCutoffLow <= kQTermMax &&
                          (long long)kQTermMax * CS_MAX_STRIDE < (1ll << (31 - kPosBits)),
                      "QTRIM key: sum << kPosBits | position must fit an int");
        int sum = 0, bestkey = (1 << kPosBits) - 1;  // sum 0 at a position beyond every real one: only sums > 0 replace it
        bool alive = live;
        auto exact4 = [&](uint32_t w, int pbase, bool take) {  // the four bases of one dword, 3' -> 5', with range checks
#pragma unroll
          for (int b = 3; b >= 0; --b) {
            const int p = pbase + b;
            const bool in = take && (p <= p_last) && (p >= s);
            const int nsum = sum + cq - (int)((w >> (b * 8)) & 0xffu);
            alive = alive && !(in && nsum < 0);
            const bool on_b = in && alive;
            sum = on_b ? nsum : sum;
            const int key = (nsum << kPosBits) | p;
            bestkey = on_b ? max(bestkey, key) : bestkey;
          }
        };
        const int dw_top = p_last >> 2;
        uint32_t w_top = 0;
        if (live) w_top = q[max(dw_top, 0)];
        exact4(w_top, 4 * dw_top, live);
        // Below the top dword the WAVE walks, not the lane.  Three reads in four stop inside the top dword (the first
        // base already drives the sum negative); one in ten walks on for 20 to 110 bases, and a lane-per-read loop
        // makes all 64 lanes pay for the longest of them (85 bases per tile on the bench reads, 7 on average).  So the
        // reads that are still alive are served four at a time, 16 lanes each: lane i of a group takes the read's
        // i-th dword below the position reached, the running sums come from a prefix scan over the group (DPP row
        // shifts), the first lane whose sums turn negative ends the walk, the best (sum, position) key of the lanes up
        // to it is a row maximum.  One round = 64 bases of four reads.
        int dw = dw_top - 1;                       // next dword of this lane's read
        bool run = alive && (4 * dw_top > s);      // positions left below the top dword
        const int grp = lane >> 4, idx = lane & 15;
        unsigned long long todo = __ballot(run);
        while (todo) {  // wave-uniform
          unsigned long long t = todo;
          const int l0 = __builtin_ctzll(t);
          t &= t - 1ull;
          const int l1 = t ? __builtin_ctzll(t) : -1;
          t &= t - 1ull;  // (0 stays 0)
          const int l2 = t ? __builtin_ctzll(t) : -1;
          t &= t - 1ull;
          const int l3 = t ? __builtin_ctzll(t) : -1;
          const int src = grp == 0 ? l0 : grp == 1 ? l1 : grp == 2 ? l2 : l3;  // the read this lane's group serves
          const int from = max(src, 0);
          const int r_sum = __shfl(sum, from, 64);
          const int r_pk = __shfl((s << 16) | (dw & 0xffff), from, 64);
          const uint32_t r_gr = SCAN ? row0 + (uint32_t)from : (uint32_t)__shfl((int)gr, from, 64);
          const int r_s = r_pk >> 16, r_dw = r_pk & 0xffff;
          const int d = r_dw - idx;                       // this lane's dword of that read
          const bool ok = src >= 0 && d >= (r_s >> 2);
          uint32_t w = 0;
          if (ok) w = reinterpret_cast<const uint32_t *>(ma.qual + (size_t)r_gr * a.stride_dw * 4u)[d];
          // positions below the interval's start (the low bytes of its lowest dword) add nothing: their sums repeat the
          // one before, same sum at a lower position -- such a key never wins
          const int skip = r_s - 4 * d;  // low bytes outside the interval (<= 0: none; 1..3 in the lowest dword)
          const int c3 = cq - (int)(w >> 24);
          const int c2 = skip > 2 ? 0 : cq - (int)((w >> 16) & 0xffu);
          const int c1 = skip > 1 ? 0 : cq - (int)((w >> 8) & 0xffu);
          const int c0 = skip > 0 ? 0 : cq - (int)(w & 0xffu);
          const int p3 = c3, p2 = p3 + c2, p1 = p2 + c1, p0 = p1 + c0;  // sums inside the dword, 3' -> 5'
          const int tot = ok ? p0 : 0;
          int incl = tot;  // inclusive scan over the 16 lanes of the group
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
          const int off = r_sum + incl - tot;  // the read's running sum in front of this dword
          const int a3 = off + p3, a2 = off + p2, a1 = off + p1, a0 = off + p0;
          const int o2 = a3 | a2, o1 = o2 | a1, o0 = o1 | a0;  // sign bit: some sum down to here was negative
          const unsigned long long nm = __ballot(ok && o0 < 0);
          const uint32_t seg = ((grp & 2) ? (uint32_t)(nm >> 32) : (uint32_t)nm) >> ((grp & 1) * 16) & 0xffffu;
          const int first = seg ? __builtin_ctz(seg) : 16;  // the group's first lane with a negative sum
          const bool before = ok && idx < first, at = ok && idx == first;
          const int pb = 4 * d;
          const int k3 = (before || (at && a3 >= 0)) ? ((a3 << kPosBits) | (pb + 3)) : 0;
          const int k2 = (before || (at && o2 >= 0)) ? ((a2 << kPosBits) | (pb + 2)) : 0;
          const int k1 = (before || (at && o1 >= 0)) ? ((a1 << kPosBits) | (pb + 1)) : 0;
          const int k0 = before ? ((a0 << kPosBits) | pb) : 0;  // (the lane AT the stop has a negative sum by its last base)
          int kmax = max(max(k3, k2), max(k1, k0));  // maximum over the group, in every lane of it
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x121 /* row_ror:1 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x122 /* row_ror:2 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x124 /* row_ror:4 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x128 /* row_ror:8 */, 0xf, 0xf, false));
          // back to the reads' own lanes: from the last lane of the group that served them
          const int mine = lane == l0 ? 0 : lane == l1 ? 1 : lane == l2 ? 2 : lane == l3 ? 3 : -1;
          const int back = 16 * max(mine, 0) + 15;
          const int g_key = __shfl(kmax, back, 64);
          const int g_end = __shfl((max(r_sum + incl, 0) << 5) | first, back, 64);  // running sum behind the group | first
          if (mine >= 0) {
            bestkey = max(bestkey, g_key);
            const bool stopped = (g_end & 31) < 16;
            sum = g_end >> 5;
            dw -= 16;
            run = !stopped && dw >= (s >> 2);
          }
          todo = __ballot(run);
        }
        if (live && (bestkey >> kPosBits) > 0) stop = (bestkey & ((1 << kPosBits) - 1)) - s;
      }
      if constexpr (FILT >= FILT_ENDS) {
        // The 5' walk of quality_trim_index (cutoff_front), for ops that have one: forward from s over the WHOLE interval
        // the op saw, whatever the 3' walk above decided -- sum += cutoff_front - (q[i] - base), stop at the first
        // negative sum, start = one behind the first strict maximum.  One lane per read, dwords straight from the read's
        // row like the walk above, the bytes of the first and last dword outside [s, e) passed over; 5' ends are the
        // good end of a read, a walk is expected to end in its first dword.  A plain int sum: at most kQTermMax a base
        // over a row, the bound of the 3' key's sum.  (The cutoff is the high half of the op's last dword: a scalar load.)
        static_assert(offsetof(cs_op, q_cutoff_front) == 282 && sizeof(cs_op) == 284, "cs_op: q_cutoff_front ends the struct");
        const int front = (int)reinterpret_cast<const uint32_t *>(&d.op)[70] >> 16;
        int start = 0;
        if (front != 0) {  // wave-uniform; 0: the reference's op, no byte is looked at
          const int cf = front + (int)op.q_base;
          if (on && n > 0) {
            const int d_last = (e - 1) >> 2;
            int sum = 0, best = 0;
            bool dead = false;
            for (int dwf = s >> 2; dwf <= d_last && !dead; ++dwf) {
              const uint32_t w = q[dwf];
#pragma unroll
              for (int b = 0; b < 4; ++b) {
                const int p = 4 * dwf + b;
                const bool in = !dead && p >= s && p < e;
                const int nsum = sum + cf - (int)((w >> (b * 8)) & 0xffu);
                dead = dead || (in && nsum < 0);
                const bool on_b = in && !dead;
                sum = on_b ? nsum : sum;
                const bool up = on_b && sum > best;
                best = up ? sum : best;
                start = up ? p + 1 - s : start;
              }
            }
          }
          if (start >= stop) start = stop = 0;  // (the two walks crossed: nothing is left, reported as [s, s))
        }
        if (on) {
          if (stop - start < n) fm |= CS_F_QTRIMMED;
          qc += (uint32_t)(n - (stop - start));
          e = s + stop;
          s += start;
        }
      } else if (on) {
        if (stop < n) fm |= CS_F_QTRIMMED;
        qc += (uint32_t)(n - stop);
        e = s + stop;
      }
      CS_T_MARK(pt, 5);
    } else if (kind == CS_OP_NEXTSEQ) {
      if constexpr (FILT >= FILT_NEXTSEQ) {
        // cutadapt's NextseqQualityTrimmer (--nextseq-trim): the 3' walk of the CS_OP_QTRIM branch above with one more
        // input, the read's base at each position -- a 'G' adds 1 whatever its quality byte says.  The same top-dword
        // exact step, the same wave walk (four live reads, 16 lanes each), the same (sum, position) key; wherever a
        // quality dword is loaded the sequence dword at the same index of the same row is loaded with it.  The read's
        // OWN bytes decide on every tile: raw tiles fold case for the aligner and 'g' must not count, and in the wave
        // walk a lane serves other lanes' reads, whose codes are not in its row -- so no choice between codes and bytes
        // is made at all (compare CS_OP_NTRIM below).  A G's term lies within kQTermMax like every other one
        // (cs_plan_create refuses a cutoff outside [kQCutoffLow, kQCutoffHigh] - base): the key's static_assert holds.
        // The op never moves s.  (FILT_NEXTSEQ, not FILT_ENDS: see the enum.)
        const uint32_t *q = reinterpret_cast<const uint32_t *>(ma.qual + (size_t)gr * a.stride_dw * 4u);
        const uint32_t *bs = ma.seq + (size_t)gr * a.stride_dw;
        const int cq = (int)op.q_cutoff + (int)op.q_base;
        auto term = [&](uint32_t w, uint32_t g, int b) -> int {  // what byte b of a dword adds
          return ((g >> (b * 8)) & 0xffu) == 0x47u ? 1 : cq - (int)((w >> (b * 8)) & 0xffu);
        };
        int stop = n;
        const bool live = on && n > 0;
        const int p_last = s + n - 1;
        constexpr int kPosBits = 11;
        static_assert(CS_MAX_STRIDE < (1 << kPosBits) - 1 && kQTermMax >= 1 &&
                          (long long)kQTermMax * CS_MAX_STRIDE < (1ll << (31 - kPosBits)),
                      "NEXTSEQ key: sum << kPosBits | position must fit an int");
        int sum = 0, bestkey = (1 << kPosBits) - 1;
        bool alive = live;
        const int dw_top = p_last >> 2;
        uint32_t w_top = 0, g_top = 0;
        if (live) {
          w_top = q[max(dw_top, 0)];
          g_top = bs[max(dw_top, 0)];
        }
#pragma unroll
        for (int b = 3; b >= 0; --b) {  // the top dword, 3' -> 5', with range checks
          const int p = 4 * dw_top + b;
          const bool in = live && (p <= p_last) && (p >= s);
          const int nsum = sum + term(w_top, g_top, b);
          alive = alive && !(in && nsum < 0);
          const bool on_b = in && alive;
          sum = on_b ? nsum : sum;
          const int key = (nsum << kPosBits) | p;
          bestkey = on_b ? max(bestkey, key) : bestkey;
        }
        int dw = dw_top - 1;
        bool run = alive && (4 * dw_top > s);
        const int grp = lane >> 4, idx = lane & 15;
        unsigned long long todo = __ballot(run);
        while (todo) {  // wave-uniform
          unsigned long long tt = todo;
          const int l0 = __builtin_ctzll(tt);
          tt &= tt - 1ull;
          const int l1 = tt ? __builtin_ctzll(tt) : -1;
          tt &= tt - 1ull;
          const int l2 = tt ? __builtin_ctzll(tt) : -1;
          tt &= tt - 1ull;
          const int l3 = tt ? __builtin_ctzll(tt) : -1;
          const int src = grp == 0 ? l0 : grp == 1 ? l1 : grp == 2 ? l2 : l3;
          const int from = max(src, 0);
          const int r_sum = __shfl(sum, from, 64);
          const int r_pk = __shfl((s << 16) | (dw & 0xffff), from, 64);
          const uint32_t r_gr = SCAN ? row0 + (uint32_t)from : (uint32_t)__shfl((int)gr, from, 64);
          const int r_s = r_pk >> 16, r_dw = r_pk & 0xffff;
          const int dd = r_dw - idx;  // this lane's dword of that read
          const bool ok = src >= 0 && dd >= (r_s >> 2);
          uint32_t w = 0, g = 0;
          if (ok) {
            w = reinterpret_cast<const uint32_t *>(ma.qual + (size_t)r_gr * a.stride_dw * 4u)[dd];
            g = (ma.seq + (size_t)r_gr * a.stride_dw)[dd];
          }
          const int skip = r_s - 4 * dd;  // low bytes outside the interval: they add nothing, 'G' or not
          const int c3 = term(w, g, 3);
          const int c2 = skip > 2 ? 0 : term(w, g, 2);
          const int c1 = skip > 1 ? 0 : term(w, g, 1);
          const int c0 = skip > 0 ? 0 : term(w, g, 0);
          const int p3 = c3, p2 = p3 + c2, p1 = p2 + c1, p0 = p1 + c0;
          const int tot = ok ? p0 : 0;
          int incl = tot;
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
          const int off = r_sum + incl - tot;
          const int a3 = off + p3, a2 = off + p2, a1 = off + p1, a0 = off + p0;
          const int o2 = a3 | a2, o1 = o2 | a1, o0 = o1 | a0;
          const unsigned long long nm = __ballot(ok && o0 < 0);
          const uint32_t seg = ((grp & 2) ? (uint32_t)(nm >> 32) : (uint32_t)nm) >> ((grp & 1) * 16) & 0xffffu;
          const int first = seg ? __builtin_ctz(seg) : 16;
          const bool before = ok && idx < first, at = ok && idx == first;
          const int pb = 4 * dd;
          const int k3 = (before || (at && a3 >= 0)) ? ((a3 << kPosBits) | (pb + 3)) : 0;
          const int k2 = (before || (at && o2 >= 0)) ? ((a2 << kPosBits) | (pb + 2)) : 0;
          const int k1 = (before || (at && o1 >= 0)) ? ((a1 << kPosBits) | (pb + 1)) : 0;
          const int k0 = before ? ((a0 << kPosBits) | pb) : 0;
          int kmax = max(max(k3, k2), max(k1, k0));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x121 /* row_ror:1 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x122 /* row_ror:2 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x124 /* row_ror:4 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x128 /* row_ror:8 */, 0xf, 0xf, false));
          const int mine = lane == l0 ? 0 : lane == l1 ? 1 : lane == l2 ? 2 : lane == l3 ? 3 : -1;
          const int back = 16 * max(mine, 0) + 15;
          const int g_key = __shfl(kmax, back, 64);
          const int g_end = __shfl((max(r_sum + incl, 0) << 5) | first, back, 64);
          if (mine >= 0) {
            bestkey = max(bestkey, g_key);
            const bool stopped = (g_end & 31) < 16;
            sum = g_end >> 5;
            dw -= 16;
            run = !stopped && dw >= (s >> 2);
          }
          todo = __ballot(run);
        }
        if (live && (bestkey >> kPosBits) > 0) stop = (bestkey & ((1 << kPosBits) - 1)) - s;
        if (on) {
          if (stop < n) fm |= CS_F_QTRIMMED;
          qc += (uint32_t)(n - stop);
          e = s + stop;
        }
      }
    } else if (kind == CS_OP_POLYA) {
      if constexpr (POLYA) {
        // cutadapt's PolyATrimmer (--poly-a), poly_a_trim_index: from the read's 3' end a base 'A' adds 1 to the score,
        // any other byte takes 2 and counts as an error; a position qualifies while errors * 5 <= length, and the FIRST
        // qualifying position of the highest score > 0 is where the tail begins; tails shorter than 3 stay.
        // With score = length - 3 * errors the rate test is 5 * score >= 2 * length: no error count is kept, and the
        // result is a maximum over (score << kPosBits | position) keys, CS_OP_QTRIM's key (a lower position wins only
        // with a higher score).  Unlike that walk this one has no "sum < 0" end: it is over when no later position can
        // beat the best score (score + bases left <= best) or qualify (5 * (score + bases left) < 2 * n), on random
        // bases after about 0.27 n of them.  Every read walks, so the WAVE walks from the start, in rounds of 64 bases
        // (16 dwords) of a read.  The FIRST round of every read is served statically, 16 reads at a time, four lanes
        // each: lane q of a quad takes the read's dwords 4q .. 4q + 3 below its top one, scores by a prefix scan over
        // the quad, the best key a quad maximum -- four turns a tile, and a 150-base read without a tail is settled.
        // Reads that go on (tails, long rows) are then served four at a time, 16 lanes each, a dword a lane, as
        // CS_OP_QTRIM serves its live reads: scores by a prefix scan over the group, the best key a row maximum.
        // The read's OWN bytes decide on every tile, as for CS_OP_NEXTSEQ and for its reasons: case matters ('a' is an
        // error, raw tiles fold it), and a lane serves other lanes' reads.
        // The head form (reversed: poly-T at the 5' end) is the same walk on the mirrored row: position p of the row is
        // position 2047 - p, so dword d is dword 511 - d with its bytes swapped, [s, e) is [2048 - e, 2048 - s), and the
        // first position in walk order is again the highest one.  |score| <= 2 * CS_MAX_STRIDE: the key fits an int.
        constexpr int kPosBits = 11, kTop = (1 << kPosBits) - 1;
        static_assert(CS_MAX_STRIDE <= kTop + 1 && (kTop & 3) == 3 && 2ll * CS_MAX_STRIDE < (1ll << (31 - kPosBits)),
                      "POLYA key: score << kPosBits | (mirrored) position must fit an int");
        const bool rev = op.reversed != 0;            // wave-uniform
        const uint32_t match = rev ? 0x54u : 0x41u;   // 'T' / 'A', upper case only
        const bool live = on && n > 0;
        const int ms = rev ? (kTop + 1) - e : s;      // the interval in walk coordinates: [ms, ms + n)
        const int p_last = ms + n - 1;
        int sum = 0, bestkey = kTop;  // score 0 at a position beyond every real one: only scores > 0 replace it
        int dw = max(p_last, 0) >> 2;  // next dword of this lane's read (walk coordinates)
        bool run = live;
        const int grp = lane >> 4, idx = lane & 15;
        unsigned long long todo = __ballot(run);
        auto settled = [&](int score, int best, int left) -> bool {  // no base left, or none that could change the result
          return left <= 0 || score + left <= best || 5 * (score + left) < 2 * n;
        };
        for (int turn = 0; turn < 4; ++turn) {  // the first round, lanes 16 * turn .. 16 * turn + 15; wave-uniform
          if (((todo >> (16 * turn)) & 0xffffull) == 0ull) continue;
          const int from = 16 * turn + (lane >> 2), quad = lane & 3;
          const bool r_run = ((todo >> from) & 1ull) != 0ull;
          const uint32_t r_pk = (uint32_t)__shfl((int)((uint32_t)ms | ((uint32_t)max(p_last, 0) << 12) | ((uint32_t)dw << 23)), from, 64);
          const uint32_t r_gr = SCAN ? row0 + (uint32_t)from : (uint32_t)__shfl((int)gr, from, 64);
          const int r_ms = (int)(r_pk & 0xfffu), r_last = (int)((r_pk >> 12) & 0x7ffu), r_dw = (int)(r_pk >> 23);
          const uint32_t *rowp = ma.seq + (size_t)r_gr * a.stride_dw;
          const int d0 = r_dw - 4 * quad;  // this lane's four dwords: d0 down to d0 - 3
          uint32_t g4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {  // (a dword inside the interval's dwords, and so is its mirror image: inside the row)
            const int dd = d0 - j;
            g4[j] = 0;
            if (r_run && dd >= (r_ms >> 2)) g4[j] = rev ? __builtin_bswap32(rowp[(kTop >> 2) - dd]) : rowp[dd];
          }
          int sc[16], tot = 0;  // the scores inside the lane's 16 bases, 3' -> 5'; bases outside the interval add nothing
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 3; b >= 0; --b) {
              const int p = 4 * (d0 - j) + b;
              const bool in = r_run && p >= r_ms && p <= r_last;
              tot += !in ? 0 : ((g4[j] >> (b * 8)) & 0xffu) == match ? 1 : -2;
              sc[4 * j + 3 - b] = tot;
            }
          int incl = tot;  // inclusive scan over the quad (the read's score starts at 0: this is its first round)
          const int up1 = __builtin_amdgcn_update_dpp(0, incl, 0x90 /* quad_perm:[0,0,1,2] */, 0xf, 0xf, false);
          incl += quad >= 1 ? up1 : 0;
          const int up2 = __builtin_amdgcn_update_dpp(0, incl, 0x44 /* quad_perm:[0,1,0,1] */, 0xf, 0xf, false);
          incl += quad >= 2 ? up2 : 0;
          const int off = incl - tot;
          int kmax = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 3; b >= 0; --b) {
              const int p = 4 * (d0 - j) + b, s1 = off + sc[4 * j + 3 - b];
              const bool q = r_run && p >= r_ms && p <= r_last && s1 > 0 && 5 * s1 >= 2 * (r_last - p + 1);
              kmax = max(kmax, q ? ((s1 << kPosBits) | p) : 0);
            }
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0xB1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x4E /* quad_perm:[2,3,0,1] */, 0xf, 0xf, false));
          // back to the reads' own lanes: lane 16 * turn + i was served by quad i, whose last lane has the read's score
          const int back = 4 * (lane & 15) + 3;
          const int g_key = __shfl(kmax, back, 64);
          const int g_sum = __shfl(incl, back, 64);
          if ((lane >> 4) == turn && run) {
            bestkey = max(bestkey, g_key);
            sum = g_sum;
            dw -= 16;
            run = !settled(sum, bestkey >> kPosBits, 4 * dw + 4 - ms);
          }
        }
        todo = __ballot(run);
        while (todo) {  // wave-uniform
          unsigned long long tt = todo;
          const int l0 = __builtin_ctzll(tt);
          tt &= tt - 1ull;
          const int l1 = tt ? __builtin_ctzll(tt) : -1;
          tt &= tt - 1ull;
          const int l2 = tt ? __builtin_ctzll(tt) : -1;
          tt &= tt - 1ull;
          const int l3 = tt ? __builtin_ctzll(tt) : -1;
          const int src = grp == 0 ? l0 : grp == 1 ? l1 : grp == 2 ? l2 : l3;  // the read this lane's group serves
          const int from = max(src, 0);
          const int r_sum = __shfl(sum, from, 64);
          const uint32_t r_pk = (uint32_t)__shfl((int)((uint32_t)ms | ((uint32_t)max(p_last, 0) << 12) | ((uint32_t)dw << 23)), from, 64);
          const uint32_t r_gr = SCAN ? row0 + (uint32_t)from : (uint32_t)__shfl((int)gr, from, 64);
          const int r_ms = (int)(r_pk & 0xfffu), r_last = (int)((r_pk >> 12) & 0x7ffu), r_dw = (int)(r_pk >> 23);
          const int dd = r_dw - idx;  // this lane's dword of that read
          const bool ok = src >= 0 && dd >= (r_ms >> 2);
          uint32_t g = 0;
          if (ok) {  // (dd lies inside the interval's dwords, and so does its mirror image: both inside the row)
            g = (ma.seq + (size_t)r_gr * a.stride_dw)[rev ? (kTop >> 2) - dd : dd];
            if (rev) g = __builtin_bswap32(g);
          }
          const int pb = 4 * dd;
          auto term = [&](int b) -> int {  // what byte b adds; nothing outside the interval (top and lowest dword)
            const bool in = ok && pb + b >= r_ms && pb + b <= r_last;
            return !in ? 0 : ((g >> (b * 8)) & 0xffu) == match ? 1 : -2;
          };
          const int c3 = term(3), c2 = term(2), c1 = term(1), c0 = term(0);
          const int p3 = c3, p2 = p3 + c2, p1 = p2 + c1, p0 = p1 + c0;  // scores inside the dword, 3' -> 5'
          const int tot = p0;
          int incl = tot;  // inclusive scan over the 16 lanes of the group
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
          incl += __builtin_amdgcn_update_dpp(0, incl, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
          const int off = r_sum + incl - tot;  // the read's score in front of this dword
          auto key = [&](int b, int sc) -> int {  // the candidate that ends at byte b with score sc
            const int p = pb + b;
            const bool q = ok && p >= r_ms && p <= r_last && sc > 0 && 5 * sc >= 2 * (r_last - p + 1);
            return q ? ((sc << kPosBits) | p) : 0;
          };
          int kmax = max(max(key(3, off + p3), key(2, off + p2)), max(key(1, off + p1), key(0, off + p0)));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x121 /* row_ror:1 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x122 /* row_ror:2 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x124 /* row_ror:4 */, 0xf, 0xf, false));
          kmax = max(kmax, __builtin_amdgcn_update_dpp(0, kmax, 0x128 /* row_ror:8 */, 0xf, 0xf, false));
          // back to the reads' own lanes: from the last lane of the group that served them
          const int mine = lane == l0 ? 0 : lane == l1 ? 1 : lane == l2 ? 2 : lane == l3 ? 3 : -1;
          const int back = 16 * max(mine, 0) + 15;
          const int g_key = __shfl(kmax, back, 64);
          const int g_sum = __shfl(r_sum + incl, back, 64);  // the read's score behind the group's 64 bases
          if (mine >= 0) {
            bestkey = max(bestkey, g_key);
            sum = g_sum;
            dw -= 16;
            run = !settled(sum, bestkey >> kPosBits, 4 * dw + 4 - ms);  // (bases of the interval below the position reached)
          }
          todo = __ballot(run);
        }
        if (on) {
          int index = n;
          if (live && (bestkey >> kPosBits) > 0) index = (bestkey & kTop) - ms;
          if (index > n - 3) index = n;
          polya_bp += (uint32_t)(n - index);
          if (rev)
            s = e - index;
          else
            e = s + index;
        }
      }
    } else if (kind == CS_OP_SHORTEN) {
      if constexpr (FILT >= FILT_SHORTEN) {
        // cutadapt's Shortener (-l / -L): min(n, |length|) bases stay, the first ones or, length < 0, the last ones.
        // Lane-local; the length is wave-uniform (a scalar dword of the op).  |length| is formed unsigned -- 2^31 for
        // INT32_MIN, which no int holds -- and n, never negative, is compared with it as such.  No flag, no counter.
        const int length = op.length;
        const int keep = (int)min((uint32_t)n, length < 0 ? 0u - (uint32_t)length : (uint32_t)length);
        if (on) {
          if (length >= 0)
            e = s + keep;
          else
            s = e - keep;
        }
      }
    } else if (kind == CS_OP_NTRIM) {
      if constexpr (FILT >= FILT_ENDS) {
        // cutadapt's NEndTrimmer: the runs of 'N' (upper case only) at both ends of [s, e) go.  A fast-form coded tile
        // vouches for every byte being A, C, G, T or N, code 7 is 'N' and nothing else (count_n_nibbles); everywhere else
        // -- raw tiles fold case, exact-form tiles and the resolve kernel's mix codes 4..7 -- the read's own bytes decide.
        // A read without an N at either end, nearly every read, costs one test per end.
        // (The choice is made ONCE, on a scalar: as a wave-uniform bool tested inside the two loops below it was kept in a
        // lane mask that the first loop rewrote under its shrinking exec mask, and lanes that had left that loop early
        // took the tile's codes on an exact-form tile in the second one -- an 'n' next to a trimmed 'N' went with it.)
        const bool vouched = __builtin_amdgcn_readfirstlane((SCAN && CODED && a.fast_recode == 1u && !fast_failed) ? 1 : 0) != 0;
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(ma.seq + (size_t)gr * a.stride_dw);
        auto trim_ends = [&](auto is_n) {
          if (on && n > 0) {
            int lead = 0;
            while (lead < n && is_n(s + lead)) ++lead;
            if (lead == n) {
              e = s;
            } else {  // (some base of the interval is no N: the walk from the end stops there at the latest)
              s += lead;
              while (e > s && is_n(e - 1)) --e;
            }
          }
        };
        if (vouched)
          trim_ends([&](int pos) -> bool { return ((myrow[pos >> 3] >> ((pos & 7) << 2)) & 7u) == 7u; });
        else
          trim_ends([&](int pos) -> bool { return bytes[pos] == 0x4Eu; });
      }
    }
  }

  // ---- scan kernel: the tile's deferred reads.  Their records wait in the LDS ring as a rule (reservation a tile
  // later, see above); only a tile that defers more reads than the ring takes reserves and writes at once
  const bool fin = here && !deferred;
  uint32_t q_pos = 0;
  unsigned long long def_mask = 0;
  bool park = false;  // wave-uniform: this tile's records fit the ring
  if (SCAN) {
    def_mask = __ballot(deferred && !refl);
    // the ring takes this tile's records behind the ones it keeps (those whose reservation was not asked for yet)
    park = (pend_asked ? 0u : pend_count) + (uint32_t)__popcll(def_mask) <= (uint32_t)kRingRecords;
    if (def_mask && !park && lane == 0)
      q_pos = atomic_add_later(&a.defer_count[mate * kTileCounterStride], (uint32_t)__popcll(def_mask));
  }

  if (fin) {
    if (e - s < min_length) fm |= CS_F_TOO_SHORT;
    static_assert(sizeof(cs_result) == 8 && offsetof(cs_result, stop) == 2 && offsetof(cs_result, cap_off) == 4 &&
                  offsetof(cs_result, cap_len) == 6 && offsetof(cs_result, flags) == 7, "cs_result layout");
    if ((((uintptr_t)ma.out) & 7u) == 0) {  // (wave-uniform) the record as ONE eight-byte store, not five narrow ones
      uint2 r;
      r.x = ((uint32_t)s & 0xffffu) | ((uint32_t)e << 16);
      r.y = (capo & 0xffffu) | (((qc >> 16) & 0xffu) << 16) | (fm << 24);
      *reinterpret_cast<uint2 *>(ma.out + gr) = r;
    } else {
      cs_result r;
      r.start = (uint16_t)s;
      r.stop = (uint16_t)e;
      r.cap_off = (uint16_t)capo;
      r.cap_len = (uint8_t)(qc >> 16);
      r.flags = (uint8_t)fm;
      ma.out[gr] = r;
    }
    if (ma.cap2) {
      cs_cap2 c2;
      c2.off = (uint16_t)(capo >> 16);
      c2.len = (uint8_t)(qc >> 24);
      c2._pad = 0;
      ma.cap2[gr] = c2;
    }
    if (ma.bc) ma.bc[gr] = (uint8_t)(meta >> 16);
  }

  // ---- the filters of the final interval (cs_plan_set_max_n / _max_length / _max_ee): kernels of their own (FILT), so
  // that a plan without a filter runs exactly the code it ran before (in the scan kernel's register budget any code
  // here costs a spill), and a plan with TooManyN alone the code it ran before the other two came
  if constexpr (FILT != FILT_NONE) {
    const bool with_n = FILT == FILT_MAXN || plan->max_n_on;  // (wave-uniform, like the two below)
    bool many = false;
    if (fin && with_n) {
      uint32_t nn;
      // the fast form vouched for every byte of the tile exactly when the wave's staging has not failed (mode 1 only:
      // mode 2 never stages again, whatever the bytes are)
      if (SCAN && CODED && a.fast_recode == 1u && !fast_failed)
        nn = count_n_nibbles(myrow, s, e);
      else if (!CODED)
        nn = count_n_bytes(myrow, s, e);
      else  // an exact-form tile (or the resolve kernel's): the read's own bytes
        nn = count_n_bytes(ma.seq + (size_t)gr * a.stride_dw, s, e);
      many = too_many_n(nn, e - s, plan->max_n);
    }
    const uint32_t w_many = wave_count(many);
    if (lane == 0 && w_many) atomicAdd(&sacc[ST_TOO_MANY_N], w_many);
    uint32_t xf = many ? (uint32_t)CS_X_TOO_MANY_N : 0u;
    if constexpr (FILT >= FILT_ALL) {
      const bool is_long = fin && plan->max_length_on && e > s && (uint32_t)(e - s) > plan->max_length;
      bool errs = false;
      if (plan->max_ee_on && ma.qual) {  // the read's own quality row, as the quality trimmer reads it
        double ee = 0.0;
        if (fin)
          ee = expected_errors(reinterpret_cast<const uint32_t *>(ma.qual + (size_t)gr * a.stride_dw * 4u), s, e,
                               plan->ee_table, plan->ee_reversed != 0);
        errs = ee > plan->max_ee;
      }
      xf |= (is_long ? (uint32_t)CS_X_TOO_LONG : 0u) | (errs ? (uint32_t)CS_X_TOO_MANY_EE : 0u);
      const uint32_t w_long = wave_count(is_long), w_errs = wave_count(errs);
      unsigned long long *xst = a.stats + kXStatBase + mate * kXStatWords;
      if (lane == 0 && w_long) atomicAdd(&xst[XST_TOO_LONG], (unsigned long long)w_long);
      if (lane == 0 && w_errs) atomicAdd(&xst[XST_TOO_MANY_EE], (unsigned long long)w_errs);
    }
    if (fin && ma.xflags) ma.xflags[gr] = (uint8_t)xf;
  }

  // ---- statistics of this tile (reads that finished here): wave sums -> LDS accumulators
  {
    const uint32_t w_reads = wave_count(fin);
    // (rows of up to 1020 bases: a wave's sums stay below 2^16, two of them share one reduction)
    const bool narrow = a.stride_dw <= 255u;  // wave-uniform
    uint32_t w_in, w_out, w_qt, w_exact;
    if (narrow) {
      const uint32_t io = wave_sum(fin ? ((uint32_t)len | ((uint32_t)(e - s) << 16)) : 0u);
      const uint32_t qx = wave_sum((fin ? (qc & 0xffffu) : 0u) | (((meta >> 8) & 0xffu) << 16));
      w_in = io & 0xffffu, w_out = io >> 16, w_qt = qx & 0xffffu, w_exact = qx >> 16;
    } else {
      w_in = wave_sum(fin ? (uint32_t)len : 0u);
      w_out = wave_sum(fin ? (uint32_t)(e - s) : 0u);
      w_qt = wave_sum(fin ? (qc & 0xffffu) : 0u);
      w_exact = wave_sum((meta >> 8) & 0xffu);
    }
    const uint32_t w_short = wave_count(fin && (fm & CS_F_TOO_SHORT));
    const uint32_t w_untr = wave_count(fin && (fm & CS_F_UNTRIMMED));
    // (diagnostic: reads the existence-only scan could not clear -- they are filtered exactly by the resolve kernel)
    const uint32_t w_refilter = SCAN ? wave_count(deferred && rec_rmax == 0xffu) : 0u;
    if (lane == 0) {
      if (w_refilter) atomicAdd(&sacc[ST_RESERVED], w_refilter);
      atomicAdd(&sacc[ST_READS], w_reads);
      atomicAdd(&sacc[ST_IN_BP], w_in);
      atomicAdd(&sacc[ST_OUT_BP], w_out);
      atomicAdd(&sacc[ST_QTRIM_BP], w_qt);
      atomicAdd(&sacc[ST_TOO_SHORT], w_short);
      atomicAdd(&sacc[ST_UNTRIMMED], w_untr);
      atomicAdd(&sacc[ST_EXACT_DP], w_exact);
    }
    for (int t = 0; t < n_ops; ++t) {
      const unsigned long long bal = __ballot(fin && ((fm >> (8 + t)) & 1u));
      if (lane == 0 && bal) atomicAdd(&sacc[ST_OPS + plan->ops[mate][t].f.stat_slot], (uint32_t)__popcll(bal));
    }
  }

  if (SCAN && refl_any) {  // records of the queue's top region (same layout as below)
    const uint32_t qb = (uint32_t)__builtin_amdgcn_readfirstlane((int)refl_q);
    if (refl) {
      uint4 ra, rb;
      ra.x = gr;
      ra.y = (uint32_t)s | ((uint32_t)e << 16);
      ra.z = rec_win;
      ra.w = rec_rows;
      rb.x = (fm >> 8) | (meta & 0xff000000u);
      rb.y = (fm & 0xffu) | ((meta & 0xffu) << 8) | ((rec_rmax & 0xffu) << 16) | ((qc << 8) & 0xff000000u);
      rb.z = capo;
      rb.w = (qc >> 24) | ((qc & 0xffffu) << 8) | ((meta << 8) & 0xff000000u);
      uint4 *rec = a.defer[mate] + (size_t)(a.defer_cap - 1u - (qb + refl_rank)) * 2u;
      rec[0] = ra;
      rec[1] = rb;
    }
  }
  if (SCAN && pend_asked) flush_ring();  // (reads the ring before this tile's records go in)
  if (SCAN && def_mask) {
    // 32-byte record: everything the resolve kernel needs to pick the chain up at op def_t
    if (!park) q_pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)q_pos);
    if (deferred && !refl) {
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(def_mask >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)def_mask, 0u));
      uint4 ra, rb;
      ra.x = gr;
      ra.y = (uint32_t)s | ((uint32_t)e << 16);
      ra.z = rec_win;
      ra.w = rec_rows;
      rb.x = (fm >> 8) | (meta & 0xff000000u);
      rb.y = (fm & 0xffu) | ((meta & 0xffu) << 8) | ((rec_rmax & 0xffu) << 16) | ((qc << 8) & 0xff000000u);
      rb.z = capo;
      rb.w = (qc >> 24) | ((qc & 0xffffu) << 8) | ((meta << 8) & 0xff000000u);
      uint4 *rec = park ? ring + (pend_count + rank) * 2u : a.defer[mate] + (size_t)(q_pos + rank) * 2u;
      rec[0] = ra;
      rec[1] = rb;
    }
    if (park) pend_count += (uint32_t)__popcll(def_mask);
  }
  next_id = same_unit ? tile_id + 1 : SCAN ? unit_start(a.static_units + my_counter + n_counters * fetched) : fetched;
  next_id = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_id);  // lane 0 asked
  __syncthreads();  // every lane is done with the tile buffer before the next tile lands in it
  CS_T_MARK(pt, 6);
  }  // persistent tile / batch loop
  if (SCAN && pend_count) {  // what is still parked when the block runs out of tiles
    if (!pend_asked && wave_lane_fresh() == 0u) pend_q = atomicAdd(&a.defer_count[mate * kTileCounterStride], pend_count);
    flush_ring();
  }
#ifdef CS_PHASE_TIMERS
  // -DCS_PHASE_TIMERS=1: the scan kernel reports, =2: the resolve kernel does
  if ((CS_PHASE_TIMERS == 1) == SCAN) {
    if (lane == 0)
      for (int i = 0; i < 8; ++i) atomicAdd(&sacc[ST_OPS + 16 + i], pt.acc[i] >> 6);  // units of 64 cycles
    if (lane == 0) {  // op slots 13..15 are free in every preset (<= 13 ops per mate)
      atomicAdd(&sacc[ST_OPS + 13], pt.passes);
      atomicAdd(&sacc[ST_OPS + 14], pt.steps);
      atomicAdd(&sacc[ST_OPS + 15], pt.items);
    }
  }
  __syncthreads();
#endif

  // one global atomic per counter per block (the LDS accumulators are 32-bit: a block sees
  // far fewer than 2^32 bases)
  const int tid_end = SCAN ? (int)wave_lane_fresh() : tid;
  if constexpr (POLYA) {  // (a lane's own 32-bit sum, the wave's in 64 bits)
    const unsigned long long w_polya = (unsigned long long)wave_sum(polya_bp & 0xffffu) + ((unsigned long long)wave_sum(polya_bp >> 16) << 16);
    if (tid_end == 0 && w_polya) atomicAdd(&a.stats[kPolyABase + mate], w_polya);
  }
  if (tid_end < kStatWords && sacc[tid_end])
    atomicAdd(&a.stats[(size_t)mate * kStatWords + tid_end], (unsigned long long)sacc[tid_end]);
}

}  // namespace csdev
