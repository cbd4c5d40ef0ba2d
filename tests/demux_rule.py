"""Demultiplexing (``CS_OP_DEMUX``) held to its parity definition on ENUMERATED reads: the op must
equal B independent ``--ensure-inline-barcode`` runs of the oracle, merged by a fixed rule -- an exact copy of a barcode
wins, else the lowest index claims the read, more than one claimant sets ``CS_F_AMBIGUOUS``.

What is here (no GPU code; shared by tests/test_demux_cpu.py and tests/test_gpu_demux_enumerated.py):

  universes   every string of length 0 .. m + k over a small alphabet (``universe``; U1, U2, U3 below)
  barcodes    crowded sets, written out: a centre at a HIGH index behind its own neighbours (one substitution at the first
              and at the last base, two substitutions, the centre shifted by one base either way), a homopolymer and a
              period-two barcode; a spread set (pairwise edit distance >= 3); a set of one
  the rule    ``oracle_runs`` + ``merge``: B oracle runs of the same chain with the barcode's own PrefixAdapter /
              SuffixAdapter op in the demultiplexer's place, merged with numpy
  the table   ``table_index``: where a read's entry lies, from the header's words (include/cutseq_hip.h,
              cs_plan_set_demux), written without looking at cutseq_amd/demux.py
  the lists   ``alive_plain``: which barcodes a plain edit-distance table (no band, no cap, no pruning) leaves alive
              behind every prefix; ``walk_model``: the library's banded, capped walk restated (the comment above
              ``DemuxWalk`` in cutseq_hip.hip), with the planted ``DEFECTS`` that the CPU tests must tell from it
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

import oracle
from cutseq_amd import abi, plan as planmod

NONE = abi.CS_DEMUX_NONE
FOLD, SENSITIVE = abi.CS_CASE_FOLD, abi.CS_CASE_SENSITIVE
RULES = (abi.CS_SELECT_LEFTMOST, abi.CS_SELECT_SCORE)
TIES = (abi.CS_TIE_INSERTION, abi.CS_TIE_DELETION)
BLOCK = 262_144  # reads per launch: the command line's block size


# ---- universes and barcode sets

class Universe(NamedTuple):
    name: str
    alphabet: str
    m: int
    rate: float
    k: int
    reads: int
    crowded: tuple
    spread: tuple
    single: tuple

    @property
    def span(self) -> int:
        return self.m + self.k

    def sets(self):
        return {"crowded": self.crowded, "spread": self.spread, "single": self.single}


U1 = Universe("U1", "ACTGN", 6, 0.2, 1, 97_656,
              crowded=("CCGTCA", "ACGTCC", "ACTTCA", "CGTCAA", "AACGTC", "ACGTCA", "TTGACG", "AAAAAA", "ACACAC"),
              spread=("ACGTCA", "TTGACG", "GGATTC", "CATAGG", "TCCGAT"),
              single=("ACGTCA",))
U2 = Universe("U2", "ACN", 11, 0.2, 2, 2_391_484,
              crowded=("CCCACAACACC", "ACCACAACACA", "ACCCCAAAACC", "CCACAACACCA", "CACCACAACAC", "ACCACAACACC",
                       "AAAAAAAAAAA", "ACACACACACA"),
              spread=("ACCACAACACC", "CCCCCCAAAAA", "AAAAACCCCCC", "CACACCCACAA"),
              single=("ACCACAACACC",))
U3 = Universe("U3", "AC", 16, 0.25, 4, 2_097_151,
              crowded=("CCCACAACACCCAACA", "ACCACAACACCCAACC", "ACCAAAACACCAAACA", "CCACAACACCCAACAC", "AACCACAACACCCAAC",
                       "ACCACAACACCCAACA", "AAAAAAAAAAAAAAAA", "ACACACACACACACAC"),
              spread=("ACCACAACACCCAACA", "CCCCCCCCAAAAAAAA", "AAAAAAAACCCCCCCC", "CACACCCACAAAACCC"),
              single=("ACCACAACACCCAACA",))
UNIVERSES = {"U1": U1, "U2": U2, "U3": U3}
CENTRE_AT = {"U1": 5, "U2": 5, "U3": 5}  # the crowded sets' centre: every neighbour has a lower index

TG = bytes.maketrans(b"AC", b"TG")  # U2 once more over {T, G, N}: digits 2 and 3 of the table index


def to_tg(codes: Sequence[str]):
    return tuple(c.translate({ord("A"): "T", ord("C"): "G"}) for c in codes)


def edit_distance(a: str, b: str) -> int:
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def universe(alphabet: str, span: int, stride: Optional[int] = None):
    """Every string over ``alphabet`` of length 0 .. span, shortest first, the first base most significant -> (seq
    [n, stride] uint8, padded with ``N``; qual, ``I`` throughout; len [n] uint16)."""
    letters = np.frombuffer(alphabet.encode(), dtype=np.uint8)
    a = len(alphabet)
    stride = max(4, (span + 3) // 4 * 4) if stride is None else stride
    n = sum(a ** L for L in range(span + 1))
    seq = np.full((n, stride), ord("N"), dtype=np.uint8)
    lens = np.empty(n, dtype=np.uint16)
    at = 0
    for L in range(span + 1):
        count = a ** L
        idx = np.arange(count, dtype=np.int64)
        for j in range(L):
            seq[at:at + count, j] = letters[(idx // a ** (L - 1 - j)) % a]
        lens[at:at + count] = L
        at += count
    return seq, np.full_like(seq, ord("I")), lens


def reads_of(u: Universe, tg: bool = False):
    seq, qual, lens = universe(u.alphabet, u.span)
    if tg:
        seq = np.frombuffer(seq.tobytes().translate(TG), dtype=np.uint8).reshape(seq.shape).copy()
    return seq, qual, lens


def with_front(batch, c: int, cycle: bytes = b"ACGTN"):
    """The same reads behind ``c`` bases that cycle through A, C, G, T, N (for a CutOp to remove)."""
    seq, _qual, lens = batch
    stride = (seq.shape[1] + c + 3) // 4 * 4
    out = np.full((len(lens), stride), ord("N"), dtype=np.uint8)
    out[:, :c] = np.frombuffer((cycle * (c // len(cycle) + 1))[:c], dtype=np.uint8)
    out[:, c:c + seq.shape[1]] = seq
    return out, np.full_like(out, ord("I")), (lens + c).astype(np.uint16)


def with_tail(batch, seed: int = 7, most: int = 24, alphabet: bytes = b"ACGTN"):
    """The reads of full length with 1 .. ``most`` further bases behind them, drawn from ``alphabet`` (fixed seed; read
    number i gets i % most + 1 of them)."""
    seq, _qual, lens = batch
    span = int(lens.max())
    rows = seq[lens == span][:, :span]
    rng = np.random.default_rng(seed)
    stride = (span + most + 3) // 4 * 4
    out = np.full((len(rows), stride), ord("N"), dtype=np.uint8)
    out[:, :span] = rows
    more = np.arange(len(rows)) % most + 1
    out[:, span:span + most] = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), (len(rows), most))]
    return out, np.full_like(out, ord("I")), (span + more).astype(np.uint16)


def lower(batch):
    seq, qual, lens = batch
    return np.frombuffer(seq.tobytes().lower(), dtype=np.uint8).reshape(seq.shape).copy(), qual, lens


# ---- the rule: B oracle runs, merged

def chain(op, front=(), behind=(), rule=RULES[0], tie=TIES[0], case_rule=FOLD) -> planmod.TrimPlan:
    return planmod.TrimPlan(r1=planmod.MateChain([*front, op, *behind]), r2=None, has_umi=False, min_length=0,
                            untrimmed_filter=False, select_rule=rule, indel_tie=tie, case_rule=case_rule)


def demux_chain(codes, rate, form: str, **kw) -> planmod.TrimPlan:
    """``form``: ``table`` (look-up table of every prefix), ``ops5`` (the barcodes' own PrefixAdapter ops) or ``ops3``
    (SuffixAdapter ops, the barcodes end the read)."""
    op = planmod.DemuxOp(list(codes), rate, abi.CS_F_INLINE, required=False, by_ops=form != "table", at_end=form == "ops3")
    assert op.tabulated == (form == "table")
    return chain(op, **kw)


def oracle_runs(codes, rate, batch, at_end=False, threads=1, **kw):
    """One run per barcode: its own PrefixAdapter (``at_end``: SuffixAdapter) op where the demultiplexer stands."""
    make = planmod.suffix if at_end else planmod.prefix
    out = []
    for code in codes:
        tp = chain(make(code, rate, abi.CS_F_INLINE), **kw)
        a1, n1, _a2, _n2 = tp.pack()
        out.append(oracle.trim_mate(a1, n1, tp.params(), *batch, threads=threads)[0])
    return out


class Expected(NamedTuple):
    bc: np.ndarray        # [n] uint8: barcode index or CS_DEMUX_NONE
    res: np.ndarray       # [n] RESULT_DTYPE
    assigned: int         # op_matched of the demultiplexer's slot
    matched: np.ndarray   # [B, n] bool: the runs that matched
    exact: np.ndarray     # [B, n] bool: ... with an exact copy of the barcode at the anchored end


def merge(runs, codes, batch, at_end=False, case_rule=FOLD, front: int = 0) -> Expected:
    """The merge rule.  ``front``: bases a CutOp removed in front of the op (the interval starts there)."""
    seq, _qual, lens = batch
    m, n = len(codes[0]), len(lens)
    L = lens.astype(np.int64)
    s0 = np.minimum(front, L)
    letters = seq if case_rule == SENSITIVE else np.frombuffer(seq.tobytes().upper(), dtype=np.uint8).reshape(seq.shape)
    matched = np.stack([(r["flags"] & abi.CS_F_INLINE) != 0 for r in runs])
    at = (L - m if at_end else s0)[:, None] + np.arange(m)[None, :]
    own = np.take_along_axis(letters, np.clip(at, 0, seq.shape[1] - 1), axis=1)
    exact = np.zeros_like(matched)
    for b, code in enumerate(codes):
        cut_m = (runs[b]["stop"] == L - m) if at_end else (runs[b]["start"] == s0 + m)
        same = (own == np.frombuffer(code.encode(), dtype=np.uint8)[None, :]).all(axis=1) & (L - s0 >= m)
        exact[b] = matched[b] & cut_m & same
    assert int(exact.sum(axis=0).max(initial=0)) <= 1
    bc = np.where(exact.any(axis=0), exact.argmax(axis=0), np.where(matched.any(axis=0), matched.argmax(axis=0), NONE))
    pick = np.where(bc == NONE, 0, bc)
    res = np.stack(runs)[pick, np.arange(n)]
    res["flags"] |= np.where(matched.sum(axis=0) > 1, abi.CS_F_AMBIGUOUS, 0).astype(np.uint8)
    return Expected(bc.astype(np.uint8), res, int((bc != NONE).sum()), matched, exact)


def expect(codes, rate, batch, at_end=False, case_rule=FOLD, front_bases: int = 0, threads=1, **kw) -> Expected:
    front = (planmod.CutOp(front_bases),) if front_bases else ()
    runs = oracle_runs(codes, rate, batch, at_end, threads, front=front + tuple(kw.pop("front", ())), case_rule=case_rule, **kw)
    return merge(runs, codes, batch, at_end, case_rule, front_bases)


# ---- the table index, as the header documents it

def table_index(seq, lens, span: int, start: int = 0, at_end: bool = False, fold: bool = True) -> np.ndarray:
    """cs_plan_set_demux: first the entry of the empty prefix, then the 5 prefixes of length 1, ... up to length ``span``,
    each block indexed by sum(digit[t] * 5^t) with digit = 0, 1, 2, 3 for A, C, T, G and 4 for anything else.  A read
    with fewer than ``span`` bases has the slot of its own length.  ``at_end``: the read's last bases, last base first
    (the candidate lists of a 3' op)."""
    digit_of = np.full(256, 4, dtype=np.int64)
    for d, ch in enumerate("ACTG"):
        digit_of[ord(ch)] = d
        if fold:
            digit_of[ord(ch.lower())] = d
    L = lens.astype(np.int64)
    s = np.minimum(start, L)
    take = np.minimum(L - s, span)
    idx = np.zeros(len(L), dtype=np.int64)
    for t in range(span):
        col = (L - 1 - t) if at_end else (s + t)
        d = digit_of[seq[np.arange(len(L)), np.clip(col, 0, seq.shape[1] - 1)]]
        idx += np.where(t < take, d * 5 ** t, 0)
    return (5 ** take - 1) // 4 + idx


# ---- the candidate table of a plan (cs_plan_demux_view)

class Lists(NamedTuple):
    depth: int
    first: np.ndarray  # uint32 [slots]: offset into pool << 8 | candidates
    pool: np.ndarray   # uint8

    def entries(self):
        """-> (slot, position in pool) of every list entry, slot by slot in list order."""
        cnt = (self.first & 0xFF).astype(np.int64)
        off = (self.first >> 8).astype(np.int64)
        slot = np.repeat(np.arange(len(cnt)), cnt)
        return slot, np.arange(len(slot)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(off, cnt)

    def check_shape(self, n_codes: int) -> None:
        """Offsets and counts inside ``pool``, indices below B, every list strictly ascending -- the order the device
        tries the candidates in: "the lowest index claims the read" holds only then."""
        assert len(self.first) == slots_of(self.depth)
        cnt = (self.first & 0xFF).astype(np.int64)
        off = (self.first >> 8).astype(np.int64)
        assert int((off + cnt)[cnt > 0].max(initial=0)) <= len(self.pool)
        assert not self.first[cnt == 0].any()
        slot, pos = self.entries()
        ids = self.pool[pos].astype(np.int64)
        assert int(ids.max(initial=0)) < n_codes
        inside = slot[1:] == slot[:-1]
        assert np.all(ids[1:][inside] > ids[:-1][inside])

    def member(self, n_codes: int) -> np.ndarray:
        """[B, slots] bool: barcode b is in the list of the slot."""
        slot, pos = self.entries()
        out = np.zeros((n_codes, len(self.first)), dtype=bool)
        out[self.pool[pos], slot] = True
        return out


def library_lists(codes, rate, at_end: bool = False) -> Lists:
    """The host walk of the library on these barcodes (needs no GPU: a plan is host data)."""
    from cutseq_amd import capi
    L = capi.load()
    op = planmod.DemuxOp(list(codes), rate, abi.CS_F_INLINE, required=False, by_ops=True, at_end=at_end)
    tp = chain(op)
    a1, n1, _a2, _n2 = tp.pack()
    params = tp.params()
    h = C.c_void_p()
    capi.check(L.cs_plan_create(C.cast(a1, C.c_void_p), n1, None, 0, C.byref(params), C.byref(h)))
    try:
        ops = planmod.pack_ops(op.barcode_ops(), limit=255)
        capi.check(L.cs_plan_set_demux_ops(h, 1, 0, C.cast(ops, C.c_void_p), len(codes)))
        depth, n_first, n_pool = C.c_int(), C.c_size_t(), C.c_size_t()
        first, pool = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        capi.check(L.cs_plan_demux_view(h, 1, 0, C.byref(depth), C.byref(first), C.byref(n_first), C.byref(pool), C.byref(n_pool)))
        f = np.ctypeslib.as_array(first, shape=(n_first.value,)).copy()
        p = np.ctypeslib.as_array(pool, shape=(n_pool.value,)).copy() if n_pool.value else np.zeros(0, dtype=np.uint8)
    finally:
        L.cs_plan_destroy(h)
    return Lists(int(depth.value), f, p)


def slots_of(depth: int) -> int:
    return (5 ** (depth + 1) - 1) // 4


def alive_plain(codes, k: int, depth: int, at_end: bool = False, prune: bool = False) -> np.ndarray:
    """[B, slots] bool, from the full edit-distance table of barcode against prefix (anchored at both starts; every row,
    no band, no cap): a barcode can still match behind a prefix when some cell of the prefix's last column is <= k, or
    when the last row was <= k at this or an earlier column.  Slots in the table's order, level by level: a prefix of L
    bases with last digit c sits at (its first L - 1 bases' index) + c * 5^(L-1) of block L.  ``prune``: prefixes behind
    which the barcode is dead are not extended (row 0 grows and every other cell is one of three neighbours plus
    something: a column's minimum never falls) -- the same table in a fraction of the time, shown equal on U1."""
    out = np.zeros((len(codes), slots_of(depth)), dtype=bool)
    for b, code in enumerate(codes):
        digits = ["ACTG".index(ch) for ch in (code[::-1] if at_end else code)]
        m = len(digits)
        col = np.arange(m + 1, dtype=np.int16)[None, :]  # the empty prefix
        done = np.zeros(1, dtype=bool)
        idx = np.zeros(1, dtype=np.int64)
        base = 0
        out[b, 0] = True
        for L in range(1, depth + 1):
            base += 5 ** (L - 1)
            cols, dones, idxs = [], [], []
            for c in range(5):
                new = np.empty_like(col)
                new[:, 0] = L
                for i in range(1, m + 1):
                    new[:, i] = np.minimum(np.minimum(col[:, i - 1] + (0 if digits[i - 1] == c else 1), col[:, i] + 1), new[:, i - 1] + 1)
                cols.append(new)
                dones.append(done | (new[:, m] <= k))
                idxs.append(idx + c * 5 ** (L - 1))
            col, done, idx = np.concatenate(cols), np.concatenate(dones), np.concatenate(idxs)
            alive = done | (col.min(axis=1) <= k)
            out[b, base + idx[alive]] = True
            if prune:
                col, done, idx = col[alive], done[alive], idx[alive]
    return out


# ---- the library's walk, restated

DEFECTS = ("band_k_minus_1", "cap_at_k", "done_forgotten", "row0_not_counted_up")


def walk_model(codes, k: int, depth: int, at_end: bool = False, defect: Optional[str] = None) -> np.ndarray:
    """The comment above ``DemuxWalk``: depth-first over the prefixes, one column per barcode still alive; only the rows
    within k of the diagonal are computed, the others hold the cap; costs are clamped at the cap k + 1 -- nothing at or
    above it is told apart, a cell counts while it is BELOW the cap; a barcode whose last row got there is ``done``: a
    candidate whatever follows.  -> [B, slots] bool."""
    assert defect is None or defect in DEFECTS
    m = len(codes[0])
    digits = [["ACTG".index(ch) for ch in (code[::-1] if at_end else code)] for code in codes]
    cap = k if defect == "cap_at_k" else k + 1
    band = k - 1 if defect == "band_k_minus_1" else k
    block = [slots_of(L - 1) if L else 0 for L in range(depth + 2)]
    out = np.zeros((len(codes), slots_of(depth)), dtype=bool)

    def walk(length, idx, pw, alive):
        for b, _col, _done in alive:
            out[b, block[length] + idx] = True
        if length == depth:
            return
        for c in range(5):
            nxt = []
            for b, col, done in alive:
                if done:
                    nxt.append((b, col, True))
                    continue
                new = [cap] * (m + 1)
                if defect != "row0_not_counted_up":  # (the defect: the row stays what the fill put there)
                    new[0] = min(length + 1, cap)
                for i in range(max(1, length + 1 - band), min(m, length + 1 + band) + 1):
                    new[i] = min(col[i - 1] + (0 if digits[b][i - 1] == c else 1), col[i] + 1, new[i - 1] + 1, cap)
                now_done = new[m] < cap and defect != "done_forgotten"
                if now_done or min(new) < cap:
                    nxt.append((b, new, now_done))
            if nxt:
                walk(length + 1, idx + c * pw, pw * 5, nxt)

    walk(0, 0, 1, [(b, [min(i, cap) for i in range(m + 1)], False) for b in range(len(codes))])
    return out


def required_lists(matched: np.ndarray, slot: np.ndarray, n_slots: int) -> np.ndarray:
    """[B, slots] bool: barcode b matches SOME read whose table slot this is (``matched`` [B, n], ``slot`` [n]) -- what a
    candidate list must hold at least."""
    out = np.zeros((matched.shape[0], n_slots), dtype=bool)
    for b in range(matched.shape[0]):
        out[b, slot[matched[b]]] = True
    return out
