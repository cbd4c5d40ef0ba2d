"""The homopolymer (poly-A tail / poly-T head) closed forms restated for the tests, and the ENUMERATED reads that hold
the kernels' forms to them (``trim_kernel.hip.inc``: FILTER_POLY_TAIL / FILTER_POLY_HEAD -- ``poly_maybe``, ``poly_maps``,
``poly_tail_wave``, ``poly_head_wave`` on coded tiles, ``poly_tail<false>`` / ``poly_head<false>`` on raw tiles; DESIGN.md
section 2.4).  The ops are ``NonInternalBackAdapter(X * m)`` and ``NonInternalFrontAdapter(X * m)`` (cutseq/run.py:388-413,
673-716).

The rule (``rule_tail``, ``rule_head``; ``rules_tail`` / ``rules_head`` say the same with numpy over rows): with every
reference base equal, the only candidate cells are those of the last column (tail: rows m .. 1, in that order) or of the
last row (head: columns 1 .. min(n, m), in that order), and cell values follow from counting the foreign bases next to
the anchored end -- tail row i <= n: (cost b_i, score i - 2 b_i, origin n - i); tail row i > n: (cost (i - n) + b_n,
score n - 2 b_n, origin 0); head column j <= m: (cost b_j, score j - 2 b_j, origin j - m).  EVERY row / column is
visited and judged by cutadapt's "update best" predicate; nothing is skipped.  Head columns beyond m are reachable when
the first m bases hold at most k foreign ones: there the closed form makes no claim (``DP``).  Neither the oracle, pyref
nor the product is called.

``shortcut`` is the road the coded tiles take, as the kernel takes it: a verdict from the 32 bases next to the anchored
end (checked at min_overlap and at the threshold's steps), two rounds of 64 stops that leave a bitmap of foreign bases
and one of acceptable stops, and the wave walks over the acceptable stops.  It is a MODEL for the CPU tests: ``DEFECTS``
names ten ways of getting it wrong, and the tests show that the enumerated reads tell every one of them from the rule.

Reads are kept by what matters -- ``Reads.rev[r, q]``: base number q FROM THE ANCHORED END of read r is foreign -- and
turned into letters for either end by ``place``: a tail read is the head read reversed.  Everything is deterministic.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

from cutseq_amd import abi, plan as planmod

DP = "DP"
LEFTMOST, SCORE = abi.CS_SELECT_LEFTMOST, abi.CS_SELECT_SCORE
RULES = (LEFTMOST, SCORE)


# ---- the rule, one read at a time

def better(rule: int, m: int, best, cost: int, score: int, origin: int, length: int) -> bool:
    """cutadapt's Aligner.locate "update best"; best: (origin, cost, score, length) or None."""
    if best is None:
        return True
    b_origin, b_cost, b_score, b_length = best
    if rule == SCORE:
        return score > b_score or (score == b_score and cost < b_cost)
    return (origin <= b_origin + m // 2 and score > b_score) or (length > b_length and score > b_score)


def rule_tail(read: str, base: str, m: int, k: int, thr: Sequence[int], min_overlap: int, rule: int):
    """-> the kept interval (0, stop), or None without a hit.  (k is the budget thr[m]; no row needs it by name.)"""
    n = len(read)
    best = None
    for i in range(m, 0, -1):
        if i <= n:
            b = sum(ch != base for ch in read[n - i:])
            cost, score, origin = b, i - 2 * b, n - i
        else:
            b = sum(ch != base for ch in read)
            cost, score, origin = (i - n) + b, n - 2 * b, 0
        if i >= min_overlap and cost <= thr[i] and better(rule, m, best, cost, score, origin, i):
            best = (origin, cost, score, i)
    return None if best is None else (0, best[0])


def rule_head(read: str, base: str, m: int, k: int, thr: Sequence[int], min_overlap: int, rule: int):
    """-> the kept interval (start, n), None without a hit, or DP where columns beyond m are reachable."""
    n = len(read)
    if n > m and sum(ch != base for ch in read[:m]) <= k:
        return DP
    best, b = None, 0
    for j in range(1, min(n, m) + 1):
        b += read[j - 1] != base
        if j >= min_overlap and b <= thr[j] and better(rule, m, best, b, j - 2 * b, j - m, j):
            best = (j - m, b, j - 2 * b, j)
    return None if best is None else (best[3], n)


# ---- the coded tiles' road, as a model

DEFECTS = (
    "maybe_without_step_checks",   # poly_maybe: only "the budget lasts 32 bases"
    "maybe_at_min_overlap_only",   # poly_maybe: checked at min_overlap, never at the steps
    "one_ballot_round",            # poly_maps: 64 stops, no second round
    "stop_above_min_overlap",      # poly_maps: q > min_overlap in place of >=
    "threshold_of_next_stop",      # poly_maps: thr[q + 1] in place of thr[q]
    "head_replaces_on_equal_score",
    "head_without_last_column",
    "tail_without_rows_longer_than_the_read",
    "tail_without_the_whole_stretch",
    "tail_stops_ascending",
)
HEAD_DEFECTS = DEFECTS[:5] + DEFECTS[5:7]
TAIL_DEFECTS = DEFECTS[:5] + DEFECTS[7:]
M64 = (1 << 64) - 1


def _bits_up(x: int):
    while x:
        low = x & -x
        yield low.bit_length() - 1
        x ^= low


def shortcut_bits(fg: int, n: int, m: int, k: int, thr: Sequence[int], min_overlap: int, rule: int, head: bool,
                  defect: Optional[str] = None):
    """``shortcut`` on a bitmap: bit q of ``fg`` is set when base number q from the anchored end is foreign."""
    assert defect is None or defect in DEFECTS
    if n == 0:  # (the op loop leaves empty intervals alone)
        return None
    lim = min(n, m)
    fl = fg & ((1 << lim) - 1)
    # poly_maybe: the 32 bases next to the anchored end
    maybe = (fl & 0xFFFFFFFF).bit_count() <= k
    if defect != "maybe_without_step_checks":
        steps = [i for i in range(1, min(m, 64) + 1) if thr[i] != thr[i - 1]]  # (the kernel keeps 64 step bits)
        p = min_overlap
        while p <= 32:
            if p <= lim and (fl & ((1 << p) - 1)).bit_count() <= thr[p]:
                maybe = True
            if defect == "maybe_at_min_overlap_only":
                break
            later = [i for i in steps if i > p]
            if not later:
                break
            p = later[0]
    if not maybe:
        return None
    # poly_maps: two ballots of 64
    total = fm = am = 0
    for half in range(1 if defect == "one_ballot_round" else 2):
        if half * 64 >= lim or total > k:
            break
        bits = (fl >> (64 * half)) & M64
        rank, acc = total, 0
        for lane in _bits_up(bits):
            q = half * 64 + lane
            far = q > min_overlap if defect == "stop_above_min_overlap" else q >= min_overlap
            if far and rank <= (thr[q + 1] if defect == "threshold_of_next_stop" else thr[q]):
                acc |= 1 << lane
            rank += 1
        fm |= bits << (64 * half)
        am |= acc << (64 * half)
        total += bits.bit_count()
    below = lambda i: (fm & ((1 << i) - 1)).bit_count()
    if head:  # poly_head_wave
        best = None  # (score, column)
        for j in _bits_up(am):
            score = j - 2 * below(j)
            if best is None or score > best[0] or (defect == "head_replaces_on_equal_score" and score == best[0]):
                best = (score, j)
        alive = total <= k
        if defect != "head_without_last_column" and alive and lim >= min_overlap and total <= thr[lim]:
            score = lim - 2 * total
            if best is None or score > best[0] or (defect == "head_replaces_on_equal_score" and score == best[0]):
                best = (score, lim)
        if alive and n > m:
            return DP
        return None if best is None else (best[1], n)
    # poly_tail_wave
    best = None

    def consider(i, cost, score, origin):
        nonlocal best
        if i >= min_overlap and cost <= thr[i] and better(rule, m, best, cost, score, origin, i):
            best = (origin, cost, score, i)

    b = total
    if b <= k:
        if n < m and defect != "tail_without_rows_longer_than_the_read":
            for i in range(min(m, n + k - b), n, -1):
                consider(i, (i - n) + b, n - 2 * b, 0)
        if defect != "tail_without_the_whole_stretch":
            consider(lim, b, lim - 2 * b, n - lim)
    stops = list(_bits_up(am))
    for i in (stops if defect == "tail_stops_ascending" else reversed(stops)):
        bi = below(i)
        consider(i, bi, i - 2 * bi, n - i)
    return None if best is None else (0, best[0])


def shortcut(read: str, base: str, m: int, k: int, thr: Sequence[int], min_overlap: int, rule: int, head: bool,
             defect: Optional[str] = None):
    """The coded path on one read (as the aligner sees it) -> what ``rule_head`` / ``rule_tail`` return."""
    seen = read if head else read[::-1]
    fg = sum(1 << q for q, ch in enumerate(seen) if ch != base)
    return shortcut_bits(fg, len(read), m, k, thr, min_overlap, rule, head, defect)


# ---- the universe

class Reads(NamedTuple):
    rev: np.ndarray      # [n, width] bool: base number q from the anchored end is foreign
    lens: np.ndarray     # [n] int64
    body_at: np.ndarray  # [n] int64: where the body starts (counted from the anchored end)
    body: np.ndarray     # [n] int64: 0 none, 1 one foreign base, 2 twenty foreign bases, 3 forty more of the base


DISTANCES = (tuple(range(10)) + (14, 15, 16, 17, 23, 24, 25, 30, 31, 32, 33, 34, 47, 48, 55, 56, 57, 62, 63, 64, 65, 66,
                                 90, 91, 92, 98, 99, 100, 101, 102, 119, 120, 121, 126, 127, 128, 129, 130))
assert len(DISTANCES) == 48
BODIES = ((0, False), (1, True), (20, True), (40, False))  # (length, foreign)
PERIODS = (3, 4, 5, 6, 7, 8, 9, 13)
RUNS = (7, 14, 20, 27, 31, 32, 33, 40, 47, 63, 64, 65, 67, 99, 100, 101, 107, 127, 128, 129, 140)
WIDTH = 180  # the longest read: 140 + 40 (periodic), 130 + 9 + 40 (windows)


def _finish(rev, at, body) -> Reads:
    rows = np.arange(len(at))
    lens = at.copy()
    for kind, (length, foreign) in enumerate(BODIES):
        mine = body == kind
        lens[mine] += length
        if foreign:
            for t in range(length):
                rev[rows[mine], at[mine] + t] = True
    assert int(lens.max(initial=0)) <= rev.shape[1]
    return Reads(rev, lens, at, body)


def windows(max_len: int) -> Reads:
    """Every string over {base, foreign} of length 0..max_len, ``d`` pure bases from the anchored end for every d of
    DISTANCES, behind every body of BODIES: (2^(max_len + 1) - 1) * 48 * 4 reads."""
    wl = np.concatenate([np.full(1 << L, L, dtype=np.int64) for L in range(max_len + 1)])
    wv = np.concatenate([np.arange(1 << L, dtype=np.int64) for L in range(max_len + 1)])
    nw, nd, nb = len(wl), len(DISTANCES), len(BODIES)
    n = nb * nd * nw
    body = np.repeat(np.arange(nb), nd * nw)
    d = np.tile(np.repeat(np.array(DISTANCES, dtype=np.int64), nw), nb)
    wl, wv = np.tile(wl, nb * nd), np.tile(wv, nb * nd)
    rev = np.zeros((n, WIDTH), dtype=bool)
    rows = np.arange(n)
    for t in range(max_len):
        mine = wl > t
        rev[rows[mine], d[mine] + t] = ((wv[mine] >> t) & 1).astype(bool)
    return _finish(rev, d + wl, body)


def periodic() -> Reads:
    """A foreign base every p positions at every phase, in runs of every length of RUNS, behind every body: 4 620 reads
    that hold the budget at and around rate * length."""
    spec = [(b, p, ph, r) for b in range(len(BODIES)) for p in PERIODS for ph in range(p) for r in RUNS]
    rev = np.zeros((len(spec), WIDTH), dtype=bool)
    q = np.arange(WIDTH)
    for row, (_b, p, ph, r) in enumerate(spec):
        rev[row] = (q % p == ph) & (q < r)
    return _finish(rev, np.array([s[3] for s in spec], dtype=np.int64), np.array([s[0] for s in spec], dtype=np.int64))


def join(*parts: Reads) -> Reads:
    return Reads(*[np.concatenate([p[i] for p in parts]) for i in range(4)])


def edges() -> Reads:
    """The subset for the expensive configurations: periodic() + windows(4), 10 572 reads."""
    return join(periodic(), windows(4))


def full() -> Reads:
    return join(windows(9), periodic())


def bitmaps(reads: Reads):
    """``Reads.rev`` as Python ints for ``shortcut_bits``."""
    packed = np.packbits(reads.rev, axis=1, bitorder="little")
    return [int.from_bytes(row.tobytes(), "little") for row in packed]


def letters(reads: Reads, base: str, foreign: str, lower_every: int = 0, odd_body: bool = False) -> np.ndarray:
    """The reads' letters, counted from the anchored end -> [n, width] uint8 (0 behind the read).  ``lower_every``: every
    such base of the run is the base in lower case; ``odd_body``: the bodies of twenty hold an ``R`` and a ``.``."""
    q = np.arange(reads.rev.shape[1])
    out = np.where(reads.rev, ord(foreign), ord(base)).astype(np.uint8)
    if lower_every:
        out[~reads.rev & (q[None, :] % lower_every == 1)] = ord(base.lower())
    if odd_body:
        rows = np.flatnonzero(reads.body == 2)
        out[rows, reads.body_at[rows] + 3] = ord("R")
        out[rows, reads.body_at[rows] + 7] = ord(".")
    out[q[None, :] >= reads.lens[:, None]] = 0
    return out


def place(lett: np.ndarray, lens: np.ndarray, head: bool, pad: int = 0, pad_letter: str = "G", stride: Optional[int] = None):
    """Letters counted from the anchored end -> (seq [n, stride] uint8, lens [n] uint16) of the reads themselves: a head
    read as it stands, a tail read reversed; ``pad`` more bases at the anchored end for a CutOp to remove."""
    n, w = lett.shape
    stride = (w + pad + 3) // 4 * 4 if stride is None else stride
    rows = np.zeros((n, stride), dtype=np.uint8)
    rows[:, :pad] = ord(pad_letter)
    rows[:, pad:pad + w] = lett
    total = lens.astype(np.int64) + pad
    if not head:
        at = total[:, None] - 1 - np.arange(stride)[None, :]
        rows = np.where(at >= 0, np.take_along_axis(rows, np.maximum(at, 0), axis=1), 0).astype(np.uint8)
    return np.ascontiguousarray(rows), total.astype(np.uint16)


def strings(seq: np.ndarray, lens: np.ndarray):
    return [seq[i, :lens[i]].tobytes().decode() for i in range(len(lens))]


# ---- the rule over rows

def _counts(reads: Reads) -> np.ndarray:
    """[n, width + 1]: foreign bases among the first i from the anchored end."""
    out = np.zeros((reads.rev.shape[0], reads.rev.shape[1] + 1), dtype=np.int16)
    np.cumsum(reads.rev, axis=1, dtype=np.int16, out=out[:, 1:])
    return out


class Best:
    def __init__(self, n: int):
        self.have = np.zeros(n, dtype=bool)
        self.origin, self.cost, self.score, self.length = (np.zeros(n, dtype=np.int64) for _ in range(4))

    def offer(self, rule, m, ok, cost, score, origin, length):
        if rule == SCORE:
            wins = (score > self.score) | ((score == self.score) & (cost < self.cost))
        else:
            wins = ((origin <= self.origin + m // 2) & (score > self.score)) | ((length > self.length) & (score > self.score))
        take = ok & (~self.have | wins)
        self.have |= take
        for mine, new in ((self.origin, origin), (self.cost, cost), (self.score, score), (self.length, length)):
            mine[take] = np.broadcast_to(new, take.shape)[take]


def rules_tail(reads: Reads, m: int, k: int, thr: Sequence[int], min_overlap: int, rule: int):
    """``rule_tail`` on every read -> (hit [n] bool, stop [n]: where the kept interval ends)."""
    n, counts = reads.lens, _counts(reads)
    whole = counts[np.arange(len(n)), n].astype(np.int64)
    best = Best(len(n))
    w = reads.rev.shape[1]
    for i in range(m, 0, -1):
        inside = i <= n
        b = counts[:, min(i, w)].astype(np.int64)
        cost = np.where(inside, b, (i - n) + whole)
        score = np.where(inside, i - 2 * b, n - 2 * whole)
        origin = np.where(inside, n - i, 0)
        best.offer(rule, m, (cost <= thr[i]) & (i >= min_overlap), cost, score, origin, i)
    return best.have, np.where(best.have, best.origin, n)


def rules_head(reads: Reads, m: int, k: int, thr: Sequence[int], min_overlap: int, rule: int):
    """``rule_head`` on every read -> (hit [n] bool, start [n], dp [n] bool: no claim)."""
    n, counts = reads.lens, _counts(reads)
    w = reads.rev.shape[1]
    dp = (n > m) & (counts[:, min(m, w)] <= k)
    best = Best(len(n))
    for j in range(1, min(m, w) + 1):
        b = counts[:, j].astype(np.int64)
        best.offer(rule, m, (j <= n) & (b <= thr[j]) & (j >= min_overlap), b, j - 2 * b, j - m, j)
    hit = best.have & ~dp
    return hit, np.where(hit, best.length, 0), dp


# ---- the settings

PARAMS = ((100, .15, 3),  # the reference's own (cutseq/run.py:389-390, 674-675)
          (100, .3, 1), (100, .4, 3), (128, .15, 3), (127, .1, 64), (65, .1, 33), (64, .3, 10), (63, .2, 1), (33, .15, 1),
          (32, .25, 32), (20, 0.0, 3), (8, .5, 5), (2, .5, 1), (1, 0.0, 1))
MODEL_PARAMS = ((100, .15, 3), (33, .15, 1), (20, 0.0, 3), (64, .3, 10), (65, .1, 33), (8, .5, 5))
TAIL_BASE, HEAD_BASE = "A", "T"


def tie_of(index: int) -> int:
    return (abi.CS_TIE_INSERTION, abi.CS_TIE_DELETION)[index % 2]


def foreign_of(base: str, index: int) -> str:
    """The foreign letter of parameter set ``index``: the three other bases and N in turn."""
    return ([b for b in "ACGT" if b != base] + ["N"])[index % 4]


def poly_op(base: str, m: int, rate: float, min_overlap: int, head: bool) -> planmod.AdapterOp:
    if head:
        return planmod.AdapterOp("NonInternalFrontAdapter", base * m, rate, min_overlap, abi.CS_WHERE_FRONT_NOT_INTERNAL,
                                 abi.CS_REMOVE_BEFORE, match_flag=abi.CS_F_POLY)
    return planmod.AdapterOp("NonInternalBackAdapter", base * m, rate, min_overlap, abi.CS_WHERE_BACK_NOT_INTERNAL,
                             abi.CS_REMOVE_AFTER, match_flag=abi.CS_F_POLY)


def cuts_of(index: int):
    """The cuts c (bases a CutOp removes at the op's own end, in front of it) that parameter set ``index`` runs behind:
    the reference's own set meets all eight, every other set two."""
    return tuple(range(8)) if index == 0 else (index % 8, (index + 4) % 8)


# Reads a kernel got wrong, kept by name: (name, read as the tail form sees it, (m, rate, min_overlap), rule, head).
NAMED: tuple = ()
