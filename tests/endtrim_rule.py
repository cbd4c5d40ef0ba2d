"""The two read-end modifiers behind the adapter work, restated for the tests: cutadapt's quality trimming with a 5'
cutoff (``qualtrim.pyx quality_trim_index(qualities, cutoff_front, cutoff_back, base)``) and its ``NEndTrimmer``
(``--trim-n``), as ``include/cutseq_hip.h`` states them for CS_OP_QTRIM / CS_OP_NTRIM.  Plain Python over one read and
numpy int64 over rows: neither can overflow, neither calls the oracle, pyref or the product.  The 3' walk is the one of
tests/qtrim_rule.py (``stop`` / ``stops``), imported, not restated.

QualityTrimmer(cutoff_front=F, cutoff_back=B, base) on an interval of n bases with qualities q[0..n):
  back   from n - 1 down: sum += B - (q[i] - base); stop at the first negative sum; ``stop`` = the position of the first
         strict maximum, n when no sum is positive
  front  from 0 up: sum += F - (q[i] - base); stop at the first negative sum; ``start`` = one behind the position of the
         first strict maximum, 0 when no sum is positive.  The walk runs over ALL of q[0..n), not over q[0..stop)
  start >= stop: nothing is left (reported as the empty interval at the interval's start); else [start, stop) is left.
NEndTrimmer() on the bases of an interval: the leading and the trailing run of the byte ``N`` (0x4E, upper case only:
the patterns are ``^N+`` and ``N+$`` without IGNORECASE) go; all ``N``: nothing is left.

``apply_tail`` layers both over intervals that something else decided (the C oracle knows neither): that is how the GPU
tests get their expected records for chains that end ``..., QTrimOp(F, B)[, NTrimOp()]``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

import qtrim_rule as R

F_QTRIMMED = R.F_QTRIMMED
F_TOO_SHORT = 0x20  # CS_F_TOO_SHORT (include/cutseq_hip.h)
N = 0x4E
CHUNK = R.CHUNK


# ---- the rules, one read

def start(qual: bytes, cutoff: int, base: int = 33) -> int:
    s = best = 0
    at = 0
    for i, b in enumerate(qual):
        s += cutoff - (b - base)
        if s < 0:
            break
        if s > best:
            best, at = s, i + 1
    return at


def qtrim(qual: bytes, front: int, back: int, base: int = 33) -> tuple:
    """-> (start, stop); (0, 0) for every empty result."""
    a, b = start(qual, front, base), R.stop(qual, back, base)
    return (0, 0) if a >= b else (a, b)


def ntrim(seq: bytes) -> tuple:
    """-> (start, stop); (0, 0) when nothing is left."""
    a = 0
    while a < len(seq) and seq[a] == N:
        a += 1
    if a == len(seq):
        return 0, 0
    b = len(seq)
    while seq[b - 1] == N:
        b -= 1
    return a, b


# ---- the rules over rows

class Fronts(NamedTuple):
    start: np.ndarray  # relative to the interval's start, like ``start``
    brk: np.ndarray    # position (in the row) of the first negative sum, -1: the walk reaches the interval's end
    last: np.ndarray   # the last position (in the row) the walk looks at, -1: an empty interval


def fronts(qual_rows: np.ndarray, begin, end, cutoff: int, base: int = 33) -> Fronts:
    """The front walk on the interval [begin, end) of every row of ``qual_rows`` [n, stride]."""
    q = np.asarray(qual_rows)
    n, w = q.shape
    begin = np.broadcast_to(np.asarray(begin, dtype=np.int64), (n,))
    end = np.broadcast_to(np.asarray(end, dtype=np.int64), (n,))
    cols = np.arange(w, dtype=np.int64)
    out = Fronts(np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64))
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(lo + CHUNK, n))
        s, e = begin[sl, None], end[sl, None]
        inside = (cols >= s) & (cols < e)
        term = np.where(inside, int(cutoff) + int(base) - q[sl].astype(np.int64), 0)
        run = np.cumsum(term, axis=1)  # run[i]: the sum once position i is added
        neg = inside & (run < 0)
        brk = np.where(neg.any(axis=1), np.argmax(neg, axis=1), -1)
        seen = inside & ((cols < brk[:, None]) | (brk[:, None] < 0))
        top = np.where(seen, run, 0).max(axis=1, initial=0)
        hit = seen & (run == top[:, None]) & (top[:, None] > 0)  # first strict maximum: the lowest such position
        pos = np.argmax(hit, axis=1)
        out.start[sl] = np.where(top > 0, pos + 1 - begin[sl], 0)
        out.brk[sl] = brk
        out.last[sl] = np.where(end[sl] > begin[sl], np.where(brk >= 0, brk, end[sl] - 1), -1)
    return out


def qtrims(qual_rows: np.ndarray, begin, end, front: int, back: int, base: int = 33):
    """-> (start [n], stop [n]) as positions in the rows; an empty result is (begin, begin)."""
    n = len(qual_rows)
    begin = np.broadcast_to(np.asarray(begin, dtype=np.int64), (n,))
    end = np.broadcast_to(np.asarray(end, dtype=np.int64), (n,))
    a = fronts(qual_rows, begin, end, front, base).start
    b = R.stops(qual_rows, begin, end, back, base)
    empty = a >= b
    return begin + np.where(empty, 0, a), begin + np.where(empty, 0, b)


def ntrims(seq_rows: np.ndarray, begin, end):
    """-> (start [n], stop [n]) as positions in the rows; nothing left: (begin, begin)."""
    seq = np.asarray(seq_rows)
    n, w = seq.shape
    begin = np.broadcast_to(np.asarray(begin, dtype=np.int64), (n,))
    end = np.broadcast_to(np.asarray(end, dtype=np.int64), (n,))
    cols = np.arange(w, dtype=np.int64)
    a, b = np.empty(n, np.int64), np.empty(n, np.int64)
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(lo + CHUNK, n))
        keep = (cols >= begin[sl, None]) & (cols < end[sl, None]) & (seq[sl] != N)
        some = keep.any(axis=1)
        a[sl] = np.where(some, np.argmax(keep, axis=1), begin[sl])
        b[sl] = np.where(some, w - np.argmax(keep[:, ::-1], axis=1), begin[sl])
    return a, b


# ---- layered over intervals that something else decided

class Tail(NamedTuple):
    """The end of a chain: ``QualityTrimmer(front, back, base)`` (``back`` None: no such op), then ``NEndTrimmer()``
    where ``trim_n``."""
    front: int = 0
    back: Optional[int] = None
    base: int = 33
    trim_n: bool = False


class Ends(NamedTuple):
    start: np.ndarray
    stop: np.ndarray
    flags: np.ndarray
    cut: int  # what the quality trimmer took (cs_stats.qualtrim_bp gains it)


def apply_tail(seq_rows, qual_rows, begin, end, flags, tail: Tail, min_length: int = 0) -> Ends:
    """The chain's tail on the intervals [begin, end) with the flags the ops in front of it left (CS_F_TOO_SHORT in
    them is dropped and decided again, on the final interval)."""
    n = len(seq_rows)
    begin = np.broadcast_to(np.asarray(begin, dtype=np.int64), (n,)).copy()
    end = np.broadcast_to(np.asarray(end, dtype=np.int64), (n,)).copy()
    end = np.maximum(end, begin)
    flags = np.broadcast_to(np.asarray(flags, dtype=np.int64), (n,)) & ~F_TOO_SHORT
    cut = 0
    if tail.back is not None:
        a, b = qtrims(qual_rows, begin, end, tail.front, tail.back, tail.base)
        took = (end - begin) - (b - a)
        flags = flags | np.where(took > 0, F_QTRIMMED, 0)
        cut = int(took.sum())
        begin, end = a, b
    if tail.trim_n:
        begin, end = ntrims(seq_rows, begin, end)
    flags = flags | np.where(end - begin < min_length, F_TOO_SHORT, 0)
    return Ends(begin, end, flags, cut)


def split_tail(ops: Sequence, qtrim_type, ntrim_type):
    """A chain's ops -> (the ops in front of its trailing QTrimOp / NTrimOp, Tail)."""
    ops = list(ops)
    trim_n = bool(ops) and isinstance(ops[-1], ntrim_type)
    if trim_n:
        ops.pop()
    tail = Tail(trim_n=trim_n)
    if ops and isinstance(ops[-1], qtrim_type):
        q = ops.pop()
        tail = Tail(q.cutoff_front, q.cutoff_back, q.base, trim_n)
    return ops, tail


# ---- inputs: the mirror image of a qtrim_rule family (what was built for the 3' walk meets the 5' walk)

def mirror(rows: R.Rows) -> R.Rows:
    """Every row's string behind its f pad bytes, reversed (qualities and bases)."""
    lens = rows.lens.astype(np.int64)
    n, w = rows.qual.shape
    cols = np.arange(w, dtype=np.int64)[None, :]
    body = (cols >= rows.f) & (cols < lens[:, None])
    src = np.where(body, rows.f + lens[:, None] - 1 - cols, cols)
    idx = np.arange(n)[:, None]
    return R.Rows(np.ascontiguousarray(rows.seq[idx, src]), np.ascontiguousarray(rows.qual[idx, src]), rows.lens, rows.f)


def both(rows: R.Rows) -> R.Rows:
    """A family and its mirror image, one behind the other."""
    m = mirror(rows)
    return R.Rows(np.concatenate([rows.seq, m.seq]), np.concatenate([rows.qual, m.qual]),
                  np.concatenate([rows.lens, m.lens]), rows.f)
