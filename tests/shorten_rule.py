"""cutadapt's ``Shortener(length)`` (``-l`` / ``--length``, ``-L`` for read 2), restated for the tests as
``include/cutseq_hip.h`` states it for CS_OP_SHORTEN.  Plain Python over one read and numpy int64 over rows: neither can
overflow (|-2^31| is an ordinary int64), neither calls the oracle, pyref or the product.

The rule on an interval [s, e) of n = e - s bases:
  length >= 0   ``read[:length]``: e = s + min(n, length); length 0 leaves [s, s)
  length <  0   ``read[length:]``: s = e - min(n, -length): the last |length| bases stay
No flag and no counter: TooShort, the filters and the statistics see the result.

``apply_tail`` / ``split_tail`` are those of tests/nextseq_rule.py for chains that end
``...[, NextSeqTrimOp(c)][, QTrimOp(F, B)][, ShortenOp(length)][, NTrimOp()]``.  The op sits BETWEEN the quality trimmer
and the N trimmer, so the existing tail is applied without its N trim, then the read is shortened, then the N trim runs.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

import endtrim_rule as E
import nextseq_rule as N

F_TOO_SHORT = E.F_TOO_SHORT
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the rule, one read

def shorten(n: int, length: int) -> tuple:
    """-> (start, stop) of what ``Shortener(length)`` leaves of a read of n bases: Python's own slice."""
    kept = range(n)[:length] if length >= 0 else range(n)[length:]
    if len(kept) == 0:  # length 0 (or n 0): the empty interval at the read's start, [s, s)
        return 0, 0
    return kept[0], kept[-1] + 1


# ---- the rule over rows

def shortens(begin, end, length: int):
    """-> (start [n], stop [n]) as positions in the rows, of the intervals [begin, end)."""
    begin = np.asarray(begin, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    n = end - begin
    if length >= 0:
        return begin.copy(), begin + np.minimum(n, np.int64(length))
    return end - np.minimum(n, np.int64(-int(length))), end.copy()


# ---- layered over intervals that something else decided

class Tail(NamedTuple):
    """The end of a chain: nextseq_rule's tail (NextSeq trimmer, quality trimmer, N trimmer) with ``Shortener(length)``
    (None: no such op) between its quality trimmer and its N trimmer."""
    length: Optional[int] = None
    rest: N.Tail = N.Tail()


def apply_tail(seq_rows, qual_rows, begin, end, flags, tail: Tail, min_length: int = 0) -> E.Ends:
    """nextseq_rule.apply_tail without its N trim, the shortening, the N trim, TooShort on what is left."""
    inner = tail.rest.rest
    front = N.Tail(tail.rest.nextseq, tail.rest.base, inner._replace(trim_n=False))
    ends = N.apply_tail(seq_rows, qual_rows, begin, end, flags, front, 0)
    start, stop = ends.start, ends.stop
    if tail.length is not None:
        start, stop = shortens(start, stop, tail.length)
    if inner.trim_n:
        start, stop = E.ntrims(seq_rows, start, stop)
    out = (ends.flags & ~F_TOO_SHORT) | np.where(stop - start < min_length, F_TOO_SHORT, 0)
    return E.Ends(start, stop, out, ends.cut)


def split_tail(ops: Sequence, qtrim_type, ntrim_type, nextseq_type, shorten_type):
    """A chain's ops -> (the ops in front of its trailing NextSeqTrimOp / QTrimOp / ShortenOp / NTrimOp, Tail)."""
    ops = list(ops)
    trim_n = bool(ops) and isinstance(ops[-1], ntrim_type)
    if trim_n:
        ops.pop()
    length = None
    if ops and isinstance(ops[-1], shorten_type):
        length = ops.pop().length
    ops, rest = N.split_tail(ops, qtrim_type, ntrim_type, nextseq_type)
    assert not rest.rest.trim_n  # (an N trimmer in front of the Shortener: not a chain the compiler builds)
    return ops, Tail(length, N.Tail(rest.nextseq, rest.base, rest.rest._replace(trim_n=trim_n)))
