"""cutadapt's ``NextseqQualityTrimmer(cutoff, base)`` (``--nextseq-trim``; ``qualtrim.pyx nextseq_trim_index``), restated
for the tests as ``include/cutseq_hip.h`` states it for CS_OP_NEXTSEQ.  Plain Python over one read and numpy int64 over
rows: neither can overflow, neither calls the oracle, pyref or the product.

The rule on an interval of n bases b[0..n) with quality bytes q[0..n): walk from n - 1 down,
``sum += 1 if b[i] == 'G' else cutoff - (q[i] - base)``; stop at the first negative sum; ``stop`` = the position of the
first strict maximum, n when no sum is positive.  ``G`` is the byte 0x47: ``g`` is an ordinary base.

That is the quality trimmer's 3' walk (tests/qtrim_rule.py) on qualities in which every ``G`` carries the byte
``cutoff + base - 1``.  ``stop`` spells the rule out; ``stops`` uses the property -- ``qtrim_rule.stops`` on the
substituted rows (int64: the byte may be -2 or -1 at the low end of the accepted cutoffs).  The tests hold the two to
each other.

``apply_tail`` / ``split_tail`` are those of tests/endtrim_rule.py for chains that end
``..., NextSeqTrimOp(cutoff)[, QTrimOp(F, B)][, NTrimOp()]``: the C oracle knows none of the three.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

import endtrim_rule as E
import qtrim_rule as R

G = 0x47
F_QTRIMMED = R.F_QTRIMMED
CUTOFF_LOW, CUTOFF_HIGH = -1, 256  # cutoff + base the op accepts (outside: CS_ERR_ARG, no clamp)


# ---- the rule, one read

def stop(seq: bytes, qual: bytes, cutoff: int, base: int = 33) -> int:
    assert len(seq) == len(qual)
    s = best = 0
    at = len(qual)
    for i in range(len(qual) - 1, -1, -1):
        s += 1 if seq[i] == G else cutoff - (qual[i] - base)
        if s < 0:
            break
        if s > best:
            best, at = s, i
    return at


# ---- the rule over rows: a G is a base of quality byte cutoff + base - 1

def as_qualities(seq_rows: np.ndarray, qual_rows: np.ndarray, cutoff: int, base: int = 33, g=(G,)) -> np.ndarray:
    """The quality rows (int64) with ``cutoff + base - 1`` under every ``G``.  ``g``: the bytes read as G -- the tests
    pass (0x47, 0x67) to say what a case-folding reading would give."""
    q = np.asarray(qual_rows).astype(np.int64)
    q[np.isin(np.asarray(seq_rows), g)] = int(cutoff) + int(base) - 1
    return q


def stops(seq_rows: np.ndarray, qual_rows: np.ndarray, begin, end, cutoff: int, base: int = 33, g=(G,)) -> np.ndarray:
    """-> stop [n], relative to ``begin``, of the interval [begin, end) of every row."""
    return R.stops(as_qualities(seq_rows, qual_rows, cutoff, base, g), begin, end, cutoff, base)


# ---- layered over intervals that something else decided

class Tail(NamedTuple):
    """The end of a chain: ``NextseqQualityTrimmer(nextseq, base)`` (None: no such op), then endtrim_rule's tail."""
    nextseq: Optional[int] = None
    base: int = 33
    rest: E.Tail = E.Tail()


def apply_tail(seq_rows, qual_rows, begin, end, flags, tail: Tail, min_length: int = 0) -> E.Ends:
    """endtrim_rule.apply_tail with the NextSeq trimmer in front; ``cut`` is what both quality trimmers took."""
    n = len(seq_rows)
    begin = np.broadcast_to(np.asarray(begin, dtype=np.int64), (n,)).copy()
    end = np.broadcast_to(np.asarray(end, dtype=np.int64), (n,)).copy()
    end = np.maximum(end, begin)
    flags = np.broadcast_to(np.asarray(flags, dtype=np.int64), (n,))
    cut = 0
    if tail.nextseq is not None:
        keep = stops(seq_rows, qual_rows, begin, end, tail.nextseq, tail.base)
        took = (end - begin) - keep
        flags = flags | np.where(took > 0, F_QTRIMMED, 0)
        cut = int(took.sum())
        end = begin + keep
    ends = E.apply_tail(seq_rows, qual_rows, begin, end, flags, tail.rest, min_length)
    return E.Ends(ends.start, ends.stop, ends.flags, ends.cut + cut)


def split_tail(ops: Sequence, qtrim_type, ntrim_type, nextseq_type):
    """A chain's ops -> (the ops in front of its trailing NextSeqTrimOp / QTrimOp / NTrimOp, Tail)."""
    ops, rest = E.split_tail(ops, qtrim_type, ntrim_type)
    if ops and isinstance(ops[-1], nextseq_type):
        op = ops.pop()
        return ops, Tail(op.cutoff, op.base, rest)
    return ops, Tail(rest=rest)


# ---- inputs: a qtrim_rule family carried over to the new walk

def with_g(rows: R.Rows, cutoff: int = R.CUTOFF, base: int = R.BASE) -> R.Rows:
    """Every base of delta +1 inside a row's string becomes a ``G`` whose quality byte is ``~`` at even positions and
    ``!`` at odd ones: under the NextSeq rule at (cutoff, base) the row means what the original means under the plain
    quality trimmer, so ``qtrim_rule.expected`` of the ORIGINAL rows is the expected result."""
    cols = np.arange(rows.qual.shape[1])[None, :]
    inside = (cols >= rows.f) & (cols < rows.lens.astype(np.int64)[:, None])
    plus = inside & (rows.qual == R.qbyte(+1, cutoff, base))
    seq, qual = rows.seq.copy(), rows.qual.copy()
    seq[plus] = G
    qual[plus] = np.where(cols % 2 == 0, ord("~"), ord("!")).astype(np.uint8).repeat(len(seq), axis=0)[plus]
    return R.Rows(seq, qual, rows.lens, rows.f)
