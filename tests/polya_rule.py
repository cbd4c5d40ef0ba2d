"""cutadapt's ``PolyATrimmer`` (``--poly-a``; ``qualtrim.pyx::poly_a_trim_index``), restated for the tests as
``include/cutseq_hip.h`` states it for CS_OP_POLYA.  Plain Python over one read, numpy over rows; neither calls the
oracle, pyref or the product.  The rule is RECALLED from cutadapt; ``tools/pin_against_cutadapt.py``
holds it to cutadapt itself wherever that is installed.

The rule on the bases b[0..n) of an interval.  Bytes are compared exactly: only ``A`` (head form: ``T``) matches.

    tail:  score = errors = best = 0; index = n
           for i = n-1 down to 0:
               if b[i] == 'A': score += 1   else: score -= 2; errors += 1
               if score > best and errors * 5 <= n - i:   best = score; index = i
           if index > n - 3: index = n            # tails shorter than 3 are ignored
           keep [0, index)                        # trimmed_bases += n - index
    head:  the mirror image: 'T', i = 0 .. n-1, condition errors * 5 <= i + 1, index = i + 1,
           if index < 3: index = 0;  keep [index, n);  trimmed_bases += index

Equivalent facts (``rows_keep`` is built on them, ``tests/test_polya_cpu.py`` holds them to the loops by enumeration):
  * a candidate of length l with e errors has score l - 3e, so ``errors * 5 <= l``  <=>  ``5 * score >= 2 * l``;
  * the result is the FIRST position in walk order that attains the maximum score among the qualifying positions with
    score > 0: a maximum over (score, position) keys;
  * a walk that stands at length l with score sc is settled when ``sc + (n - l) <= best`` (no later position can beat the
    best one) or ``5 * (sc + n - l) < 2 * n`` (no later position can qualify).

``model`` is the kernels' road -- rounds of 64 bases aligned to the row's dwords, keys, the two exits -- as a MODEL for
the CPU tests: ``DEFECTS`` names four ways of getting the rule wrong, and the tests show that the enumerated reads tell
every one of them from the loops.

The universes: ``universe_e`` (every string over {A, C} of length 0..14), ``universe_m`` (every string over {A, a, N} of
length 0..8), ``universe_h`` (the homopolymer universe of tests/poly_rule.py placed with base A / T, plain and with
lower-case letters mixed in).  Each comes for the tail as it stands and translated (A -> T, C -> G, a -> t) for the head.
"""
from __future__ import annotations

import functools
import itertools
from typing import NamedTuple, Optional

import numpy as np

import poly_rule as P

TAIL_BASE, HEAD_BASE = ord("A"), ord("T")
MIN_TAIL = 3


# ---- the rule, one read: the loops as cutadapt writes them

def tail_index(b: bytes) -> int:
    """poly_a_trim_index(b, revcomp=False) -> index: b[:index] stays."""
    n = len(b)
    score = errors = best = 0
    index = n
    for i in range(n - 1, -1, -1):
        if b[i] == TAIL_BASE:
            score += 1
        else:
            score -= 2
            errors += 1
        if score > best and errors * 5 <= n - i:
            best = score
            index = i
    if index > n - MIN_TAIL:
        index = n
    return index


def head_index(b: bytes) -> int:
    """poly_a_trim_index(b, revcomp=True) -> index: b[index:] stays."""
    n = len(b)
    score = errors = best = 0
    index = 0
    for i in range(n):
        if b[i] == HEAD_BASE:
            score += 1
        else:
            score -= 2
            errors += 1
        if score > best and errors * 5 <= i + 1:
            best = score
            index = i + 1
    if index < MIN_TAIL:
        index = 0
    return index


def keep(b: bytes, head: bool) -> tuple:
    """-> (start, stop) of what the trimmer leaves of b."""
    return (head_index(b), len(b)) if head else (0, tail_index(b))


# ---- the closed-form facts, one read

def by_facts(b: bytes, head: bool) -> tuple:
    """``keep`` from the facts alone: scores l - 3e, the rate test on the score, the first maximum among the qualifying
    positions -- no running best, no error test."""
    n = len(b)
    walk = b[::-1] if not head else b
    base = HEAD_BASE if head else TAIL_BASE
    best, length, e = 0, 0, 0
    for l in range(1, n + 1):
        e += walk[l - 1] != base
        score = l - 3 * e
        if 5 * score >= 2 * l and score > best:  # (strictly greater: the first position of a score keeps it)
            best, length = score, l
    if length < MIN_TAIL:
        length = 0
    return (length, n) if head else (0, n - length)


# ---- the kernels' road, as a model

DEFECTS = ("rate_strict",      # errors * 5 < length in place of <=
           "min_two",          # tails of 2 go
           "last_maximum",     # the LAST position of the highest score
           "lower_case_match")  # 'a' / 't' counted as a match


class Walked(NamedTuple):
    start: int
    stop: int
    bases: int  # bases the walk looked at before it was settled


def model(b: bytes, head: bool, s: int = 0, defect: Optional[str] = None) -> Walked:
    """The wave walk on one read whose interval begins at row position ``s`` (the rounds are aligned to the row's dwords):
    a round takes the 16 dwords below the position reached, keeps the best (score, position) key, and the walk ends when
    no later position can beat the best score or qualify."""
    assert defect is None or defect in DEFECTS
    n = len(b)
    base = HEAD_BASE if head else TAIL_BASE
    # walk coordinates: position p of the mirrored row for the head form (trim_kernel.hip.inc, CS_OP_POLYA)
    top = max(2047, (s + n + 3) // 4 * 4 + 3)  # (rows end at 2047; a longer read gets a mirror of its own size)
    ms = (top + 1) - (s + n) if head else s
    walk = b[::-1] if head else b  # walk[p - ms]: the base at walk position p
    p_last = ms + n - 1
    score, best_key = 0, (0, top)  # (score, position): a higher position wins among equal scores
    dw = max(p_last, 0) >> 2
    looked = 0
    running = n > 0
    while running:
        for p in range(min(4 * dw + 3, p_last), max(4 * (dw - 15), ms) - 1, -1):
            ch = walk[p - ms]
            match = ch == base or (defect == "lower_case_match" and ch == base + 32)
            score += 1 if match else -2
            length = p_last - p + 1
            looked += 1
            rate = 5 * score > 2 * length if defect == "rate_strict" else 5 * score >= 2 * length
            if score > 0 and rate:
                key = (score, -p) if defect == "last_maximum" else (score, p)
                if key > best_key:
                    best_key = key
        dw -= 16
        left = 4 * dw + 4 - ms
        running = left > 0 and score + left > best_key[0] and 5 * (score + left) >= 2 * n
    index = n
    if best_key[0] > 0:
        index = abs(best_key[1]) - ms
    if index > n - (2 if defect == "min_two" else MIN_TAIL):
        index = n
    return Walked(n - index, n, looked) if head else Walked(0, index, looked)


# ---- the rule over rows: prefix sums and the closed form

def rows_keep(seq: np.ndarray, begin, end, head: bool, chunk: int = 32768):
    """The trimmer on the intervals [begin, end) of the rows -> (start [n], stop [n]) as positions in the rows."""
    begin = np.broadcast_to(np.asarray(begin, dtype=np.int64), (len(seq),)).copy()
    end = np.maximum(np.broadcast_to(np.asarray(end, dtype=np.int64), (len(seq),)), begin)
    length = np.zeros(len(seq), dtype=np.int64)
    for lo in range(0, len(seq), chunk):  # (bounded temporaries: the homopolymer universe has 200 000 rows)
        sl = slice(lo, lo + chunk)
        n = end[sl] - begin[sl]
        width = int(n.max(initial=0))
        if width == 0:
            continue
        step = np.arange(width, dtype=np.int64)[None, :]  # l - 1
        at = (begin[sl, None] + step) if head else (end[sl, None] - 1 - step)
        inside = step < n[:, None]
        letters = np.take_along_axis(seq[sl], np.clip(at, 0, seq.shape[1] - 1), axis=1)
        match = (letters == (HEAD_BASE if head else TAIL_BASE)) & inside
        score = np.cumsum(np.where(match, 1, -2), axis=1, dtype=np.int64)
        good = inside & (score > 0) & (5 * score >= 2 * (step + 1))
        masked = np.where(good, score, 0)
        length[sl] = np.where(masked.max(axis=1) > 0, masked.argmax(axis=1) + 1, 0)  # argmax: the first maximum
    length = np.where(length < MIN_TAIL, 0, length)
    if head:
        return begin + length, end.copy()
    return begin.copy(), end - length


def trimmed(begin, end, start, stop) -> int:
    """``PolyATrimmer.trimmed_bases`` of a batch."""
    return int(((np.asarray(end, dtype=np.int64) - begin) - (np.asarray(stop, dtype=np.int64) - start)).sum())


# ---- the universes

class Rows(NamedTuple):
    seq: np.ndarray   # [n, stride] uint8
    qual: np.ndarray  # [n, stride] uint8: 'I' under every base
    lens: np.ndarray  # [n] uint16


def rows_of(reads, stride: Optional[int] = None, pad: bytes = b"N") -> Rows:
    longest = max((len(r) for r in reads), default=0)
    stride = max(4, (longest + 3) // 4 * 4) if stride is None else stride
    seq = np.full((len(reads), stride), pad[0], dtype=np.uint8)
    lens = np.zeros(len(reads), dtype=np.uint16)
    for i, r in enumerate(reads):
        seq[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        lens[i] = len(r)
    return with_qualities(seq, lens)


def with_qualities(seq: np.ndarray, lens: np.ndarray) -> Rows:
    under = np.arange(seq.shape[1])[None, :] < lens.astype(np.int64)[:, None]
    return Rows(np.ascontiguousarray(seq), np.where(under, ord("I"), ord("!")).astype(np.uint8), lens.astype(np.uint16))


HEAD_LETTERS = bytes.maketrans(b"ACac", b"TGtg")


def strings(alphabet: bytes, longest: int):
    return [bytes(t) for L in range(longest + 1) for t in itertools.product(alphabet, repeat=L)]


@functools.lru_cache(maxsize=None)
def universe_e(head: bool):
    """Every string over {A, C} of length 0..14 (head: {T, G}): 32 767 reads."""
    reads = strings(b"AC", 14)
    return [r.translate(HEAD_LETTERS) for r in reads] if head else reads


@functools.lru_cache(maxsize=None)
def universe_m(head: bool):
    """Every string over {A, a, N} of length 0..8 (head: {T, t, N}): 9 841 reads."""
    reads = strings(b"AaN", 8)
    return [r.translate(HEAD_LETTERS) for r in reads] if head else reads


@functools.lru_cache(maxsize=None)
def _full() -> P.Reads:
    return P.full()


def universe_h(head: bool, lower_every: int = 0, foreign: str = "C", pad: int = 0) -> Rows:
    """tests/poly_rule.py's universe (201 036 reads) with base A for the tail, T for the head; ``lower_every``: every
    such base of the runs in lower case; ``pad``: that many G in front of (head) / behind (tail) the read, for a cut."""
    reads = _full()
    base = "T" if head else "A"
    seq, lens = P.place(P.letters(reads, base, foreign, lower_every=lower_every), reads.lens, head, pad=pad, stride=P.WIDTH + 8)
    seq[seq == 0] = ord("N")  # (behind the reads: the letter this package's own producers pad with)
    return with_qualities(seq, lens)
