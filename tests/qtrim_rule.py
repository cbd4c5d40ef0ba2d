"""cutadapt's 3' quality trimming (``qualtrim.pyx quality_trim_index``, ``cutoff_front = 0``) restated for the tests,
and the ENUMERATED inputs that hold the trimmers of every kernel to it (``trim_kernel.hip.inc``, the CS_OP_QTRIM branch
of the scan and the resolve kernel; ``long_kernel.hip.inc``, quality_stop).

The rule: walk the interval from its last base down, ``sum += cutoff - (q - base)``; stop at the first negative sum; the
answer is the position of the first strict maximum of the sums seen (the interval's length when no sum is positive).
``stop`` says it with Python ints, ``stops`` with numpy int64 over rows: neither can overflow, neither calls the
oracle, pyref or the product.

``geometry`` says WHERE the tile kernels look at a position -- which dword below the dword of the interval's last base,
hence which round of 64 bases and which of the 16 lanes of a group -- and nothing about sums or keys: the tests use it
only to show that the families reach every lane in every role.

A quality byte is named by its delta: the byte that adds ``delta`` to the sum under (cutoff, base) is
``cutoff + base - delta``; delta 0 is neutral, a negative delta is a GOOD base.  Every family is deterministic (no seed);
sequence bytes are ``A``; a family built "behind f" has ``f`` bytes of quality ``!`` in front of every row for a
``CutOp(+f)`` to remove -- a kernel that read them would notice.  Bytes behind a row's length are ``!`` as well.
"""
from __future__ import annotations

import itertools
from typing import NamedTuple, Sequence

import numpy as np

import universe as U

CUTOFF, BASE = 20, 33
F_QTRIMMED = 0x10  # CS_F_QTRIMMED (include/cutseq_hip.h)
PAD = ord("!")
CHUNK = 1 << 15


# ---- the rule

def stop(qual: bytes, cutoff: int, base: int = 33) -> int:
    s = best = 0
    at = len(qual)
    for i in range(len(qual) - 1, -1, -1):
        s += cutoff - (qual[i] - base)
        if s < 0:
            break
        if s > best:
            best, at = s, i
    return at


class Walks(NamedTuple):
    stop: np.ndarray  # relative to the interval's start, like ``stop``
    brk: np.ndarray   # position (in the row) of the first negative sum, -1: the walk reaches the start
    best: np.ndarray  # position (in the row) of the first strict maximum, -1: no positive sum


def walks(qual_rows: np.ndarray, start, end, cutoff: int, base: int = 33) -> Walks:
    """The rule on the interval [start, end) of every row of ``qual_rows`` [n, stride]; start / end: scalars or [n]."""
    q = np.asarray(qual_rows)
    n, w = q.shape
    start = np.broadcast_to(np.asarray(start, dtype=np.int64), (n,))
    end = np.broadcast_to(np.asarray(end, dtype=np.int64), (n,))
    cols = np.arange(w, dtype=np.int64)
    out = Walks(np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64))
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(lo + CHUNK, n))
        s, e = start[sl, None], end[sl, None]
        inside = (cols >= s) & (cols < e)
        term = np.where(inside, int(cutoff) + int(base) - q[sl].astype(np.int64), 0)
        run = np.cumsum(term[:, ::-1], axis=1)[:, ::-1]  # run[i]: the sum once position i is added
        neg = inside & (run < 0)
        brk = np.where(neg.any(axis=1), w - 1 - np.argmax(neg[:, ::-1], axis=1), -1)  # cut at the first negative
        seen = inside & (cols > brk[:, None])
        top = np.where(seen, run, 0).max(axis=1, initial=0)
        hit = seen & (run == top[:, None]) & (top[:, None] > 0)  # first strict maximum: the highest such position
        pos = w - 1 - np.argmax(hit[:, ::-1], axis=1)
        out.stop[sl] = np.where(top > 0, pos - start[sl], end[sl] - start[sl])
        out.brk[sl] = brk
        out.best[sl] = np.where(top > 0, pos, -1)
    return out


def stops(qual_rows: np.ndarray, start, end, cutoff: int, base: int = 33) -> np.ndarray:
    return walks(qual_rows, start, end, cutoff, base).stop


def clamp(cutoff: int, base: int = 33) -> int:
    """The cutoff as cs_plan_create keeps it: cutoff + base in [-1, 256] (outside, every term has one sign)."""
    return max(-1 - base, min(int(cutoff), 256 - base))


class Place(NamedTuple):
    rel: np.ndarray    # dwords below the dword of the interval's last base (0: that dword, judged per lane)
    round: np.ndarray  # 1, 2, ...: the round of 16 dwords that serves it (0 for rel 0)
    lane: np.ndarray   # 0..15: the lane of the group that serves it (-1 for rel 0)


def geometry(start, end, pos) -> Place:
    """Where the tile kernels look at position ``pos`` of the interval [start, end), end > start."""
    end, pos = np.asarray(end, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    rel = ((end - 1) >> 2) - (pos >> 2)
    return Place(rel, np.where(rel > 0, (rel - 1) // 16 + 1, 0), np.where(rel > 0, (rel - 1) % 16, -1))


# ---- the families

class Rows(NamedTuple):
    seq: np.ndarray   # [n, stride] uint8
    qual: np.ndarray  # [n, stride] uint8
    lens: np.ndarray  # [n] uint16
    f: int            # bytes in front of every row that are not part of the family's string


def qbyte(delta: int, cutoff: int = CUTOFF, base: int = BASE) -> int:
    b = cutoff + base - delta
    assert 0 <= b <= 255, (delta, cutoff, base)
    return b


def finish(qual: np.ndarray, lens: np.ndarray, f: int) -> Rows:
    """``qual``'s rows hold the strings from column f on: prefix and padding filled, sequence ``A``."""
    cols = np.arange(qual.shape[1])
    qual[:, :f] = PAD
    qual[cols[None, :] >= lens[:, None]] = PAD
    seq = np.where(cols[None, :] < lens[:, None], ord("A"), 0).astype(np.uint8)
    return Rows(seq, np.ascontiguousarray(qual), lens.astype(np.uint16), f)


def strings(byte_values: Sequence[int], max_len: int):
    """Every string over ``byte_values`` of length 0..max_len -> (bytes [n, width], len [n])."""
    letters = "ABCDEFGH"[:len(byte_values)]
    s, ln = U.reads_universe(letters, max_len)
    lut = np.zeros(256, dtype=np.uint8)
    for ch, b in zip(letters, byte_values):
        lut[ord(ch)] = b
    return lut[s], ln


def behind(body: np.ndarray, lens: np.ndarray, f: int, stride: int) -> Rows:
    qual = np.zeros((len(lens), stride), dtype=np.uint8)
    w = min(body.shape[1], stride - f)
    assert int(lens.max(initial=0)) <= w
    qual[:, f:f + w] = body[:, :w]
    return finish(qual, lens.astype(np.int64) + f, f)


ALPHABETS = ((-1, 0, +1), (-3, +1, +2))


def f1(f: int, alphabet=ALPHABETS[0], max_len: int = 10, cutoff: int = CUTOFF, base: int = BASE, stride: int = 16) -> Rows:
    """Enumeration: every string over three deltas, length 0..max_len."""
    body, ln = strings([qbyte(d, cutoff, base) for d in alphabet], max_len)
    return behind(body, ln, f, stride)


def f1_bytes(f: int, byte_values: Sequence[int], max_len: int = 10, stride: int = 16) -> Rows:
    body, ln = strings(byte_values, max_len)
    return behind(body, ln, f, stride)


def windows(max_len: int, alphabet=ALPHABETS[0]):
    return [w for L in range(max_len + 1) for w in itertools.product(alphabet, repeat=L)]


def placed(f: int, stride: int, items, cutoff: int = CUTOFF, base: int = BASE) -> Rows:
    """Rows ``neutral x a + window + neutral x d`` (the last base +1 where ``tail``) from (a, window, d, tail) items."""
    n = len(items)
    a = np.fromiter((it[0] for it in items), np.int64, n)
    wl = np.fromiter((len(it[1]) for it in items), np.int64, n)
    d = np.fromiter((it[2] for it in items), np.int64, n)
    tail = np.fromiter((it[3] for it in items), bool, n)
    lens = f + a + wl + d + tail
    assert int(lens.max(initial=0)) <= stride
    qual = np.full((n, stride), qbyte(0, cutoff, base), dtype=np.uint8)
    rows = np.arange(n)
    for j in range(int(wl.max(initial=0))):
        m = wl > j
        qual[rows[m], f + a[m] + j] = np.fromiter((qbyte(it[1][j], cutoff, base) for it, mm in zip(items, m) if mm), np.uint8)
    qual[rows[tail], lens[tail] - 1] = qbyte(+1, cutoff, base)
    return finish(qual, lens, f)


DEPTHS = range(136)


def f2(product: str, f: int, max_window=None, depths=DEPTHS, stride: int = 152) -> Rows:
    """A window at every depth.  Product "A": windows of length 0..4 behind two neutral bases; "B": windows of length
    0..2 that open the interval."""
    a, wmax = (2, 4) if product == "A" else (0, 2)
    wins = windows(wmax if max_window is None else max_window)
    return placed(f, stride, [(a, w, d, tail) for w in wins for d in depths for tail in (False, True)])


F3_LANES = ((0,), (63,), (15, 16), (31, 32), (20, 40, 63), (0, 21, 42, 63), (3, 17, 30, 44, 60),
            (1, 9, 18, 27, 36, 45, 62), tuple(range(64)))
F3_WINDOWS = ((-1,), (-1, -1, +1))  # (the walk meets a window last byte first)


def f3(f: int, stride: int = 152):
    """Occupancy: tiles of 64 consecutive rows, dead rows (last base -1: the walk ends in the top dword) but for k
    walkers at chosen lanes whose walks end in rounds 1, 2 and 3 -- or, in every other tile, all in round 2.
    -> (Rows, [k per tile])."""
    items, ks = [], []
    for lanes in F3_LANES:
        for win in F3_WINDOWS:
            for equal in (False, True):
                at = {lane: i for i, lane in enumerate(lanes)}
                for lane in range(64):
                    if lane in at:
                        i = at[lane]
                        items.append((2, win, 80 if equal else (20, 80, 140)[i % 3] + i // 3 % 4, False))
                    else:
                        items.append((16 + lane % 7, (-1,), 0, False))
                ks.append(len(lanes))
    return placed(f, stride, items), ks


F4_LENGTHS = tuple(range(1020, 1029)) + tuple(range(1532, 1537))


def f4(f: int, stride: int = 1536):
    """Long rows: windows of length 0..3 at positions around 1024, at depths 63..65, and at the interval's start;
    then, per length, every byte ``!`` and every byte ``~``.  Lengths are the strings' (the row has f more)."""
    wins = windows(3)
    items = []
    for L in F4_LENGTHS:
        L = min(L, stride - f)
        for w in wins:
            room = L - len(w)
            spots = [p for p in (1022, 1023, 1024, 1025) if p <= room] + [room - d for d in (63, 64, 65)] + [0, 1]
            for a in spots:
                for tail in (False, True):
                    if room - a - tail >= 0:
                        items.append((a, w, room - a - tail, tail))
    rows = placed(f, stride, items)
    flat = np.full((2 * len(F4_LENGTHS), stride), PAD, dtype=np.uint8)
    lens = np.zeros(len(flat), dtype=np.int64)
    for i, L in enumerate(F4_LENGTHS):
        L = min(L, stride - f)
        lens[2 * i] = lens[2 * i + 1] = L + f
        flat[2 * i, f:f + L] = ord("!")
        flat[2 * i + 1, f:f + L] = ord("~")
    extra = finish(flat, lens, f)
    return Rows(np.concatenate([rows.seq, extra.seq]), np.concatenate([rows.qual, extra.qual]),
                np.concatenate([rows.lens, extra.lens]), f)


F5_SETTINGS = ((0, 33), (2, 33), (41, 33), (93, 33), (20, 64))
F5_EDGE_BYTES = (0, qbyte(0), 255)  # at the default setting: deltas +53, 0, -202

F6_CUTOFFS = (-32768, -35, -34, -33, 222, 223, 224, 1000, 32767)


def f6_short(stride: int = 40) -> Rows:
    """40 x ``I``, then F1's first alphabet up to length 8."""
    body, ln = strings([qbyte(d) for d in ALPHABETS[0]], 8)
    qual = np.zeros((1 + len(ln), stride), dtype=np.uint8)
    qual[0, :40] = ord("I")
    qual[1:, :body.shape[1]] = body
    return finish(qual, np.concatenate([[40], ln.astype(np.int64)]), 0)


def f6_long(stride: int = 1536) -> Rows:
    """1 500 x ``I`` (and a full row of it, and 1 500 x ``!``, ``5`` and byte 255), in rows of stride 1536."""
    spec = [(1500, ord("I")), (1536, ord("I")), (1500, ord("!")), (1500, ord("5")), (1500, 255), (1536, 0)]
    qual = np.zeros((len(spec), stride), dtype=np.uint8)
    for i, (L, b) in enumerate(spec):
        qual[i, :L] = b
    return finish(qual, np.array([L for L, _ in spec], dtype=np.int64), 0)


def expected(rows: Rows, f: int, cutoff: int, base: int = 33, end=None, flags=0) -> tuple:
    """What ``[CutOp(+f), QTrimOp(cutoff, base)]`` leaves of rows whose interval ends at ``end`` (default: the length)
    -> (start [n], stop [n], flags [n], quality-trimmed bases)."""
    lens = rows.lens.astype(np.int64)
    end = lens if end is None else np.asarray(end, dtype=np.int64)
    start = np.minimum(f, end)
    keep = stops(rows.qual, start, end, cutoff, base)
    cut = (end - start) - keep
    return start, start + keep, np.asarray(flags) | np.where(cut > 0, F_QTRIMMED, 0), int(cut.sum())
