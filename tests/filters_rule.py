"""cutadapt's TooLong (``-M``) and TooManyExpectedErrors (``--max-ee``) restated in Python for the tests, with the route
and precedence rule of the three discarding filters (``tests/maxn_rule.py`` has TooManyN).  The oracle knows nothing of
filters, so the tests take the oracle's intervals and apply these rules (``include/cutseq_hip.h``,
cs_plan_set_max_length / cs_plan_set_max_ee)."""
import numpy as np

import maxn_rule
from cutseq_amd import abi

# T[b] = 10 ** (-(b - 33) / 10), indexed by the raw quality byte
EE_TABLE = [10 ** (-(b - 33) / 10) for b in range(256)]

# the order of the discarding steps: (total's name, bit)
ORDER = (("too_long", abi.CS_X_TOO_LONG), ("too_many_n", abi.CS_X_TOO_MANY_N), ("too_many_ee", abi.CS_X_TOO_MANY_EE))


def too_long(length: int, max_length: int) -> bool:
    return length > max_length


def expected_errors(qual: bytes) -> float:
    """``qual``: the quality bytes of the final interval.  A left-to-right sum in double."""
    e = 0.0
    for b in qual:
        e += EE_TABLE[b]
    return e


def too_many_ee(qual: bytes, max_ee: float) -> bool:
    return expected_errors(qual) > max_ee


def xflags(seq: np.ndarray, qual: np.ndarray, res: np.ndarray, max_length=None, max_n=None, max_ee=None) -> np.ndarray:
    """Expected ``cs_reads.xflags`` for rows ``seq`` / ``qual`` [n, stride] and results ``res`` (RESULT_DTYPE, or any
    record array with ``start`` and ``stop``); a filter that is None is off."""
    out = np.zeros(len(res), dtype=np.uint8)
    starts, stops = res["start"].astype(np.int64), res["stop"].astype(np.int64)
    for i in range(len(res)):
        s, e = int(starts[i]), int(stops[i])
        if max_length is not None and too_long(max(e - s, 0), max_length):
            out[i] |= abi.CS_X_TOO_LONG
        if max_n is not None and maxn_rule.too_many_n(seq[i, s:e].tobytes(), max_n):
            out[i] |= abi.CS_X_TOO_MANY_N
        if max_ee is not None and too_many_ee(qual[i, s:e].tobytes(), max_ee):
            out[i] |= abi.CS_X_TOO_MANY_EE
    return out


def route(flags1: int, flags2: int, x1: int, x2: int, untrimmed_filter: bool):
    """TooShort -> TooLong -> TooManyN -> TooManyExpectedErrors -> IsUntrimmedAny -> sink, pair filter "any".
    -> 0 / 1 / 2 for the trimmed / short / untrimmed route, or the name of the discarding filter that takes the pair
    (the first in that order)."""
    f, x = flags1 | flags2, x1 | x2
    if f & abi.CS_F_TOO_SHORT:
        return 1
    for name, bit in ORDER:
        if x & bit:
            return name
    if untrimmed_filter and (f & abi.CS_F_UNTRIMMED):
        return 2
    return 0
