"""cutadapt's TooManyN (``--max-n``) restated in Python for the tests: the oracle knows nothing of the filter, so the
tests take the oracle's intervals and apply this rule (``include/cutseq_hip.h``, cs_plan_set_max_n)."""
import numpy as np

from cutseq_amd import abi


def too_many_n(seq: bytes, count: float) -> bool:
    """``seq``: the final interval of the read.  count < 1: proportion (strict >, an empty read is kept)."""
    n = seq.lower().count(b"n")
    if count < 1.0:
        return len(seq) > 0 and n / len(seq) > count
    return n > count


def xflags(seq: np.ndarray, res: np.ndarray, count: float) -> np.ndarray:
    """Expected ``cs_reads.xflags`` for rows ``seq`` [n, stride] and results ``res`` (RESULT_DTYPE)."""
    out = np.zeros(len(res), dtype=np.uint8)
    starts, stops = res["start"].astype(np.int64), res["stop"].astype(np.int64)
    for i in range(len(res)):
        if too_many_n(seq[i, starts[i]:stops[i]].tobytes(), count):
            out[i] = abi.CS_X_TOO_MANY_N
    return out


def route(flags1: int, flags2: int, x1: int, x2: int, untrimmed_filter: bool):
    """TooShort -> TooManyN (discard: None) -> IsUntrimmedAny -> sink, pair filter "any"."""
    f = flags1 | flags2
    if f & abi.CS_F_TOO_SHORT:
        return 1
    if (x1 | x2) & abi.CS_X_TOO_MANY_N:
        return None
    if untrimmed_filter and (f & abi.CS_F_UNTRIMMED):
        return 2
    return 0
