"""``--too-long-output`` restated for the tests: ``filters_rule`` with the one changed line -- a pair whose first
catching filter is TooLong goes to stream 3 when the option is on -- and the four streams the rule makes of the string
pipeline's records (``test_gpu_filters_cli.apply_rule`` with the fourth)."""
import filters_rule
from cutseq_amd import abi

NAMES = [name for name, _bit in filters_rule.ORDER]


def route(flags1: int, flags2: int, x1: int, x2: int, untrimmed_filter: bool, too_long_route: bool = True):
    """``filters_rule.route``; 3 instead of ``"too_long"`` with ``too_long_route``."""
    where = filters_rule.route(flags1, flags2, x1, x2, untrimmed_filter)
    return 3 if too_long_route and where == "too_long" else where


def bits_of(record: bytes, max_length, max_n, max_ee) -> int:
    """The CS_X_* bits of one final read, taken from its output record (FASTQ)."""
    import maxn_rule
    _name, seq, _plus, qual = record.split(b"\n")[:4]
    x = 0
    if max_length is not None and filters_rule.too_long(len(seq), max_length):
        x |= abi.CS_X_TOO_LONG
    if max_n is not None and maxn_rule.too_many_n(seq, max_n):
        x |= abi.CS_X_TOO_MANY_N
    if max_ee is not None and filters_rule.too_many_ee(qual, max_ee):
        x |= abi.CS_X_TOO_MANY_EE
    return x


def apply_rule(records, max_length=None, max_n=None, max_ee=None, too_long_route: bool = True):
    """``records``: [(route, record 1, record 2 | None)] of the string pipeline, no filter.
    -> streams[route][mate] (four of them), {filter: pairs it caught first}, the pair bits of the pairs TooShort did not
    take.  ``gone["too_long"]`` counts the pairs TooLong caught whether they are written (stream 3) or not."""
    streams = [[b"", b""] for _ in range(4)]
    gone = dict.fromkeys(NAMES, 0)
    pair_bits = []
    for rt, a, b in records:
        x1 = bits_of(a, max_length, max_n, max_ee)
        x2 = bits_of(b, max_length, max_n, max_ee) if b is not None else 0
        flags = abi.CS_F_TOO_SHORT if rt == 1 else (abi.CS_F_UNTRIMMED if rt == 2 else 0)
        where = route(flags, 0, x1, x2, True, too_long_route)
        if rt != 1:
            pair_bits.append(x1 | x2)
        if where == 3:
            gone["too_long"] += 1
        elif where in gone:
            gone[where] += 1
            continue
        else:
            assert where == rt
        streams[where][0] += a
        if b is not None:
            streams[where][1] += b
    return streams, gone, pair_bits
