"""cs_text_create_interleaved on the GPU: one text holding both mates' records (CS_INTERLEAVE_IN) and one stream per route
(CS_INTERLEAVE_OUT).  Every expected value is tests/interleave_rule.py applied to the TWO-FILE engine's run of the same
records -- never the interleaved engine's own output; the two-file engine is held to oracle/pyref.py by the rest of the
suite.

Plans: TAKARAV3 paired with --ensure-inline-barcode on the 1000-pair fixture (the scheme has no inline barcode, so its
route 2 is empty: routes 0 and 1 are asserted non-empty), and the same reads under a scheme WITH an inline barcode that
every other pair is given, so that routes 0, 1 and 2 are all non-empty (asserted)."""
import ctypes as C
import gzip
import statistics

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import interleave_rule
import util
from test_gpu_demux import scheme_with
from test_gpu_filters import fastq_text
from test_gpu_too_long_output import HUGE, as_fasta

pytestmark = pytest.mark.gpu

R1 = str(util.GOLDEN / "fixture1k_R1.fq.gz")
R2 = str(util.GOLDEN / "fixture1k_R2.fq.gz")
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 513]  # the wave and the 256-record scan-block boundaries
MODES = {"in": (True, False), "out": (False, True), "in+out": (True, True)}
INLINE = "ACGTAC"
STRIDE = 160

_CACHE = {}


def fixture():
    if "rec" not in _CACHE:
        _CACHE["rec"] = (util.read_fastq_gz(R1), util.read_fastq_gz(R2))
    return _CACHE["rec"]


def inline_fixture():
    """The fixture with the inline barcode at the start of mate 1 of every other pair, and every fifth pair cut down to
    25 bases (too short once barcode and UMI are gone)."""
    if "inline" not in _CACHE:
        rec1, rec2 = fixture()
        rec1 = [(n, (INLINE.encode() + s[len(INLINE):]) if i % 2 == 0 else s, q) for i, (n, s, q) in enumerate(rec1)]
        rec1 = [(n, s[:25], q[:25]) if i % 5 == 0 else (n, s, q) for i, (n, s, q) in enumerate(rec1)]
        rec2 = [(n, s[:25], q[:25]) if i % 5 == 0 else (n, s, q) for i, (n, s, q) in enumerate(rec2)]
        _CACHE["inline"] = (rec1, rec2)
    return _CACHE["inline"]


def text_of(rec):
    return fastq_text([r[0] for r in rec], [r[1] for r in rec], [r[2] for r in rec])


def takara_engine(max_length=None):
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True, untrimmed_requested=True)
    if max_length is not None:
        tp.max_length = max_length
    return TrimEngine(tp, device=0, slots=0)


def inline_engine():
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    return TrimEngine(util.compile_plan(scheme_with(INLINE), st, True, untrimmed_requested=True), device=0, slots=0)


class Run:
    """One batch through a text engine: streams[route][mate] as fetched, and everything the host reads back."""

    def __init__(self, eng, text1, text2, n, woven_in=False, woven_out=False, mate2_first=False, stride=STRIDE, **kw):
        texts = [text1] if woven_in else [text1, text2]
        with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(t) for t in texts) + 1024, max_records=max(n, 1),
                                 stride=stride, interleave_in=woven_in, interleave_out=woven_out, mate2_first=mate2_first,
                                 **kw) as te:
            te.submit(0, text1, len(text1), None if woven_in else text2, 0 if woven_in else len(text2), n)
            self.res = te.wait(0)
            self.sizes, self.raw, count = te.routes(0)
            self.count = [int(c) for c in count]
            self.discards = te.discards(0) if eng.plan.has_filters else None
            out = [np.empty(max(int(self.res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
            te.fetch(0, out[0], None if woven_out else out[1])
        self.streams = textpath.split_routes(self.sizes, out, True)


def check(eng, rec1, rec2, mode, two=None, mate2_first=False, compress=False, fasta=False, fasta_classes=(), **kw):
    """The interleaved run of a batch against the rule applied to the two-file run -> the two-file run."""
    woven_in, woven_out = MODES[mode]
    n = len(rec1)
    text1, text2 = text_of(rec1), text_of(rec2)
    if fasta:
        kw = dict(kw, fasta=True)
    if two is None:
        two = Run(eng, text1, text2, n, **kw)  # plain text, whatever `compress` says: the reference
    got = Run(eng, interleave_rule.weave(text1, text2) if woven_in else text1, text2, n, woven_in=woven_in,
              woven_out=woven_out, mate2_first=mate2_first, compress=compress, **kw)
    routes = len(two.streams)
    assert len(got.streams) == routes
    for q in range(routes):
        is_fasta = fasta or q in fasta_classes
        if woven_out:
            want = [interleave_rule.weave(two.streams[q][0], two.streams[q][1], fasta=is_fasta, mate2_first=mate2_first), b""]
        else:
            want = list(two.streams[q])
        for m in range(2):
            data = got.streams[q][m]
            assert len(data) == int(got.sizes[q][m])
            if compress:  # each non-empty stream one gzip member, an empty one no bytes
                assert bool(data) == bool(want[m]), (q, m)
                if data:
                    assert data[:3] == b"\x1f\x8b\x08", (q, m)
                    assert gzip.decompress(data) == want[m], (mode, q, m)
            else:
                assert data == want[m], (mode, q, m)
            assert int(got.raw[q][m]) == len(want[m]), (q, m)
        if woven_out:
            assert int(got.sizes[q][1]) == 0 and int(got.raw[q][1]) == 0
            if q < 3:
                assert int(got.res.route_bytes[q][1]) == 0 and int(got.res.text_bytes[q][1]) == 0
                assert int(got.res.route_bytes[q][0]) == int(got.sizes[q][0])
    # counts: what the two-file run gives
    assert got.count == two.count and sum(got.count) + (sum(got.discards) if got.discards and routes == 3 else 0) == n
    assert [int(c) for c in got.res.route_count] == [int(c) for c in two.res.route_count]
    assert [int(b) for b in got.res.written_bp] == [int(b) for b in two.res.written_bp]
    assert got.discards == two.discards
    assert int(got.res.n_records) == n
    if woven_out:
        assert int(got.res.out_bytes[1]) == 0
        if not compress:
            assert int(got.res.out_bytes[0]) == int(two.res.out_bytes[0]) + int(two.res.out_bytes[1])
    elif not compress:
        assert [int(b) for b in got.res.out_bytes] == [int(b) for b in two.res.out_bytes]
    if woven_in:
        assert int(got.res.n_lines[1]) == 0 and int(got.res.n_lines[0]) in (8 * n, max(8 * n - 1, 0))
    return two


# ---- batches at the scan edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_batches_at_the_wave_and_scan_block_edges(mode):
    rec1, rec2 = fixture()
    with takara_engine() as eng:
        whole = Run(eng, text_of(rec1), text_of(rec2), len(rec1))
        assert whole.count[0] > 0 and whole.count[1] > 0  # (no inline barcode in TAKARAV3: route 2 is empty)
        for n in SIZES:
            two = _CACHE.get(("two", n))
            _CACHE[("two", n)] = check(eng, rec1[:n], rec2[:n], mode, two=two)
            if n in (1, 257, 513) and mode != "in":
                check(eng, rec1[:n], rec2[:n], mode, two=_CACHE[("two", n)], mate2_first=True)


@pytest.mark.parametrize("mode", list(MODES))
def test_all_three_routes_with_an_inline_barcode(mode):
    rec1, rec2 = inline_fixture()
    with inline_engine() as eng:
        for n in (257, 1000):
            two = check(eng, rec1[:n], rec2[:n], mode, two=_CACHE.get(("inline", n)))
            _CACHE[("inline", n)] = two
            assert all(c > 0 for c in two.count[:3]), two.count
        if mode != "in":
            check(eng, rec1[:257], rec2[:257], mode, two=_CACHE[("inline", 257)], mate2_first=True)


@pytest.mark.parametrize("mode", list(MODES))
def test_gzip_members_hold_both_mates(mode):
    rec1, rec2 = fixture()
    with takara_engine() as eng:
        for n in (1, 257, 1000):
            two = check(eng, rec1[:n], rec2[:n], mode, compress=True)
        # several 32 KB deflate chunks in the trimmed stream of the whole fixture
        assert len(two.streams[0][0]) + len(two.streams[0][1]) > 64 * 1024
        assert two.streams[2] == [b"", b""]  # ... and an empty route, which stays without bytes
        if mode != "in":
            check(eng, rec1[:257], rec2[:257], mode, compress=True, mate2_first=True)


def final_lengths(run):
    return [len(line) for q in (0, 2) for m in range(2) for line in run.streams[q][m].split(b"\n")[1::4]]


@pytest.mark.parametrize("mode", list(MODES))
def test_the_too_long_route_is_woven_too(mode):
    rec1, rec2 = fixture()
    n = 513
    rec1, rec2 = rec1[:n], rec2[:n]
    if "median" not in _CACHE:
        with takara_engine() as eng:
            _CACHE["median"] = int(statistics.median(final_lengths(Run(eng, text_of(rec1), text_of(rec2), n))))
    with takara_engine(max_length=_CACHE["median"]) as eng:
        two = check(eng, rec1, rec2, mode, too_long_route=True)
        assert len(two.streams) == 4 and two.count[3] > 0 and two.count[0] > 0
        assert two.discards == (two.count[3], 0, 0)
        check(eng, rec1, rec2, mode, too_long_route=True, compress=True)
        # the class-3 FASTA bits, for both mates: one stream has one format
        fa = Run(eng, text_of(rec1), text_of(rec2), n, too_long_route=True, fasta_routes=0xC0)
        assert fa.streams[3] == [as_fasta(two.streams[3][0]), as_fasta(two.streams[3][1])]
        check(eng, rec1, rec2, mode, two=fa, too_long_route=True, fasta_routes=0xC0, fasta_classes=(3,))


@pytest.mark.parametrize("mode", list(MODES))
def test_fasta_records_are_woven_by_twos(mode):
    rec1, rec2 = fixture()
    with takara_engine() as eng:
        two = check(eng, rec1[:257], rec2[:257], mode, fasta=True)
        assert two.streams[0][0].startswith(b">") and two.streams[0][0].count(b"\n") == 2 * two.count[0]


# ---- reads and texts of odd shapes -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["in", "in+out"])
def test_a_read_longer_than_the_rows_in_mate_2_is_found_in_the_shared_text(mode):
    import random
    rng = random.Random(3)
    rec1, rec2 = [list(r[:2]) for r in fixture()]
    long_seq = util.random_dna(rng, HUGE).encode()
    rec2[1] = (rec2[1][0], long_seq, bytes(rng.randint(40, 73) for _ in range(HUGE)))
    with takara_engine() as eng:
        two = check(eng, rec1, rec2, mode)
        assert int(two.res.n_long[1]) == 1 and int(two.res.max_len) == HUGE
        got = Run(eng, interleave_rule.weave(text_of(rec1), text_of(rec2)), None, 2, woven_in=True)
        assert int(got.res.n_long[1]) == 1 and int(got.res.n_long[0]) == 0 and int(got.res.max_len) == HUGE
        assert max(len(line) for line in b"".join(got.streams[0] + got.streams[1]).split(b"\n")) > 60000


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", ["crlf", "no-final-line-end", "empty-pair"])
def test_text_shapes(mode, shape):
    woven_in, woven_out = MODES[mode]
    rec1, rec2 = [list(r[:65]) for r in fixture()]
    if shape == "empty-pair":  # a pair whose reads are both empty, in the middle and at the very end
        for i in (7, 64):
            rec1[i], rec2[i] = (rec1[i][0], b"", b""), (rec2[i][0], b"", b"")
    text1, text2 = text_of(rec1), text_of(rec2)
    if shape == "crlf":
        text1, text2 = text1.replace(b"\n", b"\r\n"), text2.replace(b"\n", b"\r\n")
    if shape == "no-final-line-end":  # in the interleaved text this is mate 2's quality line
        text2 = text2[:-1]
    n = len(rec1)
    with takara_engine() as eng:
        two = Run(eng, text1, text2, n)
        woven = interleave_rule.weave(text1, text2)
        assert woven.endswith(text2[-20:]) and interleave_rule.deinterleave(woven) == (text1, text2)
        got = Run(eng, woven if woven_in else text1, text2, n, woven_in=woven_in, woven_out=woven_out)
        for q in range(3):
            want = [interleave_rule.weave(*two.streams[q]), b""] if woven_out else two.streams[q]
            assert got.streams[q] == want, (shape, q)
        assert got.count == two.count and sum(got.count) == n
        assert b"\r" not in b"".join(got.streams[0])


def test_errors_of_an_interleaved_text_name_the_pair():
    rec1, rec2 = [list(r[:600]) for r in fixture()]
    n = 600

    def error_of(text, pairs=n):
        with textpath.TextEngine(eng, slots=1, max_text_bytes=len(text) + 1024, max_records=n, stride=STRIDE,
                                 interleave_in=True) as te:
            te.submit(0, text, len(text), None, 0, pairs)
            with pytest.raises(textpath.TextFormatError) as exc:
                te.wait(0)
            return exc.value.code, exc.value.record

    with takara_engine() as eng:
        _errors(error_of, rec1, rec2)


def _errors(error_of, rec1, rec2):
    bad2 = list(rec2)
    for i in (3, 300):
        bad2[i] = (b"other" + bad2[i][0], bad2[i][1], bad2[i][2])
    assert error_of(interleave_rule.weave(text_of(rec1), text_of(bad2))) == (abi.CS_TEXT_ERR_IDS_DIFFER, 3)
    # mate 2's record of pair 299 without its '+' (the line is there: the line count holds)
    recs = interleave_rule._records(interleave_rule.weave(text_of(rec1), text_of(rec2)), 4)
    lines = recs[2 * 299 + 1].split(b"\n")
    assert lines[2] == b"+"
    lines[2] = b"-"
    broken = recs[:2 * 299 + 1] + [b"\n".join(lines)] + recs[2 * 299 + 2:]
    assert error_of(b"".join(broken)) == (abi.CS_TEXT_ERR_MALFORMED, 299)
    # ... and with the ids of pairs 3 and 300 differing as well, the smallest record wins
    recs2 = interleave_rule._records(interleave_rule.weave(text_of(rec1), text_of(bad2)), 4)
    assert error_of(b"".join(recs2[:2 * 299 + 1] + [b"\n".join(lines)] + recs2[2 * 299 + 2:])) == (abi.CS_TEXT_ERR_IDS_DIFFER, 3)
    # one record short
    assert error_of(b"".join(recs[:-1]))[0] == abi.CS_TEXT_ERR_LINE_COUNT


# ---- the C ABI ---------------------------------------------------------------------------------------------------

def raw_params(plan, **fields):
    p = abi.cs_text_params()
    p.has_umi = 1 if plan.has_umi else 0
    p.untrimmed_filter = 1 if plan.untrimmed_filter else 0
    p.max_tag = textpath.max_tag(plan)
    for key, value in fields.items():
        setattr(p, key, value)
    return p


def raw_create(eng, params, interleave, max_text_bytes=1 << 16, max_records=64):
    """-> (return code, handle) of cs_text_create_interleaved, or of cs_text_create for ``interleave`` None."""
    L = capi.load()
    h = C.c_void_p()
    if interleave is None:
        rc = L.cs_text_create(eng._eng_h, C.byref(params), 1, max_text_bytes, max_records, STRIDE, C.byref(h))
    else:
        rc = L.cs_text_create_interleaved(eng._eng_h, C.byref(params), interleave, 1, max_text_bytes, max_records, STRIDE,
                                          C.byref(h))
    return rc, h


REFUSALS = {
    "unknown bit": (8, {}),
    "unknown bit beside a known one": (abi.CS_INTERLEAVE_IN | 16, {}),
    "mate 2 first without an interleaved output": (abi.CS_INTERLEAVE_OUT_MATE2_FIRST, {}),
    "mate 2 first with an interleaved input alone": (abi.CS_INTERLEAVE_IN | abi.CS_INTERLEAVE_OUT_MATE2_FIRST, {}),
    "bins": (abi.CS_INTERLEAVE_OUT, {"n_bins": 4}),
    "bins with an interleaved input": (abi.CS_INTERLEAVE_IN, {"n_bins": 4}),
    "one class, two formats": (abi.CS_INTERLEAVE_OUT, {"fasta_routes": 0x01}),
    "one class, two formats (mate 2's bit)": (abi.CS_INTERLEAVE_IN | abi.CS_INTERLEAVE_OUT, {"fasta_routes": 0x08}),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refused_with_cs_err_arg(case):
    interleave, fields = REFUSALS[case]
    with takara_engine() as eng:
        rc, h = raw_create(eng, raw_params(eng.plan, **fields), interleave)
        assert rc == abi.CS_ERR_ARG and not h.value, case
        if "fasta_routes" in fields:  # (the same bits are fine where every mate has a stream of its own)
            rc, h = raw_create(eng, raw_params(eng.plan, **fields), abi.CS_INTERLEAVE_IN)
            assert rc == 0
            capi.load().cs_text_destroy(h)


@pytest.mark.parametrize("bits", [abi.CS_INTERLEAVE_IN, abi.CS_INTERLEAVE_OUT, abi.CS_INTERLEAVE_IN | abi.CS_INTERLEAVE_OUT])
def test_refused_on_a_single_end_plan(bits):
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], planmod.CutadaptConfig(), False)
    with TrimEngine(tp, device=0, slots=0) as eng:
        rc, h = raw_create(eng, raw_params(tp), bits)
        assert rc == abi.CS_ERR_ARG and not h.value
        assert b"single-end" in capi.load().cs_last_error()


def test_a_woven_buffer_of_a_gibibyte_is_refused():
    """600 MiB per mate is inside cs_text_create's bound; their sum in one buffer is not (offsets keep 30 bits).  With an
    interleaved input the same bytes bound the ONE text, and the output with it."""
    big = 600 << 20
    with takara_engine() as eng:
        rc, h = raw_create(eng, raw_params(eng.plan), abi.CS_INTERLEAVE_OUT, max_text_bytes=big)
        assert rc == abi.CS_ERR_ARG and not h.value and b"1 GiB" in capi.load().cs_last_error()
        rc, h = raw_create(eng, raw_params(eng.plan), abi.CS_INTERLEAVE_IN | abi.CS_INTERLEAVE_OUT, max_text_bytes=1 << 30)
        assert rc == abi.CS_ERR_ARG and not h.value


def test_without_the_bits_it_is_cs_text_create():
    rec1, rec2 = [r[:257] for r in fixture()]
    text1, text2 = text_of(rec1), text_of(rec2)
    L = capi.load()
    outs = []
    with takara_engine() as eng:
        for interleave in (None, 0):
            rc, h = raw_create(eng, raw_params(eng.plan), interleave, max_text_bytes=len(text1) + len(text2), max_records=257)
            assert rc == 0
            try:
                capi.check(L.cs_text_submit(h, 0, textpath._address(text1), len(text1), textpath._address(text2), len(text2), 257))
                res = abi.cs_text_result()
                capi.check(L.cs_text_wait(h, 0, C.byref(res)))
                out = [np.empty(int(res.out_bytes[m]), dtype=np.uint8) for m in range(2)]
                capi.check(L.cs_text_fetch(h, 0, out[0].ctypes.data, out[1].ctypes.data))
                outs.append((bytes(res), out[0].tobytes(), out[1].tobytes()))
            finally:
                L.cs_text_destroy(h)
    assert outs[0] == outs[1] and outs[0][1] and outs[0][2]
