"""--max-n (cutadapt's TooManyN) on the CPU side: CLI, C ABI declaration, the rule, the host chunk formatter's
precedence (TooShort > TooManyN > IsUntrimmedAny > sink) and the two reports."""
import ctypes as C
import math
import re
import tempfile
from pathlib import Path

import numpy as np
import pytest

from cutseq_amd import abi, capi, fastq, plan as planmod, report, run
from cutseq_amd.common import BUILDIN_ADAPTERS

import maxn_rule

ROOT = Path(__file__).resolve().parents[1]


def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


def test_cli_accepts_max_n_and_passes_it_on():
    args = run.resolve_args(_args("--max-n", "0.1"))
    assert args.max_n == 0.1
    st = run.settings_from_args(args)
    assert st.max_n == 0.1
    assert planmod.compile_paired(planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), st).max_n == 0.1
    assert run.settings_from_args(run.resolve_args(_args())).max_n is None
    assert "--max-n" in run.build_parser().format_help()


@pytest.mark.parametrize("bad", ["-1", "-0.5", "nan"])
def test_cli_rejects_negative_and_nan(bad, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args(f"--max-n={bad}"))
    assert exc.value.code == 1  # the CLI's own check (_fail), not argparse's usage error (2)
    assert "--max-n: the count must not be negative" in caplog.text


def test_entry_point_is_declared_and_exported():
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"int cs_plan_set_max_n\(cs_plan \*plan, double count\);", header)
    assert "cs_plan_set_max_n" in capi.EXPORTS
    assert abi.CS_ABI_VERSION == 7 and abi.CS_X_TOO_MANY_N == 1
    assert "n_too_many_n" in dict(abi.cs_stats._fields_) and "xflags" in dict(abi.cs_reads._fields_)
    assert "n_too_many_n" in dict(abi.cs_text_result._fields_) and C.sizeof(abi.cs_text_result) == 176


def test_entry_point_rejects_bad_counts():
    from cutseq_amd import build
    build.build()
    L = capi.load()
    tp = planmod.single_adapter_plan("AGATCGGAAGAGC")
    a1, n1, _a2, _n2 = tp.pack()
    params = tp.params()
    h = C.c_void_p()
    capi.check(L.cs_plan_create(C.cast(a1, C.c_void_p), n1, None, 0, C.byref(params), C.byref(h)))
    try:
        for bad in (-1.0, -1e-300, math.nan):
            assert L.cs_plan_set_max_n(h, bad) == abi.CS_ERR_ARG
        for good in (0.0, 0.1, 1.0, 2.5, math.inf):
            assert L.cs_plan_set_max_n(h, good) == abi.CS_OK
        assert L.cs_plan_set_max_n(None, 0.0) == abi.CS_ERR_ARG
    finally:
        L.cs_plan_destroy(h)


@pytest.mark.parametrize("seq, count, want", [
    (b"", 0, False), (b"", 0.1, False), (b"", 1, False),
    (b"ACGT", 0, False), (b"ACGN", 0, True), (b"ACGn", 0, True),
    (b"N" * 10, 0.1, True), (b"N" + b"A" * 9, 0.1, False), (b"NN" + b"A" * 8, 0.1, True),
    (b"NAA", 1 / 3, False), (b"NNA", 1 / 3, True), (b"nNA", 1 / 3, True),
    (b"NNNAAAAAAA", 0.7, False), (b"NNNNNNNNAA", 0.7, True),
    (b"NA", 1, False), (b"NN", 1, True), (b"nN", 1, True),
    (b"NNA", 2.5, False), (b"NNN", 2.5, True),
    (b"N" * 100, math.inf, False),
])
def test_rule_hand_table(seq, count, want):
    assert maxn_rule.too_many_n(seq, count) is want


def _chunk(d, paired, n):
    recs = [(f"r{i}".encode(), b"ACGTN" * 8, b"I" * 40) for i in range(n)]
    for mate in (1, 2) if paired else (1,):
        Path(d, f"{mate}.fq").write_bytes(b"".join(b"@" + nm + b"/%d\n" % mate + s + b"\n+\n" + q + b"\n"
                                                   for nm, s, q in recs))
    (c,) = list(fastq.read_chunks(str(Path(d, "1.fq")), str(Path(d, "2.fq")) if paired else None))
    return c


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("bins", [False, True])
def test_host_formatter_precedence(paired, bins):
    """Hand-made results and xflags: every combination of short / N / untrimmed on either mate."""
    st = planmod.CutadaptConfig()
    tp = planmod.compile_paired(planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), st) if paired else \
        planmod.compile_single(planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), st)
    tp.untrimmed_filter = True
    combos = [(a, b, c, d) for a in range(8) for b in range(8) for c in (0, 1) for d in (0, 1)]
    n = len(combos)
    with tempfile.TemporaryDirectory() as d:
        c = _chunk(d, paired, n)
    res1 = np.zeros(n, dtype=abi.RESULT_DTYPE)
    res2 = np.zeros(n, dtype=abi.RESULT_DTYPE)
    xf1, xf2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    bits = (0, abi.CS_F_TOO_SHORT, abi.CS_F_UNTRIMMED)
    for i, (f1, f2, x1, x2) in enumerate(combos):
        res1[i] = (1, 30, 0, 0, (bits[1] if f1 & 1 else 0) | (bits[2] if f1 & 2 else 0))
        res2[i] = (2, 31, 0, 0, (bits[1] if f2 & 1 else 0) | (bits[2] if f2 & 2 else 0))
        xf1[i], xf2[i] = x1, x2
    if not paired:
        res2 = None
    want = [maxn_rule.route(int(res1[i]["flags"]), int(res2[i]["flags"]) if paired else 0, int(xf1[i]),
                            int(xf2[i]) if paired else 0, True) for i in range(n)]
    if bins:
        bc = np.zeros(n, dtype=np.uint8)  # every pair carries barcode 0
        _data, counts = fastq.format_chunk(c, tp, res1, None, res2, xflags=(xf1, xf2 if paired else None), n_bins=1,
                                           bc=bc)
        assert counts[3] == want.count(0)
        assert counts[1] == want.count(1) and counts[2] == want.count(2)
    else:
        data, counts = fastq.format_chunk(c, tp, res1, None, res2, xflags=(xf1, xf2 if paired else None))
        assert counts == [want.count(0), want.count(1), want.count(2)]
        # the records of a route are the pairs of that route, in input order (name r<i>)
        for r in range(3):
            names = re.findall(rb"^@(r\d+)", data[r][0], re.M)
            assert names == [f"r{i}".encode() for i in range(n) if want[i] == r]
            if paired:
                assert re.findall(rb"^@(r\d+)", data[r][1], re.M) == names
        # without xflags nothing is discarded
        _data, counts0 = fastq.format_chunk(c, tp, res1, None, res2)
        assert sum(counts0) == n
    assert n - sum(counts) == want.count(None)
    # the run totals count the same pairs
    part = report.new_totals()
    lens = np.full(n, 40, dtype=np.uint16)
    report.account_chunk(part, tp, lens, res1, lens if paired else None, res2, xflags=(xf1, xf2 if paired else None))
    assert part["too_many_n"] == want.count(None)


def _totals(too_many_n):
    t = report.new_totals()
    t.update(in_pairs=10, routes=[5, 2, 1], in_bp=[1000, 1000], written_bp=[400, 400], too_many_n=too_many_n,
             stats=[[abi.cs_stats().as_dict(), abi.cs_stats().as_dict()]])
    return t


@pytest.mark.parametrize("max_n", [None, 0.0, 2.0])
def test_reports(max_n):
    st = planmod.CutadaptConfig()
    st.max_n = max_n
    tp = planmod.compile_paired(planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), st)
    t = _totals(2 if max_n is not None else 0)
    head, vals = report.minimal_report(tp, t).split("\n")
    col = head.split("\t").index("too_many_n")
    assert vals.split("\t")[col] == ("2" if max_n is not None else "0")
    d = report.json_report(tp, t, planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), "a", "b", "c", "d", "e", "f",
                           None, None)
    assert d["read_counts"]["filtered"]["too_many_n"] == (2 if max_n is not None else None)
    assert d["read_counts"]["output"] == 5


def test_totals_merge_sums_too_many_n():
    a, b = report.new_totals(), report.new_totals()
    a["too_many_n"], b["too_many_n"] = 3, 4
    report.merge_totals(a, b)
    assert a["too_many_n"] == 7
