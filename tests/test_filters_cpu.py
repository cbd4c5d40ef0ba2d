"""-M/--max-length (TooLong) and --max-ee (TooManyExpectedErrors) on the CPU side: CLI, C ABI declarations, the rules,
the host chunk formatter's precedence (TooShort > TooLong > TooManyN > TooManyExpectedErrors > IsUntrimmedAny > sink),
the two reports and the totals that travel between ranks."""
import ctypes as C
import json
import math
import re
import tempfile
from pathlib import Path

import numpy as np
import pytest

from cutseq_amd import abi, capi, fastq, plan as planmod, ranks, report, run
from cutseq_amd.common import BUILDIN_ADAPTERS

import filters_rule

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])


def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


# ---- the command line ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv, length, ee", [
    (["-M", "30"], 30, None), (["--max-length", "0"], 0, None), (["--max-ee", "1.5"], None, 1.5),
    (["--max-expected-errors", "0"], None, 0.0), (["-M", "70000", "--max-ee", "inf"], 70000, math.inf), ([], None, None),
])
def test_cli_accepts_the_options_and_passes_them_on(argv, length, ee):
    args = run.resolve_args(_args(*argv))
    assert args.max_length == length and args.max_ee == ee
    st = run.settings_from_args(args)
    assert st.max_length == length and st.max_ee == ee and st.max_n is None
    for tp in (planmod.compile_paired(TAKARA, st), planmod.compile_single(TAKARA, st)):
        assert tp.max_length == length and tp.max_ee == ee
        assert tp.has_filters is bool(argv)


def test_cli_help_names_the_options():
    text = run.build_parser().format_help()
    assert "--max-length" in text and "-M LEN" in text and "--max-ee" in text


@pytest.mark.parametrize("bad, message", [
    ("-M=-1", "-M/--max-length: the length must not be negative"),
    ("--max-ee=-1", "--max-ee: the number of expected errors must not be negative"),
    ("--max-ee=-0.5", "--max-ee: the number of expected errors must not be negative"),
    ("--max-ee=nan", "--max-ee: the number of expected errors must not be negative"),
])
def test_cli_rejects_negative_and_nan(bad, message, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args(bad))
    assert exc.value.code == 1  # the CLI's own check (_fail), not argparse's usage error (2)
    assert message in caplog.text


@pytest.mark.parametrize("first", [b">", b"#"])
def test_max_ee_refuses_fasta_input(tmp_path, caplog, first):
    fa = tmp_path / "reads.fa"
    fa.write_bytes((b"# a comment\n" if first == b"#" else b"") + b">r1\nACGTACGTACGTACGTACGTACGT\n")
    with pytest.raises(SystemExit) as exc:
        run.main([str(fa), "-A", "TAKARAV3", "--max-ee", "1", "-o", str(tmp_path / "out.fa")])
    assert exc.value.code == 1
    assert "--max-ee needs qualities" in caplog.text and "reads.fa" in caplog.text


def test_dry_run_is_unchanged(capsys):
    outs = []
    for extra in ([], ["-M", "40"], ["--max-ee", "2"], ["-M", "40", "--max-ee", "2", "--max-n", "0"]):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", "r2.fq.gz", *extra])
        outs.append(capsys.readouterr().out)
    assert outs[0] and outs[1] == outs[0] and outs[2] == outs[0] and outs[3] == outs[0]


# ---- the C ABI -------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_exported():
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"int cs_plan_set_max_length\(cs_plan \*plan, uint32_t length\);", header)
    assert re.search(r"int cs_plan_set_max_ee\(cs_plan \*plan, double errors\);", header)
    assert re.search(r"int cs_xflag_counts_fetch\(cs_engine \*eng, uint64_t counts\[2\]\[CS_X_COUNTS\], int reset\);", header)
    assert re.search(r"int cs_text_discards\(cs_text \*t, uint32_t slot, uint32_t pairs\[3\]\);", header)
    assert re.search(r"CS_X_TOO_LONG = 0x02", header) and re.search(r"CS_X_TOO_MANY_EE = 0x04", header)
    for name in ("cs_plan_set_max_length", "cs_plan_set_max_ee", "cs_xflag_counts_fetch", "cs_text_discards"):
        assert name in capi.EXPORTS
    assert (abi.CS_X_TOO_MANY_N, abi.CS_X_TOO_LONG, abi.CS_X_TOO_MANY_EE, abi.CS_X_COUNTS) == (1, 2, 4, 3)


def test_pinned_abi_is_unchanged():
    assert abi.CS_ABI_VERSION == 7
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"#define CS_ABI_VERSION 7\b", header)
    assert C.sizeof(abi.cs_text_result) == 176 and C.sizeof(abi.cs_text_params) == 48
    assert C.sizeof(abi.cs_stats) == 8 * (8 + abi.CS_MAX_OPS + 1)


def test_library_exports_the_calls_and_checks_their_arguments():
    from cutseq_amd import build
    build.build()
    L = capi.load()  # (raises when an entry of capi.EXPORTS is missing)
    tp = planmod.single_adapter_plan("AGATCGGAAGAGC")
    a1, n1, _a2, _n2 = tp.pack()
    params = tp.params()
    h = C.c_void_p()
    capi.check(L.cs_plan_create(C.cast(a1, C.c_void_p), n1, None, 0, C.byref(params), C.byref(h)))
    try:
        for bad in (-1.0, -1e-300, math.nan):
            assert L.cs_plan_set_max_ee(h, bad) == abi.CS_ERR_ARG
        for good in (0.0, 0.1, 1.0, 2.5, math.inf):
            assert L.cs_plan_set_max_ee(h, good) == abi.CS_OK
        for good in (0, 1, 65535, 70000, 0xFFFFFFFF):
            assert L.cs_plan_set_max_length(h, good) == abi.CS_OK
        assert L.cs_plan_set_max_ee(None, 0.0) == abi.CS_ERR_ARG
        assert L.cs_plan_set_max_length(None, 0) == abi.CS_ERR_ARG
    finally:
        L.cs_plan_destroy(h)
    counts = ((C.c_uint64 * 3) * 2)()
    assert L.cs_xflag_counts_fetch(None, C.byref(counts), 0) == abi.CS_ERR_ARG
    pairs = (C.c_uint32 * 3)()
    assert L.cs_text_discards(None, 0, C.byref(pairs)) == abi.CS_ERR_ARG


# ---- the rules -------------------------------------------------------------------------------------------------

def test_expected_errors_table_and_sum():
    assert filters_rule.EE_TABLE[33] == 1.0 and filters_rule.EE_TABLE[43] == 0.1 and filters_rule.EE_TABLE[53] == 0.01
    assert filters_rule.EE_TABLE[0] == 10 ** 3.3 and len(filters_rule.EE_TABLE) == 256
    assert filters_rule.expected_errors(b"") == 0.0
    assert filters_rule.expected_errors(b"!!!") == 3.0
    # the order of the adds is part of the rule: the same bytes the other way round give another double
    qual = bytes([126, 33, 40, 75, 34, 90, 61, 33, 50, 47] * 12)
    assert filters_rule.expected_errors(qual) != filters_rule.expected_errors(qual[::-1])


@pytest.mark.parametrize("qual, bound, want", [
    (b"", 0.0, False), (b"~", 0.0, True), (b"+", 0.1, False), (b"++", 0.1, True), (b"!", 1.0, False), (b"!!", 1.0, True),
    (b"!" * 500, math.inf, False),
])
def test_too_many_ee_hand_table(qual, bound, want):
    assert filters_rule.too_many_ee(qual, bound) is want


@pytest.mark.parametrize("length, bound, want", [(0, 0, False), (1, 0, True), (30, 30, False), (31, 30, True),
                                                 (65535, 65535, False), (65535, 70000, False)])
def test_too_long_hand_table(length, bound, want):
    assert filters_rule.too_long(length, bound) is want


# ---- the host formatter and the run totals ---------------------------------------------------------------------

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
    """Hand-made results and xflags: short / untrimmed on either mate times every combination of the three bits on
    either mate."""
    st = planmod.CutadaptConfig()
    tp = planmod.compile_paired(TAKARA, st) if paired else planmod.compile_single(TAKARA, st)
    tp.untrimmed_filter = True
    mates2 = range(8) if paired else (0,)
    combos = [(f1, f2, x1, x2) for f1 in range(4) for f2 in (range(4) if paired else (0,)) for x1 in range(8) for x2 in mates2]
    n = len(combos)
    with tempfile.TemporaryDirectory() as d:
        c = _chunk(d, paired, n)
    res1 = np.zeros(n, dtype=abi.RESULT_DTYPE)
    res2 = np.zeros(n, dtype=abi.RESULT_DTYPE)
    xf1, xf2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for i, (f1, f2, x1, x2) in enumerate(combos):
        res1[i] = (1, 30, 0, 0, (abi.CS_F_TOO_SHORT if f1 & 1 else 0) | (abi.CS_F_UNTRIMMED if f1 & 2 else 0))
        res2[i] = (2, 31, 0, 0, (abi.CS_F_TOO_SHORT if f2 & 1 else 0) | (abi.CS_F_UNTRIMMED if f2 & 2 else 0))
        xf1[i], xf2[i] = x1, x2
    if not paired:
        res2 = None
    want = [filters_rule.route(int(res1[i]["flags"]), int(res2[i]["flags"]) if paired else 0, int(xf1[i]),
                               int(xf2[i]) if paired else 0, True) for i in range(n)]
    # what the test claims to cover occurs: every bit combination discarded, TooShort over each of them, every filter
    # the first to catch a pair that a later one catches too, and pairs that are kept
    names = [name for name, _bit in filters_rule.ORDER]
    for x in range(1, 8):
        hits = [i for i in range(n) if (int(xf1[i]) | (int(xf2[i]) if paired else 0)) == x]
        assert any(want[i] in names for i in hits) and any(want[i] == 1 for i in hits), x
        first = next(name for name, bit in filters_rule.ORDER if x & bit)
        assert all(want[i] in (1, first) for i in hits), x
    assert all(want.count(k) > 0 for k in (0, 1, 2, *names))
    xflags = (xf1, xf2 if paired else None)
    if bins:
        bc = np.zeros(n, dtype=np.uint8)  # every pair carries barcode 0
        _data, counts = fastq.format_chunk(c, tp, res1, None, res2, xflags=xflags, n_bins=1, bc=bc)
        assert counts[3] == want.count(0)
        assert counts[1] == want.count(1) and counts[2] == want.count(2)
        written = counts[3] + counts[1] + counts[2]
    else:
        data, counts = fastq.format_chunk(c, tp, res1, None, res2, xflags=xflags)
        assert counts == [want.count(0), want.count(1), want.count(2)]
        for r in range(3):  # the records of a route are the pairs of that route, in input order (name r<i>)
            got = re.findall(rb"^@(r\d+)", data[r][0], re.M)
            assert got == [f"r{i}".encode() for i in range(n) if want[i] == r]
            if paired:
                assert re.findall(rb"^@(r\d+)", data[r][1], re.M) == got
        written = sum(counts)
    assert n - written == sum(want.count(k) for k in names)
    # the run totals count every discarded pair once, under the first filter that caught it
    part = report.new_totals()
    lens = np.full(n, 40, dtype=np.uint16)
    report.account_chunk(part, tp, lens, res1, lens if paired else None, res2, xflags=xflags)
    for k in names:
        assert part[k] == want.count(k), k
    kept = [i for i in range(n) if want[i] == 0]
    assert part["written_bp"][0] == 29 * len(kept) and part["in_pairs"] == n


def _totals(**kw):
    t = report.new_totals()
    t.update(in_pairs=20, routes=[5, 2, 1], in_bp=[1000, 1000], written_bp=[400, 400],
             stats=[[abi.cs_stats().as_dict(), abi.cs_stats().as_dict()]])
    t.update(kw)
    return t


@pytest.mark.parametrize("max_length, max_ee", [(None, None), (40, None), (None, 1.5), (0, 0.0)])
def test_reports(max_length, max_ee):
    st = planmod.CutadaptConfig()
    st.max_length, st.max_ee = max_length, max_ee
    tp = planmod.compile_paired(TAKARA, st)
    t = _totals(too_long=3 if max_length is not None else 0, too_many_ee=4 if max_ee is not None else 0)
    head, vals = report.minimal_report(tp, t).split("\n")
    col = head.split("\t").index("too_long")
    assert vals.split("\t")[col] == ("3" if max_length is not None else "0")
    assert len(head.split("\t")) == len(vals.split("\t")) == 13  # no new column
    d = report.json_report(tp, t, TAKARA, "a", "b", "c", "d", "e", "f", None, None)
    filtered = d["read_counts"]["filtered"]
    assert filtered["too_long"] == (3 if max_length is not None else None)
    assert filtered["too_many_expected_errors"] == (4 if max_ee is not None else None)
    assert filtered["too_many_n"] is None and filtered["casava_filtered"] is None
    assert set(filtered) == set(report.FILTER_KEYS)
    assert d["read_counts"]["output"] == 5


def test_totals_merge_and_rank_files_carry_the_counts(tmp_path):
    a, b = report.new_totals(), report.new_totals()
    a.update(too_long=3, too_many_ee=5, too_many_n=1)
    b.update(too_long=4, too_many_ee=6, too_many_n=2)
    report.merge_totals(a, b)
    assert (a["too_long"], a["too_many_ee"], a["too_many_n"]) == (7, 11, 3)
    old = {k: v for k, v in report.new_totals().items() if k not in ("too_long", "too_many_ee")}
    report.merge_totals(a, old)  # (totals without the keys add nothing)
    assert (a["too_long"], a["too_many_ee"]) == (7, 11)
    a.update(stats=[], devices=[0])
    ranks.dump_totals({"totals_file": str(tmp_path / "t.json")}, a)
    back = json.loads((tmp_path / "t.json").read_text())
    assert back["too_long"] == 7 and back["too_many_ee"] == 11 and back["too_many_n"] == 3
