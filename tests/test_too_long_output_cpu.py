"""--too-long-output on the CPU side: the command line, the output files' groups and formats, the C ABI declarations,
the host chunk formatter's fourth stream (the hand table of test_filters_cpu.py), the JSON report's keys and the totals
that travel between ranks."""
import ctypes as C
import json
import re
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from cutseq_amd import abi, capi, fastq, plan as planmod, ranks, report, run, textio
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.outputs import OutputLayout

import filters_rule
import toolong_rule
from test_filters_cpu import _chunk, _totals

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])


def _args(*extra, inputs=("r1.fq.gz", "r2.fq.gz")):
    return run.build_parser().parse_args(["-A", "TAKARAV3", *inputs, *extra])


# ---- the command line ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inputs, names", [(("r1.fq.gz",), ["long.fq.gz"]), (("r1.fq.gz", "r2.fq.gz"), ["l1.fq.gz", "l2.fq"])])
def test_cli_accepts_one_name_per_input(inputs, names):
    args = run.resolve_args(_args("-M", "30", "--too-long-output", *names, inputs=inputs))
    assert args.too_long_file == names and args.max_length == 30
    # the three default file classes stay three, and there is no default name from -O
    assert [len(getattr(args, attr)) for attr, _word in run.OUTPUT_CLASSES] == [len(inputs)] * 3
    plain = run.resolve_args(_args("-M", "30", "-O", "pre", inputs=inputs))
    assert not plain.too_long_file


def test_cli_help_names_the_option():
    text = run.build_parser().format_help()
    assert "--too-long-output FILE [FILE ...]" in text


@pytest.mark.parametrize("argv, message", [
    (["--too-long-output", "a.fq", "b.fq"], "--too-long-output needs -M/--max-length"),
    (["-M", "30", "--too-long-output", "a.fq"], "Number of too-long output files (1) must match number of input files (2)."),
    (["-M", "30", "--too-long-output", "a.fq", "b.fq", "c.fq"], "Number of too-long output files (3) must match"),
    (["-M", "30", "--too-long-output", "a.fq", "b.fq", "--demux-barcodes", "codes.tsv"],
     "--too-long-output cannot be combined with --demux-barcodes"),
])
def test_cli_refuses(argv, message, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args(*argv))
    assert exc.value.code == 1  # the CLI's own check (_fail), not argparse's usage error (2)
    assert message in caplog.text


def test_fastq_named_file_for_fasta_input_is_refused():
    groups = [["t1.fa", "t2.fa"], ["s1.fa", "s2.fa"], [None, None], ["long1.fa", "long2.fastq.gz"]]
    with pytest.raises(fastq.FastqFormatError) as exc:
        textio.output_formats(groups, has_qualities=False)
    assert "long2.fastq.gz" in str(exc.value)
    groups[3][1] = "long2.fa"
    assert textio.output_formats(groups, has_qualities=False) == 0xFF


def test_dry_run_and_list_adapters_are_unchanged(capsys):
    outs = []
    for extra in ([], ["-M", "40"], ["-M", "40", "--too-long-output", "a.fq", "b.fq"]):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", "r2.fq.gz", *extra])
        outs.append(capsys.readouterr().out)
    assert outs[0] and outs[1] == outs[0] and outs[2] == outs[0]
    lists = []
    for extra in ([], ["-M", "40", "--too-long-output", "a.fq"]):
        with pytest.raises(SystemExit):
            run.main(["--list-adapters", *extra])
        lists.append(capsys.readouterr().out)
    assert lists[0] and lists[1] == lists[0]


# ---- the output files' groups and formats ----------------------------------------------------------------------

def _names(paired=True, **kw):
    mates = 2 if paired else 1
    base = dict(output_file=["t1.fq", "t2.fq"][:mates], short_file=["s1.fq", "s2.fq"][:mates],
                untrimmed_file=[None, None][:mates], too_long_file=None)
    base.update(kw)
    layout = OutputLayout.of(base["output_file"], base["short_file"], base["untrimmed_file"], base["too_long_file"], paired=paired)
    return SimpleNamespace(outputs=layout)


def test_output_name_groups_gain_a_fourth_group_that_is_never_swapped():
    args = _names(too_long_file=["l1.fa", "l2.fq"])
    assert textio.output_name_groups(args, True, False, 0) == [["t1.fq", "t2.fq"], ["s1.fq", "s2.fq"], [None, None], ["l1.fa", "l2.fq"]]
    # paired --auto-rc on a '-' library: only the trimmed pair's files change places
    assert textio.output_name_groups(args, True, True, 0) == [["t2.fq", "t1.fq"], ["s1.fq", "s2.fq"], [None, None], ["l1.fa", "l2.fq"]]
    assert textio.output_name_groups(_names(False, too_long_file=["l.fq"]), False, False, 0)[3] == ["l.fq"]
    # without the option: three groups, as ever
    assert len(textio.output_name_groups(_names(), True, False, 0)) == 3
    assert len(textio.output_name_groups(_names(), True, True, 0)) == 3


def test_output_formats_class_3_bits_go_by_the_files_own_names():
    groups = textio.output_name_groups(_names(too_long_file=["l1.fa", "l2.fq"]), True, False, 0)
    assert textio.output_formats(groups, has_qualities=True) == 1 << 6          # class 3, mate 1
    groups = textio.output_name_groups(_names(too_long_file=["l1.fq.gz", "l2.fasta.gz"]), True, False, 0)
    assert textio.output_formats(groups, has_qualities=True) == 1 << 7          # class 3, mate 2
    groups = textio.output_name_groups(_names(too_long_file=["l1.fa", "l2.fa"]), True, False, 0)
    assert textio.output_formats(groups, has_qualities=True) == 0xC0
    groups = textio.output_name_groups(_names(False, too_long_file=["l.fa"]), False, False, 0)
    assert textio.output_formats(groups, has_qualities=True) == 1 << 6
    # a name that says nothing follows the input
    groups = textio.output_name_groups(_names(too_long_file=["l1.txt", "l2.txt"]), True, False, 0)
    assert textio.output_formats(groups, has_qualities=True) == 0


# ---- the C ABI -------------------------------------------------------------------------------------------------

def test_abi_carries_the_member_in_the_reserved_byte():
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"uint8_t too_long_route;", header) and "_reserved[1]" not in header
    assert re.search(r"#define CS_ABI_VERSION 7\b", header) and abi.CS_ABI_VERSION == 7
    assert C.sizeof(abi.cs_text_params) == 48 and C.sizeof(abi.cs_text_result) == 176
    assert abi.cs_text_params.too_long_route.offset == 47 and abi.cs_text_params.too_long_route.size == 1
    assert abi.cs_text_params.info.offset == 46
    assert abi.cs_text_params().too_long_route == 0
    # the header says what cs_text_discards means now that the pairs are written
    assert re.search(r"pairs\[0\] keeps counting them", header) and "count[3] of cs_text_routes" in header


def test_library_refuses_what_it_can_without_a_gpu():
    from cutseq_amd import build
    build.build()
    L = capi.load()
    p = abi.cs_text_params()
    p.too_long_route = 1
    h = C.c_void_p()
    assert L.cs_text_create(None, C.byref(p), 1, 1 << 20, 1024, 152, C.byref(h)) == abi.CS_ERR_ARG
    assert not h.value
    sizes = (C.c_uint64 * 8)()
    assert L.cs_text_routes(None, 0, sizes, sizes, None) == abi.CS_ERR_ARG
    pairs = (C.c_uint32 * 3)()
    assert L.cs_text_discards(None, 0, C.byref(pairs)) == abi.CS_ERR_ARG
    # -M is what the route needs: the plan call that switches it on takes every 32-bit length
    tp = planmod.single_adapter_plan("AGATCGGAAGAGC")
    a1, n1, _a2, _n2 = tp.pack()
    params = tp.params()
    plan = C.c_void_p()
    capi.check(L.cs_plan_create(C.cast(a1, C.c_void_p), n1, None, 0, C.byref(params), C.byref(plan)))
    try:
        assert L.cs_plan_set_max_length(plan, 0) == abi.CS_OK and L.cs_plan_set_max_length(plan, 0xFFFFFFFF) == abi.CS_OK
    finally:
        L.cs_plan_destroy(plan)


def test_host_formatter_structs_match_the_library():
    fastq._lib()  # (raises when the ctypes mirrors and the library's structs differ in size)
    assert fastq._FormatParams.too_long_route.offset == 18 and C.sizeof(fastq._FormatParams) == 56
    assert C.sizeof(fastq._FormatOut) == 8 * (8 + 8 + 4 + 2 + 2)


# ---- the host formatter ----------------------------------------------------------------------------------------

def _hand_table(paired):
    """test_filters_cpu.test_host_formatter_precedence's table: every flag x xflag combination on either mate."""
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
    want = [toolong_rule.route(int(res1[i]["flags"]), int(res2[i]["flags"]) if paired else 0, int(xf1[i]),
                               int(xf2[i]) if paired else 0, True) for i in range(n)]
    return tp, c, res1, res2, (xf1, xf2 if paired else None), want


@pytest.mark.parametrize("paired", [False, True])
def test_host_formatter_fourth_stream(paired):
    tp, c, res1, res2, xflags, want = _hand_table(paired)
    n = len(want)
    # the rule sends pairs to every stream and to both discarding filters that are left; TooLong wins over the other two
    assert all(want.count(k) > 0 for k in (0, 1, 2, 3, "too_many_n", "too_many_ee")) and "too_long" not in want
    pair_x = [int(xflags[0][i]) | (int(xflags[1][i]) if paired else 0) for i in range(n)]
    for x in (3, 6, 7):  # TooLong together with the others: stream 3 unless TooShort took the pair
        assert {want[i] for i in range(n) if pair_x[i] == x} == {1, 3}, x
    off, counts_off = fastq.format_chunk(c, tp, res1, None, res2, xflags=xflags)
    data, counts = fastq.format_chunk(c, tp, res1, None, res2, xflags=xflags, too_long_route=True)
    assert len(data) == 4 and len(counts) == 4 and len(off) == 3 and len(counts_off) == 3
    assert counts == [want.count(0), want.count(1), want.count(2), want.count(3)]
    for r in range(4):  # the records of a stream are the pairs of that route, in input order (name r<i>), both mates
        got = re.findall(rb"^@(r\d+)", data[r][0], re.M)
        assert got == [f"r{i}".encode() for i in range(n) if want[i] == r], r
        if paired:
            assert re.findall(rb"^@(r\d+)", data[r][1], re.M) == got, r
    # written as trimmed: the interval [1, 30) of mate 1, [2, 31) of mate 2
    first = data[3][0].split(b"\n")[:4]
    assert first[1] == (b"ACGTN" * 8)[1:30] and first[3] == b"I" * 29
    if paired:
        assert data[3][1].split(b"\n")[1] == (b"ACGTN" * 8)[2:31]
    # streams 0 .. 2 are what they are with the option off
    assert data[:3] == off and counts[:3] == counts_off
    assert n - sum(counts_off) == counts[3] + want.count("too_many_n") + want.count("too_many_ee")
    # ... and so is every count of the run totals: too_long keeps counting the pairs TooLong caught
    part = report.new_totals()
    lens = np.full(n, 40, dtype=np.uint16)
    report.account_chunk(part, tp, lens, res1, lens if paired else None, res2, xflags=xflags)
    assert part["too_long"] == counts[3]
    assert part["too_many_n"] == want.count("too_many_n") and part["too_many_ee"] == want.count("too_many_ee")
    assert part["written_bp"][0] == 29 * want.count(0) and part["in_pairs"] == n


def test_host_formatter_turns_the_too_long_records_round_single_end():
    tp, c, res1, _res2, xflags, want = _hand_table(False)
    tp.reverse_complement = True
    data, counts = fastq.format_chunk(c, tp, res1, None, None, xflags=xflags, too_long_route=True)
    assert counts[3] == want.count(3) > 0
    rec = data[3][0].split(b"\n")[:4]
    kept = (b"ACGTN" * 8)[1:30]
    assert rec[1] == kept[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")) and rec[1] != kept
    assert data[0][0].split(b"\n")[1] == rec[1]  # like every other route's


def test_host_formatter_refuses_the_route_with_bins():
    tp, c, res1, res2, xflags, _want = _hand_table(True)
    with pytest.raises(ValueError):
        fastq.format_chunk(c, tp, res1, None, res2, xflags=xflags, n_bins=1, bc=np.zeros(len(res1), dtype=np.uint8),
                           too_long_route=True)


# ---- the reports and the ranks ---------------------------------------------------------------------------------

def test_json_report_gains_the_keys_only_when_asked():
    st = planmod.CutadaptConfig()
    st.max_length = 40
    tp = planmod.compile_paired(TAKARA, st)
    t = _totals(too_long=3)
    plain = report.json_report(tp, t, TAKARA, "a", "b", "c", "d", "e", "f", None, None)
    asked = report.json_report(tp, t, TAKARA, "a", "b", "c", "d", "e", "f", None, None, too_long_files=["l1", "l2"])
    assert "too_long1" not in plain["output"] and "too_long2" not in plain["output"]
    assert asked["output"]["too_long1"] == "l1" and asked["output"]["too_long2"] == "l2"
    assert {k: v for k, v in asked["output"].items() if not k.startswith("too_long")} == plain["output"]
    assert asked["read_counts"] == plain["read_counts"] and asked["basepair_counts"] == plain["basepair_counts"]
    assert asked["read_counts"]["filtered"]["too_long"] == 3 and asked["read_counts"]["output"] == 5
    single = report.json_report(planmod.compile_single(TAKARA, st), t, TAKARA, "a", None, "c", None, "e", None, None, None,
                                too_long_files=["l1"])
    assert single["output"]["too_long1"] == "l1" and single["output"]["too_long2"] is None
    assert report.minimal_report(tp, t) == report.minimal_report(tp, _totals(too_long=3))


def test_rank_groups_and_totals(tmp_path):
    args = _names(too_long_file=["l1.fq.gz", "l2.fa"], untrimmed_file=[None, None])
    groups = ranks.output_groups(args)
    assert groups["too_long_file"] == ["l1.fq.gz", "l2.fa"]
    assert [ranks.part_name(n, 1) for n in groups["too_long_file"]] == ["l1.fq.gz.rank1.part.fq.gz", "l2.fa.rank1.part.fa"]
    assert "too_long_file" not in ranks.output_groups(_names())
    a, b = report.new_totals(), report.new_totals()
    a.update(too_long=3, routes=[5, 2, 1])
    b.update(too_long=4, routes=[6, 1, 0])
    report.merge_totals(a, b)
    assert a["too_long"] == 7 and a["routes"] == [11, 3, 1]  # (no fourth route in the totals)
    a.update(stats=[], devices=[0])
    ranks.dump_totals({"totals_file": str(tmp_path / "t.json")}, a)
    assert json.loads((tmp_path / "t.json").read_text())["too_long"] == 7
