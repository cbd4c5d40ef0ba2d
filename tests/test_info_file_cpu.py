"""--info-file on the CPU side: CLI flag and refusals, C ABI declarations and struct sizes, the adapter-name function,
rank part names, and the specification module (tests/info_rule.py) on hand-written reads."""
import ctypes as C
import re
from pathlib import Path

import pytest

from cutseq_amd import abi, capi, plan as planmod, ranks, report, run
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig
from oracle import pyref

import info_rule

ROOT = Path(__file__).resolve().parents[1]


def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


def test_cli_accepts_info_file():
    args = run.resolve_args(_args("--info-file", "info.txt.gz"))
    assert args.info_file == "info.txt.gz"
    assert run.resolve_args(_args()).info_file is None
    assert "--info-file" in run.build_parser().format_help()


def test_cli_refuses_info_file_with_demultiplexing(tmp_path, caplog):
    barcodes = tmp_path / "bc.tsv"
    barcodes.write_text("a\tACGTAC\nb\tTTGACA\n")
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args("--info-file", "info.txt", "--demux-barcodes", str(barcodes)))
    assert exc.value.code == 1
    assert "--info-file cannot be combined with --demux-barcodes" in caplog.text


def test_cli_refuses_info_file_on_the_host_path(monkeypatch, caplog):
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args("--info-file", "info.txt"))
    assert exc.value.code == 1
    assert "--info-file needs the text path" in caplog.text


def test_entry_points_are_declared_and_exported():
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    for sym in ("cs_text_info", "cs_text_fetch_info"):
        assert re.search(rf"\bint {sym}\(cs_text \*", header), sym
        assert sym in capi.EXPORTS
    lib = C.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "cs_text_info") and hasattr(lib, "cs_text_fetch_info")
    assert "CS_TEXT_ERR_INFO_MISMATCH = 5" in header and abi.CS_TEXT_ERR_INFO_MISMATCH == 5
    assert "CS_TEXT_ERR_INFO_OVERFLOW = 6" in header and abi.CS_TEXT_ERR_INFO_OVERFLOW == 6


def test_abi_is_unchanged_and_info_defaults_to_zero():
    assert abi.CS_ABI_VERSION == 7
    assert C.sizeof(abi.cs_text_params) == 48 and C.sizeof(abi.cs_text_result) == 176
    p = abi.cs_text_params()
    assert p.info == 0
    # the byte sits where the first reserved byte sat: nothing else moved
    assert abi.cs_text_params.info.offset == abi.cs_text_params.fasta_routes.offset + 1 == 46
    assert abi.cs_text_params.fasta_out.offset == 44 and abi.cs_text_params.n_bins.offset == 40
    assert (abi.CS_INFO_ON, abi.CS_INFO_GZIP, abi.CS_INFO_NO_QUAL) == (1, 2, 4)
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert "#define CS_ABI_VERSION 7" in header and "uint8_t info;" in header


@pytest.mark.parametrize("paired", [False, True])
def test_adapter_names_count_the_adapter_ops_of_the_chain(paired):
    st = planmod.CutadaptConfig()
    st.trim_polyA = st.trim_polyA_wo_direction = True
    bc = BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])
    tp = planmod.compile_paired(bc, st) if paired else planmod.compile_single(bc, st)
    names = planmod.info_adapter_names(tp.r1.ops)
    idx = [i for i, op in enumerate(tp.r1.ops) if isinstance(op, planmod.AdapterOp)]
    assert list(names) == idx and [names[i] for i in idx] == [str(k + 1) for k in range(len(idx))]
    assert len(idx) >= 4  # 5' adapter, 3' adapter, two poly ops
    # the same numbering as the specification's, and as the JSON report's first adapter
    pipe = (pyref.PairedPipeline if paired else pyref.SinglePipeline)(bc, pyref.Settings(trim_polyA=True, trim_polyA_wo_direction=True))
    assert sorted(info_rule.adapter_ordinals(pipe.mods).values()) == list(range(1, len(idx) + 1))
    assert planmod.info_adapter_names([planmod.CutOp(3), planmod.QTrimOp(20)]) == {}


def test_json_report_names_the_info_file_only_when_asked():
    bc = BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])
    tp = planmod.compile_paired(bc, planmod.CutadaptConfig())
    totals = report.new_totals()
    totals.update(in_pairs=10, routes=[5, 2, 1], in_bp=[1000, 1000], written_bp=[400, 400],
                  stats=[[abi.cs_stats().as_dict(), abi.cs_stats().as_dict()]])
    files = ("in1", "in2", "o1", "o2", "s1", "s2", None, None)
    without = report.json_report(tp, totals, bc, *files)
    keys = ["output1", "output2", "short1", "short2", "untrimmed1", "untrimmed2"]
    assert list(without["output"]) == keys
    assert report.json_report(tp, totals, bc, *files, info_file=None)["output"] == without["output"]
    given = report.json_report(tp, totals, bc, *files, info_file="info.tsv.gz")
    assert list(given["output"]) == keys + ["info_file"] and given["output"]["info_file"] == "info.tsv.gz"
    assert {k: given["output"][k] for k in keys} == without["output"]
    for block in ("input", "read_counts", "basepair_counts", "adapters_read1", "adapters_read2"):
        assert given[block] == without[block]


@pytest.mark.parametrize("files", [["r1.fq.gz"], ["r1.fq.gz", "r2.fq.gz"]], ids=["single", "paired"])
def test_dry_run_output_does_not_change_with_the_option(files, capsys, caplog):
    import logging

    def dry(*extra):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            run.run_cutseq(run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "--trim-polyA", "-n", *files, *extra])))
        return capsys.readouterr().out, [r.getMessage() for r in caplog.records]

    plain = dry()
    assert dry("--info-file", "info.tsv") == plain
    assert plain[0] or plain[1]  # (single-end prints the steps, paired logs them)


def test_rank_part_names_keep_the_container_suffix():
    assert ranks.part_name("info.txt", 0) == "info.txt"
    assert ranks.part_name("info.txt", 2) == "info.txt.rank2.part"
    assert ranks.part_name("out/info.tsv.gz", 1) == "out/info.tsv.gz.rank1.part.gz"
    assert ranks.part_name("info.txt.zst", 3) == "info.txt.zst.rank3.part.zst"
    # the table is one of the files every rank writes a part of -- only when it was asked for
    groups = ranks.output_groups(run.resolve_args(_args("--info-file", "info.tsv.gz")))
    assert groups["info_file"] == ["info.tsv.gz"]
    assert [ranks.part_name(n, 1) for n in groups["info_file"]] == ["info.tsv.gz.rank1.part.gz"]
    assert "info_file" not in ranks.output_groups(run.resolve_args(_args()))
    assert list(ranks.output_groups(run.resolve_args(_args()))) == ["output_file", "short_file", "untrimmed_file"]


# ---- the specification on hand-written reads -------------------------------------------------------------------------

SCHEME = "ACACGACGCTCTTCCGATCT>AGATCGGAAGAGCACACGTC"  # a 5' and a 3' adapter, nothing else
P5, P7 = "ACACGACGCTCTTCCGATCT", "AGATCGGAAGAGCACACGTC"
INSERT = "GGCCTTGGCATTGCGTCCAAGGCTTGACCTGA"


def _single(scheme=SCHEME, **kw):
    return pyref.SinglePipeline(BarcodeConfig(scheme), pyref.Settings(**kw))


def _read(seq, name="r comment/1", qual=None):
    return pyref.Read(name, seq, qual if qual is not None else "I" * len(seq))


def test_rule_one_match():
    seq = INSERT + P7 + "CC"
    got = info_rule.single_rows(_single(), _read(seq))
    n = len(INSERT)
    assert got == "\t".join(["r", "0", str(n), str(n + 20), INSERT, P7, "CC", "2", "I" * n, "I" * 20, "II", ""]) + "\n"


def test_rule_several_matches_in_chain_order_and_rightmost_front_coordinates():
    seq = "TT" + P5 + INSERT + P7
    got = info_rule.single_rows(_single(), _read(seq)).split("\n")
    assert got[-1] == "" and len(got) == 3
    first, second = got[0].split("\t"), got[1].split("\t")
    assert len(first) == len(second) == 12
    # the 5' hit in forward coordinates of the whole read (RightmostFrontAdapter.match_to maps them back)
    assert first[1:8] == ["0", "2", "22", "TT", P5, INSERT + P7, "1"]
    assert first[8] + first[9] + first[10] == "I" * len(seq) and first[11] == ""
    # the 3' op saw the read without what the 5' match removed
    assert second[1:8] == ["0", str(len(INSERT)), str(len(INSERT) + 20), INSERT, P7, "", "2"]
    assert second[4] + second[5] + second[6] == INSERT + P7


def test_rule_rightmost_front_takes_the_last_copy():
    seq = P5 + "GG" + P5 + INSERT
    row = info_rule.single_rows(_single(), _read(seq)).split("\n")[0].split("\t")
    assert row[2:4] == ["22", "42"] and row[4] == P5 + "GG" and row[6] == INSERT


def test_rule_no_match_shows_the_final_read():
    qual = "I" * (len(INSERT) - 4) + "####"
    got = info_rule.single_rows(_single(), _read(INSERT, qual=qual))
    assert got == "\t".join(["r", "-1", INSERT[:-4], "I" * (len(INSERT) - 4), ""]) + "\n"  # quality-trimmed


def test_rule_fasta_has_empty_quality_columns():
    one = info_rule.single_rows(_single(), _read(INSERT + P7, qual="~" * (len(INSERT) + 20)), has_qual=False)
    assert "~" not in one and one.split("\t")[8:12] == ["", "", "", "\n"]
    none = info_rule.single_rows(_single(min_quality=0), _read(INSERT, qual="~" * len(INSERT)), has_qual=False)
    assert none == f"r\t-1\t{INSERT}\t\t\n"


def test_rule_auto_rc_turns_the_final_read_only():
    scheme = SCHEME.replace(">", "<")  # a '-' library
    pipe = _single(scheme, auto_rc=True)
    assert pipe.rc
    qual = "".join(chr(40 + i) for i in range(len(INSERT)))
    got = info_rule.single_rows(pipe, _read(INSERT, qual=qual))
    rc = INSERT.translate(pyref.COMPLEMENT)[::-1]
    assert got == f"r\t-1\t{rc}\t{qual[::-1]}\t\n"
    row = info_rule.single_rows(pipe, _read(INSERT + P7)).split("\t")
    assert row[4:7] == [INSERT, P7, ""]  # a match row shows the read as the op saw it: not turned


def test_rule_umi_tag_and_cutters_between_matches():
    scheme = "ACACGACGCTCTTCCGATCTNNNN>NNNAGATCGGAAGAGCACACGTC"  # 5' and 3' UMIs, single-end
    pipe = _single(scheme)
    seq = "ACGT" + INSERT + "TGA" + P7
    got = info_rule.single_rows(pipe, _read(seq, name="x.1"))
    row = got.split("\t")
    assert row[0] == "x_ACGTTGA" and row[4] == "ACGT" + INSERT + "TGA" and row[7] == "2"


def test_rule_paired_is_about_read_one():
    bc = BarcodeConfig(SCHEME)
    pipe = pyref.PairedPipeline(bc, pyref.Settings())
    r1 = _read(INSERT + P7, name="p/1")
    r2 = _read("TTGACCA" * 5 + bc.p5.rc, name="p/2")
    got = info_rule.paired_rows(pipe, r1, r2)
    assert got.count("\n") == 1 and got.split("\t")[0] == "p" and got.split("\t")[4:7] == [INSERT, P7, ""]
    none = info_rule.paired_rows(pipe, _read(INSERT, name="p/1"), r2)
    assert none == f"p\t-1\t{INSERT}\t{'I' * len(INSERT)}\t\n"


def test_census_counts_what_the_guards_need():
    text = (info_rule.single_rows(_single(), _read("TT" + P5 + INSERT + P7, name="a")) +
            info_rule.single_rows(_single(), _read(INSERT, name="b")) +
            info_rule.single_rows(_single(), _read(INSERT + P7, name="c"))).encode()
    assert info_rule.census(text) == (1, 1, {"1": 1, "2": 2})
