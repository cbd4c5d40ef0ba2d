"""--interleaved on the CPU side: the rule (tests/interleave_rule.py), the command line's names and refusals, the C ABI
declarations, the output files' groups and formats, the JSON report's keys and the reader's blocks of whole pairs."""
import ctypes as C
import gzip
import re
from pathlib import Path
from types import SimpleNamespace

import pytest

from cutseq_amd import abi, capi, fastq, plan as planmod, report, run, textio
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.outputs import OutputLayout

import interleave_rule

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])


def _recs(n, mate, line_end=b"\n"):
    return [b"@r%d/%d x" % (i, mate) + line_end + b"ACGT" * (3 + i % 30) + line_end + b"+" + line_end
            + b"IIII" * (3 + i % 30) + line_end for i in range(n)]


# ---- the rule --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("line_end", [b"\n", b"\r\n"])
@pytest.mark.parametrize("final_newline", [True, False])
def test_the_rule_round_trips(line_end, final_newline):
    one, two = b"".join(_recs(7, 1, line_end)), b"".join(_recs(7, 2, line_end))
    if not final_newline:
        two = two[:-len(line_end)]
    woven = interleave_rule.weave(one, two)
    assert woven.count(b"@r") == 14 and woven.endswith(two[-8:])
    assert woven.startswith(_recs(1, 1, line_end)[0] + _recs(1, 2, line_end)[0])
    assert interleave_rule.deinterleave(woven) == (one, two)
    assert interleave_rule.weave(*interleave_rule.deinterleave(woven)) == woven
    assert interleave_rule.deinterleave(b"") == (b"", b"") and interleave_rule.weave(b"", b"") == b""


def test_the_rule_on_fasta_mate2_first_and_a_mate_1_without_its_last_line_end():
    fa1, fa2 = b">a\nAC\n>b\nGT\n", b">a2\nTT\n>b2\nCC\n"
    assert interleave_rule.weave(fa1, fa2, fasta=True) == b">a\nAC\n>a2\nTT\n>b\nGT\n>b2\nCC\n"
    assert interleave_rule.weave(fa1, fa2, fasta=True, mate2_first=True) == b">a2\nTT\n>a\nAC\n>b2\nCC\n>b\nGT\n"
    one, two = b"".join(_recs(3, 1)), b"".join(_recs(3, 2))
    assert interleave_rule.weave(one[:-1], two) == interleave_rule.weave(one, two)  # (mate 1's last line ends inside)
    swapped = interleave_rule.weave(one, two, mate2_first=True)
    assert interleave_rule.deinterleave(swapped) == (two, one)
    with pytest.raises(ValueError):
        interleave_rule.weave(one, two[:two.rfind(b"@")])
    with pytest.raises(ValueError):
        interleave_rule.deinterleave(one[:one.rfind(b"@")] + two)  # five records


# ---- the command line ------------------------------------------------------------------------------------------

def _args(*extra, inputs=("in.fq.gz",)):
    return run.build_parser().parse_args(["-A", "TAKARAV3", *inputs, "--interleaved", *extra])


def _names(args):
    return [getattr(args, attr) for attr, _word in run.OUTPUT_CLASSES]


def test_one_input_file_holds_the_pairs_and_the_outputs_follow_o():
    args = run.resolve_args(_args())
    assert args.paired and args.interleaved_in and args.interleaved_out
    assert _names(args) == [["in_trimmed.fastq.gz"], ["in_short.fastq.gz"], [None]]
    args = run.resolve_args(_args("-O", "pre", "--ensure-inline-barcode", "-u", "u.fq"))
    assert _names(args) == [["pre_trimmed.fastq.gz"], ["pre_short.fastq.gz"], ["u.fq"]]
    args = run.resolve_args(_args("-o", "-", "-s", "s.fq"))
    assert args.interleaved_out and _names(args) == [["-"], ["s.fq"], [None]]
    # two names for -o: split output, two names in every class, the stem from -O or the one input
    args = run.resolve_args(_args("-o", "o1.fq", "o2.fq"))
    assert args.paired and args.interleaved_in and not args.interleaved_out
    assert _names(args) == [["o1.fq", "o2.fq"], ["in_short_R1.fastq.gz", "in_short_R2.fastq.gz"], [None, None]]
    args = run.resolve_args(_args("-o", "o1.fq", "o2.fq", "-O", "pre", "-M", "30", "--too-long-output", "l1.fq", "l2.fq"))
    assert args.short_file == ["pre_short_R1.fastq.gz", "pre_short_R2.fastq.gz"] and args.too_long_file == ["l1.fq", "l2.fq"]
    # the plan is the paired plan, as if two files had been given
    tp = run.compile_plan(args, TAKARA, run.settings_from_args(args))
    assert tp.paired and tp.r2 is not None


def test_two_input_files_write_interleaved_outputs():
    args = run.resolve_args(_args(inputs=("a_R1.fq.gz", "a_R2.fq.gz")))
    assert args.paired and not args.interleaved_in and args.interleaved_out
    assert _names(args) == [["a_trimmed.fastq.gz"], ["a_short.fastq.gz"], [None]]
    args = run.resolve_args(_args("-o", "o.fq", "-O", "pre", "-M", "40", "--too-long-output", "long.fa", "-m", "20",
                                  inputs=("a_R1.fq.gz", "a_R2.fq.gz")))
    assert _names(args) == [["o.fq"], ["pre_short.fastq.gz"], [None]] and args.too_long_file == ["long.fa"]
    # --ranks is fine here: the parts are concatenated in rank order
    args = run.resolve_args(_args("--ranks", "2", inputs=("a_R1.fq.gz", "a_R2.fq.gz")))
    assert args.interleaved_out and args.ranks == 2


def test_without_the_option_nothing_changes():
    args = run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq", "r2.fq"]))
    assert args.paired and not args.interleaved_in and not args.interleaved_out
    assert args.output_file == ["r1_trimmed_R1.fastq.gz", "r2_trimmed_R2.fastq.gz"]
    args = run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq"]))
    assert not args.paired and args.output_file == ["r1_trimmed_R1.fastq.gz"]
    assert not run.compile_plan(args, TAKARA, run.settings_from_args(args)).paired


@pytest.mark.parametrize("argv, inputs, message", [
    (["--demux-barcodes", "codes.tsv"], ("in.fq",), "--interleaved cannot be combined with --demux-barcodes"),
    (["--ranks", "2"], ("in.fq",), "--interleaved input cannot be split between --ranks"),
    (["-o", "a.fq", "b.fq"], ("r1.fq", "r2.fq"), "would have nothing to do"),
    (["-o", "a.fq", "b.fq", "c.fq"], ("in.fq",), "Number of trimmed output files (3) must match the number this --interleaved run"),
    (["-s", "a.fq", "b.fq"], ("in.fq",), "Number of short output files (2) must match the number this --interleaved run "
                                         "writes per class: 1"),
    (["-o", "a.fq", "b.fq", "-s", "s.fq"], ("in.fq",), "Number of short output files (1) must match the number this "
                                                       "--interleaved run writes per class: 2"),
    (["-u", "a.fq", "b.fq"], ("r1.fq", "r2.fq"), "Number of untrimmed output files (2) must match"),
    (["-M", "30", "--too-long-output", "a.fq", "b.fq", "-m", "20"], ("r1.fq", "r2.fq"),
     "Number of too-long output files (2) must match the number this --interleaved run writes per class: 1"),
])
def test_cli_refuses(argv, inputs, message, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args(*argv, inputs=inputs))
    assert exc.value.code == 1
    assert message in caplog.text


def test_the_record_path_is_refused(monkeypatch, caplog):
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    with pytest.raises(SystemExit):
        run.resolve_args(_args())
    assert "--interleaved needs the text path" in caplog.text


def test_Q_needs_a_second_read_and_an_interleaved_file_has_one(caplog):
    args = run.resolve_args(_args("-Q", "5,15"))
    assert args.min_quality_r2 == 15 and args.min_quality_front_r2 == 5
    with pytest.raises(SystemExit):
        run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "in.fq", "-Q", "15"]))
    assert "-Q sets the quality cutoff of the second read" in caplog.text


def test_dry_run_prints_the_paired_steps(capsys, caplog):
    import logging
    with caplog.at_level(logging.INFO):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", "r2.fq.gz"])
        two = (capsys.readouterr().out, [r.getMessage() for r in caplog.records])
        caplog.clear()
        run.main(["-A", "TAKARAV3", "--dry-run", "in.fq.gz", "--interleaved"])
        one = (capsys.readouterr().out, [r.getMessage() for r in caplog.records])
    assert two[0].startswith("p5: ") and two[1] and one == two
    assert "--interleaved" in run.build_parser().format_help()


# ---- the output files' groups and formats, the report ----------------------------------------------------------

def test_one_name_per_class_and_no_swap():
    args = SimpleNamespace(outputs=OutputLayout.of(["t.fq"], ["s.fa"], [None], ["l.fq.gz"], paired=True, interleaved_out=True))
    for swap in (False, True):  # (paired --auto-rc on a '-' library: the device leads with mate 2 instead)
        assert textio.output_name_groups(args, True, swap, 0) == [["t.fq"], ["s.fa"], [None], ["l.fq.gz"]]
    groups = textio.output_name_groups(args, True, False, 0)
    # one file, one format: both mates' bits of the class
    assert textio.output_formats([g * 2 for g in groups], has_qualities=True) == 0b1100
    args.outputs = OutputLayout.of(["a", "b"], ["c", "d"], [None, None], None, paired=True)
    assert textio.output_name_groups(args, True, True, 0) == [["b", "a"], ["c", "d"], [None, None]]


def test_json_report_names_the_single_files_under_the_mate_1_keys():
    tp = planmod.compile_paired(TAKARA, planmod.CutadaptConfig())
    totals = report.new_totals()
    totals.update(stats=[], devices=[0], seconds=1.0, bin_names=None)
    plain = report.json_report(tp, totals, TAKARA, "a", "b", "c", "d", "e", "f", None, None)
    assert plain["input"] == {"path1": "a", "path2": "b", "paired": True, "interleaved": False}
    woven = report.json_report(tp, totals, TAKARA, "in.fq", None, "o.fq", None, "s.fq", None, None, None,
                               too_long_files=["l.fq"], interleaved=True)
    assert woven["input"] == {"path1": "in.fq", "path2": None, "paired": True, "interleaved": True}
    out = woven["output"]
    assert (out["output1"], out["output2"], out["short1"], out["short2"]) == ("o.fq", None, "s.fq", None)
    assert (out["too_long1"], out["too_long2"]) == ("l.fq", None)
    assert woven["read_counts"] == plain["read_counts"] and woven["basepair_counts"] == plain["basepair_counts"]
    single = report.json_report(planmod.compile_single(TAKARA, planmod.CutadaptConfig()), totals, TAKARA, "a", None, "c",
                                None, "e", None, None, None)
    assert single["input"] == {"path1": "a", "path2": None, "paired": False, "interleaved": False}


# ---- the C ABI -------------------------------------------------------------------------------------------------

def test_header_declares_the_function_and_the_constants():
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"enum \{ CS_INTERLEAVE_IN = 1, CS_INTERLEAVE_OUT = 2, CS_INTERLEAVE_OUT_MATE2_FIRST = 4 \};", header)
    assert re.search(r"int cs_text_create_interleaved\(cs_engine \*eng, const cs_text_params \*params, uint32_t interleave,\s*"
                     r"uint32_t n_slots, uint64_t max_text_bytes, uint32_t max_records,\s*uint32_t stride, cs_text \*\*out\);",
                     header)
    assert (abi.CS_INTERLEAVE_IN, abi.CS_INTERLEAVE_OUT, abi.CS_INTERLEAVE_OUT_MATE2_FIRST) == (1, 2, 4)
    assert "cs_text_create_interleaved" in capi.EXPORTS and "cs_text_create" in capi.EXPORTS
    # the ABI everything else is pinned to has not moved
    assert re.search(r"#define CS_ABI_VERSION 7\b", header) and abi.CS_ABI_VERSION == 7
    assert C.sizeof(abi.cs_text_params) == 48 and C.sizeof(abi.cs_text_result) == 176
    source = (ROOT / "cutseq_amd" / "csrc" / "cutseq_hip.hip").read_text()
    assert "return cs_text_create_interleaved(eng, params, 0u, n_slots, max_text_bytes, max_records, stride, out);" in source


# ---- the reader ------------------------------------------------------------------------------------------------

@pytest.fixture
def unpinned(monkeypatch):
    """The text path keeps its blocks in page-locked memory; without a GPU an ordinary arena stands in."""
    monkeypatch.setattr(fastq, "PINNED", fastq._Arena())


def _drain(reader):
    got, blocks = b"", []
    while True:
        b = reader.get()
        if b is None:
            break
        text = bytes(memoryview(b.buf)[: b.nbytes])
        blocks.append((b.n, b.first_record, text.count(b"\n") + (0 if text.endswith(b"\n") else 1)))
        got += text
        b.release()
    reader.close()
    return got, blocks


def _woven_file(tmp_path, container, pairs):
    one, two = b"".join(_recs(pairs, 1)), b"".join(_recs(pairs, 2))
    woven = interleave_rule.weave(one, two)
    if container == "fasta":
        lines = woven.split(b"\n")
        data = b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))
        path = tmp_path / "in.fa"
        path.write_bytes(data)
    elif container == "gz":
        path = tmp_path / "in.fq.gz"
        path.write_bytes(gzip.compress(woven, 1))
    elif container == "gz-members":
        path = tmp_path / "in.fq.gz"
        recs = interleave_rule._records(woven, 4)
        path.write_bytes(b"".join(gzip.compress(b"".join(recs[lo:lo + 999]), 1) for lo in range(0, len(recs), 999)))
    else:
        path = tmp_path / "in.fq"
        path.write_bytes(woven)
    return str(path), woven


@pytest.mark.parametrize("container", ["plain", "gz", "gz-members", "fasta"])
def test_reader_blocks_hold_whole_pairs(tmp_path, unpinned, container):
    pairs = 5203
    path, woven = _woven_file(tmp_path, container, pairs)
    got, blocks = _drain(textio.TextReader(path, 2 * 1500, interleaved=True))
    assert [b[0] for b in blocks] == [1500, 1500, 1500, 703]          # pairs per block ...
    assert [b[1] for b in blocks] == [0, 1500, 3000, 4500]            # ... counted in pairs
    assert all(lines == 8 * n for n, _first, lines in blocks)         # an even number of records each
    if container != "fasta":
        assert got == woven.rstrip(b"\n")
    else:  # (re-shaped to four lines with invented qualities: the names and bases are the file's)
        assert got.split(b"\n")[0::4] == woven.rstrip(b"\n").split(b"\n")[0::4]
        assert got.split(b"\n")[1::4] == woven.rstrip(b"\n").split(b"\n")[1::4]


@pytest.mark.parametrize("container", ["plain", "gz"])
def test_an_odd_record_count_raises(tmp_path, unpinned, container):
    one, two = b"".join(_recs(2001, 1)), b"".join(_recs(2000, 2))
    data = interleave_rule.weave(one[:one.rfind(b"@")], two) + one[one.rfind(b"@"):]
    path = tmp_path / ("odd.fq.gz" if container == "gz" else "odd.fq")
    path.write_bytes(gzip.compress(data, 1) if container == "gz" else data)
    with pytest.raises(fastq.FastqFormatError) as exc:
        _drain(textio.TextReader(str(path), 2 * 1500, interleaved=True))
    assert "interleaved input is incomplete" in str(exc.value) and "no partner" in str(exc.value)
    # the same file read as single-end is fine
    assert [b[0] for b in _drain(textio.TextReader(str(path), 3000))[1]] == [3000, 1001]


def test_the_block_cutting_function_itself():
    assert textio.TextReader.pair_count(0, "x") == 0 and textio.TextReader.pair_count(3000, "x") == 1500
    with pytest.raises(fastq.FastqFormatError) as exc:
        textio.TextReader.pair_count(3001, "in.fq")
    assert "in.fq" in str(exc.value) and "the last record has no partner" in str(exc.value)
    with pytest.raises(ValueError):
        textio.TextReader("x.fq", 3001, interleaved=True)  # blocks of an odd number of records
