"""The output layout (cutseq_amd/outputs.py) against the behaviour lock tests/golden/output_layout.json.

The golden file was written by tools/record_output_layout.py at commit 67d8daf, the last one in which ``resolve_args``,
``textio``, ``ranks`` and ``run_cutseq`` each derived the output files for themselves; it is never written again by
the code under test.  Everything it holds per command line is recomputed here through the layout and compared for
equality."""
import dataclasses
import json
import logging
from pathlib import Path

import pytest

from cutseq_amd import outputs, plan as planmod, ranks, report, run, textio

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "output_layout.json").read_text())


@pytest.fixture(scope="module")
def barcodes(tmp_path_factory):
    path = tmp_path_factory.mktemp("layout") / "barcodes.tsv"
    path.write_text("b1\tACGTACGT\nb2\tTGCATGCA\n")
    return str(path)


def _resolve(argv, barcodes):
    return run.resolve_args(run.build_parser().parse_args([barcodes if a == "{barcodes}" else a for a in argv]))


def _text(layout, tp, fasta, gpu_deflate=True):
    try:
        return {"options": dataclasses.asdict(textio.text_options(layout, tp, fasta, gpu_deflate))}
    except Exception as exc:  # noqa: BLE001 -- (the golden file names the type and the message)
        return {"error": [type(exc).__name__, str(exc)]}


@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_layout_equals_the_recorded_behaviour(case, barcodes):
    want = GOLDEN["cases"][case]
    args = _resolve(want["argv"], barcodes)
    layout = args.outputs
    barcode = planmod.BarcodeConfig(args.adapter_scheme)
    tp = run.compile_plan(args, barcode, run.settings_from_args(args))
    assert (layout.paired, layout.interleaved_in, layout.interleaved_out) == (want["paired"], want["interleaved_in"], want["interleaved_out"])
    assert tp.paired == want["paired"] and tp.swap_outputs == want["swap_outputs"]
    # the resolved names per class: in the layout, and in the attributes resolve_args still fills for its callers
    names = {c.key: list(c.names) for c in layout.classes if not c.barcode}
    names.setdefault("too_long_file", None)
    names["info_file"] = layout.info_file
    assert names == want["names"]
    assert {key: getattr(args, key) for key in want["names"]} == want["names"]
    assert (args.paired, args.interleaved_in, args.interleaved_out) == (want["paired"], want["interleaved_in"], want["interleaved_out"])
    n_bins = len(tp.demux.barcodes) if tp.demux is not None else 0
    assert layout.n_bins == n_bins and [c.key for c in layout.classes if c.barcode] == (list(args.demux[0]) if n_bins else [])
    assert [c.route for c in layout.classes] == [0, 1, 2] + [3] * (len(layout.classes) - 3)
    for swap in (False, True):
        assert layout.name_groups(swap) == want["name_groups"][str(swap)]
        assert textio.output_name_groups(args, tp.paired, swap, n_bins) == want["name_groups"][str(swap)]
    assert layout.too_long_route == (len(want["name_groups"]["False"]) == 4 and not n_bins)
    # the ranks: the spec's groups, the parts' names, and back
    groups = layout.rank_groups()
    assert groups == want["rank_groups"] == ranks.output_groups(args) and list(groups) == list(want["rank_groups"])
    parts = {key: [ranks.part_name(name, 1) for name in group] for key, group in groups.items()}
    assert parts == want["rank_parts"]
    assert layout.with_rank_names(parts).rank_groups() == parts
    if not n_bins:  # (bins: a rank has no common trimmed file, the run's layout keeps the names for its report)
        assert layout.with_rank_names(json.loads(json.dumps(groups))) == layout
    assert sorted(layout.names()) == sorted(n for group in groups.values() for n in group if n)
    # the JSON report's blocks, asked for as run_cutseq asks
    totals = report.new_totals()
    totals["routes"] += [0] * n_bins
    totals.update(stats=[], devices=[0], seconds=1.0, bin_names=list(args.demux[0]) if n_bins else None)
    positional, keywords = layout.report_names(args.input_file)
    rep = report.json_report(tp, totals, barcode, *positional, **keywords)
    assert {"input": rep["input"], "output": rep["output"]} == want["report"]
    assert list(rep["output"]) == list(want["report"]["output"])
    # what the text engines are told
    assert _text(layout, tp, fasta=False) == want["text"]["qualities"]
    assert _text(layout, tp, fasta=True) == want["text"]["no_qualities"]
    assert _text(layout, tp, fasta=False, gpu_deflate=False) == want["text"]["qualities_host_deflate"]


@pytest.mark.parametrize("case", sorted(GOLDEN["refused"]))
def test_refused_command_lines_say_what_they_said(case, barcodes, caplog):
    want = GOLDEN["refused"][case]
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as exc:
        _resolve(want["argv"], barcodes)
    assert exc.value.code == want["refused"]["code"]
    assert [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR] == [want["refused"]["message"]]


def test_the_golden_file_holds_the_whole_matrix():
    assert len(GOLDEN["cases"]) == 17 and len(GOLDEN["refused"]) == 7
    assert any(c["swap_outputs"] and not c["interleaved_out"] for c in GOLDEN["cases"].values())
    assert any(c["text"]["qualities"].get("options", {}).get("mate2_first") for c in GOLDEN["cases"].values())
    assert any("options" in c["text"]["no_qualities"] for c in GOLDEN["cases"].values())


def test_run_still_exports_the_class_table():
    assert run.OUTPUT_CLASSES is outputs.OUTPUT_CLASSES
    assert run.OUTPUT_CLASSES == (("output_file", "trimmed"), ("short_file", "short"), ("untrimmed_file", "untrimmed"))
