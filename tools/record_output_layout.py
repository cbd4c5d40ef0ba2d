#!/usr/bin/env python3
"""Record what the command line decides about its output files: tests/golden/output_layout.json.

    python tools/record_output_layout.py [FILE]

For every command line of MATRIX: the resolved names per output class, ``textio.output_name_groups`` with and without
the --auto-rc swap, the rank spec's groups and part names, the "input" / "output" blocks of the JSON report as
``run_cutseq`` asks for them, and the text options ``run_text_pipeline`` hands to its workers for an input with and
without qualities (or the error it raises) and with CUTSEQ_GPU_DEFLATE=0; for every command line of REFUSED the
message and the exit code.  No GPU and no input file is needed: the pipeline's readers, writers and workers and the
run itself are replaced by stand-ins that record what they are handed, so the figures are the product's own, whatever
its internals look like.

The committed file was written by the commit BEFORE the output layout object (cutseq_amd/outputs.py) existed and is
the behaviour lock of that change (tests/test_output_layout_cpu.py recomputes it through the layout): do not write it
again from a later tree -- run this tool to a scratch FILE and compare instead.
"""
from __future__ import annotations

import contextlib
import dataclasses
import inspect
import io
import json
import logging
import os
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from cutseq_amd import ranks, report, run, textio  # noqa: E402
from cutseq_amd.common import BarcodeConfig  # noqa: E402

BARCODES = "{barcodes}"  # stands for the barcode list's path (a temporary file: two barcodes, b1 and b2)
BARCODE_LINES = "b1\tACGTACGT\nb2\tTGCATGCA\n"
DEMUX_SCHEME = "ACACGACGCTCTTCCGATCT(ACGTACGT)NNNNNNNN>AGATCGGAAGAGCACACGTC"
A = ["-A", "TAKARAV3"]

MATRIX = {
    "one input": A + ["r1.fq.gz"],
    "one input, -u": A + ["r1.fq.gz", "-u", "u.fq"],
    "two inputs": A + ["r1.fq.gz", "r2.fq.gz"],
    "two inputs, -O": A + ["r1.fq.gz", "r2.fq.gz", "-O", "pre"],
    "two inputs, all named": A + ["r1.fq.gz", "r2.fq.gz", "-o", "a.fq", "b.fa", "-s", "c.fq.gz", "d.fq.gz", "-u", "e", "f"],
    "two inputs, inline barcode ensured": ["-a", DEMUX_SCHEME, "r1.fq.gz", "r2.fq.gz", "--ensure-inline-barcode"],
    "two inputs, too-long files": A + ["r1.fq.gz", "r2.fq.gz", "-M", "100", "--too-long-output", "l1.fa", "l2.fq"],
    "two inputs, info file": A + ["r1.fq.gz", "r2.fq.gz", "--info-file", "i.tsv.gz"],
    "two inputs, FASTA names, info file": A + ["r1.fa", "r2.fa", "-o", "a.fa", "b.fa", "-s", "c.fa", "d.fasta", "--info-file", "i.tsv"],
    "two inputs, --auto-rc": A + ["r1.fq.gz", "r2.fq.gz", "--auto-rc", "-o", "a.fa", "b.fq"],
    "interleaved, two inputs, --auto-rc": A + ["r1.fq.gz", "r2.fq.gz", "--interleaved", "--auto-rc"],
    "interleaved, one input": A + ["in.fq.gz", "--interleaved"],
    "interleaved, one input, -o a b": A + ["in.fq.gz", "--interleaved", "-o", "a", "b"],
    "interleaved, two inputs, -o a": A + ["r1.fq.gz", "r2.fq.gz", "--interleaved", "-o", "a"],
    "interleaved, one input, too-long and info": A + ["in.fq.gz", "--interleaved", "-M", "100", "--too-long-output",
                                                      "l.fq.gz", "--info-file", "i.tsv"],
    "demux": ["-a", DEMUX_SCHEME, "r1.fq.gz", "r2.fq.gz", "--demux-barcodes", BARCODES],
    "demux, -O": ["-a", DEMUX_SCHEME, "r1.fq.gz", "r2.fq.gz", "--demux-barcodes", BARCODES, "-O", "pre"],
}
REFUSED = {
    "interleaved, two inputs, two -o": A + ["r1.fq", "r2.fq", "--interleaved", "-o", "a.fq", "b.fq"],
    "interleaved with demux": A + ["in.fq", "--interleaved", "--demux-barcodes", BARCODES],
    "too-long files without -M": A + ["r1.fq", "r2.fq", "--too-long-output", "a.fq", "b.fq"],
    "too-long files with demux": A + ["r1.fq", "r2.fq", "-M", "30", "--too-long-output", "a.fq", "b.fq",
                                      "--demux-barcodes", BARCODES],
    "one -s for two inputs": A + ["r1.fq", "r2.fq", "-s", "s.fq"],
    "info file with demux": A + ["r1.fq", "r2.fq", "--info-file", "i.tsv", "--demux-barcodes", BARCODES],
    "three inputs": A + ["r1.fq", "r2.fq", "r3.fq"],
}


class Stop(Exception):
    pass


@contextlib.contextmanager
def patched(obj, **attrs):
    saved = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(obj, k, v)


def resolve(argv, barcodes: str):
    """-> (args, None) or (None, {"message", "code"}) for a command line ``resolve_args`` refuses."""
    argv = [barcodes if a == BARCODES else a for a in argv]
    said = io.StringIO()
    handler = logging.StreamHandler(said)
    handler.setLevel(logging.ERROR)
    handler.setFormatter(logging.Formatter("%(message)s"))
    logging.getLogger().addHandler(handler)
    try:
        return run.resolve_args(run.build_parser().parse_args(argv)), None
    except SystemExit as exc:
        return None, {"message": said.getvalue().strip(), "code": exc.code}
    finally:
        logging.getLogger().removeHandler(handler)


def worker_options(args, tp, fasta: bool):
    """What ``run_text_pipeline`` hands to its workers -- by name, whether they arrive one by one or as one value --
    or the error it raises on the way there."""
    seen = {}

    class Reader:
        def __init__(self, *a, **kw):
            self.fasta = fasta

        def close(self):
            pass

    class Writer:
        def __init__(self, *a, **kw):
            pass

        def close(self):
            pass

    real = textio.TextWorker.__init__

    def worker(*a, **kw):
        bound = inspect.signature(real).bind(None, *a, **kw)
        bound.apply_defaults()
        for name, value in bound.arguments.items():
            if name in ("self", "tp", "device", "chunk_reads"):
                continue
            if dataclasses.is_dataclass(value):
                seen.update(dataclasses.asdict(value))
            else:
                seen[name] = value
        raise Stop

    with patched(textio, TextReader=Reader, StreamWriter=Writer, TextWorker=worker):
        try:
            textio.run_text_pipeline(args, tp, [0], 1000)
        except Stop:
            return {"options": {k: (int(v) if not isinstance(v, bool) else v) for k, v in sorted(seen.items())}}
        except Exception as exc:  # noqa: BLE001
            return {"error": [type(exc).__name__, str(exc)]}
    raise AssertionError("the pipeline went past its workers")


def report_blocks(args, tp, barcode):
    """The "input" and "output" blocks of the JSON report, as ``run_cutseq`` asks ``report.json_report`` for them."""
    seen = {}

    def pipeline(args, tp, shares=None):
        totals = report.new_totals()
        n_bins = len(tp.demux.barcodes) if tp.demux is not None else 0
        totals["routes"] += [0] * n_bins
        totals.update(stats=[], devices=[0], seconds=1.0, bin_names=list(args.demux[0]) if n_bins else None)
        return totals

    args.json_file = "report.json"
    with patched(run, run_pipeline=pipeline), patched(report, write_json=lambda path, rep: seen.update(rep)), \
            contextlib.redirect_stderr(io.StringIO()):
        run.run_cutseq(args, [])
    return {"input": seen["input"], "output": seen["output"]}


def snapshot(argv, barcodes: str) -> dict:
    args, refused = resolve(argv, barcodes)
    if refused is not None:
        return {"argv": argv, "refused": refused}
    barcode = BarcodeConfig(args.adapter_scheme)
    tp = run.compile_plan(args, barcode, run.settings_from_args(args))
    n_bins = len(tp.demux.barcodes) if tp.demux is not None else 0
    out = {"argv": argv, "paired": bool(args.paired), "interleaved_in": bool(args.interleaved_in),
           "interleaved_out": bool(args.interleaved_out), "swap_outputs": bool(tp.swap_outputs),
           "names": {attr: getattr(args, attr) for attr in ("output_file", "short_file", "untrimmed_file", "too_long_file",
                                                            "info_file")}}
    out["name_groups"] = {str(swap): textio.output_name_groups(args, tp.paired, swap, n_bins) for swap in (False, True)}
    groups = ranks.output_groups(args)
    out["rank_groups"] = groups
    out["rank_parts"] = {key: [ranks.part_name(name, 1) for name in names] for key, names in groups.items()}
    out["report"] = report_blocks(args, tp, barcode)
    out["text"] = {"qualities": worker_options(args, tp, False), "no_qualities": worker_options(args, tp, True)}
    os.environ["CUTSEQ_GPU_DEFLATE"] = "0"
    try:
        out["text"]["qualities_host_deflate"] = worker_options(args, tp, False)
    finally:
        del os.environ["CUTSEQ_GPU_DEFLATE"]
    return out


def record() -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        barcodes = os.path.join(tmp, "barcodes.tsv")
        with open(barcodes, "w") as fh:
            fh.write(BARCODE_LINES)
        return {"cases": {name: snapshot(argv, barcodes) for name, argv in MATRIX.items()},
                "refused": {name: snapshot(argv, barcodes) for name, argv in REFUSED.items()}}


if __name__ == "__main__":
    target = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "output_layout.json"
    target.write_text(json.dumps(record(), indent=1) + "\n")
    print(f"{target}: {len(MATRIX)} command lines, {len(REFUSED)} refused ones")
