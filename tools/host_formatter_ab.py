#!/usr/bin/env python3
"""The record path's host formatter alone (fastq.finish_chunk -> csh_format_chunk), CPU, one thread: 100 000 synthetic
2x150 pairs (TAKARAV3, --trim-polyA), results from the C oracle, all six plain streams open; once without bins and once
with 7 bins (bc = i % 7, every 50th record without a barcode).  ``--tree DIR`` takes ``cutseq_amd`` from another built
checkout and times it beside this one: one warm worker process per tree, the rounds alternating between them.  Prints one
JSON line per round and a summary (ms: min / median / max per tree and form); with ``--tree``, also whether this tree's
median lies inside the other's min .. max or below it.

  python tools/host_formatter_ab.py [--tree DIR] [--pairs 100000] [--rounds 12] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FORMS = (("plain", 0), ("bins7", 7))


def worker(tree: str, pairs: int):
    """One round of every form per line read from stdin; the times go to stdout."""
    sys.path.insert(0, tree)
    import numpy as np

    import oracle
    from cutseq_amd import abi, fastq, plan as planmod, synth
    from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig

    st = planmod.CutadaptConfig()
    st.trim_polyA = True
    tp = planmod.compile_paired(BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), st)
    b = synth.generate_pairs(pairs, 150, seed=1234)
    a1, n1, a2, n2 = tp.pack()
    res1, _, _ = oracle.trim_mate(a1, n1, tp.params(), b.seq1, b.qual1, b.len1)
    res2, _, _ = oracle.trim_mate(a2, n2, tp.params(), b.seq2, b.qual2, b.len2)
    names1 = "".join(f"SIM:{i} 1:N:0:IDX\n" for i in range(pairs)).encode()
    names2 = names1.replace(b" 1:N", b" 2:N")
    lens = np.array([len(x) for x in names1.split(b"\n")[:-1]], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.int64)
    chunk = fastq.Chunk(pairs, b.stride, names1, offs, lens, b.seq1, b.qual1, b.len1, names2, offs, lens, b.seq2,
                        b.qual2, b.len2)
    chunk.bc = (np.arange(pairs) % 7).astype(np.uint8)
    chunk.bc[::50] = abi.CS_DEMUX_NONE
    print(json.dumps({"ready": str(Path(fastq.__file__).resolve().parents[1])}), flush=True)
    for _line in sys.stdin:
        out = {}
        for form, n_bins in FORMS:
            gz = [[False, False] for _ in range(3 + n_bins)]
            t0 = time.perf_counter()
            blobs, counts = fastq.finish_chunk(chunk, tp, res1, None, res2, gz, n_bins=n_bins)
            out[form] = (time.perf_counter() - t0) * 1e3
            out[form + "_bytes"] = sum(x.n if isinstance(x, fastq.Lease) else len(x) for row in blobs for x in row if x)
            assert sum(counts) == pairs
            for row in blobs:
                for blob in row:
                    if isinstance(blob, fastq.Lease):
                        blob.release()
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.pairs)
    trees = {"this": str(ROOT)}
    if args.tree:
        trees["other"] = str(Path(args.tree).resolve())
    procs = {k: subprocess.Popen([sys.executable, __file__, "--worker", t, "--pairs", str(args.pairs)], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True) for k, t in trees.items()}
    times = {k: {form: [] for form, _ in FORMS} for k in trees}
    try:
        for k, p in procs.items():
            print(json.dumps({"tree": k, **json.loads(p.stdout.readline())}), flush=True)
        for rnd in range(args.warmup + args.rounds):
            for k in (list(procs) if rnd % 2 == 0 else list(procs)[::-1]):  # the order within a round alternates too
                procs[k].stdin.write("go\n")
                procs[k].stdin.flush()
                r = json.loads(procs[k].stdout.readline())
                print(json.dumps({"tree": k, "round": rnd - args.warmup, **r}), flush=True)
                if rnd >= args.warmup:
                    for form, _ in FORMS:
                        times[k][form].append(r[form])
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait()
    summary = {k: {form: {"min": round(min(v), 2), "median": round(statistics.median(v), 2), "max": round(max(v), 2)}
                   for form, v in forms.items()} for k, forms in times.items()}
    if args.tree:
        summary["this_median_within_or_below_other_spread"] = {
            form: summary["this"][form]["median"] <= summary["other"][form]["max"] for form, _ in FORMS}
    print(json.dumps({"summary_ms": summary, "pairs": args.pairs, "rounds": args.rounds, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
