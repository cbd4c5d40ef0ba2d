#!/usr/bin/env python3
"""The text readers alone -- two ``TextReader`` threads drained side by side, blocks dropped: the "readers alone" leg of
tools/host_io_profile.py -- over the data set of tools/e2e_bench.py, for an A/B of two trees.  Needs no GPU.

  python tools/reader_loop_ab.py WORKDIR [--make PAIRS] [--tree DIR] [--forms plain,multi_gz,bgzf] [--runs 5] [--unpinned]

``--make``: write the data set first (what ``e2e_bench.py --keep --forms bgzf_to_gz`` leaves in its work directory:
plain text, multi-member gzip, BGZF).  ``--tree``: take ``cutseq_amd`` from another built checkout.  ``--unpinned``: an
ordinary arena stands in for the page-locked one (a machine without a GPU).  One JSON line per form, ``runs`` drains
each; the legs alternate as one process per tree and round over the same files (profiles/reader_loop_ab.log).
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FILES = {"plain": "plain_R%d.fastq", "multi_gz": "syn_R%d.fastq.gz", "bgzf": "bgzf_R%d.fastq.gz"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workdir")
    ap.add_argument("--make", type=int, default=0)
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--forms", type=lambda v: v.split(","), default=list(FILES))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--unpinned", action="store_true")
    opts = ap.parse_args()
    sys.path.insert(0, str(Path(opts.tree).resolve()))
    from cutseq_amd import codec, fastq, textio
    work = Path(opts.workdir)
    if opts.make:
        sys.path.insert(1, str(ROOT))
        from tools import e2e_bench
        work.mkdir(parents=True, exist_ok=True)
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_fastq.py"), str(opts.make), str(work / "syn")], check=True)
        for m in (1, 2):
            src = codec.GzipSource(str(work / (FILES["multi_gz"] % m)), None, fastq.ARENA.take, fastq.ARENA.give)
            with open(work / (FILES["plain"] % m), "wb") as dst:
                for arr, nbytes in src.blocks():
                    dst.write(memoryview(arr)[:nbytes])
                    fastq.ARENA.give(arr)
            src.close()
        e2e_bench.write_bgzf([str(work / (FILES["plain"] % m)) for m in (1, 2)], [str(work / (FILES["bgzf"] % m)) for m in (1, 2)])
    if opts.unpinned:
        fastq.PINNED = fastq._Arena()
    for form in opts.forms:
        ins = [str(work / (FILES[form] % m)) for m in (1, 2)]
        rates = []
        for _ in range(opts.runs):
            t0 = time.perf_counter()
            readers = [textio.TextReader(p, 262144) for p in ins]
            got = 0
            while True:
                blocks = [r.get() for r in readers]
                if blocks[0] is None:
                    break
                got += blocks[0].n
                for b in blocks:
                    b.release()
            rates.append(round(got / (time.perf_counter() - t0) / 1e6, 2))
        print(json.dumps({"tree": str(Path(textio.__file__).resolve().parents[1]), "form": form, "pairs": got,
                          "cpus": len(os.sched_getaffinity(0)), "M_pairs_per_s": rates}), flush=True)


if __name__ == "__main__":
    main()
