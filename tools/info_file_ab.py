#!/usr/bin/env python3
"""What --info-file costs, through the product CLI: plain FASTQ in, .gz records out, fresh processes.

  python tools/info_file_ab.py [--pairs 8000000] [--rounds 3] [--parent DIR] [--workdir DIR]

Legs, alternating inside every round (one box, same files, page cache warm after an unmeasured first run):
  parent_off   the same command from the tree at --parent (a built checkout of the parent commit), if given
  off          this tree, no --info-file
  on_plain     this tree, --info-file info.tsv
  on_gz        this tree, --info-file info.tsv.gz (deflated on the device)
Prints one JSON line per run and a summary -- medians, the spread of the parent's own rounds, whether the median of
`off` lies inside it, and the on / off ratios -- and appends the same lines to --log (default
profiles/info_file_ab.log).  Only the files this tool wrote are removed from --workdir.  Kernel times per block come
from a run of its own under rocprofv3 --kernel-trace --stats (tools/text_profile.sh shows the form).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LOG = None  # open log file


def emit(obj) -> None:
    line = json.dumps(obj)
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def run(tree: Path, work: Path, extra, tag: str, n: int) -> dict:
    for old in work.glob("out_*"):
        old.unlink()
    for old in work.glob("info.tsv*"):
        old.unlink()
    cmd = [sys.executable, "-m", "cutseq_amd.run", "-A", "TAKARAV3", "--trim-polyA", "-O", str(work / "out"),
           str(work / "plain_R1.fastq"), str(work / "plain_R2.fastq")] + extra
    env = dict(os.environ, PYTHONPATH=str(tree), CUTSEQ_PROGRESS="0")
    env.setdefault("CUTSEQ_CHUNK_READS", "262144")
    t0 = time.perf_counter()
    subprocess.run(cmd, cwd=tree, env=env, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    info = next(iter(work.glob("info.tsv*")), None)
    res = {"leg": tag, "seconds": round(dt, 3), "M_pairs_per_s": round(n / dt / 1e6, 3),
           "info_bytes": info.stat().st_size if info else 0}
    emit(res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", type=str, default=None)
    ap.add_argument("--workdir", type=str, default="/dev/shm/cutseq_info_ab")
    ap.add_argument("--log", type=str, default=str(ROOT / "profiles" / "info_file_ab.log"))
    args = ap.parse_args()
    global LOG
    LOG = open(args.log, "a")
    n, work = args.pairs, Path(args.workdir)
    made_dir = not work.exists()
    work.mkdir(parents=True, exist_ok=True)
    emit({"tool": "tools/info_file_ab.py", "command": "cutseq -A TAKARAV3 --trim-polyA -O out plain_R1.fastq plain_R2.fastq "
          "[--info-file info.tsv[.gz]]", "pairs": n, "rounds": args.rounds, "block_records": os.environ.get("CUTSEQ_CHUNK_READS", "262144")})
    sys.path.insert(0, str(ROOT))
    subprocess.run([sys.executable, str(ROOT / "tools" / "make_fastq.py"), str(n), str(work / "syn")], check=True)
    from cutseq_amd import codec, fastq
    for m in (1, 2):
        src = codec.GzipSource(str(work / f"syn_R{m}.fastq.gz"), None, fastq.ARENA.take, fastq.ARENA.give)
        with open(work / f"plain_R{m}.fastq", "wb") as dst:
            for arr, nbytes in src.blocks():
                dst.write(memoryview(arr)[:nbytes])
                fastq.ARENA.give(arr)
        src.close()
        (work / f"syn_R{m}.fastq.gz").unlink()
    legs = [("off", ROOT, []), ("on_plain", ROOT, ["--info-file", str(work / "info.tsv")]),
            ("on_gz", ROOT, ["--info-file", str(work / "info.tsv.gz")])]
    if args.parent:
        legs.insert(0, ("parent_off", Path(args.parent).resolve(), []))
    run(ROOT, work, [], "warmup", n)
    got = {tag: [] for tag, _, _ in legs}
    for _ in range(args.rounds):
        for tag, tree, extra in legs:
            got[tag].append(run(tree, work, extra, tag, n))
    med = {tag: statistics.median(r["seconds"] for r in rs) for tag, rs in got.items()}
    summary = {"pairs": n, "rounds": args.rounds, "median_seconds": med,
               "on_plain_over_off": round(med["on_plain"] / med["off"], 3), "on_gz_over_off": round(med["on_gz"] / med["off"], 3),
               "info_bytes": {tag: rs[-1]["info_bytes"] for tag, rs in got.items() if tag.startswith("on")}}
    if args.parent:
        lo, hi = min(r["seconds"] for r in got["parent_off"]), max(r["seconds"] for r in got["parent_off"])
        summary["parent_spread_seconds"] = [lo, hi]
        summary["off_median_inside_parent_spread"] = lo <= med["off"] <= hi
    emit({"summary": summary})
    for pattern in ("plain_R[12].fastq", "out_*", "info.tsv*"):  # what this tool wrote, nothing else
        for f in work.glob(pattern):
            f.unlink()
    if made_dir:
        try:
            work.rmdir()
        except OSError:
            pass


if __name__ == "__main__":
    main()
