#!/usr/bin/env python3
"""Tier E through the product CLI, in-process, with start-up amortised.

  python tools/e2e_bench.py [pairs] [workdir] [--forms plain_warm,plain_to_gz] [--tree DIR] [--keep] [--extra='-M 100']

``--forms plain_to_gz_warm`` (only when named) runs plain -> gz twice in the process and reports the second run too, with
the bytes of the output files (``--extra='-t 16 --bgzf'`` against ``--extra='-t 16'``: profiles/bgzf_out_ab.log).
``--forms bgzf_to_gz`` (only when named) adds BGZF input: the same records bgzip-style, read with and without
``CUTSEQ_GPU_INFLATE=1`` (the caller sets it), once cold and once warm.
``--forms bam_to_gz`` (only when named) adds unaligned BAM input: the same records as R1.bam + R2.bam, written by the
tests' BAM rule in BGZF blocks of 65 280 bytes at zlib level 6, once cold and once warm (profiles/bam_input_ab.log).

Writes a synthetic paired data set once (plain text and multi-member gzip), then runs
``cutseq_amd.run.main`` on it: plain -> plain twice (the second run has warm buffers and page cache),
gz -> gz once.  Prints one JSON object.  Not the headline metric: bench.py reports the HBM-resident rate.

For an A/B of two commits on one machine: ``--forms`` runs only the named forms (``plain_warm`` brings its cold run
along), ``--tree DIR`` takes ``cutseq_amd`` from another built checkout (the data set is always written by this
tree's ``make_fastq.py``: both legs read the same files), ``--keep`` leaves the data set in the work directory (and
reuses the one that is there), so that the legs can alternate, one process each, over the same files.
profiles/fanout_ab.log was measured this way.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    if sys.argv[1:2] == ["--write-ubam"]:  # the child process of the bam_to_gz form: FASTQ FASTQ BAM BAM
        return write_ubam(sys.argv[2:4], sys.argv[4:6])
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=8_000_000)
    ap.add_argument("workdir", nargs="?", default="/dev/shm/cutseq_e2e")
    ap.add_argument("--forms", type=lambda v: v.split(","), default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--extra", type=lambda v: v.split(), default=[],
                    help="more command-line options for every run, e.g. --extra='-M 100 --max-ee 1'")
    opts = ap.parse_args()
    if opts.tree:
        sys.path.insert(0, str(Path(opts.tree).resolve()))
    n = opts.pairs
    # the steady-state regime: blocks of 262 144 records, what inputs of 25 M pairs and more get (smaller inputs get
    # smaller blocks -- a fresh process spends more time page-locking big buffers than it saves: tools/cold_runs.py)
    os.environ.setdefault("CUTSEQ_CHUNK_READS", "262144")
    work = Path(opts.workdir)
    work.mkdir(parents=True, exist_ok=True)
    free = shutil.disk_usage(work).free
    need = n * 2 * 340 * 3
    if free < need:
        raise SystemExit(f"{work}: {free >> 20} MiB free, {need >> 20} MiB needed for {n} pairs")
    out = {"pairs": n, "workdir": str(work), "cpus": len(os.sched_getaffinity(0)), "extra": opts.extra}
    from cutseq_amd import codec, fastq, run as cli
    out["tree"] = str(Path(cli.__file__).resolve().parents[1])
    have = opts.keep and all((work / f"{stem}_R{m}.{end}").exists() for m in (1, 2) for stem, end in (("syn", "fastq.gz"), ("plain", "fastq")))
    t0 = time.perf_counter()
    if not have:
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_fastq.py"), str(n), str(work / "syn")], check=True)
    out["make_gz_s"] = round(time.perf_counter() - t0, 2)

    t0 = time.perf_counter()
    for m in () if have else (1, 2):  # plain copies of the same records
        src = codec.GzipSource(str(work / f"syn_R{m}.fastq.gz"), None, fastq.ARENA.take, fastq.ARENA.give)
        with open(work / f"plain_R{m}.fastq", "wb") as dst:
            for arr, nbytes in src.blocks():
                dst.write(memoryview(arr)[:nbytes])
                fastq.ARENA.give(arr)
        src.close()
    out["gunzip_s"] = round(time.perf_counter() - t0, 2)

    plain_in = [str(work / "plain_R1.fastq"), str(work / "plain_R2.fastq")]
    bam_in = [str(work / f"ubam_R{m}.bam") for m in (1, 2)]
    if opts.forms and "bam_to_gz" in opts.forms and not (opts.keep and all(Path(p).exists() for p in bam_in)):
        # in a process of its own, like make_fastq.py, and before this one runs anything: the writer's process pool must
        # not be forked from a process that holds a GPU
        t0 = time.perf_counter()
        subprocess.run([sys.executable, str(Path(__file__).resolve()), "--write-ubam", *plain_in, *bam_in], check=True)
        out["make_bam_s"] = round(time.perf_counter() - t0, 2)

    def run(tag, inputs, outputs):
        if opts.forms and tag not in opts.forms and not (tag == "plain_cold" and "plain_warm" in opts.forms) \
                and not (tag == "bgzf_to_gz_warm" and "bgzf_to_gz" in opts.forms) \
                and not (tag == "bam_to_gz_warm" and "bam_to_gz" in opts.forms) \
                and not (tag == "plain_to_gz" and "plain_to_gz_warm" in opts.forms):
            return
        for old in work.glob("o[12].fastq"), work.glob("s[12].fastq"), work.glob("gzout_*"):
            for f in old:  # a run writes NEW files: freeing the previous run's gigabytes of tmpfs pages is not its job
                f.unlink()
        t0 = time.perf_counter()
        try:
            cli.main(["-A", "TAKARAV3", "--trim-polyA"] + opts.extra + inputs + outputs)
        except SystemExit as exc:  # pragma: no cover
            if exc.code:
                raise
        dt = time.perf_counter() - t0
        out[tag] = {"seconds": round(dt, 3), "M_pairs_per_s": round(n / dt / 1e6, 3)}


    plain_out = ["-o", str(work / "o1.fastq"), str(work / "o2.fastq"), "-s", str(work / "s1.fastq"), str(work / "s2.fastq")]
    run("plain_cold", plain_in, plain_out)
    run("plain_warm", plain_in, plain_out)
    gz_in = [str(work / "syn_R1.fastq.gz"), str(work / "syn_R2.fastq.gz")]
    run("gz_to_gz", gz_in, ["-O", str(work / "gzout")])
    run("gz_to_gz_warm", gz_in, ["-O", str(work / "gzout")])
    run("plain_to_gz", plain_in, ["-O", str(work / "gzout")])
    if opts.forms and "plain_to_gz_warm" in opts.forms:
        run("plain_to_gz_warm", plain_in, ["-O", str(work / "gzout")])
        out["plain_to_gz_warm"]["output_bytes"] = {f.name: f.stat().st_size for f in sorted(work.glob("gzout_*"))}
    if opts.forms and "bgzf_to_gz" in opts.forms:
        # bgzip'd input (what CUTSEQ_GPU_INFLATE=1 inflates on the device): written with the tests' BGZF writer -- there
        # is no bgzip here --, 65 280 bytes of text per block at zlib level 6 (bgzip's default), the pool compressing
        bgzf_in = [str(work / f"bgzf_R{m}.fastq.gz") for m in (1, 2)]
        if not (opts.keep and all(Path(p).exists() for p in bgzf_in)):
            write_bgzf(plain_in, bgzf_in)
        run("bgzf_to_gz", bgzf_in, ["-O", str(work / "gzout")])
        run("bgzf_to_gz_warm", bgzf_in, ["-O", str(work / "gzout")])
    if opts.forms and "bam_to_gz" in opts.forms:
        out["bam_bytes"] = [Path(p).stat().st_size for p in bam_in]
        run("bam_to_gz", bam_in, ["-O", str(work / "gzout")])
        run("bam_to_gz_warm", bam_in, ["-O", str(work / "gzout")])
    # the usual sequencer output: ONE gzip member per file (gzip -1 of the first half of the records), which no
    # reader can enter in the middle
    n_single = n // 2
    if opts.forms and "single_member_gz_to_gz" not in opts.forms:
        return finish(work, out, opts.keep)
    t0 = time.perf_counter()
    procs = []
    for m in (1, 2):
        head = subprocess.Popen(["head", "-n", str(4 * n_single), str(work / f"plain_R{m}.fastq")], stdout=subprocess.PIPE)
        procs.append((head, subprocess.Popen(["gzip", "-1"], stdin=head.stdout, stdout=open(work / f"single_R{m}.fastq.gz", "wb"))))
    for head, gz in procs:
        gz.wait()
        head.wait()
    out["make_single_member_gz_s"] = round(time.perf_counter() - t0, 2)
    n_all, n = n, n_single
    single_in = [str(work / "single_R1.fastq.gz"), str(work / "single_R2.fastq.gz")]
    run("single_member_gz_to_gz", single_in, ["-O", str(work / "gzout")])
    out["single_member_gz_to_gz"]["pairs"] = n_single
    n = n_all
    finish(work, out, opts.keep)


def write_bgzf(sources, targets, level=6, piece=64 * 65280):
    sys.path.insert(0, str(ROOT / "tests"))
    import bgzf_rule
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(os.sched_getaffinity(0))) as pool:
        for src, dst in zip(sources, targets):
            with open(src, "rb") as fin, open(dst, "wb") as fout:
                pending = []
                while True:
                    data = fin.read(piece)
                    if data:
                        pending.append(pool.submit(bgzf_rule.bgzf, data, 65280, level))
                    while pending and (not data or len(pending) > 64):
                        fout.write(pending.pop(0).result())
                    if not data:
                        break
                fout.write(bgzf_rule.EOF_MARKER)


def _bam_records(lines):
    """Pool job of write_ubam: the four-line records ``lines`` as BAM records, back to back."""
    import bam_rule
    minus33 = bytes((i - 33) & 0xFF for i in range(256))
    return b"".join(bam_rule.record_bytes(bam_rule.Rec(lines[i][1:-1], lines[i + 1][:-1], lines[i + 3][:-1].translate(minus33)))
                    for i in range(0, len(lines), 4))


def write_ubam(sources, targets, level=6, piece=64 * 65280, records=50_000):
    """Plain FASTQ files as unaligned BAM by tests/bam_rule.py: the records are built by a pool of processes, the stream is
    cut into BGZF blocks of 65 280 bytes wherever they fall, as samtools does, and compressed by a pool of threads; at
    most 16 of each.  Runs in a process of its own (``--write-ubam``) that never opens a GPU."""
    sys.path.insert(0, str(ROOT / "tests"))
    import itertools
    import bam_rule
    from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
    cpus = min(16, len(os.sched_getaffinity(0)))
    with ProcessPoolExecutor(cpus) as procs, ThreadPoolExecutor(cpus) as threads:
        for src, dst in zip(sources, targets):
            with open(src, "rb") as fin, open(dst, "wb") as fout:
                stream, blocks, jobs = bytearray(bam_rule.header_bytes(b"@HD\tVN:1.6\tSO:unsorted\n")), [], []

                def drain(everything):
                    while len(stream) >= piece or (everything and stream):
                        blocks.append(threads.submit(bam_rule.bgzf_rule.bgzf, bytes(stream[:piece]), 65280, level))
                        del stream[:piece]
                    while blocks and (everything or len(blocks) > 4 * cpus):
                        fout.write(blocks.pop(0).result())

                while True:
                    lines = list(itertools.islice(fin, 4 * records))
                    if lines:
                        jobs.append(procs.submit(_bam_records, lines))
                    while jobs and (not lines or len(jobs) > 2 * cpus):
                        stream += jobs.pop(0).result()
                        drain(False)
                    if not lines:
                        break
                drain(True)
                fout.write(bam_rule.bgzf_rule.EOF_MARKER)


def finish(work, out, keep):
    if not keep:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
