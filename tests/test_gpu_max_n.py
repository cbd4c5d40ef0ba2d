"""--max-n (cutadapt's TooManyN) on the GPU: the scan / resolve kernels and the long-read kernel flag the reads
(cs_reads.xflags, cs_stats.n_too_many_n), the text path and the host chunk path discard the pairs, the CLI reports
them.  The oracle knows nothing of the filter: expectations are the oracle's intervals with the rule of
tests/maxn_rule.py applied."""
import gzip
import json
import random

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, run as cli, synth, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig
from cutseq_amd.engine import TrimEngine

import maxn_rule
import util

pytestmark = pytest.mark.gpu

COUNTS = [0.0, 0.02, 0.1, 1.0, 3.0]


def with_n(batch, seed, soft=True):
    """N runs at both ends of a third of the reads (trimming then changes the count), soft-masked 'n' here and there."""
    rng = np.random.default_rng(seed)
    for seq, lens in ((batch.seq1, batch.len1), (batch.seq2, batch.len2)):
        if seq is None:
            continue
        for i in np.nonzero(rng.random(batch.n) < 0.33)[0]:
            L = int(lens[i])
            a, b = int(rng.integers(0, 6)), int(rng.integers(0, 30))
            seq[i, :min(a, L)] = ord("N")
            seq[i, max(L - b, 0):L] = ord("N")
        if soft:
            for i in np.nonzero(rng.random(batch.n) < 0.05)[0]:
                j = int(rng.integers(0, max(int(lens[i]), 1)))
                if seq[i, j] == ord("N"):
                    seq[i, j] = ord("n")
    return batch


def run_engine(tp, batch):
    n = batch.n
    xf1 = np.full(n, 0xAA, dtype=np.uint8)
    xf2 = np.full(n, 0xAA, dtype=np.uint8) if tp.paired else None
    with TrimEngine(tp, device=0, slots=1, max_reads=max(n, 1), max_stride=batch.stride) as eng:
        g1, gcap2, g2 = eng.submit(0, batch.seq1, batch.qual1, batch.len1, batch.seq2, batch.qual2, batch.len2,
                                   xflags=(xf1, xf2))
        eng.wait(0)
        st = eng.stats()
    return g1, g2, xf1, xf2, st


def check_against_oracle(tp, batch, counts=COUNTS):
    (o1, _c, _s1), m2 = util.oracle_run(tp, batch, threads=8)
    for count in counts:
        tp.max_n = count
        g1, g2, xf1, xf2, st = run_engine(tp, batch)
        assert np.array_equal(g1, o1), count
        w1 = maxn_rule.xflags(batch.seq1, o1, count)
        assert np.array_equal(xf1, w1), (count, np.nonzero(xf1 != w1)[0][:5])
        assert st[0].n_too_many_n == int((w1 != 0).sum())
        if tp.paired:
            assert np.array_equal(g2, m2[0])
            w2 = maxn_rule.xflags(batch.seq2, m2[0], count)
            assert np.array_equal(xf2, w2), (count, np.nonzero(xf2 != w2)[0][:5])
            assert st[1].n_too_many_n == int((w2 != 0).sum())
    tp.max_n = None
    g1, g2, xf1, xf2, st = run_engine(tp, batch)  # no filter: xflags not written, nothing counted
    assert np.array_equal(g1, o1) and (xf1 == 0xAA).all() and st[0].n_too_many_n == 0


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("preset", sorted(BUILDIN_ADAPTERS))
def test_device_api_every_preset(preset, paired):
    st = planmod.CutadaptConfig()
    tp = util.compile_plan(BUILDIN_ADAPTERS[preset], st, paired)
    batch = with_n(synth.generate_pairs(30000, 150, scheme=BUILDIN_ADAPTERS[preset], seed=11, n_rate=0.03),
                   seed=sum(preset.encode()))
    if not paired:
        batch.seq2 = batch.qual2 = batch.len2 = None
    check_against_oracle(tp, batch)


def test_exact_tile_fallback_zero_padding_iupac_and_case_sensitive():
    st = planmod.CutadaptConfig()
    batch = with_n(synth.generate_pairs(20000, 150, scheme=BUILDIN_ADAPTERS["TAKARAV3"], seed=5, n_rate=0.03), seed=6)
    rng = np.random.default_rng(7)
    for seq, lens in ((batch.seq1, batch.len1), (batch.seq2, batch.len2)):
        for i in range(batch.n):
            seq[i, int(lens[i]):] = 0  # zero padding: every tile falls back to the exact form
        for i in np.nonzero(rng.random(batch.n) < 0.05)[0]:
            seq[i, int(rng.integers(0, int(lens[i])))] = ord(rng.choice(list("RYKMSWBDHV")))
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True)
    check_against_oracle(tp, batch, counts=[0.0, 0.1, 2.0])
    st.case_rule = abi.CS_CASE_SENSITIVE
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True)
    check_against_oracle(tp, batch, counts=[0.0, 0.1, 2.0])


def test_proportion_boundary_every_length_and_count():
    """An adapter that never matches: the interval is the whole read.  Every length 0..stride, every N count."""
    stride = 152
    reads = []
    for L in range(stride + 1):
        for n in range(L + 1):
            reads.append(("N" * n + "A" * (L - n), "I" * L))
    batch = util.batch_from_reads(reads)
    tp = planmod.single_adapter_plan("G" * 20, max_error_rate=0.0, min_overlap=20)
    for count in (1e-9, 0.1, 1 / 3, 0.2, 0.7, 0.999999):
        tp.max_n = count
        g1, _g2, xf1, _xf2, st = run_engine(tp, batch)
        want = np.array([(r[0].count("N") / len(r[0]) > count) if r[0] else False for r in reads], dtype=np.uint8)
        assert np.array_equal(xf1, want), (count, np.nonzero(xf1 != want)[0][:5])
        assert st[0].n_too_many_n == int(want.sum())


def fastq_text(names, seqs, quals):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(names, seqs, quals))


def test_long_reads_through_the_text_path():
    rng = random.Random(3)
    st = planmod.CutadaptConfig()
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, False)
    seqs, quals = [], []
    for i in range(12):
        L = rng.choice([200, 1000, 5000, 40000, 300000])
        s = bytearray(rng.choice(b"ACGT") for _ in range(L))
        for _ in range(rng.randint(0, 3)):  # N runs across the trim points (both ends) and inside
            a = rng.randint(0, L - 1)
            k = min(rng.randint(1, 400), L - a)
            s[a:a + k] = b"N" * k
        k = rng.randint(0, 8)
        s[:k] = b"N" * k
        assert len(s) == L
        seqs.append(bytes(s))
        quals.append(bytes(rng.choice(b"#5?I") for _ in range(L)))
    names = [b"long%d" % i for i in range(len(seqs))]
    # expected: the string-level restatement (no 16-bit length limit), then the rule on each kept interval
    from oracle import pyref
    pipe = pyref.SinglePipeline(BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), util.to_pyref_settings(st))
    routes = {"trimmed": 0, "short": 1, "untrimmed": 2}
    out = []
    for i in range(len(seqs)):
        rt, o = pipe.process(pyref.Read(names[i].decode(), seqs[i].decode(), quals[i].decode()))
        out.append((routes[rt], o.fastq().encode(), o.sequence.encode()))
    text = fastq_text(names, seqs, quals)
    for count in (0.0, 0.001, 50.0):
        tp.max_n = count
        with TrimEngine(tp, device=0, slots=0) as eng:
            with textpath.TextEngine(eng, slots=1, max_text_bytes=len(text) + 1024, max_records=len(seqs),
                                     stride=152) as te:
                streams, counts = te.run(text, len(seqs))
            st1, _ = eng.stats()
        x = [maxn_rule.too_many_n(kept_seq, count) for _rt, _rec, kept_seq in out]
        kept = [(rt, rec) for (rt, rec, _), xi in zip(out, x) if not (xi and rt != 1)]
        for r in range(3):
            assert streams[r][0] == b"".join(rec for rt, rec in kept if rt == r), (count, r)
        assert st1.n_too_many_n == sum(x)
        assert sum(counts) == len(kept)
        assert len(kept) < len(out) or count == 50.0


# ---- the command line ------------------------------------------------------------------------------------------

R1 = str(util.GOLDEN / "fixture1k_R1.fq.gz")
R2 = str(util.GOLDEN / "fixture1k_R2.fq.gz")


def n_inputs(tmp_path, fasta=False):
    """The 1000-pair fixture with N runs at the read ends of every fourth pair, written gzip (or FASTA, mate 1)."""
    rec = [util.read_fastq_gz(R1), util.read_fastq_gz(R2)]
    rng = random.Random(9)
    for m in range(2):
        for i in range(0, len(rec[m]), 4):
            n, s, q = rec[m][i]
            k = rng.randint(1, 12)
            s = (b"N" * k + s[k:]) if rng.random() < 0.5 else (s[:-k] + b"n" * k)
            rec[m][i] = (n, s, q)
    paths = []
    for m in range(2):
        p = tmp_path / (f"in{m + 1}.fa" if fasta else f"in{m + 1}.fq.gz")
        if fasta:
            p.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _q in rec[m]))
        else:
            with gzip.open(p, "wb") as fh:
                fh.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in rec[m]))
        paths.append(str(p))
    return rec, paths


def expect(tp, rec1, rec2, count):
    """-> streams[route] = (R1 bytes, R2 bytes | None), discarded pairs."""
    batch = util.batch_from_records(rec1, rec2)
    (o1, cap2, _), m2 = util.oracle_run(tp, batch, threads=8)
    o2 = m2[0] if m2 else None
    out = util.format_batch(tp, batch, [r[0] for r in rec1], [r[0] for r in rec2] if rec2 else None, o1, cap2, o2)
    x1 = maxn_rule.xflags(batch.seq1, o1, count) if count is not None else np.zeros(batch.n, np.uint8)
    x2 = maxn_rule.xflags(batch.seq2, o2, count) if (count is not None and o2 is not None) else np.zeros(batch.n, np.uint8)
    streams = [[b"", b""] for _ in range(3)]
    gone = 0
    for i, (rt, a, b) in enumerate(out):
        if rt != 1 and (x1[i] | x2[i]):
            gone += 1
            continue
        streams[rt][0] += a
        if b is not None:
            streams[rt][1] += b
    return streams, gone


def gunzip(p):
    with gzip.open(p, "rb") as fh:
        return fh.read()


def run_cli(tmp_path, tag, inputs, extra):
    pre = str(tmp_path / tag)
    cli.main(inputs + ["-A", "TAKARAV3", "-O", pre, "--json-file", pre + ".json"] + extra)
    rep = json.loads(open(pre + ".json").read())
    files = {}
    for kind in ("trimmed", "short", "untrimmed"):
        for m in (1, 2):
            p = f"{pre}_{kind}_R{m}.fastq.gz"
            try:
                files[(kind, m)] = gunzip(p)
            except FileNotFoundError:
                pass
    return files, rep


def test_cli_paired_text_path_host_path_ranks(tmp_path, monkeypatch):
    """TAKARAV3 paired, gz in and out, explicit -s and -u, --ensure-inline-barcode, --max-n 0.05: the text path, the
    host chunk path and --ranks 2 write the same files and counts, those of the oracle's intervals and the rule."""
    (rec1, rec2), paths = n_inputs(tmp_path)
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    st.max_n = 0.05
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True, untrimmed_requested=True)
    want, gone = expect(tp, rec1, rec2, 0.05)
    assert gone > 0
    results = []
    for tag, env, more in (("text", None, []), ("host", "0", []), ("ranks", None, ["--ranks", "2"])):
        if env is not None:
            monkeypatch.setenv("CUTSEQ_TEXT_PATH", env)
        else:
            monkeypatch.delenv("CUTSEQ_TEXT_PATH", raising=False)
        if tag == "ranks":
            monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
        short = [str(tmp_path / f"{tag}_s{m}.fq.gz") for m in (1, 2)]
        untr = [str(tmp_path / f"{tag}_u{m}.fq.gz") for m in (1, 2)]
        files, rep = run_cli(tmp_path, tag, paths, ["--ensure-inline-barcode", "-s", *short, "-u", *untr,
                                                    "--max-n", "0.05"] + more)
        monkeypatch.delenv("CUTSEQ_DEVICES", raising=False)
        assert files[("trimmed", 1)] == want[0][0] and files[("trimmed", 2)] == want[0][1], tag
        assert gunzip(short[0]) == want[1][0] and gunzip(short[1]) == want[1][1], tag
        assert gunzip(untr[0]) == want[2][0] and gunzip(untr[1]) == want[2][1], tag
        rc = rep["read_counts"]
        assert rc["filtered"]["too_many_n"] == gone, tag
        assert rc["input"] == rc["output"] + rc["filtered"]["too_short"] + rep["engine"]["is_untrimmed_any"] + gone
        assert rep["basepair_counts"]["output_read1"] == sum(len(l) for l in want[0][0].split(b"\n")[1::4])
        results.append((files, rc))
    assert results[0][1] == results[1][1] == results[2][1]


def test_cli_max_n_zero_drops_every_pair_with_n(tmp_path):
    (_rec1, _rec2), paths = n_inputs(tmp_path)
    files, rep = run_cli(tmp_path, "z", paths, ["--max-n", "0"])
    for m in (1, 2):
        seqs = files[("trimmed", m)].split(b"\n")[1::4]
        assert seqs and not any(b"N" in s.upper() for s in seqs)
    assert rep["read_counts"]["filtered"]["too_many_n"] > 0


@pytest.mark.parametrize("fasta", [False, True])
def test_cli_single_end_auto_rc_and_fasta(tmp_path, fasta):
    (rec1, _rec2), paths = n_inputs(tmp_path, fasta=fasta)
    st = planmod.CutadaptConfig()
    st.auto_rc = True
    st.max_n = 2
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, False)
    fa = [str(tmp_path / "se.fa"), str(tmp_path / "se_short.fa")]
    files, rep = run_cli(tmp_path, "se", paths[:1], ["--auto-rc", "--max-n", "2"] + (["-o", fa[0], "-s", fa[1]] if fasta else []))
    if fasta:  # FASTA in: FASTA records out (.fa names), qualities are not part of the comparison
        rec1 = [(n, s, b"I" * len(s)) for n, s, _q in rec1]
    want, gone = expect(tp, rec1, None, 2)
    got = open(fa[0], "rb").read() if fasta else files[("trimmed", 1)]
    if fasta:
        wl = want[0][0].split(b"\n")
        want_fa = b"".join(b">" + wl[i][1:] + b"\n" + wl[i + 1] + b"\n" for i in range(0, len(wl) - 1, 4))
        assert got == want_fa
    else:
        assert got == want[0][0]
    assert rep["read_counts"]["filtered"]["too_many_n"] == gone


def test_cli_flag_off_is_unchanged(tmp_path):
    (rec1, rec2), paths = n_inputs(tmp_path)
    files, rep = run_cli(tmp_path, "off", paths, [])
    st = planmod.CutadaptConfig()
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True)
    want, gone = expect(tp, rec1, rec2, None)
    assert gone == 0
    assert files[("trimmed", 1)] == want[0][0] and files[("trimmed", 2)] == want[0][1]
    assert files[("short", 1)] == want[1][0] and files[("short", 2)] == want[1][1]
    assert rep["read_counts"]["filtered"]["too_many_n"] is None
    assert rep["read_counts"]["input"] == rep["read_counts"]["output"] + rep["read_counts"]["filtered"]["too_short"]


@pytest.mark.parametrize("switch", ["", "CUTSEQ_TEXT_PATH=0"])
def test_cli_demultiplexing_run(tmp_path, monkeypatch, switch):
    """--demux-barcodes with --max-n 0.02 (the text path's format kernels for barcode routes, or the host formatter):
    every barcode's files hold what a one-barcode --ensure-inline-barcode run keeps after the rule, and the counts of
    every route and of TooManyN are the rule applied to the oracle's intervals.  Both paths write the same files."""
    from test_gpu_demux import barcode_set, plant_barcodes, scheme_with

    rng = random.Random(17)
    length, count, n = 8, 8, 12_000
    codes = barcode_set(rng, count, length, 5)
    bnames = [f"bc{i}" for i in range(count)]
    batch = synth.generate_pairs(n, 150, scheme_with(codes[0]), seed=23, n_rate=0.02)
    plant_barcodes(rng, batch, codes, length)
    nrng = np.random.default_rng(5)
    for seq, lens in ((batch.seq1, batch.len1), (batch.seq2, batch.len2)):  # N runs behind the barcode and UMI
        for i in np.nonzero(nrng.random(n) < 0.3)[0]:
            L = int(lens[i])
            seq[i, max(L - int(nrng.integers(1, 30)), 40):L] = ord("N")
            seq[i, 40 + int(nrng.integers(0, 60))] = ord("n")
    names1 = [f"SIM:{i} 1:N:0:X".encode() for i in range(n)]
    names2 = [f"SIM:{i} 2:N:0:X".encode() for i in range(n)]
    in1, in2 = str(tmp_path / "d_R1.fastq.gz"), str(tmp_path / "d_R2.fastq.gz")
    util.write_fastq(in1, names1, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(in2, names2, batch.seq2, batch.qual2, batch.len2)
    table = tmp_path / "barcodes.tsv"
    table.write_text("".join(f"{a}\t{b}\n" for a, b in zip(bnames, codes)))

    # expected: one --ensure-inline-barcode run per barcode; a pair takes the intervals of the run whose barcode it
    # carries (of any run when it carries none), then TooShort > TooManyN > IsUntrimmedAny > its barcode's files
    count_max = 0.02
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    runs = []
    for code in codes:
        one = planmod.compile_paired(BarcodeConfig(scheme_with(code)), st)
        (o1, _, _), (o2, _, _) = util.oracle_run(one, batch, threads=8)
        recs = util.format_batch(one, batch, names1, names2, o1, None, o2)
        runs.append((o1, o2, recs, maxn_rule.xflags(batch.seq1, o1, count_max), maxn_rule.xflags(batch.seq2, o2, count_max)))
    want_bins = [[b"", b""] for _ in range(count)]
    want_counts = {"short": 0, "untrimmed": 0, "too_many_n": 0}
    bin_counts = [0] * count
    for i in range(n):
        hits = [b for b in range(count) if runs[b][0][i]["flags"] & abi.CS_F_INLINE]
        assert len(hits) <= 1
        src = hits[0] if hits else count - 1
        o1, o2, recs, x1, x2 = runs[src]
        rt = maxn_rule.route(int(o1[i]["flags"]), int(o2[i]["flags"]), int(x1[i]), int(x2[i]), True)
        if rt is None:
            want_counts["too_many_n"] += 1
        elif rt == 1:
            want_counts["short"] += 1
        elif rt == 2:
            want_counts["untrimmed"] += 1
        else:
            assert hits
            want_bins[src][0] += recs[i][1]
            want_bins[src][1] += recs[i][2]
            bin_counts[src] += 1
    assert want_counts["too_many_n"] > 0 and min(bin_counts) > 0

    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "4000")
    if switch:
        monkeypatch.setenv(*switch.split("="))
    prefix = str(tmp_path / "dm")
    cli.main(["-a", scheme_with(codes[0]), "--demux-barcodes", str(table), "-O", prefix, "--json-file",
              str(tmp_path / "r.json"), "--max-n", str(count_max), in1, in2])
    for b, name in enumerate(bnames):
        assert gunzip(f"{prefix}_{name}_trimmed_R1.fastq.gz") == want_bins[b][0], name
        assert gunzip(f"{prefix}_{name}_trimmed_R2.fastq.gz") == want_bins[b][1], name
    untr = gunzip(f"{prefix}_untrimmed_R1.fastq.gz")
    assert untr.count(b"\n") // 4 == want_counts["untrimmed"]
    assert gunzip(f"{prefix}_untrimmed_R2.fastq.gz").count(b"\n") // 4 == want_counts["untrimmed"]
    rep = json.loads((tmp_path / "r.json").read_text())
    rc = rep["read_counts"]
    assert rep["engine"]["demultiplexed"] == dict(zip(bnames, bin_counts))
    assert rc["output"] == sum(bin_counts)
    assert rc["filtered"]["too_short"] == want_counts["short"]
    assert rc["filtered"]["too_many_n"] == want_counts["too_many_n"]
    assert rc["input"] == n == rc["output"] + want_counts["short"] + want_counts["untrimmed"] + want_counts["too_many_n"]
    assert rep["basepair_counts"]["output_read1"] == sum(len(l) for b in range(count)
                                                        for l in want_bins[b][0].split(b"\n")[1::4])
