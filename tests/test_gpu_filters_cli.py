"""-M/--max-length, --max-ee and --max-n together on the text path and the command line: the output files are the
string pipeline's records (oracle/pyref.py) with the pairs removed that tests/filters_rule.py discards, and the counts of
the stderr line and the JSON report are the rule's -- on the text path, the host chunk path and under --ranks 2, with
--info-file, with --demux-barcodes, and single-end with --auto-rc (where cutadapt's filters see the read turned
round)."""
import gzip
import json
import math
import random
import statistics

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, run as cli, synth
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig

import filters_rule
import maxn_rule
import util
from test_gpu_filters import order_sensitive

pytestmark = pytest.mark.gpu

R1 = str(util.GOLDEN / "fixture1k_R1.fq.gz")
R2 = str(util.GOLDEN / "fixture1k_R2.fq.gz")
NAMES = [name for name, _bit in filters_rule.ORDER]


def inputs(tmp_path):
    """The 1000-pair fixture with N runs at the read ends of every fourth pair, written gzip."""
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
        p = tmp_path / f"in{m + 1}.fq.gz"
        with gzip.open(p, "wb") as fh:
            fh.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in rec[m]))
        paths.append(str(p))
    return rec, paths


_RECORDS = {}


def pipeline_records(st, rec1, rec2, untrimmed_requested=False):
    """The string pipeline, no filter: [(route, record 1, record 2 | None)].  Computed once per setting (``inputs``
    gives the same records every time) and shared by the tests; nobody changes the list."""
    key = (st.ensure_inline_barcode, st.auto_rc, rec2 is not None, untrimmed_requested)
    if key not in _RECORDS:
        batch = util.batch_from_records(rec1, rec2)
        _RECORDS[key] = util.pyref_run(BUILDIN_ADAPTERS["TAKARAV3"], st, batch, [r[0] for r in rec1],
                                       [r[0] for r in rec2] if rec2 is not None else None, untrimmed_requested)
    return _RECORDS[key]


def bits_of(record: bytes, max_length, max_n, max_ee) -> int:
    """The CS_X_* bits of one final read, taken from its output record."""
    _name, seq, _plus, qual = record.split(b"\n")[:4]
    x = 0
    if max_length is not None and filters_rule.too_long(len(seq), max_length):
        x |= abi.CS_X_TOO_LONG
    if max_n is not None and maxn_rule.too_many_n(seq, max_n):
        x |= abi.CS_X_TOO_MANY_N
    if max_ee is not None and filters_rule.too_many_ee(qual, max_ee):
        x |= abi.CS_X_TOO_MANY_EE
    return x


def apply_rule(records, max_length=None, max_n=None, max_ee=None):
    """-> streams[route][mate], {filter: pairs}, the pair bits of the pairs TooShort did not take."""
    streams = [[b"", b""] for _ in range(3)]
    gone = dict.fromkeys(NAMES, 0)
    pair_bits = []
    for rt, a, b in records:
        x1 = bits_of(a, max_length, max_n, max_ee)
        x2 = bits_of(b, max_length, max_n, max_ee) if b is not None else 0
        where = filters_rule.route(abi.CS_F_TOO_SHORT if rt == 1 else (abi.CS_F_UNTRIMMED if rt == 2 else 0), 0, x1, x2, True)
        if rt != 1:
            pair_bits.append(x1 | x2)
        if where in gone:
            gone[where] += 1
            continue
        assert where == rt
        streams[rt][0] += a
        if b is not None:
            streams[rt][1] += b
    return streams, gone, pair_bits


def thresholds(records):
    """Median final length and median expected errors over the reads of the pairs TooShort leaves."""
    lens, ees = [], []
    for rt, a, b in records:
        if rt == 1:
            continue
        for rec in (a, b):
            if rec is not None:
                lens.append(len(rec.split(b"\n")[1]))
                ees.append(filters_rule.expected_errors(rec.split(b"\n")[3]))
    return int(statistics.median(lens)), float(statistics.median(ees))


def gunzip(p):
    with gzip.open(p, "rb") as fh:
        return fh.read()


def stderr_line(err: str) -> dict:
    lines = err.splitlines()
    at = max(i for i, line in enumerate(lines) if line.startswith("status\t"))
    return dict(zip(lines[at].split("\t"), lines[at + 1].split("\t")))


def run_cli(tmp_path, capsys, tag, paths, extra):
    pre = str(tmp_path / tag)
    capsys.readouterr()
    cli.main(paths + ["-A", "TAKARAV3", "-O", pre, "--json-file", pre + ".json"] + extra)
    line = stderr_line(capsys.readouterr().err)
    rep = json.loads(open(pre + ".json").read())
    files = {}
    for kind in ("trimmed", "short", "untrimmed"):
        for m in (1, 2):
            try:
                files[(kind, m)] = gunzip(f"{pre}_{kind}_R{m}.fastq.gz")
            except FileNotFoundError:
                pass
    return files, rep, line


def check_counts(rep, line, gone, given, n):
    rc = rep["read_counts"]
    filtered = rc["filtered"]
    for key, name in (("too_long", "too_long"), ("too_many_n", "too_many_n"), ("too_many_expected_errors", "too_many_ee")):
        assert filtered[key] == (gone[name] if name in given else None), key
    assert line["too_long"] == str(gone["too_long"]) and line["too_many_n"] == str(gone["too_many_n"])
    untrimmed = rep["engine"]["is_untrimmed_any"] or 0
    assert rc["input"] == n == rc["output"] + filtered["too_short"] + untrimmed + sum(gone.values())
    assert line["in_reads"] == str(n) and line["out_reads"] == str(rc["output"])


def test_cli_paired_all_three_text_path_host_path_ranks(tmp_path, monkeypatch, capsys):
    """TAKARAV3 paired, gz in and out, -s and -u files, --ensure-inline-barcode; -M and --max-ee at the medians and
    --max-n 0, so that every overlap of the three filters occurs and the precedence decides the counts."""
    (rec1, rec2), paths = inputs(tmp_path)
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    records = pipeline_records(st, rec1, rec2, untrimmed_requested=True)
    max_length, max_ee = thresholds(records)
    want, gone, pair_bits = apply_rule(records, max_length, 0.0, max_ee)
    # every filter takes pairs and leaves pairs; every overlap that the precedence has to settle occurs
    assert all(gone[k] > 0 for k in NAMES) and sum(gone.values()) < len(pair_bits) and pair_bits.count(0) > 0
    for overlap in (3, 5, 6, 7):  # TooManyN|TooLong, TooManyN|TooManyEE, TooLong|TooManyEE, all three
        assert overlap in pair_bits, overlap
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
        files, rep, line = run_cli(tmp_path, capsys, tag, paths,
                                   ["--ensure-inline-barcode", "-s", *short, "-u", *untr, "-M", str(max_length),
                                    "--max-ee", repr(max_ee), "--max-n", "0"] + more)
        monkeypatch.delenv("CUTSEQ_DEVICES", raising=False)
        assert files[("trimmed", 1)] == want[0][0] and files[("trimmed", 2)] == want[0][1], tag
        assert gunzip(short[0]) == want[1][0] and gunzip(short[1]) == want[1][1], tag
        assert gunzip(untr[0]) == want[2][0] and gunzip(untr[1]) == want[2][1], tag
        check_counts(rep, line, gone, NAMES, len(rec1))
        assert rep["basepair_counts"]["output_read1"] == sum(len(l) for l in want[0][0].split(b"\n")[1::4])
        results.append((rep["read_counts"], line))
    assert results[0] == results[1] == results[2]


@pytest.mark.parametrize("which", ["too_long", "too_many_ee"])
def test_cli_paired_one_filter_alone(tmp_path, capsys, which):
    (rec1, rec2), paths = inputs(tmp_path)
    st = planmod.CutadaptConfig()
    records = pipeline_records(st, rec1, rec2)
    max_length, max_ee = thresholds(records)
    if which == "too_long":
        want, gone, _ = apply_rule(records, max_length=max_length)
        extra = ["--max-length", str(max_length)]
    else:
        want, gone, _ = apply_rule(records, max_ee=max_ee)
        extra = ["--max-expected-errors", repr(max_ee)]
    kept = want[0][0].count(b"\n") // 4
    assert gone[which] > 0 and kept > 0 and sum(gone.values()) == gone[which]
    files, rep, line = run_cli(tmp_path, capsys, which, paths, extra)
    assert files[("trimmed", 1)] == want[0][0] and files[("trimmed", 2)] == want[0][1]
    assert files[("short", 1)] == want[1][0] and files[("short", 2)] == want[1][1]
    check_counts(rep, line, gone, [which], len(rec1))


def test_cli_without_the_options_reports_none_and_zero(tmp_path, capsys):
    (rec1, rec2), paths = inputs(tmp_path)
    want, gone, _ = apply_rule(pipeline_records(planmod.CutadaptConfig(), rec1, rec2))
    files, rep, line = run_cli(tmp_path, capsys, "off", paths, [])
    assert files[("trimmed", 1)] == want[0][0] and files[("trimmed", 2)] == want[0][1]
    check_counts(rep, line, gone, [], len(rec1))


def test_cli_info_file_is_written_in_front_of_the_filters(tmp_path, capsys):
    (rec1, rec2), paths = inputs(tmp_path)
    records = pipeline_records(planmod.CutadaptConfig(), rec1, rec2)
    max_length, max_ee = thresholds(records)
    _want, gone, _ = apply_rule(records, max_length, None, max_ee)
    assert gone["too_long"] > 0 and gone["too_many_ee"] > 0
    plain, with_filters = str(tmp_path / "plain.tsv"), str(tmp_path / "filtered.tsv")
    _f, rep0, _l = run_cli(tmp_path, capsys, "i0", paths, ["--info-file", plain])
    _f, rep1, line = run_cli(tmp_path, capsys, "i1", paths, ["--info-file", with_filters, "-M", str(max_length),
                                                              "--max-ee", repr(max_ee)])
    table = open(plain, "rb").read()
    assert table and open(with_filters, "rb").read() == table  # discarded pairs keep their rows
    check_counts(rep1, line, gone, ["too_long", "too_many_ee"], len(rec1))
    assert rep1["read_counts"]["output"] < rep0["read_counts"]["output"]


@pytest.mark.parametrize("switch", ["", "CUTSEQ_TEXT_PATH=0"])
def test_cli_single_end_auto_rc_sums_in_the_order_of_the_written_read(tmp_path, monkeypatch, capsys, switch):
    """--auto-rc reverse-complements before cutadapt's filters: the expected errors are summed over the qualities as
    they are written.  --max-ee at the exact sum of one read keeps it, the next double below discards it -- and that
    read's sum differs when taken in the input's order."""
    (rec1, _rec2), paths = inputs(tmp_path)
    st = planmod.CutadaptConfig()
    st.auto_rc = True
    records = pipeline_records(st, rec1, None)
    quals = [a.split(b"\n")[3] for rt, a, _b in records if rt == 0]
    pick = next(q for q in quals if len(q) >= 100 and order_sensitive(q))
    exact = filters_rule.expected_errors(pick)
    assert exact != filters_rule.expected_errors(pick[::-1])
    if switch:
        monkeypatch.setenv(*switch.split("="))
    outs = []
    for tag, bound in (("at", exact), ("below", math.nextafter(exact, 0.0))):
        want, gone, _ = apply_rule(records, max_ee=bound)
        assert gone["too_many_ee"] > 0 and want[0][0]
        files, rep, line = run_cli(tmp_path, capsys, tag, paths[:1], ["--auto-rc", "--max-ee", repr(bound)])
        assert files[("trimmed", 1)] == want[0][0], tag
        check_counts(rep, line, gone, ["too_many_ee"], len(rec1))
        outs.append(gone["too_many_ee"])
    assert outs[1] == outs[0] + 1


@pytest.mark.parametrize("switch", ["", "CUTSEQ_TEXT_PATH=0"])
def test_cli_demultiplexing_run(tmp_path, monkeypatch, capsys, switch):
    """--demux-barcodes with -M, --max-n and --max-ee: every barcode's files hold what a one-barcode
    --ensure-inline-barcode run keeps after the rule; the counts of every route and filter are the rule's."""
    from test_gpu_demux import barcode_set, plant_barcodes, scheme_with

    rng = random.Random(17)
    length, count, n = 8, 4, 3000
    codes = barcode_set(rng, count, length, 5)
    bnames = [f"bc{i}" for i in range(count)]
    batch = synth.generate_pairs(n, 150, scheme_with(codes[0]), seed=23, n_rate=0.02)
    plant_barcodes(rng, batch, codes, length)
    names1 = [f"SIM:{i} 1:N:0:X".encode() for i in range(n)]
    names2 = [f"SIM:{i} 2:N:0:X".encode() for i in range(n)]
    in1, in2 = str(tmp_path / "d_R1.fastq.gz"), str(tmp_path / "d_R2.fastq.gz")
    util.write_fastq(in1, names1, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(in2, names2, batch.seq2, batch.qual2, batch.len2)
    table = tmp_path / "barcodes.tsv"
    table.write_text("".join(f"{a}\t{b}\n" for a, b in zip(bnames, codes)))

    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    runs = []
    for code in codes:
        one = planmod.compile_paired(BarcodeConfig(scheme_with(code)), st)
        (o1, _, _), (o2, _, _) = util.oracle_run(one, batch, threads=8)
        runs.append((o1, o2, util.format_batch(one, batch, names1, names2, o1, None, o2)))
    spans = np.concatenate([o["stop"].astype(int) - o["start"].astype(int) for o in runs[0][:2]])
    max_length = int(np.median(spans[spans >= 20]))
    max_ee = float(np.median([filters_rule.expected_errors(rec.split(b"\n")[3]) for _rt, a, b in runs[0][2] for rec in (a, b)]))
    max_n = 1.0
    want_bins = [[b"", b""] for _ in range(count)]
    want = {"short": 0, "untrimmed": 0, **dict.fromkeys(NAMES, 0)}
    bin_counts = [0] * count
    for i in range(n):
        hits = [b for b in range(count) if runs[b][0][i]["flags"] & abi.CS_F_INLINE]
        assert len(hits) <= 1
        src = hits[0] if hits else count - 1
        o1, o2, recs = runs[src]
        x1, x2 = (bits_of(rec, max_length, max_n, max_ee) for rec in recs[i][1:3])
        rt = filters_rule.route(int(o1[i]["flags"]), int(o2[i]["flags"]), x1, x2, True)
        if rt in NAMES:
            want[rt] += 1
        elif rt == 1:
            want["short"] += 1
        elif rt == 2:
            want["untrimmed"] += 1
        else:
            assert hits
            want_bins[src][0] += recs[i][1]
            want_bins[src][1] += recs[i][2]
            bin_counts[src] += 1
    assert all(want[k] > 0 for k in NAMES) and min(bin_counts) > 0

    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "1000")
    if switch:
        monkeypatch.setenv(*switch.split("="))
    prefix = str(tmp_path / "dm")
    capsys.readouterr()
    cli.main(["-a", scheme_with(codes[0]), "--demux-barcodes", str(table), "-O", prefix, "--json-file",
              str(tmp_path / "r.json"), "-M", str(max_length), "--max-n", str(max_n), "--max-ee", repr(max_ee), in1, in2])
    line = stderr_line(capsys.readouterr().err)
    for b, name in enumerate(bnames):
        assert gunzip(f"{prefix}_{name}_trimmed_R1.fastq.gz") == want_bins[b][0], name
        assert gunzip(f"{prefix}_{name}_trimmed_R2.fastq.gz") == want_bins[b][1], name
    assert gunzip(f"{prefix}_untrimmed_R1.fastq.gz").count(b"\n") // 4 == want["untrimmed"]
    rep = json.loads((tmp_path / "r.json").read_text())
    rc = rep["read_counts"]
    assert rep["engine"]["demultiplexed"] == dict(zip(bnames, bin_counts))
    assert rc["output"] == sum(bin_counts) and rc["filtered"]["too_short"] == want["short"]
    assert rc["filtered"]["too_long"] == want["too_long"] and rc["filtered"]["too_many_n"] == want["too_many_n"]
    assert rc["filtered"]["too_many_expected_errors"] == want["too_many_ee"]
    assert line["too_long"] == str(want["too_long"]) and line["too_many_n"] == str(want["too_many_n"])
    assert rc["input"] == n == rc["output"] + want["short"] + want["untrimmed"] + sum(want[k] for k in NAMES)
