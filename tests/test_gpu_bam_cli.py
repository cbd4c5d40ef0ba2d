"""Unaligned BAM inputs on the command line: every output file (decompressed), the info table and the JSON report (input
paths aside) of a run on BAM files equal those of the same command on the FASTQ files tests/bam_rule.py renders from
those BAMs.  The 10 000-pair fixture as R1.bam + R2.bam and as one interleaved pairs.bam, in BGZF blocks of 4096 bytes
(records straddle blocks) and reader blocks of 1000 records (records straddle those too).

The two legs of a comparison write to the same file names, one after the other, so the reports name the same outputs;
the wall time, the command line and the input paths are taken out before reports are compared."""
import gzip
import io
import json
import os
import sys
from collections import Counter

import pytest

from cutseq_amd import fastq, run as cli

import bam_rule
import util
from test_gpu_demux import scheme_with

pytestmark = pytest.mark.gpu
PLAN = ["-A", "TAKARAV3", "--trim-polyA"]
N = 10_000


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{"bam": [R1.bam, R2.bam], "fq": [R1.fq, R2.fq], "woven_bam": pairs.bam, "woven_fq": pairs.fq}; the FASTQ files
    are ``read_bam`` of the BAM files."""
    d = tmp_path_factory.mktemp("bam_in")
    mates = []
    for m in (1, 2):
        recs = util.read_fastq_gz(util.GOLDEN / f"fixture10k_R{m}.fq.gz")
        assert len(recs) == N
        mates.append([bam_rule.Rec(name, seq, bytes(q - 33 for q in qual), tags=bam_rule.TAGS[i % 3]) for i, (name, seq, qual) in enumerate(recs)])
    out = {"bam": [], "fq": []}
    for m, records in enumerate(mates, 1):
        data = bam_rule.write_bam(records, bam_rule.HEADER_TEXT, block_bytes=4096)
        (d / f"R{m}.bam").write_bytes(data)
        (d / f"R{m}.fq").write_bytes(bam_rule.read_bam(data))
        out["bam"].append(str(d / f"R{m}.bam"))
        out["fq"].append(str(d / f"R{m}.fq"))
    woven = bam_rule.write_bam([r for pair in zip(*mates) for r in pair], block_bytes=4096, eof=False)
    (d / "pairs.bam").write_bytes(woven)
    (d / "pairs.fq").write_bytes(bam_rule.read_bam(woven))
    out["woven_bam"], out["woven_fq"] = str(d / "pairs.bam"), str(d / "pairs.fq")
    return out


@pytest.fixture(autouse=True)
def one_device(monkeypatch):
    monkeypatch.setenv("CUTSEQ_DEVICES", "0")
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "1000")
    for name in ("CUTSEQ_GPU_INFLATE", "CUTSEQ_GPU_DEFLATE", "CUTSEQ_TEXT_PATH"):
        monkeypatch.delenv(name, raising=False)


def leg(tmp_path, ins, options, stdin=None, monkeypatch=None):
    """One run into tmp_path/out -> ({file name: decompressed bytes}, the report without times and paths)."""
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    for name in os.listdir(out):
        os.remove(out / name)
    argv = list(ins) + PLAN + ["--json-file", str(out / "report.json")] + [o.replace("OUT/", str(out) + "/") for o in options]
    if stdin is not None:
        with open(stdin, "rb") as fh:
            monkeypatch.setattr(sys, "stdin", type("In", (), {"buffer": io.BytesIO(fh.read())})())
    cli.main(argv)
    rep = json.loads((out / "report.json").read_text())
    rep["engine"]["seconds"] = rep["command_line_arguments"] = None
    rep["input"]["path1"] = rep["input"]["path2"] = None
    files = {}
    for name in sorted(os.listdir(out)):
        if name != "report.json":
            data = (out / name).read_bytes()
            files[name] = gzip.decompress(data) if name.endswith(".gz") else data
    return files, rep


def same(tmp_path, fq_ins, bam_ins, options, stdin=None, monkeypatch=None):
    want_files, want_rep = leg(tmp_path, fq_ins, options)
    got_files, got_rep = leg(tmp_path, bam_ins, options, stdin, monkeypatch)
    assert want_rep["read_counts"]["input"] == N and want_rep["read_counts"]["output"] > 0
    assert got_rep == want_rep
    assert sorted(got_files) == sorted(want_files) and len(want_files) >= 1
    for name in want_files:
        assert got_files[name] == want_files[name], name
    return want_files


PAIRED_OUT = ["-o", "OUT/o1.fastq.gz", "OUT/o2.fastq.gz", "-s", "OUT/s1.fastq.gz", "OUT/s2.fastq.gz"]
FORMS = {
    "gz": PAIRED_OUT,
    "plain": ["-o", "OUT/o1.fastq", "OUT/o2.fastq", "-s", "OUT/s1.fastq", "OUT/s2.fastq"],
    "bgzf": PAIRED_OUT + ["--bgzf"],
    "info": PAIRED_OUT + ["--info-file", "OUT/info.tsv"],
    "rename": PAIRED_OUT + ["--rename", "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}"],
    "too-long": PAIRED_OUT + ["-M", "50", "--too-long-output", "OUT/l1.fastq.gz", "OUT/l2.fastq.gz"],
    "interleaved-out": ["--interleaved", "-o", "OUT/o.fastq.gz", "-s", "OUT/s.fastq.gz"],
}


@pytest.mark.parametrize("form", list(FORMS))
def test_two_bam_files(tmp_path, inputs, form):
    files = same(tmp_path, inputs["fq"], inputs["bam"], FORMS[form])
    if form == "info":
        assert files["info.tsv"].count(b"\n") >= N
    if form == "too-long":
        assert files["l1.fastq.gz"].count(b"\n") > 400


@pytest.mark.parametrize("form", ["interleaved-out", "gz-info"])
def test_one_interleaved_bam(tmp_path, inputs, form):
    options = FORMS["interleaved-out"] + (["--info-file", "OUT/info.tsv.gz"] if form == "gz-info" else [])
    same(tmp_path, [inputs["woven_fq"]], [inputs["woven_bam"]], options)


def test_a_bam_on_standard_input(tmp_path, inputs, monkeypatch):
    same(tmp_path, [inputs["woven_fq"]], ["-"], FORMS["interleaved-out"], stdin=inputs["woven_bam"], monkeypatch=monkeypatch)


def test_single_end(tmp_path, inputs):
    same(tmp_path, inputs["fq"][:1], inputs["bam"][:1], ["-o", "OUT/o.fastq.gz", "-s", "OUT/s.fastq"])


def test_demultiplexing(tmp_path, inputs, monkeypatch):
    """The BAM pair through --demux-barcodes: every barcode's files as from the FASTQ pair.  The three most frequent
    six-base starts of mate 1 serve as the inline barcodes."""
    starts = Counter(r[1][:6] for r in util.read_fastq_gz(util.GOLDEN / "fixture10k_R1.fq.gz") if b"N" not in r[1][:6])
    codes = [c.decode() for c, _ in starts.most_common(3)]
    table = tmp_path / "barcodes.tsv"
    table.write_text("".join(f"bc{i}\t{c}\n" for i, c in enumerate(codes)))
    monkeypatch.setattr(sys.modules[__name__], "PLAN", ["-a", scheme_with(codes[0]), "--demux-barcodes", str(table)])
    want_files, want_rep = leg(tmp_path, inputs["fq"], ["-O", "OUT/dm"])
    got_files, got_rep = leg(tmp_path, inputs["bam"], ["-O", "OUT/dm"])
    assert got_rep == want_rep and sorted(got_files) == sorted(want_files) and len(want_files) >= 8
    assert all(got_files[name] == want_files[name] for name in want_files)
    assert any(want_files[f"dm_bc{i}_trimmed_R1.fastq.gz"] for i in range(3))


def _woven(n, rename_at=None):
    pairs = []
    for m in (1, 2):
        recs = util.read_fastq_gz(util.GOLDEN / f"fixture10k_R{m}.fq.gz")[:n]
        pairs.append([bam_rule.Rec(name if (i, m) != (rename_at, 2) else b"someone_else", seq, bytes(q - 33 for q in qual))
                      for i, (name, seq, qual) in enumerate(recs)])
    return [r for pair in zip(*pairs) for r in pair]


def test_a_file_of_one_bad_record(tmp_path, monkeypatch):
    """The only record's parts leave its block: its own message, under any block size."""
    monkeypatch.chdir(tmp_path)
    rec = _woven(1)[0]
    stream = bam_rule.header_bytes() + bam_rule.record_bytes(rec, l_seq=len(rec.seq) + 40)
    (tmp_path / "one.bam").write_bytes(bam_rule.wrap(stream))
    with pytest.raises(fastq.FastqFormatError, match="name, cigar, bases and qualities of record 0 exceed its block_size"):
        cli.main(["one.bam"] + PLAN + ["-o", "o.fq", "-s", "s.fq"])
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "1")
    good = _woven(3)[::2]
    stream = bam_rule.header_bytes() + b"".join(bam_rule.record_bytes(r) for r in good) + bam_rule.record_bytes(rec, l_seq=len(rec.seq) + 40)
    (tmp_path / "four.bam").write_bytes(bam_rule.wrap(stream))
    with pytest.raises(fastq.FastqFormatError, match="name, cigar, bases and qualities of record 3 exceed its block_size"):
        cli.main(["four.bam"] + PLAN + ["-o", "o.fq", "-s", "s.fq"])


def test_mate_names_that_differ_count_pairs_as_for_fastq(tmp_path, monkeypatch):
    """Pair 2345 of an interleaved BAM (the third reader block) has a mate of another name: the message of the FASTQ
    run on the same records, with its record number."""
    monkeypatch.chdir(tmp_path)
    data = bam_rule.write_bam(_woven(3000, rename_at=2345), block_bytes=4096)
    (tmp_path / "pairs.bam").write_bytes(data)
    (tmp_path / "pairs.fq").write_bytes(bam_rule.read_bam(data))
    messages = []
    for name in ("pairs.fq", "pairs.bam"):
        with pytest.raises(ValueError) as exc:
            cli.main(["--interleaved", name] + PLAN + ["-o", "o.fq", "-s", "s.fq"])
        messages.append(str(exc.value))
    assert messages[0] == messages[1] and "Input read IDs not identical in record 2346" in messages[0]
    # ... while a refused record of the same block is named by its own number in the file
    records = _woven(3000)
    records[2 * 2345 + 1] = records[2 * 2345 + 1]._replace(flag=0x10)
    (tmp_path / "aligned.bam").write_bytes(bam_rule.write_bam(records, block_bytes=4096))
    with pytest.raises(fastq.FastqFormatError, match="only unaligned BAM is supported: record 4691 is aligned"):
        cli.main(["--interleaved", "aligned.bam"] + PLAN + ["-o", "o.fq", "-s", "s.fq"])


def test_a_refused_record_names_its_place_in_the_file(tmp_path, inputs):
    """An aligned record in the third reader block of mate 2's file: the run ends with the record's number in the file."""
    recs = util.read_fastq_gz(util.GOLDEN / "fixture10k_R2.fq.gz")[:3000]
    records = [bam_rule.Rec(name, seq, bytes(q - 33 for q in qual), flag=0x10 if i == 2345 else 0x4) for i, (name, seq, qual) in enumerate(recs)]
    (tmp_path / "bad_R2.bam").write_bytes(bam_rule.write_bam(records, block_bytes=4096))
    first = util.read_fastq_gz(util.GOLDEN / "fixture10k_R1.fq.gz")[:3000]
    (tmp_path / "R1.bam").write_bytes(bam_rule.write_bam([bam_rule.Rec(n, s, bytes(q - 33 for q in qual)) for n, s, qual in first], block_bytes=4096))
    with pytest.raises(fastq.FastqFormatError, match="mate 2: only unaligned BAM is supported: record 2345 is aligned"):
        cli.main([str(tmp_path / "R1.bam"), str(tmp_path / "bad_R2.bam")] + PLAN + ["-o", str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq"),
                                                                                   "-s", str(tmp_path / "s1.fq"), str(tmp_path / "s2.fq")])
