"""Unaligned BAM input, the parts that need no GPU: the rule's own round trip, the host walker against it (whole and in
pieces), the reader's BAM mode, the refusals the host raises, and the shared record decisions of include/cutseq_bam.h as a
host program under the sanitizers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cutseq_amd import fastq, run, textio

import bam_rule
from test_inflate_cpu import unpinned  # noqa: F401  (the fixture: an ordinary arena for the pinned one)

ROOT = Path(__file__).resolve().parents[1]
UNIVERSE = bam_rule.universe()


def test_universe_covers_what_it_says():
    labels = [label for label, _, _ in UNIVERSE]
    assert labels == [f"edges/{b}" for b in (37, 64, 4096, 65280)] + [f"count/{n}" for n in (1, 255, 256, 257, 600)]
    edges = bam_rule.edge_records()
    assert {len(r.seq) for r in edges} >= set(bam_rule.L_SEQS)
    assert {len(r.name) for r in edges} >= {0, 1, 2, 31, 32, 33, 254}
    assert {0, 93} <= {q for r in edges for q in r.qual}
    for parity in (0, 1):  # every code at both nibble positions
        assert {c for r in edges for c in r.seq[parity::2]} >= set(bam_rule.LETTERS)
    assert any(r.cigar for r in edges) and {r.tags for r in edges} == set(bam_rule.TAGS)


@pytest.mark.parametrize("label,records,kw", UNIVERSE, ids=[u[0] for u in UNIVERSE])
def test_rule_round_trip(label, records, kw):
    data = bam_rule.write_bam(records, **kw)
    want = b"".join(b"@" + r.name + b"\n" + r.seq + b"\n+\n" + bytes(q + 33 for q in r.qual) + b"\n" for r in records)
    assert bam_rule.read_bam(data) == want
    assert data.endswith(bam_rule.bgzf_rule.EOF_MARKER) == kw.get("eof", True)
    body, offsets, texts = bam_rule.split(data)
    assert len(offsets) == len(records) + 1 and offsets[-1] == len(body) and b"".join(texts) == want


def test_corrupt_cases_raise_their_message():
    cases = bam_rule.corrupt()
    assert {c.code for c in cases} == set(bam_rule.MESSAGES)  # one input per refusal at least
    for c in cases:
        with pytest.raises(bam_rule.BamError) as exc:
            bam_rule.read_bam(bam_rule.wrap(c.stream, 64))
        assert str(exc.value) == bam_rule.MESSAGES[c.code].format(n=c.record), c.label


# ---------------------------------------------------------------- the host walker through ctypes

def _walk(stream: bytes, start: int, max_records: int):
    L = textio._host()
    buf = np.frombuffer(stream + b"\xa5" * 8, dtype=np.uint8)  # (the walk gets the stream's size, not the array's)
    offs = np.full(max_records + 1, 0xFFFFFFFF, dtype=np.uint32)
    nxt, text, bad = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    found = L.csh_bam_walk(buf.ctypes.data, len(stream), start, max_records, offs.ctypes.data, C.byref(nxt), C.byref(text), C.byref(bad))
    assert np.all(offs[found:] == 0xFFFFFFFF)
    return int(found), [int(x) for x in offs[:found]], int(nxt.value), int(text.value), int(bad.value)


def _header(stream: bytes) -> int:
    buf = np.frombuffer(stream + b"\xa5" * 8, dtype=np.uint8)
    return int(textio._host().csh_bam_header(buf.ctypes.data, len(stream)))


@pytest.mark.parametrize("label,records,kw", UNIVERSE, ids=[u[0] for u in UNIVERSE])
def test_walker_agrees_with_the_rule(label, records, kw):
    stream = bam_rule.inflated(records, kw.get("header_text", b""), kw.get("refs", ()))
    rows = list(bam_rule.read_records(stream))
    head = _header(stream)
    assert head == bam_rule.header_size(stream) == (rows[0][0] if rows else len(stream))
    found, offs, nxt, text, bad = _walk(stream, head, len(records) + 5)
    assert (found, offs, nxt, bad) == (len(rows), [r[0] for r in rows], len(stream), 0)
    assert text == sum(len(r[2]) for r in rows)
    # max_records stops the walk in front of that record
    for cap in (0, 1, len(rows) - 1):
        if 0 <= cap < len(rows):
            found, offs, nxt, text, bad = _walk(stream, head, cap)
            assert (found, nxt, bad, text) == (cap, rows[cap][0], 0, sum(len(r[2]) for r in rows[:cap]))


def test_walker_on_every_prefix_of_a_small_case():
    """The carry logic: whatever byte a buffer ends at, the header is "not yet" or its size, the walk finds exactly the
    records that lie completely inside, and says where the first incomplete one starts."""
    records = bam_rule.edge_records()[:9]
    stream = bam_rule.inflated(records, bam_rule.HEADER_TEXT, bam_rule.REFS)
    rows = list(bam_rule.read_records(stream))
    head = bam_rule.header_size(stream)
    for k in range(len(stream) + 1):
        assert _header(stream[:k]) == (head if k >= head else 0), k
        if k >= head:
            whole = [r for r in rows if r[1] <= k]
            found, offs, nxt, text, bad = _walk(stream[:k], head, 100)
            assert (found, offs, bad) == (len(whole), [r[0] for r in whole], 0), k
            assert nxt == (whole[-1][1] if whole else head) and text == sum(len(r[2]) for r in whole), k
    # ... and a walk that goes on from where the last one stopped finds the rest
    mid = rows[4][1] + 3
    found, offs, nxt, _, _ = _walk(stream[:mid], head, 100)
    more, offs2, nxt2, _, _ = _walk(stream, nxt, 100)
    assert offs + offs2 == [r[0] for r in rows] and nxt2 == len(stream)


def test_walker_and_header_refusals():
    for c in bam_rule.corrupt():
        if c.where != "stream":
            continue
        head = _header(c.stream)
        if c.code == bam_rule.BAD_MAGIC:
            assert head == -1, c.label
        elif c.code == bam_rule.BAD_HEADER_LENGTH:
            assert head == -2, c.label
        elif c.code == bam_rule.ENDS_IN_HEADER:
            assert head == 0, c.label
        else:
            found, _, nxt, _, bad = _walk(c.stream, head, 100)
            assert found == c.record and bad == (1 if c.code == bam_rule.BLOCK_SIZE else 0) and nxt < len(c.stream), c.label
    assert _header(b"BA") == 0 and _header(b"BX") == -1 and _header(b"") == 0


# ---------------------------------------------------------------- the reader's BAM mode

def _bam_blocks(reader):
    out = []
    while True:
        b = reader.get()
        if b is None:
            break
        offs = b.offsets.view(np.uint32)[: (2 if reader.interleaved else 1) * b.n + 1].tolist()
        out.append((bytes(memoryview(b.buf)[: b.nbytes]), offs, b.n, b.first_record, b.text_bytes))
        b.release()
    reader.close()
    return out


@pytest.mark.parametrize("chunk_reads", [1, 2, 3, 256, 1000])
def test_reader_cuts_blocks_of_whole_records(tmp_path, unpinned, chunk_reads):  # noqa: F811
    records = bam_rule.edge_records() + bam_rule.random_records(600, seed=3)
    data = bam_rule.write_bam(records, bam_rule.HEADER_TEXT, bam_rule.REFS, block_bytes=64 if chunk_reads < 256 else 4096)
    body, offsets, texts = bam_rule.split(data)
    path = tmp_path / "in.bam"
    path.write_bytes(data)
    reader = textio.TextReader(str(path), chunk_reads)
    assert reader.bam and not reader.fasta and reader.gz
    blocks = _bam_blocks(reader)
    assert [b[2] for b in blocks] == [chunk_reads] * (len(records) // chunk_reads) + ([len(records) % chunk_reads] if len(records) % chunk_reads else [])
    assert [b[3] for b in blocks] == list(range(0, len(records), chunk_reads))
    assert b"".join(b[0] for b in blocks) == body
    at = 0
    for raw, offs, n, first, text_bytes in blocks:
        assert offs == [o - offsets[first] for o in offsets[first:first + n + 1]] and offs[-1] == len(raw)
        assert text_bytes == sum(len(t) for t in texts[first:first + n])
        at += n
    assert at == len(records)


def test_reader_interleaved_blocks_count_pairs(tmp_path, unpinned):  # noqa: F811
    r1 = bam_rule.random_records(301, seed=8)
    woven = [r for pair in zip(r1, bam_rule.mate_of(r1)) for r in pair]
    path = tmp_path / "pairs.bam"
    path.write_bytes(bam_rule.write_bam(woven, block_bytes=4096))
    blocks = _bam_blocks(textio.TextReader(str(path), 2 * 100, interleaved=True))
    assert [(b[2], b[3], len(b[1])) for b in blocks] == [(100, 0, 201), (100, 100, 201), (100, 200, 201), (1, 300, 3)]
    path.write_bytes(bam_rule.write_bam(woven[:-1], block_bytes=4096))
    with pytest.raises(fastq.FastqFormatError, match="ends after an odd number of records"):
        _bam_blocks(textio.TextReader(str(path), 2 * 100, interleaved=True))


def test_reader_on_standard_input(tmp_path, unpinned, monkeypatch):  # noqa: F811
    import io
    import sys
    records = bam_rule.random_records(257, seed=9)
    data = bam_rule.write_bam(records, block_bytes=4096)
    monkeypatch.setattr(sys, "stdin", type("In", (), {"buffer": io.BytesIO(data)})())
    reader = textio.TextReader("-", 100)
    assert reader.bam and reader.sequential
    blocks = _bam_blocks(reader)
    assert [b[2] for b in blocks] == [100, 100, 57] and b"".join(b[0] for b in blocks) == bam_rule.split(data)[0]


def test_reader_raises_what_the_walker_finds(tmp_path, unpinned):  # noqa: F811
    for c in bam_rule.corrupt():
        if c.where != "stream" or c.code == bam_rule.BAD_MAGIC:  # (a wrong magic is no BAM: the FASTQ reader's business)
            continue
        path = tmp_path / "bad.bam"
        path.write_bytes(bam_rule.wrap(c.stream, 64, eof=False))
        with pytest.raises(fastq.FastqFormatError) as exc:
            _bam_blocks(textio.TextReader(str(path), 2))
        assert bam_rule.MESSAGES[c.code].format(n=c.record) in str(exc.value), c.label
    # the header routine's own refusal of the magic
    pend = textio._PendingRecords(textio._HOST, 4, "x.bam")
    try:
        pend.buf[:4] = np.frombuffer(b"BAM\x02", dtype=np.uint8)
        pend.added(4, 0)
        pend.goal = 1
        with pytest.raises(fastq.FastqFormatError) as exc:
            pend.refresh()
        assert bam_rule.MESSAGES[bam_rule.BAD_MAGIC] in str(exc.value)
    finally:
        pend.close()


def test_a_share_of_a_bam_is_refused(tmp_path, unpinned):  # noqa: F811
    path = tmp_path / "in.bam"
    path.write_bytes(bam_rule.write_bam(bam_rule.random_records(10, seed=1)))
    with pytest.raises(ValueError, match="only plain and gzip FASTQ files can be split between ranks"):
        textio.TextReader(str(path), 4, max_records=5)


# ---------------------------------------------------------------- the CLI's refusals that need no device

def _cli(tmp_path, monkeypatch, caplog, argv):
    from cutseq_amd import capi
    monkeypatch.setattr(capi, "device_count", lambda: pytest.fail("a device was asked for"))
    monkeypatch.chdir(tmp_path)
    caplog.clear()
    with pytest.raises(SystemExit) as exc:
        run.main(argv)
    assert exc.value.code == 1
    return caplog.text


def test_cli_refusals(tmp_path, monkeypatch, caplog):
    r1 = bam_rule.random_records(20, seed=2)
    (tmp_path / "R1.bam").write_bytes(bam_rule.write_bam(r1))
    (tmp_path / "R2.bam").write_bytes(bam_rule.write_bam(bam_rule.mate_of(r1)))
    (tmp_path / "R2.fq").write_bytes(bam_rule.read_bam(bam_rule.write_bam(bam_rule.mate_of(r1))))
    common = ["-A", "TAKARAV3", "-o", "o1.fq", "o2.fq", "-s", "s1.fq", "s2.fq"]
    text = _cli(tmp_path, monkeypatch, caplog, ["R1.bam", "R2.bam", "--ranks", "2", *common])
    assert "R1.bam: only plain and gzip FASTQ files can be split between ranks" in text
    text = _cli(tmp_path, monkeypatch, caplog, ["R1.bam", "R2.fq", *common])
    assert "the two input files are in different formats (one BAM, one FASTQ or FASTA)" in text
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    text = _cli(tmp_path, monkeypatch, caplog, ["R1.bam", "R2.bam", *common])
    assert "R1.bam: BAM input needs the text path (CUTSEQ_TEXT_PATH unset)" in text


# ---------------------------------------------------------------- the shared decisions, as their own program

@pytest.fixture(scope="module")
def walk_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bam") / "bam_walk_check"
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tools" / "bam_walk_check.c"), "-lpthread"], check=True)
    return exe


@pytest.mark.parametrize("which", ["universe", "corrupt", "mutations"])
def test_shared_decisions_under_the_sanitizers(walk_check, tmp_path, which):
    """Exit status 0, no sanitizer report, no case that differs: the walker and the host form of the record checks and of
    the expansion give the rule's text or the rule's verdict (code and record) on every stream."""
    streams = {"universe": lambda: [bam_rule.inflated(r, kw.get("header_text", b""), kw.get("refs", ())) for _, r, kw in UNIVERSE],
               "corrupt": lambda: [c.stream for c in bam_rule.corrupt()], "mutations": bam_rule.mutations}[which]()
    assert len(streams) == {"universe": 9, "corrupt": 17, "mutations": 2000}[which]
    verdicts = [bam_rule.verdict(s)[0] for s in streams]
    if which == "universe":
        assert set(verdicts) == {bam_rule.OK}
    elif which == "corrupt":
        assert bam_rule.OK not in verdicts
    else:  # (the mutations reach every refusal, and a third of them change nothing the rule reads)
        assert set(verdicts) == {bam_rule.OK} | set(bam_rule.MESSAGES) and 400 < verdicts.count(bam_rule.OK) < 1000
    path = tmp_path / "cases.bin"
    bam_rule.write_case_file(path, streams)
    done = subprocess.run([str(walk_check), str(path)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.stdout[-3000:], done.stderr[-3000:])
    assert done.stdout.splitlines()[-1] == f"{len(streams)} cases, 0 differ"
