"""textio.TextReader's one cutting loop (``_Pending`` + the three sources) on the shapes at which it can go wrong, in
pinned memory and in an inflater's: the blocks it hands out against a splitter that knows nothing but the file's text."""
import gzip

import pytest

from cutseq_amd import fastq, textio

import bgzf_rule
from test_inflate_cpu import _TAILS, _blocks, unpinned  # noqa: F401  (the fixture: an ordinary arena for the pinned one)


def _split(text: bytes, chunk_reads: int):
    """The rule, from the text alone -> [(block text, records, first record)]: blocks of exactly ``chunk_reads``
    four-line records, the last one shorter; whole blank lines behind the last record dropped; the last record's final
    newline may be missing (and is not part of the block); an empty last read ("@id\\n\\n+\\n\\n") is kept, its empty
    quality line ended if the file does not."""
    lines = text.split(b"\n")
    rest = lines.pop()  # what stands behind the last newline
    blocks, at = [], 0
    while any(l.strip() for l in lines[at:]) or rest.strip():
        if len(lines) - at >= 4 * chunk_reads:
            blocks.append((b"".join(l + b"\n" for l in lines[at:at + 4 * chunk_reads]), chunk_reads, at // 4))
            at += 4 * chunk_reads
            continue
        tail = lines[at:] + [rest]  # every line but the last one had its newline
        last = max(i for i, l in enumerate(tail) if l.strip())
        head = b"".join(l + b"\n" for l in tail[:last])
        if last % 4 == 3:
            blocks.append((head + tail[last].rstrip(), (last + 1) // 4, at // 4))
        elif last % 4 == 2 and last + 1 < len(tail):  # a '+' line with its newline: the blank line behind it is the quality line
            blocks.append((head + tail[last] + b"\n" + tail[last + 1] + b"\n", (last + 2) // 4, at // 4))
        else:
            raise ValueError("truncated")
        break
    return blocks


def _share(text: bytes, chunk_reads: int, first: int, count: int):
    """Records [first, first + count) of the whole file's stream, as a reader that stops by count hands them out."""
    lines = text.split(b"\n")
    recs = [b"".join(l + b"\n" for l in lines[4 * i:4 * i + 4]) for i in range(first, first + count)]
    return [(b"".join(recs[i:i + chunk_reads]), len(recs[i:i + chunk_reads]), i) for i in range(0, count, chunk_reads)]


def _records(lengths):
    return [b"@r%d 1:N:0\n%s\n+\n%s\n" % (i, b"ACGT"[i % 4:i % 4 + 1] * k, b"F" * k) for i, k in enumerate(lengths)]


def _members(parts):
    """-> (a gzip file of one member per part, the members' compressed offsets)"""
    blobs = [gzip.compress(p, 1) for p in parts]
    return b"".join(blobs), [sum(len(b) for b in blobs[:i]) for i in range(len(blobs) + 1)]


def _read(path, data, chunk_reads, **kw):
    path.write_bytes(data)
    return _blocks(textio.TextReader(str(path), chunk_reads, **kw))


def _check(tmp_path, name, data, text, chunk_reads, device=False):
    """Host mode; with ``device`` the inflater's memory too: every block that ends inside the BGZF run comes from it."""
    want = _split(text, chunk_reads)
    assert [b[:3] for b in _read(tmp_path / name, data, chunk_reads)] == want
    if device:
        from cutseq_amd.inflater import HostInflater
        got = _read(tmp_path / name, data, chunk_reads, inflater=HostInflater)
        assert [b[:3] for b in got] == want
        from_inflater = text.count(b"\n") // (4 * chunk_reads)
        assert [b[3] for b in got] == [True] * from_inflater + [False] * (len(want) - from_inflater)


_NINE = _records([17, 0, 60, 33, 5, 60, 1, 48, 22])


@pytest.mark.parametrize("chunk_reads", [1, 2])
@pytest.mark.parametrize("form", ["plain", "gz-members", "bgzf-64", "bgzf-700"])
def test_several_cuts_through_one_piece_and_a_record_across_pieces(tmp_path, unpinned, form, chunk_reads):
    text = b"".join(_NINE)
    assert len(_split(text, chunk_reads)) == -(-9 // chunk_reads)
    if form == "plain":
        _check(tmp_path, "in.fq", text, text, chunk_reads)
    elif form == "gz-members":
        data, _ = _members([b"".join(_NINE[:1]), b"".join(_NINE[1:4]), b"".join(_NINE[4:])])
        _check(tmp_path, "in.fq.gz", data, text, chunk_reads)
    else:
        data = bgzf_rule.bgzf(text, int(form[5:]), 1) + bgzf_rule.EOF_MARKER
        _check(tmp_path, "in.fq.gz", data, text, chunk_reads, device=True)


@pytest.mark.parametrize("form", ["gz-members", "bgzf"])
def test_a_cut_on_a_piece_s_last_byte_with_more_text_behind(tmp_path, unpinned, form):
    """The first piece ends exactly behind record ``chunk_reads``: nothing is carried, and the next block starts with
    the next piece."""
    head, rest = b"".join(_NINE[:2]), b"".join(_NINE[2:])
    if form == "gz-members":
        data, _ = _members([head, rest[:100], rest[100:]])
        _check(tmp_path, "in.fq.gz", data, head + rest, 2)
    else:
        data = bgzf_rule.bgzf(head, len(head), 1) + bgzf_rule.bgzf(rest, 64, 1) + bgzf_rule.EOF_MARKER
        _check(tmp_path, "in.fq.gz", data, head + rest, 2, device=True)


@pytest.mark.parametrize("form", ["plain", "gz-members"])
def test_the_buffer_grows_while_copies_are_in_flight(tmp_path, unpinned, monkeypatch, form):
    """One read of 50 000 bases among short ones, pieces of 4096 bytes: the buffer grows several times under the long
    record, with the lines in front of it still on their way in (gzip: one member per line), and records straddle
    the plain file's pread pieces."""
    monkeypatch.setattr(textio, "_BLOCK", 4096)
    text = b"".join(_records([10 + 3 * i for i in range(20)] + [50_000] + [31, 0, 7, 12, 40]))
    if form == "plain":
        _check(tmp_path, "in.fq", text, text, 1)
    else:
        data, _ = _members(text.splitlines(keepends=True))
        _check(tmp_path, "in.fq.gz", data, text, 1)


def test_a_share_skips_more_lines_than_its_first_block_holds(tmp_path, unpinned):
    recs = _records([20 + i for i in range(14)])
    data, offsets = _members([b"".join(recs[lo:lo + 3]) for lo in range(0, 14, 3)])
    text = b"".join(recs)
    for chunk_reads in (1, 4):
        # from the second member (record 3) on, 16 lines in: record 7, in the middle of the third member
        got = _read(tmp_path / "in.fq.gz", data, chunk_reads, start=offsets[1], skip_lines=16)
        assert [b[:3] for b in got] == _split(b"".join(recs[7:]), chunk_reads)
        got = _read(tmp_path / "in.fq.gz", data, chunk_reads, start=offsets[1], skip_lines=16, max_records=5)
        assert [b[:3] for b in got] == _share(text, chunk_reads, 7, 5)


@pytest.mark.parametrize("form", ["plain", "gz-members"])
@pytest.mark.parametrize("max_records", [0, 1, 4])
def test_a_share_ends_behind_max_records(tmp_path, unpinned, form, max_records):
    chunk_reads = 3  # (0, 1 and chunk_reads + 1 records)
    text = b"".join(_NINE)
    data = text if form == "plain" else _members([b"".join(_NINE[:1]), b"".join(_NINE[1:4]), b"".join(_NINE[4:])])[0]
    got = _read(tmp_path / ("in.fq" if form == "plain" else "in.fq.gz"), data, chunk_reads, max_records=max_records)
    assert [b[:3] for b in got] == _share(text, chunk_reads, 0, max_records)
    assert [b[1] for b in got] == [[], [1], [3, 1]][min(max_records, 2)]


def test_a_share_stops_at_a_member_boundary(tmp_path, unpinned):
    recs = _records([20 + i for i in range(14)])
    data, offsets = _members([b"".join(recs[lo:lo + 3]) for lo in range(0, 14, 3)])
    for chunk_reads in (2, 3):
        got = _read(tmp_path / "in.fq.gz", data, chunk_reads, stop=offsets[3])
        assert [b[:3] for b in got] == _split(b"".join(recs[:9]), chunk_reads)
        got = _read(tmp_path / "in.fq.gz", data, chunk_reads, start=offsets[1], stop=offsets[3])
        assert [b[:3] for b in got] == _split(b"".join(recs[3:9]), chunk_reads)


# ---------------------------------------------------------------- the end of the input, as a function of the bytes left


@pytest.mark.parametrize("tail", sorted(_TAILS))
def test_end_of_input_on_the_tails(tail):
    extra = _TAILS[tail][0]
    body = b"".join(_NINE[:3])
    text = body[:-1] if extra is None else body + extra
    (want, records, _), = _split(text, 100)
    end, n, newline = textio._end_of_input(text, "in.fq")
    assert newline == (tail == "empty-last-read-no-newline")
    assert (n, (text + b"\n" if newline else text)[:end]) == (records, want)
    assert records == 3 + text.count(b"@e")


@pytest.mark.parametrize("text", [b"", b"\n", b" \r\n\t\n\n"])
def test_end_of_input_with_nothing_left(text):
    assert textio._end_of_input(text, "in.fq") == (0, 0, False) and _split(text, 100) == []


@pytest.mark.parametrize("tail", [b"@x\nACGT\n+", b"@x\nAC", b"@x\nACGT\n", b"@x\n\n+  "])
def test_end_of_input_in_the_middle_of_a_record(tail):
    """A '+' line as the very last byte, a file that ends inside a sequence line (or behind it), a '+' line that white
    space follows but no newline: truncated."""
    text = b"".join(_NINE[:3]) + tail
    with pytest.raises(fastq.FastqFormatError, match="in.fq: truncated FASTQ record at end of file"):
        textio._end_of_input(text, "in.fq")
    with pytest.raises(ValueError, match="truncated"):
        _split(text, 100)
