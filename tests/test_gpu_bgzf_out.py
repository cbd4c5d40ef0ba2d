"""The device BGZF writer (``cs_text_params.compress = 2``: deflate_chunks<true> and bgzf_layout in
cutseq_amd/csrc/deflate_kernels.hip.inc) held to tests/bgzf_out_rule.py: every stream is walked by BSIZE, every block
goes through the strict parser, its layout, its own CRC-32 and length, and the tokens of every dynamic block are those
of a stream that consists of that chunk alone; the Huffman codes are held to ``check_codes``.

The cases go through ``textpath.TextEngine(..., compress=2)`` the way tests/test_gpu_gzip_structure.py drives
``compress=True``: pass-through plans, the expected text is the same engine's with ``compress=False``."""
import random

import numpy as np
import pytest

from cutseq_amd import abi, textpath
from cutseq_amd.engine import TrimEngine

import bgzf_out_rule
import gzip_rule
from test_gpu_gzip_structure import (check_codes, fasta, fastq, make_plan, noisy, ordinary, records_for, run,
                                     three_routes)

pytestmark = pytest.mark.gpu

CHUNK = gzip_rule.CHUNK
BGZF = 2


def check(packed: bytes, plain: bytes, is_fasta=False, lz=True, what=""):
    """One stream as the device delivers it -> [(Member, dynamic)] per block."""
    if not plain:
        assert packed == b"", what  # a route with no bytes writes nothing
        return []
    blocks = bgzf_out_rule.check_stream(packed, plain, is_fasta, lz, what)
    for i, (member, dynamic) in enumerate(blocks):
        if dynamic:
            check_codes(member.blocks[0], (what, i))
    return blocks


def single_end(recs, lz=True, text_of=fastq, is_fasta=False, what="", **kw):
    tp = make_plan()
    text = fastq(recs)
    (plain, counts), = run(tp, text, None, len(recs), False, **kw)
    want = text_of(recs)
    assert counts == [len(recs), 0, 0] and plain[0][0] == want, what
    (packed, counts2), = run(tp, text, None, len(recs), BGZF, **kw)
    assert counts2 == counts and packed[1][0] == packed[2][0] == b""
    return want, check(packed[0][0], want, is_fasta, lz, what)


# ---- lengths ---------------------------------------------------------------------------------------------------

# The text path's shortest streams are 3 bytes (an empty FASTA record) and 6 (an empty FASTQ record): they stand for "1
# byte".  A BLOCK of one byte is there: the last chunk of CHUNK + 1 and of 2 CHUNK + 1.  0 bytes: the routes beside the
# trimmed one in every case here, and the empty batch below.
SIZES = [3, 6, 127, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 5 * CHUNK + 77]


@pytest.mark.parametrize("size", SIZES)
def test_stream_lengths(size):
    rng = random.Random(size)
    if size == 3:
        plain, blocks = single_end([(b"", b"", b"")], True, fasta, True, size, fasta=True)
    else:
        plain, blocks = single_end(records_for(size, rng), what=size)
    assert len(plain) == size and len(blocks) == (size + CHUNK - 1) // CHUNK
    assert [m.isize for m, _ in blocks] == [CHUNK] * (size // CHUNK) + [size % CHUNK] * (size % CHUNK > 0)
    if size >= CHUNK - 1:
        assert blocks[0][1] and sum(1 for t in blocks[0][0].blocks[0].tokens if t[0] == "match") > 300


def test_no_records_write_nothing():
    (packed, counts), = run(make_plan(), b"", None, 0, BGZF)
    assert counts == [0, 0, 0] and all(s == b"" for route in packed for s in route)


@pytest.mark.parametrize("size", [129, 2 * CHUNK + 1])
def test_literal_only(size, monkeypatch):
    """CUTSEQ_GPU_LZ=0: the same layout from literals alone."""
    monkeypatch.setenv("CUTSEQ_GPU_LZ", "0")
    _plain, blocks = single_end(records_for(size, random.Random(size)), lz=False, what=size)
    assert all(t[0] == "lit" for m, _ in blocks for t in m.tokens)


# ---- nothing in front of a chunk counts ------------------------------------------------------------------------

def straddling(qual: bytes, rng):
    """A stream in which the 40 quality bytes ``qual`` of one record lie 20 in front of offset CHUNK and 20 behind it
    (10 name bytes: 55 bytes of the record in front of its qualities)."""
    recs = records_for(CHUNK - 75, rng) + [(b"straddle0:", b"AC" * 20, qual)] + records_for(5000 - 21, rng, first=1000)
    text = fastq(recs)
    assert len(text) == CHUNK + 5000 and text[CHUNK - 20:CHUNK + 20] == qual and text[CHUNK + 20] == 10
    return recs, text


def test_a_run_across_the_chunk_boundary_starts_with_a_literal():
    """Forty equal quality bytes around offset CHUNK.  The gzip form starts chunk 1 with a match of distance 1 that
    reaches into chunk 0; a BGZF block must not reach in front of itself: a literal, then the rest of the run."""
    recs, text = straddling(b"I" * 40, random.Random(21))
    assert gzip_rule.tokens(text, 1, False)[:2] == [("match", 20, 1), ("lit", 10)]
    assert gzip_rule.tokens(text[CHUNK:], 0, False)[:3] == [("lit", ord("I")), ("match", 19, 1), ("lit", 10)]
    _plain, blocks = single_end(recs)
    assert [d for _, d in blocks] == [True, True]
    assert blocks[1][0].blocks[0].tokens[:3] == [("lit", ord("I")), ("match", 19, 1), ("lit", 10)]
    # the gzip form of the same stream keeps its match (nothing changed there)
    (packed, _), = run(make_plan(), text, None, len(recs), True)
    member = gzip_rule.parse_member(packed[0][0])
    second = [b for b in member.blocks if b.btype == 2][1]
    assert second.tokens[0] == ("match", 20, 1)


def test_chunk_starts_with_the_marker_inside_a_quality_line():
    """'@' as the quality byte at offset CHUNK: the block's first byte is the marker with nothing in front of it -- a
    record start by the rule at stream offset 0, one without a predecessor -- and the bytes behind it are a run."""
    qual = b"I" * 20 + b"@" * 8 + b"I" * 12
    recs, text = straddling(qual, random.Random(22))
    assert text[CHUNK] == ord("@") and text[CHUNK - 1] == ord("I")
    want = gzip_rule.tokens(text[CHUNK:], 0, False)
    assert want[:2] == [("lit", ord("@")), ("match", 7, 1)]
    _plain, blocks = single_end(recs)
    assert blocks[1][1] and blocks[1][0].blocks[0].tokens[:2] == want[:2]


def test_chunk_starts_exactly_at_a_record():
    """Chunk 1 starts with a record's '@': that name is a literal run of its own (no predecessor in the block), and the
    next record finds it at block position 0."""
    rng = random.Random(23)
    recs = records_for(CHUNK, rng) + [ordinary(rng, 2000 + i, 40) for i in range(40)]
    text = fastq(recs)
    assert text[CHUNK - 1] == 10 and text[CHUNK] == ord("@")
    want = gzip_rule.tokens(text[CHUNK:], 0, False)
    assert want[0] == ("lit", ord("@"))
    second = text.index(b"\n@", CHUNK) + 1 - CHUNK  # block position of the next record
    assert ("match", len(b"@SIM:7:FC:1103:1600"), second) in want[:second]  # (coordinates 16000 and 16003)
    _plain, blocks = single_end(recs)
    assert blocks[1][1] and blocks[1][0].blocks[0].tokens == want


# ---- stored chunks ---------------------------------------------------------------------------------------------

def test_noisy_stream_gives_the_largest_block():
    recs = records_for(2 * CHUNK + 500, random.Random(24), 0, noisy)
    _plain, blocks = single_end(recs)
    # (the last 500 bytes hold records_for's closing records, whose padded names shrink: held to the rule like any other)
    assert [d for _, d in blocks][:2] == [False, False] and len(blocks) == 3
    assert [len(m.data) for m, _ in blocks][:2] == [bgzf_out_rule.MAX_BLOCK, bgzf_out_rule.MAX_BLOCK]


# ---- routes, mates, formats ------------------------------------------------------------------------------------

@pytest.mark.parametrize("totals", [[0, 301, 33002], [33001, 2 * CHUNK + 3, 0], [33003, 301, 33002]],
                         ids=["no trimmed", "no untrimmed", "all three"])
def test_paired_three_routes(totals):
    """The routes lie back to back in the mate's buffer, blocks and all: each route's bytes are its own blocks, an empty
    route has none, and two batches on the same slot give the same bytes."""
    rng = random.Random(sum(totals))
    tp, text1, text2, n, want = three_routes(rng, totals, True)
    (plain, counts), = run(tp, text1, text2, n, False)
    assert counts == [len(w) for w in want]
    first, second = run(tp, text1, text2, n, BGZF, runs=2)
    assert first == second and first[1] == counts
    for r in range(3):
        for m in range(2):
            assert plain[r][m] == fastq(want[r]) and len(plain[r][m]) == totals[r], (r, m)
            blocks = check(first[0][r][m], plain[r][m], what=(totals, r, m))
            assert len(blocks) == (totals[r] + CHUNK - 1) // CHUNK


def test_fasta_route():
    recs = records_for(40000, random.Random(25))
    plain, blocks = single_end(recs, text_of=fasta, is_fasta=True, fasta_routes=0x01)
    names = sum(1 for t in blocks[0][0].blocks[0].tokens if t[0] == "match" and t[2] > 1)
    assert names > 0.9 * plain[:CHUNK].count(b">") - 2


def test_interleaved_route_is_one_series_of_blocks():
    rng = random.Random(26)
    recs = records_for(20000, rng)
    mate2 = [(n, bytes(rng.choices(b"AC", k=len(s) - 1)) + b"C" * min(len(s), 1), q) for n, s, q in recs]
    tp = make_plan(paired=True)
    woven = b"".join(fastq([a]) + fastq([b]) for a, b in zip(recs, mate2))
    (plain, counts), = run(tp, fastq(recs), fastq(mate2), len(recs), False, interleave_out=True)
    assert counts == [len(recs), 0, 0] and plain[0] == [woven, b""] and len(woven) == 40000
    (packed, _counts), = run(tp, fastq(recs), fastq(mate2), len(recs), BGZF, interleave_out=True)
    assert packed[0][1] == b""
    assert len(check(packed[0][0], woven)) == 2


def test_three_barcodes():
    from test_gpu_demux import barcode_set, scheme_with
    rng = random.Random(27)
    codes = barcode_set(rng, 3, 8, 4)
    tp = make_plan(scheme=scheme_with(codes[0]), barcodes=codes)
    per_barcode = [700, 1, 150]  # two chunks, one record, one chunk
    recs, want = [], [[] for _ in range(3 + len(codes))]
    for b, count in enumerate(per_barcode):
        for i in range(count):
            name, seq, qual = ordinary(rng, len(recs), 40)
            umi = bytes(rng.choices(b"AC", k=8))
            recs.append((name, codes[b].encode() + umi + seq, b"F" * 16 + qual))
            want[3 + b].append((name + b"_" + umi, seq, qual))
    rng.shuffle(recs)
    order = {n: i for i, (n, _s, _q) in enumerate(recs)}
    for w in want:
        w.sort(key=lambda rec: order[rec[0].rsplit(b"_", 1)[0]])
    text = fastq(recs)
    (plain, counts), = run(tp, text, None, len(recs), False, bins=len(codes))
    (packed, counts2), = run(tp, text, None, len(recs), BGZF, bins=len(codes))
    assert counts2 == counts == [len(w) for w in want]
    for r in range(3 + len(codes)):
        assert plain[r][0] == fastq(want[r]), r
        check(packed[r][0], plain[r][0], what=r)
    assert len(plain[3][0]) > CHUNK and bgzf_out_rule.split_blocks(packed[4][0]).__len__() == 1


def test_info_table():
    """CS_INFO_GZIP on a handle with compress = 2: the table leaves as blocks too (runs only: no line starts with '@')."""
    rng = random.Random(28)
    recs = [ordinary(rng, i, 40) for i in range(400)]
    want = b"".join(n + b"\t-1\t" + s + b"\t" + q + b"\t\n" for n, s, q in recs)
    text = fastq(recs)
    with TrimEngine(make_plan(), device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=len(text) + 1024, max_records=len(recs), stride=152,
                                 compress=BGZF, info=abi.CS_INFO_ON | abi.CS_INFO_GZIP) as te:
            te.submit(0, text, len(text), None, 0, len(recs))
            res = te.wait(0)
            size, raw, rows = te.info(0)
            table = np.empty(max(size, 1), dtype=np.uint8)
            te.fetch_info(0, table)
            out = np.empty(max(int(res.out_bytes[0]), 1), dtype=np.uint8)
            te.fetch(0, out, None)
    assert rows == len(recs) and raw == len(want) > CHUNK
    blocks = check(table[:size].tobytes(), want)
    assert len(blocks) == 2 and all(d for _, d in blocks)
    assert all(t[0] == "lit" or t[2] == 1 for m, _ in blocks for t in m.tokens)
    check(out[:int(res.route_bytes[0][0])].tobytes(), text)


# ---- a slot's tables from one batch to the next -----------------------------------------------------------------

def test_a_shorter_batch_behind_a_longer_one():
    """Two batches on one slot, the second shorter, with fewer chunks in every route: chunk tables and sizes of the first
    must not show in the second."""
    rng = random.Random(29)
    tp, a1, a2, na, want_a = three_routes(rng, [2 * CHUNK + 100, 700, CHUNK + 9], True)
    _tp, b1, b2, nb, want_b = three_routes(rng, [CHUNK - 5, 0, 303], True)
    size = max(len(a1), len(a2)) + 1024
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=size, max_records=na, stride=152, compress=BGZF) as te:
            got = [te.run(a1, na, a2), te.run(b1, nb, b2), te.run(a1, na, a2)]
    for (packed, counts), want in zip(got, (want_a, want_b, want_a)):
        assert counts == [len(w) for w in want]
        for r in range(3):
            for m in range(2):
                check(packed[r][m], fastq(want[r]), what=(r, m))
    assert got[0] == got[2]
