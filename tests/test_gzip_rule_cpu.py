"""tests/gzip_rule.py held to zlib and to hand-written expectations: the strict member parser, the Huffman references
and the matcher rule that tests/test_gpu_gzip_structure.py holds the device's gzip writer to.  No GPU, no product code."""
import itertools
import random
import struct
import zlib
from functools import lru_cache

import pytest

import bgzf_rule
import gzip_rule
from gzip_rule import GzipError, parse_member


def wrap(payload: bytes, text: bytes) -> bytes:
    return gzip_rule.HEADER + payload + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def L(data: bytes):
    return [("lit", b) for b in data]


# ---- (a) the parser --------------------------------------------------------------------------------------------

def test_parser_reinflates_what_zlib_wrote():
    """Every block of bgzf_rule.universe() (levels 0/1/6/9, Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY, sync and full flushes) as a
    gzip member: the text comes back, and the tokens replayed through the trivial expander give zlib's output."""
    seen = set()
    for case, text in bgzf_rule.universe():
        m = parse_member(wrap(case.payload, text))
        assert m.text == text == zlib.decompress(case.payload, -15), case.name
        if len(text) <= 20000 or case.name.startswith("far"):  # (the byte-wise expander is slow: the small and the far ones)
            assert gzip_rule.expand(m.tokens) == text, case.name
        assert sum(b.raw_len for b in m.blocks) == len(text) and m.blocks[-1].final
        assert all(a.end_bit == b.start_bit for a, b in zip(m.blocks, m.blocks[1:])), case.name
        seen |= {b.btype for b in m.blocks}
        for b in m.blocks:
            if b.btype == 2:
                assert len(b.litlen) == 286 and len(b.dist) == 30 and len(b.clen) == 19
                assert b.hlit + 257 <= 286 and b.hdist + 1 <= 30 and b.hclen + 4 <= 19
                assert gzip_rule.kraft(b.litlen) == 1 and gzip_rule.kraft(b.clen) == 1
    assert seen == {0, 1, 2}


def good_member():
    """A dynamic block, an empty stored block (sync flush), the final block."""
    text = bgzf_rule.fastq_text(3000, seed=5)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(text) + c.flush(zlib.Z_SYNC_FLUSH) + c.flush()
    data = wrap(payload, text)
    m = parse_member(data)
    assert [b.btype for b in m.blocks] == [2, 0, 1] and m.text == text
    return data, m


def set_bits(data: bytes, bit: int, n: int, value: int) -> bytes:
    out = bytearray(data)
    for k in range(n):
        byte, sh = (bit + k) >> 3, (bit + k) & 7
        out[byte] = (out[byte] & ~(1 << sh)) | (((value >> k) & 1) << sh)
    return bytes(out)


def corruptions():
    data, m = good_member()
    n = len(data)
    flip = lambda at: data[:at] + bytes([data[at] ^ 0x10]) + data[at + 1:]
    stored = m.blocks[1]
    nlen_at = (stored.start_bit + 3 + 7) // 8 + 2  # behind BFINAL / BTYPE, at the byte boundary: LEN, then NLEN
    assert data[nlen_at - 2:nlen_at + 2] == b"\x00\x00\xff\xff"
    dyn = m.blocks[0]
    first = next(i for i in range(dyn.hclen + 4) if dyn.clen[gzip_rule._CLEN_ORDER[i]] != 1)
    return [
        ("crc", flip(n - 8), "CRC-32"),
        ("isize", flip(n - 4), "ISIZE"),
        ("nlen", data[:nlen_at] + b"\xfe" + data[nlen_at + 1:], "NLEN"),
        # one more code of one bit in a code-length code that was complete
        ("oversubscribed", set_bits(data, dyn.start_bit + 17 + 3 * first, 3, 1), "over-subscribed"),
        ("cut-trailer", data[:-3], "truncated"),
        ("cut-body", data[:n // 2], "truncated"),
        ("garbage", data + b"\0", "behind the trailer"),
    ]


@pytest.mark.parametrize("k", range(7))
def test_parser_refuses_corruptions(k):
    name, data, word = corruptions()[k]
    with pytest.raises(GzipError, match=word) as exc:
        parse_member(data)
    assert any(ch.isdigit() for ch in str(exc.value)), (name, str(exc.value))  # (the offset)


def hand_made(dist_bit: int, second_dist_len: int = 0) -> bytes:
    """'A', then a match of length 3 and distance 1, in a dynamic block whose distance code is ONE code of one bit
    (``second_dist_len``: a second distance code).  ``dist_bit``: the bit sent for the distance."""
    b = bgzf_rule._Bits()
    b.put(1, 1); b.put(2, 2); b.put(1, 5); b.put(1 if second_dist_len else 0, 5); b.put(15, 4)
    lens = {0: 2, 1: 2, 2: 2, 18: 2}  # canonical: 0 -> 00, 1 -> 01, 2 -> 10, 18 -> 11
    for sym in bgzf_rule._CLEN_ORDER:
        b.put(lens.get(sym, 0), 3)
    for zeros in (65,):
        b.code(3, 2); b.put(zeros - 11, 7)
    b.code(1, 2)                      # 'A': one bit
    b.code(3, 2); b.put(138 - 11, 7)  # 66 .. 255: 190 zeros
    b.code(3, 2); b.put(52 - 11, 7)
    b.code(2, 2); b.code(2, 2)        # 256 and 257: two bits
    b.code(1, 2)                      # distance symbol 0: one bit
    if second_dist_len:
        b.code(second_dist_len, 2)
    b.code(0, 1)                      # 'A'
    b.code(3, 2)                      # 257: length 3
    b.code(dist_bit, 1)
    b.code(2, 2)                      # end of block
    return wrap(b.done(), b"AAAA")


def test_parser_accepts_the_single_one_bit_distance_code_and_nothing_else_incomplete():
    data = hand_made(0)
    assert zlib.decompress(data, 31) == b"AAAA"  # (zlib takes it too)
    m = parse_member(data)
    assert m.text == b"AAAA" and m.tokens == [("lit", 65), ("match", 3, 1)]
    assert m.blocks[0].dist == [1] + [0] * 29
    with pytest.raises(GzipError, match="symbol with no code"):
        parse_member(hand_made(1))  # the other bit pattern: no symbol has it
    assert parse_member(hand_made(0, second_dist_len=1)).tokens == [("lit", 65), ("match", 3, 1)]  # two codes: complete
    with pytest.raises(GzipError, match="distance 2 beyond the 1 bytes"):
        parse_member(hand_made(1, second_dist_len=1))
    with pytest.raises(GzipError, match="incomplete distance"):
        parse_member(hand_made(0, second_dist_len=2))  # lengths 1 and 2: half a bit pattern short


def test_parser_refuses_a_distance_beyond_the_output():
    b = bgzf_rule._Bits()  # fixed block: a match of length 3, distance 1, as the first token
    b.put(1, 1); b.put(1, 2); b.code(1, 7); b.code(0, 5); b.code(0, 7)
    with pytest.raises(GzipError, match="beyond the 0 bytes"):
        parse_member(wrap(b.done(), b"\0\0\0"))
    with pytest.raises(GzipError, match="beyond"):
        gzip_rule.expand([("lit", 1), ("match", 3, 2)])


# ---- (d) Huffman -----------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def feasible(n: int):
    return [ls for ls in itertools.product(range(1, max(n, 2)), repeat=n) if sum(2.0 ** -l for l in ls) <= 1.0]


@lru_cache(maxsize=None)
def brute_optimum(freqs: tuple) -> int:
    """The cheapest prefix code over ALL length vectors that satisfy Kraft's inequality (``freqs`` sorted)."""
    return min(sum(f * l for f, l in zip(freqs, ls)) for ls in feasible(len(freqs)))


def test_huffman_cost_is_the_brute_force_optimum():
    for n in range(1, 7):
        for freqs in itertools.product(range(1, 5), repeat=n):
            h = gzip_rule.huffman_cost(freqs)
            assert h.cost == brute_optimum(tuple(sorted(freqs))), freqs
            assert h.cost == sum(f * l for f, l in zip(freqs, h.lengths)) and h.depth == max(h.lengths)
            assert gzip_rule.kraft(h.lengths) == (1 if n > 1 else 0.5), freqs
            # within the limit the limited lengths are the tree's own, dealt out by rank
            lim = gzip_rule.limited_lengths(freqs, 15)
            assert gzip_rule.histogram(lim, 15) == gzip_rule.histogram(h.lengths, 15), freqs
            assert sum(f * l for f, l in zip(freqs, lim)) == h.cost
    assert gzip_rule.huffman_cost([0, 0, 0]).cost == 0
    h = gzip_rule.huffman_cost([0, 7, 0])
    assert (h.cost, h.depth, h.lengths) == (7, 1, [0, 1, 0])
    # ties take the leaf: 1 1 2 2 becomes the flat tree, not the chain of depth 3
    assert gzip_rule.huffman_cost([1, 1, 2, 2]).lengths == [2, 2, 2, 2]


def fibonacci(n: int):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


@pytest.mark.parametrize("n,maxlen", [(22, 15), (40, 15), (16, 7)])
def test_limited_lengths_on_fibonacci_frequencies(n, maxlen):
    rng = random.Random(n)
    freqs = fibonacci(n)
    rng.shuffle(freqs)
    freqs = [0, 0] + freqs[:5] + [0] + freqs[5:]
    h = gzip_rule.huffman_cost(freqs)
    assert h.depth == n - 1 > maxlen  # (the chain)
    lens = gzip_rule.limited_lengths(freqs, maxlen)
    assert max(lens) == maxlen and gzip_rule.kraft(lens) == 1
    assert all((l > 0) == (f > 0) for l, f in zip(lens, freqs))
    for (fa, la), (fb, lb) in itertools.combinations(zip(freqs, lens), 2):
        assert not (fa > fb > 0 and la > lb), (fa, la, fb, lb)  # a more frequent symbol is never longer
    assert sum(f * l for f, l in zip(freqs, lens)) > h.cost


def test_limited_lengths_equal_the_tree_where_it_fits():
    rng = random.Random(4)
    for _ in range(300):
        n = rng.randint(2, 60)
        freqs = [rng.choice([0, 1, 1, 2, 3, 5, 40, 1000]) * rng.randint(1, 3) for _ in range(n)]
        h = gzip_rule.huffman_cost(freqs)
        for maxlen in (7, 15):
            lens = gzip_rule.limited_lengths(freqs, maxlen)
            if sum(1 for f in freqs if f) >= 2:
                assert gzip_rule.kraft(lens) == 1 and max(lens) <= maxlen
            if h.depth <= maxlen:
                assert gzip_rule.histogram(lens, maxlen) == gzip_rule.histogram(h.lengths, maxlen)
                assert sum(f * l for f, l in zip(freqs, lens)) == h.cost


# ---- (c) the matcher -------------------------------------------------------------------------------------------

def toks(text, chunk=0, fasta=False, lz=True):
    got = gzip_rule.tokens(text, chunk, fasta, lz)
    base = chunk * gzip_rule.CHUNK
    assert gzip_rule.expand(got, text[:base]) == text[base:base + gzip_rule.CHUNK]  # whatever it finds, it is the text
    return got


def test_tokens_runs():
    assert toks(b"xAAAAy") == L(b"xAAAAy")  # three bytes equal to the one in front of them: no match
    assert toks(b"xAAAAAy") == L(b"xA") + [("match", 4, 1)] + L(b"y")
    assert toks(b"AAAAA") == L(b"A") + [("match", 4, 1)]  # (stream offset 0 has no byte in front)
    assert toks(b"AAAA") == L(b"AAAA")
    assert toks(b"xAAAAAy", lz=False) == L(b"xAAAAAy")
    # across a slice's end: two matches
    text = b"ab" * 60 + b"G" * 20 + b"y"
    assert toks(text) == L(b"ab" * 60 + b"G") + [("match", 7, 1), ("match", 12, 1)] + L(b"y")
    # ... and a stretch of three behind the edge stays literal: the cap cuts a run, it does not lengthen one
    text = b"ab" * 60 + b"G" * 11 + b"y"
    assert toks(text) == L(b"ab" * 60 + b"G") + [("match", 7, 1)] + L(b"GGGy")
    # position 0 of chunk 1: the byte in front of the chunk counts
    text = (b"ab" * 16384)[:-1] + b"Q" + b"QQQQQz"
    assert len(text) == 32768 + 6
    assert toks(text, 1) == [("match", 5, 1)] + L(b"z")
    assert toks(text, 0)[-3:] == L(b"baQ")


def test_tokens_names():
    a, b = b"@abX\nAC\n+\nIJ\n", b"@abY\nAC\n+\nIJ\n"
    assert toks(a + b) == L(a + b)  # three bytes in common
    a, b = b"@abcX\nAC\n+\nIJ\n", b"@abcY\nAC\n+\nIJ\n"
    assert toks(a + b) == L(a) + [("match", 4, 14)] + L(b"Y\nAC\n+\nIJ\n")
    assert toks(a + b + b) == L(a) + [("match", 4, 14)] + L(b"Y\nAC\n+\nIJ\n") + [("match", 14, 14)]
    # 130 bytes in common, the second record at a slice's start: 128 of them, the rest literals
    name = (b"abcdefghij" * 25)[:246]
    a = b"@" + name + b"\nAC\n+\nIJ\n"
    b = b"@" + name[:129] + b"Z" + name[130:] + b"\nAC\n+\nIJ\n"
    assert len(a) == 256 and a[:130] == b[:130] and a[130] != b[130]
    assert toks(a + b) == L(a) + [("match", 128, 256)] + L(b[128:])
    # ... one byte later: capped at 127
    a = b"@" + name + b"k\nAC\n+\nIJ\n"
    assert toks(a + b) == L(a) + [("match", 127, 257)] + L(b[127:])
    # a record start and a run at the same place: the name first, the run where the name gives nothing
    a, b = b"@@@@@@x\nAC\n+\nIJ\n", b"@@@@@y\nAC\n+\nIJ\n"
    assert toks(a + b) == L(b"@") + [("match", 5, 1)] + L(b"x\nAC\n+\nIJ\n") + [("match", 5, 16)] + L(b"y\nAC\n+\nIJ\n")
    a, b = b"@@@@@@x\nAC\n+\nIJ\n", b"@Z@@@@@y\nAC\n+\nIJ\n"
    assert toks(a + b) == L(b"@") + [("match", 5, 1)] + L(b"x\nAC\n+\nIJ\n@Z@") + [("match", 4, 1)] + L(b"y\nAC\n+\nIJ\n")


def records64(first_extra: int = 0):
    recs = [b"@name%04d" % i + (b"klmnopqrst" * 5)[:46] + b"\nAC\n+\nIJ\n" for i in range(520)]
    assert all(len(r) == 64 for r in recs)
    recs[0] = recs[0][:9] + b"u" * first_extra + recs[0][9:]
    return recs


def test_tokens_predecessor_in_the_chunk_in_front():
    recs = records64()
    text = b"".join(recs)
    # chunk 1 starts with record 512: its predecessor lies in chunk 0, record 513's at chunk position 0
    got = toks(text, 1)
    assert got[:64] == L(recs[512]) and got[64] == ("match", 8, 64) and got[65:121] == L(recs[513][8:])
    assert toks(text, 0)[64:121] == [("match", 8, 64)] + L(recs[1][8:])
    # chunk 1 starts one byte early, with record 511's last line end: record 512 is line 1, record 513 line 5
    text = b"".join(records64(1))
    got = toks(text, 1)
    assert got[:65] == L(b"\n" + recs[512]) and got[65] == ("match", 8, 64)
    # chunk 1 starts inside record 511's name: record 512 is line 4, and what lies four lines back is no line start
    text = b"".join(records64(60))
    assert text[32768 - 1] != 10 and text[32768:].index(b"@name0512") == 60
    got = toks(text, 1)
    assert got[:124] == L(text[32768:32768 + 124])
    assert got[124] == ("match", 4, 64)  # record 513, four bytes in front of the slice's end: eight in common, four taken


def test_tokens_fasta():
    a, b, c = b">abcdX\nACAC\n", b">abcdY\nACAC\n", b">abcdZ\nACAC\n"
    want = L(a) + [("match", 5, 12)] + L(b"Y\nACAC\n") + [("match", 5, 12)] + L(b"Z\nACAC\n")
    assert toks(a + b + c, fasta=True) == want
    assert toks(a + b + c, fasta=False) == L(a + b + c)  # '>' is no record start in a FASTQ stream ...
    q = b"@abcdX\nAC\n+\nIJ\n"
    assert toks(q + q, fasta=True) == L(q + q)           # ... nor '@' in a FASTA stream
    # two lines back, not four: the third record against the second
    assert toks(a + c + c, fasta=True) == L(a) + [("match", 5, 12)] + L(b"Z\nACAC\n") + [("match", 12, 12)]


def test_tokens_line_cap():
    """Tiny identical records, twelve bytes and four lines each: record k is line 4 k, so records 1 .. 576 have a
    predecessor in the line index (4 k - 4 < 2304) and records 577 .. do not.  A match runs to its slice's end (the text
    is periodic)."""
    rec = b"@abcd\nA\n+\nI\n"
    text = rec * 600
    want = []
    for lo in range(0, len(text), 128):
        hi = min(lo + 128, len(text))
        start = max((lo + 11) // 12, 1) * 12  # the slice's first record start with a record in front of it
        if start < hi and start // 12 <= 576:
            want += L(text[lo:start]) + [("match", hi - start, 12)]
        else:
            want += L(text[lo:hi])
    got = toks(text)
    assert got == want
    at = 0  # the last match starts at record 576 or in front of it, and record 576's slice has one
    for t in got:
        if t[0] == "match":
            last = at
        at += 1 if t[0] == "lit" else t[1]
    assert last == 576 * 12
    assert gzip_rule.MAX_LINES == 2304
