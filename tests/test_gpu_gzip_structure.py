"""The device gzip writer (cutseq_amd/csrc/deflate_kernels.hip.inc) held to tests/gzip_rule.py: every member through
the strict parser, its layout against the kernel file's header comment, the tokens of every dynamic chunk against the
matcher rule, and every Huffman code against the optimal / length-limited references.  tests/test_gpu_text.py's
round-trip tests say that a member inflates to the text; these say WHAT the member is.

All cases go through ``textpath.TextEngine(..., compress=True)`` on plans that let records through unchanged (no
quality trimming, reads over {A, C}: neither adapter of the scheme finds anything in them), the expected text is what
the same engine returns with ``compress=False``, and every case first holds that text to the bytes it meant to build."""
import random

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, textpath
from cutseq_amd.engine import TrimEngine

import gzip_rule
import util

pytestmark = pytest.mark.gpu

SCHEME = "ACACGACGCTCTTCCGATCT>AGATCGGAAGAGCACACGTC"
INLINE = "ACACGACGCTCTTCCGATCT(GGG)>AGATCGGAAGAGCACACGTC"  # the same with an inline barcode: reads without it are "untrimmed"
CHUNK = gzip_rule.CHUNK
# a dynamic block's header: 17 bits, 19 code-length lengths of 3 bits, 316 code lengths of 1 .. 7 bits each
HEADER_MIN, HEADER_MAX = (17 + 57 + 316) // 8, 300
# name bytes: everything but NUL, what str.split() or a latin-1 reader could take for white space, and the line ends
NAME_BYTES = bytes(b for b in range(1, 256) if b not in b" \t\n\v\f\r\x1c\x1d\x1e\x1f\x85\xa0")


def make_plan(paired=False, min_length=0, untrimmed=False, scheme=SCHEME, barcodes=None):
    st = planmod.CutadaptConfig()
    st.min_length = min_length
    st.min_quality = -1000  # nothing is quality-trimmed, whatever the bytes say
    if barcodes:
        st.demux_barcodes = barcodes
    return util.compile_plan(scheme, st, paired, untrimmed_requested=untrimmed)


def fastq(recs) -> bytes:
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def fasta(recs) -> bytes:
    return b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _q in recs)


def pad(k: int) -> bytes:
    return (b"klmnopqrstuvw" * (k // 13 + 1))[:k]


def ordinary(rng, i: int, L: int, tag=b"SIM:7:FC"):
    """A record as sequencers write them: a name that shares all but a coordinate with its neighbours', bases without
    an adapter (the last one C: no 3' adapter starts there), qualities in runs of a few values."""
    seq = bytes(rng.choices(b"AC", k=max(L - 1, 0))) + b"C" * min(L, 1)
    qual = b"".join(bytes([rng.choice(b"IIII9-F")]) * 5 for _ in range(L // 5 + 1))[:L]
    return tag + b":%d:%d" % (1101 + i // 997, 10000 + 3 * i), seq, qual


def noisy(rng, i: int, L: int):
    """A record that hardly shrinks: 150 name bytes drawn uniformly from NAME_BYTES, no bases."""
    return bytes(rng.choices(NAME_BYTES, k=149)) + b"x", b"", b""


def records_for(total: int, rng, L=40, make=ordinary, first=0):
    """Records whose FASTQ text has exactly ``total`` bytes: ``make``'s, and a last one whose name is padded to land on
    the byte (a record takes name + 2 L + 6 bytes)."""
    recs, left = [], total
    while left > 420:
        recs.append(make(rng, first + len(recs), L))
        left -= len(recs[-1][0]) + 2 * len(recs[-1][1]) + 6
    while left:
        assert left >= 6, total
        take = left if left <= 250 else left - 130
        L_last = min(L, (take - 7) // 2) if take >= 7 else 0
        _n, seq, qual = ordinary(rng, 0, L_last)
        recs.append((pad(take - 6 - 2 * L_last), seq, qual))
        left -= take
    assert len(fastq(recs)) == total
    return recs


def run(tp, text1, text2, n, compress, runs=1, **kw):
    """-> [(streams[route][mate], counts)] of ``runs`` batches on one slot of a fresh text engine."""
    size = max(len(text1), len(text2 or b""), 1) + 1024
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=size, max_records=max(n, 1), stride=152, compress=compress, **kw) as te:
            return [te.run(text1, n, text2) for _ in range(runs)]


def check_codes(blk, what):
    """One dynamic block's three codes against its own tokens."""
    lit, dist = gzip_rule.frequencies(blk.tokens)
    cl = [blk.cl_symbols.count(s) for s in range(19)]
    coded = 0
    for name, freqs, lens, maxlen in (("literal/length", lit, blk.litlen, 15), ("distance", dist, blk.dist, 15),
                                      ("code-length", cl, blk.clen, 7)):
        w = (what, name)
        used = [s for s, f in enumerate(freqs) if f]
        assert max(lens) <= maxlen, w
        assert [s for s, l in enumerate(lens) if l] == used, w  # a code for every symbol of the block, and for no other
        single = name == "distance" and len(used) == 1 and lens[used[0]] == 1
        assert gzip_rule.kraft(lens) == 1 or single, w
        by_freq = {}
        for s in used:
            by_freq.setdefault(freqs[s], []).append(lens[s])
        order = sorted(by_freq)
        for lo, hi in zip(order, order[1:]):  # a more frequent symbol is never longer
            assert max(by_freq[hi]) <= min(by_freq[lo]), (w, lo, hi)
        h = gzip_rule.huffman_cost(freqs)
        bits = sum(freqs[s] * lens[s] for s in used)
        if h.depth <= maxlen:
            assert bits == h.cost, (w, bits, h.cost)
        # beyond the limit: the miniz-style histogram; within it that IS the tree's (test_gzip_rule_cpu.py), ties taking
        # the leaf -- another optimal tree of another shape is not what the kernel file describes
        assert gzip_rule.histogram(lens, maxlen) == gzip_rule.histogram(gzip_rule.limited_lengths(freqs, maxlen), maxlen), w
        if name != "code-length":
            coded += bits
    coded -= blk.dist[0]  # (counted once more than used)
    assert blk.end_bit - blk.data_bit == coded + gzip_rule.extra_bits(blk.tokens), what


def model_bytes(toks) -> float:
    """What an optimal code without a length limit takes for these tokens, header aside."""
    lit, dist = gzip_rule.frequencies(toks)
    hd = gzip_rule.huffman_cost(dist)
    return (gzip_rule.huffman_cost(lit).cost + hd.cost - hd.lengths[0] + gzip_rule.extra_bits(toks)) / 8


def check_stream(packed: bytes, plain: bytes, is_fasta=False, lz=True, what=""):
    """parse_member, check_layout, the text, and every dynamic chunk's tokens and codes -> the chunks."""
    member = gzip_rule.parse_member(packed)
    chunks = gzip_rule.check_layout(member, plain)
    assert member.text == plain, what
    for ch in chunks:
        want = gzip_rule.tokens(plain, ch.index, is_fasta, lz)
        size = gzip_rule.dynamic_chunk_bytes(want)
        if not ch.dynamic:  # stored for a reason: the dynamic form would be no smaller, or would not fit the bit buffer
            assert size >= ch.raw_len + 5 or size > gzip_rule.MAX_DYNAMIC, (what, ch.index, size)
        else:
            if ch.block.tokens != want:
                k = next((i for i, (a, b) in enumerate(zip(ch.block.tokens, want)) if a != b), min(len(want), len(ch.block.tokens)))
                raise AssertionError(f"{what}: chunk {ch.index}, token {k}: the device has {ch.block.tokens[k:k + 3]}, the rule {want[k:k + 3]}")
            check_codes(ch.block, (what, ch.index))
            assert ch.n_bytes == size, (what, ch.index, ch.n_bytes, size)
    return chunks


def single_end(recs, lz=True, text_of=fastq, is_fasta=False, what="", **kw):
    """``recs`` single-end through the plain plan: the uncompressed form is ``text_of(recs)``, the compressed one is
    held to the rule -> (plain, chunks)."""
    tp = make_plan()
    text = fastq(recs)
    (plain, counts), = run(tp, text, None, len(recs), False, **kw)
    want = text_of(recs)
    assert counts == [len(recs), 0, 0] and plain[0][0] == want and len(want) > 0, what
    (packed, counts2), = run(tp, text, None, len(recs), True, **kw)
    assert counts2 == counts and packed[1][0] == packed[2][0] == b""
    return want, check_stream(packed[0][0], want, is_fasta, lz, what)


# ---- lengths ---------------------------------------------------------------------------------------------------

# 1 and 2 bytes are no stream the text path can write: its shortest record is an empty FASTA record, ">\n\n" (3
# bytes); the shortest FASTQ record, "@\n\n+\n\n", has 6.  Those two and 7 stand for the smallest sizes.
SIZES = [3, 6, 7, 127, 128, 129, 255, 32767, 32768, 32769, 32768 + 127, 65536, 65537]


@pytest.mark.parametrize("size,lz", [(s, True) for s in SIZES] + [(129, False), (32769, False), (65537, False)])
def test_stream_lengths(size, lz, monkeypatch):
    """Streams of exactly ``size`` bytes: one slice and its neighbours (a last slice of 127 / 1 bytes: the CRC's
    x2nmodp path; 128: the table), one chunk and its neighbours, two chunks and one byte.  CUTSEQ_GPU_LZ=0: the same
    layout from literals alone."""
    if not lz:
        monkeypatch.setenv("CUTSEQ_GPU_LZ", "0")
    rng = random.Random(size)
    if size == 3:
        plain, chunks = single_end([(b"", b"", b"")], lz, fasta, True, size, fasta=True)
    else:
        plain, chunks = single_end(records_for(size, rng), lz, what=size)
    assert len(plain) == size and len(chunks) == (size + CHUNK - 1) // CHUNK
    if size >= 32767:
        assert chunks[0].dynamic  # (ordinary text: see test_ordinary_chunks_are_dynamic)
        if lz:
            assert sum(1 for t in chunks[0].block.tokens if t[0] == "match") > 300  # names and runs were there to find


# ---- alignment -------------------------------------------------------------------------------------------------

def three_routes(rng, totals, paired):
    """One batch whose trimmed / too-short / untrimmed streams have exactly ``totals`` bytes (per mate), under a plan
    with an inline barcode (GGG in front of mate 1: a pair without it is untrimmed), --min-length 10 and an untrimmed
    file -> (plan, text1, text2, n, want[route] records)."""
    want = [records_for(totals[0], rng, 40), records_for(totals[1], rng, 5), records_for(totals[2], rng, 40)]
    assert all(len(s) >= 10 for _n, s, _q in want[0] + want[2]) and all(len(s) < 10 for _n, s, _q in want[1])
    heads, order = [0, 0, 0], []
    while any(heads[r] < len(want[r]) for r in range(3)):  # the routes' records shuffled together, each in its order
        r = rng.choice([r for r in range(3) if heads[r] < len(want[r])])
        order.append((r, want[r][heads[r]]))
        heads[r] += 1
    # mate 1 loses the barcode where it has one; mate 2 always loses as many bases at its end (the barcode read through)
    text1 = fastq([(n, b"GGG" + s, b"FFF" + q) if r == 0 else (n, s, q) for r, (n, s, q) in order])
    text2 = fastq([(n, s + b"CCC", q + b"FFF") for _r, (n, s, q) in order]) if paired else None
    return make_plan(paired, min_length=10, untrimmed=True, scheme=INLINE), text1, text2, len(order), want


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("a", range(4))
def test_stream_base_alignment(a, paired):
    """Three non-empty routes in one batch: the streams lie back to back in the mate's buffer, so route 1 starts
    ``a`` bytes and route 2 ``a + 1`` bytes past a dword -- over the parametrisation every shift of the funnel-shift load,
    for both.  Paired: mate 2's buffer as well.  Two batches on the same slot give the same members."""
    rng = random.Random(40 + a)
    totals = [33000 + a, 301, 33002]
    assert totals[0] % 4 == a and (totals[0] + totals[1]) % 4 == (a + 1) % 4
    tp, text1, text2, n, want = three_routes(rng, totals, paired)
    (plain, counts), = run(tp, text1, text2, n, False)
    assert counts == [len(w) for w in want]
    mates = 2 if paired else 1
    for r in range(3):
        for m in range(mates):
            assert plain[r][m] == fastq(want[r]) and len(plain[r][m]) == totals[r], (r, m)
    first, second = run(tp, text1, text2, n, True, runs=2)
    assert first == second and first[1] == counts
    for r in range(3):
        for m in range(mates):
            check_stream(first[0][r][m], plain[r][m], what=(a, r, m))


# ---- stored or dynamic -----------------------------------------------------------------------------------------

def test_ordinary_chunks_are_dynamic():
    """(i) FASTQ text as sequencers write it is far from both thresholds: an optimal code for the rule's tokens plus the
    largest header a block can have stays below HALF of the bit buffer.  Such chunks must be dynamic."""
    recs = records_for(40000, random.Random(1))
    text = fastq(recs)
    for c in range(2):
        assert model_bytes(gzip_rule.tokens(text, c, False)) + HEADER_MAX < gzip_rule.MAX_DYNAMIC / 2
    _plain, chunks = single_end(recs)
    assert [ch.dynamic for ch in chunks] == [True, True]


def test_one_record_is_stored():
    """(ii) One small record: even an optimal code behind the smallest header a block can have is no shorter than the
    stored form."""
    recs = [(b"r", b"AC", b"IJ")]
    text = fastq(recs)
    assert model_bytes(gzip_rule.tokens(text, 0, False)) + HEADER_MIN >= len(text) + 5
    _plain, chunks = single_end(recs)
    assert [ch.dynamic for ch in chunks] == [False]


def shrinking_but_large(rng, i, L):
    """130 name bytes drawn uniformly from NAME_BYTES, 30 bases, 30 equal qualities: about three quarters of its size as
    a dynamic block."""
    return bytes(rng.choices(NAME_BYTES, k=129)) + b"x", bytes(rng.choices(b"AC", k=29)) + b"C", b"I" * 30


def test_chunk_that_shrinks_but_does_not_fit_is_stored():
    """(iii) Chunks that an optimal code brings well below their size (header included), but not below the 20472 bytes
    of the device's bit buffer: stored, by the second threshold alone."""
    recs = records_for(2 * CHUNK, random.Random(3), 30, shrinking_but_large)
    text = fastq(recs)
    for c in range(2):
        cost = model_bytes(gzip_rule.tokens(text, c, False))
        assert cost > gzip_rule.MAX_DYNAMIC and cost + HEADER_MAX < CHUNK, (c, cost)
    _plain, chunks = single_end(recs)
    assert [ch.dynamic for ch in chunks] == [False, False]


def partly_noisy(first: int):
    """Like shrinking_but_large with 42 drawn name bytes (the first record: ``first``) and letters for the rest."""
    def make(rng, i, L):
        k = first if i == 0 else 42
        return bytes(rng.choices(NAME_BYTES, k=k)) + pad(129 - k) + b"x", bytes(rng.choices(b"AC", k=29)) + b"C", b"I" * 30
    return make


@pytest.mark.parametrize("first,size", [(62, 20472), (72, 20473)])
def test_bit_buffer_threshold_to_the_byte(first, size):
    """The second threshold from both sides: a chunk whose dynamic form takes exactly the 20472 bytes the bit buffer
    holds is written that way, one byte more is stored.  The sizes are the rule file's (dynamic_chunk_bytes of the rule's
    tokens); the first record's name tunes them."""
    recs = records_for(CHUNK + 500, random.Random(1), 30, partly_noisy(first))
    assert gzip_rule.dynamic_chunk_bytes(gzip_rule.tokens(fastq(recs), 0, False)) == size < CHUNK
    _plain, chunks = single_end(recs)
    assert chunks[0].dynamic == (size <= gzip_rule.MAX_DYNAMIC)
    assert chunks[0].n_bytes == (size if chunks[0].dynamic else CHUNK + 5)


def test_stored_and_dynamic_chunks_alternate():
    """(iv) stored, dynamic, stored, dynamic in one stream, and each dynamic chunk begins inside a quality line that began
    in the stored chunk: twenty equal bytes in front of the chunk's start, twenty behind it.  The rule: a match of length
    20 and distance 1 as the chunk's first token -- it reaches into the stored chunk, the parser follows it there."""
    rng = random.Random(4)
    recs = []
    for half in range(2):
        recs += records_for(CHUNK - 75, rng, 0, noisy)       # hardly shrinks: stored
        recs.append((b"straddle%d:" % half, b"AC" * 20, b"I" * 40))  # 10 + 1 + 41 + 3 = 55 bytes in front of its qualities
        recs += records_for(CHUNK - 21 if half == 0 else 5000, rng, first=half * 1000)  # 96 - 75 = 21 bytes are the record's rest
    text = fastq(recs)
    assert len(text) == 3 * CHUNK + 21 + 5000
    for c in (1, 3):
        at = c * CHUNK
        assert text[at - 20:at + 20] == b"I" * 40 and text[at - 21] == text[at + 20] == 10
        want = gzip_rule.tokens(text, c, False)
        assert want[0] == ("match", 20, 1) and want[1] == ("lit", 10)
        assert model_bytes(want) + HEADER_MAX < gzip_rule.MAX_DYNAMIC / 2
    for c in (0, 2):
        assert model_bytes(gzip_rule.tokens(text, c, False)) > gzip_rule.MAX_DYNAMIC
    _plain, chunks = single_end(recs)
    assert [ch.dynamic for ch in chunks] == [False, True, False, True]
    assert chunks[1].block.tokens[0] == chunks[3].block.tokens[0] == ("match", 20, 1)


def test_every_byte_value_in_the_qualities(capsys):
    """The style of test_gpu_text.py's "every byte value" case, two chunks of it: near five of eight bits per byte, where
    the second threshold lies.  On which side it lands is printed, not asserted; whatever the device chose is held to
    the layout, and a dynamic chunk to the rule."""
    rng = random.Random(31)
    alphabet = [b for b in range(1, 256) if b not in (10, 13)]
    recs = []
    for i in range(215):
        qual = bytes(rng.choices(alphabet, k=148))
        recs.append((b"q%d" % i, bytes(rng.choices(b"AC", k=148)), qual.replace(b"@", b"A")))
    text = fastq(recs)
    _plain, chunks = single_end(recs)
    with capsys.disabled():
        for ch in chunks:
            print(f"\nevery byte value, chunk {ch.index}: {'dynamic' if ch.dynamic else 'stored'}, {ch.n_bytes} bytes for "
                  f"{ch.raw_len}; an optimal code for the rule's tokens: {model_bytes(gzip_rule.tokens(text, ch.index, False)):.0f}", end="")


# ---- formats and routes ----------------------------------------------------------------------------------------

def test_fasta_route():
    """``fasta_routes`` bit 0: the trimmed stream as FASTA -- '>' starts a record, the name two lines back."""
    recs = records_for(40000, random.Random(5))
    plain, chunks = single_end(recs, text_of=fasta, is_fasta=True, fasta_routes=0x01)
    names = sum(1 for t in chunks[0].block.tokens if t[0] == "match" and t[2] > 1)
    assert names > 0.9 * plain[:CHUNK].count(b">") - 2  # (nearly every record: FASTQ's rule would find none of them)


@pytest.mark.parametrize("mask", [0b011001, 0b100110])
def test_mixed_formats_in_one_batch(mask):
    """Streams of both formats in one launch (bit 2 * class + mate): every chunk takes the rule of ITS route's class."""
    rng = random.Random(6)
    totals = [33001, 2001, 9002]
    tp, text1, text2, n, want = three_routes(rng, totals, True)
    (plain, counts), = run(tp, text1, text2, n, False, fasta_routes=mask)
    (packed, counts2), = run(tp, text1, text2, n, True, fasta_routes=mask)
    assert counts2 == counts == [len(w) for w in want]
    for r in range(3):
        for m in range(2):
            is_fasta = bool((mask >> (2 * r + m)) & 1)
            assert plain[r][m] == (fasta if is_fasta else fastq)(want[r]), (r, m)
            chunks = check_stream(packed[r][m], plain[r][m], is_fasta, what=(mask, r, m))
            if r == 0:
                assert chunks[0].dynamic and any(t[0] == "match" and t[2] > 1 for t in chunks[0].block.tokens)


@pytest.mark.parametrize("per_barcode,mask", [(1, 0), (150, 0x40)], ids=["one read each", "fasta bins"])
def test_demultiplexed_routes(per_barcode, mask):
    """Route class 3: one stream per barcode behind the three fixed routes.  One read per barcode is the smallest batch
    that fills every barcode's route (one-record members: a record of two-letter bases and runs of qualities is
    smaller as a dynamic block than stored, check_layout holds either form to its bound); 150 each, as FASTA, are
    dynamic chunks under the rule of class 3's format."""
    from test_gpu_demux import barcode_set, scheme_with
    rng = random.Random(7)
    codes = barcode_set(rng, 4, 8, 4)
    tp = make_plan(scheme=scheme_with(codes[0]), barcodes=codes)
    recs, want = [], [[] for _ in range(3 + len(codes))]
    for i in range(per_barcode * len(codes)):
        b = i % len(codes)
        name, seq, qual = ordinary(rng, i, 40)
        umi = bytes(rng.choices(b"AC", k=8))
        recs.append((name, codes[b].encode() + umi + seq, b"F" * 16 + qual))
        want[3 + b].append((name + b"_" + umi, seq, qual))
    name, seq, qual = ordinary(rng, len(recs), 40)  # no barcode: untrimmed, and its first eight bases are taken for the UMI
    recs.append((name, b"CCCCCCCC" + seq, b"F" * 8 + qual))
    want[2].append((name + b"_CCCCCCCC", seq, qual))
    text = fastq(recs)
    kw = dict(bins=len(codes), fasta_routes=mask)
    (plain, counts), = run(tp, text, None, len(recs), False, **kw)
    (packed, counts2), = run(tp, text, None, len(recs), True, **kw)
    assert counts2 == counts == [len(w) for w in want]
    for r in range(3 + len(codes)):
        is_fasta = bool(mask >> 6) and r >= 3
        assert plain[r][0] == (fasta if is_fasta else fastq)(want[r]), r
        if not want[r]:
            assert packed[r][0] == b""
            continue
        chunks = check_stream(packed[r][0], plain[r][0], is_fasta, what=r)
        assert len(chunks) == 1 and (chunks[0].dynamic or per_barcode == 1 or r < 3)


def test_interleaved_output():
    """``interleave_out``: both mates' records woven into one stream, so the name four lines back is the other mate's
    record of the SAME pair -- the rule does not care whose, and neither may the device."""
    rng = random.Random(8)
    recs = records_for(20000, rng)
    mate2 = [(n, bytes(rng.choices(b"AC", k=len(s) - 1)) + b"C" * min(len(s), 1), q) for n, s, q in recs]
    tp = make_plan(paired=True)
    woven = b"".join(fastq([a]) + fastq([b]) for a, b in zip(recs, mate2))
    (plain, counts), = run(tp, fastq(recs), fastq(mate2), len(recs), False, interleave_out=True)
    assert counts == [len(recs), 0, 0] and plain[0] == [woven, b""] and len(woven) == 40000
    (packed, _counts), = run(tp, fastq(recs), fastq(mate2), len(recs), True, interleave_out=True)
    assert packed[0][1] == b""
    chunks = check_stream(packed[0][0], woven)
    whole = [t for t in chunks[0].block.tokens if t[0] == "match" and t[1] >= len(recs[0][0]) + 2]
    assert len(whole) > 80  # '@', the whole name and the line end: the mate's


def test_info_table():
    """The --info-file table with CS_INFO_GZIP goes through the same kernels as one more stream: layout, round trip, and
    the FASTQ rule's tokens (no line of the table starts with '@': runs only)."""
    rng = random.Random(9)
    recs = [ordinary(rng, i, 40) for i in range(400)]
    want = b"".join(n + b"\t-1\t" + s + b"\t" + q + b"\t\n" for n, s, q in recs)
    text = fastq(recs)
    tables = {}
    with TrimEngine(make_plan(), device=0, slots=0) as eng:
        for info in (abi.CS_INFO_ON, abi.CS_INFO_ON | abi.CS_INFO_GZIP):
            with textpath.TextEngine(eng, slots=1, max_text_bytes=len(text) + 1024, max_records=len(recs), stride=152, info=info) as te:
                te.submit(0, text, len(text), None, 0, len(recs))
                res = te.wait(0)
                size, raw, rows = te.info(0)
                table = np.empty(max(size, 1), dtype=np.uint8)
                te.fetch_info(0, table)
                te.fetch(0, np.empty(max(int(res.out_bytes[0]), 1), dtype=np.uint8), None)
                assert rows == len(recs)
                tables[info] = table[:size].tobytes()
    assert tables[abi.CS_INFO_ON] == want and len(want) > CHUNK
    chunks = check_stream(tables[abi.CS_INFO_ON | abi.CS_INFO_GZIP], want)
    assert all(ch.dynamic for ch in chunks)
    assert all(t[0] == "lit" or t[2] == 1 for ch in chunks for t in ch.block.tokens)


# ---- the line index's cap --------------------------------------------------------------------------------------

def test_line_cap():
    """Records of 16 bytes: 8192 line ends in a chunk, of which the device indexes 2304.  Record k of the chunk is line
    4 k: records 1 .. 576 find their predecessor's name, records 577 .. 2047 do not, and the next chunk starts over."""
    recs = [(b"abcd%04d" % i, b"A", b"I") for i in range(2100)]
    text = fastq(recs)
    assert len(text) == 2100 * 16 and text[:CHUNK].count(b"\n") > gzip_rule.MAX_LINES + 4
    want = gzip_rule.tokens(text, 0, False)
    at, last = 0, 0
    for t in want:
        if t[0] == "match":
            assert t[2] == 16 and at % 16 == 0
            last = at
        at += 1 if t[0] == "lit" else t[1]
    assert last == 576 * 16 and sum(1 for t in want if t[0] == "match") == 576
    _plain, chunks = single_end(recs)
    assert [ch.dynamic for ch in chunks] == [True, True]
    assert sum(1 for t in chunks[1].block.tokens if t[0] == "match") == 2100 - 2048 - 1
