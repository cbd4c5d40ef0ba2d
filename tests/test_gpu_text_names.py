"""The header work of the text path on ODD NAMES: text_parse_records (SuffixRemover literals, the id field, the packed
``offset | length << 16``), text_check_pairs (dnaio's id comparison, the error key), format_copy (the id and UMI tag
copies) and the name column of info_copy -- against the C oracle's results formatted by the record logic ``hostfmt``.

Reference surface replaced: ``SuffixRemover``, ``Renamer.parse_name``, ``PairedEndRenamer`` and dnaio's
``record_names_match`` (cutseq/run.py:330, 377-380, 537-542, 642-645).  The names are ENUMERATED
(tests/names_universe.py: 19 608 + 2 801 of them, 47 854 matching and 2 812 mismatching pairs); tests/test_names_cpu.py
holds the specification to ``str.split`` and the host formatter to the specification on the same names.

A name that ends in ``\\r`` is expected WITHOUT that byte throughout: the line reader takes ``\\r\\n`` as the line end
(names_universe.as_read).
"""
import ctypes
import functools
import gzip
import random

import pytest

from cutseq_amd import abi, capi, plan as planmod, synth, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import info_rule
import names_universe as nu
import util
from test_gpu_info_file import run_with_info
from test_gpu_per_file_format import as_fasta
from test_gpu_text import fastq_text, oracle_streams, run_text

pytestmark = pytest.mark.gpu

TAKARAV3 = BUILDIN_ADAPTERS["TAKARAV3"]


def run_engine(tp, text1, text2, n, stride, **kw):
    """test_gpu_text.run_text with the engine's other switches (``compress``, ``fasta``)."""
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2 or b""), 1) + 1024,
                                 max_records=max(n, 1), stride=stride, **kw) as te:
            return te.run(text1, n, text2)


def as_read(names):
    return [nu.as_read(n) for n in names]


# ---- every name, single end ------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def single_case(scheme):
    """U1 then U2 on reads of 40 nt with the scheme's adapters planted -> (names, plan, batch, streams, counts); computed
    once, shared by the tests below."""
    names = nu.single_names()
    tp = util.compile_plan(scheme, planmod.CutadaptConfig(), False)
    batch = synth.generate_pairs(len(names), nu.READ_LEN, scheme, seed=41, single_end=True, adapter_fraction=0.5)
    streams, counts, _ = oracle_streams(tp, batch, as_read(names), None)
    assert sum(1 for c in counts if c) >= 2, counts  # routes are mixed
    if tp.has_umi:
        assert tp.needs_cap2 and streams[0][0].count(b"_") == counts[0]  # '{id}_{cut_prefix}{cut_suffix}', names hold no '_'
    return names, tp, batch, streams, counts


@pytest.mark.parametrize("compress", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("scheme", [nu.SCHEME_TWO_UMIS, nu.SCHEME_NO_UMI], ids=["two-umis", "no-umi"])
def test_every_name_single_end(scheme, compress):
    """U1 and U2 (22 409 records) through a plan with a UMI and two captures and through one without, as text and as gzip
    members written on the device (deflate_chunks' name matcher sees these names too): byte-identical per route."""
    names, tp, batch, want, want_counts = single_case(scheme)
    text = fastq_text(names, batch.seq1, batch.qual1, batch.len1)
    if not compress:
        got, counts = run_text(tp, text, None, batch.n, batch.stride)
    else:
        got, counts = run_engine(tp, text, None, batch.n, batch.stride, compress=True)
        got = [[gzip.decompress(x) if x else x for x in row] for row in got]
    assert counts == want_counts
    for route in range(3):
        assert got[route][0] == want[route][0], (route, textpath.ROUTES[route])


@pytest.mark.parametrize("eol,final_newline", [(b"\r\n", True), (b"\n", False)], ids=["crlf", "no-final-newline"])
def test_line_ends_around_odd_names(eol, final_newline):
    """The U2 batch with ``\\r\\n`` line ends and without the final newline: the expectation is the one of the ``\\n`` run.
    (The reader takes ONE ``\\r`` with the line end, so in front of ``\\r\\n`` a name that ends in ``\\r`` is written without
    it: the header line's bytes are the same as in the ``\\n`` run.)"""
    names, tp, batch, _, _ = single_case(nu.SCHEME_TWO_UMIS)
    lo = len(nu.u1())
    assert names[lo:] == list(nu.u2())
    sub = synth.SynthBatch(batch.seq1[lo:], batch.qual1[lo:], batch.len1[lo:], None, None, None)
    want, want_counts, _ = oracle_streams(tp, sub, as_read(names[lo:]), None)
    written = [nu.as_read(n) for n in names[lo:]] if eol == b"\r\n" else names[lo:]
    text = fastq_text(written, sub.seq1, sub.qual1, sub.len1, eol, final_newline)
    got, counts = run_text(tp, text, None, sub.n, sub.stride)
    assert counts == want_counts
    for route in range(3):
        assert got[route][0] == want[route][0], route


# ---- pairs -----------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def paired_plan():
    tp = util.compile_plan(TAKARAV3, planmod.CutadaptConfig(), True)  # '{id}_{r1.cut_prefix}{r2.cut_prefix}'
    assert tp.has_umi
    assert tuple(s.encode() for s in tp.r1.name_suffixes) == nu.SUFFIXES[0]
    assert tuple(s.encode() for s in tp.r2.name_suffixes) == nu.SUFFIXES[1]
    return tp


@functools.lru_cache(maxsize=None)
def paired_case():
    """The whole matching pool on reads of 40 nt -> (plan, names1, names2, batch)."""
    matching, _ = nu.pools()
    batch = synth.generate_pairs(len(matching), nu.READ_LEN, TAKARAV3, seed=42, adapter_fraction=0.5)
    return paired_plan(), [a for a, _ in matching], [b for _, b in matching], batch


def test_every_matching_pair():
    """The whole matching pool through TAKARAV3 paired as ONE batch: no error, both mates' streams equal
    hostfmt.format_pair."""
    tp, names1, names2, batch = paired_case()
    want, want_counts, _ = oracle_streams(tp, batch, as_read(names1), as_read(names2))
    assert sum(1 for c in want_counts if c) >= 2, want_counts
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2)
    got, counts = run_text(tp, text1, text2, batch.n, batch.stride)
    assert counts == want_counts
    for route in range(3):
        for m in range(2):
            assert got[route][m] == want[route][m], (route, m)


def test_info_table_carries_the_same_names():
    """info_copy has its own copy of the id: every 30th pair of the matching pool (1 596 pairs; the table's
    specification aligns in Python) with the info table on, the table compared WHOLE against tests/info_rule.py -- the
    name column holds tabs on these names, so it cannot be cut out of a row."""
    tp, names1, names2, batch = paired_case()
    sel = range(0, batch.n, 30)
    assert 1024 < len(sel) <= 4096

    def records(names, seq, qual, lens, read):
        return [((nu.as_read(names[i]) if read else names[i]), util.row_bytes(seq, lens, i), util.row_bytes(qual, lens, i)) for i in sel]

    want = info_rule.table(TAKARAV3, planmod.CutadaptConfig(), records(names1, batch.seq1, batch.qual1, batch.len1, True),
                           records(names2, batch.seq2, batch.qual2, batch.len2, True))
    assert any(row.count(b"\t") > 11 for row in want.split(b"\n"))  # names with tabs are there
    text1 = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in records(names1, batch.seq1, batch.qual1, batch.len1, False))
    text2 = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in records(names2, batch.seq2, batch.qual2, batch.len2, False))
    table, sizes, _streams, _res = run_with_info(tp, text1, text2, len(sel), batch.stride)
    assert sizes[2] == want.count(b"\n")
    assert table == want


def test_mismatching_pairs_are_found_and_the_first_one_is_named():
    """200 pairs of the mismatching pool (fixed seed; ``\\v`` and ``\\x1c`` names among them: for dnaio's rule only space and
    tab end an id), each inside 600 otherwise matching pairs at record 0, 63, 64, 255, 256, 257 or 599 in turn:
    CS_TEXT_ERR_IDS_DIFFER naming that record.  Then two and three mismatching pairs in different blocks of
    text_check_pairs (records 3, 300, 599): the SMALLEST record is named -- TextMeta.err is the smallest (record, code)
    key, and a thread must not leave because a later record's key is already there.  These cases pin the contract; they
    are not expected to catch that race reliably (it takes a block of a later record to finish its atomicMin before an
    earlier block reads the word), and nothing here loops to provoke it.  Last, every pair mismatching: record 0.
    After every error the same engine formats a good batch correctly."""
    tp = paired_plan()
    good = nu.good_pairs()
    batch = synth.generate_pairs(nu.ERR_BATCH, nu.READ_LEN, TAKARAV3, seed=43, adapter_fraction=0.5)
    want, want_counts, _ = oracle_streams(tp, batch, as_read([a for a, _ in good]), as_read([b for _, b in good]))

    def texts(pairs):
        return (fastq_text([a for a, _ in pairs], batch.seq1, batch.qual1, batch.len1),
                fastq_text([b for _, b in pairs], batch.seq2, batch.qual2, batch.len2))

    good1, good2 = texts(good)
    sample = nu.mismatch_sample()
    assert any(b"\v" in a for a, _ in sample) and any(b"\x1c" in a for a, _ in sample)
    _, mismatching = nu.pools()
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 17, max_records=nu.ERR_BATCH, stride=batch.stride) as te:

            def expect_error(pairs, record, what):
                t1, t2 = texts(pairs)
                with pytest.raises(textpath.TextFormatError) as e:
                    te.run(t1, nu.ERR_BATCH, t2)
                assert (e.value.code, e.value.record) == (abi.CS_TEXT_ERR_IDS_DIFFER, record), what
                streams, counts = te.run(good1, nu.ERR_BATCH, good2)  # the engine is still usable, and right
                assert counts == want_counts and streams == want, what

            streams, counts = te.run(good1, nu.ERR_BATCH, good2)
            assert counts == want_counts and streams == want
            for i, bad in enumerate(sample):
                k = nu.ERR_POSITIONS[i % len(nu.ERR_POSITIONS)]
                expect_error(good[:k] + [bad] + good[k + 1:], k, (i, bad, k))
            for where in ((3, 300), (3, 599), (3, 300, 599), (300, 599)):
                pairs = list(good)
                for j, k in enumerate(where):
                    pairs[k] = sample[j]
                expect_error(pairs, where[0], where)
            expect_error(mismatching[:nu.ERR_BATCH], 0, "every pair")


# ---- long ids and long tags in format_copy ----------------------------------------------------------------------------

# format_copy's id copy: a dword at 4 * lane, one at 4 * lane + 128, a tail of n & 3 bytes, a loop from byte 256 on (steps
# of 128) -- lengths around every one of these borders, and the largest ones the 16-bit packing holds
ID_LENGTHS = ([0, 1, 2, 3, 4, 5, 7, 8] + list(range(124, 133)) + list(range(252, 261)) + list(range(380, 389))
              + list(range(4093, 4100)) + [65_533, 65_534, 65_535])
HEADER_MAX = 65_535
# paired schemes whose two UMIs give a tag ('_' + both captures) of 37 bytes (more than one byte per lane: the tag loop
# runs once for some lanes) and of 511 bytes (the loop runs 15 times).  255 is the longest N run the plan compiler takes
# for a captured cut (cs_result.cap_len is 8 bits), so 1 + 255 + 255 is the longest tag there is.  Reads of 40 nt hold 20 +
# 16 captured bases; the 255 + 255 of the other scheme need reads of 600 nt (single end, both captures come from one read)
TAG_SCHEMES = {"tag37": ("ACACGACGCTCTTCCGATCT" + "N" * 20 + "<" + "N" * 16 + "AGATCGGAAGAGCACACGTC", 40, 37),
               "tag511": ("ACACGACGCTCTTCCGATCT" + "N" * 255 + "<" + "N" * 255 + "AGATCGGAAGAGCACACGTC", 600, 511)}
LETTERS = bytes(random.Random(65535).choices(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", k=HEADER_MAX))


def long_headers():
    """[(header, what)]: every id length in three forms -- the id alone (a one-field header is its own id), ``<id> c`` and
    ``  <id> c`` (an id offset of 2); where the comment would take the header beyond 65 535 bytes the id gives way.  Plus
    65 500 blanks in front of ``id c``: a near-maximal id offset."""
    out = []
    for n in ID_LENGTHS:
        out.append((LETTERS[:n], ("alone", n)))
        out.append((LETTERS[:min(n, HEADER_MAX - 2)] + b" c", ("comment", n)))
        out.append((b"  " + LETTERS[:min(n, HEADER_MAX - 4)] + b" c", ("offset 2", n)))
    out.append((b" " * 65_500 + b"id c", ("offset 65500", 2)))
    return out


@functools.lru_cache(maxsize=None)
def long_case(tag, paired):
    """Every header of long_headers() at all four byte alignments of the text: in front of each record stands one whose
    name is 0 to 3 blanks (its pair id is empty in both mates), chosen so that the header starts at 0, 1, 2, 3 mod 4.
    -> (plan, batch, text1, text2 | None, names1, streams, counts)"""
    scheme, read_len, tag_len = TAG_SCHEMES[tag]
    st = planmod.CutadaptConfig()
    st.min_length = 0        # nothing is too short: the longest records reach the sink
    st.auto_rc = not paired  # single end: a reverse-complement plan, the byte-wise branch of format_copy
    tp = util.compile_plan(scheme, st, paired)
    assert tp.has_umi and (paired or (tp.reverse_complement and tp.needs_cap2))
    assert textpath.max_tag(tp) == tag_len
    headers = long_headers()
    n = 2 * 4 * len(headers)
    batch = synth.generate_pairs(n, read_len, scheme, seed=44, single_end=not paired, adapter_fraction=0.3)
    texts, all_names = [], []
    for seq, qual, lens in ((batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2))[:2 if paired else 1]:
        parts, names, at, i = [], [], 0, 0
        body = [b"\n" + util.row_bytes(seq, lens, k) + b"\n+\n" + util.row_bytes(qual, lens, k) + b"\n" for k in range(n)]
        for header, _what in headers:
            for align in range(4):
                fill = (align - (at + 1 + len(body[i]) + 1)) % 4  # '@' fill body '@' -> the header's first byte
                for name in (b" " * fill, header):
                    rec = b"@" + name + body[i]
                    parts.append(rec)
                    names.append(name)
                    at += len(rec)
                    i += 1
                assert (at - len(rec) + 1) % 4 == align
        texts.append(b"".join(parts))
        all_names.append(names)
    streams, counts, _ = oracle_streams(tp, batch, all_names[0], all_names[1] if paired else None)
    assert counts[0] == n
    longest = max(len(line) for line in streams[0][0].split(b"\n")[::4])
    assert longest == 1 + HEADER_MAX + tag_len, longest  # '@', a 65 535-byte id and the full tag: such a record is in the sink
    return tp, batch, texts[0], (texts[1] if paired else None), all_names[0], streams, counts


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single-rc"])
@pytest.mark.parametrize("tag", list(TAG_SCHEMES))
def test_long_ids_and_long_tags(tag, paired, fasta):
    """format_copy's id copy at every border of its four stretches and at all four alignments, ids up to the 65 535 bytes
    the packing holds, id offsets of 2 and of 65 500, UMI tags of 37 and 511 bytes -- paired and single end (reverse
    complement), FASTQ and FASTA records.  About 1 100 records, 3 MB of text per mate."""
    tp, batch, text1, text2, _names, want, want_counts = long_case(tag, paired)
    got, counts = run_engine(tp, text1, text2, batch.n, batch.stride, fasta=fasta)
    assert counts == want_counts
    for route in range(3):
        for m in range(2 if paired else 1):
            expect = as_fasta(want[route][m]) if fasta else want[route][m]
            if got[route][m] != expect:  # (not the 3 MB streams in the assertion message)
                a, b = got[route][m].split(b"\n"), expect.split(b"\n")
                first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                x, y = (a + [b""])[first], (b + [b""])[first]
                at = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                pytest.fail(f"route {route} mate {m}: line {first} differs at byte {at} (lengths {len(x)} / {len(y)}): "
                            f"{x[at:at + 16]!r} != {y[at:at + 16]!r}")


def test_header_limit():
    """A header of 65 536 bytes does not fit the 16-bit header length: CS_TEXT_ERR_MALFORMED naming that record, nothing
    is formatted (README, deviations); 65 535 bytes next to it are fine.  This pins what the code does."""
    tp = util.compile_plan(nu.SCHEME_NO_UMI, planmod.CutadaptConfig(), False)
    rec = lambda name: b"@" + name + b"\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n"
    ok = rec(b"first") + rec(LETTERS) + rec(b"last")
    bad = rec(b"first") + rec(LETTERS[:HEADER_MAX - 2] + b" c") + rec(LETTERS + b"x") + rec(b"last")
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 18, max_records=8, stride=24) as te:
            streams, counts = te.run(ok, 3, None)
            assert sum(counts) == 3 and b"@" + LETTERS + b"\n" in streams[0][0]
            te.submit(0, bad, len(bad), None, 0, 4)
            res = abi.cs_text_result()
            capi.check(te.L.cs_text_wait(te._h, 0, ctypes.byref(res)))
            assert (res.error, res.error_record) == (abi.CS_TEXT_ERR_MALFORMED, 2)
            assert list(res.route_count) == [0, 0, 0] and list(res.out_bytes) == [0, 0]
            assert all(int(res.route_bytes[q][m]) == 0 for q in range(3) for m in range(2))
            with pytest.raises(textpath.TextFormatError) as e:
                te.run(bad, 4, None)
            assert (e.value.code, e.value.record) == (abi.CS_TEXT_ERR_MALFORMED, 2)
            assert te.run(ok, 3, None) == (streams, counts)
