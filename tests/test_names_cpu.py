"""CPU twin of tests/test_gpu_text_names.py (no GPU): the name universe of tests/names_universe.py through the HOST parser
and formatter (csh_fastq_parse / csh_format_chunk of cutseq_host.c, the CUTSEQ_TEXT_PATH=0 path) against the record
logic ``hostfmt`` -- and ``hostfmt.read_id`` itself against Python's ``str.split``, which is what the reference calls.
Specification, host C and device kernels are each held to the next: spec == str.split here, host C == spec here, device ==
spec in the GPU file.
"""
import numpy as np
import pytest

from cutseq_amd import abi, fastq, plan as planmod, synth
from cutseq_amd.common import BUILDIN_ADAPTERS

import hostfmt
import names_universe as nu
import util


def test_universe_sizes_and_pools():
    """19 608 + 2 801 names; every one of them in a pair; both pools well filled; the white space nobody tested before
    is in the mismatching pool: behind a ``\\v`` or a ``\\x1c`` the id goes on for dnaio's pair check."""
    assert len(nu.u1()) == 19_608 and len(nu.u2()) == 2_801
    assert not any(b"\n" in n for n in nu.u1() + nu.u2())
    matching, mismatching = nu.pools()
    assert len(set(matching)) == len(matching) and len(set(mismatching)) == len(mismatching)
    assert not set(matching) & set(mismatching)
    for blank in (b"\v", b"\f", b"\x1c"):
        assert (b"a" + blank, b"a" + blank + b"c2") in mismatching
    assert (b"a ", b"a c2") in matching and (b"a\t", b"a\tc2") in matching
    assert (b"a/1", b"a/2") in matching and (b"a.1/1", b"a.1/2") in matching and (b"/1", b"/1") in mismatching
    assert (b"a/1.1", b"a/1.2") in mismatching  # mate 1 loses '.1' and then '/1', mate 2 only '.2'
    sample = nu.mismatch_sample()
    assert len(sample) == 200 and sample == nu.mismatch_sample()
    assert any(b"\v" in a for a, _ in sample) and any(b"\x1c" in a for a, _ in sample)


def test_read_id_is_str_split_on_every_name():
    """``Renamer.parse_name`` is ``name.split(maxsplit=1)`` on a ``str``: ``\\x1c`` .. ``\\x1f`` separate fields there (and
    not for ``bytes.split``, which this specification used to call: 'a\\x1cb c' had the id 'a\\x1cb')."""
    for name in nu.u1() + nu.u2() + (b"a\x1cb c", b"a\x1db c", b"a\x1eb", b"\x1fa b", b"a\x1c", b"\x1c\x1d"):
        fields = name.decode("ascii").split(maxsplit=1)
        want = fields[0].encode() if len(fields) == 2 else name
        assert hostfmt.read_id(name) == want, name


def chunk_of(text1: bytes, text2, n: int, stride: int) -> fastq.Chunk:
    """The host parser on whole texts (what fastq.read_chunks does per block, without files and threads)."""
    h1 = fastq._parse("mate 1", text1, n, stride, 0)
    if text2 is None:
        return fastq.Chunk(n, stride, h1.raw, h1.name_off, h1.name_len, h1.seq, h1.qual, h1.lens)
    h2 = fastq._parse("mate 2", text2, n, stride, 0)
    return fastq.Chunk(n, stride, h1.raw, h1.name_off, h1.name_len, h1.seq, h1.qual, h1.lens,
                       h2.raw, h2.name_off, h2.name_len, h2.seq, h2.qual, h2.lens)


def fastq_text(names, seq, qual, lens, eol=b"\n"):
    return b"".join(b"@" + name + eol + seq[i, :int(lens[i])].tobytes() + eol + b"+" + eol + qual[i, :int(lens[i])].tobytes() + eol
                    for i, name in enumerate(names))


def spec_streams(tp, batch, names1, names2, r1, cap2, r2):
    recs = util.format_batch(tp, batch, names1, names2, r1, cap2, r2)
    streams = [[b"".join(x[1] for x in recs if x[0] == route),
                b"".join(x[2] for x in recs if x[0] == route) if names2 is not None else b""] for route in range(3)]
    return streams, [sum(1 for x in recs if x[0] == route) for route in range(3)]


@pytest.mark.parametrize("scheme", [nu.SCHEME_TWO_UMIS, nu.SCHEME_NO_UMI], ids=["two-umis", "no-umi"])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_host_formatter_on_every_name_single_end(scheme, eol):
    """U1 and U2, single end.  A name that ends in ``\\r`` is expected without it (the parser takes ``\\r\\n`` as the line
    end); with ``\\r\\n`` line ends the same names are written (names_universe.as_read), so the expectation is the same."""
    names = nu.single_names()
    tp = util.compile_plan(scheme, planmod.CutadaptConfig(), False)
    batch = synth.generate_pairs(len(names), nu.READ_LEN, scheme, seed=41, single_end=True, adapter_fraction=0.5)
    (r1, cap2, _), _ = util.oracle_run(tp, batch, threads=8)
    want, want_counts = spec_streams(tp, batch, [nu.as_read(n) for n in names], None, r1, cap2, None)
    assert sum(1 for c in want_counts if c) >= 2, want_counts
    written = names if eol == b"\n" else [nu.as_read(n) for n in names]
    c = chunk_of(fastq_text(written, batch.seq1, batch.qual1, batch.len1, eol), None, batch.n, batch.stride)
    data, counts = fastq.format_chunk(c, tp, r1, cap2, None)
    assert counts == want_counts
    for route in range(3):
        assert data[route][0] == want[route][0], route


@pytest.fixture(scope="module")
def paired_case():
    scheme = BUILDIN_ADAPTERS["TAKARAV3"]
    tp = util.compile_plan(scheme, planmod.CutadaptConfig(), True)
    assert tuple(s.encode() for s in tp.r1.name_suffixes) == nu.SUFFIXES[0]
    assert tuple(s.encode() for s in tp.r2.name_suffixes) == nu.SUFFIXES[1]
    return scheme, tp


def test_host_formatter_on_every_matching_pair(paired_case):
    scheme, tp = paired_case
    matching, _ = nu.pools()
    batch = synth.generate_pairs(len(matching), nu.READ_LEN, scheme, seed=42, adapter_fraction=0.5)
    (r1, cap2, _), (r2, _, _) = util.oracle_run(tp, batch, threads=8)
    names1, names2 = [a for a, _ in matching], [b for _, b in matching]
    want, want_counts = spec_streams(tp, batch, [nu.as_read(n) for n in names1], [nu.as_read(n) for n in names2], r1, cap2, r2)
    assert sum(1 for c in want_counts if c) >= 2, want_counts
    c = chunk_of(fastq_text(names1, batch.seq1, batch.qual1, batch.len1), fastq_text(names2, batch.seq2, batch.qual2, batch.len2),
                 batch.n, batch.stride)
    data, counts = fastq.format_chunk(c, tp, r1, cap2, r2)
    assert counts == want_counts
    for route in range(3):
        for m in range(2):
            assert data[route][m] == want[route][m], (route, m)


def test_host_formatter_names_the_first_mismatching_pair(paired_case):
    """200 mismatching pairs, each at one of the positions of names_universe.ERR_POSITIONS inside 600 matching pairs;
    two and three mismatching pairs (the first one counts); every pair mismatching (record 0)."""
    scheme, tp = paired_case
    good = nu.good_pairs()
    batch = synth.generate_pairs(nu.ERR_BATCH, nu.READ_LEN, scheme, seed=43)
    res = np.zeros(nu.ERR_BATCH, dtype=abi.RESULT_DTYPE)

    def run(pairs):
        c = chunk_of(fastq_text([a for a, _ in pairs], batch.seq1, batch.qual1, batch.len1),
                     fastq_text([b for _, b in pairs], batch.seq2, batch.qual2, batch.len2), batch.n, batch.stride)
        return fastq.format_chunk(c, tp, res, None, res.copy())

    run(good)
    sample = nu.mismatch_sample()
    for i, bad in enumerate(sample):
        k = nu.ERR_POSITIONS[i % len(nu.ERR_POSITIONS)]
        with pytest.raises(ValueError, match="Input read IDs not identical") as e:
            run(good[:k] + [bad] + good[k + 1:])
        assert e.value.record == k, (i, bad, k)
    for where in ((3, 300), (3, 300, 599), (300, 599)):
        pairs = list(good)
        for j, k in enumerate(where):
            pairs[k] = sample[j]
        with pytest.raises(ValueError) as e:
            run(pairs)
        assert e.value.record == where[0]
    _, mismatching = nu.pools()
    with pytest.raises(ValueError) as e:
        run(mismatching[:nu.ERR_BATCH])
    assert e.value.record == 0

