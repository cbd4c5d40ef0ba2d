"""BGZF input inflated on the device, the parts that need no GPU: the shared decoder as a host program under the
sanitizers, codec.bgzf_index, the reader's device mode over the host inflater, and the switch's paper work."""
import struct
import subprocess
import zlib
from pathlib import Path

import pytest

from cutseq_amd import abi, codec, fastq, switches

import bgzf_rule

ROOT = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------- the decoder, one lane, as its own program


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("inflate") / "inflate_host_check"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                    "-o", str(exe), str(ROOT / "tools" / "inflate_host_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("which", ["universe", "corrupt", "mutations"])
def test_shared_decoder_under_the_sanitizers(host_check, tmp_path, which):
    """Exit status 0 and no sanitizer report; every verdict ("refused or not") and every accepted text as zlib has it;
    the guard bytes around every output region untouched."""
    cases = {"universe": lambda: [c for c, _ in bgzf_rule.universe()], "corrupt": bgzf_rule.corrupt_cases,
             "mutations": bgzf_rule.mutations}[which]()
    assert len(cases) == {"universe": 56, "corrupt": 92, "mutations": 2000}[which]
    path = tmp_path / "cases.bin"
    bgzf_rule.write_case_file(path, cases)
    run = subprocess.run([str(host_check), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    rows = [tuple(map(int, line.split())) for line in run.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(len(cases)))
    accepted = 0
    for case, (_, verdict, adler, lines, guards) in zip(cases, rows):
        ok, text = bgzf_rule.expected(case)
        assert guards == 1, case.name
        assert (verdict == 0) == ok, (case.name, verdict)
        if ok:
            accepted += 1
            assert (adler, lines) == (zlib.adler32(text), text.count(b"\n")), case.name
    if which == "universe":
        assert accepted == len(cases)
    else:
        assert 0 < accepted < len(cases) // 10  # (a few flips hit bits that carry nothing)


def test_the_hand_made_blocks_fail_for_their_reason():
    """zlib's own words for the blocks assembled by hand: each one is refused for the reason it was built for."""
    want = {"stored-nlen": "stored block lengths", "btype-3": "invalid block type", "hlit-287": "too many length or distance",
            "clen-oversubscribed": "invalid code lengths set", "repeat-first": "invalid bit length repeat",
            "match-first": "invalid distance too far back", "no-end-of-block": "missing end-of-block"}
    cases = {c.name: c for c in bgzf_rule.corrupt_cases()}
    for name, words in want.items():
        with pytest.raises(zlib.error, match=words):
            zlib.decompressobj(-15).decompress(cases[name].payload)


# ---------------------------------------------------------------- codec.bgzf_index


def _rows_of(text, block_bytes, level=6):
    rows, at = [], 0
    data = bgzf_rule.bgzf(text, block_bytes, level)
    for lo in range(0, len(text), block_bytes):
        piece = text[lo:lo + block_bytes]
        payload = bgzf_rule.deflate_raw(piece, level)
        rows.append((at + 18, len(payload), len(piece), zlib.crc32(piece)))
        at += 18 + len(payload) + 8
    return data, rows


def test_bgzf_index():
    text = bgzf_rule.fastq_text(30000)
    data, rows = _rows_of(text, 4093)
    assert codec.bgzf_index(data, 0, len(data)) == (rows, len(data))
    assert codec.bgzf_index(data, 0, len(data) + 100) == (rows, len(data))
    # the EOF marker is an ordinary entry
    marked = data + bgzf_rule.EOF_MARKER
    got, end = codec.bgzf_index(marked, 0, len(marked))
    assert got == rows + [(len(data) + 18, 2, 0, 0)] and end == len(marked)
    assert codec.bgzf_index(bgzf_rule.EOF_MARKER, 0, 28) == ([(18, 2, 0, 0)], 28)
    # from the second block on; a span that ends inside a block stops in front of it
    second = rows[1][0] - 18
    assert codec.bgzf_index(data, second, len(data)) == (rows[1:], len(data))
    third = rows[2][0] - 18
    assert codec.bgzf_index(data, 0, third + 5) == (rows[:2], third)
    # a plain gzip member behind the run ends it
    import gzip
    mixed = data + gzip.compress(b"@tail\nACGT\n+\nIIII\n")
    assert codec.bgzf_index(mixed, 0, len(mixed)) == (rows, len(data))
    # a truncated last block ends it too
    assert codec.bgzf_index(data[:-3], 0, len(data)) == (rows[:-1], rows[-1][0] - 18)
    # other subfields in front of BC in the extra field
    piece = text[:1000]
    payload = bgzf_rule.deflate_raw(piece)
    odd = bgzf_rule.member(payload, zlib.crc32(piece), len(piece), extra_first=b"XY" + struct.pack("<H", 3) + b"abc")
    assert codec.bgzf_index(odd + data, 0, len(odd) + len(data))[0][:2] == [(12 + 7 + 6, len(payload), 1000, zlib.crc32(piece)),
                                                                           (len(odd) + 18, rows[0][1], rows[0][2], rows[0][3])]
    # a block that promises more text than the format allows is not BGZF
    big = bgzf_rule.member(payload, zlib.crc32(piece), 65537)
    assert codec.bgzf_index(big, 0, len(big)) == ([], 0)
    assert codec.bgzf_index(b"", 0, 0) == ([], 0)


# ---------------------------------------------------------------- the reader's device mode over the host inflater


@pytest.fixture
def unpinned(monkeypatch):
    monkeypatch.setattr(fastq, "PINNED", fastq._Arena())


def _blocks(reader):
    out = []
    while True:
        b = reader.get()
        if b is None:
            break
        src = b.dbuf if b.dbuf is not None else b.buf
        out.append((bytes(memoryview(src)[: b.nbytes]), b.n, b.first_record, b.dbuf is not None))
        b.release()
    reader.close()
    return out


def _records(n, seed=1):
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        k = rng.randint(0, 150) if i % 97 else 0
        out.append(b"@r%d 1:N:0\n%s\n+\n%s\n" % (i, "".join(rng.choice("ACGT") for _ in range(k)).encode(), b"F" * k))
    return out


_TAILS = {
    "plain-end": (b"", True), "no-eof-marker": (b"", False), "no-final-newline": (None, True), "blank-lines": (b"\n\n\r\n", True),
    "empty-last-read": (b"@e\n\n+\n\n", True), "empty-last-read-no-newline": (b"@e\n\n+\n", False),
}


@pytest.mark.parametrize("block_bytes", [700, 4093, 65280])
@pytest.mark.parametrize("tail", sorted(_TAILS))
def test_device_mode_hands_out_the_host_mode_s_blocks(tmp_path, unpinned, block_bytes, tail):
    from cutseq_amd import textio
    from cutseq_amd.inflater import HostInflater
    extra, marker = _TAILS[tail]
    body = b"".join(_records(1450))
    text = body[:-1] if extra is None else body + extra
    path = tmp_path / "in.fq.gz"
    path.write_bytes(bgzf_rule.bgzf(text, block_bytes, 1) + (bgzf_rule.EOF_MARKER if marker else b""))
    want = _blocks(textio.TextReader(str(path), 300))
    got = _blocks(textio.TextReader(str(path), 300, inflater=HostInflater))
    assert [b[:3] for b in got] == [b[:3] for b in want]
    assert [b[1] for b in got][:4] == [300] * 4 and sum(b[1] for b in got) == 1450 + (extra or b"").count(b"@e")
    assert [b[3] for b in got] == [True] * 4 + [False] * (len(got) - 4)  # whole blocks from the inflater, the rest from the host
    assert not any(b[3] for b in want)


def test_device_mode_bgzf_then_a_plain_member_and_the_marker_alone(tmp_path, unpinned):
    import gzip
    from cutseq_amd import textio
    from cutseq_amd.inflater import HostInflater
    recs = _records(1000, seed=2)
    cut = len(b"".join(recs[:620])) + 11  # the plain member begins in the middle of a record
    text = b"".join(recs)
    path = tmp_path / "mixed.fq.gz"
    path.write_bytes(bgzf_rule.bgzf(text[:cut], 4093, 6) + gzip.compress(text[cut:], 1))
    want = _blocks(textio.TextReader(str(path), 300))
    got = _blocks(textio.TextReader(str(path), 300, inflater=HostInflater))
    assert [b[:3] for b in got] == [b[:3] for b in want] and [b[1] for b in got] == [300, 300, 300, 100]
    assert [b[3] for b in got] == [True, True, False, False]
    # both mates decide on their own: a plain gzip file ignores the inflater
    plain = tmp_path / "plain.fq.gz"
    plain.write_bytes(gzip.compress(text, 1))
    called = []
    assert _blocks(textio.TextReader(str(plain), 300, inflater=lambda: called.append(1))) == want and not called
    # a file of the EOF marker alone: no records
    only = tmp_path / "marker.fq.gz"
    only.write_bytes(bgzf_rule.EOF_MARKER)
    assert _blocks(textio.TextReader(str(only), 300)) == [] == _blocks(textio.TextReader(str(only), 300, inflater=HostInflater))


def test_device_mode_raises_the_host_path_s_error_for_a_corrupt_block(tmp_path, unpinned):
    from cutseq_amd import textio
    from cutseq_amd.inflater import HostInflater
    text = b"".join(_records(1000, seed=3))
    data = bytearray(bgzf_rule.bgzf(text, 4093, 6))
    rows, _ = codec.bgzf_index(bytes(data), 0, len(data))
    data[rows[len(rows) // 2][0] + 40] ^= 0x10
    path = tmp_path / "bad.fq.gz"
    path.write_bytes(bytes(data))
    errors = []
    for kw in ({}, {"inflater": HostInflater}):
        with pytest.raises(OSError, match="corrupt gzip data") as err:
            _blocks(textio.TextReader(str(path), 300, **kw))
        errors.append(str(err.value))
    assert errors[0] == errors[1]

    class Suspicious(HostInflater):  # refuses a block libdeflate takes: the decoders disagree, an engine fault
        def inflate(self, mapped, lo, rows, buf, at):
            lines, _ = super().inflate(mapped, lo, rows, buf, at)
            return lines, 1

    good = tmp_path / "good.fq.gz"
    good.write_bytes(bgzf_rule.bgzf(text, 4093, 6))
    with pytest.raises(RuntimeError, match="disagrees with libdeflate"):
        _blocks(textio.TextReader(str(good), 300, inflater=Suspicious))


# ---------------------------------------------------------------- the switch


def test_switch_hygiene():
    entry = {s.name: s for s in switches.TABLE}["CUTSEQ_GPU_INFLATE"]
    assert entry.kind == switches.FLAG_OFF and entry.default is False and entry.reader == "python"
    assert "`CUTSEQ_GPU_INFLATE" in (ROOT / "INTEGRATION.md").read_text()
    assert abi.CS_ABI_VERSION == 7 and "#define CS_ABI_VERSION 7" in (ROOT / "include" / "cutseq_hip.h").read_text()
    from cutseq_amd import build
    assert {p.name for p in build.DEPS} >= {"inflate_kernels.hip.inc", "cutseq_inflate.h"}


def test_with_the_switch_off_nothing_new_is_loaded(monkeypatch):
    """The inflater module is imported by the device mode alone."""
    import subprocess, sys
    code = ("import sys; from cutseq_amd import textio, textpath, codec, run; "
            "sys.exit(1 if 'cutseq_amd.inflater' in sys.modules else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=str(ROOT)).returncode == 0
