"""--bgzf on the CPU side: the rule file (tests/bgzf_out_rule.py) against bgzf_rule's writer and zlib, the host form
(codec.bgzf_blocks), the writer's EOF marker, the text options, the command line and its refusals, the C header."""
import dataclasses
import gzip
import random
import re
import struct
import zlib
from pathlib import Path

import pytest

from cutseq_amd import codec, plan as planmod, run, textio
from cutseq_amd.common import BUILDIN_ADAPTERS

import bgzf_out_rule
import bgzf_rule
import gzip_rule

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])
EOF = bgzf_rule.EOF_MARKER


# ---- the rule file ---------------------------------------------------------------------------------------------

def test_split_blocks_walks_what_bgzf_rule_writes():
    text = bgzf_rule.fastq_text(150000)
    data = bgzf_rule.bgzf(text, 65280, 1) + EOF
    blocks = bgzf_out_rule.split_blocks(data)
    assert len(blocks) == 3 + 1 and blocks[-1] == EOF and b"".join(blocks) == data
    assert b"".join(gzip.decompress(b) for b in blocks) == text == gzip.decompress(data)
    assert bgzf_out_rule.split_blocks(b"") == [] and bgzf_out_rule.split_blocks(EOF) == [EOF]


@pytest.mark.parametrize("damage, message", [
    (lambda d: d + b"\0", "trailing bytes"),
    (lambda d: d[:-1], "the data ends at byte"),
    (lambda d: d[:3] + b"\x00" + d[4:], "not the BGZF header"),               # no FEXTRA
    (lambda d: d[:9] + b"\x03" + d[10:], "not the BGZF header"),              # another OS byte
    (lambda d: d[:16] + struct.pack("<H", 26) + d[18:], "an empty block has 28"),
    (lambda d: gzip.compress(b"x") + d, "not the BGZF header"),               # an ordinary member in front
])
def test_split_blocks_refuses(damage, message):
    data = bgzf_rule.bgzf(b"ACGT\n" * 100, 65280, 1) + EOF
    with pytest.raises(bgzf_out_rule.BgzfError, match=message):
        bgzf_out_rule.split_blocks(damage(data))
    # an extra subfield in front of BC is BGZF, but not this writer's header
    other = bgzf_rule.member(bgzf_rule.deflate_raw(b"x"), zlib.crc32(b"x"), 1, extra_first=b"XY\x01\x00\x07")
    with pytest.raises(bgzf_out_rule.BgzfError, match="not the BGZF header"):
        bgzf_out_rule.split_blocks(other)


def _device_like_block(chunk: bytes, stored: bool, reach_back: bool = False) -> bytes:
    """A block laid out as the device lays one out, made with zlib: a non-final block of the chunk behind a sync flush
    (which IS the empty non-final stored block), then 03 00.  ``stored``: level 0.  Its tokens are zlib's, not the
    rule's: check_block must accept the layout and refuse the tokens."""
    c = zlib.compressobj(0 if stored else 1, zlib.DEFLATED, -15)
    body = c.compress(chunk) + c.flush(zlib.Z_SYNC_FLUSH)
    if stored:
        body = body[:-5]  # (level 0: the stored block itself is non-final already; drop the flush's empty one)
    payload = body + b"\x03\x00"
    return bgzf_rule.member(payload, zlib.crc32(chunk), len(chunk))


def test_check_block_on_layouts_made_with_zlib():
    rng = random.Random(5)
    noise = rng.randbytes(3000)
    block = _device_like_block(noise, stored=True)
    assert gzip.decompress(block) == noise
    member, dynamic = bgzf_out_rule.check_block(block, noise)  # incompressible: stored for the reason the rule accepts
    assert not dynamic and [b.btype for b in member.blocks] == [0, 1]
    text = bgzf_rule.fastq_text(3000)
    with pytest.raises(AssertionError):  # text that shrinks has no reason to be stored
        bgzf_out_rule.check_block(_device_like_block(text, stored=True), text)
    block = _device_like_block(text, stored=False)
    assert gzip.decompress(block) == text
    with pytest.raises(AssertionError):  # zlib's matches (or its fixed block) are not the rule's tokens
        bgzf_out_rule.check_block(block, text)
    with pytest.raises(AssertionError):  # the text is the chunk's own
        bgzf_out_rule.check_block(_device_like_block(noise, stored=True), noise[:-1] + b"x")
    with pytest.raises(gzip_rule.GzipError):  # the CRC is the chunk's own
        bad = bytearray(_device_like_block(noise, stored=True))
        bad[-8] ^= 1
        bgzf_out_rule.check_block(bytes(bad), noise)
    # the largest block: a stored chunk of CHUNK bytes
    full = rng.randbytes(bgzf_out_rule.CHUNK)
    block = _device_like_block(full, stored=True)
    assert len(block) == bgzf_out_rule.MAX_BLOCK == 32801
    bgzf_out_rule.check_block(block, full)


def test_the_rule_of_a_block_is_the_rule_at_stream_offset_0():
    """What the issue fixes: nothing in front of a chunk counts.  A run that straddles the chunk boundary starts chunk 1
    with a match of distance 1 in the gzip form and with a literal in the BGZF form."""
    text = b"@r\n" + b"A" * (bgzf_out_rule.CHUNK - 20 - 3) + b"I" * 40 + b"\n"
    at = bgzf_out_rule.CHUNK
    assert text[at - 20:at + 20] == b"I" * 40
    assert gzip_rule.tokens(text, 1, False)[0] == ("match", 20, 1)
    alone = gzip_rule.tokens(text[at:], 0, False)
    assert alone[:2] == [("lit", ord("I")), ("match", 19, 1)]
    # '@' at the chunk's first byte: a record start at offset 0 of its own stream, whatever stood in front of it
    text = b"@r\nAC\n+\n" + b"I" * (at - 8) + b"@@@@\n"
    assert text[at] == ord("@") and text[at - 1] != 10
    assert gzip_rule.expand(gzip_rule.tokens(text[at:], 0, False)) == text[at:]


def test_check_file_counts_blocks_and_wants_the_marker():
    rng = random.Random(6)
    text = rng.randbytes(2 * bgzf_out_rule.CHUNK + 10)
    blocks = [_device_like_block(c, stored=True) for c in bgzf_out_rule.chunks_of(text)]
    data = b"".join(blocks) + EOF
    assert bgzf_out_rule.check_file(data, text) == blocks
    assert bgzf_out_rule.check_file(EOF, b"") == []
    with pytest.raises(AssertionError):
        bgzf_out_rule.check_file(b"".join(blocks), text)  # no marker
    with pytest.raises(AssertionError):
        bgzf_out_rule.check_file(b"".join(blocks[:2]) + EOF, text)  # a chunk is missing
    with pytest.raises(AssertionError):
        bgzf_out_rule.check_file(blocks[0] + EOF + b"".join(blocks[1:]) + EOF, text)  # an empty block inside one piece
    # two parts (ranks), each chunked on its own, an empty block between them
    a, b = text[:40000], text[40000:]
    parts = [_device_like_block(c, stored=True) for piece in (a, b) for c in bgzf_out_rule.chunks_of(piece)]
    joined = b"".join(parts[:2]) + EOF + b"".join(parts[2:]) + EOF
    assert len(parts) == 3 and len(bgzf_out_rule.check_file(joined, text, parts=[len(a), len(b)])) == 3
    with pytest.raises(AssertionError):  # (the file's own chunking is another: 32768 + 32768 + 10)
        bgzf_out_rule.check_file(joined, text)
    assert gzip.decompress(joined) == text


# ---- the host form ---------------------------------------------------------------------------------------------

INPUTS = {
    "empty": b"",
    "one byte": b"A",
    "65280": bgzf_rule.fastq_text(65280),
    "65281": bgzf_rule.fastq_text(65281),
    "200 KB of FASTQ": bgzf_rule.fastq_text(200000),
    "70000 random bytes": random.Random(70000).randbytes(70000),
}


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_bgzf_blocks(name):
    data = INPUTS[name]
    out = codec.bgzf_blocks(data)
    blocks = bgzf_out_rule.split_blocks(out)
    assert len(blocks) == (len(data) + 65279) // 65280
    assert all(len(b) <= 65536 for b in blocks)
    rows, end = codec.bgzf_index(out, 0, len(out))
    assert end == len(out) and len(rows) == len(blocks)
    texts = [gzip.decompress(b) for b in blocks]
    assert all(0 < len(t) <= 65280 for t in texts) and b"".join(texts) == data
    for (payload, nbytes, isize, crc), b, t in zip(rows, blocks, texts):
        assert out[payload:payload + nbytes] == b[18:-8] and isize == len(t) and crc == zlib.crc32(t)
        assert zlib.decompressobj(-15).decompress(b[18:-8]) == t
        gzip_rule.parse_member(b)  # (strict: complete codes, nothing behind the trailer)
    assert gzip.decompress(out + EOF) == data
    assert codec.bgzf_blocks(memoryview(bytearray(data))) == out and codec.bgzf_blocks(data, 1) == out
    if name == "70000 random bytes":  # incompressible: the first block is stored, 65280 + 5 + 26 bytes
        assert len(blocks[0]) == 65280 + 5 + 26 and blocks[0][18] == 1


def test_the_marker_is_htslibs():
    assert codec.BGZF_EOF == EOF and len(codec.BGZF_EOF) == 28
    assert codec.BGZF_HEADER == bgzf_out_rule.HEADER
    assert gzip.decompress(codec.BGZF_EOF) == b""


# ---- the writer ------------------------------------------------------------------------------------------------

class _Shared:
    def __init__(self):
        self.n = 0

    def done(self):
        self.n += 1


def test_stream_writer_host_branch_ends_in_exactly_one_marker(tmp_path):
    pieces = [bgzf_rule.fastq_text(n, seed=n) for n in (1000, 70000, 1, 130561)]
    path = tmp_path / "out.fastq.gz"
    w = textio.StreamWriter(str(path), bgzf=True)
    shared = _Shared()
    for p in pieces:
        w.put(memoryview(p), shared)
    w.close()
    assert shared.n == len(pieces)
    data = path.read_bytes()
    blocks = bgzf_out_rule.split_blocks(data)
    assert blocks[-1] == EOF and sum(1 for b in blocks if b == EOF) == 1 and data.count(EOF) == 1
    assert len(blocks) == 1 + sum((len(p) + 65279) // 65280 for p in pieces)
    assert gzip.decompress(data) == b"".join(pieces)
    rows, end = codec.bgzf_index(data, 0, len(data))
    assert end == len(data) and rows[-1][2] == 0


def test_stream_writer_without_a_put_is_the_marker_alone(tmp_path):
    for kw in (dict(), dict(precompressed=True)):
        path = tmp_path / "empty.fq.gz"
        textio.StreamWriter(str(path), bgzf=True, **kw).close()
        assert path.read_bytes() == EOF


def test_stream_writer_precompressed_branch_passes_blocks_through_and_closes_once(tmp_path):
    text = bgzf_rule.fastq_text(100000)
    device = bgzf_rule.bgzf(text, 32768, 1)  # (any blocks: the branch does not look into them)
    path = tmp_path / "pre.fq.gz"
    w = textio.StreamWriter(str(path), precompressed=True, bgzf=True)
    shared = _Shared()
    w.put(memoryview(device[:50000]), shared)
    w.put(memoryview(device[50000:]), shared)
    w.close()
    assert path.read_bytes() == device + EOF


def test_other_writers_are_untouched(tmp_path):
    """bgzf acts on gzip files only; without it a gzip file is what it was."""
    text = bgzf_rule.fastq_text(5000)
    for name, flag, check in (("a.fq", True, lambda d: d == text),
                              ("b.fq.gz", False, lambda d: d[:4] == b"\x1f\x8b\x08\x00" and gzip.decompress(d) == text),
                              ("c.fq.gz", True, lambda d: d[-28:] == EOF and gzip.decompress(d) == text)):
        path = tmp_path / name
        w = textio.StreamWriter(str(path), bgzf=flag)
        w.put(memoryview(text), _Shared())
        w.close()
        assert check(path.read_bytes()), name
    path = tmp_path / "none.fq.gz"
    textio.StreamWriter(str(path)).close()
    assert path.read_bytes()[:4] == b"\x1f\x8b\x08\x00" and gzip.decompress(path.read_bytes()) == b""
    path = tmp_path / "d.fq.bz2"
    textio.StreamWriter(str(path), bgzf=True).close()
    assert not path.read_bytes().endswith(EOF)


# ---- the command line ------------------------------------------------------------------------------------------

def _args(*extra, inputs=("in_R1.fq.gz", "in_R2.fq.gz")):
    return run.build_parser().parse_args([*inputs, "-A", "TAKARAV3", "--bgzf", *extra])


def _options(args, gpu_deflate=True, fasta=False):
    tp = run.compile_plan(args, TAKARA, run.settings_from_args(args))
    return textio.text_options(args.outputs, tp, fasta, gpu_deflate)


def test_the_option_reaches_the_layout_and_the_engines():
    args = run.resolve_args(_args())
    assert args.bgzf and args.outputs.bgzf
    assert _options(args).compress == 2
    assert _options(args, gpu_deflate=False).compress is False
    # one plain output: the host compresses the others, as blocks
    args = run.resolve_args(_args("-s", "s1.fq", "s2.fq"))
    assert args.outputs.bgzf and not _options(args).compress
    # the info table: the device's when the records are, the host's when they are not -- never a plain member
    args = run.resolve_args(_args("--info-file", "t.tsv.gz"))
    opt = _options(args)
    assert opt.compress == 2 and opt.info & 2
    args = run.resolve_args(_args("--info-file", "t.tsv.gz", "-o", "o1.fq", "o2.fq"))
    opt = _options(args)
    assert not opt.compress and opt.info & 1 and not opt.info & 2
    # barcodes' files and --too-long-output are outputs like the others
    args = run.resolve_args(_args("-M", "100", "--too-long-output", "l1.fq.gz", "l2.fq.gz"))
    assert _options(args).compress == 2
    # a rank's layout keeps the flag
    groups = args.outputs.rank_groups()
    assert args.outputs.with_rank_names(groups).bgzf


def test_without_the_option_nothing_changes():
    argv = ["-A", "TAKARAV3", "in_R1.fq.gz", "in_R2.fq.gz", "--info-file", "t.tsv.gz"]
    args = run.resolve_args(run.build_parser().parse_args(argv))
    assert args.bgzf is False and args.outputs.bgzf is False
    opt = _options(args)
    assert opt.compress is True and opt.info & 2
    assert set(dataclasses.asdict(opt)) == {"compress", "bins", "fasta_routes", "info", "too_long_route", "interleave_in",
                                            "interleave_out", "mate2_first"}
    args = run.resolve_args(run.build_parser().parse_args(argv + ["-o", "o1.fq", "o2.fq"]))
    opt = _options(args)
    assert opt.compress is False and opt.info & 2  # (the parent's: a .gz table beside plain records is the device's)


def test_text_engine_passes_the_value_through():
    import inspect
    from cutseq_amd import textpath
    src = inspect.getsource(textpath.TextEngine.__init__)
    assert "p.compress = 2 if compress == 2 else (1 if compress else 0)" in src
    assert (True == 2) is False  # noqa: E712 -- (``True`` stays 1)


def test_no_gzip_output_is_refused(caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args("-o", "o1.fq", "o2.fq", "-s", "s1.fq", "s2.fq.zst"))
    assert exc.value.code == 1 and "--bgzf: no output of this run is a gzip file" in caplog.text
    caplog.clear()
    with pytest.raises(SystemExit):  # standard output is not a gzip file
        run.resolve_args(_args("--interleaved", "-o", "-", "-s", "s.fq", inputs=("in.fq",)))
    assert "no output of this run is a gzip file" in caplog.text
    # one is enough, and the info table counts
    assert run.resolve_args(_args("-o", "o1.fq", "o2.fq", "-s", "s1.fq", "s2.fq", "--info-file", "t.tsv.gz")).outputs.bgzf
    assert run.resolve_args(_args("-o", "o1.fq", "o2.fq")).outputs.bgzf  # (the -O default of -s is a .gz name)


def test_the_record_path_is_refused(monkeypatch, caplog):
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args())
    assert exc.value.code == 1 and "--bgzf needs the text path" in caplog.text


def test_fastq_writers_never_see_a_bgzf_run(monkeypatch, caplog):
    """The one configuration in which fastq.py's own writers would write a .gz output is the record path: a layout with
    the flag that reaches ``run_pipeline`` there is refused before a device or a file is opened."""
    args = run.resolve_args(_args())
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    from cutseq_amd import capi, fastq
    monkeypatch.setattr(capi, "device_count", lambda: pytest.fail("a device was asked for"))
    monkeypatch.setattr(fastq, "OutputFile", lambda *a, **k: pytest.fail("fastq.py's writer was opened"))
    with pytest.raises(SystemExit) as exc:
        run.run_pipeline(args, None)
    assert exc.value.code == 1 and "write plain gzip members, not BGZF" in caplog.text


def test_help_and_documents_name_the_option():
    text = run.build_parser().format_help()
    assert "--bgzf" in text and "BGZF" in text
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"2: BGZF", header) and "EOF marker" in header
    assert "compress = 2" in (ROOT / "INTEGRATION.md").read_text()
    assert "--bgzf" in (ROOT / "README.md").read_text()
