"""BGZF as the tool writes it (``--bgzf``, ``cs_text_params.compress = 2``) as plain rules.  No GPU, no product code:
``gzip_rule`` (the strict parser, the matcher, the sizes), ``bgzf_rule`` (the EOF marker) and ``zlib`` only.
tests/test_bgzf_out_cpu.py holds this file to zlib and the host writer to this file, tests/test_gpu_bgzf_out.py the
device.

A file is a series of blocks and ends with the 28-byte EOF marker.  A block is a gzip member of its own:

    18 bytes   1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00, then BSIZE: the block's size less one, 16 bits
    the data   the device: one 32 768-byte chunk of the stream as deflate_chunks stages it -- a dynamic block and an
               empty stored block, both non-final, or a non-final stored block -- and 03 00, the final empty fixed block
    8 bytes    CRC-32 and length of the block's OWN text

``split_blocks``  walks a file by BSIZE; every header must be those 18 bytes.
``check_block``   one block of the device against the chunk of text it holds: nothing in front of the chunk counts, so
                  its tokens are those of a stream that consists of the chunk alone.
``check_file``    a whole file against its text.
"""
import zlib
from typing import List

import bgzf_rule
import gzip_rule

CHUNK = gzip_rule.CHUNK
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")  # BSIZE follows
EOF_MARKER = bgzf_rule.EOF_MARKER
MAX_BLOCK = 18 + CHUNK + 5 + 10  # a stored chunk: the device's largest block
assert MAX_BLOCK == 32801 and EOF_MARKER[:16] == HEADER and len(EOF_MARKER) == 28


class BgzfError(ValueError):
    """What ``split_blocks`` refuses; the message names the byte offset."""


def split_blocks(data: bytes) -> List[bytes]:
    """The blocks of ``data``, the EOF marker (if there) among them.  Raises BgzfError where a block does not start with
    the 18 header bytes exactly, is smaller than an empty block can be, or does not lie inside ``data`` whole --
    trailing bytes are such a block."""
    data = bytes(data)
    blocks, pos = [], 0
    while pos < len(data):
        if len(data) - pos < 18:
            raise BgzfError(f"byte {pos}: {len(data) - pos} trailing bytes are no block header")
        if data[pos:pos + 16] != HEADER:
            raise BgzfError(f"byte {pos}: not the BGZF header: {data[pos:pos + 16].hex()}")
        size = int.from_bytes(data[pos + 16:pos + 18], "little") + 1
        if size < 28:
            raise BgzfError(f"byte {pos}: BSIZE names {size} bytes, an empty block has 28")
        if pos + size > len(data):
            raise BgzfError(f"byte {pos}: a block of {size} bytes, the data ends at byte {len(data)}")
        blocks.append(data[pos:pos + size])
        pos += size
    return blocks


def chunks_of(text: bytes) -> List[bytes]:
    return [text[lo:lo + CHUNK] for lo in range(0, len(text), CHUNK)]


def check_block(block: bytes, chunk_text: bytes, fasta: bool = False, lz: bool = True, what=""):
    """One block of the device holding ``chunk_text`` -> (its gzip_rule.Member, True if the chunk is dynamic)."""
    assert 0 < len(chunk_text) <= CHUNK, (what, len(chunk_text))
    assert block[:16] == HEADER and int.from_bytes(block[16:18], "little") == len(block) - 1, what
    assert len(block) <= MAX_BLOCK, (what, len(block))
    member = gzip_rule.parse_member(block)  # (strict: blocks, codes, the trailer's CRC-32 and ISIZE, nothing behind it)
    assert member.header_len == 18, (what, member.header_len)
    assert member.text == chunk_text, what
    assert member.crc == zlib.crc32(chunk_text) and member.isize == len(chunk_text), what
    blocks = member.blocks
    data = blocks[0]
    assert data.start_bit == 18 * 8 and not data.final and data.raw_len == len(chunk_text), (what, data)
    if data.btype == 2:
        assert len(blocks) == 3, (what, blocks)
        empty = blocks[1]
        assert empty.btype == 0 and not empty.final and empty.raw_len == 0, (what, empty)
        end = empty.end_bit
    else:
        assert data.btype == 0 and len(blocks) == 2, (what, blocks)
        end = data.end_bit
    last = blocks[-1]
    assert last.btype == 1 and last.final and last.raw_len == 0 and last.start_bit == end and end % 8 == 0, (what, last)
    assert block[end // 8:end // 8 + 2] == b"\x03\x00" and len(block) == end // 8 + 10, what
    n_bytes = end // 8 - 18
    # the tokens: the rule at stream offset 0 of a stream that is this chunk -- no run reaches in front of the chunk,
    # the chunk starts a line, a marker at its first byte starts a record
    want = gzip_rule.tokens(chunk_text, 0, fasta, lz)
    size = gzip_rule.dynamic_chunk_bytes(want)
    if data.btype == 2:
        if data.tokens != want:
            k = next((i for i, (a, b) in enumerate(zip(data.tokens, want)) if a != b), min(len(want), len(data.tokens)))
            raise AssertionError(f"{what}: token {k}: the block has {data.tokens[k:k + 3]}, the rule {want[k:k + 3]}")
        assert n_bytes == size < len(chunk_text) + 5 and n_bytes <= gzip_rule.MAX_DYNAMIC, (what, n_bytes, size)
    else:  # stored for a reason: the dynamic form would be no smaller, or would not fit the bit buffer
        assert n_bytes == len(chunk_text) + 5, (what, n_bytes)
        assert size >= len(chunk_text) + 5 or size > gzip_rule.MAX_DYNAMIC, (what, size)
    return member, data.btype == 2


def check_stream(data: bytes, text: bytes, fasta: bool = False, lz: bool = True, what=""):
    """A route's bytes as the device delivers them (no EOF marker): one block per chunk of ``text``, in order -> the
    (Member, dynamic) of every block."""
    blocks = split_blocks(data)
    chunks = chunks_of(text)
    assert len(blocks) == len(chunks), (what, len(blocks), len(chunks))
    return [check_block(b, c, fasta, lz, (what, i)) for i, (b, c) in enumerate(zip(blocks, chunks))]


def check_file(data: bytes, text: bytes, fasta: bool = False, lz: bool = True, parts=None, what=""):
    """A file of the device's blocks: the chunks of ``text`` in order, then the EOF marker.  ``parts``: the text lengths
    of the pieces the file was put together from (batches, ranks), each chunked on its own; an empty block (the marker's
    bytes) may sit between two pieces.  -> the blocks without the empty ones."""
    blocks = split_blocks(data)
    assert blocks and blocks[-1] == EOF_MARKER, (what, "the file does not end with the EOF marker")
    assert data[-28:] == EOF_MARKER
    pieces, at = [], 0
    for n in (parts if parts is not None else [len(text)]):
        pieces.append(text[at:at + n])
        at += n
    assert at == len(text), (what, at, len(text))
    want = [c for piece in pieces for c in chunks_of(piece)]
    full = [b for b in blocks[:-1] if b != EOF_MARKER]
    if parts is None:
        assert len(full) == len(blocks) - 1, (what, "an empty block inside a file of one piece")
    assert len(full) == len(want), (what, len(full), len(want))
    for i, (b, c) in enumerate(zip(full, want)):
        check_block(b, c, fasta, lz, (what, i))
    return full
