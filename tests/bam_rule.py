"""Unaligned BAM for the BAM-input tests: a writer, a reader that renders FASTQ or refuses, the universe of small edge
inputs, one corrupt input per refusal, seeded mutations.  No GPU, no product code: plain loops over the bytes.

The format (SAM specification, section 4), all little-endian: a BGZF stream that inflates to ``BAM\\1``, l_text, text,
n_ref, n_ref x (l_name, name, l_ref), then records -- block_size and that many bytes: refID, pos, l_read_name (u8), mapq
(u8), bin (u16), n_cigar_op (u16), flag (u16), l_seq (u32), next_refID, next_pos, tlen, the NUL-terminated read name,
4 bytes per cigar op, two bases per byte (high nibble first, ``=ACMGRSVTWYHKDBN``), l_seq raw Phred values, tags.

The rule: a record becomes ``@name\\n<letters>\\n+\\n<qual + 33>\\n``; tags, cigar, mapq, bin and positions are not
read.  Refused, in this order for a record (the first that holds), each naming the 0-based record: block_size < 32; a
block the stream ends inside; fixed part + name + cigar + bases + qualities beyond block_size; an empty name or one
without its NUL; flag bit 0x4 not set (aligned); a line end inside the name; qual[0] == 0xFF with l_seq > 0; a quality
above 93.  Refused for the stream: a wrong magic, a negative header length, an end inside the header.
"""
import gzip
import random
import struct
from typing import List, NamedTuple, Sequence, Tuple

import bgzf_rule

LETTERS = b"=ACMGRSVTWYHKDBN"
MAGIC = b"BAM\x01"

# verdict codes (what tools/bam_walk_check.c prints): the records' are the device's CS_TEXT_ERR_BAM_* values
OK, BAD_MAGIC, BAD_HEADER_LENGTH, ENDS_IN_HEADER, ENDS_IN_RECORD = 0, 1, 2, 3, 4
BLOCK_SIZE, OVERRUN, NAME, ALIGNED, NAME_LINE_END, NO_QUAL, QUAL_RANGE = 16, 17, 18, 19, 20, 21, 22

MESSAGES = {
    BAD_MAGIC: "malformed BAM: the stream does not start with the magic 'BAM\\1'",
    BAD_HEADER_LENGTH: "malformed BAM: a negative length in the header",
    ENDS_IN_HEADER: "malformed BAM: the stream ends inside the header",
    ENDS_IN_RECORD: "malformed BAM: the stream ends inside record {n}",
    BLOCK_SIZE: "malformed BAM: record {n} has a block_size below 32",
    OVERRUN: "malformed BAM: name, cigar, bases and qualities of record {n} exceed its block_size",
    NAME: "malformed BAM: the read name of record {n} is empty or lacks its NUL",
    ALIGNED: "only unaligned BAM is supported: record {n} is aligned",
    NAME_LINE_END: "malformed BAM: a line end inside the read name of record {n}",
    NO_QUAL: "BAM record without qualities: record {n}",
    QUAL_RANGE: "malformed BAM: a quality above 93 in record {n}",
}


_CODE_OF = bytes(LETTERS.index(c) if c in LETTERS else 0xFF for c in range(256))  # (0xFF: no BAM letter; the writer fails)
_HIGH_LETTER = bytes(LETTERS[i >> 4] for i in range(256))
_LOW_LETTER = bytes(LETTERS[i & 15] for i in range(256))
_PLUS_33 = bytes((i + 33) & 0xFF for i in range(256))


class BamError(ValueError):
    def __init__(self, code: int, record: int = 0):
        super().__init__(MESSAGES[code].format(n=record))
        self.code, self.record = code, record


class Rec(NamedTuple):
    name: bytes              # without the NUL
    seq: bytes               # letters of LETTERS
    qual: bytes              # raw Phred values, len(seq) of them
    flag: int = 0x4 | 0x1 | 0x8  # unmapped (what samtools import writes sets 0x4; the other bits are not read)
    tags: bytes = b""
    cigar: Tuple[int, ...] = ()
    mapq: int = 0


def record_bytes(r: Rec, block_size=None, l_read_name=None, l_seq=None, nul=b"\0") -> bytes:
    """One record; the keyword arguments overwrite what the fields would say (corrupt inputs)."""
    codes = r.seq.translate(_CODE_OF) + b"\0"  # (an odd length: the last low nibble is 0)
    packed = bytes(hi << 4 | lo for hi, lo in zip(codes[0:len(r.seq):2], codes[1::2]))
    name = r.name + nul
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) if l_read_name is None else l_read_name, r.mapq, 4680,
                       len(r.cigar), r.flag, len(r.seq) if l_seq is None else l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", op) for op in r.cigar) + bytes(packed) + r.qual + r.tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header_bytes(text: bytes = b"", refs: Sequence[Tuple[bytes, int]] = ()) -> bytes:
    out = MAGIC + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def inflated(records: Sequence[Rec], header_text: bytes = b"", refs=()) -> bytes:
    return header_bytes(header_text, refs) + b"".join(record_bytes(r) for r in records)


def wrap(stream: bytes, block_bytes: int = 65280, level: int = 6, eof: bool = True) -> bytes:
    return bgzf_rule.bgzf(stream, block_bytes, level) + (bgzf_rule.EOF_MARKER if eof else b"")


def write_bam(records: Sequence[Rec], header_text: bytes = b"", refs=(), block_bytes: int = 65280, level: int = 6,
              eof: bool = True) -> bytes:
    return wrap(inflated(records, header_text, refs), block_bytes, level, eof)


def header_size(data: bytes) -> int:
    """Bytes of the header of the inflated stream ``data``, or the stream's refusal."""
    if data[:4] != MAGIC[:len(data[:4])]:
        raise BamError(BAD_MAGIC)
    at = 4
    if len(data) < at + 4:
        raise BamError(ENDS_IN_HEADER)
    l_text, = struct.unpack_from("<i", data, at)
    if l_text < 0:
        raise BamError(BAD_HEADER_LENGTH)
    at += 4 + l_text
    if len(data) < at + 4:
        raise BamError(ENDS_IN_HEADER)
    n_ref, = struct.unpack_from("<i", data, at)
    if n_ref < 0:
        raise BamError(BAD_HEADER_LENGTH)
    at += 4
    for _ in range(n_ref):
        if len(data) < at + 4:
            raise BamError(ENDS_IN_HEADER)
        l_name, = struct.unpack_from("<i", data, at)
        if l_name < 0:
            raise BamError(BAD_HEADER_LENGTH)
        at += 4 + l_name + 4
        if len(data) < at:
            raise BamError(ENDS_IN_HEADER)
    return at


def fastq_of_record(rec: bytes, index: int) -> bytes:
    """``rec``: block_size and the block, complete.  -> the FASTQ record, or the record's refusal."""
    block_size, = struct.unpack_from("<i", rec, 0)
    l_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<BBHHHI", rec, 12)
    if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > block_size:
        raise BamError(OVERRUN, index)
    name = rec[36:36 + l_name]
    if l_name == 0 or name[-1] != 0:
        raise BamError(NAME, index)
    if not flag & 0x4:
        raise BamError(ALIGNED, index)
    if b"\n" in name[:-1] or b"\r" in name[:-1]:
        raise BamError(NAME_LINE_END, index)
    seq_at = 36 + l_name + 4 * n_cigar
    qual = rec[seq_at + (l_seq + 1) // 2:seq_at + (l_seq + 1) // 2 + l_seq]
    if l_seq and qual[0] == 0xFF:
        raise BamError(NO_QUAL, index)
    if l_seq and max(qual) > 93:
        raise BamError(QUAL_RANGE, index)
    packed = rec[seq_at:seq_at + (l_seq + 1) // 2]
    letters = bytearray(2 * len(packed))
    letters[0::2] = packed.translate(_HIGH_LETTER)  # byte i of the table: the letter of i's high nibble
    letters[1::2] = packed.translate(_LOW_LETTER)
    return b"@" + name[:-1] + b"\n" + bytes(letters[:l_seq]) + b"\n+\n" + qual.translate(_PLUS_33) + b"\n"


def read_records(data: bytes):
    """The inflated stream ``data`` -> [(start, end)] of its records, then per record the text; the first refusal in
    record order is raised.  A generator of (start, end, fastq)."""
    at, index = header_size(data), 0
    while at < len(data):
        if len(data) < at + 4:
            raise BamError(ENDS_IN_RECORD, index)
        block_size, = struct.unpack_from("<i", data, at)
        if block_size < 32:
            raise BamError(BLOCK_SIZE, index)
        if len(data) < at + 4 + block_size:
            raise BamError(ENDS_IN_RECORD, index)
        yield at, at + 4 + block_size, fastq_of_record(data[at:at + 4 + block_size], index)
        at += 4 + block_size
        index += 1


def read_inflated(data: bytes) -> bytes:
    return b"".join(text for _, _, text in read_records(data))


def read_bam(data: bytes) -> bytes:
    """A BAM file's bytes -> its reads as FASTQ text, or BamError.  (The BGZF EOF marker is not required.)"""
    return read_inflated(gzip.decompress(data))


def split(data: bytes):
    """A good BAM file -> (record bytes back to back, offsets of n + 1 entries, [fastq per record])."""
    stream = gzip.decompress(data)
    rows = list(read_records(stream))
    base = rows[0][0] if rows else len(stream)
    return stream[base:], [s - base for s, _, _ in rows] + [len(stream) - base], [t for _, _, t in rows]


# ---- the universe ----------------------------------------------------------------------------------------------------

L_SEQS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 150)
NAME_LENGTHS = (1, 2, 31, 32, 33, 254, 0)  # (0: the empty name, l_read_name == 1)
HEADER_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\n"
REFS = ((b"chr1", 248956422), (b"chrM", 16569))
TAGS = (b"", b"RGZa\0", b"RXZACGT\0NMC\x03XYi\x10\x27\0\0")
BLOCK_BYTES = (37, 64, 4096, 65280)
COUNTS = (1, 255, 256, 257, 600)


def _name(rng: random.Random, n: int, k: int) -> bytes:
    stem = b"r%d" % k
    if n <= len(stem):
        return (b"%d" % (k % 10)) * n
    return stem + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz:_#0123456789") for _ in range(n - len(stem)))


def edge_records(seed: int = 11) -> List[Rec]:
    rng = random.Random(seed)
    out = []
    for k, l_seq in enumerate(L_SEQS):
        seq = bytes(rng.choice(b"ACGTN") for _ in range(l_seq))
        qual = bytes(rng.choice((0, 93, 2, 40, rng.randrange(94))) for _ in range(l_seq))
        out.append(Rec(_name(rng, NAME_LENGTHS[k % len(NAME_LENGTHS)], k), seq, qual, tags=TAGS[k % 3],
                       cigar=(() if k % 4 else (l_seq << 4 | 4, 16))))
    for k, n in enumerate(NAME_LENGTHS):  # every name length on a read that has bases
        out.append(Rec(_name(rng, n, 100 + k), b"ACGTACGTAC", bytes(range(10)), tags=TAGS[(k + 1) % 3]))
    # every nibble code at both nibble positions; qualities 0 and 93 at both ends
    out.append(Rec(b"codes_even", LETTERS, b"\0" + bytes([93]) * 14 + b"\0"))
    out.append(Rec(b"codes_odd", b"A" + LETTERS, bytes([93]) + b"\0" * 15 + bytes([93]), flag=0x4 | 0x40))
    return out


def random_records(n: int, seed: int, lo: int = 20, hi: int = 160) -> List[Rec]:
    rng = random.Random(seed)
    out = []
    for k in range(n):
        l_seq = rng.randrange(lo, hi)
        out.append(Rec(b"read%d:%d" % (seed, k), bytes(rng.choice(b"ACGT") for _ in range(l_seq)),
                       bytes(rng.randrange(2, 42) for _ in range(l_seq)), tags=TAGS[k % 3] if k % 5 == 0 else b""))
    return out


def mate_of(records: Sequence[Rec], seed: int = 5) -> List[Rec]:
    """Mate 2 of every record: the same name, bases and qualities of its own."""
    rng = random.Random(seed)
    out = []
    for r in records:
        l_seq = max(0, len(r.seq) + rng.randrange(-3, 4)) if r.seq else 0
        out.append(Rec(r.name, bytes(rng.choice(b"ACGTN") for _ in range(l_seq)), bytes(rng.randrange(94) for _ in range(l_seq)),
                       flag=0x4 | 0x80, tags=r.tags))
    return out


def universe() -> List[tuple]:
    """[(label, records, write_bam keyword arguments)]"""
    out = []
    for block_bytes in BLOCK_BYTES:
        out.append((f"edges/{block_bytes}", edge_records(), dict(block_bytes=block_bytes, header_text=HEADER_TEXT if block_bytes != 64 else b"",
                                                                refs=REFS if block_bytes != 64 else ())))
    for n in COUNTS:
        out.append((f"count/{n}", random_records(n, seed=n), dict(block_bytes=4096 if n == 600 else 65280, eof=n != 255)))
    return out


# ---- corrupt inputs: one per refusal ---------------------------------------------------------------------------------

class Corrupt(NamedTuple):
    label: str
    stream: bytes   # inflated
    code: int
    record: int
    where: str      # "stream": the host finds it walking the chain; "record": the device checks the record


def corrupt() -> List[Corrupt]:
    good = random_records(5, seed=77, lo=30, hi=40)
    head = header_bytes(HEADER_TEXT, REFS)

    def at(k: int, bad: bytes) -> bytes:
        return head + b"".join(bad if i == k else record_bytes(r) for i, r in enumerate(good))

    r = good[2]
    whole = at(-1, b"")
    out = [
        Corrupt("block_size 31", at(2, struct.pack("<i", 31) + record_bytes(r)[4:]), BLOCK_SIZE, 2, "stream"),
        Corrupt("negative block_size", at(1, struct.pack("<i", -5) + record_bytes(r)[4:]), BLOCK_SIZE, 1, "stream"),
        Corrupt("l_seq beyond the block", at(2, record_bytes(r, l_seq=len(r.seq) + 40)), OVERRUN, 2, "record"),
        Corrupt("l_seq 2^32 - 1", at(0, record_bytes(r, l_seq=0xFFFFFFFF)), OVERRUN, 0, "record"),
        Corrupt("l_read_name 0", at(3, record_bytes(Rec(b"", r.seq, r.qual), l_read_name=0, nul=b"")), NAME, 3, "record"),
        Corrupt("no NUL", at(2, record_bytes(r, nul=b"x")), NAME, 2, "record"),
        Corrupt("aligned", at(4, record_bytes(r._replace(flag=0x10))), ALIGNED, 4, "record"),
        Corrupt("newline in name", at(2, record_bytes(r._replace(name=b"a\nb"))), NAME_LINE_END, 2, "record"),
        Corrupt("carriage return in name", at(1, record_bytes(r._replace(name=b"ab\r"))), NAME_LINE_END, 1, "record"),
        Corrupt("no qualities", at(2, record_bytes(r._replace(qual=b"\xff" * len(r.qual)))), NO_QUAL, 2, "record"),
        Corrupt("quality 94", at(2, record_bytes(r._replace(qual=r.qual[:-1] + bytes([94])))), QUAL_RANGE, 2, "record"),
        Corrupt("quality 255 inside", at(0, record_bytes(r._replace(qual=r.qual[:7] + b"\xff" + r.qual[8:]))), QUAL_RANGE, 0, "record"),
        Corrupt("ends inside a record", whole[:-9], ENDS_IN_RECORD, 4, "stream"),
        Corrupt("ends inside a block_size", whole + b"\x40\0", ENDS_IN_RECORD, 5, "stream"),
        Corrupt("ends inside the header", head[:-3], ENDS_IN_HEADER, 0, "stream"),
        Corrupt("negative l_text", MAGIC + struct.pack("<i", -1) + whole[8:], BAD_HEADER_LENGTH, 0, "stream"),
        Corrupt("wrong magic", b"BAM\x02" + whole[4:], BAD_MAGIC, 0, "stream"),
    ]
    for c in out:  # the rule agrees with the list
        try:
            read_inflated(c.stream)
            raise AssertionError(c.label)
        except BamError as exc:
            assert (exc.code, exc.record) == (c.code, c.record), (c.label, exc.code, exc.record)
    return out


def mutations(n: int = 2000, seed: int = 4242) -> List[bytes]:
    """Seeded byte mutations of the universe's (inflated) streams: what the rule says about each is the expectation."""
    rng = random.Random(seed)
    streams = [inflated(records, kw.get("header_text", b""), kw.get("refs", ())) for label, records, kw in universe()
               if label.startswith("edges") or label in ("count/1", "count/255")]
    out = []
    for _ in range(n):
        s = bytearray(rng.choice(streams))
        if len(s) > 20000:
            lo = rng.randrange(len(s) - 20000)
            s = bytearray(header_bytes() + bytes(s[lo:lo + 4000]))  # (a window: mostly an early bad block_size)
        for _ in range(rng.choice((1, 1, 2, 4))):
            i = rng.randrange(len(s))
            kind = rng.randrange(4)
            if kind == 0:
                s[i] = rng.randrange(256)
            elif kind == 1:
                s[i] ^= 1 << rng.randrange(8)
            elif kind == 2:
                s[i] = rng.choice((0, 0xFF, 0x0A, 0x0D, 94, 93))
            else:
                del s[i:i + rng.randrange(1, 9)]
        out.append(bytes(s))
    return out


def verdict(stream: bytes):
    """-> (code, record, text | b"") of an inflated stream by the rule."""
    try:
        return OK, 0, read_inflated(stream)
    except BamError as exc:
        return exc.code, exc.record, b""


def write_case_file(path, streams: Sequence[bytes]) -> None:
    """What tools/bam_walk_check.c reads: "CSBC", count, then per case the stream's size, the expected verdict code,
    record and text size, the stream and the text."""
    with open(path, "wb") as fh:
        fh.write(b"CSBC" + struct.pack("<I", len(streams)))
        for s in streams:
            code, record, text = verdict(s)
            fh.write(struct.pack("<IIII", len(s), code, record, len(text)) + s + text)
