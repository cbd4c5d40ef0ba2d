"""BGZF for the inflate tests: a writer, the universe of well-formed blocks, the fixed list of corrupt ones, seeded
mutations, and what zlib says about each (the expected verdict).  No GPU, no product code.

A *case* is what one entry of the device's block table describes: the deflate payload of one block, the text length
the trailer promises (``out_len``, ISIZE) and its CRC-32.  Expected: ``zlib.decompressobj(-15)`` takes the payload
without an error, ends its stream, uses all input, and length and ``zlib.crc32`` equal the trailer's -- accepted, with
that text -- or the case is refused.  Which verdict code refuses it is not compared.
"""
import random
import struct
import zlib
from typing import List, NamedTuple, Optional

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Case(NamedTuple):
    name: str
    payload: bytes
    out_len: int
    crc: int


def deflate_raw(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_every: Optional[int] = None,
                flush_mode: int = zlib.Z_SYNC_FLUSH) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_every is None:
        return c.compress(data) + c.flush()
    out = b""
    for lo in range(0, len(data), flush_every):
        out += c.compress(data[lo:lo + flush_every]) + c.flush(flush_mode)
    return out + c.flush()


def member(payload: bytes, crc: int, isize: int, extra_first: bytes = b"") -> bytes:
    """One BGZF block around ``payload``; ``extra_first``: other subfields in front of BC in the extra field."""
    xlen = len(extra_first) + 6
    total = 12 + xlen + len(payload) + 8
    assert total <= 65536, total
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_first + b"BC" + struct.pack("<HH", 2, total - 1)
            + payload + struct.pack("<II", crc, isize))


def bgzf(text: bytes, block_bytes: int = 65280, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY,
         flush_every: Optional[int] = None) -> bytes:
    """``text`` as BGZF blocks of ``block_bytes`` of text each, without the EOF marker (append EOF_MARKER for one)."""
    out = []
    for lo in range(0, len(text), block_bytes):
        piece = text[lo:lo + block_bytes]
        out.append(member(deflate_raw(piece, level, strategy, flush_every), zlib.crc32(piece), len(piece)))
    return b"".join(out)


def expected(case: Case):
    """-> (accepted, text | None) by zlib."""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(case.payload)
    except zlib.error:
        return False, None
    if not d.eof or d.unused_data or len(text) != case.out_len or zlib.crc32(text) != case.crc:
        return False, None
    return True, text


def fastq_text(n_bytes: int, seed: int = 7) -> bytes:
    rng = random.Random(seed)
    out, i = [], 0
    size = 0
    while size < n_bytes:
        n = rng.randint(30, 151)
        rec = (f"@SIM:{seed}:{i} 1:N:0:ACGT\n" + "".join(rng.choice("ACGT") for _ in range(n)) + "\n+\n"
               + "".join(rng.choice("FFFFF:,#") for _ in range(n)) + "\n").encode()
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


def case_of(name: str, text: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, flush_mode=zlib.Z_SYNC_FLUSH) -> Case:
    return Case(name, deflate_raw(text, level, strategy, flush_every, flush_mode), len(text), zlib.crc32(text))


_STRATEGIES = (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huff", zlib.Z_HUFFMAN_ONLY))


def universe() -> List[tuple]:
    """About 60 well-formed blocks -> [(Case, text)]."""
    rng = random.Random(20240607)
    r = rng.randbytes(32768)
    kinds = [("fastq", fastq_text(60000)), ("run", b"G" * 65536), ("random", rng.randbytes(65280)), ("one", b"\n"), ("empty", b"")]
    out = []
    for kind, text in kinds:
        for level in (0, 1, 6, 9):
            out.append((case_of(f"{kind}-l{level}", text, level), text))
        for sname, strategy in _STRATEGIES:
            for level in (1, 9):
                out.append((case_of(f"{kind}-l{level}-{sname}", text, level, strategy), text))
    for sname, strategy in (("default", zlib.Z_DEFAULT_STRATEGY),) + _STRATEGIES:
        out.append((case_of(f"far-l9-{sname}", r + r, 9, strategy), r + r))  # matches at distance 32 768
    text = fastq_text(20000, seed=11)
    out.append((case_of("sync-700", text, 6, flush_every=700), text))  # empty stored blocks, odd bit offsets behind them
    out.append((case_of("full-700", text, 6, flush_every=700, flush_mode=zlib.Z_FULL_FLUSH), text))
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, bits: int):
        """``bits`` bits of ``value``, least significant first (header fields, extra bits)."""
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, bits: int):
        """A Huffman code, most significant bit first."""
        for i in range(bits - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def done(self) -> bytes:
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


_CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _hand_made() -> List[Case]:
    out = []
    text = b"ACGT" * 5
    crc = zlib.crc32(text)
    # stored block whose NLEN is not the complement of LEN
    out.append(Case("stored-nlen", b"\x01" + struct.pack("<HH", len(text), (~len(text) & 0xFFFF) ^ 0x0100) + text, len(text), crc))
    # block type 3
    b = _Bits(); b.put(1, 1); b.put(3, 2); b.put(0, 13)
    out.append(Case("btype-3", b.done() + text, len(text), crc))
    # dynamic header with HLIT = 30 (287 codes)
    b = _Bits(); b.put(1, 1); b.put(2, 2); b.put(30, 5); b.put(0, 5); b.put(15, 4)
    for _ in range(19):
        b.put(4, 3)
    b.put(0, 64)
    out.append(Case("hlit-287", b.done(), len(text), crc))
    # over-subscribed code-length code: three codes of one bit
    b = _Bits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    lens = {0: 1, 8: 1, 7: 1}
    for sym in _CLEN_ORDER:
        b.put(lens.get(sym, 0), 3)
    b.put(0, 64)
    out.append(Case("clen-oversubscribed", b.done(), len(text), crc))
    # the first code length is a repeat (16): nothing to repeat.  Code-length code: 16 and 0 with one bit each.
    b = _Bits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    lens = {16: 1, 0: 1}
    for sym in _CLEN_ORDER:
        b.put(lens.get(sym, 0), 3)
    b.code(1, 1)  # canonical: 0 -> '0', 16 -> '1'
    b.put(0, 2)
    b.put(0, 64)
    out.append(Case("repeat-first", b.done(), len(text), crc))
    # fixed block whose first symbol is a match: length code 257 (0000001), distance code 0 (00000), then end-of-block
    b = _Bits(); b.put(1, 1); b.put(1, 2); b.code(1, 7); b.code(0, 5); b.code(0, 7)
    out.append(Case("match-first", b.done(), 3, zlib.crc32(b"\0\0\0")))
    # dynamic block whose literal/length code has no end-of-block: literals 'A' and 'C' only, one bit each
    b = _Bits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    lens = {0: 1, 1: 2, 18: 2}  # code lengths: 0 -> '0', 1 -> '10', 18 -> '11'
    for sym in _CLEN_ORDER:
        b.put(lens.get(sym, 0), 3)
    def zeros(n):  # symbol 18: 11..138 zeros
        while n >= 11:
            k = min(n, 138)
            b.code(3, 2); b.put(k - 11, 7)
            n -= k
        for _ in range(n):
            b.code(0, 1)
    zeros(65); b.code(2, 2); zeros(1); b.code(2, 2); zeros(257 - 68)  # 'A' = 65, 'C' = 67 with length 1, the rest 0
    b.code(2, 2)  # one distance code of length 1
    for _ in range(32):
        b.code(0, 1)
    b.put(0, 64)
    out.append(Case("no-end-of-block", b.done(), 32, zlib.crc32(b"A" * 32)))
    return out


def corrupt_cases() -> List[Case]:
    """The fixed, seeded list.  (A few of its bit flips land where they change nothing zlib objects to -- an unused bit
    of the last byte --: ``expected`` says so, the list does not assume.)"""
    rng = random.Random(1951)
    text = fastq_text(2048, seed=3)
    bases = [case_of("stored", text, 0), case_of("fixed", text, 6, zlib.Z_FIXED), case_of("dynamic", text, 6)]
    out = []
    for base in bases:
        p, n, crc = base.payload, base.out_len, base.crc
        out.append(Case(f"{base.name}-crc", p, n, crc ^ 0x00010000))
        out.append(Case(f"{base.name}-isize+1", p, n + 1, crc))
        out.append(Case(f"{base.name}-isize-1", p, n - 1, crc))
        out.append(Case(f"{base.name}-cut1", p[:-1], n, crc))
        out.append(Case(f"{base.name}-half", p[:len(p) // 2], n, crc))
        out.append(Case(f"{base.name}-cut-all", b"", n, crc))
        out.append(Case(f"{base.name}-short-out", p, n - 100, zlib.crc32(text[:n - 100])))
    for i in range(64):
        base = bases[i % 3]
        bit = rng.randrange(8 * len(base.payload)) if i >= 12 else i // 3  # the first ones in the block header
        p = bytearray(base.payload)
        p[bit >> 3] ^= 1 << (bit & 7)
        out.append(Case(f"{base.name}-flip{bit}", bytes(p), base.out_len, base.crc))
    return out + _hand_made()


def mutations(n: int = 2000, seed: int = 4242) -> List[Case]:
    """Further seeded damage for the host build only: bit flips, truncations, byte splices."""
    rng = random.Random(seed)
    pool = [c for c, _ in universe() if 0 < len(c.payload) < 30000] + corrupt_cases()[:21:7]
    out = []
    for i in range(n):
        base = pool[rng.randrange(len(pool))]
        p = bytearray(base.payload)
        kind = rng.randrange(3)
        if kind == 0:
            for _ in range(rng.randint(1, 4)):
                bit = rng.randrange(8 * len(p))
                p[bit >> 3] ^= 1 << (bit & 7)
        elif kind == 1:
            del p[rng.randrange(len(p)):]
        else:
            a, b = sorted((rng.randrange(len(p) + 1), rng.randrange(len(p) + 1)))
            other = pool[rng.randrange(len(pool))].payload
            lo = rng.randrange(len(other))
            p[a:b] = other[lo:lo + rng.randint(0, 64)]
        out.append(Case(f"mut{i}-{base.name}", bytes(p), base.out_len, base.crc))
    return out


def write_case_file(path, cases: List[Case]) -> None:
    """What tools/inflate_host_check.cpp reads: "CSIC", count, then per case comp_len, out_len, crc and the payload."""
    with open(path, "wb") as fh:
        fh.write(b"CSIC" + struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(struct.pack("<III", len(c.payload), c.out_len, c.crc) + c.payload)
