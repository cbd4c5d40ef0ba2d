"""The device gzip writer (cutseq_amd/csrc/deflate_kernels.hip.inc) as plain rules: a strict parser of one gzip member,
the member's layout as conditions, the LZ77 matcher as byte loops, and Huffman references.  No GPU, no product code:
Python and ``zlib`` (for CRC-32) only.  tests/test_gzip_rule_cpu.py holds this file to zlib,
tests/test_gpu_gzip_structure.py holds the device to this file.

(a) ``parse_member``   RFC 1952 / RFC 1951 bit by bit: blocks, code lengths, tokens; refuses what a lenient inflater
                       lets through (incomplete codes, bytes behind the trailer, ...) with the offset in the message.
(b) ``check_layout``   what the header comment of the kernel file promises about a member.
(c) ``tokens``         the matcher: runs and the previous record's name, found per 128-byte slice.
(d) ``huffman_cost`` / ``limited_lengths``   the optimal code and the miniz-style length limit.
"""
import zlib
from typing import List, NamedTuple, Optional

CHUNK = 32768          # raw bytes per deflate block of the device
SLICE = 128            # raw bytes per thread: no match crosses a slice's end
MIN_MATCH = 4          # shortest run and shortest name match
MAX_LINES = 2304       # line ends of a chunk the device indexes
MAX_DYNAMIC = 20472    # bytes of a dynamic chunk that fit the device's bit buffer (5120 words less 8 bytes)
HEADER = bytes.fromhex("1f8b08000000000000ff")

_CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_LITS = [("lit", b) for b in range(256)]


class GzipError(ValueError):
    """What the strict parser refuses; the message names the bit or byte offset."""


class Block:
    """One deflate block.  ``btype`` 0 stored / 1 fixed / 2 dynamic; offsets in bits from the member's first byte;
    ``tokens``: this block's own (a stored block's bytes as literals).  Dynamic blocks: ``litlen`` (286 lengths),
    ``dist`` (30), ``clen`` (19, by symbol), ``hlit`` / ``hdist`` / ``hclen`` as found, ``cl_symbols``: the code-length
    symbols as sent (with 16 / 17 / 18 where the writer used them), ``data_bit``: where the tokens start."""

    def __init__(self, btype, final, start_bit):
        self.btype, self.final, self.start_bit = btype, final, start_bit
        self.end_bit = self.data_bit = start_bit
        self.raw_len = 0
        self.tokens = []
        self.litlen = self.dist = self.clen = self.cl_symbols = None
        self.hlit = self.hdist = self.hclen = None

    def __repr__(self):
        return f"Block(btype={self.btype}, final={self.final}, bits={self.start_bit}..{self.end_bit}, raw_len={self.raw_len})"


class Member(NamedTuple):
    data: bytes
    header_len: int
    blocks: List[Block]
    text: bytes      # re-inflated from the tokens
    crc: int
    isize: int

    @property
    def tokens(self):
        return [t for b in self.blocks for t in b.tokens]


def expand(tokens, window: bytes = b"") -> bytes:
    """The trivial LZ77 expander: ``tokens`` behind ``window`` (what earlier blocks produced) -> the new bytes."""
    out = bytearray(window)
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            _, length, dist = t
            if dist > len(out):
                raise GzipError(f"distance {dist} beyond the {len(out)} bytes produced so far")
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(window):])


def _reverse(code: int, bits: int) -> int:
    return int(format(code, f"0{bits}b")[::-1], 2)


def _code_table(lengths, what: str, at: int, single_bit_ok: bool = False):
    """Canonical code of RFC 1951 3.2.2 as a look-up table on the next ``maxlen`` bits (LSB first): entry = symbol << 4
    | length, 0 where no symbol has that code.  Refuses over-subscribed and incomplete codes; ``single_bit_ok``: a code
    of ONE symbol with one bit is let through (the pattern '1' then has no symbol)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    kraft = sum(count[l] << (15 - l) for l in range(1, 16))
    if kraft > 1 << 15:
        raise GzipError(f"over-subscribed {what} code in the block at bit {at}")
    if kraft < 1 << 15 and not (single_bit_ok and count[1] == 1 and len(lengths) - count[0] == 1):
        raise GzipError(f"incomplete {what} code in the block at bit {at}")
    maxlen = max(lengths)
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1] * (l > 1)) << 1
        nxt[l] = code
    table = [0] * (1 << maxlen)
    for sym, l in enumerate(lengths):
        if l:
            r = _reverse(nxt[l], l)
            nxt[l] += 1
            table[r::1 << l] = [sym << 4 | l] * (1 << (maxlen - l))
    return table, maxlen


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        _FIXED = _code_table(lit, "fixed literal/length", 0), _code_table([5] * 32, "fixed distance", 0)
    return _FIXED


class _Bits:
    def __init__(self, data: bytes, pos: int):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def at(self) -> int:
        return self.pos * 8 - self.n

    def take(self, k: int) -> int:
        while self.n < k:
            if self.pos >= len(self.data):
                raise GzipError(f"truncated: the data ends at byte {len(self.data)} inside a field of {k} bits")
            self.acc |= self.data[self.pos] << self.n
            self.pos += 1
            self.n += 8
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def align(self):
        drop = self.n & 7
        self.acc >>= drop
        self.n -= drop

    def symbol(self, table, maxlen: int, what: str) -> int:
        data = self.data
        while self.n < maxlen and self.pos < len(data):
            self.acc |= data[self.pos] << self.n
            self.pos += 1
            self.n += 8
        e = table[self.acc & ((1 << maxlen) - 1)]
        l = e & 15
        if l == 0:
            raise GzipError(f"a {what} symbol with no code at bit {self.at()}")
        if l > self.n:
            raise GzipError(f"truncated: the data ends at byte {len(data)} inside a {what} code")
        self.acc >>= l
        self.n -= l
        return e >> 4


def _dynamic_header(r: _Bits, blk: Block):
    at = blk.start_bit
    blk.hlit, blk.hdist, blk.hclen = r.take(5), r.take(5), r.take(4)
    nlit, ndist = blk.hlit + 257, blk.hdist + 1
    if nlit > 286 or ndist > 30:
        raise GzipError(f"HLIT {blk.hlit} / HDIST {blk.hdist} name more codes than exist, block at bit {at}")
    clen = [0] * 19
    for i in range(blk.hclen + 4):
        clen[_CLEN_ORDER[i]] = r.take(3)
    blk.clen = clen
    ctab, cmax = _code_table(clen, "code-length", at)
    lens, sent = [], []
    while len(lens) < nlit + ndist:
        sym = r.symbol(ctab, cmax, "code-length")
        sent.append(sym)
        if sym < 16:
            lens.append(sym)
            continue
        if sym == 16:
            if not lens:
                raise GzipError(f"a repeat with nothing to repeat at bit {r.at()}")
            rep, val = 3 + r.take(2), lens[-1]
        elif sym == 17:
            rep, val = 3 + r.take(3), 0
        else:
            rep, val = 11 + r.take(7), 0
        if len(lens) + rep > nlit + ndist:
            raise GzipError(f"a repeat runs past the last code length at bit {r.at()}")
        lens += [val] * rep
    blk.cl_symbols = sent
    blk.litlen = lens[:nlit] + [0] * (286 - nlit)
    blk.dist = lens[nlit:] + [0] * (30 - ndist)
    if blk.litlen[256] == 0:
        raise GzipError(f"no end-of-block code in the block at bit {at}")
    return _code_table(blk.litlen, "literal/length", at), _code_table(blk.dist, "distance", at, single_bit_ok=True)


def _coded_block(r: _Bits, blk: Block, out: bytearray, ltab, lmax, dtab, dmax):
    toks = blk.tokens
    data, size = r.data, len(r.data)
    lmask = (1 << lmax) - 1
    acc, n, pos = r.acc, r.n, r.pos
    while True:
        while n < lmax and pos < size:
            acc |= data[pos] << n
            pos += 1
            n += 8
        e = ltab[acc & lmask]
        l = e & 15
        if l == 0 or l > n:
            r.acc, r.n, r.pos = acc, n, pos
            if l == 0:
                raise GzipError(f"a literal/length symbol with no code at bit {r.at()}")
            raise GzipError(f"truncated: the data ends at byte {size} inside a literal/length code")
        acc >>= l
        n -= l
        sym = e >> 4
        if sym < 256:
            out.append(sym)
            toks.append(_LITS[sym])
            continue
        r.acc, r.n, r.pos = acc, n, pos
        if sym == 256:
            return
        if sym > 285:
            raise GzipError(f"literal/length symbol {sym} does not exist, bit {r.at()}")
        length = _LEN_BASE[sym - 257] + r.take(_LEN_EXTRA[sym - 257])
        ds = r.symbol(dtab, dmax, "distance")
        if ds > 29:
            raise GzipError(f"distance symbol {ds} does not exist, bit {r.at()}")
        dist = _DIST_BASE[ds] + r.take(_DIST_EXTRA[ds])
        if dist > len(out):
            raise GzipError(f"distance {dist} beyond the {len(out)} bytes produced so far, bit {r.at()}")
        start = len(out) - dist
        if dist >= length:
            out += out[start:start + length]
        else:
            seg = bytes(out[start:])
            out += (seg * (length // dist + 1))[:length]
        toks.append(("match", length, dist))
        acc, n, pos = r.acc, r.n, r.pos


def parse_member(data: bytes) -> Member:
    """One gzip member, strictly.  Raises GzipError; see the module's head for what it refuses."""
    data = bytes(data)
    if len(data) < 10:
        raise GzipError(f"truncated: {len(data)} bytes are no gzip header")
    if data[:3] != b"\x1f\x8b\x08":
        raise GzipError("byte 0: not a gzip member with the deflate method")
    flg, pos = data[3], 10
    if flg & 0xE0:
        raise GzipError("byte 3: reserved flag bits are set")
    try:
        if flg & 4:
            pos += 2 + int.from_bytes(data[pos:pos + 2], "little")
        for bit in (8, 16):
            if flg & bit:
                pos = data.index(b"\0", pos) + 1
        if flg & 2:
            pos += 2
    except ValueError:
        raise GzipError("truncated: the header's optional fields do not end") from None
    if pos > len(data):
        raise GzipError("truncated: the header's optional fields do not end")
    header_len = pos
    r = _Bits(data, pos)
    out = bytearray()
    blocks = []
    while True:
        start = r.at()
        final, btype = r.take(1), r.take(2)
        blk = Block(btype, final, start)
        before = len(out)
        if btype == 0:
            r.align()
            n, nn = r.take(16), r.take(16)
            if n != (~nn & 0xFFFF):
                raise GzipError(f"LEN {n:#06x} is not the complement of NLEN {nn:#06x} at bit {r.at() - 32}")
            assert r.n % 8 == 0
            lo = r.pos - r.n // 8
            if lo + n > len(data):
                raise GzipError(f"truncated: a stored block of {n} bytes at byte {lo}, the data ends at byte {len(data)}")
            r.pos, r.acc, r.n = lo + n, 0, 0
            blk.data_bit = lo * 8
            piece = data[lo:lo + n]
            out += piece
            blk.tokens = [_LITS[b] for b in piece]
        elif btype == 1:
            (ltab, lmax), (dtab, dmax) = _fixed_tables()
            blk.data_bit = r.at()
            _coded_block(r, blk, out, ltab, lmax, dtab, dmax)
        elif btype == 2:
            (ltab, lmax), (dtab, dmax) = _dynamic_header(r, blk)
            blk.data_bit = r.at()
            _coded_block(r, blk, out, ltab, lmax, dtab, dmax)
        else:
            raise GzipError(f"block type 3 at bit {start}")
        blk.end_bit = r.at()
        blk.raw_len = len(out) - before
        blocks.append(blk)
        if final:
            break
    r.align()
    end = r.pos - r.n // 8
    if len(data) < end + 8:
        raise GzipError(f"truncated: {len(data) - end} bytes of trailer at byte {end}")
    if len(data) > end + 8:
        raise GzipError(f"{len(data) - end - 8} bytes behind the trailer, which ends at byte {end + 8}")
    crc, isize = int.from_bytes(data[end:end + 4], "little"), int.from_bytes(data[end + 4:end + 8], "little")
    text = bytes(out)
    if crc != zlib.crc32(text):
        raise GzipError(f"CRC-32 at byte {end}: the trailer says {crc:#010x}, the text has {zlib.crc32(text):#010x}")
    if isize != len(text) & 0xFFFFFFFF:
        raise GzipError(f"ISIZE at byte {end + 4}: the trailer says {isize}, the text has {len(text)} bytes")
    return Member(data, header_len, blocks, text, crc, isize)


# ---- (b) the device's layout -----------------------------------------------------------------------------------

class Chunk(NamedTuple):
    index: int
    dynamic: bool
    block: Block     # the chunk's data block
    n_bytes: int     # what the chunk takes in the member
    raw_len: int


def check_layout(member: Member, text: bytes) -> List[Chunk]:
    """Asserts the layout the kernel file's header comment promises for the member of ``text``; -> its chunks."""
    assert member.data[:10] == HEADER and member.header_len == 10, member.data[:10].hex()
    n_chunks = (len(text) + CHUNK - 1) // CHUNK
    blocks = member.blocks
    chunks, i, at = [], 0, 80
    for c in range(n_chunks):
        raw = min(CHUNK, len(text) - c * CHUNK)
        assert i < len(blocks), f"chunk {c}: the member ends after {i} blocks"
        b = blocks[i]
        assert b.start_bit == at and at % 8 == 0, f"chunk {c} starts at bit {b.start_bit}, expected {at}"
        assert not b.final, f"chunk {c}: a final block in front of the member's last"
        assert b.raw_len == raw, f"chunk {c}: raw length {b.raw_len}, expected {raw}"
        if b.btype == 2:
            assert i + 1 < len(blocks), f"chunk {c}: nothing behind the dynamic block"
            e = blocks[i + 1]
            assert e.btype == 0 and not e.final and e.raw_len == 0, f"chunk {c}: no empty stored block behind the dynamic block: {e}"
            end = e.end_bit
            i += 2
        else:
            assert b.btype == 0, f"chunk {c}: block type {b.btype}"
            end = b.end_bit
            i += 1
        assert end % 8 == 0, f"chunk {c} ends at bit {end}"
        n_bytes = (end - at) // 8
        if b.btype == 2:
            assert n_bytes < raw + 5, f"chunk {c}: a dynamic chunk of {n_bytes} bytes for {raw} raw ones: stored is smaller"
            assert n_bytes <= MAX_DYNAMIC, f"chunk {c}: a dynamic chunk of {n_bytes} bytes"
        else:
            assert n_bytes == raw + 5
        chunks.append(Chunk(c, b.btype == 2, b, n_bytes, raw))
        at = end
    assert i == len(blocks) - 1, f"{len(blocks) - i} blocks behind the last chunk, expected the final one alone"
    last = blocks[i]
    assert last.btype == 1 and last.final and last.raw_len == 0 and last.start_bit == at, last
    assert member.data[at // 8:at // 8 + 2] == b"\x03\x00"
    assert len(member.data) == at // 8 + 10
    assert member.crc == zlib.crc32(text) and member.isize == len(text) & 0xFFFFFFFF
    assert member.text == text
    return chunks


# ---- (c) the matcher -------------------------------------------------------------------------------------------

def tokens(text: bytes, chunk_index: int, fasta: bool, lz: bool = True) -> list:
    """The tokens of chunk ``chunk_index`` of the stream ``text``.  Every 128-byte slice of the chunk is scanned left to
    right on its own.  At a record start -- the marker ('@', FASTA '>') directly behind a line end, or at stream offset
    0 -- the name match is tried first: the record's line index q is the number of the CHUNK's line ends in front of it;
    its predecessor starts ``lines`` (4, FASTA 2) line ends back, behind line end q - lines - 1 of the chunk, or at
    chunk position 0 when q == lines and the chunk starts a line; there is none when it lies in the chunk in front, or
    when q - lines >= 2304.  The match is the common prefix of the two, capped at the slice's end, taken when >= 4
    bytes.  Otherwise a run: a maximal stretch of bytes each equal to the byte in front of it (the byte in front of
    the chunk counts; stream offset 0 has none), capped at the slice's end, is a match of distance 1 when >= 4 bytes
    long.  Everything else is a literal.  ``lz=False``: literals only."""
    base = chunk_index * CHUNK
    chunk = text[base:base + CHUNK]
    if not lz:
        return [("lit", b) for b in chunk]
    marker = ord(">" if fasta else "@")
    lines = 2 if fasta else 4
    line_ends = [i for i, b in enumerate(chunk) if b == 10]
    chunk_starts_line = base == 0 or text[base - 1] == 10

    def byte_before(i):  # of chunk position i: None at stream offset 0
        return text[base + i - 1] if base + i > 0 else None

    out = []
    q = 0  # line ends of the chunk in front of position i
    for lo in range(0, len(chunk), SLICE):
        hi = min(lo + SLICE, len(chunk))
        i = lo
        while i < hi:
            length = dist = 0
            before = byte_before(i)
            if chunk[i] == marker and (before is None or before == 10):
                pred = None
                if q == lines and chunk_starts_line:
                    pred = 0
                elif q > lines and q - lines < MAX_LINES:
                    pred = line_ends[q - lines - 1] + 1
                if pred is not None:
                    while i + length < hi and chunk[pred + length] == chunk[i + length]:
                        length += 1
                    dist = i - pred
            if length < MIN_MATCH:
                length, dist = 0, 1
                while i + length < hi and chunk[i + length] == byte_before(i + length):
                    length += 1
            if length >= MIN_MATCH:
                out.append(("match", length, dist))
            else:
                length = max(length, 1)  # (a short stretch: literals, none of which can start a longer one)
                out += [("lit", b) for b in chunk[i:i + length]]
            q += chunk.count(b"\n", i, i + length)
            i += length
    return out


# ---- (d) Huffman references ------------------------------------------------------------------------------------

def length_symbol(length: int) -> int:
    return 257 + max(k for k in range(29) if _LEN_BASE[k] <= length) if length < 258 else 285


def distance_symbol(dist: int) -> int:
    return max(k for k in range(30) if _DIST_BASE[k] <= dist)


def frequencies(toks):
    """-> (literal/length[286], distance[30]) of a block with these tokens, as the device counts them: the end of block
    once, and distance symbol 0 once more than it is used (a block names at least one distance code)."""
    lit, dist = [0] * 286, [0] * 30
    for t in toks:
        if t[0] == "lit":
            lit[t[1]] += 1
        else:
            lit[length_symbol(t[1])] += 1
            dist[distance_symbol(t[2])] += 1
    lit[256] += 1
    dist[0] += 1
    return lit, dist


def extra_bits(toks) -> int:
    return sum(_LEN_EXTRA[length_symbol(t[1]) - 257] + _DIST_EXTRA[distance_symbol(t[2])] for t in toks if t[0] == "match")


class Huffman(NamedTuple):
    cost: int        # sum of frequency * length: optimal
    depth: int       # of THIS tree (two-queue merge, ties take the leaf)
    lengths: list    # per symbol, 0: unused


def huffman_cost(freqs) -> Huffman:
    """The optimal prefix code without a length limit.  One used symbol: one bit."""
    leaves = sorted((f, s) for s, f in enumerate(freqs) if f)
    n = len(leaves)
    lengths = [0] * len(freqs)
    if n == 0:
        return Huffman(0, 0, lengths)
    if n == 1:
        lengths[leaves[0][1]] = 1
        return Huffman(leaves[0][0], 1, lengths)
    weight = [f for f, _ in leaves]
    parent = [0] * (2 * n - 1)
    leaf, inode = 0, n
    for _ in range(n - 1):
        pick = []
        for _ in range(2):
            if leaf < n and (inode >= len(weight) or weight[leaf] <= weight[inode]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(inode)
                inode += 1
        weight.append(weight[pick[0]] + weight[pick[1]])
        parent[pick[0]] = parent[pick[1]] = len(weight) - 1
    depth = [0] * (2 * n - 1)
    for v in range(2 * n - 3, -1, -1):
        depth[v] = depth[parent[v]] + 1
    for k, (_, s) in enumerate(leaves):
        lengths[s] = depth[k]
    return Huffman(sum(f * depth[k] for k, (f, _) in enumerate(leaves)), max(depth[:n]), lengths)


def histogram(lengths, maxlen: Optional[int] = None) -> list:
    """-> count[l] for l = 0 .. maxlen (default: the longest), count[0] = 0: unused symbols are not counted."""
    top = max(list(lengths) + [0]) if maxlen is None else maxlen
    count = [0] * (top + 1)
    for l in lengths:
        if l:
            count[l] += 1
    return count


def limited_lengths(freqs, maxlen: int) -> list:
    """Lengths per symbol under the miniz-style limit: the optimal tree's length histogram with everything above
    ``maxlen`` folded into ``maxlen``, Kraft's sum repaired by the published loop (drop one code of the limit, split the
    longest shorter code in two), and the lengths dealt out by rank: the rarest symbols get the longest codes."""
    h = huffman_cost(freqs)
    used = sorted((f, s) for s, f in enumerate(freqs) if f)
    out = [0] * len(freqs)
    if len(used) < 2:
        return h.lengths
    count = [0] * (maxlen + 1)
    for l in h.lengths:
        if l:
            count[min(l, maxlen)] += 1
    total = sum(count[l] << (maxlen - l) for l in range(1, maxlen + 1))
    while total > 1 << maxlen:
        count[maxlen] -= 1
        for l in range(maxlen - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    rank = 0
    for l in range(maxlen, 0, -1):
        for _ in range(count[l]):
            out[used[rank][1]] = l
            rank += 1
    return out


def dynamic_chunk_bytes(toks) -> int:
    """What the chunk with these tokens takes as the device builds it: the block header (17 bits, all 19 code-length
    lengths, the 316 code lengths one by one, no repeat symbols), the tokens and the end of block in the limited codes,
    the empty stored block (3 bits, to the byte, LEN and NLEN)."""
    lit, dist = frequencies(toks)
    ll, dl = limited_lengths(lit, 15), limited_lengths(dist, 15)
    cl = limited_lengths([(ll + dl).count(l) for l in range(19)], 7)
    bits = (17 + 57 + sum(cl[l] for l in ll + dl) + sum(f * l for f, l in zip(lit, ll))
            + sum(f * l for f, l in zip(dist, dl)) - dl[0] + extra_bits(toks))
    return (bits + 3 + 7) // 8 + 4


def kraft(lengths) -> float:
    from fractions import Fraction
    return sum(Fraction(1, 1 << l) for l in lengths if l)
