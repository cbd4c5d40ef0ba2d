"""The record finder of the text path as a RULE on bytes, and the texts that hold it to that rule.

What it restates: the newline index and the record parser of the device (text_kernels.hip.inc: text_count_nl,
text_scan_blocks, text_write_nl, text_parse_records and its woven twin, text_check_pairs) and their host twin
(cutseq_host.c: csh_fastq_parse) -- the counterpart of dnaio's FASTQ reader as cutadapt drives it for the reference
(cutseq/run.py:434-441, 751-758).  Nothing here knows either implementation: ``bytes.split`` and loops, and of the
product only the ``abi`` constants.

The rule (:func:`parse`):

  lines     the lines of a text are ``text.split(b"\\n")``.  A batch of ``n`` records has ``4n`` line ends (``8n`` for an
            interleaved text); what follows the last of them is not looked at (case e, "bytes-behind-the-last-line-end").  It may instead have ONE fewer and a last
            byte that is not ``\\n``: the end of the text then ends the last line.  Anything else is the key
            ``(0, LINE_COUNT)`` for that text, and none of its records is looked at.  (``n = 0``: nothing is looked at.)
  \\r        exactly one trailing ``\\r`` is taken off every line; any other ``\\r`` is payload
  headers   line 0 is non-empty (behind the ``\\r`` rule) and begins with ``@``; line 2 is non-empty and begins with ``+``;
            what follows the ``+`` is compared with nothing
  lengths   lines 1 and 3 have equal lengths, the name behind the ``@`` has at most 65 535 bytes: else ``(r, MALFORMED)``.
            A well-formed read longer than ``abi.CS_MAX_READ`` is ``(r, TOO_LONG)`` (tests/test_gpu_long_reads.py builds it)
  woven     record ``r`` of mate ``m`` stands at lines ``4(2r + m) .. 4(2r + m) + 3`` of the one text

:func:`names_match` is dnaio's ``record_names_match`` on the names behind the SuffixRemover literals (``hostfmt``, held to
``str.split`` and to the host by tests/test_names_cpu.py); :func:`batch_error` is the key a batch is refused with: the
smallest ``(record, code)`` over both mates' parse keys and the ``IDS_DIFFER`` keys.

Known difference from dnaio, NOT pinned here and out of scope: dnaio is believed to refuse a non-empty ``+name`` line that
differs from the header ("Sequence descriptions don't match").  The device parser and the host parser both accept any
``+`` line, and so does this rule ("recalled and not pinned").

The writers (:func:`write`, :func:`place`, :func:`sized`, :func:`poison`) and the case lists below them are what
tests/test_reader_rule_cpu.py runs through the host parser and tests/test_gpu_text_structure.py through the device.
Deterministic: no seed is drawn anywhere.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Set, Tuple, Union

from cutseq_amd import abi

import hostfmt
import names_universe as nu

MALFORMED, TOO_LONG = abi.CS_TEXT_ERR_MALFORMED, abi.CS_TEXT_ERR_TOO_LONG
IDS_DIFFER, LINE_COUNT = abi.CS_TEXT_ERR_IDS_DIFFER, abi.CS_TEXT_ERR_LINE_COUNT
LF, CRLF = b"\n", b"\r\n"
MAX_NAME = 65535
SEG = 16384  # bytes of text per block of the newline passes (named here, not imported: the boundaries are the rule's)

Record = Tuple[bytes, bytes, bytes]  # (name, seq, qual)
Key = Tuple[int, int]                # (record, code); tuples order like the device's record << 8 | code


class Records(list):
    """What an accepted text holds: a list of (name, seq, qual)."""


# ---- the rule ----------------------------------------------------------------------------------------------------------


def line_ends(text: bytes) -> int:
    return text.count(b"\n")


def _lines(text: bytes, want: int) -> Optional[List[bytes]]:
    parts = text.split(b"\n")
    ends = len(parts) - 1
    if ends == want:
        return parts[:want]
    if ends + 1 == want and text and not text.endswith(b"\n"):
        return parts  # (the last part is not empty: the end of the text ends it)
    return None


def _strip_cr(line: bytes) -> bytes:
    return line[:-1] if line.endswith(b"\r") else line


def parse(text: bytes, n_records: int, woven: bool = False, mate: int = 0) -> Union[Records, Set[Key]]:
    """-> Records, or the set of EVERY key the text has (the smallest is what a reader reports)."""
    if n_records == 0:
        return Records()
    lines = _lines(text, (8 if woven else 4) * n_records)
    if lines is None:
        return {(0, LINE_COUNT)}
    out, keys = Records(), set()
    for r in range(n_records):
        first = 4 * (2 * r + mate) if woven else 4 * r
        head, seq, plus, qual = [_strip_cr(line) for line in lines[first:first + 4]]
        bad = not head or head[:1] != b"@" or not plus or plus[:1] != b"+"
        bad = bad or len(seq) != len(qual) or len(head) - 1 > MAX_NAME
        if bad:
            keys.add((r, MALFORMED))
        elif len(seq) > abi.CS_MAX_READ:
            keys.add((r, TOO_LONG))
        else:
            out.append((head[1:], seq, qual))
    return keys if keys else out


def names_match(name1: bytes, name2: bytes, suffixes=nu.SUFFIXES) -> bool:
    """dnaio.record_names_match as text_check_pairs applies it: on the names behind the SuffixRemover literals; the id runs
    up to the first space or tab, one trailing 1 / 2 / 3 is ignored when both ids have one."""
    return hostfmt.ids_match(hostfmt.strip_suffixes(name1, suffixes[0]), hostfmt.strip_suffixes(name2, suffixes[1]))


def _good(text: bytes, n_records: int, woven: bool, mate: int) -> Dict[int, bytes]:
    """record -> name of the well-formed records of a text that has an index."""
    out = {}
    lines = _lines(text, (8 if woven else 4) * n_records)
    for r in range(n_records):
        first = 4 * (2 * r + mate) if woven else 4 * r
        one = parse(b"\n".join(lines[first:first + 4]) + b"\n", 1)
        if isinstance(one, Records):
            out[r] = one[0][0]
        elif one == {(0, TOO_LONG)}:
            out[r] = _strip_cr(lines[first])[1:]
    return out


def batch_error(text1: bytes, text2: Optional[bytes], n_records: int, woven: bool = False, suffixes=nu.SUFFIXES) -> Optional[Key]:
    """The key a batch is refused with, or None.  ``text2`` None: single end (``woven``: both mates in ``text1``).
    An IDS_DIFFER key exists only for a record that is well formed in both mates, and only when both texts have a
    newline index."""
    if woven:
        mates = [(text1, 0), (text1, 1)]
    else:
        mates = [(text1, 0)] + ([(text2, 0)] if text2 is not None else [])
    keys: Set[Key] = set()
    indexed = True
    for text, m in mates:
        got = parse(text, n_records, woven, m)
        if not isinstance(got, Records):
            keys |= got
            indexed = indexed and (0, LINE_COUNT) not in got
    if len(mates) == 2 and indexed and n_records:
        a = _good(mates[0][0], n_records, woven, mates[0][1])
        b = _good(mates[1][0], n_records, woven, mates[1][1])
        for r in sorted(set(a) & set(b)):
            if not names_match(a[r], b[r], suffixes):
                keys.add((r, IDS_DIFFER))
    return min(keys) if keys else None


# ---- writers -----------------------------------------------------------------------------------------------------------

Lines = List[bytes]  # the four lines of a record as written, without their line ends


def record_lines(rec: Record, plus: bytes = b"+") -> Lines:
    return [b"@" + rec[0], rec[1], plus, rec[2]]


def join_lines(recs: Sequence[Lines], eol: bytes = LF, final_newline: bool = True) -> bytes:
    text = b"".join(line + eol for lines in recs for line in lines)
    return text if final_newline or not text else text[:-1]  # (without the final newline a "\r\n" text ends in "\r")


def write(records: Sequence[Record], eol: bytes = LF, final_newline: bool = True, plus: bytes = b"+") -> bytes:
    return join_lines([record_lines(r, plus) for r in records], eol, final_newline)


def _padded(records: Sequence[Record], r: int, pad: int) -> List[Record]:
    if pad < 0 or len(records[r][0]) + pad > MAX_NAME:
        raise ValueError(f"cannot pad the header of record {r} by {pad} bytes")
    out = list(records)
    out[r] = (records[r][0] + b"p" * pad, records[r][1], records[r][2])
    return out


def place(records: Sequence[Record], r: int, k: int, at: int, eol: bytes = LF) -> Tuple[bytes, List[Record]]:
    """-> (text, records as written): the ``\\n`` that ends line ``k`` of record ``r`` stands at byte ``at``, the header of
    record ``r`` padded to get it there."""
    def where(recs):
        before = write(recs[:r], eol)
        return len(before) + len(b"".join(line + eol for line in record_lines(recs[r])[:k + 1])) - 1
    recs = _padded(records, r, at - where(list(records)))
    text = write(recs, eol)
    assert text[at:at + 1] == b"\n" and line_ends(text[:at]) == 4 * r + k
    return text, recs


def place_woven(records1: Sequence[Record], records2: Sequence[Record], r: int, mate: int, k: int, at: int,
                eol: bytes = LF) -> bytes:
    """-> the interleaved text of the two mates' records in which the ``\\n`` that ends line ``k`` of record ``r`` of mate
    ``mate`` (0 / 1) stands at byte ``at`` -- line ``4(2r + mate) + k`` of the one text -- that record's header padded."""
    order = [rec for pair in zip(records1, records2) for rec in pair]
    text, _ = place(order, 2 * r + mate, k, at, eol)
    assert text[at:at + 1] == b"\n" and line_ends(text[:at]) == 4 * (2 * r + mate) + k
    return text


def split_tail(text: bytes, n_records: int, woven: bool = False) -> Tuple[bytes, bytes]:
    """-> (the text up to its 4n-th line end, what follows it): the rule looks at the first part alone."""
    parts = text.split(b"\n")
    want = (8 if woven else 4) * n_records
    if len(parts) - 1 < want:
        return text, b""
    body = b"".join(p + b"\n" for p in parts[:want])
    return body, text[len(body):]


def sized(records: Sequence[Record], total: int, eol: bytes = LF, final_newline: bool = True) -> Tuple[bytes, List[Record]]:
    """-> (text, records as written): a text of exactly ``total`` bytes, the header of record 0 padded."""
    recs = _padded(records, 0, total - len(write(records, eol, final_newline)))
    text = write(recs, eol, final_newline)
    assert len(text) == total
    return text, recs


def poison(n_bytes: int) -> Tuple[bytes, int]:
    """-> (text of exactly ``n_bytes``, its records): valid records ``@\\n\\n+\\n\\n`` back to back -- two of every three bytes
    are ``\\n`` -- the header of the last one padded to fill.  What a slot's text buffer holds behind a shorter text that
    follows: stale bytes that are newline-dense at every alignment."""
    n = n_bytes // 6
    if n < 1:
        raise ValueError("a poison text has at least one record (6 bytes)")
    text = b"@\n\n+\n\n" * (n - 1) + b"@" + b"p" * (n_bytes - 6 * n) + b"\n\n+\n\n"
    assert len(text) == n_bytes
    return text, n


# ---- reads and records of the cases ------------------------------------------------------------------------------------

STRIDE = 24               # rows of the GPU tests: a read of 25 is a long read (long_kernel.hip.inc)
MAX_LEN = 25
_BASES = b"ACGTNacgtnRYKMSWBDHVrykm"  # what tests/test_gpu_parity.py feeds the kernels: lower case and IUPAC


def read_of(i: int, length: int) -> Tuple[bytes, bytes]:
    """A read of ``length`` bases, different for every ``i``; qualities are printable ('#' .. 'J')."""
    seq = bytes(_BASES[(i * 7 + j * (3 + i % 5) + j * j) % len(_BASES)] for j in range(length))
    qual = bytes(35 + (i * 5 + j * 11) % 40 for j in range(length))
    return seq, qual


def good_records(n: int, mate: int = 1, first: int = 0) -> List[Record]:
    """``n`` records ``r<i> m<mate>`` with reads of 0 .. 25 bases (every length within any 26 records in a row)."""
    out = []
    for i in range(first, first + n):
        seq, qual = read_of(i * 2 + mate, (i * 7 + 3 * mate) % (MAX_LEN + 1))
        out.append((b"r%d m%d" % (i, mate), seq, qual))
    return out


class Case(NamedTuple):
    name: str
    text: bytes
    n: int
    woven: bool = False


# ---- a. line ends on boundaries ----------------------------------------------------------------------------------------

BOUNDARIES = (16, 64, SEG, 2 * SEG)
DELTAS = (-2, -1, 0, 1)


def boundary_cases(boundaries=BOUNDARIES) -> List[Case]:
    """The ``\\n`` of line ``k`` of a chosen record at byte ``B + delta``; with ``\\r\\n`` and delta 0 the two bytes of the line
    end straddle the boundary.  Three records (B = 16: record 0 is the chosen one, else record 1)."""
    out = []
    for B in boundaries:
        for delta in DELTAS:
            for k in range(4):
                for eol in (LF, CRLF):
                    r = 0 if B == 16 else 1
                    recs = [(b"a", b"Ac", b"I#"), (b"b x", ) + read_of(B + k, MAX_LEN if k % 2 and B > 64 else 7), (b"c", b"", b"")]
                    text, _ = place(recs, r, k, B + delta, eol)
                    out.append(Case(f"a:B={B},d={delta},k={k},{'crlf' if eol == CRLF else 'lf'}", text, 3))
    return out


def woven_boundary_cases(boundaries=(SEG,)) -> List[Case]:
    """Case a on an interleaved text: the chosen line end is line ``4(2r + m) + k`` of the ONE text, r = 1, for a record
    of each mate; three pairs."""
    out = []
    for B in boundaries:
        for delta in DELTAS:
            for k in range(4):
                for eol in (LF, CRLF):
                    for mate in (0, 1):
                        recs1 = [(b"a", b"Ac", b"I#"), (b"b x", ) + read_of(B + k, MAX_LEN if k % 2 else 7), (b"c", b"", b"")]
                        recs2 = [(b"a", ) + read_of(B + 9, 5), (b"b y", ) + read_of(B + k + 1, 7 if k % 2 else MAX_LEN), (b"c", b"G", b"#")]
                        text = place_woven(recs1, recs2, 1, mate, k, B + delta, eol)
                        out.append(Case(f"i-a:B={B},d={delta},k={k},{'crlf' if eol == CRLF else 'lf'},mate={mate + 1}", text, 3, True))
    return out


# ---- b. text ends on boundaries ----------------------------------------------------------------------------------------


def text_end_cases(segments=(1, 2)) -> List[Case]:
    """Texts of ``16384 s + d`` bytes, d in [-17, 17], ending in ``\\n`` and without the final newline (the last byte is a
    quality byte); and the text whose last line is ``IIII\\r`` without a ``\\n``."""
    recs = [(b"a x",) + read_of(1, 9), (b"b",) + read_of(2, MAX_LEN), (b"c", b"ACGT", b"IIII")]
    out = []
    for s in segments:
        for d in range(-17, 18):
            for final in (True, False):
                text, _ = sized(recs, SEG * s + d, LF, final)
                assert text.endswith(b"\n" if final else b"I")
                out.append(Case(f"b:s={s},d={d},{'nl' if final else 'no-nl'}", text, 3))
        text, _ = sized(recs, SEG * s, CRLF, False)
        assert text.endswith(b"IIII\r")
        out.append(Case(f"b:s={s},IIII-cr", text, 3))
    return out


# ---- c. bytes that look like '\n' --------------------------------------------------------------------------------------

LOOKALIKES = (0x00, 0x09, 0x0B, 0x0D, 0x7F, 0x80, 0x8A)
SPOTS = ("header-first", "header-last", "quality-first", "quality-last")


def _into_lane(before: int, filler: Lines, offset: int, lane: int) -> Lines:
    """``filler`` with its header padded so that the byte ``offset`` bytes behind it stands in byte lane ``lane`` of a
    dword, in a text that has ``before`` bytes in front of the filler."""
    for pad in range(4):
        lines = [filler[0] + b"p" * pad] + filler[1:]
        if (before + len(join_lines([lines])) + offset) % 4 == lane:
            return lines
    raise AssertionError("four paddings reach four lanes")


def lookalike_cases() -> List[Case]:
    """One text per byte and spot.  header-last / quality-last: directly in front of a line end; quality-first: directly
    behind one (the ``+`` line's); header-first: behind the ``@`` that stands directly behind one.  Per text four records
    that carry the byte, each behind a filler record whose header is padded so that the byte stands in lanes 0, 1, 2, 3
    of a dword (asserted).  ``\\r`` in front of a line end is the line end's: the sequence is written one base shorter so
    that the record stays well formed -- every case is accepted."""
    out = []
    for byte in LOOKALIKES:
        c = bytes([byte])
        for spot in SPOTS:
            recs: List[Lines] = []
            for lane in range(4):
                name, (seq, qual) = b"n%d x" % lane, read_of(byte + lane, 6)
                if spot == "header-first":
                    name = c + name
                elif spot == "header-last":
                    name = name + c
                elif spot == "quality-first":
                    qual = c + qual[1:]
                else:
                    qual = qual[:-1] + c
                    if byte == 0x0D:
                        seq = seq[:-1]
                lines = [b"@" + name, seq, b"+", qual]
                offset = {"header-first": 1, "header-last": len(lines[0]) - 1, "quality-first": len(lines[0]) + len(seq) + 4,
                          "quality-last": len(lines[0]) + len(seq) + 4 + len(qual) - 1}[spot]
                recs.append(_into_lane(len(join_lines(recs)), record_lines((b"f%d x" % lane,) + read_of(lane, 3)), offset, lane))
                at = len(join_lines(recs)) + offset
                recs.append(lines)
                assert join_lines(recs)[at] == byte and at % 4 == lane, (byte, spot, lane, at)
            out.append(Case(f"c:0x{byte:02x},{spot}", join_lines(recs), 8))
    return out


# ---- d. text_restride --------------------------------------------------------------------------------------------------

RESTRIDE_LENGTHS = (0, 1, 2, 3, 4, 5, 23, 24, 25)


def restride_cases() -> List[Case]:
    """One text per line end: the sequence line's start offset mod 4 takes 0 .. 3 for every read length (asserted), the
    quality line's with it.  The byte behind every read is its line end, never ``N`` or 0."""
    out = []
    for eol in (LF, CRLF):
        recs: List[Record] = []
        seen = set()
        for length in RESTRIDE_LENGTHS:
            for lane in range(4):
                seq, qual = read_of(length * 4 + lane, length)
                for pad in range(4):
                    rec = (b"d%d.%d " % (length, lane) + b"p" * pad, seq, qual)
                    start = len(write(recs, eol)) + 1 + len(rec[0]) + len(eol)
                    if start % 4 == lane:
                        break
                recs.append(rec)
                seen.add((start % 4, length))
        assert len(seen) == 4 * len(RESTRIDE_LENGTHS)
        out.append(Case(f"d:{'crlf' if eol == CRLF else 'lf'}", write(recs, eol), len(recs)))
    return out


# ---- e. accepted oddities ----------------------------------------------------------------------------------------------


def oddity_cases() -> List[Case]:
    a, b = (b"a x",) + read_of(3, 11), (b"b x",) + read_of(4, 8)
    la, lb = record_lines(a), record_lines(b)

    def text(*recs, eols=None):
        if eols is None:
            return join_lines(list(recs))
        lines = [line for rec in recs for line in rec]
        return b"".join(line + eol for line, eol in zip(lines, eols))

    odd = {
        "plus-name": text(la, [lb[0], lb[1], b"+b x", lb[3]]),
        "plus-anything": text([la[0], la[1], b"+@ no such name\t+", la[3]], lb),
        "plus-cr": text(la, [lb[0], lb[1], b"+\r", lb[3]]),
        "at-alone": text([b"@", la[1], la[2], la[3]], lb),
        "empty-read": text(la, [lb[0], b"", b"+", b""], la),
        "quality-begins-with-at": text(la, [lb[0], lb[1], lb[2], b"@" + lb[3][1:]], la),
        "quality-begins-with-plus": text(la, [lb[0], lb[1], lb[2], b"+" + lb[3][1:]], la),
        "sequence-begins-with-at": text(la, [lb[0], b"@" + lb[1][1:], lb[2], lb[3]], la),
        "cr-on-some-lines": text(la, lb, la, eols=[CRLF, LF, LF, CRLF, LF, CRLF, CRLF, LF, CRLF, CRLF, CRLF, LF]),
        "cr-inside-lines": text([b"@a\rx y", la[1][:4] + b"\r" + la[1][5:], b"+\r+", la[3][:4] + b"\r" + la[3][5:]], lb),
        "bytes-behind-the-last-line-end": text(la, lb) + b"@c x",
        "name-of-65535": text(la, [b"@" + b"n" * MAX_NAME, lb[1], lb[2], lb[3]], la),
    }
    return [Case("e:" + name, t, line_ends(t) // 4) for name, t in odd.items()]  # (every one ends its 4n lines)


def name_too_long_case() -> Case:
    """A name of 65 536 bytes in record 1 of 3: ``(1, MALFORMED)``.  Outside the host parser's domain (it keeps a name's
    length in 32 bits and takes it), so not in :func:`universe`."""
    a = (b"a x",) + read_of(3, 11)
    return Case("e:name-of-65536", write([a, (b"n" * (MAX_NAME + 1),) + read_of(4, 8), a]), 3)


# ---- f. every defect at every place ------------------------------------------------------------------------------------


def _set(i: int, value: bytes) -> Callable[[Lines], Lines]:
    return lambda lines: lines[:i] + [value] + lines[i + 1:]


DEFECTS: Dict[str, Callable[[Lines], Lines]] = {
    "first-byte-not-at": lambda l: [b"r" + l[0][1:]] + l[1:],
    "empty-header": _set(0, b""),
    "header-cr-alone": _set(0, b"\r"),
    "empty-plus": _set(2, b""),
    "plus-cr-alone": _set(2, b"\r"),
    "plus-other-byte": _set(2, b"-"),
    "sequence-longer": lambda l: [l[0], l[1] + b"A", l[2], l[3]],
    "quality-longer": lambda l: [l[0], l[1], l[2], l[3] + b"I"],
    "two-crs": lambda l: [l[0], b"ACGT\r\r", l[2], b"IIII\r"],
}
DEFECT_BATCH = 600
DEFECT_PLACES = (0, 1, 255, 256, 257, DEFECT_BATCH - 1)  # the edges of the 256-record blocks of the parse kernels
DEFECT_SIZES = (1, 255, 256, 257)                        # batches with the defect in their last record


def defective(n: int, defects: Sequence[Tuple[int, str]], mate: int = 1, eol: bytes = LF, final_newline: bool = True) -> bytes:
    """The text of ``good_records(n, mate)`` with the named defects in the given records."""
    recs = [record_lines(r) for r in good_records(n, mate)]
    for r, name in defects:
        recs[r] = DEFECTS[name](recs[r])
    return join_lines(recs, eol, final_newline)


def defect_places() -> List[Tuple[str, int, int]]:
    """(defect, batch size, record) of case f."""
    return ([(d, DEFECT_BATCH, r) for d in DEFECTS for r in DEFECT_PLACES]
            + [(d, n, n - 1) for d in DEFECTS for n in DEFECT_SIZES])


def defect_cases(mate: int = 1) -> List[Case]:
    return [Case(f"f:{d},n={n},r={r}", defective(n, [(r, d)], mate), n) for d, n, r in defect_places()]


# ---- g. line counts and two defects in one text ------------------------------------------------------------------------

KEY_BATCH = 800


def line_count_texts(n: int, mate: int = 1) -> Dict[str, bytes]:
    """Texts of ``n`` good records with 4n - 2 and 4n + 1 line ends, and with 4n - 1 ending in ``\\n``."""
    good = write(good_records(n, mate))
    lines = good.split(b"\n")[:-1]
    out = {"4n-2": b"\n".join(lines[:-1]),
           "4n+1": good + b"\n",
           "4n-1,ends-in-nl": b"\n".join(lines[:-1]) + b"\n"}
    assert [line_ends(t) - 4 * n for t in out.values()] == [-2, 1, -1] and out["4n-1,ends-in-nl"].endswith(b"\n")
    return out


def key_cases() -> List[Case]:
    out = [Case("g:malformed-at-10-and-700", defective(KEY_BATCH, [(700, "plus-other-byte"), (10, "quality-longer")]), KEY_BATCH),
           Case("g:no-records", b"", 0)]
    for n in (1, 5, KEY_BATCH):
        for name, text in line_count_texts(n).items():
            out.append(Case(f"g:lines={name},n={n}", text, n))
    # 4n - 1 line ends, a last byte of "\n" and an EMPTY last read: a reader that let the end of the text stand in here
    # would find n well-formed records
    text = write(good_records(4) + [(b"c", b"", b"")])[:-1]
    assert text.endswith(b"+\n") and line_ends(text) == 4 * 5 - 1
    out.append(Case("g:lines=4n-1,ends-in-nl,empty-last-read", text, 5))
    return out


# ---- h. more than 1024 segments ----------------------------------------------------------------------------------------

BIG_HEADER = 60_000


def big_case(segments: int, blank: bool = False) -> Case:
    """A text of exactly ``segments * 16384`` bytes (so: that many segments, the last one full) of records with
    60 000-byte headers; the last header is shorter, to fit.  The headers hold no blank: each is its own id, and the
    output carries all of it (``blank``: one behind the record's number, the rest is a comment that no output has)."""
    total = segments * SEG
    recs: List[Record] = []
    at = 0
    while total - at > BIG_HEADER + 200:
        seq, qual = read_of(len(recs), len(recs) % (MAX_LEN + 1))
        name = b"h%d" % len(recs) + (b" " if blank else b"")
        recs.append((name + b"p" * (BIG_HEADER - len(name)), seq, qual))
        at += len(write(recs[-1:]))
    recs.append((b"last " if blank else b"last", b"ACGTacgtN", b"IIIIIIII#"))
    text, _ = sized(recs[-1:], total - at)
    text = write(recs[:-1]) + text
    assert len(text) == total and (len(text) + SEG - 1) // SEG == segments
    return Case(f"h:{segments}-segments", text, len(recs))


# ---- i. woven ----------------------------------------------------------------------------------------------------------


def weave_lines(text1: bytes, text2: bytes, n: int) -> bytes:
    """The interleaved text of two texts that each HAVE their 4n line ends: four lines of one, four of the other.  Line
    by line, not record by record -- the lines of a malformed record are woven like any others."""
    a, b = text1.split(b"\n"), text2.split(b"\n")
    assert len(a) == len(b) == 4 * n + 1 and a[-1] == b[-1] == b""
    out = []
    for r in range(n):
        out += a[4 * r:4 * r + 4] + b[4 * r:4 * r + 4]
    return b"".join(line + b"\n" for line in out)


# ---- the universe of single texts --------------------------------------------------------------------------------------


def universe(big: bool = True) -> List[Case]:
    """Every single-text case of a .. h (i and j run the same texts another way)."""
    out = (boundary_cases() + text_end_cases() + lookalike_cases() + restride_cases() + oddity_cases() + defect_cases()
           + key_cases())
    if big:
        out += [big_case(1025), big_case(1024, blank=True)]
    assert len({c.name for c in out}) == len(out)
    return out
