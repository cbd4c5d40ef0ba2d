"""The record finder of the text path held to tests/reader_rule.py at every edge: text_count_nl, text_scan_blocks,
text_write_nl, text_parse_records and its woven twin, text_check_pairs, text_restride (text_kernels.hip.inc) and
cs_text_submit_device.

Reference surface replaced: dnaio's FASTQ reader and ``record_names_match`` as cutadapt drives them for the reference
(cutseq/run.py:434-441, 751-758, 642-645).

How an expectation is formed: the RULE says what a text holds -- ``Records`` or the key it is refused with.  Records are
packed into rows (util.batch_from_records), trimmed by the C oracle and formatted by the record logic
(test_gpu_text.oracle_streams); the device's streams must be those bytes, route by route and mate by mate, with the same
counts, line counts, longest read and number of long reads.  A refused batch must carry the rule's smallest key in
``res.error`` / ``res.error_record`` and the rule's line counts in ``res.n_lines``.  tests/test_reader_rule_cpu.py holds
the same rule to the host's parser on the same texts.

Shapes: reads of 0 .. 25 bases on rows of 24, so a read of 25 takes the long-read kernel.  Plans: one single-end plan
without a UMI (names_universe.SCHEME_NO_UMI), TAKARAV3 paired (a UMI tag on every name), and -- where quality bytes are
arbitrary (case c) -- ``plan.single_adapter_plan``: one 3' adapter and nothing else, the one plan whose chain has no
QTrimOp, so no op looks at what the quality bytes are worth.  One engine pair per test, one slot, many submits.
"""
import contextlib
import ctypes as C
import functools
from typing import NamedTuple, Optional

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine
from cutseq_amd.synth import SynthBatch

import names_universe as nu
import reader_rule as rr
import util
from test_gpu_text import oracle_streams

pytestmark = pytest.mark.gpu

STRIDE = rr.STRIDE
TEXT_CAP = 3 * rr.SEG   # every text of cases a .. g but the longest names fits; the poison text fills it


# ---- plans -------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def plan_of(which: str):
    st = planmod.CutadaptConfig()
    st.min_length = 5  # reads of 0 .. 25: both the trimmed and the short route are filled
    if which == "single":
        return util.compile_plan(nu.SCHEME_NO_UMI, st, False)
    if which == "paired":
        tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True)
        assert tp.has_umi and tuple(s.encode() for s in tp.r1.name_suffixes) == nu.SUFFIXES[0]
        return tp
    tp = planmod.single_adapter_plan("AGATCGGAAGAGC", min_length=3)
    assert not any(isinstance(op, planmod.QTrimOp) for op in tp.r1.ops) and not tp.r1.name_suffixes
    return tp


# ---- the expectation ---------------------------------------------------------------------------------------------------


class Want(NamedTuple):
    key: Optional[tuple]   # the rule's smallest key, None: accepted
    n_lines: list
    streams: Optional[list]
    counts: Optional[list]
    n_long: Optional[list]
    max_len: int


def batch_from_bytes(rec1, rec2=None) -> SynthBatch:
    """util.batch_from_records for records whose bytes are no UTF-8 (case c): the same rows, filled from bytes."""
    def pack(recs):
        seq = np.zeros((len(recs), STRIDE + 4), dtype=np.uint8)
        qual = np.zeros((len(recs), STRIDE + 4), dtype=np.uint8)
        lens = np.zeros(len(recs), dtype=np.uint16)
        for i, (_, s, q) in enumerate(recs):
            seq[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
            qual[i, :len(q)] = np.frombuffer(q, dtype=np.uint8)
            lens[i] = len(s)
        return seq, qual, lens
    a = pack(rec1)
    b = pack(rec2) if rec2 is not None else (None, None, None)
    return SynthBatch(a[0], a[1], a[2], b[0], b[1], b[2])


def expect(tp, text1, text2, n, woven=False, raw_bytes=False) -> Want:
    n_lines = [rr.line_ends(text1), rr.line_ends(text2) if text2 is not None else 0]
    key = rr.batch_error(text1, text2 if tp.paired else None, n, woven)
    if key is not None:
        return Want(key, n_lines, None, None, None, 0)
    if n == 0:
        return Want(None, [0, 0], [[b"", b""]] * 3, [0, 0, 0], [0, 0], 0)
    rec1 = rr.parse(text1, n, woven, 0)
    rec2 = rr.parse(text1 if woven else text2, n, woven, 1 if woven else 0) if tp.paired else None
    batch = (batch_from_bytes if raw_bytes else util.batch_from_records)(rec1, rec2)
    names1, names2 = [r[0] for r in rec1], [r[0] for r in rec2] if rec2 is not None else None
    streams, counts, _ = oracle_streams(tp, batch, names1, names2)
    both = [rec1] + ([rec2] if rec2 is not None else [])
    n_long = [sum(1 for _, s, _ in recs if len(s) > STRIDE) for recs in both] + [0] * (2 - len(both))
    return Want(None, n_lines, streams, counts, n_long, max(len(s) for recs in both for _, s, _ in recs))


# ---- the device --------------------------------------------------------------------------------------------------------


class Got(NamedTuple):
    fields: dict            # every field of the cs_text_result
    streams: Optional[list]  # [route][mate]; None: refused, nothing to fetch


def _plain(value):
    return np.ctypeslib.as_array(value).tolist() if hasattr(value, "_length_") else value


class Rig:
    """One TrimEngine / TextEngine pair with one slot."""

    def __init__(self, tp, text_cap=TEXT_CAP, records=None, woven=False):
        self.tp, self.woven, self.cap = tp, woven, text_cap
        if records is None:  # what the poison text holds: a record in six bytes (an interleaved text: a pair in twelve)
            records = text_cap // (12 if woven else 6)
        self.stack = contextlib.ExitStack()
        eng = self.stack.enter_context(TrimEngine(tp, device=0, slots=0))
        self.te = self.stack.enter_context(textpath.TextEngine(eng, slots=1, max_text_bytes=text_cap, max_records=records,
                                                               stride=STRIDE, interleave_in=woven))
        self.L = self.te.L
        self.dev = []
        text, n = rr.poison(text_cap)
        self.poison_text, self.poison_n = text, (n - n % 2) // 2 if woven else n
        if woven and n % 2:  # (an interleaved text holds pairs: an even number of records)
            self.poison_text = rr.poison(text_cap - 6)[0]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.dev:
            self.L.cs_free_device(0, d)
        self.stack.close()

    def _finish(self) -> Got:
        res = abi.cs_text_result()
        capi.check(self.L.cs_text_wait(self.te._h, 0, C.byref(res)))  # (TextEngine.wait raises on a refused batch)
        fields = {name: _plain(getattr(res, name)) for name, _ in res._fields_}
        if res.error:
            return Got(fields, None)
        paired = self.tp.paired
        out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
        self.te.fetch(0, out[0], out[1] if paired else None)
        return Got(fields, textpath.split_routes(res, out, paired))

    def run(self, text1, text2, n) -> Got:
        two = self.tp.paired and not self.woven
        self.te.submit(0, text1, len(text1), text2 if two else None, len(text2) if two else 0, n)
        return self._finish()

    def device_buffers(self):
        """Two device buffers of the slot's text capacity (and the bytes an odd start takes)."""
        while len(self.dev) < 2:
            d = self.L.cs_alloc_device(0, self.cap + 8)
            assert d
            self.dev.append(d)
        return self.dev

    def run_device(self, text1, text2, n, shift) -> Got:
        """The same batch from texts that lie on the device, at ``base + shift``."""
        two = self.tp.paired and not self.woven
        at = []
        for d, text in zip(self.device_buffers(), (text1, text2) if two else (text1,)):
            assert len(text) + shift <= self.cap + 8
            if text:
                capi.check(self.L.cs_copy_to_device(0, d + shift, np.frombuffer(text, dtype=np.uint8).ctypes.data, len(text)))
            at.append(d + shift)
        self.te.submit_device(0, at[0], len(text1), at[1] if two else 0, len(text2) if two else 0, n)
        return self._finish()

    def poison(self):
        """The slot takes a batch that fills its text buffers with newline-dense text: what lies behind the next,
        shorter text is then two thirds line ends, and only the kernels' masks hide it."""
        got = self.run(self.poison_text, self.poison_text, self.poison_n)
        assert got.fields["error"] == 0 and sum(got.fields["route_count"]) == self.poison_n
        assert got.fields["n_lines"][0] == rr.line_ends(self.poison_text)


def check(got: Got, want: Want, what):
    f = got.fields
    assert f["n_lines"] == want.n_lines, (what, f["n_lines"], want.n_lines)
    if want.key is not None:
        assert (f["error_record"], f["error"]) == want.key, (what, f["error_record"], f["error"], want.key)
        assert got.streams is None and f["out_bytes"] == [0, 0], what
        return
    assert f["error"] == 0, (what, f["error"], f["error_record"])
    assert f["route_count"] == want.counts, (what, f["route_count"], want.counts)
    assert f["n_long"] == want.n_long and f["max_len"] == want.max_len, (what, f["n_long"], f["max_len"])
    for route in range(3):
        for m in range(2):
            assert got.streams[route][m] == want.streams[route][m], (what, textpath.ROUTES[route], m)


def mate_of(records):
    """Another mate for ``records`` as read: the same names (they match themselves), reads of its own."""
    return [(name,) + rr.read_of(1000 + 3 * i, (len(seq) * 5 + i) % (rr.MAX_LEN + 1)) for i, (name, seq, _) in enumerate(records)]


def texts_for(tp, case):
    """[(what, text1, text2)] of a single-text case for the plan: a paired plan gets a well-formed partner text, and the
    case's text goes through once as mate 1's and once as mate 2's."""
    if not tp.paired:
        return [(case.name, case.text, None)]
    recs = rr.parse(case.text, case.n)
    assert isinstance(recs, rr.Records), case.name
    other = rr.write(mate_of(recs))
    return [((case.name, "mate 1"), case.text, other), ((case.name, "mate 2"), other, case.text)]


def run_accepted(which, cases, poison, raw_bytes=False, text_cap=TEXT_CAP):
    tp = plan_of(which)
    with Rig(tp, text_cap=text_cap) as rig:
        for case in cases:
            for what, text1, text2 in texts_for(tp, case):
                want = expect(tp, text1, text2, case.n, raw_bytes=raw_bytes)
                assert want.key is None, (what, want.key)  # every one of these is accepted
                if poison:
                    rig.poison()
                check(rig.run(text1, text2, case.n), want, what)


# ---- a .. e: accepted texts --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["single", "paired"])
def test_line_ends_on_boundaries(which):
    """a.  The ``\\n`` of line k of a record at byte B + delta, B in {16, 64, 16384, 32768} (a dword's, a load's, a thread's
    and a block's edge all lie there), delta in {-2 .. 1}, ``\\n`` and ``\\r\\n``; a poison batch through the slot before
    every case."""
    cases = rr.boundary_cases()
    assert len(cases) == 4 * 4 * 4 * 2
    run_accepted(which, cases, poison=True)


@pytest.mark.parametrize("which", ["single", "paired"])
def test_text_ends_on_boundaries(which):
    """b.  Texts of 16384 s + d bytes, s in {1, 2}, d in [-17, 17], with and without the final newline (then the
    end of the text stands in: text_write_nl), and ``IIII\\r`` as the last line; poison before every case."""
    cases = rr.text_end_cases()
    assert len(cases) == 2 * (35 * 2 + 1)
    run_accepted(which, cases, poison=True)


def test_bytes_that_look_like_a_newline():
    """c.  0x00 0x09 0x0B 0x0D 0x7F 0x80 0x8A in headers and quality lines, in every byte lane of a dword, directly in front
    of and directly behind a real line end: all accepted, the bytes come out unchanged (but the one ``\\r`` a line end
    owns).  The plan without a QTrimOp: the quality bytes are arbitrary."""
    cases = rr.lookalike_cases()
    assert len(cases) == 7 * 4
    tp = plan_of("raw")
    with Rig(tp) as rig:
        for case in cases:
            want = expect(tp, case.text, None, case.n, raw_bytes=True)
            assert want.key is None
            rig.poison()
            check(rig.run(case.text, None, case.n), want, case.name)


@pytest.mark.parametrize("which", ["single", "paired"])
def test_restride_at_every_alignment_and_length(which):
    """d.  text_restride's funnel shift: the start of the sequence line (and with it of the quality line) at offset 0 .. 3
    mod 4, crossed with read lengths 0 1 2 3 4 5 23 24 25, lower case and IUPAC bases; the byte behind a read is
    its line end."""
    cases = rr.restride_cases()
    assert [c.n for c in cases] == [36, 36]
    run_accepted(which, cases, poison=True)


@pytest.mark.parametrize("which", ["single", "paired"])
def test_accepted_oddities(which):
    """e.  ``+name`` and ``+anything``, ``+\\r``, a header of ``@`` alone, an empty read, quality lines that begin with ``@``
    or ``+``, a sequence line that begins with ``@``, ``\\r`` on some lines only, ``\\r`` inside lines, bytes behind the
    last line end, a name of 65 535 bytes -- and one byte more is refused."""
    cases = rr.oddity_cases()
    assert len(cases) == 12
    run_accepted(which, cases, poison=False, text_cap=2 * TEXT_CAP)  # (the name of 65 535 bytes)
    tp = plan_of(which)
    long_name = rr.name_too_long_case()
    with Rig(tp, text_cap=2 * TEXT_CAP) as rig:
        text2 = rr.write(mate_of([(b"a",) + r[1:] for r in rr.good_records(3)])) if tp.paired else None
        want = expect(tp, long_name.text, text2, 3)
        assert want.key == (1, rr.MALFORMED)
        check(rig.run(long_name.text, text2, 3), want, long_name.name)


# ---- f: every defect at every place ------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def good_text(n, mate):
    return rr.write(rr.good_records(n, mate))


@pytest.mark.parametrize("where", ["single", "mate1", "mate2"])
def test_every_defect_at_every_place(where):
    """f.  Nine defects x records {0, 1, 255, 256, 257, 599} of 600, and in the last record of batches of 1, 255,
    256 and 257; single end, in mate 1 alone, in mate 2 alone.  After every refused batch the same engine takes the good
    batch of that size, and it comes out right."""
    tp = plan_of("single" if where == "single" else "paired")
    places = rr.defect_places()
    assert len(places) == 90
    good = {}
    with Rig(tp) as rig:
        for defect, n, r in places:
            bad = rr.defective(n, [(r, defect)], 2 if where == "mate2" else 1)
            text1, text2 = (good_text(n, 1), bad) if where == "mate2" else (bad, good_text(n, 2) if tp.paired else None)
            want = expect(tp, text1, text2, n)
            assert want.key == (r, rr.MALFORMED)
            check(rig.run(text1, text2, n), want, (defect, n, r))
            if n not in good:
                good[n] = expect(tp, good_text(n, 1), good_text(n, 2) if tp.paired else None, n)
                assert good[n].key is None
            check(rig.run(good_text(n, 1), good_text(n, 2) if tp.paired else None, n), good[n], ("good after", defect, n, r))
        # what TextEngine.wait makes of a key: the reader's error, with the record
        text1, text2 = rr.defective(600, [(257, "two-crs")]), good_text(600, 2) if tp.paired else None
        rig.te.submit(0, text1, len(text1), text2, len(text2) if tp.paired else 0, 600)
        with pytest.raises(textpath.TextFormatError) as e:
            rig.te.wait(0, first_record=1000)
        assert (e.value.code, e.value.record) == (abi.CS_TEXT_ERR_MALFORMED, 1257)


# ---- g: the key over two defects ---------------------------------------------------------------------------------------


def key_batches(n):
    """-> [(what, text1, text2)] of paired batches of ``n`` records, each refused (the rule says with what)."""
    good1, good2 = good_text(n, 1), good_text(n, 2)
    other = [(b"x%d" % i,) + r[1:] for i, r in enumerate(rr.good_records(n, 2))]

    def ids(differ, defects=()):
        recs = rr.good_records(n, 2)
        for r in differ:
            recs[r] = other[r]
        lines = [rr.record_lines(r) for r in recs]
        for r, name in defects:
            lines[r] = rr.DEFECTS[name](lines[r])
        return rr.join_lines(lines)

    out = [("malformed at 10 and 700 of mate 1", rr.defective(n, [(700, "empty-plus"), (10, "two-crs")]), good2),
           ("malformed at 700 and 10 of mate 2", good1, rr.defective(n, [(10, "quality-longer"), (700, "empty-header")], 2)),
           ("mate 1 bad at 700, mate 2 at 300", rr.defective(n, [(700, "empty-plus")]), rr.defective(n, [(300, "empty-header")], 2)),
           ("ids differ at 100, malformed at 400", good1, ids([100], [(400, "plus-other-byte")])),
           ("ids differ at 400, malformed at 100", good1, ids([400], [(100, "plus-other-byte")])),
           ("ids differ at 400, mate 1 malformed at 100", rr.defective(n, [(100, "sequence-longer")]), ids([400])),
           ("ids differ and malformed on record 256", rr.defective(n, [(256, "sequence-longer")]), ids([256])),
           ("ids differ in three blocks", good1, ids([700, 5, 300])),
           ("ids differ in three blocks, the other order", good1, ids([255, 256, 767])),
           ("ids differ in the last record", good1, ids([n - 1]))]
    for name, text in rr.line_count_texts(n, 2).items():
        out += [(f"mate 2 has {name} line ends", good1, text),
                (f"mate 2 has {name} line ends, mate 1 malformed at 0", rr.defective(n, [(0, "empty-plus")]), text),
                (f"mate 2 has {name} line ends, mate 1 malformed at 5", rr.defective(n, [(5, "empty-plus")]), text)]
    for name, text in rr.line_count_texts(n, 1).items():
        out += [(f"mate 1 has {name} line ends", text, good2),
                (f"mate 1 has {name} line ends, mate 2 malformed at 0", text, rr.defective(n, [(0, "two-crs")], 2)),
                (f"mate 1 has {name} line ends, mate 2 malformed at 5", text, rr.defective(n, [(5, "two-crs")], 2)),
                (f"mate 1 has {name} line ends, ids differ at 0", text, ids([0]))]
    return out


G_KEYS = [(10, rr.MALFORMED), (10, rr.MALFORMED), (300, rr.MALFORMED), (100, rr.IDS_DIFFER), (100, rr.MALFORMED),
          (100, rr.MALFORMED), (256, rr.MALFORMED), (5, rr.IDS_DIFFER), (255, rr.IDS_DIFFER), (rr.KEY_BATCH - 1, rr.IDS_DIFFER)]
G_LINE_KEYS = [(0, rr.LINE_COUNT), (0, rr.MALFORMED), (0, rr.LINE_COUNT)]


def test_the_key_over_two_defects():
    """g.  One key per batch: the smallest (record, code) over both mates and the three kernels that report -- written
    down here as constants, and the rule must say the same.  Line counts 4n - 2, 4n + 1 and 4n - 1 ending in a newline,
    per mate, alone and next to a malformed record of the other mate; single end too; no records at all."""
    n = rr.KEY_BATCH
    tp = plan_of("paired")
    batches = key_batches(n)
    keys = G_KEYS + G_LINE_KEYS * 3 + (G_LINE_KEYS + [(0, rr.LINE_COUNT)]) * 3
    assert len(batches) == len(keys) == 31
    with Rig(tp) as rig:
        for (what, text1, text2), key in zip(batches, keys):
            want = expect(tp, text1, text2, n)
            assert want.key == key, (what, want.key, key)
            check(rig.run(text1, text2, n), want, what)
        good = expect(tp, good_text(n, 1), good_text(n, 2), n)
        check(rig.run(good_text(n, 1), good_text(n, 2), n), good, "the good batch afterwards")
        empty = rig.run(b"", b"", 0)
        check(empty, expect(tp, b"", b"", 0), "no records")
        assert empty.streams == [[b"", b""]] * 3
    tp = plan_of("single")
    with Rig(tp) as rig:
        for case in rr.key_cases():
            want = expect(tp, case.text, None, case.n)
            assert (want.key is None) == (case.n == 0) and (case.n == 0 or want.key in ((10, rr.MALFORMED), (0, rr.LINE_COUNT)))
            check(rig.run(case.text, None, case.n), want, case.name)


# ---- h: more than 1024 segments ----------------------------------------------------------------------------------------


def test_more_than_1024_segments():
    """h.  text_scan_blocks walks the segment counts 1024 at a time with a carry: a text of exactly 1025 segments (16 MiB
    + 16 KiB, about 280 records with 60 000-byte headers that are their own ids, so the output carries them too) and one
    of exactly 1024.  (The expectation is the slow part: the record logic walks every header byte in Python.)"""
    tp = plan_of("single")
    with Rig(tp, text_cap=1025 * rr.SEG, records=320) as rig:
        for case in (rr.big_case(1025), rr.big_case(1024, blank=True), rr.big_case(1025, blank=True)):
            assert 270 < case.n < 300
            want = expect(tp, case.text, None, case.n)
            assert want.key is None and want.n_lines[0] == 4 * case.n
            check(rig.run(case.text, None, case.n), want, case.name)


# ---- i: the woven parser -----------------------------------------------------------------------------------------------


def test_the_woven_parser_follows_the_same_rule():
    """i.  text_parse_records_woven is a copy of text_parse_records kept apart on purpose; this holds the copy to the rule:
    a at B = 16384 built ON the interleaved text (the chosen line end is line 4(2r + m) + k of the one text, for a record
    of each mate; the writer asserts the place), e with the odd text as either mate, f with every defect at every place
    in mate 1 and in mate 2, and g -- through ``interleave_in``, the expectation the rule with ``woven=True``."""
    tp = plan_of("paired")
    with Rig(tp, text_cap=3 * TEXT_CAP, woven=True) as rig:  # (the name of 65 535 bytes, once per mate)
        placed = rr.woven_boundary_cases()
        assert len(placed) == 4 * 4 * 2 * 2
        for case in placed:
            want = expect(tp, case.text, None, case.n, woven=True)
            assert want.key is None, case.name
            rig.poison()
            check(rig.run(case.text, None, case.n), want, case.name)
        odd = rr.oddity_cases()
        assert len(odd) == 12
        for case in odd:
            for what, text1, text2 in texts_for(tp, case):
                (body1, tail1), (body2, tail2) = rr.split_tail(text1, case.n), rr.split_tail(text2, case.n)
                woven = rr.weave_lines(body1, body2, case.n) + tail1 + tail2  # (bytes behind the last line end stay there)
                want = expect(tp, woven, None, case.n, woven=True)
                assert want.key is None, what
                check(rig.run(woven, None, case.n), want, ("woven", what))
        for defect, n, r in rr.defect_places():
            for mate in (1, 2):
                bad = rr.defective(n, [(r, defect)], mate)
                woven = rr.weave_lines(bad, good_text(n, 2), n) if mate == 1 else rr.weave_lines(good_text(n, 1), bad, n)
                want = expect(tp, woven, None, n, woven=True)
                assert want.key == (r, rr.MALFORMED)
                check(rig.run(woven, None, n), want, ("woven", defect, n, r, mate))
        n = rr.KEY_BATCH
        batches = [b for b in key_batches(n) if "line ends" not in b[0]]
        assert len(batches) == len(G_KEYS)
        for (what, text1, text2), key in zip(batches, G_KEYS):
            woven = rr.weave_lines(text1, text2, n)
            want = expect(tp, woven, None, n, woven=True)
            assert want.key == key, (what, want.key)
            check(rig.run(woven, None, n), want, ("woven", what))
        good = rr.weave_lines(good_text(n, 1), good_text(n, 2), n)
        lines = good.split(b"\n")[:-1]
        counts = {"8n-2": b"\n".join(lines[:-1]), "8n+1": good + b"\n", "8n-1,ends-in-nl": b"\n".join(lines[:-1]) + b"\n",
                  "8n-1": good[:-1], "8n": good}
        for name, woven in counts.items():
            want = expect(tp, woven, None, n, woven=True)
            assert want.key == (None if name in ("8n-1", "8n") else (0, rr.LINE_COUNT)), name
            check(rig.run(woven, None, n), want, ("woven", name))
        # a bad line count next to a malformed record 0 / record 5 of either mate
        for r, m in ((0, 0), (0, 1), (5, 0), (5, 1)):
            texts = [good_text(n, 1), good_text(n, 2)]
            texts[m] = rr.defective(n, [(r, "empty-plus")], m + 1)
            woven = rr.weave_lines(texts[0], texts[1], n) + b"\n"
            want = expect(tp, woven, None, n, woven=True)
            # (no index: no record of the one text is looked at, so the malformed record 0 is not seen either)
            assert want.key == (0, rr.LINE_COUNT), (r, m)
            check(rig.run(woven, None, n), want, ("woven, 8n+1", r, m))


# ---- j: text already on the device -------------------------------------------------------------------------------------


def same(a: Got, b: Got, what):
    for name in a.fields:
        assert a.fields[name] == b.fields[name], (what, name, a.fields[name], b.fields[name])
    assert a.streams == b.streams, what


SHIFTS = (0, 1, 2, 3)


def test_device_text_single_end():
    """j.  cs_text_submit_device: the B = 16384 rows of a and all of b with s = 1, every text at device address base + 0,
    1, 2 and 3; result struct and streams equal cs_text_submit's field by field.  Poison before each."""
    tp = plan_of("single")
    cases = rr.boundary_cases((rr.SEG,)) + rr.text_end_cases((1,))
    assert len(cases) == 32 + 71
    with Rig(tp) as rig:
        for case in cases:
            rig.poison()
            host = rig.run(case.text, None, case.n)
            assert host.fields["error"] == 0 and sum(host.fields["route_count"]) == case.n
            for shift in SHIFTS:
                rig.poison()
                same(rig.run_device(case.text, None, case.n, shift), host, (case.name, shift))


@pytest.mark.parametrize("where", ["single", "mate1", "mate2"])
def test_device_text_refused_batches(where):
    """j.  All of f through cs_text_submit_device -- single end, the defect in mate 1 alone, in mate 2 alone -- every batch
    with its texts at base + 0, 1, 2 and 3: the same key and the same line counts as cs_text_submit gives, and the good
    batch of every size comes out the same afterwards."""
    tp = plan_of("single" if where == "single" else "paired")
    sizes = set()
    with Rig(tp) as rig:
        for defect, n, r in rr.defect_places():
            bad = rr.defective(n, [(r, defect)], 2 if where == "mate2" else 1)
            text1, text2 = (good_text(n, 1), bad) if where == "mate2" else (bad, good_text(n, 2) if tp.paired else None)
            host = rig.run(text1, text2, n)
            assert (host.fields["error_record"], host.fields["error"]) == (r, rr.MALFORMED)
            for shift in SHIFTS:
                same(rig.run_device(text1, text2, n, shift), host, (defect, n, r, shift))
            if n not in sizes:
                sizes.add(n)
                good = good_text(n, 1), good_text(n, 2) if tp.paired else None
                host = rig.run(good[0], good[1], n)
                assert host.fields["error"] == 0 and sum(host.fields["route_count"]) == n
                for shift in SHIFTS:
                    same(rig.run_device(good[0], good[1], n, shift), host, ("good after", defect, n, shift))
