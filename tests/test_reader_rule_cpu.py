"""tests/reader_rule.py held to the host's parser (no GPU): every single-text case of the rule's universe through
csh_fastq_parse of cutseq_host.c -- the same rule in C, what the CUTSEQ_TEXT_PATH=0 path reads with -- and the rule's
writers through the rule itself.  The device is held to the rule in tests/test_gpu_text_structure.py: rule == host C here,
device == rule there.

The host parser's domain: reads no longer than its rows (28 here, so the reads of 25 are inside), names of any length
(the one case with a name of 65 536 bytes is not in the universe), and a text that HAS its line ends -- csh_fastq_parse is
handed blocks that csh_fastq_count has cut, it has no line count to refuse.  For the texts the rule refuses with
LINE_COUNT the twin is therefore the cutter: it must not find ``n`` records that fill the text.
"""
import ctypes as C

import numpy as np

from cutseq_amd import fastq

import reader_rule as rr

HOST_STRIDE = 28


def host_parse(text: bytes, n: int):
    """csh_fastq_parse on a whole text -> Records, or the index of the first record it refuses."""
    L = fastq._lib()
    buf = np.frombuffer(text if text else b"\0", dtype=np.uint8)
    rows = max(n, 1)
    seq = np.empty((rows, HOST_STRIDE), dtype=np.uint8)
    qual = np.empty((rows, HOST_STRIDE), dtype=np.uint8)
    lens = np.zeros(rows, dtype=np.uint16)
    name_off = np.zeros(rows, dtype=np.int64)
    name_len = np.zeros(rows, dtype=np.int32)
    rc = L.csh_fastq_parse(buf.ctypes.data, len(text), n, HOST_STRIDE, seq.ctypes.data, qual.ctypes.data, lens.ctypes.data,
                           name_off.ctypes.data, name_len.ctypes.data)
    if rc < 0:
        return -int(rc) - 1
    out = rr.Records()
    for i in range(n):
        k, at = int(lens[i]), int(name_off[i])
        out.append((text[at:at + int(name_len[i])], seq[i, :k].tobytes(), qual[i, :k].tobytes()))
    return out


def host_cuts(text: bytes, n: int) -> bool:
    """csh_fastq_count at the end of a file: does it find ``n`` complete records that fill the text?"""
    L = fastq._lib()
    buf = np.frombuffer(text if text else b"\0", dtype=np.uint8)
    consumed, longest = C.c_int64(0), C.c_int32(0)
    got = L.csh_fastq_count(buf.ctypes.data, len(text), n, 1, C.byref(consumed), C.byref(longest))
    return int(got) == n and int(consumed.value) == len(text)


def test_the_rule_and_the_host_parser_agree_on_the_universe():
    """Verdict and first bad record of every case; the records of every accepted one.  The universe's size and its
    refusals are constants: a universe that shrinks fails here."""
    cases = rr.universe()
    assert len(cases) == 128 + 142 + 28 + 2 + 12 + 90 + 12 + 2 == 416
    refused = line_count = 0
    per_group = {}
    for c in cases:
        want = rr.parse(c.text, c.n, c.woven)
        per_group[c.name[0]] = per_group.get(c.name[0], 0) + 1
        if not isinstance(want, rr.Records):
            refused += 1
            assert rr.batch_error(c.text, None, c.n) == min(want), c.name
        if want == {(0, rr.LINE_COUNT)}:
            line_count += 1
            assert not host_cuts(c.text, c.n), c.name
            continue
        got = host_parse(c.text, c.n)
        if isinstance(want, rr.Records):
            assert isinstance(got, rr.Records), (c.name, got)
            assert got == want, c.name
            assert len(want) == c.n and max([len(s) for _, s, _ in want] + [0]) <= rr.MAX_LEN
            # the cutter hands on what the rule looks at: the text up to its 4n-th line end (one case has bytes behind it)
            body, tail = rr.split_tail(c.text, c.n)
            assert host_cuts(body, c.n) or not c.n, c.name
            assert bool(tail) == (c.name == "e:bytes-behind-the-last-line-end") and (not tail or not host_cuts(c.text, c.n))
        else:
            assert not isinstance(got, rr.Records), c.name
            assert min(want) == (got, rr.MALFORMED), (c.name, got, min(want))
    assert per_group == {"a": 128, "b": 142, "c": 28, "d": 2, "e": 12, "f": 90, "g": 12, "h": 2}
    assert (refused, line_count) == (101, 10)


def test_the_defects_are_refused_where_they_stand_and_nowhere_else():
    """Case f by its own construction: the key is the defect's record, whichever of the nine it is; the text without the
    defect is accepted."""
    places = rr.defect_places()
    assert len(places) == 9 * (6 + 4)
    for (defect, n, r), case in zip(places, rr.defect_cases()):
        assert rr.parse(case.text, case.n) == {(r, rr.MALFORMED)}, case.name
    for n in (rr.DEFECT_BATCH,) + rr.DEFECT_SIZES:
        good = rr.parse(rr.defective(n, []), n)
        assert good == rr.good_records(n) and isinstance(good, rr.Records)
    assert {len(s) for _, s, _ in rr.good_records(rr.DEFECT_BATCH)} == set(range(rr.MAX_LEN + 1))


def test_round_trip_through_the_writer():
    """records -> writer -> parse -> the same records, for both line ends, with and without the final newline; woven
    texts give each mate its own."""
    r1, r2 = rr.good_records(70, 1), rr.good_records(70, 2)
    for eol in (rr.LF, rr.CRLF):
        for final in (True, False):
            text = rr.write(r1, eol, final)
            got = rr.parse(text, len(r1))
            assert isinstance(got, rr.Records) and got == r1, (eol, final)
            assert rr.line_ends(text) == 4 * len(r1) - (0 if final else 1)
            assert rr.parse(text, len(r1) + 1) == {(0, rr.LINE_COUNT)} == rr.parse(text, len(r1) - 1)
            assert host_parse(text, len(r1)) == r1
    woven = rr.weave_lines(rr.write(r1), rr.write(r2), 70)
    assert rr.parse(woven, 70, woven=True, mate=0) == r1 and rr.parse(woven, 70, woven=True, mate=1) == r2
    assert rr.parse(woven[:-1], 70, woven=True, mate=1) == r2 and rr.parse(woven, 140) != r1
    assert rr.parse(woven + b"\n", 70, woven=True) == {(0, rr.LINE_COUNT)}
    assert rr.parse(b"", 0) == [] and rr.parse(b"", 1) == {(0, rr.LINE_COUNT)}


def test_the_writers_put_things_where_they_say():
    recs = rr.good_records(5)
    cases = rr.woven_boundary_cases()
    assert len(cases) == 4 * 4 * 2 * 2
    for c in cases:  # (place_woven asserts the place; here: both mates' records come back, and the names pair up)
        r1, r2 = rr.parse(c.text, 3, woven=True, mate=0), rr.parse(c.text, 3, woven=True, mate=1)
        assert isinstance(r1, rr.Records) and isinstance(r2, rr.Records) and rr.batch_error(c.text, None, 3, woven=True) is None
    for eol in (rr.LF, rr.CRLF):
        for r, k, at in ((0, 0, 16), (2, 3, 4096), (4, 1, rr.SEG + 1)):
            text, written = rr.place(recs, r, k, at, eol)
            assert text[at] == 10 and rr.line_ends(text[:at]) == 4 * r + k and rr.parse(text, 5) == written
            if eol == rr.CRLF:
                assert text[at - 1] == 13
        text, written = rr.sized(recs, 3 * rr.SEG - 5, eol, False)
        assert len(text) == 3 * rr.SEG - 5 and rr.parse(text, 5) == written
    for size in (6, 7, 11, 12, 4096 + 5):
        text, n = rr.poison(size)
        assert len(text) == size and n == size // 6 and isinstance(rr.parse(text, n), rr.Records)
        assert host_parse(text, n) == rr.parse(text, n)
    text, n = rr.poison(6 * 4096)
    assert rr.line_ends(text) * 3 == 2 * len(text)  # newline-dense: two of every three bytes


def test_the_batch_key_is_the_smallest_over_both_mates():
    """Case g on the rule alone (the device runs the same texts): one key per batch."""
    n = rr.KEY_BATCH
    good1, good2 = rr.write(rr.good_records(n, 1)), rr.write(rr.good_records(n, 2))
    assert rr.batch_error(good1, good2, n) is None and rr.batch_error(good1, None, n) is None
    bad = lambda mate, *defects: rr.defective(n, list(defects), mate)
    assert rr.batch_error(bad(1, (700, "empty-plus"), (10, "two-crs")), good2, n) == (10, rr.MALFORMED)
    assert rr.batch_error(bad(1, (700, "empty-plus")), bad(2, (300, "empty-header")), n) == (300, rr.MALFORMED)
    other = [(b"x%d" % i,) + r[1:] for i, r in enumerate(rr.good_records(n, 2))]

    def ids(*differ):
        recs = rr.good_records(n, 2)
        for r in differ:
            recs[r] = other[r]
        return [rr.record_lines(r) for r in recs]

    def with_defect(lines, r, name):
        lines = list(lines)
        lines[r] = rr.DEFECTS[name](lines[r])
        return rr.join_lines(lines)

    assert rr.batch_error(good1, rr.join_lines(ids(5, 300, 700)), n) == (5, rr.IDS_DIFFER)
    assert rr.batch_error(good1, with_defect(ids(100), 400, "plus-other-byte"), n) == (100, rr.IDS_DIFFER)
    assert rr.batch_error(good1, with_defect(ids(400), 100, "plus-other-byte"), n) == (100, rr.MALFORMED)
    assert rr.batch_error(bad(1, (100, "sequence-longer")), rr.join_lines(ids(100)), n) == (100, rr.MALFORMED)
    for text in rr.line_count_texts(n, 2).values():
        assert rr.batch_error(good1, text, n) == (0, rr.LINE_COUNT)
        assert rr.batch_error(bad(1, (0, "empty-plus")), text, n) == (0, rr.MALFORMED)
        assert rr.batch_error(bad(1, (5, "empty-plus")), text, n) == (0, rr.LINE_COUNT)
        assert rr.batch_error(text, rr.join_lines(ids(0)), n) == (0, rr.LINE_COUNT)  # (no index: no id is compared)
    woven = rr.weave_lines(bad(1, (700, "empty-plus")), bad(2, (300, "empty-header")), n)
    assert rr.batch_error(woven, None, n, woven=True) == (300, rr.MALFORMED)
    assert rr.batch_error(rr.weave_lines(good1, rr.join_lines(ids(256)), n), None, n, woven=True) == (256, rr.IDS_DIFFER)
    assert rr.batch_error(b"", b"", 0) is None


def test_names_match_is_the_pair_check_of_the_name_universe():
    """names_match on names as read == names_universe.pair_matches on names as written (tests/test_names_cpu.py holds that
    one to the host); spot checks of the three clauses."""
    import names_universe as nu
    matching, mismatching = nu.pools()
    for pool, want in ((matching[::7], True), (mismatching[::3], False)):
        for a, b in pool:
            assert rr.names_match(nu.as_read(a), nu.as_read(b)) == want, (a, b)
    assert rr.names_match(b"r1 x", b"r1 y") and rr.names_match(b"r1\tx", b"r1")
    assert rr.names_match(b"r/1", b"r/2") and rr.names_match(b"r3", b"r1") and not rr.names_match(b"r1", b"r")
    assert not rr.names_match(b"r1\vx", b"r1\vy")
