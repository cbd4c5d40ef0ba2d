"""cs_text_submit_bam on the GPU (bam_sizes / bam_expand in cutseq_amd/csrc/bam_kernels.hip.inc): BAM records in, and
everything the host reads back -- route streams, ``cs_text_result``, route sizes and counts, the info table -- byte for
byte what ``cs_text_submit`` gives for the FASTQ text tests/bam_rule.py renders from the same records.  The expected
value never comes from the BAM entry point.  Refused records end in their own code, message and record number, and the
engine serves a good batch afterwards; every refused input here has been through the same decisions under the
sanitizers on the host (tests/test_bam_cpu.py: ``corrupt()`` is one of its three case sets)."""
import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, rename, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import bam_rule
import util

pytestmark = pytest.mark.gpu

STRIDE = 160
TAKARAV3 = BUILDIN_ADAPTERS["TAKARAV3"]
MODES = ("single", "paired", "interleaved")
VARIANTS = {"plain": {}, "compress": dict(compress=True), "rename+info": dict(info=abi.CS_INFO_ON)}
TEMPLATES = {"single": "{id} renamed", "paired": "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}",
             "interleaved": "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}"}

_CACHE = {}


def plan_of(mode: str):
    if mode not in _CACHE:
        st = planmod.CutadaptConfig()
        _CACHE[mode] = util.compile_plan(TAKARAV3, st, mode != "single", untrimmed_requested=True)
    return _CACHE[mode]


def fixture_records(n=300):
    """Reads that do get trimmed: the head of the 1000-pair fixture as BAM records (the names keep their comments)."""
    if "fixture" not in _CACHE:
        pairs = []
        for m in (1, 2):
            recs = util.read_fastq_gz(str(util.GOLDEN / f"fixture1k_R{m}.fq.gz"), limit=n)
            pairs.append([bam_rule.Rec(name, seq, bytes(q - 33 for q in qual), tags=bam_rule.TAGS[i % 3]) for i, (name, seq, qual) in enumerate(recs)])
        _CACHE["fixture"] = tuple(pairs)
    return _CACHE["fixture"]


def batches():
    """[(label, mate 1's records, mate 2's records)]: the universe, and the fixture's reads."""
    if "batches" not in _CACHE:
        out = [(label, records, bam_rule.mate_of(records)) for label, records, _ in bam_rule.universe()
               if label in ("edges/65280",) or label.startswith("count/")]
        out.append(("fixture", *fixture_records()))
        _CACHE["batches"] = out
    return _CACHE["batches"]


def raw(records):
    """-> (record bytes, offsets as uint32 array) as the host walker hands them over."""
    blobs = [bam_rule.record_bytes(r) for r in records]
    offs = np.zeros(len(blobs) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in blobs])
    return b"".join(blobs), offs


def text(records) -> bytes:
    return b"".join(bam_rule.fastq_of_record(bam_rule.record_bytes(r), i) for i, r in enumerate(records))


def weave(a, b):
    return [r for pair in zip(a, b) for r in pair]


class Batch:
    """What one batch leaves behind, in plain values."""

    def __init__(self, te, info: bool, paired: bool):
        res = te.wait(0)
        self.result = {f: np.array(getattr(res, f)).tolist() if hasattr(getattr(res, f), "__len__") else int(getattr(res, f))
                       for f, _ in abi.cs_text_result._fields_}
        sizes, rawsizes, count = te.routes(0)
        self.sizes, self.raw_sizes, self.count = sizes.tolist(), rawsizes.tolist(), count.tolist()
        self.table = None
        if info:
            size, rawsize, rows = te.info(0)
            table = np.empty(max(size, 1), dtype=np.uint8)
            te.fetch_info(0, table)
            self.table = (table[:size].tobytes(), rawsize, rows)
        out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
        te.fetch(0, out[0], out[1] if paired and not te.interleave_out else None)
        self.streams = textpath.split_routes(sizes, out, paired)

    def __eq__(self, other):
        return self.__dict__ == other.__dict__


def submit_text(te, mode, r1, r2):
    if mode == "single":
        t1 = text(r1)
        te.submit(0, t1, len(t1), None, 0, len(r1))
    elif mode == "paired":
        t1, t2 = text(r1), text(r2)
        te.submit(0, t1, len(t1), t2, len(t2), len(r1))
    else:
        t1 = text(weave(r1, r2))
        te.submit(0, t1, len(t1), None, 0, len(r1))


def submit_bam(te, mode, r1, r2):
    if mode == "single":
        b1, o1 = raw(r1)
        te.submit_bam(0, b1, len(b1), o1, n_records=len(r1))
    elif mode == "paired":
        (b1, o1), (b2, o2) = raw(r1), raw(r2)
        te.submit_bam(0, b1, len(b1), o1, b2, len(b2), o2, n_records=len(r1))
    else:
        b1, o1 = raw(weave(r1, r2))
        te.submit_bam(0, b1, len(b1), o1, n_records=len(r1))


def engine(eng, mode, variant="plain", max_text=1 << 20, max_records=700, stride=STRIDE):
    kw = dict(VARIANTS[variant])
    if variant == "rename+info":
        kw["rename"] = rename.compile_template(TEMPLATES[mode], plan_of(mode))
    return textpath.TextEngine(eng, slots=1, max_text_bytes=max_text, max_records=max_records, stride=stride,
                               interleave_in=mode == "interleaved", **kw)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", MODES)
def test_records_give_what_their_text_gives(mode, variant):
    paired = mode != "single"
    trimmed = 0
    with TrimEngine(plan_of(mode), device=0, slots=0) as eng, engine(eng, mode, variant) as te:
        for label, r1, r2 in batches():
            submit_text(te, mode, r1, r2)
            want = Batch(te, variant == "rename+info", paired)
            submit_bam(te, mode, r1, r2)
            got = Batch(te, variant == "rename+info", paired)
            assert want.result["error"] == 0 and sum(want.count[:3]) == len(r1), label
            assert got.result == want.result, label
            assert (got.sizes, got.raw_sizes, got.count) == (want.sizes, want.raw_sizes, want.count), label
            assert got.streams == want.streams, label
            assert got.table == want.table, label
            if label == "fixture":
                trimmed = want.count[0]
    assert trimmed > 0  # (the comparison is not one of empty routes)


def test_an_empty_batch():
    with TrimEngine(plan_of("single"), device=0, slots=0) as eng, engine(eng, "single") as te:
        te.submit_bam(0, b"", 0, np.zeros(1, dtype=np.uint32), n_records=0)
        got = Batch(te, False, False)
        assert got.result["error"] == 0 and got.count[:3] == [0, 0, 0] and got.streams[0][0] == b""


def test_a_read_longer_than_the_rows():
    """70 001 bases, an odd length: the long-read kernel walks it from the expanded text, the last low nibble is no base."""
    rng = np.random.default_rng(5)
    long = bam_rule.Rec(b"long", bytes(rng.choice(list(b"ACGT"), 70001).tolist()), bytes(rng.integers(2, 41, 70001).tolist()))
    r1 = bam_rule.random_records(40, seed=4) + [long] + bam_rule.random_records(30, seed=6)
    with TrimEngine(plan_of("single"), device=0, slots=0) as eng, engine(eng, "single", max_text=1 << 19, max_records=128) as te:
        submit_text(te, "single", r1, None)
        want = Batch(te, False, False)
        submit_bam(te, "single", r1, None)
        got = Batch(te, False, False)
    assert want.result["n_long"][0] == 1 and want.result["max_len"] == 70001 and want.result["error"] == 0
    assert got == want


# ---------------------------------------------------------------- refusals

def offsets_of(stream: bytes):
    """The records of a stream whose chain is intact -> (bytes behind the header, offsets)."""
    at = base = bam_rule.header_size(stream)
    offs = [0]
    while at < len(stream):
        at += 4 + int.from_bytes(stream[at:at + 4], "little")
        offs.append(at - base)
    return stream[base:], np.array(offs, dtype=np.uint32)


RECORD_CASES = [c for c in bam_rule.corrupt() if c.where == "record"]


def test_refused_records_and_a_good_batch_afterwards():
    good = bam_rule.random_records(50, seed=12)
    assert len(RECORD_CASES) == 10 and {c.code for c in RECORD_CASES} == set(range(17, 23))
    with TrimEngine(plan_of("single"), device=0, slots=0) as eng, engine(eng, "single") as te:
        submit_text(te, "single", good, None)
        want = Batch(te, False, False)
        for c in RECORD_CASES:
            body, offs = offsets_of(c.stream)
            te.submit_bam(0, body, len(body), offs, n_records=len(offs) - 1)
            with pytest.raises(textpath.TextFormatError) as exc:
                te.wait(0, first_record=1000)
            assert (exc.value.code, exc.value.record) == (c.code, 1000 + c.record), c.label
            assert bam_rule.MESSAGES[c.code].format(n=1000 + c.record) in str(exc.value), c.label
            submit_bam(te, "single", good, None)
            assert Batch(te, False, False) == want, c.label


def test_a_batch_of_one_record_whose_parts_leave_its_block():
    """A text none of whose records counts any text (the host sizes it at 0 bytes): the record's own refusal, not an
    argument error; alone, as both records of a batch, and with the bam_first_record the CLI passes."""
    rec = bam_rule.random_records(1, seed=3)[0]
    bad = bam_rule.record_bytes(rec, l_seq=len(rec.seq) + 40)
    with TrimEngine(plan_of("single"), device=0, slots=0) as eng, engine(eng, "single") as te:
        for n in (1, 2):
            offs = np.arange(n + 1, dtype=np.uint32) * len(bad)
            te.submit_bam(0, bad * n, n * len(bad), offs, n_records=n)
            with pytest.raises(textpath.TextFormatError) as exc:
                te.wait(0, first_record=7, bam_first_record=40)
            assert (exc.value.code, exc.value.record) == (abi.CS_TEXT_ERR_BAM_OVERRUN, 40)
            assert bam_rule.MESSAGES[bam_rule.OVERRUN].format(n=40) in str(exc.value)
        good = bam_rule.random_records(3, seed=5)
        submit_text(te, "single", good, None)
        want = Batch(te, False, False)
        submit_bam(te, "single", good, None)
        assert Batch(te, False, False) == want


def test_a_refused_record_of_mate_2_and_of_an_interleaved_text():
    good = bam_rule.random_records(5, seed=77, lo=30, hi=40)  # (the records corrupt() builds on: the names pair up)
    case = next(c for c in RECORD_CASES if c.label == "aligned")
    body, offs = offsets_of(case.stream)
    g, go = raw(good)
    with TrimEngine(plan_of("paired"), device=0, slots=0) as eng:
        with engine(eng, "paired") as te:
            te.submit_bam(0, g, len(g), go, body, len(body), offs, n_records=5)
            with pytest.raises(textpath.TextFormatError) as exc:
                te.wait(0)
            assert exc.value.code == abi.CS_TEXT_ERR_BAM_ALIGNED | abi.CS_TEXT_ERR_BAM_MATE2 and exc.value.record == case.record
            assert "mate 2: only unaligned BAM is supported: record 4 is aligned" in str(exc.value)
        with engine(eng, "interleaved") as te:
            bad = bam_rule.record_bytes(good[3]._replace(flag=0))
            blobs = [bam_rule.record_bytes(r) for r in weave(good, good)]
            blobs[7] = bad  # pair 3's mate 2
            offs = np.zeros(11, dtype=np.uint32)
            offs[1:] = np.cumsum([len(b) for b in blobs])
            te.submit_bam(0, b"".join(blobs), int(offs[-1]), offs, n_records=5)
            with pytest.raises(textpath.TextFormatError) as exc:
                te.wait(0)
            assert (exc.value.code, exc.value.record) == (abi.CS_TEXT_ERR_BAM_ALIGNED, 7)


def test_arguments_refused_before_anything_is_launched():
    good = bam_rule.random_records(50, seed=12)
    body, offs = raw(good)
    with TrimEngine(plan_of("single"), device=0, slots=0) as eng, engine(eng, "single", max_text=1 << 13) as te:
        assert len(text(good)) > 1 << 13 > len(text(good[:20]))

        def refused(b, o, n, word):
            with pytest.raises(capi.CsError) as exc:
                te.submit_bam(0, b, len(b), o, n_records=n)
            assert exc.value.code == abi.CS_ERR_ARG and word in str(exc.value), str(exc.value)

        swapped = offs[:21].copy()
        swapped[[9, 10]] = swapped[[10, 9]]
        refused(body, swapped, 20, "not ascending")
        refused(body[:int(offs[20]) - 1], offs[:21], 20, "leaves")
        short = offs[:21].copy()
        short[20] = short[19] + 35
        refused(body, short, 20, "shorter than the 36 bytes")
        refused(body, offs, 50, "CUTSEQ_CHUNK_READS")  # 50 records: more text than the 8 KiB the slot takes
        with pytest.raises(capi.CsError):
            te.submit_bam(0, body, len(body), offs, body, len(body), offs, n_records=20)  # a single-end plan
        submit_text(te, "single", good[:20], None)
        want = Batch(te, False, False)
        submit_bam(te, "single", good[:20], None)
        assert Batch(te, False, False) == want
