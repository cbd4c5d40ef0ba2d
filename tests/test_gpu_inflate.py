"""The device's DEFLATE decoder (cs_inflate_bgzf), the k-th newline of device text and cs_text_submit_device.

The universe of well-formed blocks and the fixed corrupt list are those of bgzf_rule.py -- exactly what the host build
of the same decoder ran under the sanitizers (test_inflate_cpu.py); expected is what zlib says.  Every output region
lies between canary bytes, and a refused block sits between two good neighbours whose text must still be right.
"""
import ctypes as C

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import bgzf_rule
import util

pytestmark = pytest.mark.gpu
CANARY, GAP = 0xC7, 37  # (an odd gap: the regions start at every alignment)


class Device:
    """A cs_inflate handle and one device text buffer."""

    def __init__(self, max_comp, max_blocks, text_cap):
        self.L = capi.load()
        self.h = C.c_void_p()
        capi.check(self.L.cs_inflate_create(0, max_comp, max_blocks, C.byref(self.h)))
        self.cap = text_cap
        self.dtext = self.L.cs_alloc_device(0, max(text_cap, 1))
        assert self.dtext

    def close(self):
        self.L.cs_free_device(0, self.dtext)
        self.L.cs_inflate_destroy(self.h)

    def run(self, cases, first_comp_off=0, first_out_off=GAP):
        """``cases`` in one call -> (verdicts, lines, result, text regions [bytes], everything outside them is canary)."""
        comp = bytearray(b"\xEE" * first_comp_off)
        table = np.zeros(len(cases), dtype=abi.INFLATE_BLOCK_DTYPE)
        at = first_out_off
        for i, c in enumerate(cases):
            table[i] = (len(comp), at, len(c.payload), c.out_len, c.crc, 0)
            comp += c.payload + b"\xEE" * (i % 3)  # (payloads at every alignment, with bytes between that nobody may read)
            at += c.out_len + GAP
        total = at
        assert total <= self.cap
        host = np.full(total, CANARY, dtype=np.uint8)
        capi.check(self.L.cs_copy_to_device(0, self.dtext, host.ctypes.data, total))
        comp_arr = np.frombuffer(bytes(comp) or b"\0", dtype=np.uint8)
        lines = np.full(max(len(cases), 1), 0xFFFFFFFF, dtype=np.uint32)
        verdicts = np.full(max(len(cases), 1), -1, dtype=np.int32)
        res = abi.cs_inflate_result()
        capi.check(self.L.cs_inflate_bgzf(self.h, comp_arr.ctypes.data, len(comp), table.ctypes.data, len(cases), self.dtext,
                                          total, lines.ctypes.data, verdicts.ctypes.data, C.byref(res)))
        capi.check(self.L.cs_copy_to_host(0, host.ctypes.data, self.dtext, total))
        regions, outside = [], np.ones(total, dtype=bool)
        for row in table:
            lo, n = int(row["out_off"]), int(row["out_len"])
            regions.append(host[lo:lo + n].tobytes())
            outside[lo:lo + n] = False
        return verdicts[:len(cases)], lines[:len(cases)], res, regions, bool((host[outside] == CANARY).all())


@pytest.fixture(scope="module")
def dev():
    d = Device(8 << 20, 1024, 8 << 20)
    yield d
    d.close()


def test_universe_in_one_call(dev):
    cases = bgzf_rule.universe()
    verdicts, lines, res, regions, clean = dev.run([c for c, _ in cases])
    assert clean
    assert (res.verdict, res.block) == (abi.CS_INFLATE_OK, 0)
    for i, (c, text) in enumerate(cases):
        assert verdicts[i] == abi.CS_INFLATE_OK, (c.name, verdicts[i])
        assert regions[i] == text, c.name
        assert lines[i] == text.count(b"\n"), c.name


def test_corrupt_list_between_good_neighbours(dev):
    good_text = bgzf_rule.fastq_text(1500, seed=5)
    good = bgzf_rule.case_of("good", good_text, 6)
    corrupt = bgzf_rule.corrupt_cases()
    cases = [good]
    for c in corrupt:
        cases += [c, good]
    verdicts, lines, res, regions, clean = dev.run(cases)
    assert clean
    first_bad = None
    for i, c in enumerate(cases):
        ok, text = bgzf_rule.expected(c)
        assert (verdicts[i] == abi.CS_INFLATE_OK) == ok, (c.name, verdicts[i])
        if ok:
            assert regions[i] == text and lines[i] == text.count(b"\n"), c.name
        else:
            assert lines[i] == 0
            if first_bad is None:
                first_bad = i
    assert first_bad is not None and res.block == first_bad and res.verdict == verdicts[first_bad] != abi.CS_INFLATE_OK
    assert all(regions[i] == good_text for i in range(0, len(cases), 2))


def test_grid_and_offsets(dev):
    rng = np.random.default_rng(5)
    texts = [bgzf_rule.fastq_text(300, seed=100 + i) for i in range(600)]
    cases = [bgzf_rule.case_of(f"b{i}", t, int(rng.integers(0, 10))) for i, t in enumerate(texts)]
    verdicts, lines, res, regions, clean = dev.run(cases)  # more blocks than one wave per CU
    assert clean and res.verdict == abi.CS_INFLATE_OK and not verdicts.any()
    assert regions == texts and list(lines) == [t.count(b"\n") for t in texts]
    verdicts, lines, res, regions, clean = dev.run(cases[:1])
    assert clean and res.verdict == abi.CS_INFLATE_OK and regions == texts[:1] and lines[0] == texts[0].count(b"\n")
    verdicts, lines, res, regions, clean = dev.run([])
    assert clean and res.verdict == abi.CS_INFLATE_OK and regions == []
    verdicts, lines, res, regions, clean = dev.run(cases[:3], first_comp_off=1, first_out_off=1)  # odd on both sides
    assert clean and res.verdict == abi.CS_INFLATE_OK and regions == texts[:3]


def test_table_entries_outside_the_buffers_are_refused_before_the_launch(dev):
    L = dev.L
    c = bgzf_rule.case_of("x", b"ACGT\n" * 10, 6)
    comp = np.frombuffer(c.payload, dtype=np.uint8)
    lines, res = np.zeros(1, dtype=np.uint32), abi.cs_inflate_result()
    for row in ((1, 0, len(c.payload), c.out_len), (0, 0, len(c.payload) + 1, c.out_len), (0, 40, len(c.payload), c.out_len),
                (0, 2 ** 63, len(c.payload), c.out_len), (2 ** 64 - 1, 0, 2, c.out_len)):
        table = np.zeros(1, dtype=abi.INFLATE_BLOCK_DTYPE)
        table[0] = row + (c.crc, 0)
        rc = L.cs_inflate_bgzf(dev.h, comp.ctypes.data, len(c.payload), table.ctypes.data, 1, dev.dtext, c.out_len + 10,
                               lines.ctypes.data, None, C.byref(res))
        assert rc == abi.CS_ERR_ARG, row


def test_after_kth_newline_on_the_device(dev):
    L = dev.L
    text = bgzf_rule.fastq_text(70001, seed=9)  # more than four pieces of 16 KB, an odd length
    arr = np.frombuffer(text, dtype=np.uint8)
    capi.check(L.cs_copy_to_device(0, dev.dtext, arr.ctypes.data, len(text)))
    total = text.count(b"\n")
    ends = [i + 1 for i, c in enumerate(text) if c == 10]
    got = C.c_int64(-7)
    for k in (1, 2, total // 2, total - 1, total):
        capi.check(L.cs_dtext_after_kth_newline(0, dev.dtext, len(text), k, C.byref(got)))
        assert got.value == ends[k - 1], k
    for k, want in ((total + 1, -1), (10 ** 12, -1), (0, 0), (-3, 0)):
        capi.check(L.cs_dtext_after_kth_newline(0, dev.dtext, len(text), k, C.byref(got)))
        assert got.value == want, k
    capi.check(L.cs_dtext_after_kth_newline(0, dev.dtext + 3, 0, 1, C.byref(got)))
    assert got.value == -1
    off = ends[4]  # an odd start inside the buffer
    capi.check(L.cs_dtext_after_kth_newline(0, dev.dtext + off, len(text) - off, 3, C.byref(got)))
    assert got.value == ends[7] - off


def _fixture_text(n):
    rec1 = util.read_fastq_gz(util.GOLDEN / "fixture1k_R1.fq.gz")[:n]
    rec2 = util.read_fastq_gz(util.GOLDEN / "fixture1k_R2.fq.gz")[:n]
    def text(recs):
        return b"".join(b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + r[2] + b"\n" for r in recs)
    return text(rec1), text(rec2)


def _fetch_all(te, slot, paired):
    res = te.wait(slot)
    got, raw, count = te.routes(slot)
    out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
    te.fetch(slot, out[0], out[1] if paired else None)
    fields = {name: np.ctypeslib.as_array(getattr(res, name)).tolist() if hasattr(getattr(res, name), "_length_") else getattr(res, name)
              for name, _ in res._fields_}
    return fields, got.tolist(), raw.tolist(), count.tolist(), [out[m][:int(res.out_bytes[m])].tobytes() for m in range(2 if paired else 1)]


@pytest.mark.parametrize("paired,compress", [(False, False), (True, False), (True, True)])
def test_text_submit_device_equals_text_submit(dev, paired, compress):
    L = dev.L
    n = 300
    text1, text2 = _fixture_text(n)
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], planmod.CutadaptConfig(), paired)
    d1 = L.cs_alloc_device(0, len(text1))
    d2 = L.cs_alloc_device(0, len(text2))
    try:
        capi.check(L.cs_copy_to_device(0, d1, np.frombuffer(text1, dtype=np.uint8).ctypes.data, len(text1)))
        capi.check(L.cs_copy_to_device(0, d2, np.frombuffer(text2, dtype=np.uint8).ctypes.data, len(text2)))
        with TrimEngine(tp, device=0, slots=0) as eng:
            with textpath.TextEngine(eng, slots=2, max_text_bytes=max(len(text1), len(text2)) + 1024, max_records=n,
                                     stride=152, compress=compress) as te:
                te.submit(0, text1, len(text1), text2 if paired else None, len(text2) if paired else 0, n)
                want = _fetch_all(te, 0, paired)
                te.submit_device(1, d1, len(text1), d2 if paired else 0, len(text2) if paired else 0, n)
                got = _fetch_all(te, 1, paired)
    finally:
        L.cs_free_device(0, d1)
        L.cs_free_device(0, d2)
    assert got[0] == want[0] and got[1:4] == want[1:4]
    assert got[4] == want[4]
    assert sum(want[3][:3]) == n and want[0]["error"] == 0
