"""The 3' quality trimmer of every kernel against the plain rule (tests/qtrim_rule.py), on ENUMERATED inputs.

The scan kernel's wave walk (trim_kernel.hip.inc, the CS_OP_QTRIM branch: reads still alive below the dword of their
last base are served four at a time by groups of 16 lanes, running sums from a DPP prefix scan, "first strict maximum"
as a running max over packed (sum, position) keys), the same code in the resolve kernel with rows gathered by lane, and
the long-read kernel's scalar loop (long_kernel.hip.inc, quality_stop).  Path protected: cutadapt's
``QualityTrimmer(cutoff_front=0, cutoff_back=q)`` as the reference installs it (cutseq/run.py:415-417, 718-723).

Expected values are the rule's; the C oracle's results and statistics are compared as well.  tests/test_qtrim_cpu.py
shows without a GPU that the families reach every lane of a group in every role, and that oracle and rule agree.
A family is uploaded once and several plans run over it (Resident, tests/test_gpu_exhaustive.py); a plan is a PAIRED
plan whose mates run different (cut, cutoff) chains over the same rows, so mate 2's code is held too.
"""
import numpy as np
import pytest

import oracle
from cutseq_amd import abi
from cutseq_amd.engine import TrimEngine

import hostfmt
import qtrim_rule as R
import test_qtrim_cpu as T
from test_gpu_exhaustive import Resident, THREADS
from test_gpu_parity import stats_dict
from test_gpu_text import fastq_text, run_text_exposed

pytestmark = pytest.mark.gpu


class Held(Resident):
    """Resident rows whose runs also return the engine's statistics."""

    def __init__(self, rows):
        super().__init__(rows.seq, rows.qual, rows.lens)
        self.rows = rows

    def run(self, tp):
        with TrimEngine(tp, device=0, slots=0) as eng:
            eng.trim_device(self.r[0], self.r[1], self.n, self.stride, stream=self.handle)
            self.stream.synchronize()
            stats = eng.stats()
        return [o.cpu().numpy().view(abi.RESULT_DTYPE).reshape(-1) for o in self.out], stats

    def expect(self, tp):
        a1, n1, a2, n2 = tp.pack()
        params = tp.params()
        st1 = oracle.trim_mate(a1, n1, params, self.seq, self.qual, self.lens, threads=THREADS, out=self.want[0])[2]
        st2 = oracle.trim_mate(a2, n2, params, self.seq, self.qual, self.lens, threads=THREADS, out=self.want[1])[2]
        return self.want, (st1, st2)

    def check(self, tp, wants, what):
        """Device == rule (``wants``: per mate (records, quality-trimmed bases)), device == oracle, statistics too.
        -> the device's statistics."""
        got, stats = self.run(tp)
        ora, ora_stats = self.expect(tp)
        for mate in (0, 1):
            want, cut = wants[mate]
            T.differ(got[mate], want, self.rows, f"{what} mate {mate + 1}: device")
            T.differ(got[mate], ora[mate], self.rows, f"{what} mate {mate + 1}: device against the oracle")
            assert int(stats[mate].qualtrim_bp) == cut, (what, mate)
            assert int(stats[mate].out_bp) == int((want["stop"].astype(np.int64) - want["start"]).sum()), (what, mate)
            assert stats_dict(stats[mate]) == stats_dict(ora_stats[mate]), (what, mate)
        return stats


def run_scan(name, plans):
    rows = T.build(name)
    res = Held(rows)
    for m1, m2 in plans:
        tp = T.plan_of(T.chain(*m1), T.chain(*m2))
        res.check(tp, [T.rule_results(rows, m1), T.rule_results(rows, m2)], f"{name} (f, cutoff, base) = {m1} / {m2}")


@pytest.mark.parametrize("name,plans", T.SCAN_CASES, ids=[c[0] for c in T.SCAN_CASES])
def test_scan_kernel(name, plans):
    """F1..F5 through the scan kernel: the trimmer behind a cut of f bases, both mates."""
    run_scan(name, plans)


@pytest.mark.parametrize("name,plans", T.F6_CASES, ids=[c[0] for c in T.F6_CASES])
def test_scan_kernel_over_the_cutoff_range(name, plans):
    """F6: every accepted cutoff.  Before cs_plan_create clamped the cutoff, the packed key (sum << 11 | position in an
    int) overflowed: an MI355X kept 408 of 1 500 bases of ``I`` under -q 1000 (every row of F6's long inputs differed) and
    8 of 40 under -q 32767, where the rule keeps none."""
    run_scan(name, plans)


# ---- resolve kernel: [adapter, cut, trimmer] without the filter sends every non-empty read to the exact DP, the rest
# of its chain runs in the resolve kernel, rows gathered by lane

RESOLVE = ["F1a:0", "F1a:1", "F1a:2", "F1a:3", "F2B:0", "F2B:1", "F2B:2", "F2B:3", "F2A:1", "F3:0", "F3:1", "F3:2", "F3:3",
           "F4:0"]


def adapter_wants(rows, op, settings):
    end, flags = T.after_adapter(rows, op)
    return [T.rule_results(rows, m, end, flags) for m in settings], end


@pytest.mark.parametrize("name", RESOLVE)
def test_resolve_kernel(name):
    rows = T.build(name)
    if name.startswith("F4"):
        rows = R.Rows(*(np.ascontiguousarray(a[::4]) for a in rows[:3]), rows.f)
    rows = T.planted(rows, [T.ADAPTER])
    f = rows.f
    op = T.adapter_op(T.ADAPTER)
    settings = [(f, 20, 33), ((f + 1) % 4, 21, 33)]
    wants, end = adapter_wants(rows, op, settings)
    lens = rows.lens.astype(np.int64)
    assert 0 < int((end < lens).sum()) and np.array_equal(end[end < lens], lens[end < lens] - len(T.ADAPTER))
    tp = T.plan_of([op] + T.chain(*settings[0]), [op] + T.chain(*settings[1]), use_filter=False)
    stats = Held(rows).check(tp, wants, f"{name} behind an adapter, no filter")
    for mate in (0, 1):  # one exact DP per non-empty read: the whole chain behind it ran in the resolve kernel
        assert int(stats[mate].n_exact_dp) == int((lens > 0).sum())


@pytest.mark.parametrize("f", range(4))
def test_scan_kernel_with_deferred_lanes(f):
    """F3 behind an adapter WITH the filter: reads the filter cannot settle are deferred at the adapter op and are not
    ``on`` at the trimmer -- the alive set of a wave is sparse for a second reason."""
    near = T.NEAR
    copies = [near, near[:5] + "A" + near[6:], near[:6] + near[7:], near[:7] + "A" + near[7:]]
    rows = T.planted(T.build(f"F3:{f}"), copies)
    op = T.adapter_op(near, 0.1)
    assert op.k == 1
    settings = [(f, 20, 33), ((f + 1) % 4, 20, 33)]
    wants, end = adapter_wants(rows, op, settings)
    assert int((end < rows.lens).sum()) >= len(rows.lens) // 8
    tp = T.plan_of([op] + T.chain(*settings[0]), [op] + T.chain(*settings[1]), use_filter=True)
    stats = Held(rows).check(tp, wants, f"F3:{f} behind an adapter, filter on")
    for mate in (0, 1):
        assert 0 < int(stats[mate].n_exact_dp) < len(rows.lens)


# ---- long-read kernel: the same rows as FASTQ text at row stride 4

def check_long(rows, setting, what):
    tp = T.plan_of(T.chain(*setting))
    n = len(rows.lens)
    want, cut = T.rule_results(rows, setting)
    names = [b"q%d" % i for i in range(n)]
    text = fastq_text(names, rows.seq, rows.qual, rows.lens)
    records = []
    for i in range(n):
        k = int(rows.lens[i])
        route, rec = hostfmt.format_single(names[i], rows.seq[i, :k].tobytes(), rows.qual[i, :k].tobytes(), want[i], None, tp)
        assert route == 0
        records.append(rec)
    got = run_text_exposed(tp, text, None, n, 4)
    assert got.n_long[0] == int((rows.lens > 4).sum()) > 0, what
    assert got.counts == [n, 0, 0], what
    if got.streams[0][0] != b"".join(records):
        out = got.streams[0][0].split(b"\n")
        for i in range(n):
            assert out[4 * i:4 * i + 4] == records[i].split(b"\n")[:4], (what, i, want[i])
        raise AssertionError(what)
    ora, ora_st = T.oracle_results(rows, T.chain(*setting))
    T.differ(ora, want, rows, f"{what}: oracle")
    assert int(got.stats[0].qualtrim_bp) == cut and stats_dict(got.stats[0]) == stats_dict(ora_st), what


@pytest.mark.parametrize("name", ["F1a:1", "F2B:0", "F2B:1", "F2B:2", "F2B:3"])
def test_long_read_kernel(name):
    rows = T.build(name)
    check_long(rows, (rows.f, 20, 33), f"{name} as text, stride 4")


def test_long_read_kernel_over_the_cutoff_range():
    rows = T.build("F6short:0")
    for cutoff in R.F6_CUTOFFS:
        check_long(rows, (0, cutoff, 33), f"F6 short inputs as text, stride 4, cutoff {cutoff}")
