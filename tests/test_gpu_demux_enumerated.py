"""CS_OP_DEMUX on ENUMERATED reads (tests/demux_rule.py): results, barcode indices and ``op_matched`` bit-equal, on every
read, to B independent oracle runs merged by the pinned rule -- an exact copy of a barcode wins, else the lowest index,
more than one claimant sets CS_F_AMBIGUOUS.  No tolerance, no read left out.  Both forms of the op (the look-up table
of every prefix; the candidates' own ops behind the host-built lists, which is also how the tables are built), coded and
raw tiles, behind a cut at every nibble offset, lower case under both case rules, the 3' form, and the long-read
kernel's two branches.  tests/test_demux_cpu.py shows on the oracle's side alone that these universes are not vacuous.
"""
import functools

import numpy as np
import pytest

import oracle
from cutseq_amd import abi, demux, plan as planmod
from cutseq_amd.engine import TrimEngine

import demux_rule as D

pytestmark = pytest.mark.gpu

THREADS = max(1, min(8, oracle.host_threads()))
LEFT, INS = D.RULES[0], D.TIES[0]


@functools.lru_cache(maxsize=None)
def reads(name: str, tg: bool = False):
    return D.reads_of(D.UNIVERSES[name], tg)


def codes_of(name: str, which: str, tg: bool = False):
    codes = D.UNIVERSES[name].sets()[which]
    return D.to_tg(codes) if tg else codes


@functools.lru_cache(maxsize=None)
def want(name: str, which: str, rule: int = LEFT, tie: int = INS, at_end: bool = False, tg: bool = False) -> D.Expected:
    """The expectation for a whole universe: computed once, shared by the forms that must meet it, never written to."""
    u = D.UNIVERSES[name]
    e = D.expect(codes_of(name, which, tg), u.rate, reads(name, tg), at_end=at_end, threads=THREADS, rule=rule, tie=tie)
    for a in (e.bc, e.res, e.matched, e.exact):
        a.setflags(write=False)
    return e


def device_run(tp: planmod.TrimPlan, batch, slot: int = 0):
    """One engine; launches of at most D.BLOCK reads -> (results, barcode indices, op_matched of chain slot ``slot``)."""
    seq, qual, lens = batch
    n = len(lens)
    res = np.empty(n, dtype=abi.RESULT_DTYPE)
    bc = np.empty(n, dtype=np.uint8)
    with TrimEngine(tp, device=0, slots=1, max_reads=min(n, D.BLOCK), max_stride=seq.shape[1]) as eng:
        for lo in range(0, n, D.BLOCK):
            hi = min(n, lo + D.BLOCK)
            eng.submit(0, seq[lo:hi], qual[lo:hi], lens[lo:hi], out=(res[lo:hi], None, None), bc=bc[lo:hi])
            eng.wait(0)
        st, _ = eng.stats()
    return res, bc, int(st.op_matched[slot])


def same(got, e: D.Expected, batch, what):
    res, bc, op_matched = got
    for name, a, b in (("barcode", bc, e.bc), ("result", res, e.res)):
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            i = int(bad[0])
            raise AssertionError(f"{what}: {name} differs on {len(bad)} of {len(a)} reads, first {batch[0][i, :batch[2][i]].tobytes()!r}: "
                                 f"got {a[i]}, want {b[i]} (claimants {np.flatnonzero(e.matched[:, i]).tolist()})")
    assert op_matched == e.assigned, what


# ---- the by-ops form, the root of every form

@pytest.mark.parametrize("tie", D.TIES)
@pytest.mark.parametrize("rule", D.RULES)
@pytest.mark.parametrize("which", ["crowded", "spread", "single"])
def test_by_ops_form_on_every_read_of_u1(which, rule, tie):
    u = D.U1
    tp = D.demux_chain(u.sets()[which], u.rate, "ops5", rule=rule, tie=tie)
    same(device_run(tp, reads("U1")), want("U1", which, rule, tie), reads("U1"), ("U1", which, rule, tie))


@pytest.mark.parametrize("name,tg", [("U2", False), ("U2", True), ("U3", False)])
def test_by_ops_form_where_the_lists_prune(name, tg):
    """m + k = 13 and 20: the lists are decided on nine bases of up to m + k; U2 once over {A, C, N} and once over
    {T, G, N} (every digit of the list index)."""
    u = D.UNIVERSES[name]
    tp = D.demux_chain(codes_of(name, "crowded", tg), u.rate, "ops5")
    assert not tp.demux.tabulated and u.span > 9
    same(device_run(tp, reads(name, tg)), want(name, "crowded", tg=tg), reads(name, tg), (name, tg))


# ---- the table form

@pytest.mark.parametrize("tie", D.TIES)
@pytest.mark.parametrize("rule", D.RULES)
@pytest.mark.parametrize("which", ["crowded", "spread", "single"])
def test_table_form_on_every_read_of_u1(which, rule, tie):
    """Every entry of the table (barcode, cut, the 0x4000 bit) is the expectation for its own prefix, and every read
    looked up through the scan kernel gets it."""
    u = D.U1
    e = want("U1", which, rule, tie)
    seq, _q, lens = reads("U1")
    tp = D.demux_chain(u.sets()[which], u.rate, "table", rule=rule, tie=tie)
    op = tp.demux
    op.table = demux.build_table(op, 0, rule, tie)
    assert op.table.dtype == np.uint16 and len(op.table) == u.reads == demux.table_entries(u.span)
    entry = op.table[D.table_index(seq, lens, u.span)]
    assert np.array_equal(entry & 0xFF, e.bc)
    assert np.array_equal((entry >> 8) & 0xF, e.res["start"])
    assert np.array_equal((entry & 0x4000) != 0, (e.res["flags"] & abi.CS_F_AMBIGUOUS) != 0)
    assert not (entry & 0xB000).any()
    same(device_run(tp, reads("U1")), e, reads("U1"), ("U1 table", which, rule, tie))


# ---- raw tiles

def never():
    """A BackAdapter that no read here can match (40 bases, all of them needed, no error allowed; never required) and
    whose IUPAC ``N`` leaves the plan uncoded (cs_plan_create: coded tiles only when every adapter base is A, C, G or
    T): the tiles keep their bytes."""
    return planmod.back("GATTACAGATTACANGATTACAGATTACAGATTACAGATTA", 0.0, 40, flag=abi.CS_F_ADAPTER3)


@pytest.mark.parametrize("form", ["ops5", "table"])
def test_raw_tiles(form):
    u = D.U1
    e = D.expect(u.crowded, u.rate, reads("U1"), threads=THREADS, behind=(never(),))
    assert np.array_equal(e.bc, want("U1", "crowded").bc) and not (e.res["flags"] & abi.CS_F_ADAPTER3).any()
    tp = D.demux_chain(u.crowded, u.rate, form, behind=(never(),))
    same(device_run(tp, reads("U1")), e, reads("U1"), ("raw", form))


# ---- behind a cut: the anchored end at every nibble offset of the coded tile

@pytest.mark.parametrize("form", ["ops5", "table"])
@pytest.mark.parametrize("c", range(9))
def test_behind_a_cut(c, form):
    u = D.U1
    batch = D.with_front(reads("U1"), c)
    e = D.expect(u.crowded, u.rate, batch, threads=THREADS, front_bases=c)
    base = want("U1", "crowded")
    assert np.array_equal(e.bc, base.bc) and np.array_equal(e.res["start"], base.res["start"] + c)
    tp = D.demux_chain(u.crowded, u.rate, form, front=(planmod.CutOp(c),) if c else ())
    same(device_run(tp, batch, slot=1 if c else 0), e, batch, ("cut", c, form))


# ---- bases behind the span

@pytest.mark.parametrize("form", ["ops5", "table"])
def test_bases_behind_the_span_change_nothing(form):
    u = D.U1
    batch = D.with_tail(reads("U1"), seed=7, most=24)
    assert len(batch[2]) == 5 ** u.span and set(batch[2].tolist()) == set(range(u.span + 1, u.span + 25))
    e = D.expect(u.crowded, u.rate, batch, threads=THREADS)
    full = reads("U1")[2] == u.span
    base = want("U1", "crowded")
    assert np.array_equal(e.bc, base.bc[full]) and np.array_equal(e.res["start"], base.res["start"][full])
    assert np.array_equal(e.res["flags"], base.res["flags"][full]) and np.array_equal(e.res["stop"], batch[2])
    same(device_run(D.demux_chain(u.crowded, u.rate, form), batch), e, batch, ("tail", form))


# ---- lower case

@pytest.mark.parametrize("form", ["ops5", "table"])
@pytest.mark.parametrize("case_rule", [D.FOLD, D.SENSITIVE])
def test_lower_case_under_both_case_rules(case_rule, form):
    """(Coded tiles with lower case take the exact re-coding.)"""
    u = D.U1
    batch = D.lower(reads("U1"))
    e = D.expect(u.crowded, u.rate, batch, case_rule=case_rule, threads=THREADS)
    base = want("U1", "crowded")
    if case_rule == D.FOLD:
        assert np.array_equal(e.bc, base.bc) and np.array_equal(e.res, base.res)
    else:  # no lower-case base equals a barcode's: only what k errors alone allow
        assert 0 <= e.assigned < base.assigned and not e.exact.any()
    same(device_run(D.demux_chain(u.crowded, u.rate, form, case_rule=case_rule), batch), e, batch, ("lower", case_rule, form))


# ---- the 3' form

@pytest.mark.parametrize("name", ["U1", "U2"])
def test_barcodes_at_the_3prime_end(name):
    """SuffixAdapter ops, the lists walked from the read's last base backwards."""
    u = D.UNIVERSES[name]
    e = want(name, "crowded", at_end=True)
    assert e.assigned > 0 and int((e.matched.sum(axis=0) > 1).sum()) >= 100 and e.exact.any()
    tp = D.demux_chain(u.crowded, u.rate, "ops3")
    assert tp.demux.at_end
    same(device_run(tp, reads(name)), e, reads(name), (name, "ops3"))


# ---- the long-read kernel

@pytest.mark.parametrize("form", ["table", "ops5", "ops3"])
def test_long_read_kernel_on_every_read_of_u1(form):
    """U1 as FASTQ text at row stride 4: every read over 4 nt takes the long-read kernel and its demultiplexing branch.
    Same text at the natural stride (the tile kernels, held to the oracle above): same route counts, the same bytes
    in every route, the same statistics.  (The method of test_long_read_walk_demultiplexes_like_the_rows.)"""
    from cutseq_amd import textpath
    from cutseq_amd.common import BarcodeConfig
    from test_gpu_parity import stats_dict

    u = D.U1
    codes, count, at_end = u.crowded, len(u.crowded), form == "ops3"
    scheme = (f"ACACGACGCTCTTCCGATCTNNNN>({codes[0]})AGATCGGAAGAGCACACGTC" if at_end else
              f"ACACGACGCTCTTCCGATCT({codes[0]})NNNN>AGATCGGAAGAGCACACGTC")
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    st.min_length = 0  # (a matched read of at most seven bases keeps none: it goes to its barcode's route all the same)
    st.demux_barcodes = list(codes)
    tp = planmod.compile_single(BarcodeConfig(scheme), st)
    tp.demux.by_ops = form != "table"
    assert tp.demux.tabulated == (form == "table") and tp.demux.at_end == at_end
    seq, _q, lens = reads("U1")
    n = len(lens)
    text1 = b"".join(b"@U:%d 1:N:0:X\n%s\n+\n%s\n" % (i, seq[i, :lens[i]].tobytes(), b"I" * int(lens[i])) for i in range(n))

    def run(stride):
        with TrimEngine(tp, device=0, slots=0) as eng:
            with textpath.TextEngine(eng, slots=1, max_text_bytes=len(text1) + 1024, max_records=n, stride=stride, bins=count) as te:
                te.submit(0, text1, len(text1), None, 0, n)
                res = te.wait(0)
                got, _, counts = te.routes(0)
                out = np.empty(max(int(res.out_bytes[0]), 1), dtype=np.uint8)
                te.fetch(0, out)
            return textpath.split_routes(got, [out], False), counts.tolist(), int(res.n_long[0]), stats_dict(eng.stats()[0])

    want_streams, want_counts, rows_long, want_stats = run(reads("U1")[0].shape[1])
    got_streams, got_counts, n_long, got_stats = run(4)
    assert rows_long == 0 and n_long == int((lens > 4).sum()) == n - 781
    assert sum(want_counts) == n and sum(want_counts[3:]) > 1000 and want_counts[2] > 0
    assert got_counts == want_counts
    for route in range(3 + count):
        assert got_streams[route][0] == want_streams[route][0], route
    assert got_stats == want_stats
