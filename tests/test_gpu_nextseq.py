"""--nextseq-trim (CS_OP_NEXTSEQ) and -Q in every kernel against the rule of tests/nextseq_rule.py.

The op lives in the kernels of the read-end modifiers (trim_kernel.hip.inc, FILT_ENDS, scan and resolve;
long_kernel.hip.inc / info_kernels.hip.inc, the ENDS walk).  The C oracle does not know it, so the expected records are
the rule alone (chains without an adapter op) or the rule layered over what the oracle leaves of the same chain WITHOUT
its tail -- NextSeq trimmer, quality trimmer, N trimmer --, the way tests/test_gpu_endtrim.py layers its two ops.
tests/test_nextseq_cpu.py builds the inputs and shows what they reach.
"""
import dataclasses
import functools

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod
from cutseq_amd.common import BUILDIN_ADAPTERS

import filters_rule
import hostfmt
import nextseq_rule as N
import qtrim_rule as R
import test_nextseq_cpu as T
import test_endtrim_cpu as TE
import test_qtrim_cpu as Q
import util
from test_gpu_endtrim import CODED_ADAPTER, MATCH_FLAGS, MIN_LENGTH, Held, plan_of
from test_gpu_filters import RAW_ADAPTER, run_engine, takara_batch
from test_gpu_filters_cli import run_cli
from test_gpu_text import fastq_text, run_text_exposed

pytestmark = pytest.mark.gpu


def stripped(tp):
    """The plan without the trailing NextSeqTrimOp / QTrimOp / NTrimOp of its chains (what the oracle can run), the tails."""
    chains, tails = [], []
    for mate in (tp.r1, tp.r2):
        if mate is None:
            chains.append(None)
            continue
        ops, tail = N.split_tail(mate.ops, planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp)
        chains.append(dataclasses.replace(mate, ops=ops))
        tails.append(tail)
    return dataclasses.replace(tp, r1=chains[0], r2=chains[1]), tails


def layered(tp, mates):
    """``mates``: (seq, qual, lens) per mate -> (E.Ends per mate, the oracle's records of the stripped plan)."""
    base, tails = stripped(tp)
    a1, n1, a2, n2 = base.pack()
    packed = ((a1, n1), (a2, n2))
    import oracle
    out, raw = [], []
    for m, (seq, qual, lens) in enumerate(mates):
        res = oracle.trim_mate(packed[m][0], packed[m][1], base.params(), seq, qual, lens, threads=Q.THREADS)[0]
        raw.append(res)
        out.append(N.apply_tail(seq, qual, res["start"], res["stop"], res["flags"], tails[m], tp.min_length))
    return out, raw


# ---- scan kernel -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def ns1_ends(name, setting):
    """The rule on an NS1 family, kept for the family's other cases."""
    return T.rule_ends(T.family(name), setting, min_length=MIN_LENGTH)


@pytest.mark.parametrize("name,plans", T.SCAN_CASES, ids=[c[0] for c in T.SCAN_CASES])
@pytest.mark.parametrize("adapter", [None, CODED_ADAPTER, RAW_ADAPTER], ids=["plain", "coded", "raw"])
def test_scan_kernel(name, plans, adapter):
    """NS1 behind a cut of f bases, both mates on chains of their own, every setting: the chain alone, and behind an
    adapter op that matches nothing -- a coded plan (fast-form tiles in the part without a ``g``, exact-form tiles behind
    it) and a raw one (its tiles fold case: the ``g`` must not count all the same)."""
    rows = T.family(name)
    held = Held(rows)
    front = [planmod.back(adapter, 0.0, len(adapter), flag=abi.CS_F_ADAPTER3)] if adapter else []
    for m1, m2 in plans if adapter is None else plans[:1]:
        tp = plan_of(front + T.chain(*m1), front + T.chain(*m2))
        wants = [ns1_ends(name, m) for m in (m1, m2)]
        assert all(w.cut > 0 for w in wants)
        if adapter:
            layer, raw = layered(tp, [(rows.seq, rows.qual, rows.lens)] * 2)
            assert all((r["flags"] & MATCH_FLAGS == 0).all() for r in raw)
            for m in (0, 1):
                assert np.array_equal(TE.records(layer[m]), TE.records(wants[m]))
        held.check(tp, wants, f"{name} (f, nextseq, front, back) = {m1} / {m2}, adapter {adapter}")


def test_scan_kernel_without_a_quality_trimmer_behind_the_op():
    rows = T.family("NS1:2")
    m1, m2 = (2, 20, 0, None), (1, 41, 0, None)
    wants = [T.rule_ends(rows, m, min_length=MIN_LENGTH) for m in (m1, m2)]
    Held(rows).check(plan_of(T.chain(*m1), T.chain(*m2)), wants, "NS1:2, the op ends the chain")


@pytest.mark.parametrize("name", T.DEEP_CASES)
def test_scan_kernel_deep(name):
    """The qtrim_rule families with a G for every base of delta +1: every dword depth, every lane of a group in every
    role, 1 to 64 walkers per tile, rows of 1020 to 1536 bases; a full row of G (everything goes) and of g (nothing)."""
    rows, plain = T.family(name)
    f = rows.f
    want = T.plain_ends(plain, f, MIN_LENGTH)
    again = T.rule_ends(rows, (f, R.CUTOFF, 0, None), min_length=MIN_LENGTH)
    assert np.array_equal(TE.records(want), TE.records(again)) and want.cut == again.cut > 0
    # mate 2: the quality trimmer behind the op, at the op's cutoff, reads the Gs' own quality bytes
    other = T.rule_ends(rows, (f, R.CUTOFF, 0, R.CUTOFF), min_length=MIN_LENGTH)
    tp = plan_of(T.chain(f, R.CUTOFF), T.chain(f, R.CUTOFF, 0, R.CUTOFF))
    held = Held(rows)
    if (want.flags & abi.CS_F_TOO_SHORT).any():  # (NSG2B, NSG4)
        held.check(tp, [want, other], name)
        return
    # (every row of NSG2A and NSG3 stays longer than MIN_LENGTH: Held.check without its demand that some read is too short)
    got, stats = held.run(tp)
    for mate, ends in enumerate((want, other)):
        Q.differ(got[mate], TE.records(ends), rows, f"{name} mate {mate + 1}: device")
        assert int(stats[mate].qualtrim_bp) == ends.cut > 0
        assert int(stats[mate].out_bp) == int((ends.stop - ends.start).sum()) > 0
        assert int(stats[mate].n_too_short) == int(((ends.flags & abi.CS_F_TOO_SHORT) != 0).sum())


# ---- resolve kernel --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["NS1:0", "NS1:3"])
def test_resolve_kernel(name):
    """[adapter, cut, NextSeq trimmer, trimmer] without the filter: every non-empty read goes to the exact DP and
    finishes its chain in the resolve kernel, rows gathered by lane."""
    rows = Q.planted(T.family(name), [Q.ADAPTER])
    f = rows.f
    op = Q.adapter_op(Q.ADAPTER)
    settings = [(f, 20, 0, 25), ((f + 1) % 4, 10, 15, 30)]
    end, flags = Q.after_adapter(rows, op)
    lens = rows.lens.astype(np.int64)
    assert 0 < int((end < lens).sum())
    wants = [T.rule_ends(rows, m, False, end, flags, MIN_LENGTH) for m in settings]
    tp = plan_of([op] + T.chain(*settings[0]), [op] + T.chain(*settings[1]), use_filter=False)
    layer, _raw = layered(tp, [(rows.seq, rows.qual, rows.lens)] * 2)
    for m in (0, 1):
        assert np.array_equal(TE.records(layer[m]), TE.records(wants[m]))
    _got, stats = Held(rows).check(tp, wants, f"{name} behind an adapter, no filter")
    for mate in (0, 1):
        assert int(stats[mate].n_exact_dp) == int((lens > 0).sum()) > 0


# ---- long-read kernel: the same rows as FASTQ text at row stride 4 ---------------------------------------------------

def test_long_read_kernel():
    rows = T.family("NS1:1")
    setting = (1, 20, 0, 25)
    tp = plan_of(T.chain(*setting), min_length=0)
    ends = T.rule_ends(rows, setting)
    want = TE.records(ends)
    n = len(rows.lens)
    names = [b"q%d" % i for i in range(n)]
    text = fastq_text(names, rows.seq, rows.qual, rows.lens)
    records = []
    for i in range(n):
        a, b = int(ends.start[i]), int(ends.stop[i])
        records.append(b"@" + names[i] + b"\n" + rows.seq[i, a:b].tobytes() + b"\n+\n" + rows.qual[i, a:b].tobytes() + b"\n")
    for i in range(0, n, 997):  # (the product's host formatter says the same of these records)
        k = int(rows.lens[i])
        route, rec = hostfmt.format_single(names[i], rows.seq[i, :k].tobytes(), rows.qual[i, :k].tobytes(), want[i], None, tp)
        assert route == 0 and rec == records[i]
    got = run_text_exposed(tp, text, None, n, 4)
    assert got.n_long[0] == int((rows.lens > 4).sum()) > n // 2
    assert got.counts == [n, 0, 0]
    if got.streams[0][0] != b"".join(records):
        out = got.streams[0][0].split(b"\n")
        for i in range(n):
            assert out[4 * i:4 * i + 4] == records[i].split(b"\n")[:4], (i, want[i])
        raise AssertionError("long-read kernel")
    assert int(got.stats[0].qualtrim_bp) == ends.cut > 0 and int(got.stats[0].out_bp) == int((ends.stop - ends.start).sum())


# ---- with the rest of the tail and the filters -----------------------------------------------------------------------

def dark_tails(batch, seed):
    """3' tails of 1 to 40 ``G`` of quality ``I`` on every third read, the same in ``g`` on every seventh, and low
    qualities at the 5' end of every fifth."""
    rng = np.random.default_rng(seed)
    for seq, qual, lens in ((batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2)):
        for i in range(batch.n):
            n = int(lens[i])
            if i % 3 == 0 or i % 7 == 0:
                k = min(int(rng.integers(1, 41)), n)
                seq[i, n - k:n] = ord("g") if i % 7 == 0 else N.G
                qual[i, n - k:n] = ord("I")
            if i % 5 == 0:
                qual[i, :min(int(rng.integers(1, 12)), n)] = rng.integers(33, 45)
    return batch


def takara_settings(nextseq, front, back, back_r2=None, trim_n=True):
    st = planmod.CutadaptConfig()
    st.nextseq_trim, st.min_quality_front, st.min_quality, st.trim_n = nextseq, front, back, trim_n
    if back_r2 is not None:
        st.min_quality_r2, st.min_quality_front_r2 = back_r2, 0
    return st


def test_with_the_rest_of_the_tail_and_the_filters():
    """One TAKARAV3 batch, --nextseq-trim 20 -q 15,25 --trim-n --max-n 0 -M 40 --max-ee 1: the other end ops, the
    filters, TooShort and the statistics see what the op left."""
    batch = dark_tails(takara_batch(4096, 70, 51, clip=True), 52)
    st = takara_settings(20, 15, 25)
    st.max_n, st.max_length, st.max_ee = 0.0, 40, 1.0
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True)
    off = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], takara_settings(None, 15, 25), True)
    mates = [(batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2)]
    wants, raw = layered(tp, mates)
    without, _raw = layered(off, mates)
    (g1, g2), xf, stats, counts = run_engine(tp, batch)
    shorter = 0
    for m, (seq, qual, _lens) in enumerate(mates):
        want = TE.records(wants[m])
        want["cap_off"], want["cap_len"] = raw[m]["cap_off"], raw[m]["cap_len"]
        bad = np.flatnonzero((g1, g2)[m] != want)
        assert bad.size == 0, (m, bad[:5], (g1, g2)[m][bad[:5]], want[bad[:5]])
        x = filters_rule.xflags(seq, qual, want, max_length=40, max_n=0.0, max_ee=1.0)
        assert np.array_equal(xf[m], x), (m, np.flatnonzero(xf[m] != x)[:5])
        assert counts[m] == {"too_many_n": int(((x & abi.CS_X_TOO_MANY_N) != 0).sum()),
                             "too_long": int(((x & abi.CS_X_TOO_LONG) != 0).sum()),
                             "too_many_ee": int(((x & abi.CS_X_TOO_MANY_EE) != 0).sum())}
        assert all(v > 0 for v in counts[m].values()) and (x == 0).any()
        assert int(stats[m].qualtrim_bp) == wants[m].cut > without[m].cut > 0
        assert int(stats[m].out_bp) == int((wants[m].stop - wants[m].start).sum()) > 0
        assert int(stats[m].n_too_short) == int(((wants[m].flags & abi.CS_F_TOO_SHORT) != 0).sum()) > 0
        shorter += int(((wants[m].stop - wants[m].start) < (without[m].stop - without[m].start)).sum())
    assert shorter > 1000


# ---- the command line ------------------------------------------------------------------------------------------------

def expected_files(tp, batch, names):
    mates = [(batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2)]
    wants, raw = layered(tp, mates)
    res = []
    for m in range(2):
        r = TE.records(wants[m])
        r["cap_off"], r["cap_len"] = raw[m]["cap_off"], raw[m]["cap_len"]
        res.append(r)
    recs = util.format_batch(tp, batch, names, names, res[0], None, res[1])
    streams = [[b"", b""] for _ in range(3)]
    for route, r1, r2 in recs:
        streams[route][0] += r1
        streams[route][1] += r2
    return streams, wants, res, recs


def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    """TAKARAV3 pairs, --nextseq-trim 20 -q 15,10 -Q 25 --trim-n: the text path (with --info-file) and the record path
    write the same files, the ones the rule gives; the report's quality-trimmed bases are the rule's sums of both
    trimmers, -Q makes the two mates' differ; the table's no-match rows carry the final read."""
    batch = dark_tails(takara_batch(2000, 150, 61, clip=True), 62)
    names = [b"pair%d" % i for i in range(batch.n)]
    paths = [str(tmp_path / f"in{m}.fq.gz") for m in (1, 2)]
    util.write_fastq(paths[0], names, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(paths[1], names, batch.seq2, batch.qual2, batch.len2)
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], takara_settings(20, 15, 10, back_r2=25), True)
    assert tp.r1.ops[-2] == planmod.QTrimOp(10, 33, cutoff_front=15) and tp.r2.ops[-2] == planmod.QTrimOp(25, 33, cutoff_front=0)
    streams, wants, res, recs = expected_files(tp, batch, names)
    assert streams[0][0].count(b"\n") > 4 * 500 and streams[1][0].count(b"\n") > 4 * 100
    options = ["--nextseq-trim", "20", "-q", "15,10", "-Q", "25", "--trim-n"]
    info = str(tmp_path / "info.tsv")
    monkeypatch.delenv("CUTSEQ_TEXT_PATH", raising=False)
    text, rep_text, _ = run_cli(tmp_path, capsys, "text", paths, options + ["--info-file", info])
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    host, rep_host, _ = run_cli(tmp_path, capsys, "host", paths, options)
    monkeypatch.delenv("CUTSEQ_TEXT_PATH")
    assert text == host
    for kind, route in (("trimmed", 0), ("short", 1)):
        for m in (1, 2):
            assert text[(kind, m)] == streams[route][m - 1], (kind, m)
    for rep in (rep_text, rep_host):
        bp = rep["basepair_counts"]
        assert bp["quality_trimmed_read1"] == wants[0].cut and bp["quality_trimmed_read2"] == wants[1].cut
        assert wants[0].cut > 0 and wants[1].cut > 0 and wants[0].cut != wants[1].cut
        assert bp["output_read1"] == sum(len(r1.split(b"\n")[1]) for rt, r1, _r2 in recs if rt == 0) > 0
    # the table: a read without an adapter match has one row of name, -1, final sequence, final qualities
    rows = [line.split(b"\t") for line in open(info, "rb").read().split(b"\n") if line]
    none = [r for r in rows if r[1] == b"-1"]
    want_none = []
    dark = 0
    for i, (_rt, r1, _r2) in enumerate(recs):
        if int(res[0]["flags"][i]) & MATCH_FLAGS == 0:
            name, seq, _plus, qual = r1.split(b"\n")[:4]
            want_none.append([name[1:], b"-1", seq, qual, b""])
            last = int(res[0]["stop"][i])
            dark += int(i % 3 == 0 and i % 7 != 0 and int(res[0]["start"][i]) < last < int(batch.len1[i]) and batch.seq1[i, last] == N.G)
    assert none == want_none and len(none) > 100 and dark > 10
