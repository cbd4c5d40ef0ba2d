"""-q FRONT,BACK and --trim-n in every kernel against the rules of tests/endtrim_rule.py.

The front walk of the quality trimmer and the CS_OP_NTRIM op live in kernels of their own (trim_kernel.hip.inc,
FILT_ENDS, scan and resolve; long_kernel.hip.inc / info_kernels.hip.inc, the ENDS walk).  The C oracle knows neither, so
the expected records are the rules applied to what the oracle leaves of the same chain WITHOUT its trailing quality
trimmer / N trimmer (chains without an adapter op: the rules alone) -- the way tests/test_gpu_filters.py layers the
filters over the oracle.  tests/test_endtrim_cpu.py builds the inputs and shows what they reach.
"""
import dataclasses
import json

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, run as cli
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import endtrim_rule as E
import filters_rule
import hostfmt
import qtrim_rule as R
import test_endtrim_cpu as T
import test_qtrim_cpu as Q
import util
from test_gpu_exhaustive import Resident
from test_gpu_filters import RAW_ADAPTER, run_engine, takara_batch
from test_gpu_filters_cli import gunzip, run_cli
from test_gpu_text import fastq_text, run_text_exposed

pytestmark = pytest.mark.gpu

MIN_LENGTH = 2  # (of the hand-made plans: TooShort has to see the narrowed interval too)
CODED_ADAPTER = "GTGTGTGTGG"  # longer than any N-family read and its min_overlap: it matches nothing
MATCH_FLAGS = abi.CS_F_ADAPTER5 | abi.CS_F_ADAPTER3 | abi.CS_F_INLINE | abi.CS_F_POLY


def plan_of(ops1, ops2=None, use_filter=True, min_length=MIN_LENGTH):
    return planmod.TrimPlan(r1=planmod.MateChain(list(ops1)), r2=planmod.MateChain(list(ops2)) if ops2 is not None else None,
                            has_umi=False, min_length=min_length, untrimmed_filter=False, use_filter=use_filter)


class Held(Resident):
    def __init__(self, rows):
        super().__init__(rows.seq, rows.qual, rows.lens)
        self.rows = rows

    def run(self, tp):
        with TrimEngine(tp, device=0, slots=0) as eng:
            eng.trim_device(self.r[0], self.r[1], self.n, self.stride, stream=self.handle)
            self.stream.synchronize()
            stats = eng.stats()
        return [o.cpu().numpy().view(abi.RESULT_DTYPE).reshape(-1).copy() for o in self.out], stats

    def check(self, tp, wants, what):
        """Device == rule: records (start, stop, flags), qualtrim_bp, out_bp, n_too_short.  ``wants``: an E.Ends per mate."""
        got, stats = self.run(tp)
        for mate in (0, 1):
            ends = wants[mate]
            Q.differ(got[mate], T.records(ends), self.rows, f"{what} mate {mate + 1}: device")
            assert int(stats[mate].qualtrim_bp) == ends.cut, (what, mate)
            assert int(stats[mate].out_bp) == int((ends.stop - ends.start).sum()), (what, mate)
            assert int(stats[mate].n_too_short) == int(((ends.flags & abi.CS_F_TOO_SHORT) != 0).sum()) > 0, (what, mate)
            assert int(stats[mate].n_reads) == self.n
        return got, stats


def run_plain(name, plans):
    rows = T.family(name)
    held = Held(rows)
    for m1, m2 in plans:
        tp = plan_of(T.chain(*m1), T.chain(*m2))
        wants = [T.rule_ends(rows, m, min_length=MIN_LENGTH) for m in (m1, m2)]
        got, _stats = held.check(tp, wants, f"{name} (f, front, back) = {m1} / {m2}")
        for m, mate in ((m1, 0), (m2, 1)):
            if m[1] == 0:  # a zero front cutoff: the results of the plan that has never heard of one
                f, _front, back = m
                tp0 = plan_of(Q.chain(f, back), Q.chain(f, back))
                assert all(isinstance(o, planmod.QTrimOp) and o.cutoff_front == 0 for o in (tp0.r1.ops[-1], tp0.r2.ops[-1]))
                plain, _ = held.run(tp0)
                assert np.array_equal(plain[0], got[mate]) and np.array_equal(plain[1], got[mate]), (name, m)


@pytest.mark.parametrize("name,plans", T.SCAN_CASES, ids=[c[0] for c in T.SCAN_CASES])
def test_scan_kernel(name, plans):
    """F1 and its mirror image behind a cut of f bases, both mates, every (F, B) of the issue."""
    run_plain(name, plans)


@pytest.mark.parametrize("name,plans", T.DEEP_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(T.DEEP_CASES)])
def test_scan_kernel_deep_and_long_rows(name, plans):
    """Windows at every depth from the 5' end (a front walk of up to 34 dwords), full rows of 1536 bases of one byte, and
    every accepted cutoff as the front cutoff: the int sum of the front walk holds."""
    run_plain(name, plans)


# ---- N ends ----------------------------------------------------------------------------------------------------------

def stripped(tp):
    """The plan without the trailing QTrimOp / NTrimOp of its chains (what the oracle can run) and the tails."""
    chains, tails = [], []
    for mate in (tp.r1, tp.r2):
        if mate is None:
            chains.append(None)
            continue
        ops, tail = E.split_tail(mate.ops, planmod.QTrimOp, planmod.NTrimOp)
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
        out.append(E.apply_tail(seq, qual, res["start"], res["stop"], res["flags"], tails[m], tp.min_length))
    return out, raw


def n_batch(f, mask):
    rows = T.family(f"EN:{f}")
    seq = rows.seq.copy()
    if mask:
        from cutseq_amd.synth import SynthBatch
        util.soft_mask(SynthBatch(seq, rows.qual, rows.lens, None, None, None), fraction=0.2, seed=9 + f)
    return R.Rows(seq, rows.qual, rows.lens, f)


@pytest.mark.parametrize("mask", [False, True], ids=["upper", "soft-masked"])
@pytest.mark.parametrize("adapter", [CODED_ADAPTER, RAW_ADAPTER], ids=["coded", "raw"])
def test_n_ends(adapter, mask):
    """Every string over A, C, N, n behind a cut of f bases, [adapter, cut, trimmer, N trimmer]: coded plans (fast-form
    tiles in the part of the rows without an ``n``, exact-form tiles behind it and wherever the soft mask struck) and raw
    plans."""
    op = planmod.back(adapter, 0.0, len(adapter), flag=abi.CS_F_ADAPTER3)
    for f in range(4):
        rows = n_batch(f, mask)
        if mask:
            assert 0 < int((rows.seq[:9841] == ord("n")).any(axis=1).sum()) < 9841 // 2
        f2 = (f + 1) % 4
        tp = plan_of([op] + T.chain(f, 20, 20, trim_n=True), [op] + T.chain(f2, 20, 0, trim_n=True))
        wants, raw = layered(tp, [(rows.seq, rows.qual, rows.lens)] * 2)
        assert all((r["flags"] & MATCH_FLAGS == 0).all() for r in raw)
        # (the layering is what the rule alone says where no adapter matched)
        alone = T.rule_ends(rows, (f, 20, 20), trim_n=True, min_length=MIN_LENGTH)
        assert np.array_equal(alone.start, wants[0].start) and np.array_equal(alone.stop, wants[0].stop)
        Held(rows).check(tp, wants, f"N ends, f = {f}, {adapter}, mask {mask}")


# ---- resolve kernel --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["E1:0", "E1:3", "EN:1", "EN:2"])
def test_resolve_kernel(name):
    """[adapter, cut, trimmer(, N trimmer)] without the filter: every non-empty read goes to the exact DP and finishes
    its chain -- the end ops -- in the resolve kernel, rows gathered by lane."""
    rows = Q.planted(T.family(name), [Q.ADAPTER])
    trim_n = name.startswith("EN")
    f = rows.f
    op = Q.adapter_op(Q.ADAPTER)
    settings = [(f, 20, 20), ((f + 1) % 4, 21, 19)]
    end, flags = Q.after_adapter(rows, op)
    lens = rows.lens.astype(np.int64)
    assert 0 < int((end < lens).sum())
    wants = [T.rule_ends(rows, m, trim_n, end, flags, MIN_LENGTH) for m in settings]
    tp = plan_of([op] + T.chain(*settings[0], trim_n=trim_n), [op] + T.chain(*settings[1], trim_n=trim_n), use_filter=False)
    layer, _raw = layered(tp, [(rows.seq, rows.qual, rows.lens)] * 2)
    for m in (0, 1):
        assert np.array_equal(T.records(layer[m]), T.records(wants[m]))
    _got, stats = Held(rows).check(tp, wants, f"{name} behind an adapter, no filter")
    for mate in (0, 1):
        assert int(stats[mate].n_exact_dp) == int((lens > 0).sum())


# ---- long-read kernel: the same rows as FASTQ text at row stride 4 ---------------------------------------------------

@pytest.mark.parametrize("name,setting,trim_n", [("E1:1", (1, 20, 20), False), ("E1:1", (2, 20, 0), False),
                                                 ("EN:1", (1, 20, 20), True)])
def test_long_read_kernel(name, setting, trim_n):
    rows = T.family(name)
    tp = plan_of(T.chain(*setting, trim_n=trim_n), min_length=0)
    ends = T.rule_ends(rows, setting, trim_n)
    want = T.records(ends)
    n = len(rows.lens)
    names = [b"q%d" % i for i in range(n)]
    text = fastq_text(names, rows.seq, rows.qual, rows.lens)
    records = []
    for i in range(n):
        k = int(rows.lens[i])
        route, rec = hostfmt.format_single(names[i], rows.seq[i, :k].tobytes(), rows.qual[i, :k].tobytes(), want[i], None, tp)
        assert route == 0
        records.append(rec)
    got = run_text_exposed(tp, text, None, n, 4)
    assert got.n_long[0] == int((rows.lens > 4).sum()) > n // 2
    assert got.counts == [n, 0, 0]
    if got.streams[0][0] != b"".join(records):
        out = got.streams[0][0].split(b"\n")
        for i in range(n):
            assert out[4 * i:4 * i + 4] == records[i].split(b"\n")[:4], (name, i, want[i])
        raise AssertionError(name)
    assert int(got.stats[0].qualtrim_bp) == ends.cut and int(got.stats[0].out_bp) == int((ends.stop - ends.start).sum())


# ---- with the filters ------------------------------------------------------------------------------------------------

def end_runs(batch, seed):
    """N runs (upper and lower case) at the ends of every fourth read and low qualities at the 5' end of every fifth."""
    rng = np.random.default_rng(seed)
    for seq, qual, lens in ((batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2)):
        for i in range(0, batch.n, 4):
            n = int(lens[i])
            k = int(rng.integers(1, 9))
            if n >= 2 * k:
                seq[i, :k] = ord("N") if i % 8 else ord("n")
                seq[i, n - k:n] = ord("N") if i % 16 < 8 else ord("n")
        for i in range(0, batch.n, 5):
            qual[i, :int(rng.integers(1, 12))] = rng.integers(33, 45)
    return batch


def takara_settings(front, back, trim_n=True):
    st = planmod.CutadaptConfig()
    st.min_quality, st.min_quality_front, st.trim_n = back, front, trim_n
    return st


def test_with_the_filters():
    """One TAKARAV3 batch, -q 20,20 --trim-n with --max-n 0 -M 40 --max-ee 1: the filters, TooShort and the statistics
    see the end-trimmed intervals."""
    batch = end_runs(takara_batch(4096, 70, 21, clip=True), 22)
    st = takara_settings(20, 20)
    st.max_n, st.max_length, st.max_ee = 0.0, 40, 1.0
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True)
    mates = [(batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2)]
    wants, raw = layered(tp, mates)
    (g1, g2), xf, stats, counts = run_engine(tp, batch)
    every = 0
    for m, (seq, qual, _lens) in enumerate(mates):
        want = T.records(wants[m])
        want["cap_off"], want["cap_len"] = raw[m]["cap_off"], raw[m]["cap_len"]
        bad = np.flatnonzero((g1, g2)[m] != want)
        assert bad.size == 0, (m, bad[:5], (g1, g2)[m][bad[:5]], want[bad[:5]])
        x = filters_rule.xflags(seq, qual, want, max_length=40, max_n=0.0, max_ee=1.0)
        assert np.array_equal(xf[m], x), (m, np.flatnonzero(xf[m] != x)[:5])
        assert counts[m] == {"too_many_n": int(((x & abi.CS_X_TOO_MANY_N) != 0).sum()),
                             "too_long": int(((x & abi.CS_X_TOO_LONG) != 0).sum()),
                             "too_many_ee": int(((x & abi.CS_X_TOO_MANY_EE) != 0).sum())}
        assert all(v > 0 for v in counts[m].values()) and (x == 0).any()
        assert int(stats[m].qualtrim_bp) == wants[m].cut and int(stats[m].out_bp) == int((wants[m].stop - wants[m].start).sum())
        assert int(stats[m].n_too_short) == int(((wants[m].flags & abi.CS_F_TOO_SHORT) != 0).sum()) > 0
        # the end ops changed what the filters see: TooManyN would take more reads on the oracle's intervals
        before = filters_rule.xflags(seq, qual, raw[m], max_n=0.0)
        assert int((before != 0).sum()) > counts[m]["too_many_n"]
        every += int((wants[m].start > raw[m]["start"]).sum())
    assert every > 100


# ---- the command line ------------------------------------------------------------------------------------------------

def expected_files(tp, batch, names):
    mates = [(batch.seq1, batch.qual1, batch.len1)] + ([(batch.seq2, batch.qual2, batch.len2)] if tp.paired else [])
    wants, raw = layered(tp, mates)
    res = []
    for m in range(len(mates)):
        r = T.records(wants[m])
        r["cap_off"], r["cap_len"] = raw[m]["cap_off"], raw[m]["cap_len"]
        res.append(r)
    recs = util.format_batch(tp, batch, names, names, res[0], None, res[1] if tp.paired else None)
    streams = [[b"", b""] for _ in range(3)]
    for route, r1, r2 in recs:
        streams[route][0] += r1
        streams[route][1] += r2 or b""
    return streams, wants, res, recs


def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    """TAKARAV3 pairs, -q 15,10 --trim-n: the text path (with --info-file) and the record path write the same files, the
    ones the rules give; the table's no-match rows carry the end-trimmed read; the report's quality-trimmed bases are
    the rule's."""
    batch = end_runs(takara_batch(2000, 150, 31, clip=True), 32)
    names = [b"pair%d" % i for i in range(batch.n)]
    paths = [str(tmp_path / f"in{m}.fq.gz") for m in (1, 2)]
    util.write_fastq(paths[0], names, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(paths[1], names, batch.seq2, batch.qual2, batch.len2)
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], takara_settings(15, 10), True)
    streams, wants, res, recs = expected_files(tp, batch, names)
    assert streams[0][0].count(b"\n") > 4 * 500 and streams[1][0].count(b"\n") > 4 * 100
    info = str(tmp_path / "info.tsv")
    monkeypatch.delenv("CUTSEQ_TEXT_PATH", raising=False)
    text, rep_text, _ = run_cli(tmp_path, capsys, "text", paths, ["-q", "15,10", "--trim-n", "--info-file", info])
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    host, rep_host, _ = run_cli(tmp_path, capsys, "host", paths, ["-q", "15,10", "--trim-n"])
    monkeypatch.delenv("CUTSEQ_TEXT_PATH")
    assert text == host
    for kind, route in (("trimmed", 0), ("short", 1)):
        for m in (1, 2):
            assert text[(kind, m)] == streams[route][m - 1], (kind, m)
    for rep in (rep_text, rep_host):
        bp = rep["basepair_counts"]
        assert bp["quality_trimmed_read1"] == wants[0].cut and bp["quality_trimmed_read2"] == wants[1].cut
        assert wants[0].cut > 0 and bp["output_read1"] == sum(len(r1.split(b"\n")[1]) for rt, r1, _r2 in recs if rt == 0)
    # the table: a read without an adapter match has one row of name, -1, final sequence, final qualities
    rows = [line.split(b"\t") for line in open(info, "rb").read().split(b"\n") if line]
    none = [r for r in rows if r[1] == b"-1"]
    want_none = []
    changed = 0
    for i, (_rt, r1, _r2) in enumerate(recs):
        if int(res[0]["flags"][i]) & MATCH_FLAGS == 0:
            name, seq, _plus, qual = r1.split(b"\n")[:4]
            want_none.append([name[1:], b"-1", seq, qual, b""])
            first = int(res[0]["start"][i])
            changed += int(first < int(res[0]["stop"][i]) and batch.seq1[i, first - 1] == ord("N"))
    assert none == want_none and len(none) > 100 and changed > 10


def test_cli_single_end_fasta(tmp_path, capsys):
    """FASTA input: the quality op is inert, the N ends go."""
    batch = end_runs(takara_batch(600, 100, 41, clip=False), 42)
    names = [b"read%d" % i for i in range(batch.n)]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">" + names[i] + b"\n" + batch.seq1[i, :int(batch.len1[i])].tobytes() + b"\n" for i in range(batch.n)))
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], takara_settings(20, 20), False)
    from cutseq_amd.synth import SynthBatch
    inert = np.where(np.arange(batch.stride)[None, :] < batch.len1[:, None], ord("~"), 0).astype(np.uint8)
    single = SynthBatch(batch.seq1, inert, batch.len1, None, None, None)
    streams, wants, res, recs = expected_files(tp, single, names)
    assert wants[0].cut == 0 and not (wants[0].flags & abi.CS_F_QTRIMMED).any()
    pre = str(tmp_path / "fa")
    cli.main([str(fa), "-A", "TAKARAV3", "-O", pre, "-o", pre + "_trimmed.fa", "-s", pre + "_short.fa", "--json-file",
              pre + ".json", "--trim-n", "-q", "20,20"])
    capsys.readouterr()

    def as_fasta(stream):
        lines = stream.split(b"\n")
        return b"".join(b">" + lines[k][1:] + b"\n" + lines[k + 1] + b"\n" for k in range(0, len(lines) - 1, 4))

    assert open(pre + "_trimmed.fa", "rb").read() == as_fasta(streams[0][0])
    assert open(pre + "_short.fa", "rb").read() == as_fasta(streams[1][0])
    assert json.loads(open(pre + ".json").read())["basepair_counts"]["quality_trimmed_read1"] == 0
    lost = int(((res[0]["stop"] > res[0]["start"]) & (batch.seq1[np.arange(batch.n), np.maximum(res[0]["start"].astype(int) - 1, 0)] == ord("N"))
                & (res[0]["start"] > 0)).sum())
    assert lost > 20
