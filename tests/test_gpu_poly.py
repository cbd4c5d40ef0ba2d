"""The homopolymer closed forms of the tile kernels against the C oracle, bit for bit, on ENUMERATED reads
(tests/poly_rule.py; the CPU twin tests/test_poly_cpu.py holds the oracle to the plain rule and to the Python
restatement on the same reads).  Results are compared as whole 8-byte records; where ``run_both`` of
test_gpu_parity.py runs a plan, the statistics are compared too.  Paths:

  a  coded tiles, scan kernel: poly_maybe + poly_maps + poly_tail_wave / poly_head_wave
  b  the same behind a CutOp of c = 0..7 bases at the op's own end: every nibble offset of the anchored end
  c  raw tiles: poly_tail<false> / poly_head<false>
  d  resolve kernel: the op loop's !SCAN instantiation, behind an op that defers every read
  e  the reference's own chains: both poly ops on one mate, quality / N / NextSeq trimming behind the op
  f  letters: every base as the homopolymer, lower case under both case rules, IUPAC letters and dots

Every failure names the path, the op's parameters, the read and both records.  Paths protected: cutseq/run.py:388-413,
673-716.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import oracle
from cutseq_amd import abi, plan as planmod
from cutseq_amd.synth import SynthBatch

import nextseq_rule as N
import poly_rule as P
import universe as U
from test_gpu_exhaustive import Resident, THREADS
from test_gpu_parity import run_both

pytestmark = pytest.mark.gpu

RAW_ADAPTER = "ACGTNNACGTAC"  # (test_gpu_parity.py, test_adapter_with_non_acgt_base)
HELD = {}  # path -> alignments of a poly op the device was held to (printed per test: pytest -s)


class Held(Resident):
    """Resident with a batch of its own for either mate: (seq, qual, lens) each, of one shape."""

    def __init__(self, b1, b2):
        dev = torch.device("cuda:0")
        assert b1[0].shape == b2[0].shape == b1[1].shape == b2[1].shape
        self.batches = (b1, b2)
        self.n, self.stride = b1[0].shape
        self.t = [[torch.from_numpy(b[0]).to(dev), torch.from_numpy(b[1]).to(dev), torch.from_numpy(b[2].view(np.int16)).to(dev)]
                  for b in self.batches]
        self.out = [torch.zeros((self.n, 8), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.r = [abi.cs_reads(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), o.data_ptr(), None, None)
                  for t, o in zip(self.t, self.out)]
        self.stream = torch.cuda.Stream(device=dev)
        self.handle = C.c_void_p(self.stream.cuda_stream)

    def expect(self, tp):
        """The oracle on the plan -- on the plan without its trailing NextSeq / quality / N trimmers, which the rules of
        tests/nextseq_rule.py and tests/endtrim_rule.py then apply to the oracle's intervals (as test_gpu_nextseq.py)."""
        chains, tails = [], []
        for mate in (tp.r1, tp.r2):
            ops, tail = N.split_tail(mate.ops, planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp)
            plain = tail == N.Tail() or (tail.nextseq is None and not tail.rest.trim_n and tail.rest.front == 0)
            chains.append(mate if plain else dataclasses.replace(mate, ops=ops))
            tails.append(None if plain else tail)
        base = dataclasses.replace(tp, r1=chains[0], r2=chains[1])
        a1, n1, a2, n2 = base.pack()
        want = []
        for (ops, count), (seq, qual, lens), tail in zip(((a1, n1), (a2, n2)), self.batches, tails):
            res = oracle.trim_mate(ops, count, base.params(), seq, qual, lens, threads=THREADS)[0]
            if tail is not None:
                ends = N.apply_tail(seq, qual, res["start"], res["stop"], res["flags"], tail, tp.min_length)
                res = res.copy()
                res["start"], res["stop"], res["flags"] = ends.start, ends.stop, ends.flags
            want.append(res)
        return want

    def hold(self, tp, path, what, poly_ops=(1, 1)):
        """Device == oracle for both mates; ``what``: the op's parameters per mate; ``poly_ops``: poly ops per mate."""
        want = self.expect(tp)
        got = self.run(tp)
        for mate in (0, 1):
            if not np.array_equal(got[mate], want[mate]):
                seq, _qual, lens = self.batches[mate]
                bad = np.flatnonzero(got[mate] != want[mate])
                i = int(bad[0])
                raise AssertionError(f"path {path}, {what[mate]}, mate {mate + 1}: read {seq[i, :lens[i]].tobytes().decode()!r}: "
                                     f"device {got[mate][i]} != oracle {want[mate][i]} ({len(bad)} of {self.n} reads differ)")
            HELD[path] = HELD.get(path, 0) + poly_ops[mate] * self.n
        return want


def qualities(seq: np.ndarray) -> np.ndarray:
    """Phred 0..40 from the position and the row: low and high values anywhere, so that every trimmer has work."""
    rows, cols = np.indices(seq.shape)
    return np.where(seq > 0, 33 + (rows * 7 + cols * cols * 3 + (rows >> 3)) % 41, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reads_of(name: str) -> P.Reads:
    make = {"full": P.full, "w7": lambda: P.join(P.windows(7), P.periodic()), "w7only": lambda: P.windows(7), "edges": P.edges}
    return make[name]()


def batch(name, head, base, foreign, pad=0, real_qualities=False, **letters):
    reads = reads_of(name)
    seq, lens = P.place(P.letters(reads, base, foreign, **letters), reads.lens, head, pad=pad, stride=P.WIDTH + 8)
    return seq, qualities(seq) if real_qualities else np.where(seq > 0, ord("I"), 0).astype(np.uint8), lens


@functools.lru_cache(maxsize=2)
def held(name, tail_base, tail_foreign, head_base, head_foreign, pad=0, real_qualities=False, lower_every=0, odd_body=False):
    kw = dict(pad=pad, real_qualities=real_qualities, lower_every=lower_every, odd_body=odd_body)
    return Held(batch(name, False, tail_base, tail_foreign, **kw), batch(name, True, head_base, head_foreign, **kw))


def held_for(name, index, **kw):
    return held(name, P.TAIL_BASE, P.foreign_of(P.TAIL_BASE, index), P.HEAD_BASE, P.foreign_of(P.HEAD_BASE, index), **kw)


def ops_of(index, tail_base=P.TAIL_BASE, head_base=P.HEAD_BASE):
    m, rate, mo = P.PARAMS[index]
    return P.poly_op(tail_base, m, rate, mo, False), P.poly_op(head_base, m, rate, mo, True)


def names(index, rule, extra=""):
    m, rate, mo = P.PARAMS[index]
    tag = f"m={m} rate={rate} min_overlap={mo} rule={rule} tie={P.tie_of(index)}{extra}"
    return [f"tail {tag}", f"head {tag}"]


def raw_op():
    return planmod.back(RAW_ADAPTER, 0.2, 3, flag=abi.CS_F_ADAPTER3)


def hold_raw(h, tail, head, rule, tie, path, what, case=abi.CS_CASE_FOLD):
    """The two ops in plans whose OTHER chain holds an adapter with a non-ACGT base: raw tiles."""
    for chains, poly in ((([tail], [raw_op()]), (1, 0)), (([raw_op()], [head]), (0, 1))):
        tp = U.one_op_plan(chains[0], chains[1], rule, tie)
        tp.case_rule = case
        h.hold(tp, path, [f"{w} (raw tiles)" for w in what], poly_ops=poly)


def report(path):
    print(f"path {path}: {HELD.get(path, 0)} alignments so far")


PARAM_IDS = [f"{m}-{rate}-{mo}" for m, rate, mo in P.PARAMS]


@pytest.mark.parametrize("index", range(len(P.PARAMS)), ids=PARAM_IDS)
def test_a_coded_tiles_in_the_scan_kernel(index):
    """Mate 1 the tail op over the tail reads, mate 2 the head op over the head reads, under both selection rules, on
    the whole universe: windows(9) + periodic() = 201 036 reads per end (the oracle's four runs take at most 2.6 s on
    8 threads, the longest at m = 127 and 128)."""
    h = held_for("full", index)
    assert h.n == 201036
    tail, head = ops_of(index)
    for rule in P.RULES:
        h.hold(U.one_op_plan([tail], [head], rule, P.tie_of(index)), "a", names(index, rule))
    report("a")


@pytest.mark.parametrize("c", range(8))
def test_b_every_alignment_of_the_anchored_end(c):
    """The op behind a CutOp of c bases at its own end (tails: e & 7 moves, and the reads' lengths move it further; heads:
    s & 7 = c): windows(7), 48 960 reads per end with c bases of G at the anchored end for the cut to take.  The
    reference's own parameters meet every c under both rules, every other set two values of c (poly_rule.cuts_of)."""
    for index in range(len(P.PARAMS)):
        if c not in P.cuts_of(index):
            continue
        h = held_for("w7only", index, pad=c)
        assert h.n == 48960
        tail, head = ops_of(index)
        for rule in (P.RULES if index == 0 else (P.RULES[(index + c) % 2],)):
            tp = U.one_op_plan([planmod.CutOp(-c), tail], [planmod.CutOp(c), head], rule, P.tie_of(index))
            h.hold(tp, "b", names(index, rule, f" behind a cut of {c}"))
    report("b")


@pytest.mark.parametrize("index", range(len(P.PARAMS)), ids=PARAM_IDS)
def test_c_raw_tiles(index):
    """The same ops in a plan whose other chain holds ``ACGTNNACGTAC``: cs_plan_create (cutseq_hip.hip, "coded tile:
    possible when every adapter base is A/C/G/T": ``coded = coded && is_acgt(op.seq[j])`` over the adapters of BOTH mates)
    then leaves the plan uncoded, the tiles keep their bytes and the op loop calls poly_tail<false> / poly_head<false>.
    The ABI does not report which form ran.  windows(7) + periodic() = 53 580 reads per end, both rules."""
    h = held_for("w7", index)
    assert h.n == 53580
    tail, head = ops_of(index)
    for rule in P.RULES:
        hold_raw(h, tail, head, rule, P.tie_of(index), "c", names(index, rule))
    report("c")


@pytest.mark.parametrize("index", range(len(P.PARAMS)), ids=PARAM_IDS)
def test_d_resolve_kernel(index):
    """[an adapter of 65 nt or more under CS_WHERE_BACK, the poly op]: the first op has no filter, every read that is not
    empty is deferred, and the poly op runs in the resolve kernel.  The long adapter is made of two letters the reads
    do not hold, so it matches nowhere (the oracle decides either way).  edges(), 10 572 reads per end, both rules."""
    h = held_for("edges", index)
    assert h.n == 10572
    tail, head = ops_of(index)

    def long_adapter(base):
        free = [b for b in "ACGT" if b not in (base, P.foreign_of(base, index))]
        return planmod.back("".join(free[(i * i + i // 3) % 2] for i in range(65 + index)), 0.1, 3, flag=abi.CS_F_ADAPTER3)

    for rule in P.RULES:
        tp = U.one_op_plan([long_adapter(P.TAIL_BASE), tail], [long_adapter(P.HEAD_BASE), head], rule, P.tie_of(index))
        want = h.hold(tp, "d", names(index, rule, " behind a 65+ nt adapter"))
        assert not any((w["flags"] & abi.CS_F_ADAPTER3).any() for w in want)
    report("d")


E_SETS = (0, 6)  # the reference's own parameters and (64, .3, 10)


def both_ends_batch(index) -> SynthBatch:
    """Reads with a universe read at both ends: read i's head form (poly-T) in front of read (7 i + 3) mod n's tail form."""
    reads = reads_of("edges")
    n = len(reads.lens)
    other = (np.arange(n) * 7 + 3) % n
    hs, hl = P.place(P.letters(reads, P.HEAD_BASE, P.foreign_of(P.HEAD_BASE, index)), reads.lens, True)
    ts, tl = P.place(P.letters(reads, P.TAIL_BASE, P.foreign_of(P.TAIL_BASE, index)), reads.lens, False)
    seq = np.zeros((n, 2 * P.WIDTH), dtype=np.uint8)
    for i in range(n):
        j = other[i]
        seq[i, :hl[i]] = hs[i, :hl[i]]
        seq[i, hl[i]:hl[i] + tl[j]] = ts[j, :tl[j]]
    lens = (hl.astype(np.int64) + tl[other]).astype(np.uint16)
    qual = qualities(seq)
    return SynthBatch(seq, qual, lens, seq.copy(), qual.copy(), lens.copy())


@pytest.mark.parametrize("index", E_SETS, ids=[PARAM_IDS[i] for i in E_SETS])
def test_e_both_ops_on_one_mate(index):
    """--trim-polyA-wo-direction: [tail, head] on mate 1 and [head, tail] on mate 2 over reads that open with a head read
    and close with a tail read (10 572 of them), both rules, statistics compared; once without the filter."""
    b = both_ends_batch(index)
    tail, head = ops_of(index)
    for rule, use_filter in ((P.LEFTMOST, True), (P.SCORE, True), (P.LEFTMOST, False)):
        if not use_filter and index != 0:
            continue
        tp = U.one_op_plan([tail, head], [head, tail], rule, P.tie_of(index), use_filter=use_filter)
        try:
            g1, g2 = run_both(tp, b, threads=THREADS)
        except AssertionError as err:
            raise AssertionError(f"path e, {names(index, rule, f' both ops on one mate, use_filter={use_filter}')}: {err}") from err
        assert ((g1["flags"] & abi.CS_F_POLY) != 0).sum() > b.n // 4 and (g1["start"] > 0).any() and (g2["stop"] < b.len2).any()
        if use_filter:
            HELD["e"] = HELD.get("e", 0) + 4 * b.n
    report("e")


E_TAILS = {
    "quality-filters": ([planmod.QTrimOp(20)], dict(max_length=150, max_ee=2.0)),                  # the FILT_ALL kernels
    "quality-both-ends-and-n": ([planmod.QTrimOp(20, cutoff_front=15), planmod.NTrimOp()], {}),    # the read-end kernels
    "nextseq": ([planmod.NextSeqTrimOp(20), planmod.QTrimOp(20)], {}),                             # the FILT_NEXTSEQ kernels
}


@pytest.mark.parametrize("tail_name", sorted(E_TAILS))
@pytest.mark.parametrize("index", E_SETS, ids=[PARAM_IDS[i] for i in E_SETS])
def test_e_trimmers_behind_the_op(index, tail_name):
    """The poly op followed by the quality trimmer (with -M / --max-ee filters: the kernels that decide filters), by
    -q F,B + --trim-n, and by --nextseq-trim: the instantiations of the tile kernels the reference's flags select.
    Qualities run over Phred 0..40; the foreign letter is N (for --trim-n) or G (for --nextseq-trim)."""
    ops, filters = E_TAILS[tail_name]
    foreign = {"quality-both-ends-and-n": "N", "nextseq": "G"}.get(tail_name, "C")
    h = held("edges", P.TAIL_BASE, foreign, P.HEAD_BASE, foreign, real_qualities=True)
    tail, head = ops_of(index)
    for rule in P.RULES:
        tp = U.one_op_plan([tail] + ops, [head] + ops, rule, P.tie_of(index))
        for key, value in filters.items():
            setattr(tp, key, value)
        want = h.hold(tp, "e", names(index, rule, f" + {tail_name}"))
        plain = h.expect(U.one_op_plan([tail], [head], rule, P.tie_of(index)))
        for w, p in zip(want, plain):  # the trimmers had work, behind hits and elsewhere
            moved = (w["start"] != p["start"]) | (w["stop"] != p["stop"])
            assert (moved & ((p["flags"] & abi.CS_F_POLY) != 0)).sum() > 100 and ((w["flags"] & abi.CS_F_QTRIMMED) != 0).sum() > 100
    report("e")


F_SETS = (0, 8)  # the reference's own parameters and (33, .15, 1)


@pytest.mark.parametrize("base", "ACGT")
def test_f_every_base_as_the_homopolymer(base):
    """X * m for every X of ACGT at both ends (the coded tiles compare nibbles of the base's code), coded and raw."""
    for index in F_SETS:
        foreign = P.foreign_of(base, index + "ACGT".index(base))
        h = held("edges", base, foreign, base, foreign)
        tail, head = ops_of(index, base, base)
        for rule in P.RULES:
            what = names(index, rule, f" base {base} foreign {foreign}")
            h.hold(U.one_op_plan([tail], [head], rule, P.tie_of(index)), "f", what)
            hold_raw(h, tail, head, rule, P.tie_of(index), "f", what)
    report("f")


@pytest.mark.parametrize("case", [abi.CS_CASE_FOLD, abi.CS_CASE_SENSITIVE], ids=["fold", "sensitive"])
def test_f_lower_case_copies_of_the_base(case):
    """Every fifth base of the run is the base in lower case: the base itself under CS_CASE_FOLD, a foreign base under
    CS_CASE_SENSITIVE; coded (such tiles take the exact re-coding) and raw."""
    for index in F_SETS:
        h = held_for("edges", index, lower_every=5)
        assert any(b"a" in h.batches[0][0][i].tobytes() for i in range(0, h.n, 501))
        tail, head = ops_of(index)
        for rule in P.RULES:
            what = names(index, rule, f" lower case, case rule {case}")
            tp = U.one_op_plan([tail], [head], rule, P.tie_of(index))
            tp.case_rule = case
            want = h.hold(tp, "f", what)
            hold_raw(h, tail, head, rule, P.tie_of(index), "f", what, case=case)
            if index == 0:  # the two case rules part company on these reads
                tp.case_rule = abi.CS_CASE_SENSITIVE + abi.CS_CASE_FOLD - case
                assert not np.array_equal(h.expect(tp)[0], want[0])
    report("f")


def test_f_iupac_letters_and_dots_in_the_body():
    """The bodies of twenty hold an R and a dot: tiles that leave the fast re-coding; foreign to every homopolymer."""
    for index in F_SETS:
        h = held_for("edges", index, odd_body=True)
        assert any(b"R" in h.batches[0][0][i].tobytes() and b"." in h.batches[0][0][i].tobytes() for i in range(h.n))
        tail, head = ops_of(index)
        for rule in P.RULES:
            what = names(index, rule, " R and . in the body")
            h.hold(U.one_op_plan([tail], [head], rule, P.tie_of(index)), "f", what)
            hold_raw(h, tail, head, rule, P.tie_of(index), "f", what)
    report("f")
