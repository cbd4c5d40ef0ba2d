"""CPU side of the homopolymer enumeration (tests/poly_rule.py): the closed-form rule against the C oracle on every
read of the universe, the C oracle against the Python restatement at adapter lengths up to 128, the model of the coded
tiles' road against the rule -- with every planted defect showing -- and the classes of outcome the reads must hold.
The GPU file (tests/test_gpu_poly.py) then holds the kernels to the C oracle on the same reads.  Paths protected:
cutseq/run.py:388-413, 673-716.
"""
import functools
import multiprocessing as mp

import numpy as np
import pytest

import oracle
from oracle import pyref
from cutseq_amd import abi

import poly_rule as P
import universe as U

THREADS = max(1, min(8, oracle.host_threads()))


@functools.lru_cache(maxsize=None)
def reads_of(name: str) -> P.Reads:
    return {"full": P.full, "edges": P.edges, "model": lambda: P.join(P.windows(5), P.periodic())}[name]()


@functools.lru_cache(maxsize=4)
def placed(name: str, head: bool, foreign: str):
    reads = reads_of(name)
    seq, lens = P.place(P.letters(reads, P.HEAD_BASE if head else P.TAIL_BASE, foreign), reads.lens, head)
    return seq, np.where(seq > 0, ord("I"), 0).astype(np.uint8), lens


def oracle_results(batch, op, rule, tie, threads=THREADS):
    tp = U.one_op_plan([op], None, rule, tie)
    a1, n1, _a2, _n2 = tp.pack()
    return oracle.trim_mate(a1, n1, tp.params(), *batch, threads=threads)[0]


@functools.lru_cache(maxsize=None)
def oracle_on_the_universe(index: int, head: bool, rule: int):
    """Computed once, shared by the tests below (1.6 MB a result)."""
    m, rate, mo = P.PARAMS[index]
    base = P.HEAD_BASE if head else P.TAIL_BASE
    return oracle_results(placed("full", head, P.foreign_of(base, index)), P.poly_op(base, m, rate, mo, head), rule, P.tie_of(index))


def test_the_universe_is_what_it_says_and_both_forms_of_the_rule_agree():
    assert len(P.windows(9).lens) == 196416 and len(P.windows(7).lens) == 48960 and len(P.periodic().lens) == 4620
    edges = reads_of("edges")
    assert len(edges.lens) == 10572 and int(edges.lens.max()) == P.WIDTH and int(edges.lens.min()) == 0
    # a tail read is the head read reversed; padding sits at the anchored end
    lett = P.letters(edges, "A", "C")
    hs, hl = P.place(lett, edges.lens, head=True, pad=3)
    ts, tl = P.place(lett, edges.lens, head=False, pad=3)
    for i in range(0, len(hl), 97):
        h, t = hs[i, :hl[i]].tobytes(), ts[i, :tl[i]].tobytes()
        assert h == t[::-1] and h[:3] == b"GGG" and len(h) == edges.lens[i] + 3
        assert [c != ord("A") for c in h[3:]] == list(edges.rev[i, :edges.lens[i]])
    # the settings: what the rule is given is what the op holds
    for index, (m, rate, mo) in enumerate(P.PARAMS):
        for head in (False, True):
            op = P.poly_op("T" if head else "A", m, rate, mo, head)
            thr = op.thresholds()
            assert op.m == m and op.k == int(rate * m) == thr[m] and op.min_overlap == mo and thr[0] == 0
            assert all(0 <= thr[i] - thr[i - 1] <= 1 for i in range(1, m + 1))
    assert P.PARAMS[0] == (100, 0.15, 3) and set(P.MODEL_PARAMS) <= set(P.PARAMS)
    # every cut meets at least three parameter sets, the reference's own among them
    for c in range(8):
        sets = [i for i in range(len(P.PARAMS)) if c in P.cuts_of(i)]
        assert 0 in sets and len(sets) >= 3, (c, sets)
    # the rule read by read == the rule over rows
    some = P.Reads(*[a[5::41] for a in edges])
    for m, rate, mo in P.PARAMS:
        op = P.poly_op("A", m, rate, mo, False)
        thr = op.thresholds()
        for head in (False, True):
            strs = P.strings(*P.place(P.letters(some, "A", "C"), some.lens, head))
            for rule in P.RULES:
                if head:
                    hit, start, dp = P.rules_head(some, m, op.k, thr, mo, rule)
                    rows = [P.DP if d else ((int(s), len(r)) if h else None) for r, h, s, d in zip(strs, hit, start, dp)]
                    assert rows == [P.rule_head(r, "A", m, op.k, thr, mo, rule) for r in strs], (m, rate, mo, rule)
                else:
                    hit, stop = P.rules_tail(some, m, op.k, thr, mo, rule)
                    rows = [(0, int(s)) if h else None for h, s in zip(hit, stop)]
                    assert rows == [P.rule_tail(r, "A", m, op.k, thr, mo, rule) for r in strs], (m, rate, mo, rule)


def first_bad(same, reads, what):
    if not same.all():
        i = int(np.flatnonzero(~same)[0])
        q = reads.rev[i, :reads.lens[i]]
        raise AssertionError(f"{what}: read (from the anchored end, x = foreign) {''.join('x' if f else '-' for f in q)!r}: "
                             f"{int((~same).sum())} of {len(same)} reads differ")


@pytest.mark.parametrize("index", range(len(P.PARAMS)))
def test_the_rule_equals_the_c_oracle_on_the_whole_universe(index):
    """windows(9) + periodic() = 201 036 reads per end x both selection rules x both ends: 804 144 alignments per
    parameter set, 11.3 M over the 14 sets; interval and CS_F_POLY compared.  Heads whose columns beyond m are reachable
    (n > m, at most k foreign bases among the first m -- asserted from the letters) are the rule's ``DP``: left out and
    counted.  No tail read is DP: ``rules_tail`` has no such answer.
    Measured (8 threads): 1.8 s (m = 1) to 7.2 s (m = 100) a case, 62 s for the 14; the oracle's share is at most 2.6 s a case."""
    m, rate, mo = P.PARAMS[index]
    reads, tie = reads_of("full"), P.tie_of(index)
    assert len(reads.lens) == 196416 + 4620
    dps = []
    for head in (False, True):
        base = P.HEAD_BASE if head else P.TAIL_BASE
        batch = placed("full", head, P.foreign_of(base, index))
        op = P.poly_op(base, m, rate, mo, head)
        thr = op.thresholds()
        for rule in P.RULES:
            got = oracle_on_the_universe(index, head, rule)
            flag = (got["flags"] & abi.CS_F_POLY) != 0
            what = f"{'head' if head else 'tail'} m={m} rate={rate} min_overlap={mo} rule={rule} tie={tie}"
            if head:
                hit, start, dp = P.rules_head(reads, m, op.k, thr, mo, rule)
                seq, _q, lens = batch
                foreign_in_m = ((seq[:, :m] != ord(base)) & (seq[:, :m] != 0)).sum(axis=1)
                assert np.array_equal(dp, (lens > m) & (foreign_in_m <= op.k)), what
                dps.append(int(dp.sum()))
                first_bad(dp | ((got["start"] == start) & (got["stop"] == reads.lens) & (flag == hit)), reads, what)
            else:
                hit, stop = P.rules_tail(reads, m, op.k, thr, mo, rule)
                first_bad((got["start"] == 0) & (got["stop"] == stop) & (flag == hit), reads, what)
    assert dps[0] == dps[1] and (dps[0] > 0) == (m < P.WIDTH)  # (counted; the share is what it is)


# ---- the C oracle against pyref at these lengths

def _pyref_rows(args):
    head, base, m, rate, mo, rule, tie, reads = args
    al = pyref.Aligner(base * m, rate, pyref.FRONT_NOT_INTERNAL if head else pyref.BACK_NOT_INTERNAL, mo, rule, tie)
    out = []
    for read in reads:
        aln = al.locate(read)
        if aln is None:
            out.append((0, len(read), 0))
        else:
            out.append((aln[3], len(read), 1) if head else (0, aln[2], 1))
    return out


def test_c_oracle_equals_python_restatement_at_poly_lengths():
    """The independent check that the oracle itself is right at m up to 128 (the twin in test_exhaustive_cpu.py stops
    at m = 6): every PARAMS entry x both ends x both selection rules on every read of edges(): 592 032
    alignments, each computed twice (pyref prunes rows above k errors like cutadapt, so most reads cost it little).
    Measured: 56 s on 8 workers."""
    edges = reads_of("edges")
    jobs, keys = [], []
    for index, (m, rate, mo) in enumerate(P.PARAMS):
        some = edges
        for head in (False, True):
            base = P.HEAD_BASE if head else P.TAIL_BASE
            seq, lens = P.place(P.letters(some, base, P.foreign_of(base, index)), some.lens, head)
            batch = (seq, np.where(seq > 0, ord("I"), 0).astype(np.uint8), lens)
            strs = P.strings(seq, lens)
            for rule in P.RULES:
                for lo in range(0, len(strs), 64):
                    jobs.append((head, base, m, rate, mo, rule, P.tie_of(index), strs[lo:lo + 64]))
                keys.append((index, head, rule, batch, strs))
    with mp.get_context("fork").Pool(THREADS) as pool:
        rows = pool.map(_pyref_rows, jobs, chunksize=1)
    at, total = 0, 0
    for index, head, rule, batch, strs in keys:
        m, rate, mo = P.PARAMS[index]
        want = []
        while len(want) < len(strs):
            want += rows[at]
            at += 1
        got = oracle_results(batch, P.poly_op(P.HEAD_BASE if head else P.TAIL_BASE, m, rate, mo, head), rule, P.tie_of(index))
        w = np.array(want, dtype=np.int64).reshape(-1, 3)
        same = (got["start"] == w[:, 0]) & (got["stop"] == w[:, 1]) & (((got["flags"] & abi.CS_F_POLY) != 0) == (w[:, 2] != 0))
        if not same.all():
            i = int(np.flatnonzero(~same)[0])
            raise AssertionError(f"{'head' if head else 'tail'} {P.PARAMS[index]} rule {rule}: read {strs[i]!r}: C oracle {got[i]} "
                                 f"!= pyref {want[i]}")
        total += len(strs)
    assert at == len(rows) and total == 56 * 10572


# ---- the model of the coded road

def _model_rows(args):
    head, m, k, thr, mo, rule, defect, bits, lens = args
    out = np.empty(len(bits), dtype=np.int64)  # -1 none, -2 DP, else the bases removed
    for i, (fg, n) in enumerate(zip(bits, lens)):
        r = P.shortcut_bits(fg, n, m, k, thr, mo, rule, head, defect)
        out[i] = -1 if r is None else -2 if r is P.DP else (r[0] if head else n - r[1])
    return out


def test_the_model_of_the_coded_road_equals_the_rule_and_every_defect_shows():
    """``shortcut`` == the rule on windows(5) + periodic() (16 716 reads per end) over MODEL_PARAMS under both rules; every
    entry of DEFECTS changes at least one result for at least one parameter set, a tail or head defect at its own end:
    a universe shrunk below what tells them apart fails here."""
    reads = reads_of("model")
    assert len(reads.lens) == 16716
    bits, lens = P.bitmaps(reads), [int(x) for x in reads.lens]
    jobs, want = [], {}
    for m, rate, mo in P.MODEL_PARAMS:
        op = P.poly_op("A", m, rate, mo, False)
        thr, k = op.thresholds(), op.k
        for rule in P.RULES:
            hit, stop = P.rules_tail(reads, m, k, thr, mo, rule)
            want[(False, m, rule)] = np.where(hit, reads.lens - stop, -1)
            hit, start, dp = P.rules_head(reads, m, k, thr, mo, rule)
            want[(True, m, rule)] = np.where(dp, -2, np.where(hit, start, -1))
            for head in (False, True):
                for defect in (None,) + (P.HEAD_DEFECTS if head else P.TAIL_DEFECTS):
                    jobs.append((head, m, k, thr, mo, rule, defect, bits, lens))
    with mp.get_context("fork").Pool(THREADS) as pool:
        rows = pool.map(_model_rows, jobs, chunksize=1)
    changed = {(d, head): 0 for head in (False, True) for d in (P.HEAD_DEFECTS if head else P.TAIL_DEFECTS)}
    for (head, m, _k, _thr, mo, rule, defect, _b, _l), got in zip(jobs, rows):
        diff = got != want[(head, m, rule)]
        if defect is None:
            first_bad(~diff, reads, f"model {'head' if head else 'tail'} m={m} min_overlap={mo} rule={rule}")
        else:
            changed[(defect, head)] += int(diff.sum())
    assert set(d for d, _h in changed) == set(P.DEFECTS)
    print(sorted(changed.items()))
    # (a head or tail defect exists at its own end only; one of the shared steps has to show at one end at least:
    # the tail walk judges every stop against thr[i] again, so a stop wrongly let in by thr[q + 1] changes nothing there)
    assert not [d for d in P.DEFECTS if not sum(n for (dd, _h), n in changed.items() if dd == d)]
    assert not [key for key, n in changed.items() if n == 0 and key != ("threshold_of_next_stop", False)]
    # the string form is the bitmap form
    for i in range(0, len(lens), 501):
        for head in (False, True):
            s = P.strings(*P.place(P.letters(P.Reads(*[a[i:i + 1] for a in reads]), "A", "G"), reads.lens[i:i + 1], head))[0]
            op = P.poly_op("A", 33, .15, 1, head)
            assert P.shortcut(s, "A", 33, op.k, op.thresholds(), 1, 0, head) == \
                P.shortcut_bits(bits[i], lens[i], 33, op.k, op.thresholds(), 1, 0, head)


# ---- what the reads must hold

@pytest.mark.parametrize("index", [i for i, p in enumerate(P.PARAMS) if p[0] >= 20])
def test_every_class_of_outcome_is_present(index):
    """From the oracle's results on the whole universe (rule LEFTMOST), per end: reads without a hit, reads that take the
    longest row inside the budget, reads that take a shorter one, reads shorter and longer than the adapter, and reads
    that spend the budget within 32 bases and are hit all the same.  Two classes cannot exist for every setting, and
    then must be EMPTY.  A shorter row: a hit is a row of min_overlap bases or more, so there is none when
    min_overlap == m; and with k == 0 every row inside the budget is free of foreign bases, so the longest one scores
    most under the highest threshold.  A hit behind a spent budget: a row of 32 bases or more holds every foreign base
    of the first 32, so the hit is shorter than 32: min_overlap < 32; and the densest 32 bases of the universe hold 29
    foreign ones (a window of nine in front of the body of twenty): k < 29."""
    m, rate, mo = P.PARAMS[index]
    reads = reads_of("full")
    counts = P._counts(reads)
    for head in (False, True):
        base = P.HEAD_BASE if head else P.TAIL_BASE
        op = P.poly_op(base, m, rate, mo, head)
        got = oracle_on_the_universe(index, head, P.LEFTMOST)
        hit = (got["flags"] & abi.CS_F_POLY) != 0
        removed = (got["start"] if head else reads.lens - got["stop"]).astype(np.int64)
        lim = np.minimum(reads.lens, m)
        cols = np.arange(counts.shape[1])
        longest = ((counts <= op.k) & (cols[None, :] <= lim[:, None])).sum(axis=1) - 1  # counts never fall
        spent = counts[np.arange(len(lim)), np.minimum(lim, 32)] > op.k
        classes = {"no hit": ~hit, "longest": hit & (removed >= longest), "shorter": hit & (removed < longest),
                   "n < m": reads.lens < m, "n > m": reads.lens > m, "spent": hit & spent}
        possible = {"shorter": mo < m and op.k >= 1, "spent": mo < 32 and op.k < 29}
        for name, rows in classes.items():
            assert bool(rows.any()) == possible.get(name, True), (P.PARAMS[index], "head" if head else "tail", name, int(rows.sum()))
