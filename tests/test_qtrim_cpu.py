"""CPU twin of tests/test_gpu_qtrim.py: the families of tests/qtrim_rule.py meet what they promise (every lane of a
group in every role, every stop value, the designed number of walkers per tile), and the C oracle, the Python
restatement and the vectorised rule agree with the plain rule on them -- so the GPU tests may take either as the
expected value.  Also the reason why clamping the cutoff at plan creation changes no result.
"""
import functools
import itertools

import numpy as np
import pytest

import oracle
from oracle import pyref
from cutseq_amd import abi, plan as planmod

import qtrim_rule as R

THREADS = max(1, min(16, oracle.host_threads()))


# ---- plans and cases, shared with the GPU tests

def chain(f, cutoff, base=33):
    return ([planmod.CutOp(f)] if f else []) + [planmod.QTrimOp(cutoff, base)]


def plan_of(ops1, ops2=None, use_filter=True):
    return planmod.TrimPlan(r1=planmod.MateChain(list(ops1)), r2=planmod.MateChain(list(ops2)) if ops2 is not None else None,
                            has_umi=False, min_length=0, untrimmed_filter=False, use_filter=use_filter)


@functools.lru_cache(maxsize=4)
def build(name):
    """A family by name -> Rows (the last ones built are kept: the CPU twin and a GPU test ask for the same)."""
    kind, _, arg = name.partition(":")
    if kind == "F1a":
        return R.f1(int(arg), R.ALPHABETS[0])
    if kind == "F1b":
        return R.f1(int(arg), R.ALPHABETS[1])
    if kind == "F2A":
        return R.f2("A", int(arg))
    if kind == "F2B":
        return R.f2("B", int(arg))
    if kind == "F3":
        return R.f3(int(arg))[0]
    if kind == "F4":
        return R.f4(int(arg))
    if kind == "F5":
        c, b = R.F5_SETTINGS[int(arg)]
        return R.f1(1, R.ALPHABETS[0], cutoff=c, base=b)
    if kind == "F5edge":
        return R.f1_bytes(1, R.F5_EDGE_BYTES)
    if kind == "F6short":
        return R.f6_short()
    if kind == "F6long":
        return R.f6_long()
    raise KeyError(name)


def scan_cases():
    """-> [(family name, [(mate 1 (f, cutoff, base), mate 2 (f, cutoff, base)), ...])]: paired plans whose mates run
    different chains over the same rows."""
    cases = []
    for f in range(5):
        cases.append((f"F1a:{f}", [((f, 20, 33), ((f + 1) % 5, 21, 33)), ((f, 19, 33), ((f + 2) % 5, 20, 33))]))
        cases.append((f"F1b:{f}", [((f, 20, 33), ((f + 3) % 5, 18, 33))]))
    for f in range(4):
        cases.append((f"F2A:{f}", [((f, 20, 33), ((f + 1) % 4, 20, 33))]))
        cases.append((f"F2B:{f}", [((f, 20, 33), ((f + 2) % 4, 21, 33))]))
        cases.append((f"F3:{f}", [((f, 20, 33), ((f + 1) % 4, 20, 33))]))
    for f in (0, 3):
        cases.append((f"F4:{f}", [((f, 20, 33), (f, 93, 33)), ((f + 1, 20, 33), (f + 2, 19, 33))]))
    for i, (c, b) in enumerate(R.F5_SETTINGS):
        cases.append((f"F5:{i}", [((1, c, b), (2, c, b))]))
    cases.append(("F5edge:0", [((1, 20, 33), (0, 20, 33)), ((1, 0, 33), (2, 222, 33)), ((1, 20, 0), (1, 20, 255))]))
    return cases


F6_PAIRS = [(R.F6_CUTOFFS[i], R.F6_CUTOFFS[(i + 4) % len(R.F6_CUTOFFS)]) for i in range(len(R.F6_CUTOFFS))]
SCAN_CASES = scan_cases()
F6_CASES = [(name, [((0, a, 33), (0, b, 33)) for a, b in F6_PAIRS]) for name in ("F6short:0", "F6long:0")]


def rule_results(rows, setting, end=None, flags=0):
    """-> (the RESULT_DTYPE records the rule expects of one mate, its quality-trimmed bases)."""
    f, cutoff, base = setting
    start, stop, fl, cut = R.expected(rows, f, cutoff, base, end, flags)
    want = np.zeros(len(rows.lens), dtype=abi.RESULT_DTYPE)
    want["start"], want["stop"], want["flags"] = start, stop, fl
    return want, cut


def oracle_results(rows, ops, use_filter=True):
    tp = plan_of(ops, use_filter=use_filter)
    a1, n1, _a2, _n2 = tp.pack()
    res, _cap2, st = oracle.trim_mate(a1, n1, tp.params(), rows.seq, rows.qual, rows.lens, threads=THREADS)
    return res, st


def differ(got, want, rows, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: row {i} (length {int(rows.lens[i])}, qualities {rows.qual[i, :int(rows.lens[i])].tobytes()[-48:]!r}): "
                             f"{got[i]} != rule {want[i]} ({bad.size} of {len(want)} rows differ)")


# ---- ADAPTER plans (the resolve kernel and the scan kernel's deferred lanes): a 3' adapter in one read in four

ADAPTER, NEAR = "CGTC", "CGTCGTTGCAGC"


def planted(rows, copies):
    """Every fourth row ends in one of ``copies`` (in turn) where its string has room -> Rows (qualities untouched)."""
    seq = rows.seq.copy()
    lens = rows.lens.astype(np.int64)
    picks = np.arange(3, len(lens), 4)
    for j, copy in enumerate(copies):
        b = np.frombuffer(copy.encode(), dtype=np.uint8)
        sel = picks[j::len(copies)]
        sel = sel[lens[sel] - rows.f >= len(b)]
        for k in range(len(b)):
            seq[sel, lens[sel] - len(b) + k] = b[k]
    return R.Rows(seq, rows.qual, rows.lens, rows.f)


def adapter_op(seq, rate=0.0):
    return planmod.back(seq, rate, 3, flag=abi.CS_F_ADAPTER3)


def after_adapter(rows, op):
    """Where the adapter op alone leaves the interval's end, and its flags (the oracle: the aligner is not the rule's)."""
    res, _st = oracle_results(rows, [op])
    assert (res["start"] == 0).all()
    return res["stop"].astype(np.int64), res["flags"].astype(np.int64)


# ---- the rule itself

def test_rule_by_hand():
    assert R.stop(b"", 20) == 0
    assert R.stop(b"IIII", 20) == 4                     # good bases: the first sum is negative
    assert R.stop(b"II##", 20) == 2 and R.stop(b"####", 20) == 0
    assert R.stop(b"I#I#", 20) == 3                     # '#' adds 18, 'I' takes 20: 18, -2
    q = bytes(R.qbyte(d) for d in (0, +1, 0, 0))        # sums from the 3' end: 0, 0, 1, 1: first strict maximum at 1
    assert R.stop(q, 20) == 1
    q = bytes(R.qbyte(d) for d in (+1, -1, +1))         # 1, 0, 1: the tie keeps the first (3'-most) position
    assert R.stop(q, 20) == 2
    q = bytes(R.qbyte(d) for d in (+1, -1, -1, +1))     # 1, 0, -1: break; what lies below is never seen
    assert R.stop(q, 20) == 3
    # the two cases of the cutoff range (a 32-bit key of sum << 11 | position gets them wrong)
    assert R.stop(b"I" * 1500, 1000) == 0 and R.stop(b"I" * 40, 32767) == 0


@pytest.mark.parametrize("name,plans", SCAN_CASES + F6_CASES, ids=[c[0] for c in SCAN_CASES + F6_CASES])
def test_vectorised_rule_equals_the_loop_on_a_slice(name, plans):
    rows = build(name)
    step = max(1, len(rows.lens) // 400)
    pick = np.arange(0, len(rows.lens), step)
    for m1, m2 in plans[:2]:
        for f, cutoff, base in (m1, m2):
            start = np.minimum(f, rows.lens.astype(np.int64))
            got = R.stops(rows.qual[pick], start[pick], rows.lens[pick], cutoff, base)
            for k, i in enumerate(pick):
                s, e = int(start[i]), int(rows.lens[i])
                assert int(got[k]) == R.stop(rows.qual[i, s:e].tobytes(), cutoff, base), (name, int(i), f, cutoff, base)


# ---- what the families promise

def test_f1_reaches_every_stop_and_both_ends():
    for alphabet in R.ALPHABETS:
        rows = R.f1(0, alphabet)
        assert len(rows.lens) == 88573
        w = R.walks(rows.qual, 0, rows.lens, R.CUTOFF, R.BASE)
        n = rows.lens.astype(np.int64)
        for length in range(11):
            assert set(w.stop[n == length].tolist()) == set(range(length + 1)), (alphabet, length)
        assert (w.brk >= 0).any() and ((w.brk < 0) & (n > 0)).any()      # breaks before the start / never breaks
        assert ((w.brk >= 0) & (w.best >= 0)).any() and ((w.brk < 0) & (w.best >= 0)).any()
        if 0 in alphabet:  # a walk to the start on sums of exactly 0: nothing replaces the start key
            assert ((w.brk < 0) & (w.best < 0) & (n > 0)).any()
    for f in range(5):  # the interval's start at every offset inside a dword
        rows = R.f1(f)
        assert (rows.qual[:, :f] == R.PAD).all() and int(rows.lens.min()) == f and int(rows.lens.max()) == 10 + f


def f2_roles():
    """-> {role: set of (round, lane)} over both products and f = 0..3, and whether some read passes round 1 whole."""
    roles = {"break": set(), "best": set(), "skip1": set(), "skip2": set(), "skip3": set()}
    passes = False
    count = 0
    for product in "AB":
        for f in range(4):
            rows = build(f"F2{product}:{f}")
            count += len(rows.lens)
            end = rows.lens.astype(np.int64)
            start = np.minimum(f, end)
            w = R.walks(rows.qual, start, end, R.CUTOFF, R.BASE)
            live = end > start
            for role, pos, ok in (("break", w.brk, live & (w.brk >= 0)), ("best", w.best, live & (w.best >= 0))):
                g = R.geometry(start[ok], end[ok], pos[ok])
                roles[role] |= set(zip(g.round.tolist(), g.lane.tolist()))
            # the interval's lowest dword, where the walk gets there: no break, or the break inside that dword
            there = live & ((w.brk < 0) | ((w.brk >> 2) == (start >> 2)))
            g = R.geometry(start[there], end[there], start[there])
            if f:
                roles[f"skip{f}"] |= set(zip(g.round.tolist(), g.lane.tolist()))
            last = np.where(w.brk >= 0, w.brk, start)  # the lowest position the walk looks at
            passes = passes or bool((R.geometry(start[live], end[live], last[live]).rel > 16).any())
    return roles, passes, count


def test_f2_puts_every_lane_in_every_role():
    roles, passes, count = f2_roles()
    assert count == 2 * 136 * 4 * (121 + 13)
    both_rounds = {(r, lane) for r in (1, 2) for lane in range(16)}
    for role, seen in roles.items():
        assert both_rounds <= seen, (role, sorted(both_rounds - seen))
    assert passes


def alive_below_top(rows, f):
    """Rows whose walk goes on below the dword of the last base (what the wave serves four at a time)."""
    end = rows.lens.astype(np.int64)
    start = np.minimum(f, end)
    w = R.walks(rows.qual, start, end, R.CUTOFF, R.BASE)
    live = end > start
    safe_end = np.maximum(end, 1)
    below = R.geometry(start, safe_end, start).rel > 0
    brk_below = (w.brk < 0) | (R.geometry(start, safe_end, np.maximum(w.brk, 0)).rel > 0)
    return live & below & brk_below, w, start, end


@pytest.mark.parametrize("f", range(4))
def test_f3_has_the_designed_walkers_in_every_tile(f):
    rows, ks = R.f3(f)
    assert len(rows.lens) == 64 * len(ks) and len(ks) >= 30
    assert set(ks) == {1, 2, 3, 4, 5, 7, 64}
    alive, w, start, end = alive_below_top(rows, f)
    assert alive.reshape(-1, 64).sum(axis=1).tolist() == ks
    lanes = [tuple(np.flatnonzero(t).tolist()) for t in alive.reshape(-1, 64)]
    assert set(lanes) == set(R.F3_LANES)
    rounds = [set(R.geometry(start[t], end[t], w.brk[t]).round.tolist())
              for t in (np.flatnonzero(row) + 64 * i for i, row in enumerate(alive.reshape(-1, 64)))]
    assert any(r == {1, 2, 3} for r in rounds) and sum(len(r) == 1 for r in rounds) >= len(ks) // 2


def test_f4_reaches_both_sides_of_position_1024():
    rows = R.f4(0)
    assert 2000 < len(rows.lens) < 20000
    w = R.walks(rows.qual, 0, rows.lens, R.CUTOFF, R.BASE)
    for pos in (w.best, w.brk):
        assert {1022, 1023, 1024, 1025, 1026} <= set(pos.tolist())
    assert int(R.geometry(0, rows.lens.astype(np.int64), np.zeros(len(rows.lens), np.int64)).round.max()) == 24
    n = rows.lens.astype(np.int64)
    flat = slice(len(n) - 2 * len(R.F4_LENGTHS), None)
    sums93 = R.stops(rows.qual[flat], 0, n[flat], 93)
    assert sums93[0::2].tolist() == [0] * len(R.F4_LENGTHS) and sums93[1::2].tolist() == n[flat][1::2].tolist()


# ---- the oracle, the Python restatement and the rule

@pytest.mark.parametrize("name,plans", SCAN_CASES + F6_CASES, ids=[c[0] for c in SCAN_CASES + F6_CASES])
def test_oracle_equals_rule(name, plans):
    rows = build(name)
    for pair in plans:
        for setting in pair:
            want, cut = rule_results(rows, setting)
            got, st = oracle_results(rows, chain(*setting))
            differ(got, want, rows, f"{name} oracle (f, cutoff, base) = {setting}")
            assert int(st.qualtrim_bp) == cut and int(st.out_bp) == int((want["stop"].astype(np.int64) - want["start"]).sum())


@pytest.mark.parametrize("name", ["F1a:2", "F3:1", "F2B:3"])
def test_oracle_equals_rule_behind_an_adapter(name):
    rows = planted(build(name), [ADAPTER])
    op = adapter_op(ADAPTER)
    end, flags = after_adapter(rows, op)
    lens = rows.lens.astype(np.int64)
    hit = np.zeros(len(lens), dtype=bool)
    hit[3::4] = lens[3::4] - rows.f >= len(ADAPTER)
    assert hit.sum() > len(lens) // 8
    assert np.array_equal(end, np.where(hit, lens - len(ADAPTER), lens)) and np.array_equal(flags != 0, hit)
    for f in (rows.f, (rows.f + 1) % 4):
        want, cut = rule_results(rows, (f, 20, 33), end, flags)
        got, st = oracle_results(rows, [op] + chain(f, 20), use_filter=False)
        differ(got, want, rows, f"{name} oracle behind the adapter, f = {f}")
        assert int(st.qualtrim_bp) == cut


def test_pyref_equals_rule():
    body, ln = R.strings([R.qbyte(d) for d in R.ALPHABETS[0]], 8)
    texts = [b"I" * 40] + [body[i, :int(ln[i])].tobytes() for i in range(len(ln))]
    assert len(texts) == 1 + 9841
    for cutoff in (20, 19, 21) + R.F6_CUTOFFS:
        for q in texts:
            keep = R.stop(q, cutoff)
            got = pyref.quality_trim_index(q.decode("latin-1"), 0, cutoff)
            assert got == ((0, keep) if keep else (0, 0)), (q, cutoff)


def test_oracle_sums_in_64_bits():
    """-q 32767 on 70 000 bases of ``I``: a 32-bit sum wraps at 65 000 of them."""
    assert oracle.quality_trim_index("I" * 70000, 32767) == 0 == R.stop(b"I" * 70000, 32767)
    assert oracle.quality_trim_index("I" * 70000, -32768) == 70000


# ---- the clamp (cs_plan_create): outside [-1, 256] every term cutoff + base - byte has one sign

CLAMP_BYTES = (0, 33, 34, 53, 54, 73, 126, 127, 200, 255)
CLAMP_CUTOFFS = R.F6_CUTOFFS + (-36, 221, 225, 0, 20, 41)


def test_terms_have_one_sign_outside_the_clamp():
    for cq in (-2, -1, 256, 257):
        signs = {np.sign(cq - b) for b in range(256)}
        assert len(signs) == 1 and 0 not in signs
    for base in (0, 33, 64, 255):
        for cutoff in CLAMP_CUTOFFS:
            c = R.clamp(cutoff, base)
            assert -1 <= c + base <= 256 and (c == cutoff or not -1 <= cutoff + base <= 256)


def test_clamped_cutoff_changes_no_result():
    texts = [bytes(t) for L in range(4) for t in itertools.product(CLAMP_BYTES, repeat=L)]
    texts += [bytes(CLAMP_BYTES[int(ch)] for ch in f"{i * 7919 % 10 ** 12:012d}") for i in range(1889)]
    assert len(texts) == 3000 and len(CLAMP_CUTOFFS) == 15
    for q in texts:
        for cutoff in CLAMP_CUTOFFS:
            assert R.stop(q, cutoff) == R.stop(q, R.clamp(cutoff)), (q, cutoff)
    for rows in (R.f6_short(), R.f6_long(), R.f1_bytes(1, R.F5_EDGE_BYTES, max_len=8)):
        for base in (33, 64, 0, 255):
            for cutoff in CLAMP_CUTOFFS:
                assert np.array_equal(R.stops(rows.qual, 0, rows.lens, cutoff, base),
                                      R.stops(rows.qual, 0, rows.lens, R.clamp(cutoff, base), base)), (cutoff, base)
