"""The leading walk's quiet columns as cs_plan_create computes them (DevOp::quiet_groups, trim_kernel.hip.inc
quiet_columns) against a brute-force scan, column by column, of what may end where:

  * the 3' op (m rows, k errors, no free reference start) has a candidate in column j only if j >= m - k: row m of
    column j costs at least m - j; the columns Aligner.locate visits are all of them (free query ends);
  * the 5' op has one only where its table says T(j) >= 0 (DevOp::pair_tn, restated here from the thresholds).

Q is the largest multiple of eight with no 3' candidate in a column <= Q and T(j) = -1 for every j < Q.  Every 5' op
with m + k <= 31 (m, k, min_overlap: the merged walk takes no other) meets 3' ops whose m - k covers 1..32; short
adapters are kept in the walk with CUTSEQ_LOG_ALWAYS=1.  No GPU: a plan is host data."""
import ctypes as C

import pytest

from cutseq_amd import abi, capi, plan as planmod

import universe as U

BASES = "ACGT"


def dna(m, salt):
    return "".join(BASES[(i * 7 + salt * 3 + (i * i) // 5) % 4] for i in range(m))


def walk_info(L, ops1, ops2):
    tp = U.one_op_plan(ops1, ops2, abi.CS_SELECT_LEFTMOST, abi.CS_TIE_INSERTION)
    a1, n1, a2, n2 = tp.pack()
    params = tp.params()
    h = C.c_void_p()
    capi.check(L.cs_plan_create(C.cast(a1, C.c_void_p), n1, C.cast(a2, C.c_void_p), n2, C.byref(params), C.byref(h)))
    try:
        out = []
        for mate in (1, 2):
            info = (C.c_uint32 * 6)()
            capi.check(L.cs_plan_walk_info(h, mate, C.byref(info)))
            out.append(list(info))
        return out
    finally:
        L.cs_plan_destroy(h)


def t_of(op5, j):
    """T(j): the largest thr[i] over suffix lengths i in [min_overlap, m] with |i - j| <= thr[i]; k behind column m + k."""
    thr = op5.thresholds()
    if j > op5.m + op5.k:
        return op5.k
    return max([thr[i] for i in range(op5.min_overlap, op5.m + 1) if abs(i - j) <= thr[i]], default=-1)


def brute_q(op3, op5):
    if op3.where & abi.CS_REF_START:
        return 0
    cand3 = lambda j: j >= op3.m - op3.k
    q = 0
    while q + 8 <= 32 and not any(cand3(j) for j in range(0, q + 9)) and \
            (op5 is None or all(t_of(op5, j) < 0 for j in range(1, q + 8))):
        q += 8
    return q


@pytest.fixture(scope="module")
def lib():
    from cutseq_amd import build
    build.build()
    return capi.load()


def test_quiet_groups_of_every_pair_match_the_column_scan(lib, monkeypatch):
    monkeypatch.setenv("CUTSEQ_LOG_ALWAYS", "1")
    threes = [(m, k) for m in range(1, 33) for k in range(0, min(m, 8)) if (m + 3 * k) % 5 in (0, 2)]
    assert {m - k for m, k in threes} == set(range(1, 33))
    seen, at = set(), 0
    for m5 in range(1, 32):
        for k5 in range(0, min(m5, 15)):
            if m5 + k5 > 31:
                continue
            for mo5 in range(1, m5 + 1):
                chains, wants = [], []
                for _mate in range(2):
                    m3, k3 = threes[at % len(threes)]
                    at += 1
                    op5 = planmod.rightmost_front(dna(m5, at), U.rate_for(k5, m5), mo5, abi.CS_F_ADAPTER5)
                    op3 = planmod.back(dna(m3, at + 1), U.rate_for(k3, m3), min(3, m3), at % 11 == 0, abi.CS_F_ADAPTER3)
                    assert (op5.k, op3.k) == (k5, k3)
                    chains.append([op5, op3])
                    wants.append((op3, op5))
                for info, (op3, op5) in zip(walk_info(lib, *chains), wants):
                    assert info[0] == 2, (op5, op3)
                    tn = [(info[2 + (j - 1) // 8] >> (4 * ((j - 1) % 8))) & 15 for j in range(1, 33)]
                    assert tn == [t_of(op5, j) + 1 for j in range(1, 33)], (op5, op3)
                    q = brute_q(op3, op5)
                    assert info[1] * 8 == q, (op5, op3, info, q)
                    seen.add(q)
    assert seen == {0, 8, 16, 24}


def test_quiet_groups_of_a_lone_forward_op(lib, monkeypatch):
    monkeypatch.setenv("CUTSEQ_LOG_ALWAYS", "1")
    ops = [(m, k, anywhere) for m in range(1, 33) for k in range(0, min(m, 9)) for anywhere in (False, True)]
    for lo in range(0, len(ops), 2):
        pair = [planmod.back(dna(m, m + k), U.rate_for(k, m), min(3, m), anywhere, abi.CS_F_ADAPTER3) for m, k, anywhere in ops[lo:lo + 2]]
        for info, op in zip(walk_info(lib, [pair[0]], [pair[1]]), pair):
            assert info[0] == 1, op
            assert info[1] * 8 == brute_q(op, None), (op, info)
            assert info[2:] == [0, 0, 0, 0]


def test_no_quiet_groups_without_the_walk(lib, monkeypatch):
    """An op the item log would not take (a short adapter with a loose bound) keeps the op loop's filter: no walk, Q = 0;
    so does a chain under CUTSEQ_PAIR=0."""
    loose = planmod.back(dna(12, 1), U.rate_for(3, 12), 3, False, abi.CS_F_ADAPTER3)
    assert walk_info(lib, [loose], [loose]) == [[0] * 6, [0] * 6]
    op5 = planmod.rightmost_front(dna(20, 2), U.rate_for(2, 20), 10, abi.CS_F_ADAPTER5)
    op3 = planmod.back(dna(20, 3), U.rate_for(4, 20), 3, False, abi.CS_F_ADAPTER3)
    assert [i[:2] for i in walk_info(lib, [op5, op3], [op5, op3])] == [[2, 1], [2, 1]]  # (TAKARAV3's shape: Q = 8)
    monkeypatch.setenv("CUTSEQ_PAIR", "0")
    assert walk_info(lib, [op5, op3], [op5, op3]) == [[0] * 6, [0] * 6]
