"""CPU side of the demultiplexing enumeration (tests/demux_rule.py): what the oracle's B runs say on every read of the
universes (and that the universes hold what they must, so nothing below passes vacuously), and the library's host walk
-- the candidate lists of ``cs_plan_set_demux_ops``, read through ``cs_plan_demux_view`` -- against those runs: a
barcode missing from a list is a read silently left unassigned, a list out of order is a read in the wrong file.  The
GPU file (tests/test_gpu_demux_enumerated.py) then holds the kernels to the same expectation, read by read.
"""
import functools
import itertools
import random

import numpy as np
import pytest

import oracle
from cutseq_amd import abi, demux

import demux_rule as D
import util

THREADS = max(1, min(8, oracle.host_threads()))


@pytest.fixture(scope="module", autouse=True)
def lib():
    from cutseq_amd import build, capi
    build.build()
    return capi.load()


@functools.lru_cache(maxsize=None)
def reads(name: str):
    return D.reads_of(D.UNIVERSES[name])


@functools.lru_cache(maxsize=None)
def expected(name: str, which: str, at_end: bool = False) -> D.Expected:
    """Computed once, shared by the tests below."""
    u = D.UNIVERSES[name]
    return D.expect(u.sets()[which], u.rate, reads(name), at_end=at_end, threads=THREADS)


@functools.lru_cache(maxsize=None)
def lists(name: str, which: str, at_end: bool = False) -> D.Lists:
    u = D.UNIVERSES[name]
    return D.library_lists(u.sets()[which], u.rate, at_end)


CASES = [(name, which) for name in D.UNIVERSES for which in ("crowded", "spread", "single")]


def test_the_universes_and_barcode_sets_are_what_they_say():
    for name, u in D.UNIVERSES.items():
        seq, qual, lens = reads(name)
        assert len(lens) == u.reads == sum(len(u.alphabet) ** L for L in range(u.span + 1))
        assert u.k == int(u.rate * u.m) and int(lens.max()) == u.span and seq.shape[1] % 4 == 0
        assert len({seq[i, :lens[i]].tobytes() for i in range(0, len(lens), 997)}) == len(range(0, len(lens), 997))
        assert np.all(qual == ord("I")) and np.all(seq[np.arange(seq.shape[1])[None, :] >= lens[:, None]] == ord("N"))
        centre = u.crowded[D.CENTRE_AT[name]]
        assert u.single == (centre,) and centre in u.spread
        flip = {"A": "C", "C": "A", "G": "T", "T": "G"}
        near = [flip[centre[0]] + centre[1:], centre[:-1] + flip[centre[-1]]]
        assert near == list(u.crowded[:2])
        two = u.crowded[2]
        assert sum(a != b for a, b in zip(two, centre)) in ((1, 2) if name == "U1" else (2,))  # (U1: the set as first tried)
        assert u.crowded[3][:-1] == centre[1:] and u.crowded[4][1:] == centre[:-1]  # one base to either side
        assert any(len(set(c)) == 1 for c in u.crowded) and any(c == (c[:2] * u.m)[:u.m] and c[0] != c[1] for c in u.crowded)
        assert all(D.edit_distance(a, b) >= 3 for a, b in itertools.combinations(u.spread, 2)) and len(u.spread) >= 4
        for codes in u.sets().values():
            assert len(set(codes)) == len(codes) and all(len(c) == u.m and set(c) <= set("ACGT") for c in codes)
    assert D.to_tg(D.U2.crowded)[0] == "GGGTGTTGTGG"
    tg = D.reads_of(D.U2, tg=True)[0]
    assert set(np.unique(tg)) == {ord("T"), ord("G"), ord("N")}


def test_the_table_index_is_the_headers():
    """``table_index`` against the layout ``cutseq_amd/demux.py`` lays its prefixes out in: a bijection of U1 onto the
    table of m + k = 7, and the prefix at a read's index is the read."""
    seq, _qual, lens = reads("U1")
    idx = D.table_index(seq, lens, D.U1.span)
    assert np.array_equal(np.sort(idx), np.arange(demux.table_entries(D.U1.span)))
    pseq, plens = demux.all_prefixes(D.U1.span)
    assert np.array_equal(plens[idx], lens)
    inside = np.arange(pseq.shape[1])[None, :] < lens[:, None]
    assert np.array_equal(np.where(inside, pseq[idx], 0), np.where(inside, seq[:, :pseq.shape[1]], 0))
    # by hand: "" -> 0; "C" -> 1 + 1; "AT" -> 6 + 0 + 2 * 5; lower case folds or is "other"; the last bases, last first
    rows, rl = util.pack_reads([("", ""), ("C", "I"), ("AT", "II"), ("at", "II"), ("GATTC", "IIIII")])[::2]
    assert D.table_index(rows, rl, 3).tolist() == [0, 2, 16, 16, 31 + 3 + 0 + 2 * 25]
    assert D.table_index(rows, rl, 3, fold=False).tolist()[3] == 6 + 4 + 4 * 5
    assert D.table_index(rows, rl, 3, at_end=True).tolist() == [0, 2, 6 + 2 + 0, 6 + 2 + 0, 31 + 1 + 2 * 5 + 2 * 25]
    assert D.table_index(rows, rl, 3, start=1).tolist() == [0, 0, 1 + 2, 1 + 2, 31 + 0 + 2 * 5 + 2 * 25]


@pytest.mark.parametrize("name", list(D.UNIVERSES))
def test_the_crowded_universes_are_not_vacuous(name):
    """On the oracle's expectation alone, before anything is compared with it.  Measured with the sets of demux_rule.py
    (matched reads, ambiguous reads, reads whose exact copy is not the lowest matching index, most claimants, cuts):
    U1 2.2 %, 248, 13, 6, 5..7; U2 2.4 %, 17 022, 65, 7, 9..13; U3 79.8 %, 1 276 384, 186, 7, 12..20."""
    u = D.UNIVERSES[name]
    e = expected(name, "crowded")
    claimants = e.matched.sum(axis=0)
    assigned = e.bc != D.NONE
    assert np.array_equal(assigned, claimants > 0) and e.assigned == int(assigned.sum())
    beaten = e.exact.any(axis=0) & (e.exact.argmax(axis=0) != e.matched.argmax(axis=0))
    cuts = sorted(set(e.res["start"][assigned].tolist()))
    print(name, f"matched {assigned.mean():.3%} ambiguous {int((claimants > 1).sum())} exact-not-lowest {int(beaten.sum())} "
                f"most claimants {int(claimants.max())} cuts {cuts}")
    assert int((claimants > 1).sum()) >= 100
    assert int(beaten.sum()) >= 10
    assert np.all(e.bc[beaten] == e.exact.argmax(axis=0)[beaten]) and np.all(e.bc[beaten] > e.matched.argmax(axis=0)[beaten])
    assert cuts == list(range(u.m - u.k, u.m + u.k + 1))
    assert int(claimants.max()) >= 5
    assert np.array_equal((e.res["flags"] & abi.CS_F_AMBIGUOUS) != 0, claimants > 1)
    if name != "U1":  # the lists prune on nine bases of up to m + k: some nine-base prefix needs three barcodes or more
        li = lists(name, "crowded")
        assert li.depth == 9 < u.span
        seq, _q, lens = reads(name)
        need = D.required_lists(e.matched, D.table_index(seq, lens, 9), D.slots_of(9))
        assert int(need[:, D.slots_of(8):].sum(axis=0).max()) >= 3
    else:
        assert lists(name, "crowded").depth == u.span == 7


def check_superset(li: D.Lists, e: D.Expected, batch, at_end: bool, what):
    """Both halves of the claim, over every read: a read shorter than ``depth`` finds every barcode that matches it in
    the list of its own slot; a longer read finds, in the list of its ``depth``-base prefix, every barcode that matches
    ANY read of the universe with that prefix."""
    seq, _q, lens = batch
    slot = D.table_index(seq, lens, li.depth, at_end=at_end)
    member = li.member(e.matched.shape[0])
    for short in (True, False):
        mine = (lens < li.depth) == short
        assert mine.any()
        need = D.required_lists(e.matched[:, mine], slot[mine], len(li.first))
        lost = need & ~member
        assert not lost.any(), (what, "short" if short else "long", int(lost.sum()), np.argwhere(lost)[:3].tolist())
    return member


@pytest.mark.parametrize("name,which", CASES)
def test_every_list_holds_every_barcode_the_oracle_matches(name, which):
    """U1, U2 and U3 under every barcode set: the superset, the shape of the lists, and -- more than the superset -- the
    lists are exactly the barcodes a plain edit-distance table leaves alive (so a slot no barcode can match is 0)."""
    u = D.UNIVERSES[name]
    codes = u.sets()[which]
    li = lists(name, which)
    assert li.depth == min(u.span, 9)
    li.check_shape(len(codes))
    member = check_superset(li, expected(name, which), reads(name), False, (name, which))
    plain = D.alive_plain(codes, u.k, li.depth, prune=name != "U1")
    assert np.array_equal(member, plain)
    assert np.array_equal(li.first == 0, ~plain.any(axis=0))
    if name == "U1":
        assert np.array_equal(plain, D.alive_plain(codes, u.k, li.depth, prune=True))


@pytest.mark.parametrize("name,which", [("U1", "crowded"), ("U1", "spread"), ("U1", "single"), ("U2", "crowded")])
def test_the_lists_of_a_3prime_op_hold_every_barcode_the_suffix_runs_match(name, which):
    """``at_end``: SuffixAdapter runs; the lists are indexed by the read's last bases, last base first."""
    u = D.UNIVERSES[name]
    codes = u.sets()[which]
    li = lists(name, which, True)
    li.check_shape(len(codes))
    e = expected(name, which, True)
    assert e.assigned > 0 and (which != "crowded" or int((e.matched.sum(axis=0) > 1).sum()) >= 100)
    L = reads(name)[2].astype(np.int64)
    assert np.all((e.res["start"] == 0) & ((e.bc == D.NONE) | (L - e.res["stop"] >= u.m - u.k)))
    member = check_superset(li, e, reads(name), True, (name, which, "at_end"))
    assert np.array_equal(member, D.alive_plain(codes, u.k, li.depth, at_end=True, prune=True))
    # the 5' lists of the reversed barcodes: the same table
    assert np.array_equal(member, D.library_lists([c[::-1] for c in codes], u.rate).member(len(codes)))


def barcodes_255():
    """The 255 x 20-base set of test_gpu_demux.py::test_demux_equals_independent_runs (same seed, same draws, same
    acceptance rule; the distances of a candidate to every accepted barcode at once)."""
    rng = random.Random(20 * 100 + 255)
    codes, have = [], np.zeros((0, 20), dtype=np.uint8)
    while len(codes) < 255:
        c = util.random_dna(rng, 20)
        row = np.frombuffer(c.encode(), dtype=np.uint8)
        prev = np.tile(np.arange(21), (len(codes), 1))
        for i in range(1, 21):  # rows: the candidate's bases; columns: the accepted barcodes' bases
            cur = np.empty_like(prev)
            cur[:, 0] = i
            for j in range(1, 21):
                cur[:, j] = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + (have[:, j - 1] != row[i - 1]))
            prev = cur
        if np.all(prev[:, 20] >= 4):
            codes.append(c)
            have = np.vstack([have, row[None, :]])
    return codes


def test_the_depth_fallback_keeps_the_superset():
    """255 barcodes of 20 bases with four errors: the lists of nine-base prefixes exceed the table format and the library
    settles for shorter prefixes.  2 000 planted reads with 0..5 edits each (substitutions, insertions, deletions; every
    other read has its first edit within the first nine bases) against 255 oracle runs."""
    codes = barcodes_255()
    assert len(set(codes)) == 255 and all(D.edit_distance(a, b) >= 4 for a, b in itertools.combinations(codes[:24], 2))
    li = D.library_lists(codes, 0.2)
    assert 1 <= li.depth < 9
    li.check_shape(255)
    rng = random.Random(5)
    rows, edits, early = [], [], []
    for i in range(2000):
        s = list(codes[rng.randrange(255)])
        n_edits = i % 6
        for e in range(n_edits):
            at = rng.randrange(min(9, len(s))) if (e == 0 and i % 2) else rng.randrange(len(s))
            kind = "sid"[(i // 6 + e) % 3]
            if kind == "s":
                s[at] = rng.choice("ACGT".replace(s[at], ""))
            elif kind == "i":
                s.insert(at, rng.choice("ACGT"))
            else:
                del s[at]
        seq = "".join(s) + util.random_dna(rng, 32 - len(s))
        rows.append((seq, "I" * 32))
        edits.append(n_edits)
        early.append(bool(n_edits and i % 2))
    batch = util.pack_reads(rows)
    e = D.expect(codes, 0.2, batch, threads=THREADS)
    edits, early = np.array(edits), np.array(early)
    hit = e.bc != D.NONE
    assert all(hit[edits == n].mean() > 0.9 for n in range(5)) and 0 < hit[edits == 5].mean() < 1  # at k and at k + 1
    assert int((hit & early).sum()) >= 500
    slot = D.table_index(batch[0], batch[2], li.depth)
    need = D.required_lists(e.matched, slot, len(li.first))
    assert not (need & ~li.member(255)).any()


def test_the_lists_do_not_depend_on_the_thread_count(monkeypatch):
    """subtrees on host threads, merged in pre-order -- the same table whatever the count."""
    rng = random.Random(8)
    plex = sorted({util.random_dna(rng, 16) for _ in range(96)})  # (many subtrees with work in them: k = 3)
    for codes, rate in ((D.U3.crowded, D.U3.rate), (D.U2.crowded, D.U2.rate), (D.U1.crowded, D.U1.rate), (plex, 0.2)):
        got = []
        for threads in ("1", "8"):
            monkeypatch.setenv("CUTSEQ_HOST_THREADS", threads)
            got.append(D.library_lists(codes, rate))
        assert got[0].depth == got[1].depth and len(got[0].pool) > 0
        assert got[0].first.tobytes() == got[1].first.tobytes() and got[0].pool.tobytes() == got[1].pool.tobytes()


def test_the_walk_restated_equals_the_library_and_every_planted_defect_shows():
    """The checks above are not decoration: ``walk_model`` (the comment above ``DemuxWalk``, restated) produces the
    library's table on U1 and U2, and each planted defect -- a band of k - 1, the cap at k, ``done`` forgotten, row 0 left
    at the fill -- loses a barcode that the oracle matches: the superset check fails on some universe."""
    fails = {d: [] for d in D.DEFECTS}
    for name in ("U1", "U2"):
        u = D.UNIVERSES[name]
        li, e = lists(name, "crowded"), expected(name, "crowded")
        seq, _q, lens = reads(name)
        member = li.member(len(u.crowded))
        assert np.array_equal(D.walk_model(u.crowded, u.k, li.depth), member)
        need = D.required_lists(e.matched, D.table_index(seq, lens, li.depth), len(li.first))
        assert not (need & ~member).any()
        for d in D.DEFECTS:
            if (need & ~D.walk_model(u.crowded, u.k, li.depth, defect=d)).any():
                fails[d].append(name)
    print(fails)
    assert all(fails.values()), fails
    assert set(fails["done_forgotten"]) == {"U1"}  # (U2's shortest match ends at base nine, where its table ends)


def test_the_view_refuses_what_has_no_lists(lib):
    """cs_plan_demux_view: CS_ERR_ARG for an op of the table form, for a by-ops op whose ops are not attached yet, for an
    op that is no demultiplexer, for a missing op or output; the pointers of a good call go into the plan's own storage."""
    import ctypes as C
    from cutseq_amd import plan as planmod

    def create(tp):
        a1, n1, _a2, _n2 = tp.pack()
        params, h = tp.params(), C.c_void_p()
        assert lib.cs_plan_create(C.cast(a1, C.c_void_p), n1, None, 0, C.byref(params), C.byref(h)) == 0
        return h

    depth, n_first, n_pool = C.c_int(), C.c_size_t(), C.c_size_t()
    first, pool = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
    outs = (C.byref(depth), C.byref(first), C.byref(n_first), C.byref(pool), C.byref(n_pool))
    h = create(D.demux_chain(D.U1.crowded, D.U1.rate, "table", behind=(planmod.prefix("ACGT", 0.0),)))
    assert lib.cs_plan_demux_view(h, 1, 0, *outs) == abi.CS_ERR_ARG  # the table form
    assert lib.cs_plan_demux_view(h, 1, 1, *outs) == abi.CS_ERR_ARG  # an adapter op
    assert lib.cs_plan_demux_view(h, 1, 2, *outs) == abi.CS_ERR_ARG and lib.cs_plan_demux_view(h, 2, 0, *outs) == abi.CS_ERR_ARG
    lib.cs_plan_destroy(h)
    tp = D.demux_chain(D.U1.crowded, D.U1.rate, "ops5")
    h = create(tp)
    assert lib.cs_plan_demux_view(h, 1, 0, *outs) == abi.CS_ERR_ARG  # nothing attached yet
    ops = planmod.pack_ops(tp.demux.barcode_ops(), limit=255)
    assert lib.cs_plan_set_demux_ops(h, 1, 0, C.cast(ops, C.c_void_p), len(D.U1.crowded)) == 0
    assert lib.cs_plan_demux_view(h, 1, 0, C.byref(depth), None, C.byref(n_first), C.byref(pool), C.byref(n_pool)) == abi.CS_ERR_ARG
    assert lib.cs_plan_demux_view(h, 1, 0, *outs) == 0
    assert depth.value == 7 and n_first.value == D.slots_of(7) and n_pool.value == len(lists("U1", "crowded").pool)
    again = C.POINTER(C.c_uint32)()
    assert lib.cs_plan_demux_view(h, 1, 0, C.byref(depth), C.byref(again), C.byref(n_first), C.byref(pool), C.byref(n_pool)) == 0
    assert C.addressof(again.contents) == C.addressof(first.contents)  # a view, not a copy
    assert bytes(C.string_at(pool, n_pool.value)) == lists("U1", "crowded").pool.tobytes()
    lib.cs_plan_destroy(h)
