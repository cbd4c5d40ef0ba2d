"""The edges of the scan kernel's leading walk (trim_kernel.hip.inc, myers_pair) and of the tile staging in front of it,
held to the C oracle bit for bit:

  * the quiet leading groups (DevOp::quiet_groups, Q columns): 3' ops with m - k of 7, 8, 9, 16 and 17 and 5' ops whose
    T(j) turns >= 0 at, in front of and behind a group boundary -- Q = 0, 8 and 16, checked through cs_plan_walk_info;
  * the columns behind the last whole group: every read length 1..41 and 149..152, as tiles of 64 equal reads, as tiles
    with one lane of another length and as fully mixed tiles;
  * planted hits at the seams: a 3' adapter whose alignment ends exactly in column Q, Q + 1, ..., m - k (the first
    column that can hold one), n - 1 and n, 5' partial hits that end in columns Q and Q + 1;
  * the staging forms: row strides 152 (the coded tile is linear in the source), 160 (padded) and 8 (rows shorter
    than a quad), from a 16-byte aligned base and from one four bytes off, 'N' padding (the fast re-coding) and zero
    padding (the exact re-coding).

Every case: a few thousand reads, the plan with the filter on, with the filter off, and with CUTSEQ_PAIR=0 (the two
scans apart) -- all three equal to the oracle, so equal to each other.  Short adapters stay in the walk through
CUTSEQ_LOG_ALWAYS=1 (their candidates may flood the item log: those reads take the resolve kernel, same results)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import oracle
from cutseq_amd import abi, capi, plan as planmod
from cutseq_amd.engine import TrimEngine

import universe as U

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, oracle.host_threads()))
TILE = 64
LENGTHS = list(range(1, 42)) + [149, 150, 151, 152]
RULE, TIE = abi.CS_SELECT_LEFTMOST, abi.CS_TIE_INSERTION


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


class Chain:
    """A 5' + 3' pair (or a lone 3' op: m5 == 0) and what its walk must look like."""

    def __init__(self, seed, m3, k3, m5=0, k5=0, mo5=0, anywhere=False, q=0):
        rng = random.Random(seed)
        self.a3, self.a5, self.q, self.m3, self.k3, self.mo5 = dna(rng, m3), dna(rng, m5), q, m3, k3, mo5
        self.ops = [planmod.back(self.a3, U.rate_for(k3, m3), 3, anywhere, abi.CS_F_ADAPTER3)]
        if m5:
            self.ops.insert(0, planmod.rightmost_front(self.a5, U.rate_for(k5, m5), mo5, abi.CS_F_ADAPTER5))
        assert self.ops[-1].k == k3 and (not m5 or self.ops[0].k == k5)

    def __repr__(self):
        return f"Chain(3' {self.a3} k={self.k3}, 5' {self.a5} min_overlap={self.mo5}, Q={self.q})"

    def plant(self, rng, n):
        """A read of length n with one of the seam hits (or none)."""
        read = list(dna(rng, n))
        kind = rng.randrange(8)
        a3, m3 = self.a3, self.m3
        if kind == 0:  # the 3' adapter's tail at the read's start: its alignment ends in column c
            c = rng.choice([self.q, self.q + 1, m3 - self.k3 - 1, m3 - self.k3, m3 - self.k3 + 1, m3])
            c = max(1, min(c, m3, n))
            read[:c] = a3[m3 - c:]
        elif kind == 1:  # the whole adapter, ending in column c near the first one that can hold it
            c = min(n, m3 + rng.choice([0, 1, 2, 8 - m3 % 8]))
            if c >= m3:
                read[c - m3:c] = a3
        elif kind in (2, 3):  # ... ending in column n - 1 or n (a read shorter than the adapter: its head, cut at the end)
            c = n - (kind - 2)
            if c >= 1:
                lo = max(0, c - m3)
                read[lo:c] = a3[:c - lo]
        elif kind == 4 and self.a5:  # a 5' partial hit: the adapter's last x bases in front, x = Q or Q + 1 (or min_overlap)
            x = rng.choice([self.q, self.q + 1, self.mo5, len(self.a5)])
            x = max(1, min(x, len(self.a5), n))
            read[:x] = self.a5[len(self.a5) - x:]
        if kind < 5 and rng.random() < 0.4 and n > 2:  # ... with one error somewhere in front
            p = rng.randrange(min(n, 30))
            what = rng.randrange(3)
            if what == 0:
                read[p] = rng.choice("ACGT")
            elif what == 1:
                read.insert(p, rng.choice("ACGT"))
            else:
                del read[p]
        return "".join(read)[:n].ljust(n, "A")


def lengths_by_layout(rng, lengths):
    """Tiles of 64 equal reads, tiles with one lane of another length, fully mixed tiles."""
    out = []
    for n in lengths:
        out += [n] * TILE
    for i, n in enumerate(lengths):
        tile = [n] * TILE
        tile[(i * 11 + 5) % TILE] = lengths[(i * 7 + 3) % len(lengths)] if len(lengths) > 1 else n
        out += tile
    out += [rng.choice(lengths) for _ in range(len(lengths) * TILE)]
    return out


def make_reads(seed, chains, stride, pad):
    rng = random.Random(seed)
    lens = lengths_by_layout(rng, [n for n in LENGTHS if n <= stride])
    seq = np.full((len(lens), stride), pad, dtype=np.uint8)
    qual = np.full((len(lens), stride), pad and ord("I"), dtype=np.uint8)
    for i, n in enumerate(lens):
        seq[i, :n] = np.frombuffer(rng.choice(chains).plant(rng, n).encode(), dtype=np.uint8)
        qual[i, :n] = ord("I")
    return seq, qual, np.array(lens, dtype=np.uint16)


class OnDevice:
    """The reads on the device, the sequence rows `offset` bytes behind a 16-byte aligned address; both mates read them."""

    def __init__(self, seq, qual, lens, offset):
        dev = torch.device("cuda:0")
        self.seq, self.qual, self.lens = seq, qual, lens
        self.n, self.stride = seq.shape
        self.buf = torch.zeros(seq.size + 32, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.buf[offset:offset + seq.size].copy_(torch.from_numpy(seq.reshape(-1)))
        self.t = [torch.from_numpy(qual).to(dev), torch.from_numpy(lens.view(np.int16)).to(dev)]
        self.out = [torch.zeros((self.n, 8), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.r = [abi.cs_reads(self.buf.data_ptr() + offset, self.t[0].data_ptr(), self.t[1].data_ptr(), o.data_ptr(), None, None)
                  for o in self.out]
        self.stream = torch.cuda.Stream(device=dev)

    def run(self, tp):
        for o in self.out:
            o.fill_(0xEE)
        with TrimEngine(tp, device=0, slots=0) as eng:
            info = []
            for mate in (1, 2):
                w = (C.c_uint32 * 6)()
                capi.check(eng.L.cs_plan_walk_info(eng._plan_h, mate, C.byref(w)))
                info.append(list(w))
            eng.trim_device(self.r[0], self.r[1], self.n, self.stride, stream=C.c_void_p(self.stream.cuda_stream))
            self.stream.synchronize()
        return [o.cpu().numpy().view(abi.RESULT_DTYPE).reshape(-1).copy() for o in self.out], info

    def expect(self, tp):
        a1, n1, a2, n2 = tp.pack()
        params = tp.params()
        want = [np.zeros(self.n, dtype=abi.RESULT_DTYPE) for _ in range(2)]
        oracle.trim_mate(a1, n1, params, self.seq, self.qual, self.lens, threads=THREADS, out=want[0])
        oracle.trim_mate(a2, n2, params, self.seq, self.qual, self.lens, threads=THREADS, out=want[1])
        return want


def check(monkeypatch, chains, stride=152, offset=0, pad=ord("N"), seed=1):
    seq, qual, lens = make_reads(seed, chains, stride, pad)
    assert 1000 <= len(lens) <= 10000
    dev = OnDevice(seq, qual, lens, offset)
    monkeypatch.setenv("CUTSEQ_LOG_ALWAYS", "1")
    want = None
    for form in ("filter", "no filter", "CUTSEQ_PAIR=0"):
        tp = U.one_op_plan(chains[0].ops, chains[1].ops, RULE, TIE, use_filter=form != "no filter")
        if form == "CUTSEQ_PAIR=0":
            monkeypatch.setenv("CUTSEQ_PAIR", "0")
        want = want or dev.expect(tp)
        got, info = dev.run(tp)
        for mate in (0, 1):
            if form == "filter":  # the walk is what runs, with the quiet groups the case is about
                assert info[mate][:2] == [2 if chains[mate].a5 else 1, chains[mate].q // 8], (chains[mate], info[mate])
            elif form == "CUTSEQ_PAIR=0":
                assert info[mate][:2] == [0, 0]
            if not np.array_equal(got[mate], want[mate]):
                i = int(np.flatnonzero(got[mate] != want[mate])[0])
                raise AssertionError(f"{chains[mate]} {form}: read {i} {seq[i, :lens[i]].tobytes().decode()!r} (n = {lens[i]}): device "
                                     f"{got[mate][i]} != oracle {want[mate][i]} ({int((got[mate] != want[mate]).sum())} of {len(lens)} differ)")


# 3' (m, k) with m - k = 7, 8, 9, 16, 17; 5' (m, k, min_overlap): T(j) >= 0 from column min_overlap - thr[min_overlap] on
PAIRS = {
    "m-k=7,Q=0": dict(m3=8, k3=1, m5=20, k5=2, mo5=10, q=0),
    "m-k=8,Q=0": dict(m3=9, k3=1, m5=20, k5=2, mo5=10, q=0),
    "m-k=9,Q=8": dict(m3=10, k3=1, m5=20, k5=2, mo5=10, q=8),       # T(9) >= 0: column 8 is clear
    "m-k=9,Q=8,T(8)": dict(m3=11, k3=2, m5=20, k5=2, mo5=9, q=8),   # T(8) >= 0: the last quiet column is tested
    "m-k=16,Q=8": dict(m3=20, k3=4, m5=20, k5=2, mo5=10, q=8),      # the shape of the chains the reference compiles
    "m-k=17,Q=8": dict(m3=19, k3=2, m5=20, k5=2, mo5=17, q=8),      # T(15) >= 0 keeps the second group out
    "m-k=17,Q=16": dict(m3=19, k3=2, m5=20, k5=2, mo5=18, q=16),    # T(16) >= 0, T(15) = -1
    "m-k=16,T early,Q=0": dict(m3=20, k3=4, m5=20, k5=2, mo5=3, q=0),  # T(3) >= 0: no quiet column
    "m-k=16,free start,Q=0": dict(m3=20, k3=4, m5=20, k5=2, mo5=10, anywhere=True, q=0),
    "m-k=25,Q=24": dict(m3=27, k3=2, m5=28, k5=1, mo5=26, q=24),
    "lone m-k=17,Q=16": dict(m3=19, k3=2, q=16),
    "lone m-k=9,Q=8": dict(m3=10, k3=1, q=8),
}
BENCH = ("m-k=16,Q=8", "m-k=17,Q=16")


@pytest.mark.parametrize("names", [("m-k=7,Q=0", "m-k=8,Q=0"), ("m-k=9,Q=8", "m-k=9,Q=8,T(8)"), ("m-k=16,Q=8", "m-k=17,Q=8"),
                                   ("m-k=17,Q=16", "m-k=16,T early,Q=0"), ("m-k=16,free start,Q=0", "m-k=25,Q=24"),
                                   ("lone m-k=17,Q=16", "lone m-k=9,Q=8")])
def test_quiet_groups_and_tails_against_the_oracle(names, monkeypatch):
    chains = [Chain(11 + i, **PAIRS[name]) for i, name in enumerate(names)]
    check(monkeypatch, chains)


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("stride", [152, 160, 8])
def test_staging_forms_against_the_oracle(stride, offset, monkeypatch):
    chains = [Chain(21 + i, **PAIRS[name]) for i, name in enumerate(BENCH)]
    check(monkeypatch, chains, stride=stride, offset=offset, seed=2)


@pytest.mark.parametrize("stride", [152, 160])
def test_zero_padding_takes_the_exact_recoding(stride, monkeypatch):
    chains = [Chain(31 + i, **PAIRS[name]) for i, name in enumerate(BENCH)]
    check(monkeypatch, chains, stride=stride, pad=0, seed=3)
