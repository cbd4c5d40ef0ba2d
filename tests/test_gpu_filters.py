"""-M/--max-length (TooLong) and --max-ee (TooManyExpectedErrors) in the trimming kernels: every kernel path flags the
reads (cs_reads.xflags) and counts them per mate (cs_xflag_counts_fetch) as the rules of tests/filters_rule.py say,
applied to the oracle's intervals -- the oracle knows nothing of filters.  The text path and the CLI:
tests/test_gpu_filters_cli.py."""
import math
import random

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, synth, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig
from cutseq_amd.engine import TrimEngine

import filters_rule
import util

pytestmark = pytest.mark.gpu

ADAPTER = "AGATCGGAAGAGCACACGTC"
RAW_ADAPTER = "AGATCGGAAGAGCNCACGTC"  # not all A/C/G/T: the plan is not coded, its tiles stay raw bytes
FILL = 0xAA


def qualities(rng: random.Random, length: int, k: int) -> str:
    """All of 33..126; every seventh row holds one value (the two ends of the range among them)."""
    if k % 7 == 0:
        return chr((33, 126, 40, 75)[(k // 7) % 4] if (k // 7) % 5 else rng.randint(33, 126)) * length
    return "".join(chr(rng.randint(33, 126)) for _ in range(length))


def adapter_reads(seed: int, lengths, adapter: str = ADAPTER, edits: int = 2, with_n: float = 0.1):
    """Reads for a single 3' adapter plan: three in four carry the adapter (whole or cut off by the read's end, up to
    ``edits`` edits) behind an insert of any length, so the final interval ends anywhere in the row, is empty (adapter
    at position 0, or an empty read) or spans the row (no adapter)."""
    rng = random.Random(seed)
    reads = []
    for k, length in enumerate(lengths):
        s = util.random_dna(rng, length)
        if rng.random() < 0.75:  # (well over half: the median final length lies below the read length)
            insert = rng.randint(0, length)
            s = (s[:insert] + util.mutate(rng, adapter.replace("N", "A"), rng.randint(0, edits)) + util.random_dna(rng, length))
        s = s[:length]
        if rng.random() < with_n and length:
            j = rng.randrange(length)
            s = s[:j] + "N" * min(rng.randint(1, 4), length - j) + s[j + 4:]
            s = (s + util.random_dna(rng, length))[:length]
        reads.append((s, qualities(rng, length, k)))
    return reads


def short_lengths(seed: int, top: int = 72, each: int = 28):
    lengths = [length for length in range(top + 1) for _ in range(each)]
    random.Random(seed).shuffle(lengths)
    return lengths


def takara_batch(n: int, read_len: int, seed: int, clip: bool):
    """The generator's TAKARAV3 pairs with qualities from all of 33..126; ``clip``: a third of the reads cut to a random
    length from 0 on."""
    batch = synth.generate_pairs(n, read_len, scheme=BUILDIN_ADAPTERS["TAKARAV3"], seed=seed, n_rate=0.02, threads=8)
    rng = random.Random(seed)
    for qual, lens in ((batch.qual1, batch.len1), (batch.qual2, batch.len2)):
        for i in range(n):
            if clip and i % 3 == 0:
                lens[i] = rng.randint(0, int(lens[i]))
            q = qualities(rng, int(lens[i]), i)
            qual[i, :len(q)] = np.frombuffer(q.encode(), dtype=np.uint8)
    return batch


def run_engine(tp, batch):
    n = batch.n
    xf1 = np.full(n, FILL, dtype=np.uint8)
    xf2 = np.full(n, FILL, dtype=np.uint8) if tp.paired else None
    with TrimEngine(tp, device=0, slots=1, max_reads=max(n, 1), max_stride=batch.stride) as eng:
        g1, _cap2, g2 = eng.submit(0, batch.seq1, batch.qual1, batch.len1, batch.seq2, batch.qual2, batch.len2,
                                   xflags=(xf1, xf2))
        eng.wait(0)
        st = eng.stats()
        counts = eng.xflag_counts()
    return (g1, g2), (xf1, xf2), st, counts


def order_sensitive(qual: bytes) -> bool:
    """The left-to-right sum of these qualities differs from the sum taken right to left, in pairs and in four
    interleaved partial sums: a kernel that adds in any of those orders misses the threshold below."""
    t = [filters_rule.EE_TABLE[b] for b in qual]
    e = filters_rule.expected_errors(qual)
    pairs = t[:]
    while len(pairs) > 1:
        pairs = [sum(pairs[i:i + 2]) for i in range(0, len(pairs), 2)]
    lanes = [0.0] * 4
    for i, x in enumerate(t):
        lanes[i % 4] += x
    return e != filters_rule.expected_errors(qual[::-1]) and e != pairs[0] and e != (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])


def setup(tp, max_length=None, max_n=None, max_ee=None):
    tp.max_length, tp.max_n, tp.max_ee = max_length, max_n, max_ee
    return tp


def check(tp, batch, threshold_read: bool, want_resolve: bool = False):
    """Every -M and --max-ee value of the issue on one batch; -> the oracle's results per mate."""
    m1, m2 = util.oracle_run(tp, batch, threads=8)
    mates = [(batch.seq1, batch.qual1, m1[0])] + ([(batch.seq2, batch.qual2, m2[0])] if tp.paired else [])
    finals = np.concatenate([o["stop"].astype(np.int64) - o["start"].astype(np.int64) for _s, _q, o in mates])
    ees = [filters_rule.expected_errors(q[i, int(o["start"][i]):int(o["stop"][i])].tobytes())
           for _s, q, o in mates for i in range(batch.n)]
    median, mid = int(np.median(finals)), float(np.median(ees))
    ee_values = [0.0, math.inf, mid]
    pick = None
    if threshold_read:  # a read of at least 100 final bases with mixed qualities, whose sum depends on the order
        q, o = mates[0][1], mates[0][2]
        for i in range(batch.n):
            s, e = int(o["start"][i]), int(o["stop"][i])
            if e - s >= 100 and len(set(q[i, s:e].tobytes())) >= 20 and order_sensitive(q[i, s:e].tobytes()):
                pick = i
                break
        assert pick is not None
        exact = ees[pick]
        ee_values += [exact, math.nextafter(exact, 0.0)]
    configs = [dict(max_length=v) for v in (0, 1, median, 65535, 70000)] + [dict(max_ee=v) for v in ee_values]
    configs.append(dict(max_length=median, max_n=0.0, max_ee=mid))
    seen = []
    for cfg in configs:
        (g1, g2), xf, st, counts = run_engine(setup(tp, **cfg), batch)
        bits = 0
        for m, (seq, qual, want_res) in enumerate(mates):
            assert np.array_equal((g1, g2)[m], want_res), cfg
            want = filters_rule.xflags(seq, qual, want_res, **cfg)
            assert np.array_equal(xf[m], want), (cfg, m, np.nonzero(xf[m] != want)[0][:5])
            assert counts[m] == {"too_many_n": int(((want & abi.CS_X_TOO_MANY_N) != 0).sum()),
                                 "too_long": int(((want & abi.CS_X_TOO_LONG) != 0).sum()),
                                 "too_many_ee": int(((want & abi.CS_X_TOO_MANY_EE) != 0).sum())}, (cfg, m)
            assert st[m].n_too_many_n == counts[m]["too_many_n"]
            bits |= int(np.bitwise_or.reduce(want)) if len(want) else 0
            seen.append((cfg, m, want))
        if want_resolve:
            assert st[0].n_exact_dp > 0  # (reads that got their flags from the resolve kernel)
        if len(cfg) == 3:  # all three together: each of them fires somewhere, and some read is left alone
            assert bits == 7 and any((w == 0).any() for c, _m, w in seen if c is cfg)
    # the filters took some reads and left some (the rule alone decides that), and the extreme values did what they say
    def taken(**cfg):
        return [int((w != 0).sum()) for c, _m, w in seen if c == cfg]
    assert all(0 < t < batch.n for t in taken(max_length=median)) and all(0 < t < batch.n for t in taken(max_ee=mid))
    assert sum(taken(max_length=65535)) == 0 and sum(taken(max_length=70000)) == 0 and sum(taken(max_ee=math.inf)) == 0
    assert sum(taken(max_length=0)) == int((finals > 0).sum())
    if pick is not None:  # equality keeps the read, the next double below discards it
        at, below = [[w for c, m, w in seen if c == dict(max_ee=v) and m == 0][0] for v in ee_values[3:]]
        assert at[pick] == 0 and below[pick] == abi.CS_X_TOO_MANY_EE
    # no filter: results as before, the caller's xflags keep their fill pattern, nothing is counted
    (g1, g2), xf, st, counts = run_engine(setup(tp), batch)
    for m, (_seq, _qual, want_res) in enumerate(mates):
        assert np.array_equal((g1, g2)[m], want_res) and (xf[m] == FILL).all()
        assert counts[m] == {"too_many_n": 0, "too_long": 0, "too_many_ee": 0}
    return [o for _s, _q, o in mates]


def offsets(results):
    starts = {int(v) % 4 for o in results for v in o["start"][o["stop"] > o["start"]]}
    stops = {int(v) % 4 for o in results for v in o["stop"][o["stop"] > o["start"]]}
    return starts, stops


def single_plan(adapter=ADAPTER):
    return planmod.single_adapter_plan(adapter, max_error_rate=0.1, min_overlap=3)


def paired_plan():
    return util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], planmod.CutadaptConfig(), True)


def test_scan_kernel_fast_tiles_single_adapter():
    """Upper-case A/C/G/T/N only: the coded plan's tiles take the fast form.  Lengths 0..72 in rows of 72 bytes: final
    intervals that are empty, that end at every offset mod 4 and that span the whole row."""
    batch = util.batch_from_reads(adapter_reads(1, short_lengths(2)))
    assert batch.stride == 72
    (o1,) = check(single_plan(), batch, threshold_read=False)
    span = o1["stop"].astype(int) - o1["start"].astype(int)
    assert (span[batch.len1 > 0] == 0).any() and (span == batch.stride).any()
    assert offsets([o1])[1] == {0, 1, 2, 3}
    check(single_plan(), util.batch_from_reads(adapter_reads(3, [150] * 1024)), threshold_read=True)


def test_scan_kernel_fast_tiles_takara_pairs():
    """The paired TAKARAV3 chain (cuts at both ends, two adapters, quality trimming): intervals that start and end at
    every offset mod 4."""
    results = check(paired_plan(), takara_batch(2048, 70, 5, clip=True), threshold_read=False)
    assert offsets(results) == ({0, 1, 2, 3}, {0, 1, 2, 3})
    check(paired_plan(), takara_batch(1024, 150, 6, clip=False), threshold_read=True)


def exact_form(batch, seed):
    """IUPAC codes and lower-case bytes in one read in ten: their tiles fall back to the exact form."""
    rng = np.random.default_rng(seed)
    for seq, lens in ((batch.seq1, batch.len1), (batch.seq2, batch.len2)):
        if seq is None:
            continue
        for i in np.nonzero((rng.random(batch.n) < 0.1) & (lens > 0))[0]:
            j = int(rng.integers(0, int(lens[i])))
            seq[i, j] = ord(rng.choice(list("RYKMSWBDHV")))
            k = int(rng.integers(0, int(lens[i])))
            seq[i, k] = ord(chr(seq[i, k]).lower())
    return batch


def test_scan_kernel_exact_form_tiles():
    check(single_plan(), exact_form(util.batch_from_reads(adapter_reads(7, short_lengths(8))), 9), threshold_read=False)
    check(paired_plan(), exact_form(takara_batch(2048, 70, 10, clip=True), 11), threshold_read=False)
    check(paired_plan(), exact_form(takara_batch(1024, 150, 12, clip=False), 13), threshold_read=True)


def test_scan_kernel_raw_tiles():
    tp = single_plan(RAW_ADAPTER)
    check(tp, util.batch_from_reads(adapter_reads(14, short_lengths(15), RAW_ADAPTER)), threshold_read=False)
    check(tp, util.batch_from_reads(adapter_reads(16, [150] * 1024, RAW_ADAPTER)), threshold_read=True)


def test_reads_deferred_to_the_resolve_kernel():
    """Adapters with up to four edits: the scan kernel cannot settle many of them and defers the read."""
    reads = adapter_reads(17, [150] * 1024 + short_lengths(18, each=8), edits=4)
    tp = planmod.single_adapter_plan(ADAPTER, max_error_rate=0.2, min_overlap=3)
    check(tp, util.batch_from_reads(reads), threshold_read=True, want_resolve=True)


# ---- the long-read kernel (text path: reads longer than the rows) ----------------------------------------------

def fastq_text(names, seqs, quals):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(names, seqs, quals))


def test_long_read_kernel_through_the_text_path():
    """Rows of 152 bytes and reads of about 2 000 nt (one of 5 000: longer than 70 000 mod 2^16): every read takes the
    long-read kernel.  Expected records: the string-level restatement; the rule on each final read."""
    rng = random.Random(3)
    st = planmod.CutadaptConfig()
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, False)
    seqs, quals = [], []
    for i in range(24):
        length = 5000 if i == 5 else rng.randint(1800, 2200)
        s = bytearray(rng.choice(b"ACGT") for _ in range(length))
        if i % 3 == 0:
            a = rng.randint(0, length - 10)
            s[a:a + 6] = b"NNNNNN"
        seqs.append(bytes(s))
        quals.append(qualities(rng, length, i).encode())
    names = [b"long%d" % i for i in range(len(seqs))]
    from oracle import pyref
    pipe = pyref.SinglePipeline(BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"]), util.to_pyref_settings(st))
    routes = {"trimmed": 0, "short": 1, "untrimmed": 2}
    out = []
    for i in range(len(seqs)):
        rt, o = pipe.process(pyref.Read(names[i].decode(), seqs[i].decode(), quals[i].decode()))
        rec = o.fastq().encode()
        out.append((routes[rt], rec, rec.split(b"\n")[1], rec.split(b"\n")[3]))
    ees = sorted(filters_rule.expected_errors(q) for _rt, _rec, _s, q in out)
    lens = sorted(len(s) for _rt, _rec, s, _q in out)
    mid_ee, median = ees[len(ees) // 2], lens[len(lens) // 2]
    exact = next(filters_rule.expected_errors(q) for _rt, _rec, _s, q in out if len(q) >= 100 and order_sensitive(q))
    text = fastq_text(names, seqs, quals)
    configs = [dict(max_length=v) for v in (0, 1, median, 65535, 70000)]
    configs += [dict(max_ee=v) for v in (0.0, math.inf, mid_ee, exact, math.nextafter(exact, 0.0))]
    configs.append(dict(max_length=median, max_n=0.0, max_ee=mid_ee))
    taken = {}
    for k, cfg in enumerate(configs):
        setup(tp, **cfg)
        with TrimEngine(tp, device=0, slots=0) as eng:
            with textpath.TextEngine(eng, slots=1, max_text_bytes=len(text) + 1024, max_records=len(seqs),
                                     stride=152) as te:
                streams, counts = te.run(text, len(seqs))
                discards = te.discards(0)
            xc, _ = eng.xflag_counts()
        x = []
        for _rt, _rec, s, q in out:
            x.append((abi.CS_X_TOO_LONG if cfg.get("max_length") is not None and filters_rule.too_long(len(s), cfg["max_length"]) else 0)
                     | (abi.CS_X_TOO_MANY_N if cfg.get("max_n") is not None and filters_rule.maxn_rule.too_many_n(s, cfg["max_n"]) else 0)
                     | (abi.CS_X_TOO_MANY_EE if cfg.get("max_ee") is not None and filters_rule.too_many_ee(q, cfg["max_ee"]) else 0))
        flag_of = {0: 0, 1: abi.CS_F_TOO_SHORT, 2: abi.CS_F_UNTRIMMED}
        where = [filters_rule.route(flag_of[rt], 0, xi, 0, True) for (rt, _rec, _s, _q), xi in zip(out, x)]
        for r in range(3):
            assert streams[r][0] == b"".join(rec for (_rt, rec, _s, _q), w in zip(out, where) if w == r), (cfg, r)
        assert xc == {"too_long": sum(1 for xi in x if xi & abi.CS_X_TOO_LONG),
                      "too_many_n": sum(1 for xi in x if xi & abi.CS_X_TOO_MANY_N),
                      "too_many_ee": sum(1 for xi in x if xi & abi.CS_X_TOO_MANY_EE)}, cfg
        assert discards == tuple(where.count(name) for name, _bit in filters_rule.ORDER), cfg
        assert sum(counts) == len(out) - sum(discards)
        taken[k] = sum(discards)
    n = len(out)
    assert 0 < taken[2] < n and 0 < taken[7] < n and 0 < taken[10] < n
    assert taken[3] == taken[4] == taken[6] == 0 and taken[9] == taken[8] + 1
