"""The long-read kernel (long_kernel.hip.inc) held to the oracle: the third implementation of the op chain.

The text path sends every read longer than its row stride to that kernel (text_kernels.hip.inc, text_parse_records),
and the host starts at a stride of 152: the first batches of a 2 x 250 library are trimmed there entirely.  The kernel
has its own locate (three-int cells), its own SHORTCUT_FIND, its own case folding and coded / raw query bytes, cutters
and captures, quality trimming, both demultiplexing forms and its own statistics atomics.  Here it meets the aligner
settings of tests/universe.py, the odd alphabets of util.odd_alphabet_cases, reads beyond the oracle's 16-bit lengths
(against oracle/pyref.py, which has no length limit), the CS_MAX_READ edge, and long tile rows whose windows start
late in the read (the strip DP with true_init false, trim_kernel.hip.inc).

Every text-path run here asserts (test_gpu_text.check_text_path): (a) n_long per mate equals the number of reads
longer than the stride, so the kernel provably ran; (b) the streams equal the oracle's results formatted by the
record logic, route by route; (c) the per-mate statistics equal the oracle's.
"""
import random

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig
from cutseq_amd.engine import TrimEngine
from cutseq_amd.synth import SynthBatch
from oracle import pyref

import universe as U
import util
from test_gpu_parity import one_adapter_plan, run_both, stats_dict
from test_gpu_text import check_text_path, fastq_text, oracle_streams, run_text_exposed

pytestmark = pytest.mark.gpu


def text_of(names, batch: SynthBatch, paired: bool):
    t1 = fastq_text(names[0], batch.seq1, batch.qual1, batch.len1)
    t2 = fastq_text(names[1], batch.seq2, batch.qual2, batch.len2) if paired else None
    return t1, t2


# ---------------------------------------------------------------------------------------------------------------------
# 1. every aligner setting, enumerated reads, through the long-read kernel

UNIVERSE_ADAPTER_STEP = 6  # every sixth adapter over {A,C,G} of length 3..7: 545 adapters, the rotation meets all 504


@pytest.mark.parametrize("rule,tie", [(abi.CS_SELECT_LEFTMOST, abi.CS_TIE_INSERTION), (abi.CS_SELECT_LEFTMOST, abi.CS_TIE_DELETION),
                                      (abi.CS_SELECT_SCORE, abi.CS_TIE_INSERTION), (abi.CS_SELECT_SCORE, abi.CS_TIE_DELETION)])
def test_every_setting_on_enumerated_reads(rule, tie):
    """Every read over {A,C,G} up to 8 nt and over {A,C,G,N} up to 5 nt (11 206 reads), at row stride 4: every read of
    5 nt or more walks its chain in the long-read kernel.  Adapters: every sixth of tests/universe.py's {A,C,G} list
    (lengths 3..7), one setting each by the universe's rotation, which meets all 504 SETTINGS (both rules, both tie
    orders: this case's quarter of them); paired plans run two (adapter, setting) ops per launch over the same reads."""
    ads = U.adapters("ACG")[::UNIVERSE_ADAPTER_STEP]
    seq, qual, lens = U.stack([U.reads_universe("ACG", 8), U.reads_universe("ACGN", 5)], 8)
    batch = SynthBatch(seq, qual, lens, seq, qual, lens)
    names = [b"u%d" % i for i in range(batch.n)]
    text1, text2 = text_of((names, names), batch, True)
    items = [it for r, t, its in U.schedule(len(ads), 1) if (r, t) == (rule, tie) for it in its]
    met = {si for _a, si in items}
    assert len(met) == 126 and all(U.SETTINGS[si][4:] == (rule, tie) for si in met)
    for lo in range(0, len(items), 2):
        pair = (items[lo:lo + 2] * 2)[:2]
        ops = [U.adapter_op(ads[a], U.SETTINGS[si]) for a, si in pair]
        tp = U.one_op_plan([ops[0]], [ops[1]], rule, tie)
        what = [f"adapter {ads[a]} setting {U.SETTINGS[si]}" for a, si in pair]
        got = check_text_path(tp, batch, text1, text2, 4, oracle_streams(tp, batch, names, names), what)
        assert got.n_long[0] == int((lens > 4).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 3. odd alphabets, qualities and settings


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_odd_alphabets_and_settings_through_the_long_read_kernel(seed):
    """util.odd_alphabet_cases (lower case, IUPAC, '.', every printable quality, case-sensitive plans, SHORTCUT_FIND,
    schemes with N in their adapters: uncoded plans -- the coded / raw query bytes of query_code) at row stride 4."""
    for k, (scheme, st, paired, reads1, reads2, untrimmed_requested) in enumerate(util.odd_alphabet_cases(seed, rounds=4, pairs=800)):
        batch = util.batch_from_reads(reads1, reads2 if paired else None)
        tp = util.compile_plan(scheme, st, paired, untrimmed_requested=untrimmed_requested)
        names1 = [b"F:%d 1" % i for i in range(batch.n)]
        names2 = [b"F:%d 2" % i for i in range(batch.n)] if paired else None
        text1, text2 = text_of((names1, names2), batch, paired)
        check_text_path(tp, batch, text1, text2, 4, oracle_streams(tp, batch, names1, names2), (seed, k, scheme))


# ---------------------------------------------------------------------------------------------------------------------
# 4. reads beyond the oracle's 16-bit lengths, against pyref


def cg(rng: random.Random, n: int) -> str:
    """Background the TAKARAV3 chain cannot match: no A, no T (its adapters and the poly-A / poly-T ops need them)."""
    return "".join(rng.choice("CG") for _ in range(n))


def test_reads_beyond_sixteen_bit_lengths_equal_pyref():
    """Reads of 65 535 (CS_LEN_SKIP) to 300 000 nt: 3' adapters (exact and damaged) and partial adapters planted beyond
    position 65 535, a 60-base poly-A in front of one, a low-quality tail, UMI captures in the names, a pair with one long
    mate, next to ordinary 150-nt pairs -- TAKARAV3 with --trim-polyA at the default row stride.  Expected: pyref (string
    slicing, no length limit), record by record; and the planted adapter is the one that trimmed."""
    rng = random.Random(65536)
    scheme = BUILDIN_ADAPTERS["TAKARAV3"]
    bc = BarcodeConfig(scheme)
    a1, a2 = bc.p7.fw, bc.p5.rc  # the 3' adapters of mate 1 and mate 2
    hi, lo = "I", "#"
    pairs = []  # (seq1, qual1, seq2, qual2, where mate 1's adapter starts or None, the same for mate 2)

    def plain(n):
        return cg(rng, n), hi * n

    def planted(n_before, adapter, n_after, poly_a=0):
        s = cg(rng, n_before) + "A" * poly_a + adapter + cg(rng, n_after)
        return s, hi * len(s)

    s1, q1 = planted(70_000, a1, 30)
    s2, q2 = planted(90_000, a2, 40, poly_a=60)
    pairs.append((s1, q1, s2, q2, 70_000, 90_000))
    s1, q1 = plain(65_535)
    s2, q2 = plain(65_536)
    q2 = q2[:-300] + lo * 300  # a low-quality tail on mate 2
    pairs.append((s1, q1, s2, q2, None, None))
    s1, q1 = planted(65_536 - 17, a1, 65_535 - 65_536 + 17 - len(a1) + 20)  # the adapter across position 65 535
    s2, q2 = planted(65_540, a2, 0)
    pairs.append((s1, q1, s2, q2, 65_519, 65_540))
    d1 = util.mutate(rng, a1, 2, "CG")
    s1, q1 = planted(200_000, d1, 50)
    s2, q2 = plain(150)
    pairs.append((s1, q1, s2, q2, 200_000, None))  # only mate 1 is long
    s1, q1 = planted(120_000, a1[:12], 0)  # partial adapters at the 3' end
    s2, q2 = planted(100_000, a2[:8] + ("C" if a2[8] != "C" else "G"), 0)
    pairs.append((s1, q1, s2, q2, 120_000, 100_000))
    s1, q1 = plain(80_000)
    q1 = q1[:-500] + lo * 500  # a low-quality tail: quality trimming, 500 bases
    d2 = util.mutate(rng, a2, 2, "CG")
    s2, q2 = planted(300_000, d2, 700, poly_a=60)
    pairs.append((s1, q1, s2, q2, None, 300_000))
    s1, q1 = plain(150)
    s2, q2 = planted(66_000, a2, 10)
    pairs.append((s1, q1, s2, q2, None, 66_000))  # only mate 2 is long
    for i in range(5):  # ordinary pairs around them (the tile kernels' side of the same batch)
        s1, q1 = plain(150)
        s2, q2 = planted(100, a2, 50 - len(a2)) if i % 2 else plain(150)
        pairs.insert(2 * i, (s1, q1, s2, q2, None, 100 if i % 2 else None))

    st = planmod.CutadaptConfig()
    st.trim_polyA = True
    tp = util.compile_plan(scheme, st, True)
    pipe = pyref.PairedPipeline(bc, util.to_pyref_settings(st))
    routes = {"trimmed": 0, "short": 1, "untrimmed": 2}
    want = [[b"", b""] for _ in range(3)]
    counts = [0, 0, 0]
    names1 = [b"LONG:%d 1:N:0:X" % i for i in range(len(pairs))]
    names2 = [b"LONG:%d 2:N:0:X" % i for i in range(len(pairs))]
    out_bp = [0, 0]
    too_short = [0, 0]
    for i, (s1, q1, s2, q2, p1, p2) in enumerate(pairs):
        rt, o1, o2 = pipe.process(pyref.Read(names1[i].decode(), s1, q1), pyref.Read(names2[i].decode(), s2, q2))
        want[routes[rt]][0] += o1.fastq().encode()
        want[routes[rt]][1] += o2.fastq().encode()
        counts[routes[rt]] += 1
        for m, (o, p, s) in enumerate(((o1, p1, s1), (o2, p2, s2))):
            out_bp[m] += len(o)
            too_short[m] += len(o) < st.min_length
            if p is not None:  # the planted adapter trimmed: the read ends shortly before it, the bases kept are its own
                assert p - 100 <= len(o) <= p and o.sequence in s[:p], (i, m, len(o), p)
    qtrim_bp = [pipe.mods[-1][m].trimmed_bases for m in range(2)]
    assert qtrim_bp[0] >= 480 and qtrim_bp[1] >= 280  # (the cutters take a few of those bases first)
    # the UMI (first 8 bases of mate 2) is in the names
    assert all(b"_" in rec.split(b"\n")[0] for rec in want[0][0].split(b"\n@") if rec)

    seqs = [[p[0] for p in pairs], [p[2] for p in pairs]]
    quals = [[p[1] for p in pairs], [p[3] for p in pairs]]
    texts = [b"".join(b"@" + nm + b"\n" + s.encode() + b"\n+\n" + q.encode() + b"\n" for nm, s, q in zip(nms, seqs[m], quals[m]))
             for m, nms in enumerate((names1, names2))]
    got = run_text_exposed(tp, texts[0], texts[1], len(pairs), 152)
    for m in range(2):
        assert got.n_long[m] == sum(len(s) > 152 for s in seqs[m]), (m, got.n_long)
    assert got.counts == counts
    for route in range(3):
        for m in range(2):
            assert got.streams[route][m] == want[route][m], (textpath.ROUTES[route], m)
    for m in range(2):
        st_m = got.stats[m]
        assert int(st_m.n_reads) == len(pairs)
        assert int(st_m.in_bp) == sum(len(s) for s in seqs[m])
        assert int(st_m.out_bp) == out_bp[m]
        assert int(st_m.qualtrim_bp) == qtrim_bp[m]
        assert int(st_m.n_too_short) == too_short[m]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the CS_MAX_READ edge


def test_a_read_beyond_cs_max_read_is_refused_and_the_engine_goes_on():
    """A record of CS_MAX_READ + 1 nt raises ReadTooLong (the parse kernel reports it, the long-read kernel is gated
    off); the same text engine then trims a normal batch correctly.  (A read of exactly CS_MAX_READ nt is NOT trimmed
    here: one lane would walk 16 M bases per op.)"""
    st = planmod.CutadaptConfig()
    scheme = BUILDIN_ADAPTERS["TAKARAV3"]
    tp = util.compile_plan(scheme, st, False)
    n_big = abi.CS_MAX_READ + 1
    big = b"@huge\n" + b"C" * n_big + b"\n+\n" + b"I" * n_big + b"\n"
    rng = random.Random(5)
    reads = [(cg(rng, 100) + BarcodeConfig(scheme).p7.fw + cg(rng, 30), "I" * 150) for _ in range(50)]
    reads += [(util.random_dna(rng, rng.choice([20, 150, 400])), "") for _ in range(50)]
    reads = [(s, q or "I" * len(s)) for s, q in reads]
    batch = util.batch_from_reads(reads)
    names = [b"n%d" % i for i in range(batch.n)]
    text = fastq_text(names, batch.seq1, batch.qual1, batch.len1)
    want_streams, want_counts, want_stats = oracle_streams(tp, batch, names, None)
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=len(big) + 1024, max_records=256, stride=152) as te:
            with pytest.raises(textpath.ReadTooLong) as e:
                te.run(big, 1)
            assert e.value.longest == n_big
            te.submit(0, text, len(text), None, 0, batch.n)
            res = te.wait(0)
            out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
            te.fetch(0, out[0], None)
            streams = textpath.split_routes(res, out, False)
        st1, _ = eng.stats()
    assert int(res.n_long[0]) == int((batch.len1 > 152).sum()) > 0
    assert [int(c) for c in res.route_count] == want_counts
    assert [streams[r][0] for r in range(3)] == [want_streams[r][0] for r in range(3)]
    assert stats_dict(st1) == stats_dict(want_stats[0])  # (the refused batch counted nothing)


# ---------------------------------------------------------------------------------------------------------------------
# 6. long tile rows: strip-DP windows that start late in the read


STRIP_ADAPTERS = ("AGATCGGAAGAGCACACGTC", "CTGTCTCTTATACACATCTCCGAGCCCACGAGAC")


def late_hit_reads(rng: random.Random, ad: str, count: int):
    """Reads of 400..1536 nt: a damaged full-length adapter late in the read, often a second copy at some distance
    behind it, partial hits at the 3' end, and bases equal to the adapter's first base just in front of a copy (matches
    in the column after a window's first one)."""
    k = int(0.2 * len(ad))
    reads = []
    for i in range(count):
        n = abi.CS_MAX_STRIDE if i % 10 == 0 else rng.randint(400, abi.CS_MAX_STRIDE)
        s = util.random_dna(rng, n)
        tail = util.mutate(rng, ad, rng.randint(0, k))
        lead = ad[0] * rng.randint(0, 4) + util.random_dna(rng, rng.randint(0, k + 1))
        block = lead + tail
        if rng.random() < 0.6:
            block += util.random_dna(rng, rng.choice([0, 1, 2, 5, 13, 40, 120])) + util.mutate(rng, ad, rng.randint(0, k + 1))
        if rng.random() < 0.5:
            block += util.random_dna(rng, rng.randint(0, 30)) + util.mutate(rng, ad[: rng.randint(3, len(ad))], rng.randint(0, 1))
        at = max(0, n - len(block) - rng.choice([0, 0, 1, 5, 30, 200]))
        s = (s[:at] + block + s[at + len(block):])[:n] if rng.random() < 0.85 else s
        reads.append((s, "I" * len(s)))
    return reads


@pytest.mark.parametrize("where", list(U.WHERES))
def test_late_windows_in_long_rows_three_ways(where):
    """Every WHERE x rule x tie x rightmost on reads of 400..1536 nt (1536 = CS_MAX_STRIDE) with late hits: tile kernels
    == oracle (results, cap2, statistics) with the exact DP provably reached, then the same batch through the text
    path at stride 4 (every read in the long-read kernel) == oracle."""
    rng = random.Random(where * 7 + 1)
    exact_dp = 0
    for rule in (abi.CS_SELECT_LEFTMOST, abi.CS_SELECT_SCORE):
        for tie in (abi.CS_TIE_INSERTION, abi.CS_TIE_DELETION):
            for rightmost in (False, True):
                ad = STRIP_ADAPTERS[(rule + tie + rightmost) % 2]
                batch = util.batch_from_reads(late_hit_reads(rng, ad, 160))
                assert batch.stride <= abi.CS_MAX_STRIDE
                remove = abi.CS_REMOVE_BEFORE if where in U.REMOVE_BEFORE_WHERES else abi.CS_REMOVE_AFTER
                tp = one_adapter_plan(ad, 0.2, 3, where, remove, rightmost, rule=rule, tie=tie)
                run_both(tp, batch)
                with TrimEngine(tp, device=0, slots=1, max_reads=batch.n, max_stride=batch.stride) as eng:
                    eng.trim(batch.seq1, batch.qual1, batch.len1)
                    exact_dp += int(eng.stats()[0].n_exact_dp)
                names = [b"s%d" % i for i in range(batch.n)]
                text = fastq_text(names, batch.seq1, batch.qual1, batch.len1)
                check_text_path(tp, batch, text, None, 4, oracle_streams(tp, batch, names, None), (where, rule, tie, rightmost))
    assert exact_dp > 0, where
