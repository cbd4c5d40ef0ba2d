"""--poly-a (CS_OP_POLYA, cutadapt's PolyATrimmer) in every kernel against the rule of tests/polya_rule.py.

The op lives in tile kernels of its own (trim_kernel.hip.inc, FILT_POLYA: on the lowest rung for plans that add nothing
else, on the highest for plans with filters or read-end ops; scan and resolve) and in the POLYA walk of
long_kernel.hip.inc / info_kernels.hip.inc.  The C oracle does not know it, so the expected records are the rule alone
(chains without an adapter op) or layered (tests/test_polya_cpu.py, ``layered``): the oracle on the ops in front of the
op, the rule, ``shorten_rule.apply_tail`` for the trimmers behind it.  ``cs_polya_bp_fetch`` must equal the rule's sums.

  a  the op alone on coded tiles, scan kernel: universes E and M at stride 16, H at its own width, both ends
  b  behind cuts of 0..7 bases at either end: every nibble and dword offset of the interval's start and end
  c  raw tiles: the other mate's chain holds an adapter with a non-ACGT base
  d  resolve kernel: behind an adapter of 65+ bases, which has no filter and defers every read
  e  reads longer than the rows: the long-read kernel, through the text path
  f  full chains on both strands with --nextseq-trim, -q F,B, -l and --trim-n behind the op
  g  the text path and the command line: records, JSON counters, --info-file, and the run without the option
"""
import functools
import json

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, run as cli, synth, textpath
from cutseq_amd.engine import TrimEngine
from cutseq_amd.synth import SynthBatch

import hostfmt
import polya_rule as A
import test_polya_cpu as T
import util

pytestmark = pytest.mark.gpu

RAW_ADAPTER = "ACGTNNACGTAC"  # not all A/C/G/T: the plan is not coded, its tiles stay raw bytes


def plan_of(ops1, ops2=None, use_filter=True, min_length=0):
    return planmod.TrimPlan(r1=planmod.MateChain(list(ops1)), r2=planmod.MateChain(list(ops2)) if ops2 is not None else None,
                            has_umi=False, min_length=min_length, untrimmed_filter=False, use_filter=use_filter)


def run_engine(tp, mates):
    """One batch (mate 1's rows, mate 2's rows) -> (records per mate, cs_stats per mate, cs_polya_bp_fetch)."""
    (s1, q1, l1), (s2, q2, l2) = mates
    with TrimEngine(tp, device=0, slots=1, max_reads=len(l1), max_stride=s1.shape[1]) as eng:
        g1, _cap2, g2 = eng.trim(s1, q1, l1, s2, q2, l2)
        stats = eng.stats()
        bp = eng.polya_bp()
        assert eng.polya_bp(reset=True) == bp and eng.polya_bp() == (0, 0)
    return (g1, g2), stats, bp


def hold(tp, mates, what, check=(0, 1)):
    """Device == layered expectation for the mates of ``check``: records, out_bp, qualtrim_bp and the poly-A counter."""
    want = T.layered(tp, mates)
    got, stats, bp = run_engine(tp, mates)
    for m in check:
        seq, _qual, lens = mates[m]
        w = T.records(want[m])
        if not np.array_equal(got[m], w):
            bad = np.flatnonzero(got[m] != w)
            i = int(bad[0])
            raise AssertionError(f"{what}, mate {m + 1}: read {seq[i, :lens[i]].tobytes()!r}: device {got[m][i]} != rule {w[i]} "
                                 f"({len(bad)} of {len(lens)} reads differ)")
        assert int(stats[m].out_bp) == int((want[m].stop - want[m].start).sum()), (what, m)
        assert int(stats[m].qualtrim_bp) == want[m].cut, (what, m)
        assert bp[m] == want[m].polya_bp, (what, m, bp)
    return want, bp


@functools.lru_cache(maxsize=None)
def small(name):
    """(tail rows, head rows) of universe E or M at stride 16."""
    reads = A.universe_e if name == "E" else A.universe_m
    return tuple(tuple(A.rows_of(reads(head), stride=16)) for head in (False, True))


@functools.lru_cache(maxsize=2)
def big(lower_every, pad=0):
    return tuple(tuple(A.universe_h(head, lower_every=lower_every, pad=pad)) for head in (False, True))


TAIL, HEAD = planmod.PolyATrimOp(False), planmod.PolyATrimOp(True)


# ---- a: the op alone, coded tiles, scan kernel -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["E", "M"])
def test_a_enumerated_reads_on_coded_tiles(name):
    """Mate 1 the tail form over the tail reads, mate 2 the head form over the head reads; then the forms swapped: a tail
    walk over poly-T heads and a head walk over poly-A tails find what little there is for them."""
    mates = small(name)
    want, bp = hold(plan_of([TAIL], [HEAD]), mates, f"a: universe {name}")
    assert bp[0] > 0 and bp[1] > 0 and bp[0] == bp[1]  # (the head reads are the tail reads translated)
    assert (want[0].stop < mates[0][2]).any() and (want[1].start > 0).any()
    hold(plan_of([HEAD], [TAIL]), mates, f"a: universe {name}, forms swapped")


@pytest.mark.parametrize("lower_every", [0, 5], ids=["plain", "lower-case"])
def test_a_homopolymer_universe_on_coded_tiles(lower_every):
    """201 036 reads per end at stride 188: tails across the dword, 32-, 64- and 128-base boundaries, a foreign base every
    p positions at every phase; once with every fifth base of the runs in lower case (an error: such tiles leave the
    fast re-coding too)."""
    mates = big(lower_every)
    assert len(mates[0][2]) == 201036
    want, bp = hold(plan_of([TAIL], [HEAD]), mates, f"a: universe H, lower_every={lower_every}")
    took = mates[0][2].astype(np.int64) - (want[0].stop - want[0].start)
    assert (took > 128).any() and bp[0] == int(took.sum())


# ---- b: behind cuts --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", range(8))
def test_b_every_offset_of_the_interval(c):
    """[CutOp(c), op] and [CutOp(-c), op] for both forms: s & 7 = c, and e moves by c against the reads' own lengths.
    E and M at stride 16; H with c bases of G at the anchored end for the cut to take."""
    for name in ("E", "M"):
        for cut in (c, -c):
            hold(plan_of([planmod.CutOp(cut), TAIL], [planmod.CutOp(cut), HEAD]), small(name), f"b: universe {name} behind a cut of {cut}")
    mates = big(0, pad=c)
    hold(plan_of([planmod.CutOp(-c), TAIL], [planmod.CutOp(c), HEAD]), mates, f"b: universe H behind a cut of {c} at the op's end")


# ---- c: raw tiles ----------------------------------------------------------------------------------------------------

def raw_op():
    return planmod.back(RAW_ADAPTER, 0.2, 3, flag=abi.CS_F_ADAPTER3)


def hold_raw(mates, what):
    """The op in plans whose OTHER chain opens with an adapter that has a non-ACGT base: cs_plan_create leaves such a plan
    uncoded, the tiles keep their bytes.  The mate whose chain is the op alone is the one held."""
    for ops1, ops2, check in (([TAIL], [raw_op(), HEAD], (0, 1)), ([raw_op(), TAIL], [HEAD], (0, 1))):
        hold(plan_of(ops1, ops2), mates, f"c: {what} (raw tiles)", check=check)


@pytest.mark.parametrize("name", ["E", "M", "H"])
def test_c_raw_tiles(name):
    hold_raw(big(5) if name == "H" else small(name), f"universe {name}")
    if name != "H":  # behind a cut on raw tiles too
        for cut in (3, -5):
            hold(plan_of([planmod.CutOp(cut), TAIL], [raw_op(), planmod.CutOp(cut), HEAD]), small(name), f"c: {name} cut {cut}", check=(0,))
            hold(plan_of([raw_op(), planmod.CutOp(cut), TAIL], [planmod.CutOp(cut), HEAD]), small(name), f"c: {name} cut {cut}", check=(1,))


# ---- d: resolve kernel -----------------------------------------------------------------------------------------------

def long_adapter(letters, length=67):
    return planmod.back("".join(letters[(i * i + i // 3) % 2] for i in range(length)), 0.1, 3, flag=abi.CS_F_ADAPTER3)


@pytest.mark.parametrize("name", ["E", "M", "H"])
def test_d_resolve_kernel(name):
    """[an adapter of 67 nt under CS_WHERE_BACK, the op]: the adapter has no filter, every read that is not empty is
    deferred and finishes its chain -- the op with it -- in the resolve kernel.  The adapter is made of two letters the
    reads do not hold (the oracle decides either way).  Also behind a cut, where the deferred interval starts off a dword."""
    mates = big(5) if name == "H" else small(name)
    if name == "H":  # (every 7th read: the exact DP of 200 000 reads against 67 bases is not what this test is about)
        mates = tuple(tuple(np.ascontiguousarray(x[::7]) for x in mate) for mate in mates)
    chains = ([long_adapter("GT"), TAIL], [long_adapter("AC"), HEAD])
    tp = plan_of(*chains)
    want, bp = hold(tp, mates, f"d: universe {name} behind a 67 nt adapter")
    assert bp[0] > 0 and bp[1] > 0
    got, stats, _bp = run_engine(tp, mates)
    for m in (0, 1):
        assert int(stats[m].n_exact_dp) == int((mates[m][2] > 0).sum()) > 0
    cut = ([planmod.CutOp(3), long_adapter("GT"), TAIL], [planmod.CutOp(5), long_adapter("AC"), HEAD])
    hold(plan_of(*cut), mates, f"d: universe {name} behind cuts and a 67 nt adapter")


# ---- e: reads longer than the rows -----------------------------------------------------------------------------------

LONG_LENGTHS = (1537, 4099, 300000)
SHAPES = ("all", "every5th", "every4th", "foreign-last", "random")


def long_reads(head):
    """Per length: all A; a foreign base every 5th position (qualifies); every 4th (does not); one foreign last base in
    front of As; random bases.  Written as the tail form sees them from the 3' end; the head form is the mirror image."""
    base, other = (ord("T"), ord("G")) if head else (ord("A"), ord("C"))
    rng = np.random.default_rng(11)
    reads = []
    for n in LONG_LENGTHS:
        walk = np.full((len(SHAPES), n), base, dtype=np.uint8)
        walk[1, 4::5] = other
        walk[2, 3::4] = other
        walk[3, 0] = other
        walk[4] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
        reads += [bytes(w) if head else bytes(w[::-1]) for w in walk]
    return reads


def run_text(tp, text1, text2, n, stride):
    """One batch through a fresh text engine -> (streams[route][mate], counts, n_long, stats, polya_bp)."""
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2)) + 1024, max_records=n, stride=stride) as te:
            te.submit(0, text1, len(text1), text2, len(text2), n)
            res = te.wait(0)
            out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
            te.fetch(0, out[0], out[1])
            streams = textpath.split_routes(res, out, True)
        return streams, [int(c) for c in res.route_count], [int(res.n_long[0]), int(res.n_long[1])], eng.stats(), eng.polya_bp()


def text_of(names, reads):
    return b"".join(b"@" + nm + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for nm, r in zip(names, reads))


def test_e_long_read_kernel():
    """Reads of 1537, 4099 and 300 000 bases at rows of 64: every one takes the long-read kernel's scalar walk."""
    tails, heads = long_reads(False), long_reads(True)
    n = len(tails)
    names = [b"long%d" % i for i in range(n)]
    tp = plan_of([TAIL], [HEAD])
    streams, counts, n_long, stats, bp = run_text(tp, text_of(names, tails), text_of(names, heads), n, 64)
    assert n_long == [n, n] and counts == [n, 0, 0]
    want = [b"", b""]
    sums = [0, 0]
    kept = []
    for i in range(n):
        for m, (reads, head) in enumerate(((tails, False), (heads, True))):
            r = reads[i]
            row = np.frombuffer(r, dtype=np.uint8)[None, :]
            a, b = A.rows_keep(row, 0, np.array([len(r)]), head)
            a, b = int(a[0]), int(b[0])
            if len(r) < 5000:
                assert (a, b) == A.keep(r, head)
            want[m] += hostfmt.fastq_record(names[i], r, b"I" * len(r), a, b)
            sums[m] += len(r) - (b - a)
            kept.append(b - a)
    for k, length in enumerate(LONG_LENGTHS):
        # all: nothing stays; every 5th: nothing but what lies behind the last position of the highest score (1537 ends
        # "CAA" in walk order, 300 000 on the foreign base itself); every 4th: the rate holds for 15 bases (3 errors) and
        # no further; one foreign last base: nothing stays; random: next to everything
        per = kept[10 * k:10 * k + 10:2]
        assert per[:4] == [0, {1537: 3, 4099: 0, 300000: 1}[length], length - 15, 0] and per[4] > length - 40, (length, per)
    for m in (0, 1):
        if streams[0][m] != want[m]:
            lines = streams[0][m].split(b"\n")
            raise AssertionError((m, [len(lines[4 * i + 1]) for i in range(n)], kept[m::2]))
        assert int(stats[m].out_bp) == sum(kept[m::2])
    assert list(bp) == sums and min(sums) > 900000


# ---- f: full chains --------------------------------------------------------------------------------------------------

def chain_settings(**extra):
    st = planmod.CutadaptConfig()
    st.poly_a = True
    for key, value in extra.items():
        setattr(st, key, value)
    return st


FULL = dict(nextseq_trim=20, min_quality=10, min_quality_front=15, length=100, trim_n=True)


def mates_of(batch):
    return (batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2)


@pytest.mark.parametrize("scheme", [T.TAKARA, T.TAKARA_PLUS], ids=["minus", "plus"])
@pytest.mark.parametrize("extra", [{}, FULL], ids=["alone", "with-the-tail"])
def test_f_full_chains(scheme, extra):
    """4096 synthetic pairs through TAKARAV3 (a '<' library: read 1 loses a poly-T head, read 2 a poly-A tail) and through
    the '>' scheme of the same parts, the option alone (the lowest-rung kernels) and with --nextseq-trim 20 -q 15,10 -l 100
    --trim-n behind it (the highest-rung kernels); both mates against the layered expectation."""
    batch = synth.generate_pairs(4096, 150, scheme, seed=77, poly_fraction=0.3)
    tp = util.compile_plan(scheme, chain_settings(**extra), True)
    assert [o.revcomp for o in T.poly_ops(tp.r1) + T.poly_ops(tp.r2)] == ([True, False] if scheme == T.TAKARA else [False, True])
    want, bp = hold(tp, mates_of(batch), f"f: {scheme} {sorted(extra)}")
    assert bp[0] > 1000 and bp[1] > 1000
    if extra:
        assert want[0].cut > 0 and max((want[0].stop - want[0].start).max(), (want[1].stop - want[1].start).max()) == 100
    # the same chain without the op differs, and leaves the counter at zero
    off = util.compile_plan(scheme, chain_settings(poly_a=False, **extra), True)
    got_off, _stats, bp_off = run_engine(off, mates_of(batch))
    assert bp_off == (0, 0) and not np.array_equal(got_off[0], T.records(want[0]))


# ---- g: the text path and the command line ---------------------------------------------------------------------------

N_CLI = 2000


@functools.lru_cache(maxsize=None)
def cli_batch():
    return synth.generate_pairs(N_CLI, 150, T.TAKARA, seed=123, poly_fraction=0.3)


def expected_streams(tp, batch, names, want):
    res = [T.records(w) for w in want]
    streams = {0: [b"", b""], 1: [b"", b""], 2: [b"", b""]}
    for route, r1, r2 in util.format_batch(tp, batch, names, names, res[0], None, res[1]):
        streams[route][0] += r1
        streams[route][1] += r2
    return streams


def gunzip(path):
    import gzip
    with gzip.open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_g_cli_records_counters_and_info_file(gz, tmp_path, capsys):
    """About 2 000 pairs through the command line with --poly-a, plain and .gz outputs: the records equal tests/hostfmt.py
    on the layered intervals, the JSON counters equal the rule's sums, --info-file shows the narrowed final read in
    its no-match rows (read 1 of a '<' library loses its poly-T head)."""
    batch = cli_batch()
    names = [b"rec%d" % i for i in range(N_CLI)]
    ins = [str(tmp_path / "in1.fq.gz"), str(tmp_path / "in2.fq.gz")]
    util.write_fastq(ins[0], names, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(ins[1], names, batch.seq2, batch.qual2, batch.len2)
    tp = util.compile_plan(T.TAKARA, chain_settings(), True)
    want = T.layered(tp, mates_of(batch))
    streams = expected_streams(tp, batch, names, want)
    ext = "fastq.gz" if gz else "fastq"
    out = lambda tag: str(tmp_path / f"{tag}.{ext}")
    info, js = str(tmp_path / "info.tsv"), str(tmp_path / "report.json")
    cli.main(ins + ["-A", "TAKARAV3", "--poly-a", "-O", str(tmp_path / "pre"), "-o", out("o1"), out("o2"), "-s", out("s1"), out("s2"),
                    "--info-file", info, "--json-file", js])
    capsys.readouterr()
    read = gunzip if gz else (lambda p: open(p, "rb").read())
    for route, tag in ((0, "o"), (1, "s")):
        for m in (0, 1):
            assert read(out(f"{tag}{m + 1}")) == streams[route][m], (tag, m)
    assert streams[0][0] and streams[1][0]
    counts = json.load(open(js))["basepair_counts"]
    assert (counts["poly_a_trimmed_read1"], counts["poly_a_trimmed_read2"]) == (want[0].polya_bp, want[1].polya_bp)
    assert counts["poly_a_trimmed"] == want[0].polya_bp + want[1].polya_bp and min(want[0].polya_bp, want[1].polya_bp) > 1000
    # the info table: a read without an adapter match has ONE row, name / -1 / the final read / its qualities / empty
    match_flags = abi.CS_F_ADAPTER5 | abi.CS_F_ADAPTER3 | abi.CS_F_INLINE | abi.CS_F_POLY
    res1 = T.records(want[0])
    rows = [line.split(b"\t") for line in open(info, "rb").read().split(b"\n") if line]
    none = {r[0]: r for r in rows if r[1] == b"-1"}
    narrowed = 0
    head_start, _stop = A.rows_keep(batch.seq1, want[0].raw["start"], want[0].raw["stop"], True)
    for i in range(N_CLI):
        if int(res1["flags"][i]) & match_flags:
            continue
        a, b = int(res1["start"][i]), int(res1["stop"][i])
        name = hostfmt.format_pair(names[i], batch.seq1[i, :batch.len1[i]].tobytes(), batch.qual1[i, :batch.len1[i]].tobytes(), res1[i],
                                   names[i], batch.seq2[i, :batch.len2[i]].tobytes(), batch.qual2[i, :batch.len2[i]].tobytes(),
                                   T.records(want[1])[i], tp)[1].split(b"\n")[0][1:]
        assert none[name] == [name, b"-1", batch.seq1[i, a:b].tobytes(), batch.qual1[i, a:b].tobytes(), b""], i
        narrowed += int(head_start[i]) > int(want[0].raw["start"][i])  # the op took a head from this read
    assert narrowed > 0


def test_g_the_run_without_the_option_is_the_run_it_was(tmp_path, capsys):
    """The same inputs without --poly-a, with --trim-polyA as the headline has it: the records are the C oracle's -- the
    parent's expectation, to which the op has added nothing -- and the report's poly-A keys stay null."""
    import oracle
    batch = cli_batch()
    names = [b"rec%d" % i for i in range(N_CLI)]
    ins = [str(tmp_path / "in1.fq"), str(tmp_path / "in2.fq")]
    util.write_fastq(ins[0], names, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(ins[1], names, batch.seq2, batch.qual2, batch.len2)
    st = planmod.CutadaptConfig()
    st.trim_polyA = True
    tp = util.compile_plan(T.TAKARA, st, True)
    (r1, _c, _s1), (r2, _c2, _s2) = util.oracle_run(tp, batch, threads=4)
    streams = {0: [b"", b""], 1: [b"", b""], 2: [b"", b""]}
    for route, a, b in util.format_batch(tp, batch, names, names, r1, None, r2):
        streams[route][0] += a
        streams[route][1] += b
    out = lambda tag: str(tmp_path / f"{tag}.fastq")
    js = str(tmp_path / "report.json")
    cli.main(ins + ["-A", "TAKARAV3", "--trim-polyA", "-O", str(tmp_path / "pre"), "-o", out("o1"), out("o2"), "-s", out("s1"), out("s2"),
                    "--json-file", js])
    capsys.readouterr()
    for route, tag in ((0, "o"), (1, "s")):
        for m in (0, 1):
            assert open(out(f"{tag}{m + 1}"), "rb").read() == streams[route][m], (tag, m)
    rep = json.load(open(js))
    assert [rep["basepair_counts"][k] for k in ("poly_a_trimmed", "poly_a_trimmed_read1", "poly_a_trimmed_read2")] == [None] * 3
    assert "poly_a_bp" not in json.dumps(rep)
