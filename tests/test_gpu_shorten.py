"""-l/--length and -L (CS_OP_SHORTEN) in every kernel against the rule of tests/shorten_rule.py.

The op lives in tile kernels of its own (trim_kernel.hip.inc, FILT_SHORTEN, scan and resolve) and in the ENDS walk of
long_kernel.hip.inc / info_kernels.hip.inc.  The C oracle does not know it, so the expected records are the rule alone
(chains without an adapter op) or the rule layered over what the oracle leaves of the same chain WITHOUT its tail --
NextSeq trimmer, quality trimmer, Shortener, N trimmer --, the way tests/test_gpu_nextseq.py layers its op.
tests/test_shorten_cpu.py builds the inputs and shows what they reach.
"""
import dataclasses
import gzip

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, run as cli
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.synth import SynthBatch

import filters_rule
import hostfmt
import qtrim_rule as R
import shorten_rule as S
import test_endtrim_cpu as TE
import test_qtrim_cpu as Q
import test_shorten_cpu as T
import util
from test_gpu_endtrim import CODED_ADAPTER, MATCH_FLAGS, Held, plan_of
from test_gpu_filters import RAW_ADAPTER, run_engine, takara_batch
from test_gpu_filters_cli import gunzip
from test_gpu_text import fastq_text, run_text_exposed

pytestmark = pytest.mark.gpu

MIN_LENGTH = T.MIN_LENGTH
RC_SCHEME = "AGATCGGAAGAGC<ACACTCTTTCCC"  # a '-' library: --auto-rc turns single-end reads round


def stripped(tp):
    """The plan without the tail of its chains (what the oracle can run), and the tails."""
    chains, tails = [], []
    for mate in (tp.r1, tp.r2):
        if mate is None:
            chains.append(None)
            continue
        ops, tail = S.split_tail(mate.ops, planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp, planmod.ShortenOp)
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
        out.append(S.apply_tail(seq, qual, res["start"], res["stop"], res["flags"], tails[m], tp.min_length))
    return out, raw


def check(held, tp, wants, what):
    """Device == rule: records (start, stop, flags), qualtrim_bp, out_bp, n_too_short.  ``wants``: an E.Ends per mate."""
    got, stats = held.run(tp)
    for mate in (0, 1):
        ends = wants[mate]
        Q.differ(got[mate], TE.records(ends), held.rows, f"{what} mate {mate + 1}: device")
        assert int(stats[mate].qualtrim_bp) == ends.cut, (what, mate)
        assert int(stats[mate].out_bp) == int((ends.stop - ends.start).sum()), (what, mate)
        assert int(stats[mate].n_too_short) == int(((ends.flags & abi.CS_F_TOO_SHORT) != 0).sum()), (what, mate)
        assert int(stats[mate].n_reads) == held.n
    return got, stats


# ---- scan kernel -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("adapter", [None, CODED_ADAPTER, RAW_ADAPTER], ids=["plain", "coded", "raw"])
def test_scan_kernel(adapter, n):
    """Reads of every length 0..40 mixed within a tile, [adapter,] cut, quality trimmer, Shortener: every length of the
    issue on one mate or the other, min_length 20 -- TooShort flips exactly at the boundary.  Plain: the rule alone;
    behind an adapter op, coded and raw tiles: the rule over the oracle's result of the chain without its tail."""
    rows = T.mixed_rows(n)
    held = Held(rows)
    front = [planmod.back(adapter, 0.0, len(adapter), flag=abi.CS_F_ADAPTER3)] if adapter else []
    half = len(T.LENGTHS) // 2
    short_counts = set()
    for l1, l2 in zip(T.LENGTHS[:half], T.LENGTHS[half:]):
        c1, c2 = T.chain(1, l1), T.chain(2, l2)
        tp = plan_of(front + c1, front + c2, min_length=MIN_LENGTH)
        if adapter:
            wants, _raw = layered(tp, [(rows.seq, rows.qual, rows.lens)] * 2)
        else:
            wants = [T.rule_ends(rows, c, min_length=MIN_LENGTH) for c in (c1, c2)]
        _got, stats = check(held, tp, wants, f"{n} reads, -l {l1} / -L {l2}, adapter {adapter}")
        short_counts |= {int(stats[0].n_too_short), int(stats[1].n_too_short)}
    assert n in short_counts  # (-l 19: every read is too short)
    if n > 1:
        assert len(short_counts) > 1  # (-l 20: not every read)


# ---- with the rest of the tail and the filters -----------------------------------------------------------------------

def test_with_the_rest_of_the_tail_and_the_filters():
    """Chains NextSeq?, QTrim(F, B), Shorten, NTrim on reads whose quality-trimmed end and N runs straddle the cut: a read
    whose bases on both sides of the cut are N loses the one inside to --trim-n AFTER the cut.  -M 11 and --max-n 3 both
    change their verdict because of the op."""
    length = 12
    r1, r2 = T.straddle_rows(length), T.straddle_rows(-length)
    batch = SynthBatch(r1.seq, r1.qual, r1.lens, r2.seq, r2.qual, r2.lens)
    c1 = T.chain(r1.f, length, 15, 20, nextseq=20, trim_n=True)
    c2 = T.chain(r2.f, -length, 0, 20, trim_n=True)
    tp = plan_of(c1, c2, min_length=length)
    tp.max_length, tp.max_n = 11, 3.0
    off = [T.chain(r1.f, None, 15, 20, nextseq=20, trim_n=True), T.chain(r2.f, None, 0, 20, trim_n=True)]
    (g1, g2), xf, stats, counts = run_engine(tp, batch)
    for m, (rows, ops, ops_off) in enumerate(((r1, c1, off[0]), (r2, c2, off[1]))):
        ends = T.rule_ends(rows, ops, min_length=length)
        want = TE.records(ends)
        Q.differ((g1, g2)[m], want, rows, f"mate {m + 1}")
        both = np.flatnonzero(np.arange(len(rows.lens)) % 4 == 0)
        assert ((ends.stop - ends.start)[both] < length).all()  # the N inside the cut went, after the cut
        x = filters_rule.xflags(rows.seq, rows.qual, want, max_length=11, max_n=3.0)
        assert np.array_equal(xf[m], x), (m, np.flatnonzero(xf[m] != x)[:5])
        assert counts[m] == {"too_many_n": int(((x & abi.CS_X_TOO_MANY_N) != 0).sum()),
                             "too_long": int(((x & abi.CS_X_TOO_LONG) != 0).sum()), "too_many_ee": 0}
        before = filters_rule.xflags(rows.seq, rows.qual, TE.records(T.rule_ends(rows, ops_off, min_length=length)), max_length=11, max_n=3.0)
        for bit in (abi.CS_X_TOO_LONG, abi.CS_X_TOO_MANY_N):  # each filter says something else because of the op
            assert int(((before & bit) != 0).sum()) > int(((x & bit) != 0).sum()), (m, bit)
        assert (x & abi.CS_X_TOO_LONG).any() and not (x & abi.CS_X_TOO_LONG).all()
        assert int(stats[m].qualtrim_bp) == ends.cut > 0  # the op adds nothing to the quality trimmers' count
        assert int(stats[m].out_bp) == int((ends.stop - ends.start).sum()) > 0
        assert int(stats[m].n_too_short) == int(((ends.flags & abi.CS_F_TOO_SHORT) != 0).sum()) > 0


# ---- resolve kernel --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lengths", [(19, -20), (-21, 20), (S.INT32_MIN, 0)], ids=str)
def test_resolve_kernel(lengths):
    """[adapter, cut, trimmer, Shortener, N trimmer] without the filter: every non-empty read goes to the exact DP and
    finishes its chain -- the op with it -- in the resolve kernel."""
    rows = Q.planted(T.mixed_rows(130), [Q.ADAPTER])
    op = Q.adapter_op(Q.ADAPTER)
    end, flags = Q.after_adapter(rows, op)
    lens = rows.lens.astype(np.int64)
    assert 0 < int((end < lens).sum())
    chains = [T.chain(1, lengths[0], trim_n=True), T.chain(2, lengths[1], 15, 25)]
    wants = [T.rule_ends(rows, c, end, flags, MIN_LENGTH) for c in chains]
    tp = plan_of([op] + chains[0], [op] + chains[1], use_filter=False, min_length=MIN_LENGTH)
    layer, _raw = layered(tp, [(rows.seq, rows.qual, rows.lens)] * 2)
    for m in (0, 1):
        assert np.array_equal(TE.records(layer[m]), TE.records(wants[m]))
    _got, stats = check(Held(rows), tp, wants, f"-l {lengths[0]} / -L {lengths[1]} behind an adapter, no filter")
    for mate in (0, 1):
        assert int(stats[mate].n_exact_dp) == int((lens > 0).sum()) > 0


# ---- long-read kernel: four reads of 70 000 nt -----------------------------------------------------------------------

LONG = 70000


def long_rows(seed):
    """Four reads of 70 000 bases: low qualities over the last 1000 * i bases of read i, ``N`` on both sides of positions
    65 536 and 66 000 from either end."""
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(4, LONG))
    qual = np.full((4, LONG), T.HIGH, dtype=np.uint8)
    for i in range(4):
        qual[i, LONG - 1000 * i:] = T.LOW
        for at in (65536, 66000):
            seq[i, at + 1:at + 3] = ord("N")              # (f = 2: the cut of -l at lies between these two)
            seq[i, LONG - 1000 * i - at - 1:LONG - 1000 * i - at + 1] = ord("N")
    return R.Rows(seq, qual, np.full(4, LONG, dtype=np.int64), 2)


@pytest.mark.parametrize("l1,l2", [(66000, -66000), (65536, 70001), (-65536, 66000)])
def test_long_read_kernel(l1, l2):
    """Intervals beyond 16 bits: a length compared through a uint16_t would keep 464 (66 000), nothing (65 536) or 4 465
    (70 001) bases.  Pairs, -L different from -l."""
    rows = long_rows(7)
    c1, c2 = T.chain(2, l1, trim_n=True), T.chain(2, l2, trim_n=True)
    tp = plan_of(c1, c2, min_length=MIN_LENGTH)
    lens = rows.lens
    ends = [S.apply_tail(rows.seq, rows.qual, 2, lens, 0, T.tail_of(c), MIN_LENGTH) for c in (c1, c2)]
    want = [TE.records(e) for e in ends]  # (16-bit fields: not read below)
    names = [b"long%d" % i for i in range(4)]
    text = fastq_text(names, rows.seq, rows.qual, lens)
    recs = [[b"", b""] for _ in range(2)]
    for i in range(4):
        pair = []
        for m in (0, 1):
            a, b = int(ends[m].start[i]), int(ends[m].stop[i])
            assert 60000 < b - a <= min(abs((l1, l2)[m]), LONG - 2)
            pair.append(hostfmt.fastq_record(names[i], rows.seq[i].tobytes(), rows.qual[i].tobytes(), a, b))
        assert not (int(want[0]["flags"][i]) | int(want[1]["flags"][i])) & abi.CS_F_TOO_SHORT
        recs[0][0] += pair[0]
        recs[0][1] += pair[1]
    got = run_text_exposed(tp, text, text, 4, 64)
    assert got.n_long == [4, 4] and got.counts == [4, 0, 0]
    for m in (0, 1):
        if got.streams[0][m] != recs[0][m]:
            out = got.streams[0][m].split(b"\n")
            raise AssertionError((m, [len(out[4 * i + 1]) for i in range(4)], (ends[m].stop - ends[m].start).tolist()))
        assert int(got.stats[m].out_bp) == int((ends[m].stop - ends[m].start).sum())
        assert int(got.stats[m].qualtrim_bp) == ends[m].cut == 6000


# ---- the command line ------------------------------------------------------------------------------------------------

def gz_write(path, data):
    with gzip.open(path, "wb") as fh:
        fh.write(data)


def expected_records(tp, batch, names):
    mates = [(batch.seq1, batch.qual1, batch.len1)] + ([(batch.seq2, batch.qual2, batch.len2)] if tp.paired else [])
    wants, raw = layered(tp, mates)
    res = []
    for m in range(len(mates)):
        r = TE.records(wants[m])
        r["cap_off"], r["cap_len"] = raw[m]["cap_off"], raw[m]["cap_len"]
        res.append(r)
    return util.format_batch(tp, batch, names, names, res[0], None, res[1] if tp.paired else None), res


def settings(length, length_r2=None, auto_rc=False):
    st = planmod.CutadaptConfig()
    st.length, st.length_r2, st.auto_rc = length, length_r2, auto_rc
    return st


def as_fasta(stream):
    lines = stream.split(b"\n")
    return b"".join(b">" + lines[k][1:] + b"\n" + lines[k + 1] + b"\n" for k in range(0, len(lines) - 1, 4))


def info_batch():
    """Three reads of 50, 40 and 25 random bases of high quality: no adapter is expected to match."""
    rng = np.random.default_rng(3)
    lens = np.array([50, 40, 25], dtype=np.uint16)
    seq = np.full((3, 52), ord("N"), dtype=np.uint8)
    qual = np.full((3, 52), R.PAD, dtype=np.uint8)
    for i in range(3):
        seq[i, :lens[i]] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(lens[i]))
        qual[i, :lens[i]] = T.HIGH
    return SynthBatch(seq, qual, lens, None, None, None)


def test_info_table_carries_the_shortened_read(tmp_path, capsys):
    """--info-file: a read without a match has the shortened read in its final-sequence and quality columns."""
    single = info_batch()
    names = [b"r%d" % i for i in range(3)]
    path = str(tmp_path / "in.fq.gz")
    util.write_fastq(path, names, single.seq1, single.qual1, single.len1)
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], settings(-30), False)
    recs, res = expected_records(tp, single, names)
    info = str(tmp_path / "info.tsv")
    cli.main([path, "-A", "TAKARAV3", "-l", "-30", "-O", str(tmp_path / "pre"), "-o", str(tmp_path / "o.fastq.gz"), "-s", str(tmp_path / "s.fastq.gz"),
              "--info-file", info])
    capsys.readouterr()
    rows = [line.split(b"\t") for line in open(info, "rb").read().split(b"\n") if line]
    none = [r for r in rows if r[1] == b"-1"]
    want_none = []
    for i, (_rt, r1, _r2) in enumerate(recs):
        if int(res[0]["flags"][i]) & MATCH_FLAGS == 0:
            name, seq, _plus, qual = r1.split(b"\n")[:4]
            want_none.append([name[1:], b"-1", seq, qual, b""])
    assert none == want_none and len(none) >= 2
    assert any(len(r[2]) == 30 for r in none)


CLI_CASES = ["single", "paired", "interleaved", "auto-rc", "fasta", "read2-only", "record-path"]


@pytest.mark.parametrize("case", CLI_CASES)
def test_cli_end_to_end(case, tmp_path, capsys, monkeypatch):
    """A dozen records, .gz outputs compared after decompression, byte for byte with tests/hostfmt.py fed the rule's
    intervals: -l 30 single-end; -l 30 -L -25 paired; -l 30 --interleaved; -l 30 --auto-rc on a '-' library; FASTA in; and
    -L -25 alone, which shortens read 2 only; and the paired run on the record path (CUTSEQ_TEXT_PATH=0)."""
    batch = takara_batch(12, 70, 81, clip=True)
    names = [b"rec%d" % i for i in range(12)]
    paired = case in ("paired", "interleaved", "read2-only", "record-path")
    if case == "record-path":
        monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    else:
        monkeypatch.delenv("CUTSEQ_TEXT_PATH", raising=False)
    l1 = None if case == "read2-only" else 30
    l2 = -25 if case in ("paired", "read2-only", "record-path") else None
    scheme = RC_SCHEME if case == "auto-rc" else BUILDIN_ADAPTERS["TAKARAV3"]
    st = settings(l1, l2, auto_rc=case == "auto-rc")
    tp = util.compile_plan(scheme, st, paired)
    if case == "fasta":
        inert = np.where(np.arange(batch.stride)[None, :] < batch.len1[:, None], ord("~"), 0).astype(np.uint8)
        data = SynthBatch(batch.seq1, inert, batch.len1, None, None, None)
    elif paired:
        data = batch
    else:
        data = SynthBatch(batch.seq1, batch.qual1, batch.len1, None, None, None)
    recs, res = expected_records(tp, data, names)
    kept = [int(r["stop"]) - int(r["start"]) for r in res[0]]
    if l1 is None:
        assert max(kept) > 30 and not any(isinstance(o, planmod.ShortenOp) for o in tp.r1.ops)
    else:
        assert max(kept) == 30 and kept.count(30) >= 3 and min(kept) < 30
    if l2 is not None:
        kept2 = [int(r["stop"]) - int(r["start"]) for r in res[1]]
        assert max(kept2) == 25 and kept2.count(25) >= 3
    if case == "auto-rc":
        assert tp.reverse_complement
    want = {0: [b"", b""], 1: [b"", b""]}
    for route, r1, r2 in recs:
        assert route in (0, 1)
        want[route][0] += r1
        if case == "interleaved":
            want[route][0] += r2
        elif r2 is not None:
            want[route][1] += r2
    assert want[0][0] and want[1][0]
    ext = "fa.gz" if case == "fasta" else "fastq.gz"
    out = lambda tag: str(tmp_path / f"{tag}.{ext}")
    if case == "fasta":
        src = str(tmp_path / "in.fa")
        open(src, "wb").write(b"".join(b">" + names[i] + b"\n" + batch.seq1[i, :int(batch.len1[i])].tobytes() + b"\n" for i in range(12)))
        inputs = [src]
    elif case == "interleaved":
        t1 = fastq_text(names, batch.seq1, batch.qual1, batch.len1).split(b"\n")
        t2 = fastq_text(names, batch.seq2, batch.qual2, batch.len2).split(b"\n")
        woven = b"".join(b"\n".join(t[4 * i:4 * i + 4]) + b"\n" for i in range(12) for t in (t1, t2))
        src = str(tmp_path / "in12.fq.gz")
        gz_write(src, woven)
        inputs = [src, "--interleaved"]
    else:
        inputs = [str(tmp_path / "in1.fq.gz")]
        util.write_fastq(inputs[0], names, batch.seq1, batch.qual1, batch.len1)
        if paired:
            inputs.append(str(tmp_path / "in2.fq.gz"))
            util.write_fastq(inputs[1], names, batch.seq2, batch.qual2, batch.len2)
    two = case in ("paired", "read2-only", "record-path")
    argv = inputs + (["-a", RC_SCHEME, "--auto-rc"] if case == "auto-rc" else ["-A", "TAKARAV3"])
    argv += (["-l", str(l1)] if l1 is not None else []) + (["-L", str(l2)] if l2 is not None else [])
    argv += ["-O", str(tmp_path / "pre"), "-o", out("o1")] + ([out("o2")] if two else []) + ["-s", out("s1")] + ([out("s2")] if two else [])
    cli.main(argv)
    capsys.readouterr()
    shape = as_fasta if case == "fasta" else (lambda b: b)
    for route, tag in ((0, "o"), (1, "s")):
        for m in range(2 if two else 1):
            assert gunzip(out(f"{tag}{m + 1}")) == shape(want[route][m]), (case, tag, m)
