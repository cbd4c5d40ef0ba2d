"""--nextseq-trim (NextseqQualityTrimmer, CS_OP_NEXTSEQ) and -Q on the CPU side: the command line, the plan and the C ABI,
the two statements of the rule in tests/nextseq_rule.py against each other and a hand-written table, and the inputs of
tests/test_gpu_nextseq.py -- which are built here -- held to what that test needs of them, by the rules alone."""
import ctypes as C
import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, run
from cutseq_amd.common import BUILDIN_ADAPTERS

import endtrim_rule as E
import nextseq_rule as N
import qtrim_rule as R
import universe as U

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])

# ---- inputs and plans, shared with the GPU tests ---------------------------------------------------------------------

# (nextseq cutoff, -q front, -q back): the quality trimmer behind the op has work of its own
SETTINGS = ((20, 0, 20), (20, 0, 25), (10, 15, 30), (2, 20, 0), (41, 0, 20))
# NS1's six symbols (base, quality byte): an A that is good, neutral and bad under cutoff 20, a G of high quality -- the
# dark cycle --, a g of high quality -- an ordinary base --, a G of the lowest quality
SYMBOLS = ((ord("A"), R.qbyte(-1)), (ord("A"), R.qbyte(0)), (ord("A"), R.qbyte(+1)),
           (N.G, ord("I")), (ord("g"), ord("I")), (N.G, ord("!")))
NS_STRIDE = 16


def chain(f, nextseq, front=0, back=None, base=33, trim_n=False):
    ops = ([planmod.CutOp(f)] if f else []) + [planmod.NextSeqTrimOp(nextseq, base)]
    if back is not None:
        ops.append(planmod.QTrimOp(back, base, cutoff_front=front))
    return ops + ([planmod.NTrimOp()] if trim_n else [])


def ns1(f: int) -> R.Rows:
    """Every string of length 0..7 over SYMBOLS behind f bytes (``G`` of quality ``!``, for a ``CutOp(+f)`` to remove: a
    kernel that read them would count them), the strings without a ``g`` first -- whole tiles of that part keep the scan
    kernel's fast re-coding --, rows padded with the same bytes."""
    body, ln = U.reads_universe("ABCDEF", 7, stride=8)
    has_g = (body == ord("E")).any(axis=1)
    order = np.concatenate([np.flatnonzero(~has_g), np.flatnonzero(has_g)])
    body, ln = body[order], ln[order].astype(np.int64)
    lut_s, lut_q = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    for ch, (b, q) in zip(b"ABCDEF", SYMBOLS):
        lut_s[ch], lut_q[ch] = b, q
    n = len(ln)
    seq = np.full((n, NS_STRIDE), N.G, dtype=np.uint8)
    qual = np.full((n, NS_STRIDE), R.PAD, dtype=np.uint8)
    inside = np.arange(8)[None, :] < ln[:, None]
    seq[:, f:f + 8][inside] = lut_s[body][inside]
    qual[:, f:f + 8][inside] = lut_q[body][inside]
    return R.Rows(seq, qual, (ln + f).astype(np.uint16), f)


def full_rows(f: int, stride: int = 1536):
    """One full row of ``G`` and one of ``g``, both of quality ``~`` -> (Rows, the rows that mean the same to the plain
    trimmer under cutoff 20: every base delta +1 -- everything goes --, every base ``~`` -- nothing goes)."""
    lens = np.array([stride, stride], dtype=np.uint16)
    seq = np.stack([np.full(stride, N.G, np.uint8), np.full(stride, ord("g"), np.uint8)])
    qual = np.full((2, stride), ord("~"), dtype=np.uint8)
    plain = qual.copy()
    plain[0, f:] = R.qbyte(+1)
    return R.Rows(seq, qual, lens, f), R.Rows(np.full((2, stride), ord("A"), np.uint8), plain, lens, f)


def join(a: R.Rows, b: R.Rows) -> R.Rows:
    return R.Rows(np.concatenate([a.seq, b.seq]), np.concatenate([a.qual, b.qual]), np.concatenate([a.lens, b.lens]), a.f)


@functools.lru_cache(maxsize=3)
def family(name: str):
    """"NS1:f" -> Rows;  "NSG2A:f", "NSG2B:f", "NSG3:f", "NSG4:f" -> (Rows with the Gs, the qtrim_rule family they came
    from): ``qtrim_rule.expected`` of the second is the expected result of the first."""
    kind, _, arg = name.partition(":")
    f = int(arg)
    if kind == "NS1":
        return ns1(f)
    plain = {"NSG2A": lambda: R.f2("A", f), "NSG2B": lambda: R.f2("B", f), "NSG3": lambda: R.f3(f)[0],
             "NSG4": lambda: R.f4(f)}[kind]()
    rows = N.with_g(plain)
    if kind == "NSG4":
        more, more_plain = full_rows(f)
        rows, plain = join(rows, more), join(plain, more_plain)
    return rows, plain


def scan_cases():
    """-> [(family, [(mate 1 (f, nextseq, front, back), mate 2 (...)), ...])]: paired plans whose mates run different
    chains over the same rows.  Three plans a family: every family meets all five settings, every setting every f."""
    k = len(SETTINGS)
    return [(f"NS1:{f}", [((f, *SETTINGS[(f + 2 * i) % k]), ((f + 1 + i) % 4, *SETTINGS[(f + 2 * i + 1) % k])) for i in range(3)])
            for f in range(4)]


SCAN_CASES = scan_cases()
DEEP_CASES = [f"{kind}:{f}" for kind, fs in (("NSG2A", range(4)), ("NSG2B", range(4)), ("NSG3", range(4)), ("NSG4", (0, 3)))
              for f in fs]


def rule_ends(rows: R.Rows, setting, trim_n=False, end=None, flags=0, min_length=0) -> E.Ends:
    """What ``[CutOp(+f), NextSeqTrimOp(nextseq), QTrimOp(front, back)[, NTrimOp()]]`` leaves of rows whose interval ends
    at ``end`` (``back`` None: a chain without the quality trimmer)."""
    f, nextseq, front, back = setting
    lens = rows.lens.astype(np.int64)
    end = lens if end is None else np.asarray(end, dtype=np.int64)
    begin = np.minimum(f, end)
    tail = N.Tail(nextseq, 33, E.Tail(front, back, 33, trim_n))
    return N.apply_tail(rows.seq, rows.qual, begin, end, flags, tail, min_length)


def plain_ends(plain: R.Rows, f: int, min_length=0) -> E.Ends:
    """``qtrim_rule.expected`` of the rows an NSG family came from, as an E.Ends."""
    start, stop, flags, cut = R.expected(plain, f, R.CUTOFF, R.BASE)
    return E.Ends(start, stop, flags | np.where(stop - start < min_length, E.F_TOO_SHORT, 0), cut)


# ---- the rule --------------------------------------------------------------------------------------------------------

CLAMP_SEQ = b"G" * 100 + b"A" + b"G" * 300

BY_HAND = [  # (bases, qualities, cutoff, base, stop)
    (b"", b"", 20, 33, 0),
    (b"AAAA", b"IIII", 20, 33, 4),            # good bases: the first sum is negative
    (b"AAGG", b"IIII", 20, 33, 2),            # 1, 2, then the A ends the walk
    (b"AAgg", b"IIII", 20, 33, 4),            # 'g' is an ordinary base
    (b"GGGG", b"IIII", 20, 33, 0),
    (b"AAGG", b"II~!", 20, 33, 2),            # whatever the G's quality byte says
    (b"GAGG", b"I5II", 20, 33, 0),            # a neutral A between Gs: 1, 2, 2, 3
    (b"GAGG", b"IIII", 20, 33, 2),
    (b"AGAG", b"II4I", 20, 33, 1),            # 1, 2 (the A adds 1), 3, then -17
    (b"GGGA", b"!!!I", 20, 33, 4),            # Gs behind a good last base are not reached
    (b"AG", b"!!", 0, 33, 1),                 # cutoff 0: the G still adds 1, the A of quality 0 nothing
    (b"AGG", b"hhh", 20, 64, 1),
    (CLAMP_SEQ, b"I" * 401, -5000, 33, 101),  # the walk breaks at the A ...
    (CLAMP_SEQ, b"I" * 401, -34, 33, 0),      # ... at the lowest accepted cutoff it does not: no clamp can stand in
    (CLAMP_SEQ, b"I" * 401, 223, 33, 0),
    (CLAMP_SEQ.lower(), b"I" * 401, -34, 33, 401),
]


def test_rule_by_hand():
    for seq, qual, cutoff, base, want in BY_HAND:
        assert N.stop(seq, qual, cutoff, base) == want, (seq[-8:], qual[-8:], cutoff)
        s = np.frombuffer(seq, np.uint8).reshape(1, -1) if seq else np.zeros((1, 4), np.uint8)
        q = np.frombuffer(qual, np.uint8).reshape(1, -1) if qual else np.zeros((1, 4), np.uint8)
        assert int(N.stops(s, q, 0, len(seq), cutoff, base)[0]) == want, (seq[-8:], cutoff)
    assert R.clamp(-5000) == -34  # (what cs_plan_create does to a CS_OP_QTRIM cutoff: not to this op's)


def test_the_two_statements_agree_on_ns1():
    rows = family("NS1:1")
    lens = rows.lens.astype(np.int64)
    begin = np.minimum(1, lens)
    pick = np.arange(0, len(lens), 97)
    assert len(pick) >= 3000
    for cutoff in (20, 10, 2, 41, -34, 223):
        got = N.stops(rows.seq, rows.qual, begin, lens, cutoff)
        for i in pick:
            s, e = int(begin[i]), int(lens[i])
            assert int(got[i]) == N.stop(rows.seq[i, s:e].tobytes(), rows.qual[i, s:e].tobytes(), cutoff), (int(i), cutoff)
    # inside rows: intervals that end before the row does
    end = np.maximum(begin, lens - (np.arange(len(lens)) % 3))
    got = N.stops(rows.seq, rows.qual, begin, end, 20)
    for i in pick:
        s, e = int(begin[i]), int(end[i])
        assert int(got[i]) == N.stop(rows.seq[i, s:e].tobytes(), rows.qual[i, s:e].tobytes(), 20), int(i)


def test_apply_and_split_tail():
    ops = [planmod.CutOp(2)] + chain(0, 20, 15, 10, trim_n=True)
    front, tail = N.split_tail(ops, planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp)
    assert front == [planmod.CutOp(2)] and tail == N.Tail(20, 33, E.Tail(15, 10, 33, True))
    front, tail = N.split_tail(chain(3, 7), planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp)
    assert front == [planmod.CutOp(3)] and tail == N.Tail(7, 33, E.Tail())
    front, tail = N.split_tail([planmod.CutOp(3), planmod.QTrimOp(20)], planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp)
    assert front == [planmod.CutOp(3)] and tail == N.Tail(None, 33, E.Tail(0, 20, 33, False))
    seq = np.frombuffer(b"NAAAAAGG", np.uint8).reshape(1, -1)
    qual = np.frombuffer(b"IIII77II", np.uint8).reshape(1, -1)
    # the op takes GG (1, 2; the A of quality 22 makes it 0, the next one ends the walk), the quality trimmer behind it,
    # at cutoff 25, the two As of quality 22 (3, 6, then -9), the N trimmer the N in front
    ends = N.apply_tail(seq, qual, 0, 8, 0, N.Tail(20, 33, E.Tail(0, 25, 33, True)), min_length=4)
    assert (int(ends.start[0]), int(ends.stop[0]), int(ends.flags[0]), ends.cut) == (1, 4, N.F_QTRIMMED | E.F_TOO_SHORT, 4)
    ends = N.apply_tail(seq, qual, 0, 8, 0, N.Tail(20, 33, E.Tail()), min_length=4)
    assert (int(ends.start[0]), int(ends.stop[0]), int(ends.flags[0]), ends.cut) == (0, 6, N.F_QTRIMMED, 2)
    ends = N.apply_tail(seq, qual, 0, 8, 0, N.Tail(None, 33, E.Tail(0, 20, 33, False)))
    assert (int(ends.start[0]), int(ends.stop[0]), int(ends.flags[0]), ends.cut) == (0, 8, 0, 0)


# ---- the command line ------------------------------------------------------------------------------------------------

def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


@pytest.mark.parametrize("argv, nextseq, q1, q2", [
    (["--nextseq-trim", "20"], 20, (0, 20), (0, 20)),
    (["-Q", "5"], None, (0, 20), (0, 5)),
    (["-Q", "3,5"], None, (0, 20), (3, 5)),
    (["--nextseq-trim", "10", "-q", "15,30", "-Q", "25", "--trim-n"], 10, (15, 30), (0, 25)),
    (["-q", "15,10"], None, (15, 10), (15, 10)),
    (["--nextseq-trim", "-34"], -34, (0, 20), (0, 20)),
    (["--nextseq-trim", "223", "-Q", "0"], 223, (0, 20), (0, 0)),
    ([], None, (0, 20), (0, 20)),
])
def test_cli_parses_the_options_into_args_settings_and_plans(argv, nextseq, q1, q2):
    args = run.resolve_args(_args(*argv))
    given = "-Q" in argv
    assert args.nextseq_trim == nextseq and (args.min_quality_front, args.min_quality) == q1
    assert (args.min_quality_front_r2, args.min_quality_r2) == (q2 if given else (None, None))
    st = run.settings_from_args(args)
    assert st.nextseq_trim == nextseq and (st.min_quality_front, st.min_quality) == q1
    assert (st.min_quality_front_r2, st.min_quality_r2) == (q2 if given else (None, None))
    trim_n = "--trim-n" in argv
    plain = planmod.compile_paired(TAKARA, run.settings_from_args(run.resolve_args(_args())))
    tp, single = planmod.compile_paired(TAKARA, st), planmod.compile_single(TAKARA, st)
    assert tp.has_nextseq is (nextseq is not None) and single.has_nextseq is (nextseq is not None)
    for mate, base, want in ((tp.r1, plain.r1, q1), (tp.r2, plain.r2, q2), (single.r1, None, q1)):  # (-Q: mate 2 alone)
        tail = [planmod.QTrimOp(want[1], 33, cutoff_front=want[0])] + ([planmod.NTrimOp()] if trim_n else [])
        if nextseq is not None:
            tail.insert(0, planmod.NextSeqTrimOp(nextseq, 33))  # immediately in front of the chain's QTrimOp
        assert mate.ops[-len(tail):] == tail
        assert sum(isinstance(o, planmod.QTrimOp) for o in mate.ops) == 1
        assert sum(isinstance(o, planmod.NextSeqTrimOp) for o in mate.ops) == (nextseq is not None)
        if base is not None:  # everything in front of the tail is the plain plan's
            assert mate.ops[:-len(tail)] == base.ops[:-1]


def test_settings_defaults():
    st = planmod.CutadaptConfig()
    assert st.nextseq_trim is None and st.min_quality_r2 is None and st.min_quality_front_r2 is None
    args = _args()
    assert args.nextseq_trim is None and args.min_quality_r2 is None and args.min_quality_front_r2 is None
    assert repr(planmod.NextSeqTrimOp(20)) == "NextseqQualityTrimmer(cutoff=20, base=33)"


@pytest.mark.parametrize("argv, message", [
    (["--nextseq-trim", "224"], "--nextseq-trim: the cutoff must lie in [-34, 223] (got 224)"),
    (["--nextseq-trim", "-35"], "--nextseq-trim: the cutoff must lie in [-34, 223] (got -35)"),
    (["--nextseq-trim", "-5000"], "--nextseq-trim: the cutoff must lie in [-34, 223]"),
])
def test_cli_refuses_a_cutoff_outside_the_range_of_the_abi(argv, message, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args(*argv))
    assert exc.value.code == 1 and message in caplog.text  # the CLI's own check (_fail), not argparse's usage error (2)
    assert (abi.CS_Q_SUM_LOW - 33, abi.CS_Q_SUM_HIGH - 33) == (-34, 223) == (N.CUTOFF_LOW - 33, N.CUTOFF_HIGH - 33)


def test_cli_refuses_the_second_reads_cutoff_without_a_second_read(caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "-Q", "5"]))
    assert exc.value.code == 1 and "-Q" in caplog.text and "two input files" in caplog.text


@pytest.mark.parametrize("bad", ["1,2,3", "a", "1,", "1.5"])
def test_cli_refuses_malformed_cutoffs(bad, capsys):
    with pytest.raises(SystemExit) as exc:
        _args("-Q", bad)
    assert exc.value.code == 2 and "-Q" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        _args("--nextseq-trim", "1,2")
    assert exc.value.code == 2


@pytest.mark.parametrize("first", [b">", b"#"])
def test_nextseq_trim_refuses_fasta_input(tmp_path, caplog, first):
    fa = tmp_path / "reads.fa"
    fa.write_bytes((b"# a comment\n" if first == b"#" else b"") + b">r1\nACGTACGTACGTACGTACGTGGGG\n")
    with pytest.raises(SystemExit) as exc:
        run.main([str(fa), "-A", "TAKARAV3", "--nextseq-trim", "20", "-o", str(tmp_path / "out.fa")])
    assert exc.value.code == 1
    assert f"--nextseq-trim needs qualities: {fa} is a FASTA file." in caplog.text


def test_the_single_end_chain_keeps_the_order_of_the_tail():
    st = planmod.CutadaptConfig()
    st.auto_rc, st.trim_n, st.nextseq_trim, st.trim_polyA = True, True, 20, True
    tp = planmod.compile_single(planmod.BarcodeConfig("AGATCGGAAGAGC<ACACTCTTTCCC"), st)
    assert tp.reverse_complement
    steps = run.dry_run_steps(tp)
    assert steps[-3:] == ["QualityTrimmer(cutoff_front=0, cutoff_back=20, base=33)", "NEndTrimmer()", "ReverseComplementConverter()"]
    assert steps[-4] == "NextseqQualityTrimmer(cutoff=20, base=33)" and "NonInternal" in steps[-5]  # behind the poly-A step


def test_dry_run_and_help(capsys):
    def single(*extra):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", *extra])
        return capsys.readouterr().out

    plain = single()
    assert "Nextseq" not in plain
    on = single("--nextseq-trim", "18")
    lines = on.splitlines()
    at = next(i for i, line in enumerate(lines) if "NextseqQualityTrimmer" in line)
    assert lines[at] == f"Step {at + 1}: NextseqQualityTrimmer(cutoff=18, base=33)"
    assert lines[at + 1] == f"Step {at + 2}: QualityTrimmer(cutoff_front=0, cutoff_back=20, base=33)"
    del lines[at]
    assert [re.sub(r"^Step \d+: ", "", x) for x in lines] == [re.sub(r"^Step \d+: ", "", x) for x in plain.splitlines()]
    # paired: the steps come in pairs, -Q shows in the second half of the trimmer's
    st = run.settings_from_args(run.resolve_args(_args("--nextseq-trim", "18", "-Q", "3,5")))
    steps = run.dry_run_steps(planmod.compile_paired(TAKARA, st))
    assert steps[-2] == "(NextseqQualityTrimmer(cutoff=18, base=33), NextseqQualityTrimmer(cutoff=18, base=33))"
    assert steps[-1] == ("(QualityTrimmer(cutoff_front=0, cutoff_back=20, base=33), "
                         "QualityTrimmer(cutoff_front=3, cutoff_back=5, base=33))")
    assert steps[:-2] == run.dry_run_steps(planmod.compile_paired(TAKARA, run.settings_from_args(run.resolve_args(_args()))))[:-1]
    text = run.build_parser().format_help()
    assert "--nextseq-trim" in text and re.search(r"-Q \[5'CUTOFF,\]3'CUTOFF", text)


def test_readme_lists_the_options_as_built():
    readme = (ROOT / "README.md").read_text()
    assert "--nextseq-trim" in readme and "`-Q" in readme
    assert not re.search(r"Not built:[^\n]*(--nextseq-trim|`-Q`)", readme)


# ---- the plan and the C ABI ------------------------------------------------------------------------------------------

def test_pack_puts_the_op_where_the_header_says():
    arr = planmod.pack_ops(chain(3, 18, 15, 10, trim_n=True))
    assert [int(c.kind) for c in arr] == [abi.CS_OP_CUT, abi.CS_OP_NEXTSEQ, abi.CS_OP_QTRIM, abi.CS_OP_NTRIM]
    assert abi.CS_OP_NEXTSEQ == 6
    op = arr[1]
    assert (op.q_cutoff, op.q_base, op.q_cutoff_front, op.stat_slot) == (18, 33, 0, 1)
    raw = bytearray(bytes(op))
    assert len(raw) == 284 and raw[0] == 6
    at = abi.cs_op.q_cutoff.offset
    assert int.from_bytes(raw[at:at + 2], "little", signed=True) == 18 and raw[abi.cs_op.q_base.offset] == 33
    for field, size in ((abi.cs_op.kind, 1), (abi.cs_op.q_cutoff, 2), (abi.cs_op.q_base, 1), (abi.cs_op.stat_slot, abi.cs_op.stat_slot.size)):
        raw[field.offset:field.offset + size] = bytes(size)
    assert bytes(raw) == bytes(284)  # kind, cutoff, base, stat_slot: nothing else
    # no clamp on the way: what cs_plan_create refuses arrives there as given
    assert planmod.pack_ops([planmod.NextSeqTrimOp(-5000)])[0].q_cutoff == -5000
    assert planmod.pack_ops([planmod.NextSeqTrimOp(20, 64)])[0].q_base == 64


def test_abi_version_and_sizes_are_unchanged_and_the_header_agrees():
    assert abi.CS_ABI_VERSION == 7 and C.sizeof(abi.cs_op) == 284
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"#define CS_ABI_VERSION 7\b", header) and re.search(r"\bCS_OP_NEXTSEQ = 6\b", header)
    assert re.search(r"\bCS_OP_NTRIM = 5\b", header)
    src = '''#include <stdio.h>
    #include "cutseq_hip.h"
    int main(void){ printf("%zu %d %d\\n", sizeof(cs_op), (int)CS_OP_NEXTSEQ, (int)CS_ABI_VERSION); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        got = subprocess.run([f"{d}/p"], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == [284, abi.CS_OP_NEXTSEQ, 7]


# ---- the GPU test's inputs do their job (the rules alone) ------------------------------------------------------------

def test_ns1_exposes_a_kernel_that_ignores_g_or_folds_case():
    rows = family("NS1:0")
    n = len(rows.lens)
    assert n == 335923 == (6 ** 8 - 1) // 5 and rows.seq.shape[1] == NS_STRIDE
    no_g = ~(rows.seq[:, :8] == ord("g")).any(axis=1)
    first = (5 ** 8 - 1) // 4
    assert no_g[:first].all() and not no_g[first:].any() and first // 64 > 1000  # whole tiles without a g, then none
    lens = rows.lens.astype(np.int64)
    want = N.stops(rows.seq, rows.qual, 0, lens, 20)
    plain = R.stops(rows.qual, 0, lens, 20)                                     # a kernel that ignores G
    folded = N.stops(rows.seq, rows.qual, 0, lens, 20, g=(N.G, ord("g")))       # a kernel that folds case
    blind, fold = int((want != plain).sum()), int((want != folded).sum())
    print(f"NS1 at cutoff 20: {blind} rows differ from the plain trimmer, {fold} from a case-folding reading of G")
    assert blind > n // 3 and fold > n // 3
    assert (blind, fold) == (126437, 184588)
    # every family starts its intervals at another offset in the dword, and the quality trimmer behind the op works
    # (a trimmer of the op's own cutoff, or a lower one, finds nothing behind it: three settings of the five have work)
    for name, plans in SCAN_CASES[1::2]:
        rows = family(name)
        more = set()
        for setting in (m for pair in plans for m in pair):
            f, nextseq, front, back = setting
            alone = rule_ends(rows, (f, nextseq, 0, None))
            both = rule_ends(rows, setting)
            assert alone.cut > 0 and both.cut >= alone.cut, (name, setting)
            if both.cut > alone.cut + 1000:
                more.add(setting[1:])
        assert {s[1:] for pair in plans for s in pair} == set(SETTINGS) and len(more) >= 3, name


def test_nsg_families_mean_what_their_originals_mean():
    seen, under_g = set(), set()
    for name in DEEP_CASES:
        rows, plain = family(name)
        f = rows.f
        lens = rows.lens.astype(np.int64)
        is_g = rows.seq == N.G
        assert is_g.any()
        under_g |= set(np.unique(rows.qual[is_g]).tolist())
        seen |= set(np.unique(rows.seq).tolist())
        begin = np.minimum(f, lens)
        want = plain_ends(plain, f)
        got = N.stops(rows.seq, rows.qual, begin, lens, R.CUTOFF)
        assert np.array_equal(begin + got, want.stop) and np.array_equal(begin, want.start)
        # ... and not to a trimmer that reads the Gs' quality bytes
        # (NSG3's few Gs sit at odd positions for odd f, all of quality '!': its job is the occupancy of the wave walk)
        blind = int((R.stops(rows.qual, begin, lens, R.CUTOFF) != got).sum())
        assert blind > len(lens) // 10 or name.startswith("NSG3"), (name, blind)
        if name.startswith("NSG4"):
            assert rows.seq.shape[1] == 1536 and (got[-2], got[-1]) == (0, 1536 - f)
            assert (rows.seq[-2] == N.G).all() and (rows.seq[-1] == ord("g")).all() and (rows.qual[-2:] == ord("~")).all()
    assert {N.G, ord("g"), ord("A")} <= seen and under_g == {ord("~"), ord("!")}
