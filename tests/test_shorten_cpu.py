"""-l/--length and -L (cutadapt's Shortener, CS_OP_SHORTEN) on the CPU side: the rule of tests/shorten_rule.py in its two
forms, the command line, the plan and the C ABI, and the inputs of tests/test_gpu_shorten.py -- which are built here --
held to what that test needs of them, by the rule alone."""
import ctypes as C
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
import shorten_rule as S

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])

# ---- inputs and plans, shared with the GPU tests ---------------------------------------------------------------------

LENGTHS = (0, 1, 19, 20, 21, 40, 41, -1, -20, -41, S.INT32_MAX, S.INT32_MIN)  # the scan-kernel case
MIN_LENGTH = 20
STRIDE = 40
LOW, HIGH = ord("#"), ord("I")  # under cutoff 20: a base the trimmer takes, a base that ends its walk


def mixed_rows(n: int, seed: int = 5) -> R.Rows:
    """n reads of every length 0..40 in turn (row i: 40, 33, 26, ... -- 7 is a unit modulo 41, a tile of 41 rows or more
    holds every length), random A/C/G/T of high quality; every third row ends in i % 5 bases of low quality, for the
    quality trimmer in front of the op to take.  Rows padded with ``N``."""
    rng = np.random.default_rng(seed)
    lens = ((40 - 7 * np.arange(n)) % 41).astype(np.uint16)
    seq = np.full((n, STRIDE), ord("N"), dtype=np.uint8)
    qual = np.full((n, STRIDE), R.PAD, dtype=np.uint8)
    cols = np.arange(STRIDE)[None, :]
    inside = cols < lens[:, None]
    seq[inside] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, STRIDE))[inside]
    i = np.arange(n)[:, None]
    low = inside & (i % 3 == 0) & (cols >= lens[:, None].astype(np.int64) - i % 5)
    qual[inside] = HIGH
    qual[low] = LOW
    return R.Rows(seq, qual, lens, 0)


def chain(f, length, front=0, back=20, nextseq=None, trim_n=False):
    """[CutOp(+f)][, NextSeqTrimOp], QTrimOp(front, back)[, ShortenOp(length)][, NTrimOp()]: the compiler's order."""
    ops = [planmod.CutOp(f)] if f else []
    if nextseq is not None:
        ops.append(planmod.NextSeqTrimOp(nextseq))
    ops.append(planmod.QTrimOp(back, 33, cutoff_front=front))
    if length is not None:
        ops.append(planmod.ShortenOp(length))
    return ops + ([planmod.NTrimOp()] if trim_n else [])


def tail_of(ops) -> S.Tail:
    return S.split_tail(ops, planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp, planmod.ShortenOp)[1]


def straddle_rows(length: int, n: int = 192, seed: int = 11) -> R.Rows:
    """Reads of 30 to 40 bases for a chain ``CutOp(+f), ..., Shorten(length), NTrimOp`` with f = 2: around the cut
    position -- |length| bases from the 5' end of the interval, or from its 3' end for a negative length -- row i has
    ``N`` on both sides of the cut (i % 4 == 0: the one inside goes to --trim-n only AFTER the cut), on the inside only
    (1), on the outside only (2: nothing more goes) or nowhere (3); every fifth row has i % 7 bases of low quality at
    its 3' end, so that the quality-trimmed end lies on either side of a negative length's cut; every sixth row holds
    three more ``N`` further inside, for --max-n to count."""
    rng = np.random.default_rng(seed)
    f, k = 2, abs(length)
    lens = (30 + np.arange(n) % 11).astype(np.uint16)
    seq = np.full((n, STRIDE), ord("N"), dtype=np.uint8)
    qual = np.full((n, STRIDE), R.PAD, dtype=np.uint8)
    for i in range(n):
        m = int(lens[i])
        seq[i, :m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=m)
        qual[i, :m] = HIGH
        q = i % 7 if i % 5 == 0 else 0
        qual[i, m - q:m] = LOW
        inside, outside = (f + k - 1, f + k) if length >= 0 else (m - q - k, m - q - k - 1)
        if i % 4 in (0, 1) and f <= inside < m:
            seq[i, inside] = ord("N")
        if i % 4 in (0, 2) and f <= outside < m:
            seq[i, outside] = ord("N")
        if i % 6 == 0:
            seq[i, 8:11] = ord("N")
    return R.Rows(seq, qual, lens, f)


def rule_ends(rows: R.Rows, ops, end=None, flags=0, min_length=0) -> E.Ends:
    """What a chain of ``chain`` leaves of rows whose interval ends at ``end`` (default: the read's end)."""
    f = ops[0].length if isinstance(ops[0], planmod.CutOp) else 0
    lens = rows.lens.astype(np.int64)
    end = lens if end is None else np.asarray(end, dtype=np.int64)
    return S.apply_tail(rows.seq, rows.qual, np.minimum(f, end), end, flags, tail_of(ops), min_length)


# ---- the rule --------------------------------------------------------------------------------------------------------

ENUM_LENGTHS = tuple(range(-14, 15)) + (S.INT32_MAX, -S.INT32_MAX, S.INT32_MIN)


def test_rule_by_hand():
    assert S.shorten(10, 3) == (0, 3) and S.shorten(10, -3) == (7, 10)
    assert S.shorten(10, 10) == S.shorten(10, 11) == S.shorten(10, -10) == S.shorten(10, -11) == (0, 10)
    assert S.shorten(10, 0) == (0, 0) and S.shorten(0, 5) == S.shorten(0, -5) == (0, 0)
    assert S.shorten(10, S.INT32_MAX) == S.shorten(10, S.INT32_MIN) == (0, 10)
    read = b"ACGTACGTAC"
    for length in ENUM_LENGTHS:
        a, b = S.shorten(len(read), length)
        assert read[a:b] == (read[:length] if length >= 0 else read[length:])


def test_the_one_read_form_and_the_row_form_agree():
    """Every n in 0..12 at every offset 0..3 in the row, every length in -14..14 and the three ends of int32."""
    ns = np.repeat(np.arange(13, dtype=np.int64), 4)
    begin = np.tile(np.arange(4, dtype=np.int64), 13)
    end = begin + ns
    for length in ENUM_LENGTHS:
        a, b = S.shortens(begin, end, length)
        assert a.dtype == np.int64 and b.dtype == np.int64
        for i in range(len(ns)):
            one = S.shorten(int(ns[i]), length)
            got = (int(a[i] - begin[i]), int(b[i] - begin[i]))
            if one == (0, 0):  # nothing left: [s, s) for a length >= 0, [e, e) for a negative one; both empty
                assert got[0] == got[1] == (0 if length >= 0 else int(ns[i])), (int(ns[i]), length)
            else:
                assert got == one, (int(ns[i]), length)
            assert got[1] - got[0] == min(int(ns[i]), abs(length))


def test_apply_and_split_tail():
    ops = chain(3, 5, 15, 10, nextseq=18, trim_n=True)
    front, tail = S.split_tail(ops, planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp, planmod.ShortenOp)
    assert front == [planmod.CutOp(3)]
    assert tail == S.Tail(5, N.Tail(18, 33, E.Tail(15, 10, 33, True)))
    assert tail_of(chain(0, None)) == S.Tail(None, N.Tail(None, 33, E.Tail(0, 20, 33, False)))
    assert tail_of([planmod.ShortenOp(-4)]) == S.Tail(-4, N.Tail())
    # without the op the tail is nextseq_rule's
    rows = mixed_rows(130)
    lens = rows.lens.astype(np.int64)
    for trim_n in (False, True):
        t = tail_of(chain(0, None, 15, 20, nextseq=20, trim_n=trim_n))
        mine = S.apply_tail(rows.seq, rows.qual, 0, lens, 0, t, MIN_LENGTH)
        theirs = N.apply_tail(rows.seq, rows.qual, 0, lens, 0, t.rest, MIN_LENGTH)
        assert all(np.array_equal(x, y) for x, y in zip(mine[:3], theirs[:3])) and mine.cut == theirs.cut > 0
    # the op sits between the quality trimmer and the N trimmer: ACGTNN|NACG.., -l 5 --trim-n leaves ACGT
    seq = np.frombuffer(b"ACGTNNNACGTT", dtype=np.uint8)[None, :].copy()
    qual = np.full((1, 12), HIGH, dtype=np.uint8)
    ends = S.apply_tail(seq, qual, 0, 12, 0, S.Tail(5, N.Tail(rest=E.Tail(0, 20, 33, True))), 5)
    assert (int(ends.start[0]), int(ends.stop[0]), int(ends.flags[0])) == (0, 4, abi.CS_F_TOO_SHORT)
    ends = S.apply_tail(seq, qual, 0, 12, 0, S.Tail(-7, N.Tail(rest=E.Tail(0, 20, 33, True))), 5)
    assert (int(ends.start[0]), int(ends.stop[0]), int(ends.flags[0])) == (7, 12, 0)  # NNACGTT -> ACGTT
    # ... and behind the quality trimmer: the last three bases are low, -l -4 keeps the four in front of them
    qual[0, 9:] = LOW
    ends = S.apply_tail(seq, qual, 0, 12, 0, S.Tail(-4, N.Tail(rest=E.Tail(0, 20, 33, False))), 0)
    assert (int(ends.start[0]), int(ends.stop[0]), ends.cut) == (5, 9, 3) and int(ends.flags[0]) == abi.CS_F_QTRIMMED


# ---- the command line ------------------------------------------------------------------------------------------------

def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


@pytest.mark.parametrize("argv, l1, l2", [
    (["-l", "30"], 30, 30),
    (["--length", "-25"], -25, -25),
    (["-l", "30", "-L", "-25"], 30, -25),
    (["-L", "12"], None, 12),
    (["-l", "0", "--trim-n"], 0, 0),
    (["-l", "30", "-L", "31", "--trim-n", "--nextseq-trim", "20", "-q", "15,10", "-Q", "25"], 30, 31),
    (["-l", str(S.INT32_MAX), "-L", str(S.INT32_MIN)], S.INT32_MAX, S.INT32_MIN),
    ([], None, None),
])
def test_cli_parses_the_options_into_args_settings_and_plans(argv, l1, l2):
    args = run.resolve_args(_args(*argv))
    assert args.length == l1 and args.length_r2 == (l2 if "-L" in argv else None)
    st = run.settings_from_args(args)
    assert (st.length, st.length_r2) == (args.length, args.length_r2)
    without = [a for a, prev in zip(argv, [""] + argv) if a not in ("-l", "--length", "-L") and prev not in ("-l", "--length", "-L")]
    plain_st = run.settings_from_args(run.resolve_args(_args(*without)))
    plain, plain_single = planmod.compile_paired(TAKARA, plain_st), planmod.compile_single(TAKARA, plain_st)
    tp, single = planmod.compile_paired(TAKARA, st), planmod.compile_single(TAKARA, st)
    trim_n = "--trim-n" in argv
    for mate, base, want in ((tp.r1, plain.r1, l1), (tp.r2, plain.r2, l2), (single.r1, plain_single.r1, l1)):
        kinds = [type(o) for o in mate.ops]
        assert kinds.count(planmod.ShortenOp) == (want is not None)
        if want is None:
            assert mate.ops == base.ops
            continue
        at = kinds.index(planmod.ShortenOp)
        assert mate.ops[at] == planmod.ShortenOp(want)
        assert isinstance(mate.ops[at - 1], planmod.QTrimOp)  # directly behind the quality trimmer ...
        assert mate.ops[at + 1:] == ([planmod.NTrimOp()] if trim_n else [])  # ... and in front of the N trimmer
        if "--nextseq-trim" in argv:
            assert isinstance(mate.ops[at - 2], planmod.NextSeqTrimOp)
        assert mate.ops[:at] + mate.ops[at + 1:] == base.ops  # nothing else changes


def test_settings_defaults():
    st = planmod.CutadaptConfig()
    assert st.length is None and st.length_r2 is None
    args = _args()
    assert args.length is None and args.length_r2 is None
    assert repr(planmod.ShortenOp(-20)) == "Shortener(length=-20)"


def test_cli_refuses_the_second_reads_length_without_a_second_read(caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "-L", "5"]))
    assert exc.value.code == 1 and "-L" in caplog.text and "two input files" in caplog.text  # logging.error, exit 1
    # one interleaved file holds a second read
    args = run.resolve_args(run.build_parser().parse_args(["-A", "TAKARAV3", "r12.fq.gz", "--interleaved", "-L", "5", "-l", "7"]))
    assert args.outputs.paired and (args.length, args.length_r2) == (7, 5)
    tp = run.compile_plan(args, TAKARA, run.settings_from_args(args))
    assert tp.paired and tp.r1.ops[-1] == planmod.ShortenOp(7) and tp.r2.ops[-1] == planmod.ShortenOp(5)


@pytest.mark.parametrize("argv", [["-l", str(2 ** 31)], ["-L", str(-2 ** 31 - 1)]])
def test_cli_refuses_a_length_beyond_32_bits(argv, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args(*argv))
    assert exc.value.code == 1 and "32 bits" in caplog.text


@pytest.mark.parametrize("bad", ["1,2", "a", "1.5", ""])
def test_cli_refuses_malformed_lengths(bad, capsys):
    for option in ("-l", "-L"):
        with pytest.raises(SystemExit) as exc:
            _args(option, bad)
        assert exc.value.code == 2 and option in capsys.readouterr().err


def test_the_single_end_chain_shortens_in_front_of_the_reverse_complement():
    st = planmod.CutadaptConfig()
    st.auto_rc, st.trim_n, st.length = True, True, 50
    tp = planmod.compile_single(planmod.BarcodeConfig("AGATCGGAAGAGC<ACACTCTTTCCC"), st)
    assert tp.reverse_complement
    steps = run.dry_run_steps(tp)
    assert steps[-3:] == ["Shortener(length=50)", "NEndTrimmer()", "ReverseComplementConverter()"]
    assert steps[-4].startswith("QualityTrimmer(")


def test_dry_run_and_help(capsys):
    def single(*extra):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", *extra])
        return capsys.readouterr().out

    strip = lambda text: [re.sub(r"^Step \d+: ", "", x) for x in text.splitlines()]
    plain = single("--trim-n")
    assert "Shortener" not in plain
    on = single("--trim-n", "-l", "30")
    lines = on.splitlines()
    at = next(i for i, line in enumerate(lines) if "Shortener" in line)
    assert lines[at] == f"Step {at + 1}: Shortener(length=30)"
    assert lines[at - 1] == f"Step {at}: QualityTrimmer(cutoff_front=0, cutoff_back=20, base=33)"
    assert lines[at + 1] == f"Step {at + 2}: NEndTrimmer()"
    del lines[at]
    assert strip("\n".join(lines)) == strip(plain)
    # paired: the steps come in pairs, -L shows in the second half
    st = run.settings_from_args(run.resolve_args(_args("-l", "30", "-L", "-25")))
    steps = run.dry_run_steps(planmod.compile_paired(TAKARA, st))
    assert steps[-1] == "(Shortener(length=30), Shortener(length=-25))"
    assert steps[:-1] == run.dry_run_steps(planmod.compile_paired(TAKARA, run.settings_from_args(run.resolve_args(_args()))))
    # -L alone: mate 1's chain is one step shorter than mate 2's, the steps cannot come in pairs to the end
    st = run.settings_from_args(run.resolve_args(_args("-L", "-25")))
    tp = planmod.compile_paired(TAKARA, st)
    assert len(tp.r2.ops) == len(tp.r1.ops) + 1 and tp.r2.ops[-1] == planmod.ShortenOp(-25)
    assert not any(isinstance(o, planmod.ShortenOp) for o in tp.r1.ops)
    steps = run.dry_run_steps(tp)
    assert steps[-1] == "(None, Shortener(length=-25))"
    assert steps[:-1] == run.dry_run_steps(planmod.compile_paired(TAKARA, run.settings_from_args(run.resolve_args(_args()))))
    text = run.build_parser().format_help()
    assert "-l LENGTH, --length LENGTH" in text and "-L LENGTH" in text


def test_readme_lists_the_options_as_built():
    readme = (ROOT / "README.md").read_text()
    assert "-l/--length" in readme and "`-L" in readme and "CS_OP_SHORTEN" in (ROOT / "INTEGRATION.md").read_text()


# ---- the plan and the C ABI ------------------------------------------------------------------------------------------

def test_pack_puts_the_op_where_the_header_says():
    arr = planmod.pack_ops(chain(3, -30, 15, 10, trim_n=True))
    assert [int(c.kind) for c in arr] == [abi.CS_OP_CUT, abi.CS_OP_QTRIM, abi.CS_OP_SHORTEN, abi.CS_OP_NTRIM]
    assert abi.CS_OP_SHORTEN == 7
    op = arr[2]
    assert (op.length, op.stat_slot) == (-30, 2)
    raw = bytearray(bytes(op))
    at = abi.cs_op.length.offset
    assert len(raw) == 284 and raw[0] == 7 and at == abi.cs_op.seq.offset == 24
    assert int.from_bytes(raw[at:at + 4], "little", signed=True) == -30
    for field, size in ((abi.cs_op.kind, 1), (abi.cs_op.length, 4), (abi.cs_op.stat_slot, 1)):
        raw[field.offset:field.offset + size] = bytes(size)
    assert bytes(raw) == bytes(284)  # kind, length, stat_slot: nothing else
    for length in (0, S.INT32_MAX, S.INT32_MIN):
        assert planmod.pack_ops([planmod.ShortenOp(length)])[0].length == length
    for length in (S.INT32_MAX + 1, S.INT32_MIN - 1):
        with pytest.raises(ValueError):
            planmod.pack_ops([planmod.ShortenOp(length)])
    # an adapter op's bases are where they were
    ad = planmod.pack_ops([planmod.back("ACGT", 0.0, 3)])[0]
    assert bytes(ad)[24:28] == b"ACGT" and bytes(ad.seq[:4]) == b"ACGT"


def test_abi_version_and_sizes_are_unchanged_and_the_header_agrees():
    assert abi.CS_ABI_VERSION == 7 and C.sizeof(abi.cs_op) == 284
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"#define CS_ABI_VERSION 7\b", header) and re.search(r"\bCS_OP_SHORTEN = 7\b", header)
    src = '''#include <stdio.h>
    #include <stddef.h>
    #include "cutseq_hip.h"
    int main(void){ cs_op op = {0}; op.length = INT32_MIN;
      printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(cs_op), offsetof(cs_op, length), offsetof(cs_op, seq), offsetof(cs_op, thr),
             offsetof(cs_op, q_cutoff_front), (int)CS_OP_SHORTEN, (int)CS_ABI_VERSION, (int)op.seq[3]); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        got = subprocess.run([f"{d}/p"], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == [284, abi.cs_op.length.offset, abi.cs_op.seq.offset, abi.cs_op.thr.offset,
                                     abi.cs_op.q_cutoff_front.offset, abi.CS_OP_SHORTEN, 7, 0x80]


# ---- the GPU test's inputs do their job (the rule alone) -------------------------------------------------------------

def test_mixed_rows_hold_every_length_and_flip_too_short_at_the_boundary():
    for n in (1, 63, 64, 65):
        rows = mixed_rows(n)
        assert len(rows.lens) == n and int(rows.lens[0]) == 40
        assert len(set(rows.lens.tolist())) == min(n, 41)
    rows = mixed_rows(65)
    assert set(rows.lens.tolist()) == set(range(41))
    short = {}
    for length in LENGTHS:
        ends = rule_ends(rows, chain(1, length), min_length=MIN_LENGTH)
        short[length] = int(((ends.flags & abi.CS_F_TOO_SHORT) != 0).sum())
        assert ends.cut > 0  # (the quality trimmer in front of the op has work)
    # TooShort flips exactly at the boundary: 19 makes every read too short, 20 does not; -20 like 20
    assert short[0] == short[1] == short[19] == 65 and short[20] == short[-20] == short[21] < 65
    assert short[40] == short[41] == short[S.INT32_MAX] == short[S.INT32_MIN] == short[-41] == short[20]
    assert short[-1] == 65


@pytest.mark.parametrize("length", [12, -12])
def test_straddle_rows_need_the_order_of_the_tail(length):
    """Applying the N trimmer in FRONT of the op, or the op in front of the quality trimmer, gives other intervals."""
    rows = straddle_rows(length)
    ops = chain(rows.f, length, 0, 20, trim_n=True)
    right = rule_ends(rows, ops)
    lens = rows.lens.astype(np.int64)
    # N trimmer first
    t = tail_of(ops)
    early = N.apply_tail(rows.seq, rows.qual, rows.f, lens, 0, t.rest, 0)
    a, b = S.shortens(early.start, early.stop, length)
    assert int(((a != right.start) | (b != right.stop)).sum()) > 20
    # op first
    a, b = S.shortens(np.full(len(lens), rows.f), lens, length)
    late = N.apply_tail(rows.seq, rows.qual, a, b, 0, t.rest, 0)
    if length < 0:
        assert int(((late.start != right.start) | (late.stop != right.stop)).sum()) > 10
    # the example of the issue: both neighbours of the cut are N, the one inside goes after the cut
    both = np.flatnonzero(np.arange(len(lens)) % 4 == 0)
    assert ((right.stop - right.start)[both] < abs(length)).all()
