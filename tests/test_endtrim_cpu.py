"""-q FRONT,BACK (the quality trimmer's 5' cutoff) and --trim-n (NEndTrimmer) on the CPU side: the command line, the plan
and the C ABI, the rules of tests/endtrim_rule.py against oracle.pyref and a regular expression, and the inputs of
tests/test_gpu_endtrim.py -- which are built here -- held to what that test needs of them, by the rules alone."""
import ctypes as C
import functools
import itertools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from oracle import pyref
from cutseq_amd import abi, plan as planmod, run
from cutseq_amd.common import BUILDIN_ADAPTERS

import endtrim_rule as E
import qtrim_rule as R
import universe as U

ROOT = Path(__file__).resolve().parents[1]
TAKARA = planmod.BarcodeConfig(BUILDIN_ADAPTERS["TAKARAV3"])

# ---- inputs and plans, shared with the GPU tests ---------------------------------------------------------------------

FB = ((20, 20), (20, 0), (2, 20), (41, 20), (0, 20))  # (cutoff_front, cutoff_back) of the scan-kernel case
N_ALPHABET = "ACNn"
N_STRIDE = 12
LOW, HIGH = ord("#"), ord("I")  # under cutoff 20: a base the trimmer takes, a base that ends its walk


def chain(f, front, back, base=33, trim_n=False):
    ops = ([planmod.CutOp(f)] if f else []) + [planmod.QTrimOp(back, base, cutoff_front=front)]
    return ops + ([planmod.NTrimOp()] if trim_n else [])


def n_rows(f: int) -> R.Rows:
    """Every string over A, C, N, n of length 0..8 behind f bytes of ``N`` (for a ``CutOp(+f)`` to remove), the strings
    without an ``n`` first, rows padded with ``N``: whole tiles of the first part hold nothing but A, C and N (the scan
    kernel's fast re-coding stands), every tile of the second part holds an ``n`` (it falls back to the exact form).
    Row i has i % 3 bases of low quality at its 5' end and i // 3 % 3 at its 3' end: a quality trimmer in front of the
    N trimmer uncovers bases that were not at an end."""
    body, ln = U.reads_universe(N_ALPHABET, 8, stride=8)
    has_n = (body == ord("n")).any(axis=1)
    order = np.concatenate([np.flatnonzero(~has_n), np.flatnonzero(has_n)])
    body, ln = body[order], ln[order].astype(np.int64)
    n = len(ln)
    seq = np.full((n, N_STRIDE), ord("N"), dtype=np.uint8)
    qual = np.full((n, N_STRIDE), R.PAD, dtype=np.uint8)
    cols = np.arange(8)[None, :]
    inside = cols < ln[:, None]
    seq[:, f:f + 8][inside] = body[inside]
    i = np.arange(n)
    low = (cols < (i % 3)[:, None]) | (cols >= (ln - i // 3 % 3)[:, None])
    qual[:, f:f + 8][inside] = np.where(low, LOW, HIGH)[inside]
    return R.Rows(seq, qual, (ln + f).astype(np.uint16), f)


@functools.lru_cache(maxsize=3)
def family(name: str) -> R.Rows:
    kind, _, arg = name.partition(":")
    if kind == "E1":  # F1 and its mirror image, stride 16
        return E.both(R.f1(int(arg)))
    if kind == "E2":  # F2 product B, mirrored: a window at every depth from the 5' end, stride 152
        return E.mirror(R.f2("B", int(arg)))
    if kind == "E6":  # full rows of one byte, stride 1536
        return R.f6_long()
    if kind == "EN":
        return n_rows(int(arg))
    raise KeyError(name)


def scan_cases():
    """-> [(family, [(mate 1 (f, front, back), mate 2 (f, front, back)), ...])]: paired plans whose mates run different
    chains over the same rows."""
    cases = []
    for f in range(4):
        cases.append((f"E1:{f}", [((f, *FB[i]), ((f + 1 + i) % 4, *FB[(i + 1) % len(FB)])) for i in range(len(FB))]))
    return cases


def deep_cases():
    cuts = R.F6_CUTOFFS
    pairs = [((0, cuts[i], 20), (0, cuts[(i + 4) % len(cuts)], 20)) for i in range(len(cuts))]
    cases = [(f"E2:{f}", [((f, 20, 20), ((f + 1) % 4, 20, 0)), ((f, 21, 20), ((f + 2) % 4, 19, 21))]) for f in range(4)]
    cases.append(("E2:1", [((1, a[1], 20), (2, b[1], 20)) for a, b in pairs]))
    cases.append(("E6", pairs))
    return cases


SCAN_CASES, DEEP_CASES = scan_cases(), deep_cases()


def rule_ends(rows: R.Rows, setting, trim_n=False, end=None, flags=0, min_length=0) -> E.Ends:
    """What ``[CutOp(+f), QTrimOp(front, back)[, NTrimOp()]]`` leaves of rows whose interval ends at ``end``."""
    f, front, back = setting[:3]
    lens = rows.lens.astype(np.int64)
    end = lens if end is None else np.asarray(end, dtype=np.int64)
    begin = np.minimum(f, end)
    return E.apply_tail(rows.seq, rows.qual, begin, end, flags, E.Tail(front, back, 33, trim_n), min_length)


def records(ends: E.Ends) -> np.ndarray:
    want = np.zeros(len(ends.start), dtype=abi.RESULT_DTYPE)
    want["start"], want["stop"], want["flags"] = ends.start, ends.stop, ends.flags
    return want


# ---- the command line ------------------------------------------------------------------------------------------------

def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


@pytest.mark.parametrize("argv, front, back, trim_n", [
    (["-q", "15,10"], 15, 10, False), (["-q", "10"], 0, 10, False), (["-q", "0,0"], 0, 0, False),
    (["--trim-n"], 0, 20, True), (["--min-quality", "3,4", "--trim-n"], 3, 4, True), ([], 0, 20, False),
])
def test_cli_parses_the_options_into_args_settings_and_plans(argv, front, back, trim_n):
    args = run.resolve_args(_args(*argv))
    assert args.min_quality == back and isinstance(args.min_quality, int)
    assert args.min_quality_front == front and args.trim_n is trim_n
    st = run.settings_from_args(args)
    assert (st.min_quality, st.min_quality_front, st.trim_n) == (back, front, trim_n)
    for tp in (planmod.compile_paired(TAKARA, st), planmod.compile_single(TAKARA, st)):
        for mate in (tp.r1, tp.r2) if tp.paired else (tp.r1,):
            tail = mate.ops[-2:] if trim_n else mate.ops[-1:]
            assert tail[0] == planmod.QTrimOp(back, 33, cutoff_front=front)
            assert sum(isinstance(o, planmod.QTrimOp) for o in mate.ops) == 1
            assert [isinstance(o, planmod.NTrimOp) for o in mate.ops] == [False] * (len(mate.ops) - 1) + [trim_n]


def test_settings_defaults():
    st = planmod.CutadaptConfig()
    assert st.min_quality_front == 0 and st.trim_n is False


@pytest.mark.parametrize("bad", ["1,2,3", "a,b", "abc", "1,", ",2", "1.5,2"])
def test_cli_refuses_malformed_cutoffs(bad, capsys):
    with pytest.raises(SystemExit) as exc:
        _args("-q", bad)
    assert exc.value.code == 2  # an argparse usage error, as for -q abc before
    assert "-q/--min-quality" in capsys.readouterr().err


def test_the_single_end_chain_puts_the_n_trimmer_in_front_of_the_reverse_complement():
    st = planmod.CutadaptConfig()
    st.auto_rc, st.trim_n = True, True
    tp = planmod.compile_single(planmod.BarcodeConfig("AGATCGGAAGAGC<ACACTCTTTCCC"), st)
    assert tp.reverse_complement
    steps = run.dry_run_steps(tp)
    assert steps[-2:] == ["NEndTrimmer()", "ReverseComplementConverter()"] and steps[-3].startswith("QualityTrimmer(")


def test_dry_run_and_help(capsys):
    def single(*extra):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", *extra])
        return capsys.readouterr().out

    plain = single()
    assert "QualityTrimmer(cutoff_front=0, cutoff_back=20, base=33)" in plain and "NEndTrimmer" not in plain
    assert single("-q", "20") == plain
    both = single("-q", "15,10", "--trim-n")
    assert "cutoff_front=15" in both and "NEndTrimmer()" in both
    # the options change the trimmer's step and add one behind it, nothing else
    lines = both.splitlines()
    at = next(i for i, line in enumerate(lines) if "NEndTrimmer()" in line)
    assert lines[at] == f"Step {at + 1}: NEndTrimmer()" and "QualityTrimmer(cutoff_front=15, cutoff_back=10, base=33)" in lines[at - 1]
    del lines[at]
    lines[at - 1] = lines[at - 1].replace("cutoff_front=15, cutoff_back=10", "cutoff_front=0, cutoff_back=20")
    assert lines == plain.splitlines()
    # paired: the steps come in pairs
    st = run.settings_from_args(run.resolve_args(_args("-q", "15,10", "--trim-n")))
    steps = run.dry_run_steps(planmod.compile_paired(TAKARA, st))
    assert steps[-1] == "(NEndTrimmer(), NEndTrimmer())"
    assert steps[-2] == "(" + ", ".join(["QualityTrimmer(cutoff_front=15, cutoff_back=10, base=33)"] * 2) + ")"
    assert steps[:-2] == run.dry_run_steps(planmod.compile_paired(TAKARA, run.settings_from_args(run.resolve_args(_args()))))[:-1]
    text = run.build_parser().format_help()
    assert "--trim-n" in text and "5'CUTOFF,]3'CUTOFF" in text


# ---- the plan and the C ABI ------------------------------------------------------------------------------------------

def test_pack_puts_the_front_cutoff_and_the_new_kind_where_the_header_says():
    arr = planmod.pack_ops(chain(3, 15, 10, trim_n=True))
    assert [int(c.kind) for c in arr] == [abi.CS_OP_CUT, abi.CS_OP_QTRIM, abi.CS_OP_NTRIM] and abi.CS_OP_NTRIM == 5
    q = arr[1]
    assert (q.q_cutoff, q.q_cutoff_front, q.q_base) == (10, 15, 33)
    raw = bytes(q)
    assert len(raw) == 284 and int.from_bytes(raw[282:284], "little", signed=True) == 15 and raw[0] == abi.CS_OP_QTRIM
    assert bytes(arr[2]) == bytes([5]) + bytes(10) + bytes([2]) + bytes(272)  # kind, stat_slot, nothing else
    # the reference's op is what it was: every byte behind thr[] zero
    assert bytes(planmod.pack_ops([planmod.QTrimOp(20)])[0])[281:] == bytes(3)
    assert planmod.pack_ops([planmod.QTrimOp(20, cutoff_front=-40000)])[0].q_cutoff_front == -0x8000
    assert planmod.pack_ops([planmod.QTrimOp(20, cutoff_front=40000)])[0].q_cutoff_front == 0x7FFF


def test_abi_version_and_sizes_are_unchanged_and_the_header_agrees():
    assert abi.CS_ABI_VERSION == 7
    assert C.sizeof(abi.cs_op) == 284 and C.sizeof(abi.cs_params) == 32 and C.sizeof(abi.cs_stats) == 8 * (8 + abi.CS_MAX_OPS + 1)
    assert C.sizeof(abi.cs_text_params) == 48 and C.sizeof(abi.cs_text_result) == 176
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"#define CS_ABI_VERSION 7\b", header) and re.search(r"\bCS_OP_NTRIM = 5\b", header)
    src = '''#include <stdio.h>
    #include <stddef.h>
    #include "cutseq_hip.h"
    int main(void){ printf("%zu %zu %zu %zu %d\\n", sizeof(cs_op), offsetof(cs_op, q_cutoff_front), offsetof(cs_op, thr),
                           offsetof(cs_op, q_cutoff), (int)CS_OP_NTRIM); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        got = subprocess.run([f"{d}/p"], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == [C.sizeof(abi.cs_op), abi.cs_op.q_cutoff_front.offset, abi.cs_op.thr.offset,
                                     abi.cs_op.q_cutoff.offset, abi.CS_OP_NTRIM]
    assert abi.cs_op.q_cutoff_front.offset == 282


# ---- the rules -------------------------------------------------------------------------------------------------------

def test_rules_by_hand():
    assert E.start(b"", 20) == 0 and E.start(b"IIII", 20) == 0 and E.start(b"##II", 20) == 2 and E.start(b"####", 20) == 4
    assert E.start(b"#I#I", 20) == 1                      # '#' adds 18, 'I' takes 20: 18, -2
    low, high = R.qbyte(+1), R.qbyte(-1)
    q = bytes([low, high, low, low])                      # the issue's example: the two walks cross
    assert E.start(q, 20) == 4 and R.stop(q, 20) == 2 and E.qtrim(q, 20, 20) == (0, 0)
    assert E.start(q[:2], 20) == 1                        # a front walk held to [0, stop) would keep base 1
    assert E.qtrim(b"#II#", 20, 20) == (1, 3) and E.qtrim(b"#II#", 0, 20) == (0, 3) and E.qtrim(b"#II#", 20, 0) == (1, 4)
    assert E.ntrim(b"") == (0, 0) and E.ntrim(b"NNN") == (0, 0) and E.ntrim(b"NNANN") == (2, 3) and E.ntrim(b"ANNA") == (0, 4)
    assert E.ntrim(b"nNAn") == (0, 4) and E.ntrim(b"NnAnN") == (1, 4)


@pytest.mark.parametrize("alphabet", R.ALPHABETS)
def test_rule_equals_pyref_on_every_string(alphabet):
    """Every string over three deltas up to length 10, every (F, B) of {0, 2, 20, 41} x {0, 20} at base 33: the plain
    loops and the vectorised rule against oracle.pyref.quality_trim_index."""
    body, ln = R.strings([R.qbyte(d) for d in alphabet], 10)
    texts = [body[i, :int(ln[i])].tobytes() for i in range(len(ln))]
    latin = [t.decode("latin-1") for t in texts]
    assert len(texts) == 88573
    for front, back in itertools.product((0, 2, 20, 41), (0, 20)):
        a, b = E.qtrims(body, 0, ln, front, back)
        for i, t in enumerate(texts):
            want = pyref.quality_trim_index(latin[i], front, back)
            assert (int(a[i]), int(b[i])) == want, (t, front, back)
            if i % 16 == 0 or len(t) <= 6:
                assert E.qtrim(t, front, back) == want, (t, front, back)


def test_rule_equals_pyref_at_base_64():
    body, ln = R.strings([R.qbyte(d, 20, 64) for d in R.ALPHABETS[0]], 10)
    a, b = E.qtrims(body, 0, ln, 20, 20, 64)
    for i in range(len(ln)):
        t = body[i, :int(ln[i])].tobytes()
        want = pyref.quality_trim_index(t.decode("latin-1"), 20, 20, 64)
        assert (int(a[i]), int(b[i])) == want == E.qtrim(t, 20, 20, 64), t


def test_vectorised_rule_equals_the_loops_inside_rows():
    """Intervals that start at every offset and end before the row does."""
    rows = family("E1:3")
    pick = np.arange(0, len(rows.lens), 97)
    lens = rows.lens[pick].astype(np.int64)
    for f, front, back in ((0, 20, 20), (1, 20, 0), (2, 21, 19), (5, 19, 20)):
        begin = np.minimum(f, lens)
        end = np.maximum(begin, lens - (pick % 3))
        a, b = E.qtrims(rows.qual[pick], begin, end, front, back)
        na, nb = E.ntrims(rows.qual[pick], begin, end)  # (any bytes do for the N rule: here byte 0x4E is a quality)
        for k, i in enumerate(pick):
            s, e = int(begin[k]), int(end[k])
            x, y = E.qtrim(rows.qual[i, s:e].tobytes(), front, back)
            assert (int(a[k]), int(b[k])) == (s + x, s + y), (int(i), f, front, back)
            x, y = E.ntrim(rows.qual[i, s:e].tobytes())
            assert (int(na[k]), int(nb[k])) == (s + x, s + y)


def test_a_zero_front_cutoff_never_trims():
    """start = 0 for EVERY byte string once F + base <= 0, and for F = 0 over bytes >= base -- the product does not run
    the front walk at all for F = 0, which differs from the rule only on bytes below the base, where the reference's
    op (cutoff_front = 0 as cutseq installs it) is what the parent computed."""
    for front, base in ((-33, 33), (-40, 33), (-64, 64), (0, 0), (-32768, 33)):
        for L in range(6):
            for t in itertools.product((0, 1, 33, 34, 64, 255), repeat=L):
                assert E.start(bytes(t), front, base) == 0
    for L in range(6):
        for t in itertools.product((33, 34, 40, 126, 255), repeat=L):
            assert E.start(bytes(t), 0, 33) == 0
    assert E.start(bytes([32, 40]), 0, 33) == 1  # (a byte below the base: the rule trims it; the op with F = 0 does not look)
    assert R.clamp(0, 33) == 0 and R.clamp(0, 255) == 0 and R.clamp(0, 0) == 0  # the clamp leaves "no front walk" alone


def test_clamped_front_cutoff_changes_no_result():
    texts = [bytes(t) for L in range(4) for t in itertools.product((0, 33, 34, 53, 126, 255), repeat=L)]
    for q in texts:
        for cutoff in R.F6_CUTOFFS + (0, 20):
            assert E.start(q, cutoff) == E.start(q, R.clamp(cutoff)), (q, cutoff)


def test_n_rule_equals_the_regular_expressions():
    body, ln = U.reads_universe("ANn", 9, stride=12)
    a, b = E.ntrims(body, 0, ln)
    assert len(ln) == 29524
    for i in range(len(ln)):
        t = body[i, :int(ln[i])].tobytes().decode()
        m = re.match(r"^N+", t)
        rest = t[m.end():] if m else t
        m = re.search(r"N+$", rest)
        rest = rest[:m.start()] if m else rest
        x, y = E.ntrim(t.encode())
        assert t[x:y] == rest and (int(a[i]), int(b[i])) == (x, y), t


def test_mirror():
    rows = R.f1(3)
    m = E.mirror(rows)
    for i in (0, 1, 5, 100, 88572):
        k = int(rows.lens[i])
        assert m.qual[i, 3:k].tobytes() == rows.qual[i, 3:k].tobytes()[::-1] and m.qual[i, :3].tobytes() == b"!!!"
        assert m.qual[i, k:].tobytes() == rows.qual[i, k:].tobytes()
    lens = rows.lens.astype(np.int64)
    back = R.stops(rows.qual, 3, lens, 20)
    assert np.array_equal(E.fronts(m.qual, 3, lens, 20).start, (lens - 3) - back)


# ---- the GPU test's inputs do their job (the rules alone) ------------------------------------------------------------

def test_scan_inputs_collapse_and_start_at_every_offset():
    offsets, crossed = set(), 0
    for name, plans in SCAN_CASES:
        rows = family(name)
        lens = rows.lens.astype(np.int64)
        for pair in plans:
            for f, front, back in pair:
                begin = np.minimum(f, lens)
                a = E.fronts(rows.qual, begin, lens, front).start
                b = R.stops(rows.qual, begin, lens, back)
                crossed += int(((0 < b) & (b < a)).sum())
                offsets |= set((begin[lens > begin] & 3).tolist())
                if (front, back) == (20, 20) and f == rows.f:
                    assert ((0 < b) & (b < a)).any() and ((a > 0) & (a < b) & (b < lens - begin)).any()
    assert offsets == {0, 1, 2, 3} and crossed > 1000


def test_front_walks_cross_one_two_and_many_dwords():
    spans = set()
    for name, plans in SCAN_CASES[:1] + DEEP_CASES:
        rows = family(name)
        lens = rows.lens.astype(np.int64)
        for pair in plans[:2]:
            for f, front, _back in pair:
                begin = np.minimum(f, lens)
                w = E.fronts(rows.qual, begin, lens, R.clamp(front))
                live = lens > begin
                spans |= set(((w.last[live] >> 2) - (begin[live] >> 2) + 1).tolist())
    assert {1, 2, 3, 4} <= spans and any(16 < s <= 38 for s in spans) and 384 in spans  # (1 536 bases: 384 dwords)


def test_n_inputs():
    for f in range(4):
        rows = family(f"EN:{f}")
        assert len(rows.lens) == 87381 and rows.seq.shape[1] == N_STRIDE
        lens = rows.lens.astype(np.int64)
        plain = ~(rows.seq == ord("n")).any(axis=1)
        assert plain[:9841].all() and not plain[9841:].any() and 9841 // 64 > 100   # whole tiles without an n, then none
        assert set(np.unique(rows.seq[:9841]).tolist()) == {ord("A"), ord("C"), ord("N")}
        every_tile = (rows.seq[9856:9856 + 64 * ((87381 - 9856) // 64)] == ord("n")).reshape(-1, 64 * N_STRIDE).any(axis=1)
        assert every_tile.all()
        begin = np.minimum(f, lens)
        a0, b0 = E.ntrims(rows.seq, begin, lens)                       # the N rule alone
        q = E.apply_tail(rows.seq, rows.qual, begin, lens, 0, E.Tail(20, 20))
        both = E.apply_tail(rows.seq, rows.qual, begin, lens, 0, E.Tail(20, 20, 33, True))
        n = lens - begin
        assert ((n > 0) & (a0 == b0)).any()                            # N runs that cover the whole interval
        first, last = rows.seq[np.arange(len(n)), np.minimum(begin, N_STRIDE - 1)], rows.seq[np.arange(len(n)), np.maximum(lens - 1, 0)]
        assert ((n > 1) & (first == ord("n")) & (a0 == begin)).any() and ((n > 1) & (last == ord("n")) & (b0 == lens)).any()
        # an N run that the quality trimmer uncovered: no N at that end of the read, an N trimmed there all the same
        left = (q.stop > q.start) & (both.start > q.start) & (first != ord("N")) & (n > 0)
        right = (q.stop > q.start) & (both.stop < q.stop) & (last != ord("N")) & (n > 0)
        assert left.sum() > 100 and right.sum() > 100
        assert ((q.stop > q.start) & (both.stop == both.start)).any()  # ... and one that was all that was left
