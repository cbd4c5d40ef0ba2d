"""--poly-a (CS_OP_POLYA, cutadapt's PolyATrimmer) without a GPU: the rule of tests/polya_rule.py held to itself in its
three statements (the loops, the closed-form facts, numpy over rows) and to a model of the kernels' walk on ENUMERATED
reads; the plan compiler, the op table, ``cs_plan_create``, the command line and the report.

``layered`` is what tests/test_gpu_polya.py expects of a chain: the C oracle does not know the op, so the oracle runs
the ops in front of it, the rule applies the op, and ``shorten_rule.apply_tail`` the trimmers behind it.
"""
import ctypes as C
import dataclasses
import gzip
import json
import logging
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, report, run
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig

import polya_rule as A
import shorten_rule as S

ROOT = Path(__file__).resolve().parents[1]
TAKARA = BUILDIN_ADAPTERS["TAKARAV3"]          # a '-' library ("...XXX<XXXXXXNNNNNNNN...")
TAKARA_PLUS = TAKARA.replace("<", ">")         # the same parts on the other strand
NO_STRAND = "AGATCGGAAGAGC-ACACTCTTTCCC"


# ---- the layered expectation -----------------------------------------------------------------------------------------

class Layer(NamedTuple):
    start: np.ndarray
    stop: np.ndarray
    flags: np.ndarray
    cut: int       # what the quality trimmers took (cs_stats.qualtrim_bp)
    polya_bp: int  # what the PolyATrimOp took (cs_polya_bp_fetch)
    raw: np.ndarray  # the oracle's records of the ops in front (captures), None without such ops


def split(ops):
    """A chain's ops -> (the ops in front of its PolyATrimOp, that op, shorten_rule's Tail of what follows)."""
    at = [i for i, o in enumerate(ops) if isinstance(o, planmod.PolyATrimOp)]
    assert len(at) == 1, ops
    rest, tail = S.split_tail(ops[at[0] + 1:], planmod.QTrimOp, planmod.NTrimOp, planmod.NextSeqTrimOp, planmod.ShortenOp)
    assert rest == []  # (the op stands directly in front of the trimmers)
    return list(ops[:at[0]]), ops[at[0]], tail


def layered(tp, mates, threads=4):
    """``mates``: (seq, qual, lens) per mate -> a Layer per mate."""
    import oracle
    out = []
    for mate, (seq, qual, lens) in zip((tp.r1, tp.r2), mates):
        front, op, tail = split(mate.ops)
        n = len(lens)
        begin, end = np.zeros(n, dtype=np.int64), lens.astype(np.int64)
        flags, raw = np.zeros(n, dtype=np.int64), None
        if front:
            base = dataclasses.replace(tp, r1=dataclasses.replace(mate, ops=front), r2=None)
            raw = oracle.trim_mate(planmod.pack_ops(front), len(front), base.params(), seq, qual, lens, threads=threads)[0]
            begin, end, flags = raw["start"].astype(np.int64), raw["stop"].astype(np.int64), raw["flags"].astype(np.int64)
        start, stop = A.rows_keep(seq, begin, end, op.revcomp)
        ends = S.apply_tail(seq, qual, start, stop, flags, tail, tp.min_length)
        out.append(Layer(ends.start, ends.stop, ends.flags, ends.cut, A.trimmed(begin, end, start, stop), raw))
    return out


def records(layer: Layer) -> np.ndarray:
    want = np.zeros(len(layer.start), dtype=abi.RESULT_DTYPE)
    want["start"], want["stop"], want["flags"] = layer.start, layer.stop, layer.flags
    if layer.raw is not None:
        want["cap_off"], want["cap_len"] = layer.raw["cap_off"], layer.raw["cap_len"]
    return want


# ---- the rule --------------------------------------------------------------------------------------------------------

def test_rule_by_hand():
    assert A.keep(b"ACGTAAAAAAAAAA", False) == (0, 4)
    assert A.keep(b"ACGTAA", False) == (0, 6)                   # a tail of 2 stays
    assert A.keep(b"ACGTAAA", False) == (0, 4)
    assert A.keep(b"ACGTAAAC", False) == (0, 8)                 # one foreign LAST base in front of 3 A: 1 error in 4 is too many
    assert A.keep(b"ACGTAAAAC", False) == (0, 4)                # ... in front of 4 A: errors * 5 <= 5, the tail goes with it
    assert A.keep(b"ACGAAAAAAAAAC", False) == (0, 3)
    assert A.keep(b"ACGTAAAACAAAAA", False) == (0, 4)           # the rate holds at length 10 (1 error), the score goes on
    assert A.keep(b"CCCCaaaaaaaa", False) == (0, 12)            # lower case is an error
    assert A.keep(b"AAAAAAAA", False) == (0, 0)
    assert A.keep(b"", False) == (0, 0) and A.keep(b"", True) == (0, 0)
    assert A.keep(b"TTTTTTTTTTACGT", True) == (10, 14)
    assert A.keep(b"TTACGT", True) == (0, 6) and A.keep(b"TTTACGT", True) == (3, 7)
    assert A.keep(b"TTTTTTTT", True) == (8, 8)
    assert A.keep(b"AAAAAAAA", True) == (0, 8) and A.keep(b"TTTTTTTT", False) == (0, 8)


@pytest.mark.parametrize("head", [False, True], ids=["tail", "head"])
@pytest.mark.parametrize("name", ["E", "M"])
def test_the_three_statements_agree_on_the_enumerated_reads(name, head):
    """Universe E (32 767 reads) and M (9 841): the loops, the closed-form facts and the numpy form over rows give one
    answer for every read; the head form is the tail form of the mirrored, translated read."""
    reads = A.universe_e(head) if name == "E" else A.universe_m(head)
    assert len(reads) == (32767 if name == "E" else 9841)
    want = [A.keep(r, head) for r in reads]
    assert want == [A.by_facts(r, head) for r in reads]
    rows = A.rows_of(reads, stride=16)
    start, stop = A.rows_keep(rows.seq, 0, rows.lens, head)
    assert list(zip(start.tolist(), stop.tolist())) == want
    if head:  # the mirror image
        back = bytes.maketrans(b"TGtg", b"ACac")
        for r, (a, b) in zip(reads[::37], want[::37]):
            assert A.keep(r[::-1].translate(back), False) == (0, len(r) - a)
    changed = sum(1 for r, w in zip(reads, want) if w != (0, len(r)))
    assert 0 < changed < len(reads)
    assert A.trimmed(0, rows.lens, start, stop) == sum(len(r) - (b - a) for r, (a, b) in zip(reads, want)) > 0


@pytest.mark.parametrize("head", [False, True], ids=["tail", "head"])
@pytest.mark.parametrize("lower_every", [0, 5])
def test_the_numpy_form_holds_on_the_homopolymer_universe(head, lower_every):
    """Universe H, every 11th read of 201 036 (the loops are slow): the rows of tests/poly_rule.py cross the dword, 32-,
    64- and 128-base boundaries and walk the 0.2 boundary with a foreign base every p positions at every phase."""
    rows = A.universe_h(head, lower_every=lower_every)
    assert len(rows.lens) == 201036
    start, stop = A.rows_keep(rows.seq, 0, rows.lens, head)
    for i in range(lower_every, len(rows.lens), 11):
        read = rows.seq[i, :rows.lens[i]].tobytes()
        assert A.keep(read, head) == (int(start[i]), int(stop[i])), read
    took = rows.lens.astype(np.int64) - (stop - start)
    assert (took >= 128).any() and ((took > 0) & (took < 8)).any() and (took == 0).any()
    if lower_every:  # lower-case letters in the runs: errors, so less goes than from the plain rows
        plain = A.universe_h(head)
        s0, e0 = A.rows_keep(plain.seq, 0, plain.lens, head)
        assert int(took.sum()) < A.trimmed(0, plain.lens, s0, e0)


# ---- the kernels' walk as a model ------------------------------------------------------------------------------------

@pytest.mark.parametrize("head", [False, True], ids=["tail", "head"])
def test_the_model_of_the_walk_equals_the_loops(head):
    """Rounds of 64 bases aligned to the row's dwords, (score, position) keys and the two early exits: the same answer
    as the loops on E and M at every dword offset of the interval's start, and on long reads of the shapes the GPU test
    uses.  On random bases the walk is settled by its first round."""
    for reads in (A.universe_e(head), A.universe_m(head)):
        for k, r in enumerate(reads):
            assert tuple(A.model(r, head, s=k % 8)[:2]) == A.keep(r, head), (r, k % 8)
    base, other = (b"T", b"G") if head else (b"A", b"C")
    rng = np.random.default_rng(5)
    for n in (150, 1537, 4099):
        shapes = [base * n, bytes(other[0] if i % 5 == 4 else base[0] for i in range(n)),
                  bytes(other[0] if i % 4 == 3 else base[0] for i in range(n)), other + base * (n - 1),
                  bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))]
        for shape in shapes:
            read = shape if head else shape[::-1]
            for s in (0, 3):
                got = A.model(read, head, s=s)
                assert tuple(got[:2]) == A.keep(read, head), (n, read[:20])
        assert got.bases <= (64 if n == 150 else 0.4 * n)  # the random read: about 0.27 n bases, one round for 150
    assert A.model(base * 1537, head).bases == 1537  # a tail is walked to its end


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_the_enumerated_reads_expose_every_planted_defect(defect):
    """A walk with `<` for `<=` in the rate test, a minimum of 2, the last maximum, or 'a' as a match gives another
    answer than the loops on some read of E or M, for the tail and for the head."""
    for head in (False, True):
        hits = {}
        for name, reads in (("E", A.universe_e(head)), ("M", A.universe_m(head))):
            hits[name] = sum(1 for r in reads[:6000] if tuple(A.model(r, head, defect=defect)[:2]) != A.keep(r, head))
        assert sum(hits.values()) > 0, (defect, head)
        if defect == "lower_case_match":
            assert hits["M"] > 0 and hits["E"] == 0  # (only M holds lower-case letters)
        else:
            assert hits["E"] > 0


# ---- the plan --------------------------------------------------------------------------------------------------------

def settings(**flags):
    st = planmod.CutadaptConfig()
    for key, value in flags.items():
        setattr(st, key, value)
    return st


def poly_ops(chain):
    return [o for o in chain.ops if isinstance(o, planmod.PolyATrimOp)]


@pytest.mark.parametrize("scheme,r1,r2", [(TAKARA_PLUS, False, True), (TAKARA, True, False), (NO_STRAND, False, True)],
                         ids=["plus", "minus", "no-strand"])
def test_placement_and_direction(scheme, r1, r2, caplog):
    """Step 7: behind the masks, in front of NextSeqTrimOp / QTrimOp / ShortenOp / NTrimOp.  '+': read 1 tail, read 2 head;
    '-': the other way round; no strand: cutadapt's own pair, and a logging.info line that says so."""
    st = settings(poly_a=True, nextseq_trim=20, min_quality=10, min_quality_front=15, length=100, trim_n=True)
    bc = BarcodeConfig(scheme)
    with caplog.at_level(logging.INFO):
        paired = planmod.compile_paired(bc, st)
        single = planmod.compile_single(bc, st)
    assert ("--poly-a" in caplog.text and "No strand" in caplog.text) == (bc.strand is None)
    assert poly_ops(paired.r1) == [planmod.PolyATrimOp(r1)] and poly_ops(paired.r2) == [planmod.PolyATrimOp(r2)]
    assert poly_ops(single.r1) == [planmod.PolyATrimOp(r1)] and single.r2 is None
    assert paired.has_poly_a and single.has_poly_a
    for chain in (paired.r1, paired.r2, single.r1):
        front, op, tail = split(chain.ops)
        assert all(isinstance(o, (planmod.AdapterOp, planmod.CutOp)) for o in front)
        assert tail == S.Tail(100, S.N.Tail(20, 33, S.E.Tail(15, 10, 33, True)))
        assert [type(o) for o in chain.ops[len(front) + 1:]] == [planmod.NextSeqTrimOp, planmod.QTrimOp, planmod.ShortenOp, planmod.NTrimOp]
    # the plan without the option is the plan it was: the op is the only difference
    off = planmod.compile_paired(bc, settings(nextseq_trim=20, min_quality=10, min_quality_front=15, length=100, trim_n=True))
    assert not off.has_poly_a
    for on_chain, off_chain in ((paired.r1, off.r1), (paired.r2, off.r2)):
        assert [o for o in on_chain.ops if not isinstance(o, planmod.PolyATrimOp)] == off_chain.ops
    # --trim-polyA-wo-direction has no bearing on the option
    wo = planmod.compile_paired(bc, settings(poly_a=True, trim_polyA_wo_direction=True))
    assert poly_ops(wo.r1) == [planmod.PolyATrimOp(r1)] and poly_ops(wo.r2) == [planmod.PolyATrimOp(r2)]
    assert not any(isinstance(o, planmod.AdapterOp) and o.match_flag == abi.CS_F_POLY for o in wo.r1.ops + wo.r2.ops)


def test_two_poly_a_trimmers_at_one_step_are_refused():
    with pytest.raises(ValueError, match="--trim-polyA"):
        planmod.compile_paired(BarcodeConfig(TAKARA), settings(poly_a=True, trim_polyA=True))
    with pytest.raises(ValueError, match="--trim-polyA"):
        planmod.compile_single(BarcodeConfig(TAKARA), settings(poly_a=True, trim_polyA=True))


def test_settings_defaults():
    assert planmod.CutadaptConfig().poly_a is False
    assert not planmod.compile_paired(BarcodeConfig(TAKARA), planmod.CutadaptConfig()).has_poly_a
    assert repr(planmod.PolyATrimOp()) == "PolyATrimmer(revcomp=False)" and repr(planmod.PolyATrimOp(True)) == "PolyATrimmer(revcomp=True)"


# ---- the op table and the C ABI --------------------------------------------------------------------------------------

def test_pack_puts_the_op_where_the_header_says():
    arr = planmod.pack_ops([planmod.CutOp(3), planmod.PolyATrimOp(), planmod.PolyATrimOp(True), planmod.QTrimOp(20)])
    assert [int(c.kind) for c in arr] == [abi.CS_OP_CUT, abi.CS_OP_POLYA, abi.CS_OP_POLYA, abi.CS_OP_QTRIM]
    assert abi.CS_OP_POLYA == 8 and (arr[1].reversed, arr[2].reversed) == (0, 1)
    raw = bytearray(bytes(arr[2]))
    for field in (abi.cs_op.kind, abi.cs_op.reversed, abi.cs_op.stat_slot):
        raw[field.offset] = 0
    assert bytes(raw) == bytes(284)  # kind, reversed, stat_slot: nothing else


def test_abi_version_and_sizes_are_unchanged_and_the_header_agrees():
    assert abi.CS_ABI_VERSION == 7 and C.sizeof(abi.cs_op) == 284 and C.sizeof(abi.cs_params) == 32
    assert C.sizeof(abi.cs_text_result) == 176 and C.sizeof(abi.cs_stats) == 8 * (8 + abi.CS_MAX_OPS + 1)
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"#define CS_ABI_VERSION 7\b", header) and re.search(r"\bCS_OP_POLYA = 8\b", header)
    assert "int cs_polya_bp_fetch(cs_engine *eng, uint64_t bp[2], int reset);" in header
    assert "cs_polya_bp_fetch" in capi.EXPORTS


def create(ops):
    lib = capi.load()
    arr, params, handle = planmod.pack_ops(ops), planmod.TrimPlan(planmod.MateChain(list(ops)), None, False, 0, False).params(), C.c_void_p()
    rc = lib.cs_plan_create(C.cast(arr, C.c_void_p), len(ops), None, 0, C.byref(params), C.byref(handle))
    if rc == 0:
        lib.cs_plan_destroy(handle)
    return rc, arr


def test_cs_plan_create_takes_the_op():
    """Host data only: no GPU is touched.  Both forms are accepted, any other value of `reversed` is refused."""
    lib = capi.load()
    assert hasattr(lib, "cs_polya_bp_fetch")
    assert create([planmod.PolyATrimOp()])[0] == 0 and create([planmod.CutOp(2), planmod.PolyATrimOp(True), planmod.QTrimOp(20)])[0] == 0
    arr = planmod.pack_ops([planmod.PolyATrimOp(True)])
    arr[0].reversed = 2
    params, handle = planmod.TrimPlan(planmod.MateChain([]), None, False, 0, False).params(), C.c_void_p()
    assert lib.cs_plan_create(C.cast(arr, C.c_void_p), 1, None, 0, C.byref(params), C.byref(handle)) == abi.CS_ERR_ARG
    assert b"poly-A" in lib.cs_last_error()
    arr[0].kind = 9  # the next kind does not exist
    assert lib.cs_plan_create(C.cast(arr, C.c_void_p), 1, None, 0, C.byref(params), C.byref(handle)) == abi.CS_ERR_ARG
    assert lib.cs_polya_bp_fetch(None, None, 0) == abi.CS_ERR_ARG


# ---- the command line and the report ---------------------------------------------------------------------------------

def _args(*extra):
    return run.build_parser().parse_args(["-A", "TAKARAV3", "r1.fq.gz", "r2.fq.gz", *extra])


def test_cli_parses_the_option_into_args_settings_and_plans():
    args = run.resolve_args(_args("--poly-a"))
    st = run.settings_from_args(args)
    assert args.poly_a is True and st.poly_a is True and st.trim_polyA is False
    tp = run.compile_plan(args, BarcodeConfig(TAKARA), st)
    assert poly_ops(tp.r1) == [planmod.PolyATrimOp(True)] and poly_ops(tp.r2) == [planmod.PolyATrimOp(False)]  # ('-')
    off = run.resolve_args(_args())
    assert off.poly_a is False and not run.compile_plan(off, BarcodeConfig(TAKARA), run.settings_from_args(off)).has_poly_a
    text = run.build_parser().format_help()
    assert " ".join(text[text.index("  --poly-a"):].split()[1:4]) == "Extension (cutadapt's option,"


def test_cli_refuses_the_option_next_to_trim_polya(caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(_args("--poly-a", "--trim-polyA"))
    assert exc.value.code == 1 and "--poly-a" in caplog.text and "--trim-polyA" in caplog.text
    run.resolve_args(_args("--poly-a", "--trim-polyA-wo-direction"))  # (no bearing on the option: not refused)


def test_dry_run_prints_the_modifier_at_its_place(capsys):
    def single(*extra):
        run.main(["-A", "TAKARAV3", "--dry-run", "r1.fq.gz", *extra])
        return capsys.readouterr().out.splitlines()

    plain = single("--nextseq-trim", "20")
    assert not any("PolyATrimmer" in line for line in plain)
    lines = single("--nextseq-trim", "20", "--poly-a")
    at = next(i for i, line in enumerate(lines) if "PolyATrimmer" in line)
    assert lines[at] == f"Step {at + 1}: PolyATrimmer(revcomp=True)"  # (TAKARAV3 is a '-' library: read 1 loses a head)
    assert lines[at + 1] == f"Step {at + 2}: NextseqQualityTrimmer(cutoff=20, base=33)"
    assert lines[at - 1].startswith(f"Step {at}: UnconditionalCutter(")  # the mask
    del lines[at]
    strip = lambda text: [re.sub(r"^Step \d+: ", "", x) for x in text]
    assert strip(lines) == strip(plain)
    steps = run.dry_run_steps(planmod.compile_paired(BarcodeConfig(TAKARA_PLUS), settings(poly_a=True)))
    assert "(PolyATrimmer(revcomp=False), PolyATrimmer(revcomp=True))" in steps
    steps = run.dry_run_steps(planmod.compile_paired(BarcodeConfig(TAKARA), settings(poly_a=True)))
    assert "(PolyATrimmer(revcomp=True), PolyATrimmer(revcomp=False))" in steps


def totals_of(paired, poly_a_bp=None):
    stats = [{"qualtrim_bp": 5, "op_matched": [0] * abi.CS_MAX_OPS}, {"qualtrim_bp": 7, "op_matched": [0] * abi.CS_MAX_OPS}]
    totals = report.new_totals()
    totals.update(in_pairs=10, routes=[8, 2, 0], in_bp=[100, 90 if paired else 0], out_bp=[80, 70 if paired else 0],
                  written_bp=[60, 50 if paired else 0], stats=[stats], devices=[0], seconds=1.0, threads=1)
    if poly_a_bp is not None:
        totals["poly_a_bp"] = poly_a_bp
    return totals


def report_of(tp, totals):
    bc = BarcodeConfig(TAKARA)
    return report.json_report(tp, totals, bc, "a", "b" if tp.paired else None, "c", None, None, None, None, None)


def test_report_keys_on_and_off():
    bc = BarcodeConfig(TAKARA)
    keys = ("poly_a_trimmed", "poly_a_trimmed_read1", "poly_a_trimmed_read2")
    on = planmod.compile_paired(bc, settings(poly_a=True))
    got = report_of(on, totals_of(True, [11, 22]))["basepair_counts"]
    assert [got[k] for k in keys] == [33, 11, 22]
    single = planmod.compile_single(bc, settings(poly_a=True))
    got = report_of(single, totals_of(False, [11, 0]))["basepair_counts"]
    assert [got[k] for k in keys] == [11, 11, None]
    off = planmod.compile_paired(bc, settings(trim_polyA=True))
    rep = report_of(off, totals_of(True))
    assert [rep["basepair_counts"][k] for k in keys] == [None, None, None]
    assert list(rep["basepair_counts"]) == list(report_of(on, totals_of(True, [1, 2]))["basepair_counts"])  # same keys, same order
    # the stderr line has no column for the counter
    assert report.minimal_report(on, totals_of(True, [11, 22])) == report.minimal_report(off, totals_of(True))


def test_ranks_sum_the_counter():
    """--ranks: every rank's totals file carries its counter, merge_totals adds them; a run without the option writes
    and merges no such key."""
    from cutseq_amd import ranks
    import tempfile
    into = report.new_totals()
    for part in ([3, 4], [10, 20]):
        with tempfile.NamedTemporaryFile("r+", suffix=".json") as fh:
            ranks.dump_totals({"totals_file": fh.name}, totals_of(True, part))
            report.merge_totals(into, json.load(open(fh.name)))
    assert into["poly_a_bp"] == [13, 24]
    with tempfile.NamedTemporaryFile("r+", suffix=".json") as fh:
        ranks.dump_totals({"totals_file": fh.name}, totals_of(True))
        part = json.load(open(fh.name))
    assert "poly_a_bp" not in part
    plain = report.new_totals()
    report.merge_totals(plain, part)
    assert "poly_a_bp" not in plain


def test_docs_name_the_option_as_built():
    readme = (ROOT / "README.md").read_text()
    assert "--poly-a" in readme and "profiles/poly_a_ab.log" in readme
    assert "CS_OP_POLYA" in (ROOT / "INTEGRATION.md").read_text() and "cs_polya_bp_fetch" in (ROOT / "INTEGRATION.md").read_text()
    design = (ROOT / "DESIGN.md").read_text()
    assert "PolyATrimmer" in design and "poly_a_trim_index" in design


# ---- pinned against cutadapt, where the fixture exists -----------------------------------------------------------------

PINS = sorted((ROOT / "tests" / "golden").glob("polya_cutadapt_*.json.gz"))


@pytest.mark.skipif(not PINS, reason="no tests/golden/polya_cutadapt_*.json.gz: run tools/pin_against_cutadapt.py where cutadapt is installed")
def test_the_rule_is_cutadapts():
    for path in PINS:
        with gzip.open(path, "rt") as fh:
            fixture = json.load(fh)
        rule = next(c for c in fixture["cases"] if c["kind"] == "poly_a")
        assert rule["reads"] == 2 * (32767 + 9841) and rule["differ"] == [], rule["differ"][:3]
