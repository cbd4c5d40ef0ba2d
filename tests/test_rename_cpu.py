"""--rename on the CPU side: the rule (tests/rename_rule.py) against Python's own ``str.format`` and
``str.split(maxsplit=1)`` on every name of the universe, the product's template compiler against the rule, the command
line's refusals and dry-run text, the ranks' command lines and the C ABI's declarations."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import pytest

from cutseq_amd import abi, capi, fastq, plan as planmod, ranks, rename, run, textio
from cutseq_amd.common import BUILDIN_ADAPTERS

import names_universe as nu
import rename_rule
import util

ROOT = Path(__file__).resolve().parents[1]
TAKARAV3 = BUILDIN_ADAPTERS["TAKARAV3"]
SCHEME_UMI3_ONLY = "ACACGACGCTCTTCCGATCT>NNNNNAGATCGGAAGAGCACACGTC"  # its one capture is the SUFFIX
SCHEME_UMI5_ONLY = "ACACGACGCTCTTCCGATCTNNNN>AGATCGGAAGAGCACACGTC"
SINGLE_CAPTURES = {"cut_prefix": b"ACGT", "cut_suffix": b"TTG"}
PAIRED_CAPTURES = {"r1.cut_prefix": b"ACGTAC", "r2.cut_prefix": b"GG"}


# ---- the rule against Python --------------------------------------------------------------------------------------

def python_says(template: str, name: bytes, captures: dict, rn: int) -> bytes:
    """cutadapt's expression: ``template.format(...)`` over ``name.split(maxsplit=1)`` of the decoded name."""
    text = name.decode("latin-1")
    fields = text.split(maxsplit=1)
    rid, comment = fields if len(fields) == 2 else (text, "")
    mates = {f"r{k}": SimpleNamespace(cut_prefix=captures.get(f"r{k}.cut_prefix", b"").decode()) for k in (1, 2)}
    own = captures.get(f"r{rn}.cut_prefix", captures.get("cut_prefix", b"")).decode()
    return template.replace("\\t", "\t").format(header=text, id=rid, comment=comment, rn=rn, cut_prefix=own,
                                                cut_suffix=captures.get("cut_suffix", b"").decode(), **mates).encode("latin-1")


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_the_rule_is_pythons_format_and_split_on_every_name(paired):
    names = [nu.as_read(n) for n in nu.u1() + nu.u2()]
    assert len(names) == 22_409
    templates = rename_rule.PAIRED_TEMPLATES if paired else rename_rule.SINGLE_TEMPLATES
    captures = PAIRED_CAPTURES if paired else SINGLE_CAPTURES
    for template in templates:
        pieces = rename_rule.compile_rule(template, paired)
        for rn in (1, 2) if paired else (1,):
            for name in names:
                got = rename_rule.render(pieces, name, captures, rn)
                if got != python_says(template, name, captures, rn):
                    pytest.fail(f"{template!r} on {name!r} (rn {rn}): {got!r} != {python_says(template, name, captures, rn)!r}")


def test_the_rule_on_comments():
    pieces = rename_rule.compile_rule("{id}|{comment}|{header}", False)
    assert rename_rule.render(pieces, b"r1 1:N:0:ACGT", {}) == b"r1|1:N:0:ACGT|r1 1:N:0:ACGT"
    assert rename_rule.render(pieces, b"r1 \t a b  ", {}) == b"r1|a b  |r1 \t a b  "  # leading blank run gone, trailing kept
    assert rename_rule.render(pieces, b"  r1  ", {}) == b"  r1  ||  r1  "              # one field: the id is the name
    assert rename_rule.render(pieces, b"", {}) == b"||"
    assert rename_rule.render(rename_rule.compile_rule("{comment}", False), b"lonely", {}) == b""  # '@\n' is legal


# ---- the product's compiler against the rule ----------------------------------------------------------------------

def _plan(scheme, paired):
    return util.compile_plan(scheme, planmod.CutadaptConfig(), paired)


def render_segments(compiled, name: bytes, cap, rn: int) -> bytes:
    """What the device makes of ``cs_text_set_rename``'s table, in Python: ``cap[(mate, kind)]`` are the captures as the
    kernels hold them -- (0 | 1, CS_RENAME_CAPTURE | CS_RENAME_CAPTURE2)."""
    rid, comment = rename_rule.split_name(name)
    out = b""
    for kind, mate, off, length in compiled.segments:
        if kind == abi.CS_RENAME_LITERAL:
            out += compiled.literals[off:off + length]
        elif kind in (abi.CS_RENAME_CAPTURE, abi.CS_RENAME_CAPTURE2):
            out += cap.get((rn - 1 if mate == abi.CS_RENAME_OWN else mate, kind), b"")
        else:
            out += {abi.CS_RENAME_HEADER: name, abi.CS_RENAME_ID: rid, abi.CS_RENAME_COMMENT: comment,
                    abi.CS_RENAME_MATE: str(rn).encode()}[kind]
    return out


@pytest.mark.parametrize("scheme, paired, device_captures, captures", [
    # single end: the device's first / second capture are the chain's first / second capturing cut
    (nu.SCHEME_TWO_UMIS, False, {(0, abi.CS_RENAME_CAPTURE): b"ACGT", (0, abi.CS_RENAME_CAPTURE2): b"TTG"}, SINGLE_CAPTURES),
    (SCHEME_UMI3_ONLY, False, {(0, abi.CS_RENAME_CAPTURE): b"TTGCA"}, {"cut_suffix": b"TTGCA"}),
    (SCHEME_UMI5_ONLY, False, {(0, abi.CS_RENAME_CAPTURE): b"ACGT"}, {"cut_prefix": b"ACGT"}),
    (nu.SCHEME_NO_UMI, False, {}, {}),
    (nu.SCHEME_TWO_UMIS, True, {(0, abi.CS_RENAME_CAPTURE): b"ACGTAC", (1, abi.CS_RENAME_CAPTURE): b"GG"}, PAIRED_CAPTURES),
    (TAKARAV3, True, {(1, abi.CS_RENAME_CAPTURE): b"GGTTACGT"}, {"r2.cut_prefix": b"GGTTACGT"}),  # (a 3' UMI only: mate 2 starts with it)
    (SCHEME_UMI5_ONLY, True, {(0, abi.CS_RENAME_CAPTURE): b"ACGT"}, {"r1.cut_prefix": b"ACGT"}),
    (nu.SCHEME_NO_UMI, True, {}, {}),
], ids=["two-umis", "umi3-only", "umi5-only", "no-umi", "two-umis-paired", "takarav3-paired", "umi5-only-paired", "no-umi-paired"])
def test_the_compiled_table_renders_what_the_rule_renders(scheme, paired, device_captures, captures):
    tp = _plan(scheme, paired)
    names = [b"", b"id", b"id c", b" id  c d ", b"a\tb\x1cc ", b"   "]
    for template in rename_rule.PAIRED_TEMPLATES if paired else rename_rule.SINGLE_TEMPLATES:
        compiled = rename.compile_template(template, tp)
        assert compiled.template == template and len(compiled.segments) <= abi.CS_RENAME_MAX_SEGMENTS
        assert len(compiled.literals) <= abi.CS_RENAME_MAX_LITERAL
        pieces = rename_rule.compile_rule(template, paired)
        for rn in (1, 2) if paired else (1,):
            for name in names:
                assert render_segments(compiled, name, device_captures, rn) == rename_rule.render(pieces, name, captures, rn), \
                    (template, name, rn)


def test_a_scheme_with_a_3_prime_umi_only_captures_its_suffix_first():
    tp = _plan(SCHEME_UMI3_ONLY, False)
    assert [op.capture for op in tp.r1.ops if isinstance(op, planmod.CutOp) and op.capture] == [1]
    assert rename.compile_template("{id}:{cut_suffix}", tp).segments[-1] == (abi.CS_RENAME_CAPTURE, 0, 0, 0)
    assert rename.compile_template("{cut_prefix}", tp).segments == ()  # no such cut: empty
    both = rename.compile_template("{cut_suffix}-{cut_prefix}", _plan(nu.SCHEME_TWO_UMIS, False))
    assert [s[0] for s in both.segments] == [abi.CS_RENAME_CAPTURE2, abi.CS_RENAME_LITERAL, abi.CS_RENAME_CAPTURE]


def test_the_defaults_are_the_references_templates():
    assert rename.default_template(False, False) == rename.default_template(False, True) == "{id}"
    assert rename.default_template(True, False) == "{id}_{cut_prefix}{cut_suffix}"
    assert rename.default_template(True, True) == "{id}_{r1.cut_prefix}{r2.cut_prefix}"


# ---- refusals -----------------------------------------------------------------------------------------------------

REFUSED_BY_BOTH = [
    ("{id", "a lone '{' at position 1"),
    ("x}y", "a lone '}' at position 2"),
    ("{id}}", "a lone '}' at position 5"),
    ("{i{d}", "a lone '{' at position 1"),
    ("{}", "{} is an empty or positional field"),
    ("{0}", "{0} is an empty or positional field"),
    ("{id:>5}", "{id:>5} carries a conversion or a format spec"),
    ("{id!r}", "{id!r} carries a conversion or a format spec"),
    ("{name}", "unknown variable {name}"),
    ("{id[0]}", "{id[0]} is not a variable"),
    ("{r3.cut_prefix}", "unknown variable {r3.cut_prefix}"),
    ("a\rb", "the byte '\\r' at position 2 is not printable ASCII or a TAB"),
    ("a\nb", "the byte '\\n' at position 2 is not printable ASCII or a TAB"),
    ("café", "the byte 'é' at position 4 is not printable ASCII or a TAB"),
    ("\x7f", "is not printable ASCII or a TAB"),
    ("{adapter_name}", "{adapter_name} is not available: a cutseq chain has several AdapterCutters"),
    ("{match_sequence}", "{match_sequence} is not available: a cutseq chain has several AdapterCutters"),
    ("{rc}", "{rc} is not available"),
    ("{r1.adapter_name}", "{r1.adapter_name} is not available"),
    ("{r2.match_sequence}", "{r2.match_sequence} is not available"),
    ("{r2.rc}", "{r2.rc} is not available"),
    ("{id}" * 5, "copies from the header 5 times"),
    ("{header}{id}{comment}{id}{header}", "copies from the header 5 times"),
    ("x" * 256, "256 literal bytes, 255 at most"),
    ("x" * 250 + "\\t" * 6, "256 literal bytes, 255 at most"),
    ("{cut_prefix}-" * 8 + "{cut_prefix}", "17 segments"),
]
SINGLE_ONLY_REFUSALS = [
    ("{rn}", "{rn} is the number of a mate: a single-end run has none"),
    ("{r1.cut_prefix}", "unknown variable {r1.cut_prefix} (a single-end run has: header, id, comment, cut_prefix, cut_suffix)"),
]
PAIRED_ONLY_REFUSALS = [
    ("{cut_suffix}", "{cut_suffix} is not available in a paired run: its chains cut the 3' bases in front of the Renamer"),
    ("{r1.cut_suffix}", "{r1.cut_suffix} is not available in a paired run"),
    ("{r2.cut_suffix}", "{r2.cut_suffix} is not available in a paired run"),
]


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("template, message", REFUSED_BY_BOTH)
def test_refused_templates(template, message, paired):
    with pytest.raises(ValueError) as exc:
        rename.check(template, paired)
    assert message in str(exc.value) and str(exc.value).startswith("--rename: ")
    with pytest.raises(ValueError):
        rename_rule.compile_rule(template, paired)


def test_paired_refusals_differ_from_single_end_ones():
    for template, message in SINGLE_ONLY_REFUSALS:
        with pytest.raises(ValueError) as exc:
            rename.check(template, False)
        assert message in str(exc.value)
        with pytest.raises(ValueError):
            rename_rule.compile_rule(template, False)
        assert rename.check(template, True) and rename_rule.compile_rule(template, True)
    for template, message in PAIRED_ONLY_REFUSALS:
        with pytest.raises(ValueError) as exc:
            rename.check(template, True)
        assert message in str(exc.value)
        with pytest.raises(ValueError):
            rename_rule.compile_rule(template, True)
    assert rename.check("{cut_suffix}", False) and rename_rule.compile_rule("{cut_suffix}", False)
    for bad in ("{r1.cut_suffix}", "{r2.cut_suffix}"):  # single end: no such names at all
        with pytest.raises(ValueError, match="unknown variable"):
            rename.check(bad, False)


def test_what_is_accepted_at_the_limits():
    for paired, templates in ((False, rename_rule.SINGLE_TEMPLATES), (True, rename_rule.PAIRED_TEMPLATES)):
        for template in templates:
            assert [(k, v.encode() if k == "literal" else v) for k, v in rename.check(template, paired)] == \
                rename_rule.compile_rule(template, paired), template
    assert len(rename.check("{cut_prefix}-" * 8, False)) == 16
    assert rename.check("x" * 249 + "\\t" * 6, False) == [("literal", "x" * 249 + "\t" * 6)]
    assert rename.check("{{}}{{{id}}}\t", False) == [("literal", "{}{"), ("variable", "id"), ("literal", "}\t")]
    assert rename.check("", True) == []


# ---- the command line -----------------------------------------------------------------------------------------------

def _args(*extra, inputs=("in.fq.gz",), preset="TAKARAV3"):
    return run.build_parser().parse_args(["-A", preset, *inputs, *extra])


def _fails(args, caplog):
    with pytest.raises(SystemExit) as exc:
        run.resolve_args(args)
    assert exc.value.code == 1
    return caplog.text


def test_the_option_reaches_the_plan_and_the_text_worker():
    template = "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}"
    args = run.resolve_args(_args("--rename", template, inputs=("a_R1.fq.gz", "a_R2.fq.gz")))
    tp = run.compile_plan(args, planmod.BarcodeConfig(TAKARAV3), run.settings_from_args(args))
    assert tp.rename == template
    options = textio.text_options(args.outputs, tp, fasta=False, gpu_deflate=True)
    worker = textio.TextWorker(tp, 0, 1024, options)
    assert worker.rename == rename.compile_template(template, tp)
    # (TAKARAV3 has a 3' UMI only: mate 2's chain captures, {r1.cut_prefix} renders empty and takes no segment)
    assert worker.rename.segments == ((abi.CS_RENAME_ID, 0, 0, 0), (abi.CS_RENAME_LITERAL, 0, 0, 6), (abi.CS_RENAME_CAPTURE, 1, 0, 0))
    assert worker.rename.literals == b" RX:Z:"
    # without the option: no template, the engine is created as before
    args = run.resolve_args(_args(inputs=("a_R1.fq.gz", "a_R2.fq.gz")))
    tp = run.compile_plan(args, planmod.BarcodeConfig(TAKARAV3), run.settings_from_args(args))
    options = textio.text_options(args.outputs, tp, fasta=False, gpu_deflate=True)
    assert tp.rename is None and textio.TextWorker(tp, 0, 1024, options).rename is None


@pytest.mark.parametrize("extra, inputs, message", [
    (["--rename", "{rn}"], ("in.fq",), "--rename: {rn} is the number of a mate"),
    (["--rename", "{cut_suffix}"], ("r1.fq", "r2.fq"), "--rename: {cut_suffix} is not available in a paired run"),
    (["--rename", "{cut_suffix}", "--interleaved"], ("in.fq",), "--rename: {cut_suffix} is not available in a paired run"),
    (["--rename", "{id:>5}"], ("in.fq",), "--rename: {id:>5} carries a conversion or a format spec"),
    (["--rename", "{id} {match_sequence}"], ("in.fq",), "{match_sequence} is not available"),
    (["--rename", "{id}", "--demux-barcodes", "codes.tsv"], ("in.fq",), "--rename cannot be combined with --demux-barcodes"),
])
def test_cli_refuses(extra, inputs, message, caplog):
    assert message in _fails(_args(*extra, inputs=inputs), caplog)


def test_paired_variables_pass_where_the_run_is_paired():
    for extra, inputs in ((["--rename", "{id}/{rn}"], ("r1.fq", "r2.fq")), (["--rename", "{rn}", "--interleaved"], ("in.fq",)),
                          (["--rename", "{cut_suffix}"], ("in.fq",))):
        assert run.resolve_args(_args(*extra, inputs=inputs)).rename == extra[1]


def test_the_record_path_is_refused(monkeypatch, caplog):
    monkeypatch.setenv("CUTSEQ_TEXT_PATH", "0")
    assert "--rename needs the text path" in _fails(_args("--rename", "{id}"), caplog)
    assert C.sizeof(fastq._FormatParams) == 56  # the record path's formatter is not extended


def _dry_run_steps(*extra, inputs, preset="TAKARAV3"):
    args = run.resolve_args(_args(*extra, inputs=inputs, preset=preset))
    scheme = BUILDIN_ADAPTERS[preset]
    tp = run.compile_plan(args, planmod.BarcodeConfig(scheme), run.settings_from_args(args))
    return tp, run.dry_run_steps(tp)


@pytest.mark.parametrize("inputs, word, default", [
    (("in.fq",), "Renamer", "{id}_{cut_prefix}{cut_suffix}"),
    (("r1.fq", "r2.fq"), "PairedEndRenamer", "{id}_{r1.cut_prefix}{r2.cut_prefix}"),
])
def test_dry_run_text(inputs, word, default):
    tp, plain = _dry_run_steps(inputs=inputs)
    at = len(tp.r1.name_suffixes) + tp.r1.rename_at
    assert plain[at] == f"{word}({default!r})"
    _, same = _dry_run_steps("--rename", default, inputs=inputs)
    assert same == plain
    template = "{id} RX:Z:{cut_prefix}\\t{comment}"
    _, custom = _dry_run_steps("--rename", template, inputs=inputs)
    assert custom[at] == f"{word}({template!r})" and custom[:at] + custom[at + 1:] == plain[:at] + plain[at + 1:]


def test_dry_run_prints_the_step(capsys):
    run.main(["-A", "TAKARAV3", "in.fq", "-n", "--rename", "{header}"])
    assert "Renamer('{header}')" in capsys.readouterr().out


# ---- the ranks ------------------------------------------------------------------------------------------------------

def test_the_ranks_children_get_the_option():
    template = "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}\\t{comment}"
    argv = ["-A", "TAKARAV3", "a_R1.fq.gz", "a_R2.fq.gz", "--ranks", "4", "-t", "16", "--rename", template]
    child = ranks.child_argv(argv, 4)
    assert "--ranks" not in child and child[-2:] == ["-t", "4"]
    assert child[child.index("--rename") + 1] == template
    args = run.resolve_args(run.build_parser().parse_args(child + ["--rank-spec", "spec.json"]))
    assert args.rename == template and args.ranks == 1
    assert ranks.child_argv(["--rename=" + template, "--ranks=2", "x.fq"], 1) == ["--rename=" + template, "x.fq", "-t", "1"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------

def test_abi_sizes_and_version_are_unchanged_and_the_symbol_is_declared():
    assert C.sizeof(abi.cs_text_params) == 48 and C.sizeof(abi.cs_text_result) == 176 and abi.CS_ABI_VERSION == 7
    assert C.sizeof(abi.cs_rename_seg) == 4
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    assert re.search(r"#define CS_ABI_VERSION 7\b", header)
    assert re.search(r"\bint cs_text_set_rename\(cs_text \*t, const cs_rename_seg \*segments, uint32_t n, const char \*literals, "
                     r"uint32_t n_bytes\);", header)
    assert "cs_text_set_rename" in capi.EXPORTS
    for name, value in (("SEGMENTS", abi.CS_RENAME_MAX_SEGMENTS), ("LITERAL", abi.CS_RENAME_MAX_LITERAL),
                        ("HEADER", abi.CS_RENAME_MAX_HEADER)):
        assert re.search(rf"#define CS_RENAME_MAX_{name} {value}\b", header)
    kinds = re.search(r"enum \{ (CS_RENAME_LITERAL = 0,.*?) \};", header, re.S).group(1)
    for item in kinds.replace("\n", " ").split(","):
        name, value = item.split("=")
        assert getattr(abi, name.strip()) == int(value)
    assert abi.CS_RENAME_OWN == 2 and "enum { CS_RENAME_OWN = 2 };" in header


def test_the_library_exports_the_symbol():
    from cutseq_amd import build
    build.build()
    assert hasattr(capi.load(), "cs_text_set_rename")
    assert capi.load().cs_abi_version() == 7
