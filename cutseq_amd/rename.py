"""cutadapt's ``--rename TEMPLATE``: the template language and its compiler for the device.

Every chain holds a ``Renamer`` / ``PairedEndRenamer`` (cutseq/run.py:377-380, 642-645); the option replaces its
template.  The rule (recalled): ``{name}`` is a placeholder, ``{{`` and ``}}`` are braces, the
two characters ``\\t`` a TAB, everything else literal.  :func:`parse` refuses what the language does not have and
:func:`check` what a cutseq chain cannot supply, both with ``ValueError``; :func:`compile_template` turns the pieces
into the segments ``cs_text_set_rename`` takes (``include/cutseq_hip.h``).
"""
from __future__ import annotations

import re
from typing import List, NamedTuple, Tuple

from . import abi

MAX_SEGMENTS = abi.CS_RENAME_MAX_SEGMENTS
MAX_LITERAL = abi.CS_RENAME_MAX_LITERAL
MAX_HEADER = abi.CS_RENAME_MAX_HEADER

HEADER_VARIABLES = ("header", "id", "comment")
SINGLE_VARIABLES = HEADER_VARIABLES + ("cut_prefix", "cut_suffix")
PAIRED_VARIABLES = HEADER_VARIABLES + ("rn", "cut_prefix", "r1.cut_prefix", "r2.cut_prefix")
_MATCH_VARIABLES = ("adapter_name", "match_sequence", "rc")
_NAME = re.compile(r"[A-Za-z_][A-Za-z_0-9]*(\.[A-Za-z_][A-Za-z_0-9]*)*\Z")

Piece = Tuple[str, str]  # ("literal", text) or ("variable", name)


def default_template(has_umi: bool, paired: bool) -> str:
    """What the reference installs (cutseq/run.py:377-380, 642-645)."""
    if not has_umi:
        return "{id}"
    return "{id}_{r1.cut_prefix}{r2.cut_prefix}" if paired else "{id}_{cut_prefix}{cut_suffix}"


def parse(template: str) -> List[Piece]:
    """The template as literal and variable pieces, neighbouring literals joined.  Language errors only."""
    pieces: List[Piece] = []

    def literal(text: str):
        if pieces and pieces[-1][0] == "literal":
            pieces[-1] = ("literal", pieces[-1][1] + text)
        else:
            pieces.append(("literal", text))

    i, n = 0, len(template)
    while i < n:
        c = template[i]
        if template.startswith("{{", i) or template.startswith("}}", i):
            literal(c)
            i += 2
        elif c == "}":
            raise ValueError(f"--rename: a lone '}}' at position {i + 1} of {template!r} (write '}}}}' for a brace)")
        elif c == "{":
            end = template.find("}", i)
            if end < 0 or "{" in template[i + 1:end]:
                raise ValueError(f"--rename: a lone '{{' at position {i + 1} of {template!r} (write '{{{{' for a brace)")
            field = template[i + 1:end]
            shown = "{" + field + "}"
            if field == "" or field.isdigit():
                raise ValueError(f"--rename: {shown} is an empty or positional field: a placeholder names its variable")
            if "!" in field or ":" in field:
                raise ValueError(f"--rename: {shown} carries a conversion or a format spec: a placeholder is a bare name")
            if not _NAME.match(field):
                raise ValueError(f"--rename: {shown} is not a variable")
            pieces.append(("variable", field))
            i = end + 1
        elif template.startswith("\\t", i):
            literal("\t")
            i += 2
        else:
            if c != "\t" and not " " <= c <= "~":
                raise ValueError(f"--rename: the byte {c!r} at position {i + 1} is not printable ASCII or a TAB: "
                                 "a record name is one line of text")
            literal(c)
            i += 1
    return pieces


def check(template: str, paired: bool) -> List[Piece]:
    """:func:`parse`, then the variables a single-end / paired run has and the limits of the device's table."""
    pieces = parse(template)
    known = PAIRED_VARIABLES if paired else SINGLE_VARIABLES
    for kind, name in pieces:
        if kind != "variable" or name in known:
            continue
        shown = "{" + name + "}"
        bare = name.split(".", 1)[1] if name.startswith(("r1.", "r2.")) else name
        if bare in _MATCH_VARIABLES:
            raise ValueError(f"--rename: {shown} is not available: a cutseq chain has several AdapterCutters, and the "
                             "engine records no single match to name")
        if paired and bare == "cut_suffix":
            raise ValueError(f"--rename: {shown} is not available in a paired run: its chains cut the 3' bases in front "
                             "of the Renamer without capturing them")
        if not paired and name == "rn":
            raise ValueError(f"--rename: {shown} is the number of a mate: a single-end run has none (cutadapt's Renamer "
                             "does not know it either)")
        raise ValueError(f"--rename: unknown variable {shown} (a {'paired' if paired else 'single-end'} run has: "
                         f"{', '.join(known)})")
    if len(pieces) > MAX_SEGMENTS:
        raise ValueError(f"--rename: the template has {len(pieces)} segments (literal stretches and placeholders), "
                         f"{MAX_SEGMENTS} at most")
    literal = sum(len(text) for kind, text in pieces if kind == "literal")
    if literal > MAX_LITERAL:
        raise ValueError(f"--rename: the template has {literal} literal bytes, {MAX_LITERAL} at most")
    headers = sum(1 for kind, name in pieces if kind == "variable" and name in HEADER_VARIABLES)
    if headers > MAX_HEADER:
        raise ValueError(f"--rename: the template copies from the header {headers} times ({{header}}, {{id}}, "
                         f"{{comment}} together), {MAX_HEADER} at most")
    return pieces


class Compiled(NamedTuple):
    """``cs_text_set_rename``'s arguments: ``segments`` = ((kind, mate, literal offset, literal length), ...)."""
    template: str
    segments: Tuple[Tuple[int, int, int, int], ...]
    literals: bytes


def capture_slots(plan) -> dict:
    """{variable: (segment kind, mate)} for the captures the plan's chains make; a variable whose cut the scheme does not
    have renders empty and has no entry.  Single end: ``{cut_prefix}`` is the positive capturing CutOp, ``{cut_suffix}``
    the negative one -- the FIRST capture of a scheme with a 3' UMI only.  Paired: each chain captures its 5' cut."""
    from .plan import CutOp
    kinds = {1: abi.CS_RENAME_CAPTURE, 2: abi.CS_RENAME_CAPTURE2}
    slots = {}
    if not plan.paired:
        for op in plan.r1.ops:
            if isinstance(op, CutOp) and op.capture:
                slots["cut_prefix" if op.length > 0 else "cut_suffix"] = (kinds[op.capture], 0)
        return slots
    for mate, chain in enumerate((plan.r1, plan.r2)):
        if any(isinstance(op, CutOp) and op.capture == 1 and op.length > 0 for op in chain.ops):
            slots[f"r{mate + 1}.cut_prefix"] = (abi.CS_RENAME_CAPTURE, mate)
    if slots:  # (the written mate's own: empty for the mate whose chain captures nothing)
        slots["cut_prefix"] = (abi.CS_RENAME_CAPTURE, abi.CS_RENAME_OWN)
    return slots


def compile_template(template: str, plan) -> Compiled:
    pieces = check(template, plan.paired)
    slots = capture_slots(plan)
    fixed = {"header": abi.CS_RENAME_HEADER, "id": abi.CS_RENAME_ID, "comment": abi.CS_RENAME_COMMENT, "rn": abi.CS_RENAME_MATE}
    segments, literals = [], b""
    for kind, text in pieces:
        if kind == "literal":
            data = text.encode("ascii")
            segments.append((abi.CS_RENAME_LITERAL, 0, len(literals), len(data)))
            literals += data
        elif text in fixed:
            segments.append((fixed[text], 0, 0, 0))
        elif text in slots:
            segments.append((*slots[text], 0, 0))
    return Compiled(template, tuple(segments), literals)
