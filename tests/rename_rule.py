"""cutadapt's ``--rename`` as a readable rule (test infrastructure): the template language with its refusals, and a
renderer over (name bytes, captures, rn).  The product's twin is ``cutseq_amd/rename.py`` plus ``name_len`` / ``emit_name``
of text_kernels.hip.inc; ``tests/test_rename_cpu.py`` holds this rule to Python's own ``str.format`` and
``str.split(maxsplit=1)``, ``tests/test_gpu_rename.py`` the kernels to this rule.

Reference surface: ``Renamer`` / ``PairedEndRenamer`` (cutseq/run.py:377-380, 642-645) with another template.

  template    ``{name}`` placeholder, ``{{`` ``}}`` braces, backslash-t a TAB, the rest literal bytes
  {header}    the name as the Renamer gets it (behind the SuffixRemover chain)
  {id} {comment}   ``name.split(maxsplit=1)``: two fields -> the first, and the rest without its leading blanks; else the
              whole name and nothing
  single end  {cut_prefix} {cut_suffix}: what the positive / the negative capturing cut took
  paired      {rn} 1 or 2; {r1.cut_prefix} {r2.cut_prefix}; {cut_prefix} the written mate's own
"""
from __future__ import annotations

import re
from typing import Dict, List, Tuple

from names_universe import BLANKS

MAX_SEGMENTS, MAX_LITERAL, MAX_HEADER = 16, 255, 4
HEADER = ("header", "id", "comment")
SINGLE = HEADER + ("cut_prefix", "cut_suffix")
PAIRED = HEADER + ("rn", "cut_prefix", "r1.cut_prefix", "r2.cut_prefix")
_TOKEN = re.compile(r"\{\{|\}\}|\\t|\{[^{}]*\}|[^{}]", re.S)

# every template the tests render, by run kind; the defaults first
SINGLE_TEMPLATES = [
    "{id}", "{id}_{cut_prefix}{cut_suffix}", "{header}", "{comment}", "{id} {comment}", "{cut_suffix}-{cut_prefix}",
    "{id}:{cut_suffix}", "{{{id}}}\\t{comment}", "x" * 255, "{header}{id}{comment}{header}", "", "{id} RX:Z:{cut_prefix}{cut_suffix}",
]
PAIRED_TEMPLATES = [
    "{id}", "{id}_{r1.cut_prefix}{r2.cut_prefix}", "{header}", "{comment}", "{id} {comment}",
    "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}", "{id}/{rn}", "{rn}", "{{{id}}}\\t{comment}", "y" * 255,
    "{header}{id}{comment}{header}", "", "{id}_{cut_prefix} {rn}:{comment}",
]


def compile_rule(template: str, paired: bool) -> List[Tuple[str, object]]:
    """-> [("literal", bytes) | ("variable", name)], neighbouring literals joined; ValueError for everything the option
    refuses."""
    out: List[Tuple[str, object]] = []
    at = 0
    for tok in _TOKEN.finditer(template):
        if tok.start() != at:
            break
        at = tok.end()
        t = tok.group()
        if len(t) > 1 and t[0] == "{" and t != "{{":
            name = t[1:-1]
            if name == "" or name.isdigit():
                raise ValueError(f"empty or positional field {t}")
            if ":" in name or "!" in name:
                raise ValueError(f"format spec or conversion in {t}")
            bare = name[3:] if name[:3] in ("r1.", "r2.") else name
            if bare in ("adapter_name", "match_sequence", "rc"):
                raise ValueError(f"{t}: no single match to name")
            if paired and bare == "cut_suffix":
                raise ValueError(f"{t}: the paired chains do not capture their 3' cuts")
            if not paired and name == "rn":
                raise ValueError(f"{t}: no mates in a single-end run")
            if name not in (PAIRED if paired else SINGLE):
                raise ValueError(f"unknown variable {t}")
            out.append(("variable", name))
            continue
        byte = {"{{": b"{", "}}": b"}", "\\t": b"\t"}.get(t)
        if byte is None:
            if t != "\t" and not " " <= t <= "~":
                raise ValueError(f"byte {t!r} outside printable ASCII")
            byte = t.encode("ascii")
        if out and out[-1][0] == "literal":
            out[-1] = ("literal", out[-1][1] + byte)
        else:
            out.append(("literal", byte))
    if at != len(template):
        raise ValueError(f"lone brace at position {at + 1}")
    if len(out) > MAX_SEGMENTS:
        raise ValueError("too many segments")
    if sum(len(v) for k, v in out if k == "literal") > MAX_LITERAL:
        raise ValueError("too many literal bytes")
    if sum(1 for k, v in out if k == "variable" and v in HEADER) > MAX_HEADER:
        raise ValueError("too many header-derived placeholders")
    return out


def split_name(name: bytes) -> Tuple[bytes, bytes]:
    """Renamer.parse_name on bytes: (id, comment)."""
    i = 0
    while i < len(name) and name[i] in BLANKS:
        i += 1
    j = i
    while j < len(name) and name[j] not in BLANKS:
        j += 1
    k = j
    while k < len(name) and name[k] in BLANKS:
        k += 1
    if j > i and k < len(name):
        return name[i:j], name[k:]
    return name, b""


def render(pieces, name: bytes, captures: Dict[str, bytes], rn: int = 1) -> bytes:
    """The record name.  ``name``: the header behind the SuffixRemover chain.  ``captures``: single end
    {"cut_prefix", "cut_suffix"}; paired {"r1.cut_prefix", "r2.cut_prefix"} -- the written mate's own {cut_prefix} is
    looked up by ``rn``; a missing key renders empty."""
    rid, comment = split_name(name)
    values = dict(captures)
    if "r1.cut_prefix" in captures or "r2.cut_prefix" in captures:
        values["cut_prefix"] = captures.get(f"r{rn}.cut_prefix", b"")
    values.update(header=name, id=rid, comment=comment, rn=str(rn).encode())
    return b"".join(v if k == "literal" else values.get(v, b"") for k, v in pieces)
