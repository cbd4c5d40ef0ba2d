"""A small universe of record NAMES, enumerated -- the counterpart of ``tests/universe.py`` for the header work of the
text path (text_kernels.hip.inc: text_parse_records, text_check_pairs, format_copy; the name column of info_copy) and
of its host twin (cutseq_host.c: strip_suffixes, read_id, ids_match).

Reference surface replaced: ``SuffixRemover``, ``Renamer.parse_name``, ``PairedEndRenamer`` and dnaio's
``record_names_match`` (cutseq/run.py:330, 377-380, 537-542, 642-645).

  U1  every byte string of length 0..5 over ``a 1 2 / . <space> <tab>`` (19 608 names): both suffix literals of both
      mates (``.1 /1 .2 /2``), chains of them (``a/1.1``), names that are nothing but a suffix, ids that end in a mate
      digit, leading / trailing / repeated blanks, all-blank and empty headers
  U2  every byte string of length 0..4 over ``a <space> \\t \\v \\f \\r \\x1c`` (2 801 names): every kind of white space
      the id rule knows -- ``\\x1c`` is one for ``str.split`` and none for ``bytes.split`` -- none of which but space and
      tab ends an id for dnaio's pair check.  ``\\n`` is in neither alphabet: it ends the header line.

A name that ends in ``\\r`` reaches the record logic WITHOUT that byte: the line reader takes ``\\r\\n`` as the line end
(:func:`as_read`).  Everything here that classifies or expects goes by the name as read.

Pairs: mate 2's name is mate 1's under a small fixed set of edits (:func:`mates`); the specification
(``hostfmt.strip_suffixes`` per mate, then ``hostfmt.ids_match``) sorts every pair into MATCHING or MISMATCHING.  Nothing
is dropped: :func:`pools` asserts that every name of U1 and U2 sits in at least one pair and that each pool holds at
least 1 000 pairs.  Deterministic: no seed, the same names and pairs in the same order every run.
"""
from __future__ import annotations

import functools
import itertools
from typing import List, Tuple

import hostfmt

U1_ALPHABET = b"a12/. \t"
U2_ALPHABET = b"a \t\v\f\r\x1c"
SUFFIXES = ((b".1", b"/1"), (b".2", b"/2"))  # MateChain.name_suffixes of mate 1 / mate 2 (plan.compile_paired)
BLANKS = b" \t\n\v\f\r\x1c\x1d\x1e\x1f"      # str.split()'s white space below 0x80


def names(alphabet: bytes, max_len: int) -> List[bytes]:
    """Every byte string over ``alphabet`` of length 0..max_len, shortest first."""
    return [bytes(t) for n in range(max_len + 1) for t in itertools.product(alphabet, repeat=n)]


@functools.lru_cache(maxsize=None)
def u1() -> Tuple[bytes, ...]:
    out = tuple(names(U1_ALPHABET, 5))
    assert len(out) == 19_608
    return out


@functools.lru_cache(maxsize=None)
def u2() -> Tuple[bytes, ...]:
    out = tuple(names(U2_ALPHABET, 4))
    assert len(out) == 2_801
    return out


def as_read(name: bytes) -> bytes:
    """The name the line reader hands on: a ``\\r`` in front of the line's ``\\n`` belongs to the line end.  (ONE: in
    front of a ``\\r\\n`` line end, write ``as_read(name)`` to have the reader hand on what it does for ``name`` in front of
    a bare ``\\n`` -- a name that ends in ``\\r`` already carries that byte.)"""
    return name[:-1] if name.endswith(b"\r") else name


def mates(name: bytes) -> List[bytes]:
    """Mate 2's names for mate 1's ``name``, without repeats, in a fixed order:
    the identical name; the trailing mate digit of the id (up to the first space / tab) changed, 1 <-> 2; a ``.1`` /
    ``/1`` at the end of the header turned into ``.2`` / ``/2``; a different comment behind the first blank -- any blank
    of the id rule, so behind a ``\\v`` or ``\\x1c`` the "comment" is part of the id for the pair check -- or, where the
    header has no blank, a comment added."""
    out = [name]
    stop = len(hostfmt.pair_id(name))
    if stop and name[stop - 1:stop] in (b"1", b"2"):
        out.append(name[:stop - 1] + (b"2" if name[stop - 1:stop] == b"1" else b"1") + name[stop:])
    if name.endswith((b".1", b"/1")):
        out.append(name[:-1] + b"2")
    blank = next((i for i, c in enumerate(name) if c in BLANKS), None)
    out.append(name + b" c2" if blank is None else name[:blank + 1] + b"c2")
    seen, uniq = set(), []
    for m in out:
        if m not in seen:
            seen.add(m)
            uniq.append(m)
    return uniq


def pair_matches(name1: bytes, name2: bytes) -> bool:
    """The specification's verdict on a pair of names as written in the two files."""
    return hostfmt.ids_match(hostfmt.strip_suffixes(as_read(name1), SUFFIXES[0]),
                             hostfmt.strip_suffixes(as_read(name2), SUFFIXES[1]))


@functools.lru_cache(maxsize=None)
def pools():
    """-> (matching, mismatching): lists of (name1, name2) over U1 and U2, every pair in exactly one of them."""
    matching, mismatching = [], []
    in_u1 = set(u1())
    for name in u1() + tuple(n for n in u2() if n not in in_u1):  # (names over a, space and tab are in both)
        for other in mates(name):
            (matching if pair_matches(name, other) else mismatching).append((name, other))
    covered = {a for a, _ in matching} | {a for a, _ in mismatching}
    assert covered == set(u1()) | set(u2()), "a name of the universe sits in no pair"
    assert len(matching) >= 1000 and len(mismatching) >= 1000, (len(matching), len(mismatching))
    return matching, mismatching


# ---- what the CPU twin (tests/test_names_cpu.py) and the GPU tests (tests/test_gpu_text_names.py) share -----------------

SCHEME_TWO_UMIS = "ACACGACGCTCTTCCGATCTNNNN>NNNAGATCGGAAGAGCACACGTC"  # single end: '{id}_{cut_prefix}{cut_suffix}'
SCHEME_NO_UMI = "ACACGACGCTCTTCCGATCT>AGATCGGAAGAGCACACGTC"           # '{id}'
READ_LEN = 40                 # every read of these tests: short, so that adapters planted in them fill all routes
ERR_BATCH = 600               # pairs per batch of the mismatch tests: three blocks of text_check_pairs
ERR_POSITIONS = (0, 63, 64, 255, 256, 257, 599)  # first / last lanes of waves and blocks, the last record


def single_names() -> List[bytes]:
    """U1 then U2, as written into the file."""
    return list(u1() + u2())


def good_pairs(n: int = ERR_BATCH) -> List[Tuple[bytes, bytes]]:
    """``n`` matching pairs spread evenly over the matching pool."""
    matching, _ = pools()
    step = len(matching) // n
    return matching[::step][:n]


def mismatch_sample(n: int = 200, seed: int = 20) -> List[Tuple[bytes, bytes]]:
    import random
    _, mismatching = pools()
    return random.Random(seed).sample(mismatching, n)
