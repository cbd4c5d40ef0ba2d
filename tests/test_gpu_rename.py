"""cutadapt's ``--rename`` on the device (``cs_text_set_rename``; name_len / emit_name of text_kernels.hip.inc, the name
column of info_copy): every test goes through ``cs_text_*`` and compares byte for byte with ``hostfmt``'s records, the
name replaced by what the rule (tests/rename_rule.py) renders.  tests/test_rename_cpu.py holds the rule to Python's
``str.format`` and ``str.split`` and the template compiler to the rule.

Reference surface: ``Renamer`` / ``PairedEndRenamer`` with another template (cutseq/run.py:377-380, 642-645).
"""
import functools
import gzip
import json

import numpy as np
import pytest

from cutseq_amd import abi, plan as planmod, rename, run as cli, synth, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import hostfmt
import names_universe as nu
import rename_rule
import util
from test_gpu_per_file_format import as_fasta
from test_gpu_text import fastq_text

pytestmark = pytest.mark.gpu

TAKARAV3 = BUILDIN_ADAPTERS["TAKARAV3"]
SCHEME_UMI3_ONLY = "ACACGACGCTCTTCCGATCT>NNNNNAGATCGGAAGAGCACACGTC"  # its one capture is the SUFFIX
RX = "{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}"


# ---- the expectation: the oracle's results, hostfmt's records, the rule's names ----------------------------------------

def capture_names(tp, mate):
    """{1 | 2: variable} for the capturing cuts of a mate's chain: the rule's name for the device's first / second
    capture."""
    chain = tp.r1 if mate == 0 else tp.r2
    out = {}
    for op in chain.ops:
        if isinstance(op, planmod.CutOp) and op.capture:
            out[op.capture] = (f"r{mate + 1}.cut_prefix" if tp.paired else ("cut_prefix" if op.length > 0 else "cut_suffix"))
    return out


class Oracle:
    """The oracle's results for one batch, computed once; :meth:`streams` formats them under a template."""

    def __init__(self, tp, batch, names1, names2):
        self.tp, self.batch = tp, batch
        (self.res1, self.cap2, _), m2 = util.oracle_run(tp, batch, threads=8)
        self.res2 = m2[0] if m2 else None
        suffixes = [[s.encode() for s in c.name_suffixes] if c is not None else [] for c in (tp.r1, tp.r2)]
        self.names = [[hostfmt.strip_suffixes(nu.as_read(n), suffixes[0]) for n in names1],
                      [hostfmt.strip_suffixes(nu.as_read(n), suffixes[1]) for n in names2] if names2 is not None else None]
        assert names2 is None or all(hostfmt.ids_match(a, b) for a, b in zip(*self.names)), "the test's own names must pair up"
        self.rows = [[(util.row_bytes(s, ln, i), util.row_bytes(q, ln, i)) for i in range(batch.n)]
                     for s, q, ln in ((batch.seq1, batch.qual1, batch.len1), (batch.seq2, batch.qual2, batch.len2))[:2 if tp.paired else 1]]
        self.captures = []
        for i in range(batch.n):
            caps = {}
            for m, res in enumerate((self.res1, self.res2)[:2 if tp.paired else 1]):
                seq = self.rows[m][i][0]
                for which, variable in capture_names(tp, m).items():
                    r = res[i] if which == 1 else self.cap2[i]
                    off, ln = (int(r["cap_off"]), int(r["cap_len"])) if which == 1 else (int(r["off"]), int(r["len"]))
                    caps[variable] = seq[off:off + ln]
            self.captures.append(caps)
        self.routes = [hostfmt.route(int(self.res1[i]["flags"]), int(self.res2[i]["flags"]) if tp.paired else 0, tp.untrimmed_filter)
                       for i in range(batch.n)]

    def name(self, pieces, i, m):
        return rename_rule.render(pieces, self.names[m][i], self.captures[i], m + 1)

    def streams(self, template):
        """-> (streams[route][mate], counts[route]); ``template`` None: the plan's default, by hostfmt itself."""
        tp = self.tp
        pieces = rename_rule.compile_rule(template if template is not None else rename.default_template(tp.has_umi, tp.paired), tp.paired)
        parts = [[[], []] for _ in range(3)]
        counts = [0, 0, 0]
        for i, route in enumerate(self.routes):
            counts[route] += 1
            for m, res in enumerate((self.res1, self.res2)[:2 if tp.paired else 1]):
                seq, qual = self.rows[m][i]
                parts[route][m].append(hostfmt.fastq_record(self.name(pieces, i, m), seq, qual, int(res[i]["start"]), int(res[i]["stop"]),
                                                            tp.reverse_complement and not tp.paired))
        return [[b"".join(p) for p in row] for row in parts], counts


def run_renamed(tp, template, text1, text2, n, stride, max_records=None, **kw):
    """One batch through a fresh text engine with ``template`` (None: without cs_text_set_rename)."""
    compiled = rename.compile_template(template, tp) if template is not None else None
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2 or b""), 1) + 1024,
                                 max_records=max_records or max(n, 1), stride=stride, rename=compiled, **kw) as te:
            return te.run(text1, n, text2)


def first_difference(got: bytes, want: bytes) -> str:
    a, b = got.split(b"\n"), want.split(b"\n")
    line = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"line {line}: {(a + [b'<end>'])[line][:80]!r} != {(b + [b'<end>'])[line][:80]!r} ({len(got)} / {len(want)} bytes)"


def check(got, counts, want, want_counts, mates, what):
    assert counts[:3] == want_counts, what
    for route in range(3):
        for m in range(mates):
            if got[route][m] != want[route][m]:  # (not the streams themselves in the message)
                pytest.fail(f"{what}: route {route} mate {m + 1}: {first_difference(got[route][m], want[route][m])}")


# ---- every name of the universe ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def single_case(scheme):
    names = nu.single_names()
    assert len(names) == 22_409
    tp = util.compile_plan(scheme, planmod.CutadaptConfig(), False)
    batch = synth.generate_pairs(len(names), nu.READ_LEN, scheme, seed=41, single_end=True, adapter_fraction=0.5)
    oracle = Oracle(tp, batch, names, None)
    assert sum(1 for r in set(oracle.routes)) >= 2
    return tp, batch, fastq_text(names, batch.seq1, batch.qual1, batch.len1), oracle


SINGLE_CASES = ([(nu.SCHEME_TWO_UMIS, t) for t in rename_rule.SINGLE_TEMPLATES]
                + [(SCHEME_UMI3_ONLY, "{id}:{cut_suffix}"), (SCHEME_UMI3_ONLY, "{cut_prefix}|{cut_suffix}"),
                   (nu.SCHEME_NO_UMI, "{id}"), (nu.SCHEME_NO_UMI, "{id} {comment}"), (nu.SCHEME_NO_UMI, "{cut_prefix}{header}{cut_suffix}")])


@pytest.mark.parametrize("scheme, template", SINGLE_CASES,
                         ids=[f"{'two-umis' if s == nu.SCHEME_TWO_UMIS else ('umi3-only' if s == SCHEME_UMI3_ONLY else 'no-umi')}-{i}"
                              for i, (s, _t) in enumerate(SINGLE_CASES)])
def test_every_name_single_end(scheme, template):
    """The 22 409 names of U1 and U2 under every template of the list: two captures, the 3'-UMI-only scheme whose first
    capture is the suffix, no UMI at all (a capture placeholder renders empty)."""
    tp, batch, text, oracle = single_case(scheme)
    want, want_counts = oracle.streams(template)
    if scheme == SCHEME_UMI3_ONLY:
        assert all(len(c.get("cut_suffix", b"")) == 5 and "cut_prefix" not in c for c in oracle.captures[:50])
    got, counts = run_renamed(tp, template, text, None, batch.n, batch.stride)
    check(got, counts, want, want_counts, 1, template)


@functools.lru_cache(maxsize=None)
def paired_case():
    matching, _ = nu.pools()
    assert len(matching) + len(nu.pools()[1]) == 50_666
    tp = util.compile_plan(TAKARAV3, planmod.CutadaptConfig(), True)
    batch = synth.generate_pairs(len(matching), nu.READ_LEN, TAKARAV3, seed=42, adapter_fraction=0.5)
    names1, names2 = [a for a, _ in matching], [b for _, b in matching]
    oracle = Oracle(tp, batch, names1, names2)
    return (tp, batch, fastq_text(names1, batch.seq1, batch.qual1, batch.len1),
            fastq_text(names2, batch.seq2, batch.qual2, batch.len2), oracle)


@pytest.mark.parametrize("template", rename_rule.PAIRED_TEMPLATES, ids=[str(i) for i in range(len(rename_rule.PAIRED_TEMPLATES))])
def test_every_matching_pair(template):
    """The matching pool (47 854 of the 50 666 pairs) through TAKARAV3 as one batch: one template, each mate with its own
    header, id and comment, {rn} and the mate's own {cut_prefix}."""
    tp, batch, text1, text2, oracle = paired_case()
    want, want_counts = oracle.streams(template)
    got, counts = run_renamed(tp, template, text1, text2, batch.n, batch.stride)
    check(got, counts, want, want_counts, 2, template)


def test_mismatching_pairs_are_still_refused():
    """The other 2 812 pairs: "Input read IDs not identical" stays what it is under a template -- the error names the
    record, nothing is formatted, and the engine formats the next good batch by the template."""
    tp = util.compile_plan(TAKARAV3, planmod.CutadaptConfig(), True)
    good = nu.good_pairs()
    batch = synth.generate_pairs(nu.ERR_BATCH, nu.READ_LEN, TAKARAV3, seed=43, adapter_fraction=0.5)
    want, want_counts = Oracle(tp, batch, [a for a, _ in good], [b for _, b in good]).streams(RX)

    def texts(pairs):
        return (fastq_text([a for a, _ in pairs], batch.seq1, batch.qual1, batch.len1),
                fastq_text([b for _, b in pairs], batch.seq2, batch.qual2, batch.len2))

    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 17, max_records=nu.ERR_BATCH, stride=batch.stride,
                                 rename=rename.compile_template(RX, tp)) as te:
            good1, good2 = texts(good)
            for k, bad in zip(nu.ERR_POSITIONS, nu.mismatch_sample(len(nu.ERR_POSITIONS))):
                t1, t2 = texts(good[:k] + [bad] + good[k + 1:])
                with pytest.raises(textpath.TextFormatError) as e:
                    te.run(t1, nu.ERR_BATCH, t2)
                assert (e.value.code, e.value.record) == (abi.CS_TEXT_ERR_IDS_DIFFER, k)
                got, counts = te.run(good1, nu.ERR_BATCH, good2)
                check(got, counts, want, want_counts, 2, k)


# ---- lengths at the copy's edges ---------------------------------------------------------------------------------------

# header-derived segments: the tail of n & 3 bytes, the second dword at 128, the loop from byte 256 on (stretch_load /
# stretch_store); literal and capture segments: a byte per lane, the loop beyond 32
HEADER_EDGES = list(range(0, 6)) + list(range(127, 134)) + list(range(255, 262))
BYTE_EDGES = (1, 31, 32, 33)  # (0: a capture the scheme does not have, an empty literal is no segment -- covered above)
LETTERS = bytes((65 + (i * 7) % 26) for i in range(300))


def edge_names():
    """Every edge length as a lone id, as the id in front of a one-byte comment and as the comment behind a one-byte id;
    the three forms shift the header's alignment in the text as well."""
    out = []
    for n in HEADER_EDGES:
        out += [LETTERS[:n], LETTERS[:n] + b" c", b"i " + LETTERS[:n], b"  " + LETTERS[:n] + b"\t" + LETTERS[3:3 + n] + b" "]
    return out


@pytest.mark.parametrize("k", BYTE_EDGES)
def test_segment_lengths_at_the_copy_edges(k):
    """A capture of k bases and a literal of k bytes around header, id and comment of 0-5, 127-133 and 255-261 bytes."""
    scheme = "ACACGACGCTCTTCCGATCT" + "N" * k + ">AGATCGGAAGAGCACACGTC"
    st = planmod.CutadaptConfig()
    st.min_length = 0
    tp = util.compile_plan(scheme, st, False)
    names = edge_names()
    batch = synth.generate_pairs(len(names), 60, scheme, seed=45, single_end=True, adapter_fraction=0.3)
    oracle = Oracle(tp, batch, names, None)
    assert any(len(c["cut_prefix"]) == k for c in oracle.captures)
    text = fastq_text(names, batch.seq1, batch.qual1, batch.len1)
    for template in ("{cut_prefix}" + "L" * k + "{id}={comment}={header}", "{comment}" + "L" * k + "{cut_prefix}{cut_prefix}|{id}"):
        want, want_counts = oracle.streams(template)
        got, counts = run_renamed(tp, template, text, None, batch.n, batch.stride)
        check(got, counts, want, want_counts, 1, (k, template))


# ---- batch sizes, long reads ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, nu.ERR_BATCH])
def test_offsets_cross_the_blocks(n):
    """257 and 600 pairs: the output offsets of records behind the first 256-record block include the names' sizes of
    the blocks in front."""
    tp = util.compile_plan(TAKARAV3, planmod.CutadaptConfig(), True)
    batch = synth.generate_pairs(n, nu.READ_LEN, TAKARAV3, seed=46, adapter_fraction=0.5)
    names1 = [b"P%d/1" % i + b" 1:N:0:ACGT" * (i % 3) for i in range(n)]  # (names of three lengths: uneven offsets)
    names2 = [b"P%d/2" % i + b" 2:N:0:ACGT+TTGCA" * (i % 3) for i in range(n)]
    oracle = Oracle(tp, batch, names1, names2)
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2)
    for template in (RX + " {comment}", "{header}{id}{comment}{header}"):
        want, want_counts = oracle.streams(template)
        got, counts = run_renamed(tp, template, text1, text2, n, batch.stride)
        check(got, counts, want, want_counts, 2, (n, template))


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_reads_longer_than_the_rows(paired):
    """Row strides of 100 and 4 under reads of 150 nt: the captures of a long read come from the long-read kernel's
    result (LongRes), a batch mixes both kinds, a pair can have one long mate."""
    scheme = TAKARAV3 if paired else nu.SCHEME_TWO_UMIS
    tp = util.compile_plan(scheme, planmod.CutadaptConfig(), paired)
    n = 1500
    batch = synth.generate_pairs(n, 150, scheme, seed=47, single_end=not paired, adapter_fraction=0.5)
    rng = np.random.default_rng(8)
    cut = rng.random(n) < 0.4  # ragged lengths: tile reads and long reads in one batch
    batch.len1[cut] = rng.integers(0, 150, size=int(cut.sum())).astype(np.uint16)
    if paired:
        batch.len2[cut] = rng.integers(0, 150, size=int(cut.sum())).astype(np.uint16)
    names1 = [f"SIM:{i}/1 1:N:0:X".encode() if i % 3 else f"SIM:{i}.1".encode() for i in range(n)]
    names2 = [f"SIM:{i}/2 2:N:0:Y".encode() if i % 3 else f"SIM:{i}.2".encode() for i in range(n)] if paired else None
    oracle = Oracle(tp, batch, names1, names2)
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2) if paired else None
    template = "{id}_{cut_prefix} {rn}:" + RX[5:] + " {comment}" if paired else "{cut_suffix}-{cut_prefix} {id} {comment}"
    want, want_counts = oracle.streams(template)
    for stride in (batch.stride, 100, 4):
        got, counts = run_renamed(tp, template, text1, text2, n, stride)
        check(got, counts, want, want_counts, 2 if paired else 1, (stride, template))


# ---- the default template, given explicitly ------------------------------------------------------------------------------

def gunzip_streams(streams):
    return [[gzip.decompress(x) if x else x for x in row] for row in streams]


@functools.lru_cache(maxsize=None)
def plain_batch(paired, auto_rc=False, max_length=None):
    scheme = TAKARAV3 if paired else nu.SCHEME_TWO_UMIS
    st = planmod.CutadaptConfig()
    st.auto_rc = auto_rc
    st.max_length = max_length
    if auto_rc:
        scheme = scheme.replace(">", "<")
    tp = util.compile_plan(scheme, st, paired)
    n = 3000
    batch = synth.generate_pairs(n, 60, scheme, seed=48, single_end=not paired, adapter_fraction=0.5)
    names1 = [f"SIM:{i}/1 1:N:0:X\t{i}".encode() if i % 3 else f"SIM:{i}.1".encode() for i in range(n)]
    names2 = [f"SIM:{i}/2 2:N:0:Y".encode() if i % 3 else f"SIM:{i}.2".encode() for i in range(n)] if paired else None
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2) if paired else None
    return tp, batch, names1, names2, text1, text2


DEFAULT_CASES = {
    "plain-paired": (True, {}, {}),
    "plain-single": (False, {}, {}),
    "gz-paired": (True, {}, {"compress": True}),
    "gz-single": (False, {}, {"compress": True}),
    "fasta": (True, {}, {"fasta": True}),
    "mixed-formats": (True, {}, {"fasta_routes": 0b000110}),  # trimmed mate 2 and too-short mate 1 as FASTA
    "interleaved": (True, {}, {"interleave_out": True}),
    "interleaved-mate2-first": (True, {}, {"interleave_out": True, "mate2_first": True}),
    "too-long-route": (True, {"max_length": 45}, {"too_long_route": True}),
    "auto-rc-single": (False, {"auto_rc": True}, {}),
}


@pytest.mark.parametrize("case", list(DEFAULT_CASES))
def test_the_default_template_given_explicitly_changes_nothing(case):
    """The run's default template through cs_text_set_rename against the same engine without the call: the renamed
    instantiations of every format kernel (woven, four-route, mixed formats, reverse complement) and the deflate stage
    behind them give the bytes the plain ones give."""
    paired, plan_kw, engine_kw = DEFAULT_CASES[case]
    tp, batch, _n1, _n2, text1, text2 = plain_batch(paired, **plan_kw)
    if case == "auto-rc-single":
        assert tp.reverse_complement
    template = rename.default_template(tp.has_umi, tp.paired)
    assert tp.has_umi
    plain, plain_counts = run_renamed(tp, None, text1, text2, batch.n, batch.stride, **engine_kw)
    got, counts = run_renamed(tp, template, text1, text2, batch.n, batch.stride, **engine_kw)
    assert counts == plain_counts and sum(1 for c in counts if c) >= 2
    if engine_kw.get("compress"):
        plain, got = gunzip_streams(plain), gunzip_streams(got)
    assert len(got) == (4 if case == "too-long-route" else 3)
    for route in range(len(got)):
        for m in range(2):
            if got[route][m] != plain[route][m]:
                pytest.fail(f"{case}: route {route} mate {m + 1}: {first_difference(got[route][m], plain[route][m])}")
    if case == "too-long-route":
        assert counts[3] > 0 and got[3][0]
    if case.startswith("interleaved"):
        assert all(not row[1] for row in got)


def test_interleaved_input_and_a_template():
    """CS_INTERLEAVE_IN: both mates from one text, names by a template, against the two-file run's expectation."""
    tp, batch, names1, names2, text1, text2 = plain_batch(True)
    recs1, recs2 = text1.split(b"\n"), text2.split(b"\n")
    woven = b"".join(b"\n".join(recs1[4 * i:4 * i + 4]) + b"\n" + b"\n".join(recs2[4 * i:4 * i + 4]) + b"\n" for i in range(batch.n))
    template = "{id}/{rn} " + RX[5:] + "\\t{comment}"
    want, want_counts = Oracle(tp, batch, names1, names2).streams(template)
    got, counts = run_renamed(tp, template, woven, None, batch.n, batch.stride, interleave_in=True)
    check(got, counts, want, want_counts, 2, template)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_gzip_members_of_renamed_records(paired):
    """The deflate stage matches the previous record's NAME on output bytes: names by a template that hold blanks and
    tabs, as gzip members written on the device, equal the expectation after decompression."""
    tp, batch, names1, names2, text1, text2 = plain_batch(paired)
    template = ("{id}\\tRX:Z:{r1.cut_prefix}{r2.cut_prefix} {comment}" if paired else "{id}\\tRX:Z:{cut_prefix}{cut_suffix} {comment}")
    want, want_counts = Oracle(tp, batch, names1, names2).streams(template)
    assert b"\tRX:Z:" in want[0][0] and b"1:N:0:X\t" in want[0][0]
    got, counts = run_renamed(tp, template, text1, text2, batch.n, batch.stride, compress=True)
    check(gunzip_streams(got), counts, want, want_counts, 2 if paired else 1, template)


def test_fasta_records_by_a_template():
    tp, batch, names1, names2, text1, text2 = plain_batch(True)
    want, want_counts = Oracle(tp, batch, names1, names2).streams(RX)
    got, counts = run_renamed(tp, RX, text1, text2, batch.n, batch.stride, fasta_routes=0b000110)
    fasta = {(0, 1), (1, 0)}
    want = [[as_fasta(want[q][m]) if (q, m) in fasta else want[q][m] for m in range(2)] for q in range(3)]
    check(got, counts, want, want_counts, 2, "mixed formats")


# ---- the info table --------------------------------------------------------------------------------------------------

def info_tables(tp, template, text1, text2, n, stride, info):
    compiled = rename.compile_template(template, tp) if template is not None else None
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2)) + 1024, max_records=n, stride=stride,
                                 info=info, rename=compiled) as te:
            te.submit(0, text1, len(text1), text2, len(text2), n)
            res = te.wait(0)
            size, raw, rows = te.info(0)
            table = np.empty(max(size, 1), dtype=np.uint8)
            te.fetch_info(0, table)
            out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
            te.fetch(0, out[0], out[1])
    table = table[:size].tobytes()
    return (gzip.decompress(table) if info & abi.CS_INFO_GZIP else table), rows


@pytest.mark.parametrize("info", [abi.CS_INFO_ON, abi.CS_INFO_ON | abi.CS_INFO_GZIP], ids=["plain", "gz"])
def test_info_table_column_1_is_mate_1s_rendered_name(info):
    """Every row of the table: column 1 is mate 1's name as the output files carry it -- by the template --, the other
    columns are those of the table without the option, row for row.  (Names without tabs: a row splits into columns.)"""
    tp = util.compile_plan(TAKARAV3, planmod.CutadaptConfig(), True)
    n = 2000
    batch = synth.generate_pairs(n, 60, TAKARAV3, seed=49, adapter_fraction=0.6)
    names1 = [f"SIM:{i}/1 1:N:0:X {i}".encode() if i % 3 else f"SIM:{i}.1".encode() for i in range(n)]
    names2 = [f"SIM:{i}/2 2:N:0:Y".encode() if i % 3 else f"SIM:{i}.2".encode() for i in range(n)]
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2)
    oracle = Oracle(tp, batch, names1, names2)
    template = RX + " {comment}"
    default = rename_rule.compile_rule(rename.default_template(True, True), True)
    pieces = rename_rule.compile_rule(template, True)
    renamed_of = {oracle.name(default, i, 0): oracle.name(pieces, i, 0) for i in range(n)}
    assert len(renamed_of) == n
    plain, plain_rows = info_tables(tp, None, text1, text2, n, batch.stride, info)
    got, rows = info_tables(tp, template, text1, text2, n, batch.stride, info)
    assert rows == plain_rows >= n
    plain_lines, got_lines = plain.split(b"\n"), got.split(b"\n")
    assert len(plain_lines) == len(got_lines) == rows + 1 and got_lines[-1] == b""
    seen = set()
    for a, b in zip(plain_lines[:-1], got_lines[:-1]):
        name, rest = a.split(b"\t", 1)
        assert b == renamed_of[name] + b"\t" + rest
        seen.add(name)
    assert seen == set(renamed_of)


# ---- the C entry point's refusals ----------------------------------------------------------------------------------------

def test_set_rename_refuses_what_it_cannot_take():
    tp = util.compile_plan(nu.SCHEME_TWO_UMIS, planmod.CutadaptConfig(), False)
    rec = b"@a b\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n"
    seg = lambda *rows: ((abi.cs_rename_seg * max(len(rows), 1))(*rows), len(rows))
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 16, max_records=8, stride=24) as te:
            L = te.L
            bad = [
                (seg(*[(abi.CS_RENAME_ID, 0, 0, 0)] * 5), b"", "copy from the header"),
                (seg((7, 0, 0, 0)), b"", "kind 7"),
                (seg((abi.CS_RENAME_LITERAL, 0, 2, 3)), b"abcd", "reaches beyond"),
                (seg((abi.CS_RENAME_CAPTURE, 1, 0, 0)), b"", "mate 2 of a single-end plan"),
                (seg(*[(abi.CS_RENAME_LITERAL, 0, 0, 100)] * 3), b"x" * 100, "sum to 300 bytes"),
            ]
            for (table, n), literals, message in bad:
                assert L.cs_text_set_rename(te._h, table, n, literals, len(literals)) == abi.CS_ERR_ARG
                assert message in L.cs_last_error().decode()
            many = (abi.cs_rename_seg * 17)(*[(abi.CS_RENAME_MATE, 0, 0, 0)] * 17)
            assert L.cs_text_set_rename(te._h, many, 17, b"", 0) == abi.CS_ERR_ARG
            # nothing of that took hold: the default names
            streams, counts = te.run(rec, 1, None)
            assert b"".join(s[0] for s in streams).startswith(b"@a_")
            # ... and behind the first batch the names are settled
            table, n = seg((abi.CS_RENAME_ID, 0, 0, 0))
            assert L.cs_text_set_rename(te._h, table, n, b"", 0) == abi.CS_ERR_ARG
            assert "before the first cs_text_submit" in L.cs_last_error().decode()
        with textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 16, max_records=8, stride=24,
                                 rename=rename.compile_template("", tp)) as te:  # an empty name is legal
            streams, counts = te.run(rec, 1, None)
            assert b"".join(s[0] for s in streams).startswith(b"@\n")


# ---- the command line ----------------------------------------------------------------------------------------------------

R1 = str(util.GOLDEN / "fixture1k_R1.fq.gz")
R2 = str(util.GOLDEN / "fixture1k_R2.fq.gz")


def gunzip(path):
    with gzip.open(path, "rb") as fh:
        return fh.read()


def test_cli_keeps_the_comment_and_moves_the_umi_to_a_tag(tmp_path):
    """``--rename '{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix} {comment}'`` on the reference's own reads: every record is the
    default run's record with the name re-spelled (the UMI from behind '_' to the RX tag, Illumina's comment kept), the
    report's counts are those of the run without the option."""
    plain, renamed = str(tmp_path / "plain"), str(tmp_path / "renamed")
    template = RX + " {comment}"
    cli.main(["-A", "TAKARAV3", "--trim-polyA", "-O", plain, "--json-file", plain + ".json", "--info-file", plain + ".info.gz", R1, R2])
    cli.main(["-A", "TAKARAV3", "--trim-polyA", "-O", renamed, "--json-file", renamed + ".json", "--info-file", renamed + ".info.gz",
              "--rename", template, R1, R2])
    comments = [{n.split(b" ", 1)[0]: n.split(b" ", 1)[1] for n, _s, _q in util.read_fastq_gz(path)} for path in (R1, R2)]
    total = 0
    for kind in ("trimmed", "short"):
        for m in (1, 2):
            a = gunzip(f"{plain}_{kind}_R{m}.fastq.gz").split(b"\n")
            b = gunzip(f"{renamed}_{kind}_R{m}.fastq.gz").split(b"\n")
            assert len(a) == len(b) and a[1::4] == b[1::4] and a[3::4] == b[3::4]
            for old, new in zip(a[0::4], b[0::4]):
                if not old:
                    continue
                rid, umi = old[1:].rsplit(b"_", 1)
                assert new == b"@" + rid + b" RX:Z:" + umi + b" " + comments[m - 1][rid]
                total += 1
    assert total == 2000
    a, b = json.loads(open(plain + ".json").read()), json.loads(open(renamed + ".json").read())
    assert a["read_counts"] == b["read_counts"] and a["basepair_counts"] == b["basepair_counts"]
    assert a["adapters_read1"] == b["adapters_read1"] and a["adapters_read2"] == b["adapters_read2"]
    # the info table: mate 1's rendered name in column 1
    ia, ib = gunzip(plain + ".info.gz").split(b"\n"), gunzip(renamed + ".info.gz").split(b"\n")
    assert len(ia) == len(ib) > 1000
    for old, new in zip(ia[:-1], ib[:-1]):
        name, rest = old.split(b"\t", 1)
        rid, umi = name.rsplit(b"_", 1)
        assert new == rid + b" RX:Z:" + umi + b" " + comments[0][rid] + b"\t" + rest
