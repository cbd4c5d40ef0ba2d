"""--info-file on the GPU: the table the device writes (info_kernels.hip.inc) against tests/info_rule.py, byte for byte.

ABI level: every built-in preset, single and paired, with and without the flags that change the chain, on fixture reads,
synthetic reads and planted ones; the record streams of the same submit equal those of a submit without ``info``.  Every
case first proves on the EXPECTED table that it holds no-match rows, reads with several rows and a match row of every
adapter op of mate 1's chain.  Then: row stride 4 (every read in the long-read walk), a read near 100 000 nt, odd bytes,
FASTA input, the gzip member, and the command line (plain / .gz, --ranks 2, --max-n 0, paired --auto-rc, small blocks).
"""
import gzip
import json
import random
import zlib

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, run as cli, synth, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig
from cutseq_amd.engine import TrimEngine

import info_rule
import util
from test_gpu_text import run_text_exposed

pytestmark = pytest.mark.gpu

R1_10K = util.GOLDEN / "fixture10k_R1.fq.gz"
R2_10K = util.GOLDEN / "fixture10k_R2.fq.gz"

# every flag that changes the chain or the aligner on its own (so a failure names it), both selection values with and
# without the poly ops, and everything at once
FLAG_SETS = {
    "default": {},
    "polyA": {"trim_polyA": True},
    "polyA-any-dir": {"trim_polyA": True, "trim_polyA_wo_direction": True},
    "anywhere": {"force_anywhere": True},
    "uncond": {"conditional_cutter": False},
    "sel3": {"select_rule": abi.CS_SELECT_SCORE},
    "polyA+sel3": {"trim_polyA": True, "select_rule": abi.CS_SELECT_SCORE},
    "polyA-any-dir+anywhere+uncond+sel3": {"trim_polyA": True, "trim_polyA_wo_direction": True, "force_anywhere": True,
                                           "conditional_cutter": False, "select_rule": abi.CS_SELECT_SCORE},
}


def settings(flags):
    st = planmod.CutadaptConfig()
    for k, v in flags.items():
        setattr(st, k, v)
    return st


def planted_reads(scheme: str, rng: random.Random, paired: bool):
    """Reads of mate 1 on which every adapter op of the chain can match: the library's own layout around an insert with
    a poly-T head and a poly-A tail; the same with a damaged 3' adapter; a bare insert (no match at all)."""
    bc = BarcodeConfig(scheme)

    def insert(n):
        return "".join(rng.choice("CG") for _ in range(n))  # nothing the adapters or the poly ops can take

    inner = "T" * 32 + insert(40) + "A" * 32
    tail3 = "" if paired else bc.inline3.fw  # (paired: mate 1 loses inline3 to a cutter, not to an adapter op)
    core = (bc.inline5.fw + insert(bc.umi5.len) + insert(bc.mask5.len) + inner + insert(bc.mask3.len) + insert(bc.umi3.len)
            + (tail3 if not paired else insert(bc.inline3.len)))
    out = ["GG" + bc.p5.fw + core + bc.p7.fw + "CC",
           "GG" + bc.p5.fw + core + util.mutate(rng, bc.p7.fw, 1, "CG"),
           core + bc.p7.fw,
           insert(90),
           insert(12)]
    return [(s, "I" * len(s)) for s in out]


def build_case(name: str, flags: dict, paired: bool, n_fixture=100, n_synth=100, seed=11):
    """-> (scheme, st, tp, records1, records2 | None), records as [(name, seq, qual)] bytes."""
    scheme = BUILDIN_ADAPTERS.get(name, name)
    st = settings(flags)
    rng = random.Random(seed + len(name))
    rec1 = util.read_fastq_gz(R1_10K, limit=n_fixture)
    rec2 = util.read_fastq_gz(R2_10K, limit=n_fixture)
    batch = synth.generate_pairs(n_synth, 150, scheme, seed=seed, chunk_index=len(name), poly_fraction=0.2, art5_fraction=0.1)
    for i in range(n_synth):
        head = f"SYN:{i}/%d 1:N:0:X" if i % 3 else f"SYN:{i}.%d"
        rec1.append(((head % 1).encode(), util.row_bytes(batch.seq1, batch.len1, i), util.row_bytes(batch.qual1, batch.len1, i)))
        rec2.append(((head % 2).encode(), util.row_bytes(batch.seq2, batch.len2, i), util.row_bytes(batch.qual2, batch.len2, i)))
    for i, (s, q) in enumerate(planted_reads(scheme, rng, paired)):
        rec1.append((b"PLANT:%d/1" % i, s.encode(), q.encode()))
        s2 = "".join(rng.choice("CG") for _ in range(60))
        rec2.append((b"PLANT:%d/2" % i, s2.encode(), b"I" * 60))
    tp = util.compile_plan(scheme, st, paired, untrimmed_requested="INLINE" in name)
    return scheme, st, tp, rec1, (rec2 if paired else None)


def text_of(records, eol=b"\n", final_newline=True):
    body = b"".join(b"@" + n + eol + s + eol + b"+" + eol + q + eol for n, s, q in records)
    return body if final_newline else body[: -len(eol)]


def run_with_info(tp, text1, text2, n, stride, info=abi.CS_INFO_ON, max_records=None):
    """One batch with ``info`` -> (table as fetched, (bytes, text bytes, rows), streams[route][mate], res)."""
    paired = text2 is not None
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2 or b""), 1) + 1024,
                                 max_records=max_records or max(n, 1), stride=stride, info=info) as te:
            te.submit(0, text1, len(text1), text2, len(text2) if paired else 0, n)
            res = te.wait(0)
            sizes = te.info(0)
            table = np.empty(max(sizes[0], 1), dtype=np.uint8)
            te.fetch_info(0, table)
            out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
            te.fetch(0, out[0], out[1] if paired else None)
            streams = textpath.split_routes(res, out, paired)
            with pytest.raises(capi.CsError):  # the slot is free again: nothing to ask about
                te.info(0)
    return table[:sizes[0]].tobytes(), sizes, streams, res


def check_guard(want: bytes, tp, what):
    """The expected table is worth comparing against: no-match rows, reads with several rows, every adapter op."""
    no_match, multi, per_adapter = info_rule.census(want)
    names = planmod.info_adapter_names(tp.r1.ops)
    assert no_match >= 1 and multi >= 1, (what, no_match, multi)
    assert sorted(per_adapter) == sorted(names.values()), (what, per_adapter, names)


def check_case(scheme, st, tp, rec1, rec2, stride, what, untrimmed_requested=False, guard=True):
    want = info_rule.table(scheme, st, rec1, rec2, untrimmed_requested)
    if guard:
        check_guard(want, tp, what)
    text1, text2 = text_of(rec1), (text_of(rec2) if rec2 is not None else None)
    table, sizes, streams, res = run_with_info(tp, text1, text2, len(rec1), stride)
    assert table == want, (what, stride)
    assert sizes[0] == sizes[1] == len(want) and sizes[2] == want.count(b"\n"), (what, sizes)
    plain = run_text_exposed(tp, text1, text2, len(rec1), stride)
    assert streams == plain.streams, (what, stride)
    return res


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("flagset", list(FLAG_SETS))
@pytest.mark.parametrize("name", sorted(BUILDIN_ADAPTERS))
def test_table_equals_the_rule_for_every_preset(name, flagset, paired):
    scheme, st, tp, rec1, rec2 = build_case(name, FLAG_SETS[flagset], paired)
    check_case(scheme, st, tp, rec1, rec2, 152 if max(len(r[1]) for r in rec1) <= 152 else 256, (name, flagset, paired),
               untrimmed_requested="INLINE" in name)


def test_info_needs_asking_and_refuses_demultiplexing():
    st = settings({})
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, False)
    with TrimEngine(tp, device=0, slots=0) as eng:
        with textpath.TextEngine(eng, slots=1, max_text_bytes=4096, max_records=16, stride=152) as te:
            text = b"@a\nACGT\n+\nIIII\n"
            te.submit(0, text, len(text), None, 0, 1)
            te.wait(0)
            with pytest.raises(capi.CsError) as exc:
                te.info(0)
            assert exc.value.code == abi.CS_ERR_STATE
            with pytest.raises(capi.CsError) as exc:
                te.fetch_info(0, np.empty(16, dtype=np.uint8))
            assert exc.value.code == abi.CS_ERR_STATE
            te.fetch(0, np.empty(64, dtype=np.uint8))
    st.demux_barcodes = ["ACGTAC", "TTGACA"]
    tpd = util.compile_plan("ACACGACGCTCTTCCGATCT(ACGTAC)>AGATCGGAAGAGCACACGTC", st, False)
    from cutseq_amd import demux
    demux.ensure_tables(tpd, 0)
    with TrimEngine(tpd, device=0, slots=0) as eng:
        with pytest.raises(capi.CsError) as exc:
            textpath.TextEngine(eng, slots=1, max_text_bytes=4096, max_records=16, stride=152, bins=2, info=abi.CS_INFO_ON)
        assert exc.value.code == abi.CS_ERR_ARG


@pytest.mark.parametrize("name,paired", [("TAKARAV3", True), ("SMALLRNA", False), ("ECLIP10", True)])
def test_row_stride_four_sends_every_read_through_the_long_read_walk(name, paired):
    scheme, st, tp, rec1, rec2 = build_case(name, FLAG_SETS["polyA"], paired, n_fixture=60, n_synth=60)
    res = check_case(scheme, st, tp, rec1, rec2, 4, (name, paired, "stride 4"), untrimmed_requested="INLINE" in name)
    assert res.n_long[0] == sum(1 for r in rec1 if len(r[1]) > 4)


def test_a_read_near_100000_nt_with_a_planted_adapter():
    rng = random.Random(99)
    scheme = BUILDIN_ADAPTERS["TAKARAV3"]
    bc = BarcodeConfig(scheme)
    body = "".join(rng.choice("CG") for _ in range(99_950))
    long_read = body + bc.p7.fw + "CCGG"
    rec1 = [(b"short/1", b"CGCGGCGCCGCGGGCCGCGCGGCGCGCC", b"I" * 28), (b"long/1", long_read.encode(), b"I" * len(long_read)),
            (b"tail/1", (body[:200] + bc.p7.fw[:9]).encode(), b"I" * 209)]
    st = settings({})
    tp = util.compile_plan(scheme, st, False)
    want = info_rule.table(scheme, st, rec1)
    rows = want.split(b"\n")
    assert rows[1].split(b"\t")[1:4] == [b"0", b"99950", b"%d" % (99_950 + len(bc.p7.fw))]
    text1 = text_of(rec1)
    table, sizes, streams, res = run_with_info(tp, text1, None, 3, 152)
    assert table == want and res.n_long[0] == 2
    assert streams == run_text_exposed(tp, text1, None, 3, 152).streams


@pytest.mark.parametrize("seed", [1, 2])
def test_odd_bytes(seed):
    """util.odd_alphabet_cases: lower case, IUPAC, every quality character, empty reads, case-sensitive plans, FIND."""
    for k, (scheme, st, paired, reads1, reads2, untrimmed_requested) in enumerate(util.odd_alphabet_cases(seed, rounds=3, pairs=250)):
        rec1 = [(b"F:%d/1 a comment" % i if i % 2 else b"F:%d.1" % i, s.encode(), q.encode()) for i, (s, q) in enumerate(reads1)]
        rec2 = [(b"F:%d/2 a comment" % i if i % 2 else b"F:%d.2" % i, s.encode(), q.encode()) for i, (s, q) in enumerate(reads2)]
        tp = util.compile_plan(scheme, st, paired, untrimmed_requested=untrimmed_requested)
        check_case(scheme, st, tp, rec1, rec2 if paired else None, 156, (seed, k, scheme), untrimmed_requested, guard=False)


def test_line_ends_last_record_and_two_umis():
    """'\\r\\n' line ends, a last record without a line end, names with /1 and comments, 5' and 3' UMIs single-end."""
    scheme = "ACACGACGCTCTTCCGATCTNNNN>NNNAGATCGGAAGAGCACACGTC"
    st = settings({})
    tp = util.compile_plan(scheme, st, False)
    _, _, _, rec1, _ = build_case(scheme, {}, False, n_fixture=40, n_synth=40)
    rec1 = [(n + b" comment/1" if i % 2 else n, s, q) for i, (n, s, q) in enumerate(rec1)]
    want = info_rule.table(scheme, st, rec1)
    check_guard(want, tp, "two UMIs")
    assert any(b"_" in row.split(b"\t")[0] for row in want.split(b"\n")[:-1])
    for eol, final in ((b"\r\n", True), (b"\n", False), (b"\r\n", False)):
        text1 = text_of(rec1, eol, final)
        table, _, streams, _ = run_with_info(tp, text1, None, len(rec1), 152)
        assert table == want, (eol, final)
        assert streams == run_text_exposed(tp, text1, None, len(rec1), 152).streams


def test_input_without_qualities_leaves_the_quality_columns_empty():
    scheme, st, tp, rec1, _ = build_case("TAKARAV3", {"min_quality": 0}, False, n_fixture=40, n_synth=40)
    rec1 = [(n, s, b"~" * len(s)) for n, s, _q in rec1]  # what the FASTA reader hands to the device
    want = info_rule.table(scheme, st, rec1, has_qual=False)
    check_guard(want, tp, "fasta")
    assert b"~" not in want
    table, _, _, _ = run_with_info(tp, text_of(rec1), None, len(rec1), 152, info=abi.CS_INFO_ON | abi.CS_INFO_NO_QUAL)
    assert table == want and b"~" not in table


def check_gzip_member(blob: bytes, want: bytes):
    assert gzip.decompress(blob) == want
    if want:
        assert int.from_bytes(blob[-8:-4], "little") == zlib.crc32(want)
        assert int.from_bytes(blob[-4:], "little") == len(want) & 0xFFFFFFFF


def test_gzip_member_from_the_device():
    scheme, st, tp, rec1, rec2 = build_case("TAKARAV3", FLAG_SETS["polyA"], True, n_fixture=400, n_synth=300)
    want = info_rule.table(scheme, st, rec1, rec2)
    assert len(want) > 3 * 32768  # several deflate chunks
    table, sizes, _, _ = run_with_info(tp, text_of(rec1), text_of(rec2), len(rec1), 152, info=abi.CS_INFO_ON | abi.CS_INFO_GZIP)
    assert sizes[1] == len(want) and sizes[0] == len(table) < len(want)
    assert table[:3] == b"\x1f\x8b\x08"
    check_gzip_member(table, want)


# ---- command line ----------------------------------------------------------------------------------------------------


def write_inputs(tmp_path, rec1, rec2=None, gz_members=0):
    paths = []
    for mate, recs in ((1, rec1), (2, rec2)):
        if recs is None:
            continue
        path = tmp_path / (f"in_R{mate}.fastq.gz" if gz_members else f"in_R{mate}.fastq")
        if gz_members:
            with open(path, "wb") as fh:
                for lo in range(0, len(recs), gz_members):
                    fh.write(gzip.compress(text_of(recs[lo:lo + gz_members]), 1))
        else:
            path.write_bytes(text_of(recs))
        paths.append(str(path))
    return paths


def gunzip(path):
    with gzip.open(path, "rb") as fh:
        return fh.read()


def test_cli_plain_and_gz_info_files_in_many_small_blocks(tmp_path, monkeypatch):
    scheme, st, tp, rec1, rec2 = build_case("TAKARAV3", FLAG_SETS["polyA"], True, n_fixture=500, n_synth=400)
    want = info_rule.table(scheme, st, rec1, rec2)
    check_guard(want, tp, "cli")
    ins = write_inputs(tmp_path, rec1, rec2)
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "64")  # 15 blocks over three slots
    base = ["-A", "TAKARAV3", "--trim-polyA"]
    cli.main(base + ["-O", str(tmp_path / "ref")] + ins)
    cli.main(base + ["-O", str(tmp_path / "a"), "--info-file", str(tmp_path / "a.info.tsv"), "--json-file", str(tmp_path / "a.json")] + ins)
    cli.main(base + ["-O", str(tmp_path / "b"), "--info-file", str(tmp_path / "b.info.tsv.gz")] + ins)
    assert (tmp_path / "a.info.tsv").read_bytes() == want
    blob = (tmp_path / "b.info.tsv.gz").read_bytes()
    assert gunzip(tmp_path / "b.info.tsv.gz") == want
    # one member per block, each with a valid CRC and ISIZE: zlib checks both, member by member
    at, members, text = 0, 0, b""
    while at < len(blob):
        d = zlib.decompressobj(31)
        text += d.decompress(blob[at:])
        assert d.eof
        at = len(blob) - len(d.unused_data)
        members += 1
    assert text == want and members == -(-len(rec1) // 64)
    for kind in ("trimmed", "short"):
        for mate in (1, 2):
            ref = gunzip(tmp_path / f"ref_{kind}_R{mate}.fastq.gz")
            assert gunzip(tmp_path / f"a_{kind}_R{mate}.fastq.gz") == ref and gunzip(tmp_path / f"b_{kind}_R{mate}.fastq.gz") == ref
    rep = json.loads((tmp_path / "a.json").read_text())
    assert list(rep["output"])[-1] == "info_file" and rep["output"]["info_file"] == str(tmp_path / "a.info.tsv")


def test_cli_without_the_option_writes_what_the_rule_writes(tmp_path):
    """No --info-file: the outputs are those of the string-level restatement (what the existing CLI tests expect) and
    the report's output block has the keys it always had."""
    from test_gpu_cli import R1, R2, expected
    prefix = str(tmp_path / "out")
    cli.main(["-A", "TAKARAV3", "--trim-polyA", "-O", prefix, "--json-file", str(tmp_path / "r.json"), R1, R2])
    want = expected(BUILDIN_ADAPTERS["TAKARAV3"], {"trim_polyA": True}, True)
    for kind in ("trimmed", "short"):
        assert gunzip(f"{prefix}_{kind}_R1.fastq.gz") == want[kind][0]
        assert gunzip(f"{prefix}_{kind}_R2.fastq.gz") == want[kind][1]
    rep = json.loads((tmp_path / "r.json").read_text())
    assert list(rep["output"]) == ["output1", "output2", "short1", "short2", "untrimmed1", "untrimmed2"]
    assert not list(tmp_path.glob("*info*"))


@pytest.mark.parametrize("ending", ["", ".gz"])
def test_cli_two_ranks_equal_one_process(tmp_path, monkeypatch, ending):
    scheme, st, tp, rec1, rec2 = build_case("TAKARAV3", {}, True, n_fixture=600, n_synth=400)
    want = info_rule.table(scheme, st, rec1, rec2)
    ins = write_inputs(tmp_path, rec1, rec2, gz_members=100)
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "128")
    one, two = str(tmp_path / ("one.tsv" + ending)), str(tmp_path / ("two.tsv" + ending))
    cli.main(["-A", "TAKARAV3", "-O", str(tmp_path / "one"), "--info-file", one] + ins)
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    cli.main(["-A", "TAKARAV3", "-O", str(tmp_path / "two"), "--info-file", two, "--ranks", "2"] + ins)
    read = gunzip if ending else (lambda p: open(p, "rb").read())
    assert read(one) == want and read(two) == want
    if not ending:
        assert open(one, "rb").read() == open(two, "rb").read()
    assert not list(tmp_path.glob("*.part*"))


def test_cli_max_n_zero_keeps_the_rows_of_discarded_pairs(tmp_path):
    scheme, st, tp, rec1, rec2 = build_case("TAKARAV3", {}, True, n_fixture=200, n_synth=100)
    for i in range(0, len(rec1), 7):  # an N in the middle of the insert: the pair is discarded
        n, s, q = rec1[i]
        if len(s) > 30:
            rec1[i] = (n, s[:15] + b"N" + s[16:], q)
    want = info_rule.table(scheme, st, rec1, rec2)
    ins = write_inputs(tmp_path, rec1, rec2)
    info = tmp_path / "info.tsv"
    cli.main(["-A", "TAKARAV3", "-O", str(tmp_path / "o"), "--max-n", "0", "--info-file", str(info), "--json-file", str(tmp_path / "r.json")] + ins)
    rep = json.loads((tmp_path / "r.json").read_text())
    assert rep["read_counts"]["filtered"]["too_many_n"] > 0
    assert info.read_bytes() == want
    names = {row.split(b"\t")[0] for row in want.split(b"\n")[:-1]}
    assert len(names) == len(rec1)  # every input record has rows, the discarded ones included


def test_cli_paired_auto_rc_table_is_about_input_read_one(tmp_path):
    scheme, st, tp, rec1, rec2 = build_case("TAKARAV3", {"auto_rc": True}, True, n_fixture=200, n_synth=100)
    assert tp.swap_outputs
    want = info_rule.table(scheme, st, rec1, rec2)
    check_guard(want, tp, "auto-rc")
    ins = write_inputs(tmp_path, rec1, rec2)
    info = tmp_path / "info.tsv"
    cli.main(["-A", "TAKARAV3", "--auto-rc", "-O", str(tmp_path / "o"), "--info-file", str(info)] + ins)
    assert info.read_bytes() == want


def test_cli_single_end_auto_rc_turns_the_no_match_rows(tmp_path):
    scheme, st, tp, rec1, _ = build_case("TAKARAV3", {"auto_rc": True}, False, n_fixture=150, n_synth=100)
    assert tp.reverse_complement
    rec1 = [(n, s.replace(b"N", b"C"), q) for n, s, q in rec1]  # (A, C, G, T only: every complement table agrees there)
    want = info_rule.table(scheme, st, rec1)
    check_guard(want, tp, "auto-rc single")
    ins = write_inputs(tmp_path, rec1)
    info = tmp_path / "info.tsv"
    cli.main(["-A", "TAKARAV3", "--auto-rc", "-O", str(tmp_path / "o"), "--info-file", str(info)] + ins)
    assert info.read_bytes() == want
