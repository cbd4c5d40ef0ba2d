"""--too-long-output on the GPU: the pairs -M catches form a fourth stream of the text path (cs_text_params.too_long_route)
and two more files of the command line.  Expected streams: the string pipeline's records (oracle/pyref.py; for the
single-adapter plan, which no scheme expresses, the C oracle's intervals through the host formatter) routed by
tests/toolong_rule.py."""
import gzip
import json
import random

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS
from cutseq_amd.engine import TrimEngine

import toolong_rule
import util
from test_gpu_filters_cli import gunzip, inputs, pipeline_records, stderr_line, thresholds
from test_gpu_filters import ADAPTER, fastq_text

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 513]
HUGE = 70000


# ---- the reference, computed once ------------------------------------------------------------------------------

_CACHE = {}


def fixture_records(tmp_path_factory):
    """The 1000-pair fixture with the N runs of ``test_gpu_filters_cli.inputs``: (records per mate, gz paths)."""
    if "inputs" not in _CACHE:
        _CACHE["inputs"] = inputs(tmp_path_factory.mktemp("too_long_inputs"))
    return _CACHE["inputs"]


def paired_case(tmp_path_factory, min_length=20):
    """TAKARAV3 paired with --ensure-inline-barcode and untrimmed files, as the command-line runs below have them.
    -> (plan settings, records of the string pipeline, text of mate 1, text of mate 2)"""
    key = ("paired", min_length)
    if key not in _CACHE:
        (rec1, rec2), _paths = fixture_records(tmp_path_factory)
        st = planmod.CutadaptConfig()
        st.ensure_inline_barcode = True
        st.min_length = min_length
        if min_length == 20:
            records = pipeline_records(st, rec1, rec2, untrimmed_requested=True)
        else:  # (pipeline_records' cache does not know -m)
            rec1, rec2 = rec1[:257], rec2[:257]
            records = util.pyref_run(BUILDIN_ADAPTERS["TAKARAV3"], st, util.batch_from_records(rec1, rec2),
                                     [r[0] for r in rec1], [r[0] for r in rec2], True)
        _CACHE[key] = (st, records, rec1, rec2)
    return _CACHE[key]


def single_plan(min_length=20):
    """One 3' adapter that may match with a single base (cutadapt -O 1): over half of the fixture's reads lose at least
    their last base, so the median final length lies below the read length and -M at the median splits the reads."""
    return planmod.single_adapter_plan(ADAPTER, min_overlap=1, min_length=min_length)


def single_case(tmp_path_factory, min_length=20, extra=()):
    """One 3' adapter, single-end, on mate 1 of the fixture (``extra``: more (name, seq, qual) records behind it).
    -> (plan, records [(route, record, None)], the input records)"""
    key = ("single", min_length, len(extra))
    if key not in _CACHE:
        (rec1, _rec2), _paths = fixture_records(tmp_path_factory)
        rec = list(rec1) + list(extra)
        tp = single_plan(min_length)
        batch = util.batch_from_records(rec)
        (o1, cap2, _stats), _none = util.oracle_run(tp, batch, threads=8)
        _CACHE[key] = (util.format_batch(tp, batch, [r[0] for r in rec], None, o1, cap2, None), rec)
    records, rec = _CACHE[key]
    return single_plan(min_length), records, rec


def text_of(rec):
    return fastq_text([r[0] for r in rec], [r[1] for r in rec], [r[2] for r in rec])


def as_fasta(stream: bytes) -> bytes:
    lines = stream.split(b"\n")
    return b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))


def final_bases(stream: bytes) -> int:
    return sum(len(line) for line in stream.split(b"\n")[1::4])


# ---- kernel level ----------------------------------------------------------------------------------------------

def run_batch(eng, paired, rec1, rec2, stride=160, **kw):
    """One batch through a text engine with the fourth route -> (streams[route][mate] as fetched, sizes, text sizes,
    counts, result, discards)."""
    n = len(rec1)
    text1, text2 = text_of(rec1), (text_of(rec2) if paired else None)
    with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2 or b"")) + 1024, max_records=n,
                             stride=stride, too_long_route=True, **kw) as te:
        assert te.n_routes == 4
        te.submit(0, text1, len(text1), text2, len(text2) if paired else 0, n)
        res = te.wait(0)
        got, raw, count = te.routes(0)
        discards = te.discards(0)
        out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
        te.fetch(0, out[0], out[1] if paired else None)
    return textpath.split_routes(got, out, paired), got, raw, [int(c) for c in count], res, discards


def check_batch(eng, paired, records, rec1, rec2, max_length, compress=False, fasta_routes=0, stride=160):
    want, gone, _bits = toolong_rule.apply_rule(records, max_length=max_length)
    mates = 2 if paired else 1
    if fasta_routes:  # (the class-3 bits alone: the too-long records leave as FASTA, everything else as it was)
        assert fasta_routes == (0xC0 if paired else 0x40)
        want[3] = [as_fasta(want[3][0]), as_fasta(want[3][1])]
    streams, got, raw, count, res, discards = run_batch(eng, paired, rec1, rec2, stride=stride, compress=compress,
                                                        fasta_routes=fasta_routes)
    n = len(rec1)
    assert len(streams) == 4 and got.shape == (4, 2) and len(count) == 4
    for r in range(4):
        for m in range(mates):
            data = streams[r][m]
            assert len(data) == int(got[r][m])
            if compress:  # every stream a gzip member of its own; an empty route has no bytes, as ever
                assert (gzip.decompress(data) if data else b"") == want[r][m], (r, m)
                if data:
                    assert data[:3] == b"\x1f\x8b\x08"
                assert bool(data) == bool(want[r][m])
            else:
                assert data == want[r][m], (r, m)
            assert int(raw[r][m]) == len(want[r][m]), (r, m)
        assert count[r] == want[r][0].count(b"\n") // (2 if fasta_routes and r == 3 else 4), r
    for m in range(mates):
        assert int(res.out_bytes[m]) == sum(int(got[r][m]) for r in range(4))
        assert int(res.written_bp[m]) == final_bases(want[0][m])  # route 0 only
        for r in range(3):  # the summary keeps describing routes 0 .. 2
            assert int(res.route_bytes[r][m]) == int(got[r][m])
            assert int(res.text_bytes[r][m]) == (len(want[r][m]) if compress else 0)
    assert [int(res.route_count[r]) for r in range(3)] == count[:3]
    assert discards == (count[3], 0, 0) and count[3] == gone["too_long"]
    assert sum(count) == n
    return count


def paired_engine(st, max_length):
    tp = util.compile_plan(BUILDIN_ADAPTERS["TAKARAV3"], st, True, untrimmed_requested=True)
    tp.max_length = max_length
    return TrimEngine(tp, device=0, slots=0)


def single_engine(tp, max_length):
    tp.max_length = max_length
    return TrimEngine(tp, device=0, slots=0)


def test_the_rule_splits_the_fixture(tmp_path_factory):
    """-M at the median final length of the pairs TooShort leaves sends some pairs to stream 3 and not all."""
    _st, records, _r1, _r2 = paired_case(tmp_path_factory)
    want, gone, _ = toolong_rule.apply_rule(records, max_length=thresholds(records)[0])
    assert 0 < gone["too_long"] < len(records) - want[1][0].count(b"\n") // 4
    assert all(want[r][0] for r in (0, 1, 3))  # (TAKARAV3 has no inline barcode: nothing is untrimmed)
    _tp, srecords, _rec = single_case(tmp_path_factory)
    swant, sgone, _ = toolong_rule.apply_rule(srecords, max_length=thresholds(srecords)[0])
    assert 0 < sgone["too_long"] < len(srecords) - swant[1][0].count(b"\n") // 4


def test_paired_batches_at_the_scan_edges(tmp_path_factory):
    st, records, rec1, rec2 = paired_case(tmp_path_factory)
    max_length = thresholds(records)[0]
    seen = 0
    with paired_engine(st, max_length) as eng:
        for n in SIZES:
            seen += check_batch(eng, True, records[:n], rec1[:n], rec2[:n], max_length)[3]
    assert seen > 0


def test_single_end_batches_at_the_scan_edges(tmp_path_factory):
    tp, records, rec = single_case(tmp_path_factory)
    max_length = thresholds(records)[0]
    seen = 0
    with single_engine(tp, max_length) as eng:
        for n in SIZES:
            seen += check_batch(eng, False, records[:n], rec[:n], None, max_length)[3]
    assert seen > 0


@pytest.mark.parametrize("paired", [True, False])
def test_every_pair_too_long_and_none(tmp_path_factory, paired):
    """-M 0 with -m 0: streams 0 .. 2 are empty, the fourth holds the batch; -M huge: the fourth is empty."""
    n = 257
    if paired:
        st, records, rec1, rec2 = paired_case(tmp_path_factory, min_length=0)
        engine = lambda bound: paired_engine(st, bound)
    else:
        tp, records, rec1 = single_case(tmp_path_factory, min_length=0)
        rec2 = None
        engine = lambda bound: single_engine(tp, bound)
    records, rec1, rec2 = records[:n], rec1[:n], (rec2[:n] if paired else None)
    # (a read -- both reads of a pair -- trimmed to nothing is not longer than 0: such records stay where they were)
    empty = sum(1 for _rt, a, b in records if not a.split(b"\n")[1] and (b is None or not b.split(b"\n")[1]))
    with engine(0) as eng:
        count = check_batch(eng, paired, records, rec1, rec2, 0)
    assert count[3] == n - empty and count[3] > 0 and count[1] == 0
    if not empty:
        assert count[:3] == [0, 0, 0]
    with engine(HUGE) as eng:
        count = check_batch(eng, paired, records, rec1, rec2, HUGE)
    assert count[3] == 0 and sum(count[:3]) == n


@pytest.mark.parametrize("paired", [True, False])
def test_gzip_members_and_fasta_class_3(tmp_path_factory, paired):
    n = 257
    if paired:
        st, records, rec1, rec2 = paired_case(tmp_path_factory)
        max_length = thresholds(records)[0]
        eng = paired_engine(st, max_length)
    else:
        tp, records, rec1 = single_case(tmp_path_factory)
        rec2 = None
        max_length = thresholds(records)[0]
        eng = single_engine(tp, max_length)
    records, rec1, rec2 = records[:n], rec1[:n], (rec2[:n] if paired else None)
    with eng:
        count = check_batch(eng, paired, records, rec1, rec2, max_length, compress=True)
        assert count[3] > 0
        check_batch(eng, paired, records, rec1, rec2, max_length, fasta_routes=0xC0 if paired else 0x40)
        check_batch(eng, paired, records, rec1, rec2, max_length, compress=True, fasta_routes=0xC0 if paired else 0x40)


def test_reads_longer_than_the_rows_take_their_flags_from_the_long_read_kernel(tmp_path_factory):
    """Eight reads of 400 nt in rows of 160 bytes (the fixture's reads have 158 bases at most): four end in the adapter after 40 bases (not too long), four carry
    none (too long)."""
    rng = random.Random(11)
    extra = []
    for i in range(8):
        s = util.random_dna(rng, 400)
        if i % 2:
            s = (s[:40] + ADAPTER + s)[:400]
        extra.append((b"long%d" % i, s.encode(), bytes(rng.randint(40, 73) for _ in range(400))))
    tp, records, rec = single_case(tmp_path_factory, extra=tuple(extra))
    assert rec[-8:] == extra
    max_length = max(thresholds(records[:-8])[0], 60)
    keep = list(range(249)) + list(range(len(rec) - 8, len(rec)))  # 257 records, the long ones last
    records, rec = [records[i] for i in keep], [rec[i] for i in keep]
    finals = [len(a.split(b"\n")[1]) for _rt, a, _b in records[-8:]]
    assert sum(1 for f in finals if f > max_length) == 4 and sum(1 for f in finals if 20 <= f <= max_length) == 4
    with single_engine(tp, max_length) as eng:
        streams, _got, _raw, count, res, _disc = run_batch(eng, False, rec, None)
        assert int(res.n_long[0]) == 8
        assert streams[3][0].count(b"@long") == 4 and streams[0][0].count(b"@long") == 4
        check_batch(eng, False, records, rec, None, max_length)


def test_the_route_is_refused_without_max_length_and_with_bins(tmp_path_factory):
    tp = single_plan()
    with TrimEngine(tp, device=0, slots=0) as eng:  # no -M
        with pytest.raises(capi.CsError) as exc:
            textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 16, max_records=64, too_long_route=True)
        assert exc.value.code == abi.CS_ERR_ARG and "cs_plan_set_max_length" in str(exc.value)
        with pytest.raises(capi.CsError) as exc:  # ... and class 3 does not exist without the route
            textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 16, max_records=64, fasta_routes=0x40)
        assert exc.value.code == abi.CS_ERR_ARG
    from test_gpu_demux import barcode_set, scheme_with
    codes = barcode_set(random.Random(5), 4, 6, 3)
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    st.demux_barcodes = codes
    st.max_length = 50
    dtp = util.compile_plan(scheme_with(codes[0]), st, True)
    assert dtp.demux is not None and dtp.max_length == 50
    with TrimEngine(dtp, device=0, slots=0) as eng:
        with pytest.raises(capi.CsError) as exc:
            textpath.TextEngine(eng, slots=1, max_text_bytes=1 << 16, max_records=64, bins=4, too_long_route=True)
        assert exc.value.code == abi.CS_ERR_ARG and "n_bins" in str(exc.value)


# ---- the command line ------------------------------------------------------------------------------------------

def run_cli(tmp_path, capsys, tag, paths, extra, long_names=None):
    """-> ({(kind, mate): file text}, JSON report, stderr line); ``long_names``: the --too-long-output files."""
    from cutseq_amd import run as cli
    pre = str(tmp_path / tag)
    names = {"short": [f"{pre}_s{m}.fq.gz" for m in (1, 2)], "untrimmed": [f"{pre}_u{m}.fq.gz" for m in (1, 2)]}
    argv = paths + ["-A", "TAKARAV3", "-O", pre, "--json-file", pre + ".json"]
    if len(paths) == 2:
        argv += ["-s", *names["short"], "-u", *names["untrimmed"]]
    if long_names:
        argv += ["--too-long-output", *long_names]
    capsys.readouterr()
    cli.main(argv + extra)
    line = stderr_line(capsys.readouterr().err)
    rep = json.loads(open(pre + ".json").read())
    files = {}
    for m in (1, 2)[:len(paths)]:
        files[("trimmed", m)] = gunzip(f"{pre}_trimmed_R{m}.fastq.gz")
        if len(paths) == 2:
            files[("short", m)] = gunzip(names["short"][m - 1])
            files[("untrimmed", m)] = gunzip(names["untrimmed"][m - 1])
        else:
            files[("short", m)] = gunzip(f"{pre}_short_R{m}.fastq.gz")
        if long_names:
            name = long_names[m - 1]
            files[("too_long", m)] = gunzip(name) if name.endswith(".gz") else open(name, "rb").read()
    return files, rep, line


def strip_report(rep):
    rep = json.loads(json.dumps(rep))
    rep.pop("command_line_arguments")
    for key in ("too_long1", "too_long2"):
        rep["output"].pop(key, None)
    rep["engine"].pop("seconds")  # (the wall clock)
    return rep


def cli_case(tmp_path_factory):
    (rec1, rec2), paths = fixture_records(tmp_path_factory)
    st, records, _r1, _r2 = paired_case(tmp_path_factory)
    max_length, max_ee = thresholds(records)
    want, gone, pair_bits = toolong_rule.apply_rule(records, max_length, 0.0, max_ee)
    off, gone_off, _ = toolong_rule.apply_rule(records, max_length, 0.0, max_ee, too_long_route=False)
    # TooLong together with each other filter: the precedence decides what lands in the files
    for overlap in (3, 6, 7):
        assert overlap in pair_bits, overlap
    assert gone == gone_off and off[:3] == want[:3] and off[3] == [b"", b""] and all(want[3])
    assert all(gone[k] > 0 for k in toolong_rule.NAMES)
    extra = ["--ensure-inline-barcode", "-M", str(max_length), "--max-ee", repr(max_ee), "--max-n", "0"]
    return paths, want, gone, extra, len(rec1)


def check_files(files, want, tag, fasta_long=False):
    for r, kind in enumerate(("trimmed", "short", "untrimmed", "too_long")):
        for m in (1, 2):
            expect = want[r][m - 1]
            if fasta_long and kind == "too_long":
                expect = as_fasta(expect)
            assert files[(kind, m)] == expect, (tag, kind, m)


def check_counts(rep, line, gone, n):
    rc = rep["read_counts"]
    filtered = rc["filtered"]
    assert filtered["too_long"] == gone["too_long"] and filtered["too_many_n"] == gone["too_many_n"]
    assert filtered["too_many_expected_errors"] == gone["too_many_ee"]
    assert line["too_long"] == str(gone["too_long"]) and line["too_many_n"] == str(gone["too_many_n"])
    untrimmed = rep["engine"]["is_untrimmed_any"] or 0
    assert rc["input"] == n == rc["output"] + filtered["too_short"] + untrimmed + sum(gone.values())
    assert line["in_reads"] == str(n) and line["out_reads"] == str(rc["output"])


def test_cli_text_path_host_path_and_ranks(tmp_path, tmp_path_factory, monkeypatch, capsys):
    paths, want, gone, extra, n = cli_case(tmp_path_factory)
    _files, rep_off, line_off = run_cli(tmp_path, capsys, "off", paths, extra)
    results = []
    for tag, env, more in (("text", None, []), ("host", "0", []), ("ranks", None, ["--ranks", "2"])):
        if env is not None:
            monkeypatch.setenv("CUTSEQ_TEXT_PATH", env)
        else:
            monkeypatch.delenv("CUTSEQ_TEXT_PATH", raising=False)
        if tag == "ranks":
            monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
        long_names = [str(tmp_path / f"{tag}_long{m}.fq.gz") for m in (1, 2)]
        files, rep, line = run_cli(tmp_path, capsys, tag, paths, extra + more, long_names)
        monkeypatch.delenv("CUTSEQ_DEVICES", raising=False)
        check_files(files, want, tag)
        check_counts(rep, line, gone, n)
        assert rep["output"]["too_long1"] == long_names[0] and rep["output"]["too_long2"] == long_names[1]
        assert rep["basepair_counts"]["output_read1"] == final_bases(want[0][0])
        # the counts are those of the same run without the option
        assert rep["read_counts"] == rep_off["read_counts"] and rep["basepair_counts"] == rep_off["basepair_counts"]
        assert line == line_off
        results.append((rep["read_counts"], line))
    assert results[0] == results[1] == results[2]


def test_cli_many_batches_on_two_engines(tmp_path, tmp_path_factory, monkeypatch, capsys):
    paths, want, gone, extra, n = cli_case(tmp_path_factory)
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "300")
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    files, rep, line = run_cli(tmp_path, capsys, "many", paths, extra, [str(tmp_path / f"many_long{m}.fq.gz") for m in (1, 2)])
    check_files(files, want, "many")
    check_counts(rep, line, gone, n)


def test_cli_plain_fasta_files_beside_gz_fastq(tmp_path, tmp_path_factory, capsys):
    """Not every output is .gz: text comes back, the host deflates the .gz files, and the too-long files' own names
    make their records FASTA."""
    paths, want, gone, extra, n = cli_case(tmp_path_factory)
    files, rep, line = run_cli(tmp_path, capsys, "fa", paths, extra, [str(tmp_path / f"fa_long{m}.fa") for m in (1, 2)])
    check_files(files, want, "fa", fasta_long=True)
    check_counts(rep, line, gone, n)


@pytest.mark.parametrize("switch", ["", "CUTSEQ_TEXT_PATH=0"])
def test_cli_single_end_auto_rc_writes_the_records_turned_round(tmp_path, tmp_path_factory, monkeypatch, capsys, switch):
    (rec1, _rec2), paths = fixture_records(tmp_path_factory)
    st = planmod.CutadaptConfig()
    st.auto_rc = True
    records = pipeline_records(st, rec1, None)
    plain = pipeline_records(planmod.CutadaptConfig(), rec1, None)
    max_length = thresholds(records)[0]
    want, gone, _ = toolong_rule.apply_rule(records, max_length=max_length)
    unturned, _gone, _ = toolong_rule.apply_rule(plain, max_length=max_length)
    assert 0 < gone["too_long"] and want[3][0] != unturned[3][0]  # (a '-' library: the reads are turned round)
    assert sorted(len(l) for l in want[3][0].split(b"\n")[1::4]) == sorted(len(l) for l in unturned[3][0].split(b"\n")[1::4])
    if switch:
        monkeypatch.setenv(*switch.split("="))
    files, rep, line = run_cli(tmp_path, capsys, "rc", paths[:1], ["--auto-rc", "-M", str(max_length)],
                               [str(tmp_path / "rc_long.fq.gz")])
    assert files[("too_long", 1)] == want[3][0] and files[("trimmed", 1)] == want[0][0]
    assert files[("short", 1)] == want[1][0]
    assert rep["read_counts"]["filtered"]["too_long"] == gone["too_long"] and rep["output"]["too_long2"] is None


def test_cli_run_without_the_option_is_unchanged(tmp_path, tmp_path_factory, capsys):
    """-M with and without --too-long-output: the same trimmed / short / untrimmed files and the same report."""
    paths, want, gone, extra, n = cli_case(tmp_path_factory)
    # (both runs under one prefix, so that the reports name the same files; each run's files are read before the next)
    off, rep_off, line_off = run_cli(tmp_path, capsys, "same", paths, extra)
    on, rep_on, line_on = run_cli(tmp_path, capsys, "same", paths, extra, [str(tmp_path / f"with_long{m}.fq.gz") for m in (1, 2)])
    for key, data in off.items():
        assert on[key] == data, key
    check_files({**off, ("too_long", 1): want[3][0], ("too_long", 2): want[3][1]}, want, "without")
    assert "too_long1" not in rep_off["output"] and "too_long1" in rep_on["output"]
    assert strip_report(rep_on) == strip_report(rep_off)
    assert line_on == line_off
