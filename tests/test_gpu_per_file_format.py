"""Per-file output format on the GPU: FASTA and FASTQ streams in one run (``cs_text_params.fasta_routes``, reached from
the command line through the output files' names, as in the reference: cutseq/run.py:437-441, 449, 465, 754-758).

Expected bytes never come from the text path: they are the oracle's results formatted by the record logic
(``test_gpu_text.oracle_streams``, ``test_gpu_max_n.expect``), and a FASTA stream's records are re-shaped here:
``'>' + header line[1:] + '\\n' + sequence line + '\\n'``."""
import json
import random
import struct
import zlib

import numpy as np
import pytest

from cutseq_amd import abi, capi, plan as planmod, run as cli, synth, textpath
from cutseq_amd.common import BUILDIN_ADAPTERS, BarcodeConfig
from cutseq_amd.engine import TrimEngine

import maxn_rule
import util
from test_gpu_max_n import expect, gunzip, with_n
from test_gpu_text import fastq_text, oracle_streams

pytestmark = pytest.mark.gpu

# TAKARAV3 has no inline barcode, so nothing of it is ever "untrimmed": the cases that want three non-empty routes take
# this scheme (the one tests/test_gpu_cli.py uses for its untrimmed file) with --ensure-inline-barcode
INLINE = "ACACGACGCTCTTCCGATCT(GGG)NNN<XXXAGATCGGAAGAGCACACGTC"


def as_fasta(stream: bytes) -> bytes:
    lines = stream.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))


def shaped(want, mask, mates, fasta_out=False):
    """The oracle's FASTQ streams [route][mate] with the streams of ``mask`` as FASTA (routes from 3 on: class 3)."""
    return [[as_fasta(want[q][m]) if fasta_out or (mask >> (2 * min(q, 3) + m)) & 1 else want[q][m]
             for m in range(mates)] + [b""] * (2 - mates) for q in range(len(want))]


def inflate_member(data: bytes) -> bytes:
    """One gzip member, as zlib reads it; CRC-32 and ISIZE checked by hand."""
    assert data[:4] == b"\x1f\x8b\x08\x00"  # (no optional header fields: the body starts at byte 10)
    d = zlib.decompressobj(-15)
    text = d.decompress(data[10:])
    assert d.eof and len(d.unused_data) == 8, "more than one member, or a short trailer"
    crc, isize = struct.unpack("<II", d.unused_data)
    assert crc == zlib.crc32(text) and isize == len(text) & 0xFFFFFFFF
    return text


def run_engine(eng, text1, text2, n, stride, **kw):
    paired = text2 is not None
    with textpath.TextEngine(eng, slots=1, max_text_bytes=max(len(text1), len(text2 or b""), 1) + 1024,
                             max_records=max(n, 1), stride=stride, **kw) as te:
        te.submit(0, text1, len(text1), text2, len(text2) if paired else 0, n)
        res = te.wait(0)
        got, raw, count = te.routes(0)
        out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
        te.fetch(0, out[0], out[1] if paired else None)
        return res, textpath.split_routes(got if te.n_routes > 3 else res, out, paired), raw, [int(c) for c in count]


def check_streams(res, streams, want, counts, mates, compress, what):
    """Every stream equals ``want`` (already shaped), and the batch's sizes and counts agree with it."""
    for q in range(3):
        assert int(res.route_count[q]) == counts[q], what
        for m in range(mates):
            data = streams[q][m]
            assert int(res.route_bytes[q][m]) == len(data), (what, q, m)
            # text_bytes: the uncompressed size of a compressed stream; without compression the field is not used
            # (include/cutseq_hip.h: "compress = 1") and route_bytes itself is the size of the text
            assert int(res.text_bytes[q][m]) == (len(want[q][m]) if compress else 0), (what, q, m)
            if compress:
                data = inflate_member(data) if want[q][m] else data
            else:
                assert int(res.route_bytes[q][m]) == len(want[q][m]), (what, q, m)
            assert data == want[q][m], (what, textpath.ROUTES[q], m)
    for m in range(mates):
        assert int(res.out_bytes[m]) == sum(len(streams[q][m]) for q in range(3)), (what, m)
        lines = want[0][m].split(b"\n")
        step = 2 if want[0][m][:1] == b">" else 4
        assert int(res.written_bp[m]) == sum(len(l) for l in lines[1::step]), (what, m)


def fixture1k(min_length):
    rec1 = util.read_fastq_gz(util.GOLDEN / "fixture1k_R1.fq.gz")
    rec2 = util.read_fastq_gz(util.GOLDEN / "fixture1k_R2.fq.gz")
    batch = util.batch_from_records(rec1, rec2)
    st = planmod.CutadaptConfig()
    st.min_length = min_length
    st.ensure_inline_barcode = True
    return rec1, rec2, batch, st


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scheme", ["TAKARAV3", INLINE])
def test_engine_every_mask_paired(scheme, compress):
    """Paired, on fixture1k, all 64 masks of the six streams.  TAKARAV3 fills the trimmed and the too-short route (a
    scheme without an inline barcode has no untrimmed reads, whatever --min-length says); the inline scheme fills all
    three: an empty route proves nothing."""
    rec1, rec2, batch, st = fixture1k(60)
    tp = util.compile_plan(BUILDIN_ADAPTERS.get(scheme, scheme), st, True, untrimmed_requested=True)
    names1, names2 = [r[0] for r in rec1], [r[0] for r in rec2]
    want, counts, _ = oracle_streams(tp, batch, names1, names2)
    assert min(counts[:2]) > 0 and (counts[2] > 0 or scheme == "TAKARAV3"), counts
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2)
    with TrimEngine(tp, device=0, slots=0) as eng:
        for mask in range(64):
            res, streams, _raw, _count = run_engine(eng, text1, text2, batch.n, batch.stride, compress=compress,
                                                    fasta_routes=mask)
            check_streams(res, streams, shaped(want, mask, 2), counts, 2, compress, f"mask {mask:#04x}")
        # fasta_out = 0 with mask 0: all FASTQ; fasta_out = 1: all FASTA whatever the mask says
        for mask in (0, 0x15, 0x3F):
            res, streams, _raw, _count = run_engine(eng, text1, text2, batch.n, batch.stride, compress=compress,
                                                    fasta=True, fasta_routes=mask)
            check_streams(res, streams, shaped(want, 0, 2, fasta_out=True), counts, 2, compress, f"fasta_out, mask {mask:#04x}")
        with pytest.raises(capi.CsError) as exc:  # class 3 without bins
            run_engine(eng, text1, text2, batch.n, batch.stride, fasta_routes=0x40)
        assert exc.value.code == abi.CS_ERR_ARG


def test_engine_single_end_reverse_complement():
    """Single-end --auto-rc on a '-' library (the records leave reverse-complemented): the 8 masks of mate 1."""
    rec1 = util.read_fastq_gz(util.GOLDEN / "fixture1k_R1.fq.gz")
    batch = util.batch_from_records(rec1)
    scheme = INLINE
    st = planmod.CutadaptConfig()
    st.auto_rc = st.ensure_inline_barcode = st.trim_polyA = True
    st.min_length = 40
    tp = util.compile_plan(scheme, st, False, untrimmed_requested=True)
    assert tp.reverse_complement
    names1 = [r[0] for r in rec1]
    want, counts, _ = oracle_streams(tp, batch, names1, None)
    assert min(counts) > 0, counts
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    with TrimEngine(tp, device=0, slots=0) as eng:
        for compress in (False, True):
            for bits in range(8):
                mask = (bits & 1) | (bits & 2) << 1 | (bits & 4) << 2
                res, streams, _raw, _count = run_engine(eng, text1, None, batch.n, batch.stride, compress=compress,
                                                        fasta_routes=mask)
                check_streams(res, streams, shaped(want, mask, 1), counts, 1, compress, f"mask {mask:#04x}")
        for bad in (0x02, 0x08, 0x20):  # a bit of mate 2
            with pytest.raises(capi.CsError) as exc:
                run_engine(eng, text1, None, batch.n, batch.stride, fasta_routes=bad)
            assert exc.value.code == abi.CS_ERR_ARG


@pytest.mark.parametrize("compress,bin_mate", [(False, 0), (True, 1), (False, 1), (True, 0)])
def test_engine_demultiplexing_plan(compress, bin_mate):
    """Table-form demultiplexing: the class-3 bit of ONE mate, FASTQ short files, FASTA untrimmed file of the other mate.
    Expected as tests/test_gpu_text.py builds it for bins: the array API's results and barcode indices (held to the
    oracle by tests/test_gpu_demux.py), formatted by the record logic."""
    import hostfmt
    from test_gpu_demux import barcode_set, plant_barcodes, scheme_with
    rng = random.Random(78)
    codes = barcode_set(rng, 12, 8, 4)
    st = planmod.CutadaptConfig()
    st.trim_polyA = True
    st.min_length = 40
    st.demux_barcodes = codes
    n = 8_000
    batch = synth.generate_pairs(n, 150, scheme_with(codes[0]), seed=9, adapter_fraction=0.5)
    plant_barcodes(rng, batch, codes, 8)
    tp = planmod.compile_paired(BarcodeConfig(scheme_with(codes[0])), st)
    names1 = [s.encode() for s in synth.headers(n, 1)]
    names2 = [s.encode() for s in synth.headers(n, 2)]
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2)
    bc = np.empty(n, dtype=np.uint8)
    with TrimEngine(tp, device=0, slots=1, max_reads=n, max_stride=batch.stride) as eng:
        r1, _cap2, r2 = eng.submit(0, batch.seq1, batch.qual1, batch.len1, batch.seq2, batch.qual2, batch.len2, bc=bc)
        eng.wait(0)
    want = [[b"", b""] for _ in range(3 + len(codes))]
    want_counts = [0] * (3 + len(codes))
    for i in range(n):
        n1, n2 = int(batch.len1[i]), int(batch.len2[i])
        route, rec1, rec2 = hostfmt.format_pair(names1[i], batch.seq1[i, :n1].tobytes(), batch.qual1[i, :n1].tobytes(), r1[i],
                                                names2[i], batch.seq2[i, :n2].tobytes(), batch.qual2[i, :n2].tobytes(), r2[i], tp)
        if route == 0:
            route = 3 + int(bc[i])
        want[route][0] += rec1
        want[route][1] += rec2
        want_counts[route] += 1
    assert min(want_counts[1:]) > 0 and want_counts[0] == 0
    mask = 1 << (6 + bin_mate) | 1 << (4 + 1 - bin_mate)
    exp = shaped(want, mask, 2)
    with TrimEngine(tp, device=0, slots=0) as eng:
        res, streams, raw, count = run_engine(eng, text1, text2, n, batch.stride, compress=compress, bins=len(codes),
                                              fasta_routes=mask)
        with pytest.raises(capi.CsError) as exc:  # the same bit on a text engine without bins
            run_engine(eng, text1, text2, n, batch.stride, fasta_routes=mask)
        assert exc.value.code == abi.CS_ERR_ARG
    assert count == want_counts
    for q in range(3 + len(codes)):
        for m in range(2):
            data = streams[q][m]
            if compress:
                assert int(raw[q][m]) == len(exp[q][m])
                data = inflate_member(data) if exp[q][m] else data
            assert data == exp[q][m], (q, m)
        if q >= 3:  # each barcode's pair of streams: one FASTA, one FASTQ
            assert exp[q][bin_mate][:1] == b">" and exp[q][1 - bin_mate][:1] == b"@"


def test_engine_long_reads_and_max_n_discards():
    """Rows of 100 bases for reads of up to 150 (part of the batch is formatted from the long-read kernel's results,
    some pairs with one long mate), --max-n 0.02: a discarded pair appears in no stream of either format."""
    scheme = INLINE
    st = planmod.CutadaptConfig()
    st.min_length = 50
    st.ensure_inline_barcode = True
    n = 3000
    batch = with_n(synth.generate_pairs(n, 150, scheme, seed=5, poly_fraction=0.1, n_rate=0.02), seed=4)
    rng = np.random.default_rng(7)
    cut = rng.random(n) < 0.4  # ragged: a good part of the reads fits the rows
    batch.len1[cut] = rng.integers(0, 150, size=int(cut.sum())).astype(np.uint16)
    cut = rng.random(n) < 0.4
    batch.len2[cut] = rng.integers(0, 150, size=int(cut.sum())).astype(np.uint16)
    tp = util.compile_plan(scheme, st, True, untrimmed_requested=True)
    names1 = [f"SIM:{i}/1 1:N:0:X".encode() for i in range(n)]
    names2 = [f"SIM:{i}/2 2:N:0:X".encode() for i in range(n)]
    (o1, cap2, _), m2 = util.oracle_run(tp, batch, threads=8)
    recs = util.format_batch(tp, batch, names1, names2, o1, cap2, m2[0])
    x1, x2 = maxn_rule.xflags(batch.seq1, o1, 0.02), maxn_rule.xflags(batch.seq2, m2[0], 0.02)
    want, counts, gone = [[b"", b""] for _ in range(3)], [0, 0, 0], []
    for i, (rt, a, b) in enumerate(recs):
        if rt != 1 and (x1[i] | x2[i]):
            gone.append(i)
            continue
        want[rt][0] += a
        want[rt][1] += b
        counts[rt] += 1
    assert min(counts) > 0 and len(gone) > 20
    text1 = fastq_text(names1, batch.seq1, batch.qual1, batch.len1)
    text2 = fastq_text(names2, batch.seq2, batch.qual2, batch.len2)
    tp.max_n = 0.02
    with TrimEngine(tp, device=0, slots=0) as eng:
        for stride, mask in ((100, 0b100110), (100, 0b011001), (4, 0b010110), (batch.stride, 0b101001)):
            for compress in (False, True):
                res, streams, _raw, _count = run_engine(eng, text1, text2, n, stride, compress=compress, fasta_routes=mask)
                what = f"stride {stride}, mask {mask:#04x}, compress {compress}"
                assert int(res.n_long[0]) == int((batch.len1.astype(np.int64) > stride).sum()), what
                if stride == 100:
                    assert 0 < int(res.n_long[0]) < n
                assert int(res.n_too_many_n) == len(gone), what
                check_streams(res, streams, shaped(want, mask, 2), counts, 2, compress, what)
                if not compress:
                    everything = b"".join(s for row in streams for s in row)
                    for i in gone[:50]:
                        assert b"SIM:%d_" % i not in everything and b"SIM:%d\n" % i not in everything


# ---- the command line ------------------------------------------------------------------------------------------

R1 = str(util.GOLDEN / "fixture10k_R1.fq.gz")
R2 = str(util.GOLDEN / "fixture10k_R2.fq.gz")
COUNT_KEYS = ("read_counts", "basepair_counts")


def fixture10k(flags, untrimmed_requested=True):
    rec1, rec2 = util.read_fastq_gz(R1), util.read_fastq_gz(R2)
    st = planmod.CutadaptConfig()
    for k, v in flags.items():
        setattr(st, k, v)
    tp = util.compile_plan(INLINE, st, True, untrimmed_requested=untrimmed_requested)
    want, gone = expect(tp, rec1, rec2, None)
    assert gone == 0 and tp.swap_outputs == bool(flags.get("auto_rc"))
    return want


def read_out(path):
    return gunzip(path) if path.endswith(".gz") else open(path, "rb").read()


def run_named(tmp_path, tag, names, extra):
    """names: {"-o": [R1, R2], "-s": ..., "-u": ...} (file names inside tmp_path) -> ({flag: [bytes, bytes]}, report)."""
    argv = [R1, R2, "-a", INLINE, "--json-file", str(tmp_path / f"{tag}.json")] + extra
    paths = {}
    for flag, pair in names.items():
        paths[flag] = [str(tmp_path / f"{tag}_{n}") for n in pair]
        argv += [flag] + paths[flag]
    cli.main(argv)
    return {flag: [read_out(p) for p in pair] for flag, pair in paths.items()}, json.loads((tmp_path / f"{tag}.json").read_text())


def is_fasta(name):
    return name.split(".")[1] in ("fa", "fasta")


def check_cli(tmp_path, tag, names, extra, want, swap=False):
    """The run with ``names`` writes the oracle's records, every file in the shape its name asks for, and reports the
    counts of the same run under all-FASTQ names."""
    files, rep = run_named(tmp_path, tag, names, extra)
    for q, flag in enumerate(("-o", "-s", "-u")):
        for k in range(2):
            m = 1 - k if swap and flag == "-o" else k  # (the k-th -o file receives the other mate's records)
            exp = want[q][m]
            assert len(exp) > 0
            assert files[flag][k] == (as_fasta(exp) if is_fasta(names[flag][k]) else exp), (tag, flag, k)
    plain = {flag: [n.split(".")[0] + ".fq" + (".gz" if n.endswith(".gz") else "") for n in pair] for flag, pair in names.items()}
    _files, rep_fastq = run_named(tmp_path, tag + "_allfq", plain, extra)
    for key in COUNT_KEYS:
        assert rep[key] == rep_fastq[key], (tag, key)
    return files, rep


def test_cli_mixed_names_plain_and_gz(tmp_path):
    """(a) trimmed .fastq.gz, short .fa, untrimmed .fq: gzip and plain names, so text comes back and the host deflates."""
    want = fixture10k({"ensure_inline_barcode": True, "min_length": 60})
    check_cli(tmp_path, "a", {"-o": ["t1.fastq.gz", "t2.fastq.gz"], "-s": ["s1.fa", "s2.fa"], "-u": ["u1.fq", "u2.fq"]},
              ["--ensure-inline-barcode", "--min-length", "60"], want)


def test_cli_every_file_gz_device_compresses_a_mixed_run(tmp_path):
    """(b) every file .gz, R1 files FASTQ and R2 files FASTA: the device writes the gzip members of both shapes."""
    want = fixture10k({"ensure_inline_barcode": True, "min_length": 60})
    check_cli(tmp_path, "b", {"-o": ["t1.fq.gz", "t2.fa.gz"], "-s": ["s1.fastq.gz", "s2.fasta.gz"], "-u": ["u1.fq.gz", "u2.fa.gz"]},
              ["--ensure-inline-barcode", "--min-length", "60"], want)


def test_cli_auto_rc_swap_format_goes_with_the_file(tmp_path):
    """(c) paired --auto-rc on a '-' library: R2's trimmed records go to the first -o file, in THAT file's format."""
    want = fixture10k({"auto_rc": True, "ensure_inline_barcode": True, "min_length": 60})
    check_cli(tmp_path, "c", {"-o": ["first.fa", "second.fq"], "-s": ["s1.fq", "s2.fa"], "-u": ["u1.fq", "u2.fq"]},
              ["--auto-rc", "--ensure-inline-barcode", "--min-length", "60"], want, swap=True)


def test_cli_ranks_equal_one_process(tmp_path, monkeypatch):
    """(d) --ranks 2 writes what one process writes, byte for byte after decompression (and so the oracle's records)."""
    want = fixture10k({"ensure_inline_barcode": True, "min_length": 60})
    names = {"-o": ["t1.fq.gz", "t2.fa.gz"], "-s": ["s1.fa", "s2.fq"], "-u": ["u1.fasta.gz", "u2.fastq"]}
    extra = ["--ensure-inline-barcode", "--min-length", "60"]
    one, rep_one = check_cli(tmp_path, "d1", names, extra, want)
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    two, rep_two = run_named(tmp_path, "d2", names, extra + ["--ranks", "2"])
    assert two == one
    for key in COUNT_KEYS:
        assert rep_two[key] == rep_one[key], key
    assert not [p.name for p in tmp_path.iterdir() if ".part" in p.name]


def test_cli_fasta_input_with_a_fastq_named_output_fails_and_writes_nothing(tmp_path):
    """(f) dnaio's refusal, now with the file's name; no output file is created."""
    rec1 = util.read_fastq_gz(R1, limit=500)
    src = tmp_path / "in.fa"
    src.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _q in rec1))
    out, short = str(tmp_path / "o.fa"), str(tmp_path / "s.fq")
    from cutseq_amd import fastq as fastqmod
    with pytest.raises((fastqmod.FastqFormatError, SystemExit)) as exc:
        cli.main([str(src), "-A", "TAKARAV3", "-o", out, "-s", short])
    if isinstance(exc.value, SystemExit):
        assert exc.value.code not in (0, None)
    else:
        assert "Output format cannot be FASTQ since no quality values are available" in str(exc.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.fa"]
    # the same input with FASTA names everywhere runs
    cli.main([str(src), "-A", "TAKARAV3", "-o", out, "-s", str(tmp_path / "s.fasta")])
    assert open(out, "rb").read().startswith(b">")


def test_cli_fasta_input_error_names_the_file(tmp_path, caplog, capsys):
    src = tmp_path / "in.fa"
    src.write_bytes(b">r1\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    short = str(tmp_path / "s.fq")
    with pytest.raises(BaseException) as exc:
        cli.main([str(src), "-A", "TAKARAV3", "-o", str(tmp_path / "o.fa"), "-s", short])
    said = str(exc.value) + caplog.text + capsys.readouterr().err
    assert "Output format cannot be FASTQ since no quality values are available" in said and "s.fq" in said


def test_cli_demultiplexing_fasta_bins_fastq_short_files(tmp_path, monkeypatch):
    """(e) --demux-barcodes with FASTA bins and FASTQ short / untrimmed files, every file .gz.

    NOT a run a user of the command line can start: the CLI names the barcodes' files itself
    (<prefix>_<name>_trimmed_R<mate>.fastq.gz, no option changes that), so FASTA bins exist for callers of
    ``run_text_pipeline`` and of the C ABI only.  The test puts the FASTA names in where the CLI builds them
    (``resolve_args``); everything behind that point is the product's own path."""
    from test_gpu_demux import barcode_set, plant_barcodes, scheme_with
    rng = random.Random(21)
    count, n = 6, 9_000
    codes = barcode_set(rng, count, 8, 5)
    bnames = [f"bc{i}" for i in range(count)]
    batch = synth.generate_pairs(n, 150, scheme_with(codes[0]), seed=29)
    plant_barcodes(rng, batch, codes, 8)
    names1 = [f"SIM:{i} 1:N:0:X".encode() for i in range(n)]
    names2 = [f"SIM:{i} 2:N:0:X".encode() for i in range(n)]
    in1, in2 = str(tmp_path / "d_R1.fastq.gz"), str(tmp_path / "d_R2.fastq.gz")
    util.write_fastq(in1, names1, batch.seq1, batch.qual1, batch.len1)
    util.write_fastq(in2, names2, batch.seq2, batch.qual2, batch.len2)
    table = tmp_path / "barcodes.tsv"
    table.write_text("".join(f"{a}\t{b}\n" for a, b in zip(bnames, codes)))
    # expected as tests/test_gpu_max_n.py::test_cli_demultiplexing_run builds it: one --ensure-inline-barcode run of the
    # oracle per barcode; a pair takes the intervals of the run whose barcode it carries
    st = planmod.CutadaptConfig()
    st.ensure_inline_barcode = True
    runs = []
    for code in codes:
        one = planmod.compile_paired(BarcodeConfig(scheme_with(code)), st)
        (o1, _, _), (o2, _, _) = util.oracle_run(one, batch, threads=8)
        runs.append((o1, o2, util.format_batch(one, batch, names1, names2, o1, None, o2)))
    want_bins = [[b"", b""] for _ in range(count)]
    want_short = [b"", b""]
    for i in range(n):
        hits = [b for b in range(count) if runs[b][0][i]["flags"] & abi.CS_F_INLINE]
        src = hits[0] if hits else count - 1
        o1, o2, recs = runs[src]
        rt = maxn_rule.route(int(o1[i]["flags"]), int(o2[i]["flags"]), 0, 0, True)
        if rt == 0:
            want_bins[src][0] += recs[i][1]
            want_bins[src][1] += recs[i][2]
        elif rt == 1:
            want_short[0] += recs[i][1]
            want_short[1] += recs[i][2]
    assert all(a for a, _b in want_bins) and want_short[0]

    def run(tag, fasta_bins):
        prefix = str(tmp_path / tag)
        real = cli.resolve_args

        def resolve(args):
            args = real(args)
            if fasta_bins:
                args.outputs = args.outputs.with_rank_names({
                    key: [p.replace(".fastq.gz", ".fa.gz") for p in pair]
                    for key, pair in args.outputs.rank_groups().items() if key.startswith("demux_files:")})
            return args

        monkeypatch.setattr(cli, "resolve_args", resolve)
        try:
            cli.main(["-a", scheme_with(codes[0]), "--demux-barcodes", str(table), "-O", prefix, "--json-file",
                      prefix + ".json", in1, in2])
        finally:
            monkeypatch.setattr(cli, "resolve_args", real)
        return prefix, json.loads(open(prefix + ".json").read())

    prefix, rep = run("dm", True)
    for b, name in enumerate(bnames):
        for m in (0, 1):
            assert gunzip(f"{prefix}_{name}_trimmed_R{m + 1}.fa.gz") == as_fasta(want_bins[b][m]), (name, m)
    for m in (0, 1):
        assert gunzip(f"{prefix}_short_R{m + 1}.fastq.gz") == want_short[m]
        assert gunzip(f"{prefix}_untrimmed_R{m + 1}.fastq.gz")[:1] == b"@"
    _prefix, rep_fastq = run("dq", False)
    for key in COUNT_KEYS + ("engine",):
        a, b = rep[key], rep_fastq[key]
        if key == "engine":
            a, b = a["demultiplexed"], b["demultiplexed"]
        assert a == b, key
