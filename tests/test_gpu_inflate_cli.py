"""CUTSEQ_GPU_INFLATE on the command line: BGZF inputs inflated on the device give the files and the report of the
host path, byte for byte; runs outside the supported case take the host path silently; a corrupt file fails the same
way.  Which path ran comes from the CUTSEQ_PROFILE line ("inflate": device_blocks / host_blocks).

The two legs of a comparison write to the same file names, one after the other, so the reports name the same paths;
the one field that is a wall time (engine.seconds) is taken out before the reports are compared as text."""
import gzip
import json
import subprocess
import sys

import pytest

from cutseq_amd import run as cli, textio

import bgzf_rule
import util

pytestmark = pytest.mark.gpu
ROOT = str(util.GOLDEN.parents[1])
PLAN = ["-A", "TAKARAV3", "--trim-polyA"]
N = 3000


def _texts():
    rec1 = util.read_fastq_gz(util.GOLDEN / "fixture10k_R1.fq.gz")[:N]
    rec2 = util.read_fastq_gz(util.GOLDEN / "fixture10k_R2.fq.gz")[:N]
    def text(recs):
        return b"".join(b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + r[2] + b"\n" for r in recs)
    return text(rec1), text(rec2)


@pytest.fixture(scope="module")
def texts():
    return _texts()


@pytest.fixture(autouse=True)
def one_device_small_blocks(monkeypatch):
    monkeypatch.setenv("CUTSEQ_DEVICES", "0")
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "300")
    monkeypatch.setenv("CUTSEQ_PROFILE", "1")  # (child processes of --ranks sample it at import)
    monkeypatch.setattr(textio, "PROFILE", True)


def write_inputs(tmp_path, text1, text2, tail=b"", marker=True, plain_tail=False, r2_plain=False, blocks=(4093, 700), level=6):
    """R1 in 4 093-byte blocks, R2 in 700-byte blocks: the mates' spans and block boundaries never line up."""
    paths = []
    for name, text, block in (("in_R1.fq.gz", text1, blocks[0]), ("in_R2.fq.gz", text2, blocks[1])):
        if text is None:
            continue
        text = text[:-1] if tail is None else text + tail
        if name == "in_R2.fq.gz" and r2_plain:
            data = gzip.compress(text, 1)
        elif plain_tail:
            cut = len(text) * 2 // 3 + 5
            data = bgzf_rule.bgzf(text[:cut], block, 6) + gzip.compress(text[cut:], 1)
        else:
            data = bgzf_rule.bgzf(text, block, level) + (bgzf_rule.EOF_MARKER if marker else b"")
        path = tmp_path / name
        path.write_bytes(data)
        paths.append(str(path))
    return paths


def read(name):
    with open(name, "rb") as fh:
        data = fh.read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def leg(tmp_path, capfd, monkeypatch, on, inputs, extra=(), ext=".fq", outputs=None):
    """One run -> ({file name: text}, report text without the wall time, the profile line's "inflate")."""
    if on:
        monkeypatch.setenv("CUTSEQ_GPU_INFLATE", "1")
    else:
        monkeypatch.delenv("CUTSEQ_GPU_INFLATE", raising=False)
    pre = str(tmp_path / "out")
    names = outputs if outputs is not None else [f"{pre}_{kind}{m}{ext}" for kind in ("o", "s") for m in range(1, len(inputs) + 1)]
    argv = list(inputs) + PLAN + ["--json-file", pre + ".json"] + list(extra)
    if outputs is None:
        argv += ["-o", *names[:len(inputs)], "-s", *names[len(inputs):]]
    capfd.readouterr()
    cli.main(argv)
    err = capfd.readouterr().err
    profiles = [json.loads(line) for line in err.splitlines() if line.startswith('{"cutseq_profile"')]
    assert profiles, err[-2000:]
    inflate = {key: sum(p["inflate"][key] for p in profiles) for key in ("device_blocks", "host_blocks")}
    rep = json.loads(open(pre + ".json").read())
    assert "seconds" in rep["engine"]
    rep["engine"]["seconds"] = None
    return {n: read(n) for n in names}, json.dumps(rep), inflate


def both(tmp_path, capfd, monkeypatch, inputs, **kw):
    off = leg(tmp_path, capfd, monkeypatch, False, inputs, **kw)
    on = leg(tmp_path, capfd, monkeypatch, True, inputs, **kw)
    assert on[0] == off[0]
    assert on[1] == off[1]
    assert off[2]["device_blocks"] == 0
    return off, on


def test_paired_plain_outputs_and_report(tmp_path, capfd, monkeypatch, texts):
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, *texts))
    assert on[2]["device_blocks"] > 100 and on[2]["host_blocks"] == 0
    rep = json.loads(on[1])
    assert rep["read_counts"]["input"] == N
    assert sum(text.count(b"\n") for text in on[0].values()) == 2 * 4 * N  # every pair is in one of the two classes


def test_single_end(tmp_path, capfd, monkeypatch, texts):
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, texts[0], None))
    assert on[2]["device_blocks"] > 50


def test_gz_outputs(tmp_path, capfd, monkeypatch, texts):
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, *texts), ext=".fq.gz")
    assert on[2]["device_blocks"] > 100


def test_info_file_with_rename(tmp_path, capfd, monkeypatch, texts):
    info = str(tmp_path / "info.tsv")
    pre = str(tmp_path / "out")
    outputs = [f"{pre}_o1.fq", f"{pre}_o2.fq", f"{pre}_s1.fq", f"{pre}_s2.fq", info]
    extra = ["--info-file", info, "--rename", "{id}_{rn} {comment}", "-o", *outputs[:2], "-s", *outputs[2:4]]
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, *texts), extra=extra, outputs=outputs)
    assert on[2]["device_blocks"] > 100 and on[0][info].count(b"\n") >= N


@pytest.mark.parametrize("tail,marker", [(None, True), (b"\n\n\r\n", True), (b"@e\n\n+\n\n", True), (b"", False)],
                         ids=["no-final-newline", "blank-lines", "empty-last-read", "no-eof-marker"])
def test_end_of_file_variants(tmp_path, capfd, monkeypatch, texts, tail, marker):
    n = 1450  # (four whole blocks of 300 from the device, the rest through the host's end-of-input code)
    t1, t2 = (b"\n".join(t.split(b"\n")[:4 * n]) + b"\n" for t in texts)
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, t1, t2, tail=tail, marker=marker))
    assert on[2]["device_blocks"] > 50
    assert json.loads(on[1])["read_counts"]["input"] == n + (1 if tail and b"@e" in tail else 0)


def test_bgzf_followed_by_a_plain_member(tmp_path, capfd, monkeypatch, texts):
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, *texts, plain_tail=True))
    assert on[2]["device_blocks"] > 50 and on[2]["host_blocks"] > 0


def test_mates_decide_independently(tmp_path, capfd, monkeypatch, texts):
    """R1 is BGZF, R2 an ordinary gzip file: one text of a batch is on the device, the other comes from the host."""
    off, on = both(tmp_path, capfd, monkeypatch, write_inputs(tmp_path, *texts, r2_plain=True))
    assert on[2]["device_blocks"] > 50 and on[2]["host_blocks"] > 0


def test_marker_alone(tmp_path, capfd, monkeypatch):
    for name in ("in_R1.fq.gz", "in_R2.fq.gz"):
        (tmp_path / name).write_bytes(bgzf_rule.EOF_MARKER)
    off, on = both(tmp_path, capfd, monkeypatch, [str(tmp_path / "in_R1.fq.gz"), str(tmp_path / "in_R2.fq.gz")])
    assert json.loads(on[1])["read_counts"]["input"] == 0


# ---------------------------------------------------------------- outside the supported case: the host path, silently


def test_fallback_interleaved(tmp_path, capfd, monkeypatch, texts):
    import interleave_rule
    path = tmp_path / "woven.fq.gz"
    path.write_bytes(bgzf_rule.bgzf(interleave_rule.weave(*texts), 4093, 6) + bgzf_rule.EOF_MARKER)
    pre = str(tmp_path / "out")
    outputs = [f"{pre}_o.fq", f"{pre}_s.fq"]
    off, on = both(tmp_path, capfd, monkeypatch, [str(path)], extra=["--interleaved", "-o", outputs[0], "-s", outputs[1]],
                   outputs=outputs)
    assert on[2]["device_blocks"] == 0 and on[2]["host_blocks"] > 0


def test_fallback_fasta_in_bgzf(tmp_path, capfd, monkeypatch, texts):
    lines = texts[0].split(b"\n")
    fasta = b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))
    path = tmp_path / "in.fa.gz"
    path.write_bytes(bgzf_rule.bgzf(fasta, 4093, 6) + bgzf_rule.EOF_MARKER)
    pre = str(tmp_path / "out")
    outputs = [f"{pre}_o.fa", f"{pre}_s.fa"]
    off, on = both(tmp_path, capfd, monkeypatch, [str(path)], extra=["-o", outputs[0], "-s", outputs[1]], outputs=outputs)
    assert on[2]["device_blocks"] == 0 and len(on[0][outputs[0]]) > 0


def test_fallback_ranks(tmp_path, capfd, monkeypatch, texts):
    """(Stored blocks, the text eight times over: more than one 4 MB span of compressed bytes per file, so there is a
    member to enter in the middle and --ranks is not ignored.)"""
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    inputs = write_inputs(tmp_path, texts[0] * 8, texts[1] * 8, blocks=(65280, 65280), level=0)
    off, on = both(tmp_path, capfd, monkeypatch, inputs, extra=["--ranks", "2"])
    assert on[2]["device_blocks"] == 0 and json.loads(on[1])["engine"]["ranks"] == 2
    assert json.loads(on[1])["read_counts"]["input"] == 8 * N


def test_fallback_demux(tmp_path, capfd, monkeypatch, texts):
    import random
    from test_gpu_demux import barcode_set, scheme_with
    codes = barcode_set(random.Random(3), 4, 8, 4)
    table = tmp_path / "codes.tsv"
    table.write_text("".join(f"bc{i}\t{c}\n" for i, c in enumerate(codes)))
    inputs = write_inputs(tmp_path, *texts)
    pre = str(tmp_path / "dm")
    monkeypatch.setattr(sys.modules[__name__], "PLAN", ["-a", scheme_with(codes[0]), "--demux-barcodes", str(table)])
    import glob
    legs = []
    for on in (False, True):
        got = leg(tmp_path, capfd, monkeypatch, on, inputs, extra=["-O", pre], outputs=[])
        files = {n: read(n) for n in sorted(glob.glob(pre + "*.gz"))}
        legs.append((files, got[1], got[2]))
    assert legs[0][:2] == legs[1][:2] and len(legs[0][0]) >= 8
    assert legs[1][2]["device_blocks"] == 0 and legs[0][2]["device_blocks"] == 0


# ---------------------------------------------------------------- a corrupt file


def test_corrupt_block_fails_the_same_way(tmp_path, texts):
    from cutseq_amd import codec
    data = bytearray(bgzf_rule.bgzf(texts[0], 4093, 6) + bgzf_rule.EOF_MARKER)
    rows, _ = codec.bgzf_index(bytes(data), 0, len(data))
    data[rows[len(rows) // 2][0] + 100] ^= 0x04  # one payload bit of a middle block
    path = tmp_path / "bad.fq.gz"
    path.write_bytes(bytes(data))
    import os
    runs = []
    for on in ("0", "1"):
        env = dict(os.environ, CUTSEQ_GPU_INFLATE=on, CUTSEQ_PROGRESS="0")
        env.pop("CUTSEQ_PROFILE", None)
        r = subprocess.run([sys.executable, "-m", "cutseq_amd.run", str(path), *PLAN, "-o", str(tmp_path / "o.fq"), "-s",
                            str(tmp_path / "s.fq")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        messages = [line for line in r.stderr.splitlines() if "corrupt gzip data" in line]
        assert r.returncode != 0 and messages, r.stderr[-2000:]
        runs.append((r.returncode, messages[-1]))
    assert runs[0] == runs[1]
