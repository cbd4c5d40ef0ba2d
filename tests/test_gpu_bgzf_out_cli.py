"""--bgzf on the command line: the same text and the same report as without it, every .gz output a BGZF file by the
rule (tests/bgzf_out_rule.py), the host writer's legs (CUTSEQ_GPU_DEFLATE=0, one plain output), an output without
records, and the round trip: the device inflater (CUTSEQ_GPU_INFLATE=1) reads what the device writer wrote.

The legs of a comparison write to the same file names, one after the other, so the reports name the same paths; the
wall time and the command line are taken out before reports are compared as text."""
import gzip
import json

import pytest

from cutseq_amd import codec, run as cli, textio

import bgzf_out_rule
import bgzf_rule
import util

pytestmark = pytest.mark.gpu
PLAN = ["-A", "TAKARAV3", "--trim-polyA"]
N = 2000
CHUNK = bgzf_out_rule.CHUNK
EOF = bgzf_rule.EOF_MARKER


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_in")
    paths = []
    for m in (1, 2):
        recs = util.read_fastq_gz(util.GOLDEN / f"fixture10k_R{m}.fq.gz")[:N]
        path = d / f"in_R{m}.fq"
        path.write_bytes(b"".join(b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + r[2] + b"\n" for r in recs))
        paths.append(str(path))
    return paths


@pytest.fixture(autouse=True)
def one_device(monkeypatch):
    monkeypatch.setenv("CUTSEQ_DEVICES", "0")
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "300")  # seven batches: the files are put together from parts
    monkeypatch.setenv("CUTSEQ_PROFILE", "1")
    monkeypatch.setattr(textio, "PROFILE", True)
    monkeypatch.delenv("CUTSEQ_GPU_INFLATE", raising=False)
    monkeypatch.delenv("CUTSEQ_GPU_DEFLATE", raising=False)


def raw(name):
    with open(name, "rb") as fh:
        return fh.read()


def text_of(name, data):
    return gzip.decompress(data) if name.endswith(".gz") else data


def leg(tmp_path, capfd, ins, names, bgzf, extra=()):
    """One run writing -o / -s to ``names`` -> ({name: file bytes}, the report as text, the profile's "inflate")."""
    pre = str(tmp_path / "out")
    k = len(ins)
    argv = list(ins) + PLAN + ["--json-file", pre + ".json", "-o", *names[:k], "-s", *names[k:2 * k]] + list(extra)
    capfd.readouterr()
    cli.main(argv + (["--bgzf"] if bgzf else []))
    err = capfd.readouterr().err
    profiles = [json.loads(line) for line in err.splitlines() if line.startswith('{"cutseq_profile"')]
    assert profiles, err[-2000:]
    inflate = {key: sum(p["inflate"][key] for p in profiles) for key in ("device_blocks", "host_blocks")}
    rep = json.loads(open(pre + ".json").read())
    assert "seconds" in rep["engine"] and "command_line_arguments" in rep
    rep["engine"]["seconds"] = rep["command_line_arguments"] = None
    return {n: raw(n) for n in names}, json.dumps(rep), inflate


def names_in(tmp_path, ext=".fq.gz", plain=()):
    return [str(tmp_path / f"out_{kind}{m}{'.fq' if (kind, m) in plain else ext}") for kind in ("o", "s") for m in (1, 2)]


def parts_of(blocks):
    """The text lengths of the batches a file was put together from, as its blocks tell them: a batch's last block is
    the one that is not full (a batch whose bytes are a multiple of CHUNK runs on into the next: the same chunking)."""
    parts, size = [], 0
    for b in blocks:
        isize = int.from_bytes(b[-4:], "little")
        size += isize
        if 0 < isize < CHUNK:
            parts.append(size)
            size = 0
    return parts + ([size] if size else [])


def check_bgzf_file(data, text, strict, what):
    blocks = bgzf_out_rule.split_blocks(data)
    assert blocks[-1] == EOF and data.count(EOF) == 1, what
    rows, end = codec.bgzf_index(data, 0, len(data))
    assert end == len(data) and len(rows) == len(blocks) and sum(r[2] for r in rows) == len(text), what
    assert all(len(b) <= bgzf_out_rule.MAX_BLOCK for b in blocks), what
    if strict:  # (the strict parser is Python: the whole rule on the files of one leg, the walk on all of them)
        bgzf_out_rule.check_file(data, text, parts=parts_of(blocks[:-1]), what=what)


def test_same_text_same_report_and_every_file_is_bgzf(tmp_path, capfd, inputs):
    names = names_in(tmp_path)
    plain = leg(tmp_path, capfd, inputs, names, False)
    blocked = leg(tmp_path, capfd, inputs, names, True)
    assert blocked[1] == plain[1]
    rep = json.loads(plain[1])
    assert rep["read_counts"]["input"] == N
    for n in names:
        text = gzip.decompress(plain[0][n])
        assert gzip.decompress(blocked[0][n]) == text, n
        assert plain[0][n][:4] == b"\x1f\x8b\x08\x00"  # without the option: the members they were
        check_bgzf_file(blocked[0][n], text, True, n)
    assert sum(gzip.decompress(d).count(b"\n") for d in blocked[0].values()) == 2 * 4 * N
    assert len(gzip.decompress(blocked[0][names[0]])) > 7 * CHUNK // 2  # several blocks a batch, several batches


def test_one_batch_is_the_chunks_of_the_text(tmp_path, capfd, inputs, monkeypatch):
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "2048")
    names = names_in(tmp_path)
    blocked = leg(tmp_path, capfd, inputs[:1], [names[0], names[2]], True)
    for n, data in blocked[0].items():
        bgzf_out_rule.check_file(data, gzip.decompress(data), what=n)  # (no parts: the file's own chunks, then the marker)


@pytest.mark.parametrize("how", ["host deflate", "one plain output"])
def test_the_host_writer_gives_the_same_text(tmp_path, capfd, inputs, monkeypatch, how):
    names = names_in(tmp_path)
    device = leg(tmp_path, capfd, inputs, names, True)
    if how == "host deflate":
        monkeypatch.setenv("CUTSEQ_GPU_DEFLATE", "0")
        host_names = names
    else:
        host_names = names_in(tmp_path, plain={("s", 2)})
    host = leg(tmp_path, capfd, inputs, host_names, True)
    for n, h in zip(names, host_names):
        text = gzip.decompress(device[0][n])
        assert text_of(h, host[0][h]) == text, h
        if h.endswith(".gz"):
            check_bgzf_file(host[0][h], text, False, h)
        else:
            assert not host[0][h].endswith(EOF)


def test_an_output_without_records_is_the_marker_alone(tmp_path, capfd, inputs):
    names = names_in(tmp_path)
    long_names = [str(tmp_path / f"long{m}.fq.gz") for m in (1, 2)]
    info = str(tmp_path / "info.tsv.gz")
    extra = ["-M", "100000", "--too-long-output", *long_names, "--info-file", info]
    plain = leg(tmp_path, capfd, inputs, names, False, extra)
    table = gzip.decompress(raw(info))
    blocked = leg(tmp_path, capfd, inputs, names, True, extra)
    assert blocked[1] == plain[1]
    for n in long_names:
        assert raw(n) == EOF
    # the info table is an output like the others
    assert gzip.decompress(raw(info)) == table and table.count(b"\n") >= N
    check_bgzf_file(raw(info), table, True, info)


def test_ranks_parts_are_concatenated_as_they_are(tmp_path, capfd, inputs, monkeypatch):
    """--ranks 2 on one device (the pattern of test_gpu_inflate_cli's ranks leg): every rank's part is a BGZF file of
    its own, the parts are joined as they are -- rank 0's marker stays as an empty block inside the file -- and the file's
    last 28 bytes are the marker."""
    names = names_in(tmp_path)
    one = leg(tmp_path, capfd, inputs, names, True)
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    two = leg(tmp_path, capfd, inputs, names, True, ["--ranks", "2"])
    assert json.loads(two[1])["engine"]["ranks"] == 2
    for n in names:
        text = gzip.decompress(one[0][n])
        data = two[0][n]
        assert gzip.decompress(data) == text, n
        blocks = bgzf_out_rule.split_blocks(data)
        assert data[-28:] == EOF and blocks.count(EOF) == 2, n
        rows, end = codec.bgzf_index(data, 0, len(data))
        assert end == len(data) and len(rows) == len(blocks)
        bgzf_out_rule.check_file(data, text, parts=parts_of(blocks), what=n)


def test_round_trip_through_the_device_inflater(tmp_path, capfd, inputs, monkeypatch):
    """The --bgzf outputs of one run are the inputs of the next: the device decoder on the device encoder's blocks
    (three deflate blocks a member) against the host's, outputs and report byte for byte."""
    first = tmp_path / "first"
    first.mkdir()
    names = names_in(first)
    leg(first, capfd, inputs, names, True)
    second_in = names[:2]
    second = tmp_path / "second"
    second.mkdir()
    out = [str(second / f"out_{kind}{m}.fq") for kind in ("o", "s") for m in (1, 2)]
    legs = []
    for on in ("1", "0"):
        monkeypatch.setenv("CUTSEQ_GPU_INFLATE", on)
        legs.append(leg(second, capfd, second_in, out, False))
    assert legs[0][0] == legs[1][0] and legs[0][1] == legs[1][1]
    assert legs[0][2]["device_blocks"] > 0 and legs[0][2]["host_blocks"] == 0
    assert legs[1][2]["device_blocks"] == 0
    assert json.loads(legs[0][1])["read_counts"]["input"] > N // 2
