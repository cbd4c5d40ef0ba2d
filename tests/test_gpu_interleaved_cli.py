"""--interleaved on the command line.  The 1000-pair fixture is woven into one file by tests/interleave_rule.py; every
expected file is the two-file run's own file (interleaved input, split output) or the rule applied to the two-file
run's files (interleaved output)."""
import gzip
import json
import subprocess
import sys

import pytest

from cutseq_amd import run as cli

import interleave_rule
import util
from test_gpu_filters_cli import gunzip, stderr_line

pytestmark = pytest.mark.gpu

R1 = str(util.GOLDEN / "fixture1k_R1.fq.gz")
R2 = str(util.GOLDEN / "fixture1k_R2.fq.gz")
ROOT = str(util.GOLDEN.parents[1])
CLASSES = (("trimmed", "-o"), ("short", "-s"), ("untrimmed", "-u"))
PLAN = ["-A", "TAKARAV3", "--ensure-inline-barcode"]

_CACHE = {}


def read(name):
    return gunzip(name) if name.endswith(".gz") else open(name, "rb").read()


def run(tmp_path, capsys, tag, inputs, extra=(), split=True, ext=".fq.gz", plan=PLAN):
    """One in-process run -> ({class: [file text per output file]}, JSON report, stderr line, {class: names})."""
    pre = str(tmp_path / tag)
    names = {kind: [f"{pre}_{kind}{m}{ext}" for m in ((1, 2) if split else (0,))] for kind, _ in CLASSES}
    argv = list(inputs) + plan + ["--json-file", pre + ".json"]
    for kind, flag in CLASSES:
        argv += [flag, *names[kind]]
    capsys.readouterr()
    cli.main(argv + list(extra))
    line = stderr_line(capsys.readouterr().err)
    rep = json.loads(open(pre + ".json").read())
    return {kind: [read(n) for n in names[kind]] for kind, _ in CLASSES}, rep, line, names


def two_file(tmp_path_factory, capsys):
    """The two-file run of the fixture, once: the reference of every test below."""
    if "two" not in _CACHE:
        _CACHE["two"] = run(tmp_path_factory.mktemp("two_file"), capsys, "two", [R1, R2])
        files = _CACHE["two"][0]
        assert files["trimmed"][0] and files["short"][0] and files["trimmed"][0].count(b"\n") % 4 == 0
    return _CACHE["two"]


def woven_input(tmp_path, gz=False):
    data = interleave_rule.weave(gunzip(R1), gunzip(R2))
    path = tmp_path / ("woven.fq.gz" if gz else "woven.fq")
    path.write_bytes(gzip.compress(data, 1) if gz else data)
    return str(path)


def counts(rep):
    return rep["read_counts"], rep["basepair_counts"]


@pytest.mark.parametrize("ext", [".fq", ".fq.gz"])
def test_interleaved_in_split_out_is_the_two_file_run(tmp_path, tmp_path_factory, capsys, ext):
    want, want_rep, want_line, _ = two_file(tmp_path_factory, capsys)
    path = woven_input(tmp_path, gz=ext.endswith(".gz"))
    files, rep, line, names = run(tmp_path, capsys, "split", [path, "--interleaved"], ext=ext)
    assert files == want
    assert line == want_line and counts(rep) == counts(want_rep)
    assert rep["input"] == {"path1": path, "path2": None, "paired": True, "interleaved": True}
    assert want_rep["input"] == {"path1": R1, "path2": R2, "paired": True, "interleaved": False}
    assert rep["output"]["output1"] == names["trimmed"][0] and rep["output"]["output2"] == names["trimmed"][1]


@pytest.mark.parametrize("ext", [".fq", ".fq.gz"])
def test_two_files_in_one_file_per_class_out(tmp_path, tmp_path_factory, capsys, ext):
    want, want_rep, want_line, _ = two_file(tmp_path_factory, capsys)
    files, rep, line, names = run(tmp_path, capsys, "woven", [R1, R2, "--interleaved"], split=False, ext=ext)
    for kind, _ in CLASSES:
        assert files[kind] == [interleave_rule.weave(*want[kind])], kind
    assert line == want_line and counts(rep) == counts(want_rep)
    assert rep["input"] == {"path1": R1, "path2": R2, "paired": True, "interleaved": False}
    out = rep["output"]
    assert (out["output1"], out["output2"]) == (names["trimmed"][0], None)
    assert (out["short1"], out["short2"]) == (names["short"][0], None)
    if ext.endswith(".gz"):  # the device's members: one file, both mates
        assert open(names["trimmed"][0], "rb").read()[:3] == b"\x1f\x8b\x08"


def test_interleaved_both_ways_in_small_blocks_on_two_engines(tmp_path, tmp_path_factory, capsys, monkeypatch):
    want, want_rep, want_line, _ = two_file(tmp_path_factory, capsys)
    monkeypatch.setenv("CUTSEQ_CHUNK_READS", "300")
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    files, rep, line, _ = run(tmp_path, capsys, "both", [woven_input(tmp_path, gz=True), "--interleaved"], split=False)
    for kind, _ in CLASSES:
        assert files[kind] == [interleave_rule.weave(*want[kind])], kind
    assert line == want_line and counts(rep) == counts(want_rep)


def test_through_a_pipe_on_both_ends(tmp_path, tmp_path_factory, capsys):
    want = two_file(tmp_path_factory, capsys)[0]
    data = interleave_rule.weave(gunzip(R1), gunzip(R2))
    short = str(tmp_path / "short.fq")
    r = subprocess.run([sys.executable, "-m", "cutseq_amd.run", "-", "--interleaved", *PLAN, "-o", "-", "-s", short,
                        "-u", str(tmp_path / "untrimmed.fq")], input=data, capture_output=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout == interleave_rule.weave(*want["trimmed"])
    assert open(short, "rb").read() == interleave_rule.weave(*want["short"])


def test_auto_rc_on_a_minus_library_leads_with_mate_2(tmp_path, capsys):
    """Two files change names (mate 2's trimmed records are the first -o file's); one file cannot, so mate 2's record comes
    first in it -- in every class of the run, so that one rule reads all of its files."""
    two, two_rep, two_line, _ = run(tmp_path, capsys, "rc2", [R1, R2], extra=["--auto-rc"])
    files, rep, line, _ = run(tmp_path, capsys, "rc1", [R1, R2, "--interleaved"], extra=["--auto-rc"], split=False)
    assert two["trimmed"][0] != two["trimmed"][1]
    # the first -o file of the two-file run holds mate 2: the rule applied to the files as they are
    assert files["trimmed"] == [interleave_rule.weave(*two["trimmed"])]
    mate1_first = gunzip(R1).split(b"\n")[0].split()[0]
    first, second = files["trimmed"][0].split(b"\n")[0], files["trimmed"][0].split(b"\n")[4]
    assert first.split(b"_")[0] == second.split(b"_")[0]  # one pair: the same id, the UMI behind it
    assert mate1_first.startswith(b"@")
    # the too-short files are not swapped in a two-file run: mate 2 first means the rule with the mates exchanged
    assert files["short"] == [interleave_rule.weave(*two["short"], mate2_first=True)]
    assert line == two_line and counts(rep) == counts(two_rep)


def test_info_file_with_interleaved_input_is_about_read_1(tmp_path, capsys):
    info = [str(tmp_path / "two.tsv"), str(tmp_path / "one.tsv.gz")]
    run(tmp_path, capsys, "i2", [R1, R2], extra=["--info-file", info[0]])
    run(tmp_path, capsys, "i1", [woven_input(tmp_path), "--interleaved"], extra=["--info-file", info[1]], split=False)
    table = read(info[0])
    assert table.count(b"\n") >= 1000 and read(info[1]) == table


def test_interleaved_output_under_ranks(tmp_path, tmp_path_factory, capsys, monkeypatch):
    want, want_rep, want_line, _ = two_file(tmp_path_factory, capsys)
    monkeypatch.setenv("CUTSEQ_DEVICES", "0,0")
    plain = [str(tmp_path / f"in{m}.fq") for m in (1, 2)]  # (a one-member gzip file cannot be entered in the middle)
    for name, src in zip(plain, (R1, R2)):
        open(name, "wb").write(gunzip(src))
    files, rep, line, _ = run(tmp_path, capsys, "ranks", plain + ["--interleaved"], extra=["--ranks", "2"], split=False)
    for kind, _ in CLASSES:
        assert files[kind] == [interleave_rule.weave(*want[kind])], kind
    assert counts(rep) == counts(want_rep) and rep["engine"].get("ranks") == 2


def test_interleaved_input_under_ranks_is_refused(tmp_path, caplog):
    with pytest.raises(SystemExit) as exc:
        cli.main([woven_input(tmp_path), "--interleaved", *PLAN, "-O", str(tmp_path / "o"), "--ranks", "2"])
    assert exc.value.code == 1 and "--interleaved input cannot be split between --ranks" in caplog.text


def test_an_odd_record_count_ends_the_run(tmp_path):
    data = interleave_rule.weave(gunzip(R1), gunzip(R2))
    odd = tmp_path / "odd.fq"
    odd.write_bytes(b"".join(interleave_rule._records(data, 4)[:-1]))  # mate 2 of the last pair is gone
    r = subprocess.run([sys.executable, "-m", "cutseq_amd.run", str(odd), "--interleaved", *PLAN, "-O", str(tmp_path / "o")],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0
    assert "interleaved input is incomplete" in r.stderr and "no partner" in r.stderr
