"""The environment switches: one table (cutseq_amd/switches.py), one reader per layer, and documents that name them all."""
import re
from pathlib import Path

import pytest

from cutseq_amd import switches

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "cutseq_amd"
SOURCE_SUFFIXES = (".py", ".hip", ".hip.inc", ".c", ".h")
TABLE = {s.name: s for s in switches.TABLE}
NATIVE = {name for name, s in TABLE.items() if s.reader in ("native", "both")}


def sources(folder: Path):
    return sorted(p for p in folder.rglob("*") if p.is_file() and p.name.endswith(SOURCE_SUFFIXES))


def test_the_table_is_the_list_of_names_in_the_package():
    assert len(TABLE) == len(switches.TABLE)  # no name twice
    found = {}
    for path in sources(PKG):
        for line in path.read_text().splitlines():
            if re.match(r"\s*#\s*(ifndef|define|endif)\b.*_H\b", line):  # include guards
                continue
            for name in re.findall(r"CUTSEQ_[A-Z0-9_]+", line):
                found.setdefault(name, path.name)
    assert {n: f for n, f in found.items() if n not in TABLE} == {}  # named in the code, missing from the table
    assert set(TABLE) - set(found) == set()  # in the table, named nowhere
    for s in switches.TABLE:
        assert s.kind in (switches.FLAG_ON, switches.FLAG_OFF, switches.INT, switches.DEVICES, switches.PATH), s
        assert s.reader in ("python", "native", "both") and s.meaning, s


def test_the_library_reads_each_native_switch_in_one_place():
    names = []
    for path in sources(PKG / "csrc"):
        text = path.read_text()
        assert len(re.findall(r"getenv\s*\(", text)) == len(re.findall(r'getenv\s*\(\s*"CUTSEQ_[A-Z0-9_]+"\s*\)', text)), path.name
        names += re.findall(r'getenv\s*\(\s*"(CUTSEQ_[A-Z0-9_]+)"', text)
    assert sorted(names) == sorted(NATIVE)  # every call names a native entry, every native entry has exactly one call


def test_python_modules_read_switches_through_the_table_only():
    for path in sources(PKG):
        if path.suffix != ".py" or path.name == "switches.py":
            continue
        text = path.read_text()
        assert 'environ.get("CUTSEQ_' not in text and 'getenv("CUTSEQ_' not in text, path.name


def test_integration_md_names_every_switch():
    text = (ROOT / "INTEGRATION.md").read_text()
    assert [name for name in TABLE if f"`{name}" not in text] == []


def key_of(kind, reader=("python", "both")):
    return next(s.name[len(switches.PREFIX):] for s in switches.TABLE if s.kind == kind and s.reader in reader)


@pytest.mark.parametrize("kind", [switches.FLAG_ON, switches.FLAG_OFF])
def test_flag_accessor(kind, monkeypatch):
    for key in [s.name[len(switches.PREFIX):] for s in switches.TABLE if s.kind == kind and s.reader != "native"]:
        name = switches.PREFIX + key
        monkeypatch.delenv(name, raising=False)
        assert switches.enabled(key) is TABLE[name].default is (kind == switches.FLAG_ON)
        monkeypatch.setenv(name, "0")
        assert switches.enabled(key) is False
        monkeypatch.setenv(name, "1")
        assert switches.enabled(key) is True
        monkeypatch.setenv(name, "00")  # string comparison, not the library's atoi: only "0" / "1" flip a flag
        assert switches.enabled(key) is TABLE[name].default
        monkeypatch.delenv(name)


def test_int_accessor(monkeypatch):
    key = key_of(switches.INT)
    name = switches.PREFIX + key
    monkeypatch.delenv(name, raising=False)
    assert switches.int_value(key) is TABLE[name].default
    monkeypatch.setenv(name, "0")
    assert switches.int_value(key) == 0
    monkeypatch.setenv(name, "1")
    assert switches.int_value(key) == 1
    monkeypatch.setenv(name, "65536")
    assert switches.int_value(key) == 65536
    monkeypatch.setenv(name, "many")
    with pytest.raises(ValueError):
        switches.int_value(key)


def test_device_list_accessor(monkeypatch):
    key = key_of(switches.DEVICES)
    name = switches.PREFIX + key
    monkeypatch.delenv(name, raising=False)
    assert TABLE[name].default is None and switches.device_list(key, 3) == [0, 1, 2]  # default: every device
    monkeypatch.setenv(name, "0")
    assert switches.device_list(key, 3) == [0]
    monkeypatch.setenv(name, "1")
    assert switches.device_list(key, 3) == [1]
    monkeypatch.setenv(name, "0,0")
    assert switches.device_list(key, 3) == [0, 0]
    monkeypatch.setenv(name, "0,x")
    with pytest.raises(ValueError):
        switches.device_list(key, 3)


def test_path_accessor(monkeypatch):
    key = key_of(switches.PATH)
    name = switches.PREFIX + key
    monkeypatch.delenv(name, raising=False)
    assert TABLE[name].default is None and switches.path(key, "/own/lib.so") == "/own/lib.so"  # default: the caller's own
    for value in ("0", "1", "/other/lib.so"):
        monkeypatch.setenv(name, value)
        assert switches.path(key, "/own/lib.so") == value


def test_accessors_refuse_the_wrong_kind_and_the_library_s_switches():
    with pytest.raises(TypeError):
        switches.enabled(key_of(switches.INT))
    with pytest.raises(TypeError):
        switches.int_value(key_of(switches.FLAG_ON))
    with pytest.raises(TypeError):
        switches.enabled(key_of(switches.FLAG_ON, reader=("native",)))  # (atoi there, strings here: not the same parse)
    with pytest.raises(KeyError):
        switches.enabled("NO_SUCH_SWITCH")
