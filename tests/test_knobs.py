"""CPU: the table of HVN_* environment switches (hover_net_amd/knobs.py) against its two readers -- `knob` in the package,
csrc/hvn_env.h in the library -- and against INTEGRATION.md's section, which prints it."""
import glob
import os
import re

import pytest

from hover_net_amd import knobs, lib as L, tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hover_net_amd")
PY_FILES = sorted(glob.glob(os.path.join(PKG, "*.py")))
C_FILES = sorted(f for f in glob.glob(os.path.join(PKG, "csrc", "*")) if os.path.isfile(f))
NAME = r'"(HVN_[A-Z0-9_]+)"'


def read(path):
    return open(path, encoding="utf-8").read()


def test_table_is_what_the_two_readers_read():
    py = {m for f in PY_FILES if os.path.basename(f) != "knobs.py"      # every literal name inside the call's parentheses
          for call in re.findall(r"(?:\bknob\(|os\.environ(?:\.\w+\(|\[))([^()\[\]]*)", read(f)) for m in re.findall(NAME, call)}
    c = {m for f in C_FILES for m in re.findall(r"\bhvn_env_(?:int|str)\(\s*" + NAME, read(f))}
    assert py == set(knobs.PY_KNOBS)
    assert c == set(knobs.C_KNOBS)
    assert not py & c
    assert set(knobs.KNOBS) == py | c and len(knobs.KNOBS) == len(py) + len(c)
    for name, (default, meaning) in knobs.KNOBS.items():
        assert isinstance(default, str) and meaning, name
    assert tune.KNOBS is knobs.KNOBS and tune.knob is knobs.knob


def test_one_reader_per_language():
    assert [os.path.basename(f) for f in C_FILES if "getenv" in read(f)] == ["hvn_env.h"]
    # (knobs.py reads through the table, so not even it pairs os.environ with a literal name)
    assert [os.path.basename(f) for f in PY_FILES if re.search(r"os\.environ[^\n]*HVN_|getenv", read(f))] == []


def test_every_name_is_in_the_document():
    text = read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text[text.index("## 4. Environment switches"):]
    rows = dict(re.findall(r"^\| `(HVN_[A-Z0-9_]+)` \| (?:`([^`]*)`)? ?\|", section, flags=re.M))
    assert set(rows) == set(knobs.KNOBS)
    for name, (default, _) in knobs.KNOBS.items():
        assert rows[name] == default, name


def test_knob_reads_at_call_time_and_refuses_unknown_names(monkeypatch):
    with pytest.raises(KeyError):
        knobs.knob("HVN_NO_SUCH")
    monkeypatch.delenv("HVN_X3", raising=False)
    assert knobs.knob("HVN_X3") == "6"
    monkeypatch.setenv("HVN_X3", "9")
    assert knobs.knob("HVN_X3") == "9"
    monkeypatch.setenv("HVN_NO_SUCH", "1")
    with pytest.raises(KeyError):
        knobs.knob("HVN_NO_SUCH")


def test_library_variants():
    assert set(L.VARIANTS) == {"prev", "trace", "fullepi"}
