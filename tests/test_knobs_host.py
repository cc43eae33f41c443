"""The PH_* variables of the Python side (polyphonicformer_amd/knobs.py): one table, one reader, one documented list, and every
variable's meaning as it was before the table existed (tests/golden/knob_cfgs.json, recorded on the commit before it by
oracle/gen_golden_knobs.py).  Host only: no GPU, no library load."""
import json
import os
import re
import subprocess
import sys

import pytest

import helpers as Hh
from oracle import gen_golden_knobs as G
from polyphonicformer_amd import engine as E, knobs

PKG = os.path.join(Hh.REPO, "polyphonicformer_amd")


def test_no_module_but_knobs_reads_the_process_variables():
    """neither word, not even in a comment or inside a longer word"""
    seen = 0
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py") and os.path.join(root, f) != os.path.join(PKG, "knobs.py"):
                seen += 1
                with open(os.path.join(root, f)) as fh:
                    for no, line in enumerate(fh, 1):
                        assert "environ" not in line and "getenv" not in line, (f, no, line.strip())
    assert seen >= 20           # the walk found the package


def test_every_name_is_documented_and_the_printed_table_is_the_documented_one():
    with open(os.path.join(Hh.REPO, "DESIGN.md")) as f:
        doc = f.read()
    for name in knobs.KNOBS:
        assert f"`{name}`" in doc, name
    assert knobs.markdown() in doc          # DESIGN.md section 7g holds `python -m polyphonicformer_amd.knobs` as printed


def test_table_rows_are_well_formed():
    for name, k in knobs.KNOBS.items():
        assert k.name == name and re.fullmatch(r"PH_[A-Z0-9_]+", name)
        assert k.kind in ("flag", "int", "text", "raw") and k.effect in ("plan cfg", "import", "video", "build")
        assert k.doc and "\n" not in k.doc and k.reader
        assert {"flag": k.default is False, "int": k.default is None, "raw": k.default == ""}.get(k.kind, isinstance(k.default, str))


def test_unknown_name_raises_key_error():
    with pytest.raises(KeyError):
        knobs.get("PH_NO_SUCH_VARIABLE")
    with pytest.raises(KeyError):
        knobs.get("PH_CONV_WGS")            # a switch of the library, not a variable of this table


def test_get_parses_by_kind_at_the_time_of_the_call(monkeypatch):
    for name, k in knobs.KNOBS.items():
        monkeypatch.delenv(name, raising=False)
        assert knobs.get(name) == k.default and type(knobs.get(name)) is type(k.default)
        monkeypatch.setenv(name, "")
        assert knobs.get(name) == {"flag": False, "int": None}.get(k.kind, "")
        monkeypatch.setenv(name, " 7")
        assert knobs.get(name) == {"flag": True, "int": 7}.get(k.kind, " 7")
        monkeypatch.setenv(name, "0")
        assert knobs.get(name) == {"flag": True, "int": 0}.get(k.kind, "0")     # a flag is on when it is not empty
        os.environ[name] = "3"              # a direct write, as bench.py makes it, is seen as well
        assert knobs.get(name) == {"flag": True, "int": 3}.get(k.kind, "3")
        monkeypatch.delenv(name)


def test_bad_integer_raises_value_error_naming_the_variable(monkeypatch):
    Hh.clear_plan_knobs(monkeypatch)
    monkeypatch.setenv("PH_POOL_NSPLIT", "abc")
    calls = G.builders()
    for call in (calls["native_cfg"], calls["native_khead_cfg"], lambda: E.default_nsplit(2, 240)):
        with pytest.raises(ValueError, match="PH_POOL_NSPLIT"):
            call()
    # an explicit nsplit wins before the variable is parsed, as it always did
    assert calls["native_cfg(nsplit=5)"]().nsplit == 5 and calls["native_khead_cfg(nsplit=5)"]().nsplit == 5
    for name, k in knobs.KNOBS.items():
        if k.kind == "int":
            monkeypatch.setenv(name, "1.5")
            with pytest.raises(ValueError, match=name):
                knobs.get(name)


def test_default_nsplit_returns_the_variable_without_the_library(monkeypatch):
    monkeypatch.setenv("PH_POOL_NSPLIT", "6")
    assert E.default_nsplit(2, 240) == 6
    monkeypatch.setenv("PH_POOL_NSPLIT", "0")          # the known oddity (knobs.py): 0 comes back as 0 here, "the rule" in the cfgs
    assert E.default_nsplit(2, 240) == 0
    assert G.builders()["native_cfg"]().nsplit == 0


def test_every_value_means_what_it_meant_before_the_table():
    """the grid of oracle/gen_golden_knobs.py -- every variable a plan cfg is built from (and PH_VIDEO_SLOT_PRIO, which reaches
    none) x unset, "", "0", "1", "2", "3", "7", "x" (and "low") x the three builders plain and with each explicit argument that
    meets a variable -- gives the bytes, or raises the exception type, recorded on the commit before knobs.py"""
    assert set(G.VARIABLES) >= {k.name for k in knobs.KNOBS.values() if k.effect == "plan cfg"}
    assert set(G.VALUES) == {None, "", "0", "1", "2", "3", "7", "x"} and G.EXTRA_VALUES == {"PH_VIDEO_SLOT_PRIO": ("low",)}
    with open(G.PATH) as f:
        want = G.unpack(json.load(f))
    assert len(want) == len(G.builders()) * (len(G.VARIABLES) * len(G.VALUES) + 1) == 1134
    got = G.run_grid()
    assert [r[:3] for r in got] == [r[:3] for r in want]
    diff = [(g, w[3]) for g, w in zip(got, want) if g[3] != w[3]]
    assert not diff, (len(diff), diff[:5])
    # the record is not trivially constant: integers that do not parse raise, PH_NECK_OUT2=2 is refused, values change bytes
    by = {tuple(r[:3]): r[3] for r in want}
    assert by["native_cfg", "PH_POOL_NSPLIT", "x"] == by["native_khead_cfg", "PH_POOL_NSPLIT", "x"] == "ValueError"
    assert by["native_cfg", "PH_POOLX_NSPLIT", "x"] == by["native_cfg", "PH_UP2_SHARED_WGS", "x"] == "ValueError"
    assert by["native_neck_cfg", "PH_NECK_OUT2", "2"] == by["native_neck_cfg", "PH_NECK_OUT2", "3"] == "PolyheadError"
    assert by["native_khead_cfg(onepass=True)", "PH_KHEAD_TWOPASS", "0"] == "PolyheadError"
    for var in ("PH_CONV_POOLX", "PH_CONV_UP2"):                        # off, where supported, auto
        assert len({by["native_cfg", var, v] for v in ("0", "1", "2")}) == 3
    streams = [by["native_neck_cfg", "PH_NECK_STREAMS", v] for v in ("0", "1", "2")]
    assert streams[0] == streams[1] != streams[2]                       # B = 2: tower buffers only when always
    assert len({by["native_cfg", "PH_VIDEO_SLOT_PRIO", v] for v in G.VALUES + ("low",)}) == 1


_MODES = """
import importlib, json, os
os.environ.pop("PH_QUERY_FULL_SPLIT", None)
from polyphonicformer_amd import engine as E
out = [[E.MODES["fp16"].query, E.MODES["mixed16"].query]]
os.environ["PH_QUERY_FULL_SPLIT"] = "1"
out.append([E.MODES["fp16"].query, E.MODES["mixed16"].query])          # MODES is a constant: no change without a new import
importlib.reload(E)
out.append([E.MODES["fp16"].query, E.MODES["mixed16"].query])
print(json.dumps(out))
"""


def test_query_full_split_is_read_when_engine_is_imported():
    from polyphonicformer_amd import _lib
    r = subprocess.run([sys.executable, "-c", _MODES], cwd=Hh.REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    hybrid, split = [_lib.PH_PREC_QHYBRID] * 2, [_lib.PH_PREC_SPLIT] * 2
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [hybrid, hybrid, split]
