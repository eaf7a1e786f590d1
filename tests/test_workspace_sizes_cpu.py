"""Every workspace size and plan entry point that needs no device context returns what it
returned before the workspaces were described by carve functions (csrc/nc_ws.h): the values in
tests/golden/workspace_sizes.json, recorded by tests/golden/make_workspace_sizes.py from this
project's own library at the commit before.  The carver itself is checked stand-alone under the
host sanitizers.  No GPU; only sizes are computed."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

from golden import make_workspace_sizes as W

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "workspace_sizes.json").read_text())


def _flat(v):
    return [x for e in v for x in _flat(e)] if isinstance(v, list) else [v]


def test_every_entry_point_and_every_input_is_recorded():
    rec = GOLDEN["context_free"]
    assert set(rec) == set(W.CALLS) and {n: [a for a, _ in c] for n, c in rec.items()} == W.inputs()
    for name, cases in rec.items():
        flat = _flat([a for a, _ in cases])
        assert {0, 1} <= set(flat), name                               # counts of 0 and 1
        lens = {len(a[-1]) for a, _ in cases if isinstance(a[-1], list)}
        assert not lens or {1, 2, 64} <= lens, name                    # per-file lists of 1, 2 and 64
        sizes = [max(_flat(v)) for _, v in cases]                      # a case's largest number: its total
        if name != "nc_bootstrap_job_bytes":                           # (no caller-sized count)
            assert max(sizes) > 1 << 32, name
        assert max(sizes) < 1 << 63, name                              # nothing recorded had wrapped


@pytest.mark.parametrize("name", sorted(W.CALLS))
def test_sizes_equal_the_recorded_ones(name):
    from nightcore_analyzer import _native
    lib = _native.load()
    bad = [(a, got, want) for a, want in GOLDEN["context_free"][name] for got in [W.CALLS[name](lib, *a)]
           if got != want]
    assert not bad, bad[:5]


def test_carver_under_sanitizers(tmp_path):
    """csrc/nc_ws.h with tests/ws_carve_main.cpp, host compiler only, ASan + UBSan: measure and
    carve modes agree, pointers respect their alignment, sections stay apart and inside the
    measured size, skip advances, and a wrapping count latches SIZE_MAX."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ws_carve_main"
    src = Path(__file__).resolve().parent / "ws_carve_main.cpp"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), str(src)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines()[-1] == "wraps latch SIZE_MAX"
