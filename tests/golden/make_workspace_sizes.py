"""Record what the workspace size and plan entry points of libncgpu.so return.

    NCGPU_LIB=<the parent build's libncgpu.so> python tests/golden/make_workspace_sizes.py
    NCGPU_LIB=<the parent build's libncgpu.so> python tests/golden/make_workspace_sizes.py --context

The first form needs no GPU: every entry point it calls takes no context or ignores it, and only
sizes are computed, so nothing is allocated.  The second form needs one: it records the two
queries that read a live context's tables (``nc_window_stage_workspace_bytes`` and
``nc_ibi_tempogram_workspace_bytes``) under the key ``context_bound`` and leaves the rest of the
file as it is.  ``--out PATH`` writes somewhere else than ``tests/golden/workspace_sizes.json``.

The file holds recorded outputs of this project's own library, built from the commit before the
workspaces were described by carve functions (csrc/nc_ws.h); ``tests/test_workspace_sizes_cpu.py``
and ``tests/test_gpu_workspace_sizes.py`` replay it against the current build.  ``CALLS`` below is
the one place that knows how a recorded argument list is passed to each entry point.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "workspace_sizes.json"

# counts 0 and 1, then the counts at which a section of 8-, 4-, 2- and 1-byte elements is one
# element short of 256 bytes, exactly 256 bytes, and one element past
EDGE = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
FILES = [1, 2, 64]
BIG = 1 << 32                      # as a count of any element: a total above 2^32 bytes


def _i64(v):
    return np.asarray(v, np.int64)


# ----------------------------------------------------------------------------- callers
def _trim(lib, lens):
    a = _i64(lens)
    return int(lib.nc_trim_workspace_bytes(a.ctypes.data, len(lens)))


def _chroma_layout(lib, n, total):
    out = np.full(32, -7, np.int64)
    rc = int(lib.nc_chroma_workspace_layout(None, n, total, out.ctypes.data, len(out)))
    return [rc] + out[:max(rc, 0)].tolist()


def _limiter(lib, frames):
    a, off = _i64(frames), np.full(len(frames), -7, np.int64)
    return [int(lib.nc_limiter_ws_bytes(a.ctypes.data, len(frames), off.ctypes.data))] + off.tolist()


def _pv_plan(lib, p, n_in):
    n = len(n_in)
    a, ns, k, fb = _i64(n_in), np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(n + 1, -7, np.int64)
    off, size = np.full(6, -7, np.int64), C.c_size_t(7)
    rc = int(lib.nc_pv_plan(p, a.ctypes.data, n, ns.ctypes.data, k.ctypes.data, fb.ctypes.data, off.ctypes.data,
                            C.byref(size)))
    return [rc, ns.tolist(), k.tolist(), fb.tolist(), off.tolist(), int(size.value)]


# name -> call(lib, *recorded arguments) -> recorded value; no context needed
CALLS = {
    "nc_trim_workspace_bytes": _trim,
    "nc_tempo_beats_workspace_bytes": lambda lib, t: int(lib.nc_tempo_beats_workspace_bytes(t)),
    "nc_chroma_workspace_bytes": lambda lib, n, total: int(lib.nc_chroma_workspace_bytes(None, n, total)),
    "nc_chroma_workspace_layout": _chroma_layout,
    "nc_ibi_onset_workspace_bytes": lambda lib, n, t: int(lib.nc_ibi_onset_workspace_bytes(None, n, t)),
    "nc_ibi_range_workspace_bytes": lambda lib, n, t: int(lib.nc_ibi_range_workspace_bytes(None, n, t)),
    "nc_align_workspace_bytes": lambda lib, *a: int(lib.nc_align_workspace_bytes(None, *a)),
    "nc_spectral_workspace_bytes": lambda lib, *a: int(lib.nc_spectral_workspace_bytes(*a)),
    "nc_limiter_ws_bytes": _limiter,
    "nc_pv_plan": _pv_plan,
    "nc_pv_scan_ws_bytes": lambda lib, t, n: int(lib.nc_pv_scan_ws_bytes(t, n)),
    "nc_pv_lock_ws_bytes": lambda lib, t, n: int(lib.nc_pv_lock_ws_bytes(t, n)),
    "nc_bootstrap_job_bytes": lambda lib, cap, nb: int(lib.nc_bootstrap_job_bytes(cap, nb)),
}
# the same with a live context handle first
CONTEXT_CALLS = {
    "nc_window_stage_workspace_bytes": lambda lib, h, *a: int(lib.nc_window_stage_workspace_bytes(h, *a)),
    "nc_ibi_tempogram_workspace_bytes": lambda lib, h, *a: int(lib.nc_ibi_tempogram_workspace_bytes(h, *a)),
}


# ----------------------------------------------------------------------------- inputs
def _file_lists(values, big):
    """Per-file length lists of 1, 2 and 64 files (and none) over ``values``, one with ``big``."""
    out = [[]] + [[v] for v in values]
    out += [[a, b] for a, b in zip(values, values[1:] + values[:1])]
    out += [[values[(3 * i + j) % len(values)] for i in range(64)] for j in range(3)]
    return out + [[big], [1, big]]


def inputs():
    counts = EDGE + [BIG]
    per_file = [0, 1] + FILES[1:] + [31, 32, 33, 63, 65]         # 0, 1, 2, 64 files and the table edges
    frames = lambda k: (k - 1) * 512 if k > 0 else 0             # a trim file of k frames
    pv_len = [0, 1, 511, 512, 513, 2047, 2048, 2049, 22050, 3 * 22050 + 17]
    return {
        "nc_trim_workspace_bytes": [[l] for l in _file_lists(
            [0, 1, 511, 512, 513] + [frames(k) for k in EDGE[2:]], 1 << 40)],
        "nc_tempo_beats_workspace_bytes": [[t] for t in counts],
        "nc_chroma_workspace_bytes": [[n, t] for n in [0, 1, 2, 64] for t in counts + [441000 * n]],
        "nc_chroma_workspace_layout": [[n, t] for n in [0, 1, 2, 64] for t in counts + [441000 * n]] + [[1, -1]],
        "nc_ibi_onset_workspace_bytes": [[n, t] for n in per_file for t in counts],
        "nc_ibi_range_workspace_bytes": [[n, t] for n in per_file for t in counts],
        "nc_align_workspace_bytes": [
            [p, s, total, mx, lag]
            for p in [0, 1, 2, 64] for s in [1, 2, 30, 32, 33]
            for total, mx in [(0, 1), (1, 1), (2 * 63, 63), (2 * 64, 64), (2 * 65, 65), (1023, 513),
                              (2 * 512 * 32, 512 * 31), (2 * 512 * 33, 512 * 33), (10 * 441000, 441000),
                              (BIG * 4, BIG)]
            for lag in [0, 31, 32, 255]],
        "nc_spectral_workspace_bytes": [[t, n, min(t, mx)] for t in counts for n in [0] + FILES
                                        for mx in [0, 1, 32, 33, 8192, 8193]],
        "nc_limiter_ws_bytes": [[l] for l in _file_lists(
            [0, 1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, -5], 1 << 40)],
        "nc_pv_plan": [[p, l] for p in [500000, 943874, 1000000, 2000000] for l in _file_lists(pv_len, 1 << 40)]
                      + [[499999, [1]], [2000001, [1]], [1000000, [-1]], [1000000, [(1 << 40) + 1]]],
        "nc_pv_scan_ws_bytes": [[t, n] for t in counts + [-1] for n in [0] + FILES + [-1]],
        "nc_pv_lock_ws_bytes": [[t, n] for t in counts + [-1] for n in [0] + FILES + [-1]],
        "nc_bootstrap_job_bytes": [[cap, nb] for cap in EDGE + [1 << 20] for nb in [0, 1, 255, 256, 257, 5000]],
    }


def context_inputs():
    # hop 64 and hop 512 (the window stage launches only at 512; its query takes any hop)
    win = [[n, wl, hop] for hop in (64, 512) for n in [0, 1, 2, 64] for wl in [0, 1, hop * 31, hop * 63, 220500]]
    tg = [[n, t, min(t, mx), hop] for hop in (64, 512) for n in [0] + FILES for t in [0, 1, 31, 32, 33, 2048, 2049, 70000]
          for mx in [0, 1, 2048, 2049]]
    return {"nc_window_stage_workspace_bytes": win, "nc_ibi_tempogram_workspace_bytes": tg}


# ----------------------------------------------------------------------------- record
def record(lib):
    return {name: [[args, CALLS[name](lib, *args)] for args in cases] for name, cases in inputs().items()}


def record_context(lib, handle):
    return {name: [[args, CONTEXT_CALLS[name](lib, handle, *args)] for args in cases]
            for name, cases in context_inputs().items()}


def dump(doc, path):
    lines = []
    for key in ("context_free", "context_bound"):
        body = ",\n".join(f'  {json.dumps(name)}: [\n' + ",\n".join("   " + json.dumps(c, separators=(",", ":")) for c in cases)
                          + "\n  ]" for name, cases in doc.get(key, {}).items())
        lines.append(f' {json.dumps(key)}: {{\n{body}\n }}')
    Path(path).write_text("{\n" + ",\n".join(lines) + "\n}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--context", action="store_true", help="record the context-bound queries (needs a GPU)")
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    sys.path.insert(0, str(REPO / "nightcore-to-flac-analyzer_amd"))
    from nightcore_analyzer import _native
    lib = _native.load()
    doc = json.loads(OUT.read_text()) if OUT.exists() else {}
    if a.context:
        ctx = _native.Context(0)
        doc["context_bound"] = record_context(lib, ctx.h)
        ctx.close()
    else:
        doc["context_free"] = record(lib)
    dump(doc, a.out)
    print(f"{a.out}: {_native.lib_path()}:", {k: sum(len(c) for c in v.values()) for k, v in doc.items()}, "cases")


if __name__ == "__main__":
    main()
