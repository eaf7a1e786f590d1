"""Inputs and a windowed oracle for the tests of the waveform speed search (csrc/xcorr.hip behind
nc_xcorr_search, planned by ops.xcorr_speed).  No GPU in here.

search() restates the loop of oracle/refglue.py estimate_speed_xcorr_arrays and keeps, for every
window, what that function throws away: whether a gate dropped it, the best candidate, how far
it stands above the runner-up, and whether it became a correspondence.  Its (ratio, quality)
equal refglue's (test_xcorr_search_cases_cpu.py).  search(f64=True) takes the dot products and
norms in f64 as xcorr_dot_kernel does (the reference's np.dot / np.linalg.norm are f32).

Small shapes through the public parameters: a 6 s source and its 100/101 resample, windows of
0.05 s (1102 samples, stride 275, up to 39 candidates per window) and 0.1 s (2205 samples),
neither a multiple of the 256 threads of xcorr_dot_kernel, from 3 to 200 windows per search.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import scipy.signal

from oracle import refglue
from nightcore_analyzer import synth

SR = 22050
SECONDS, SEED = 6.0, 1041
WINDOWS = (3, 20, 64, 65, 80, 200)        # 64: what one thread of the finalize kernel used to hold
WINDOW_SECS = (0.05, 0.1)
RATIO_TOL, QUALITY_TOL = 1e-9, 1e-5       # the bars of test_gpu_components.test_xcorr_speed_matches_oracle
RUNNER_UP = 1e-5                          # every decision the GPU is held to stands this far clear
GATE_RMS = 1e-3                           # xcorr.py:117-118

Case = namedtuple("Case", "ya yb n_windows window_sec search_range")
Window = namedtuple("Window", "pa exp_pb lo gate best best_pb runner_up n_cand matched")
Search = namedtuple("Search", "ratio quality windows")


# --------------------------------------------------------------------------- the oracle, window by window
def search(ya, yb, sr=SR, n_windows=20, window_sec=3.0, search_range=0.05, skip_edges=0.10, f64=False):
    ya = np.asarray(ya, np.float32)
    yb = np.asarray(yb, np.float32)
    min_len = min(len(ya), len(yb))
    s, e = int(min_len * skip_edges), int(min_len * (1.0 - skip_edges))
    ya, yb = ya[s:e], yb[s:e]
    if f64:
        ya, yb = ya.astype(np.float64), yb.astype(np.float64)
    win = int(window_sec * sr)
    srch = int(search_range * len(yb))
    stride = max(1, win // 4)
    if len(ya) < win or len(yb) < win:
        return Search(1.0, 0.0, ())
    wins, corr, qual = [], [], []
    for pa in np.linspace(0, len(ya) - win, n_windows).astype(int):
        pa = int(pa)
        wa = ya[pa:pa + win]
        exp_pb = int(pa * len(yb) / len(ya))
        lo, hi = max(0, exp_pb - srch), min(len(yb) - win, exp_pb + srch)
        rms = float(np.sqrt(np.mean(wa ** 2)))
        if rms < GATE_RMS:
            wins.append(Window(pa, exp_pb, lo, "rms", -1.0, exp_pb, -1.0, 0, False))
            continue
        if lo >= hi:
            continue
        na = float(np.linalg.norm(wa))
        best_c, best_pb, second, n_cand = -1.0, exp_pb, -1.0, 0
        for pb in range(lo, hi, stride):
            wb = yb[pb:pb + win]
            nb = float(np.linalg.norm(wb))
            if nb < 1e-10:
                continue
            n_cand += 1
            c = float(np.dot(wa, wb) / (na * nb))
            if c > best_c:
                best_c, best_pb, second = c, pb, best_c
            elif c > second:
                second = c
        matched = best_c > 0
        wins.append(Window(pa, exp_pb, lo, None if n_cand else "norm", best_c, best_pb, second, n_cand, matched))
        if matched:
            corr.append((pa, best_pb))
            qual.append(best_c)
    if len(corr) < 3:
        return Search(1.0, 0.0, tuple(wins))
    a = np.array([c[0] for c in corr], dtype=float)
    b = np.array([c[1] for c in corr], dtype=float)
    return Search(float(np.polyfit(a, b, 1)[0]), float(np.median(qual)), tuple(wins))


# --------------------------------------------------------------------------- signals
@lru_cache(maxsize=None)
def source():
    y = synth.make_source(SECONDS, SEED)
    y.setflags(write=False)
    return y


@lru_cache(maxsize=None)
def faster():
    y = scipy.signal.resample_poly(source().astype(np.float64), 100, 101).astype(np.float32)
    y.setflags(write=False)
    return y


def _trimmed_geometry(len_a, len_b, n_windows, window_sec, search_range=0.05):
    """Window positions and candidate spans in untrimmed sample indices: [(a0, b_lo, b_hi_end)]."""
    min_len = min(len_a, len_b)
    s, e = int(min_len * 0.10), int(min_len * 0.90)
    n = e - s
    win, srch = int(window_sec * SR), int(search_range * n)
    out = []
    for pa in np.linspace(0, n - win, n_windows).astype(int):
        exp_pb = int(int(pa) * n / n)
        lo, hi = max(0, exp_pb - srch), min(n - win, exp_pb + srch)
        out.append((s + int(pa), s + lo, s + hi + win))
    return win, out


def gated(n_matching):
    """8 windows of 0.1 s.  The source's windows 0 and 1 are scaled to an RMS of 5e-4 (dropped by
    the 1e-3 gate) and window 2 to 2e-3 (kept).  The other signal is exact zeros over every
    candidate of windows 3, 4 and 5 (and of 7 when n_matching is 2): no candidate passes
    nb >= 1e-10.  Windows 2, 6 (and 7) match: three gives a fit, two gives (1.0, 0.0)."""
    assert n_matching in (2, 3)
    ya, yb = source().copy(), faster().copy()
    win, geo = _trimmed_geometry(len(ya), len(yb), 8, 0.1)
    for k, target in ((0, 5e-4), (1, 5e-4), (2, 2e-3)):
        a0 = geo[k][0]
        rms = float(np.sqrt(np.mean(ya[a0:a0 + win].astype(np.float64) ** 2)))
        ya[a0 - 64:a0 + win + 64] *= np.float32(target / rms)
    for k in (3, 4, 5) + ((7,) if n_matching == 2 else ()):
        yb[geo[k][1]:geo[k][2]] = 0.0
    return Case(ya, yb, 8, 0.1, 0.05)


def tied():
    """The second signal repeats one 275-sample pattern, the candidate stride of a 1102-sample
    window: every candidate window of a search holds the same samples, so its dot product and
    norm are the same bits in any implementation, and the first candidate (lo) must win.  The
    first signal is that pattern plus the source at a tenth: every correlation is above 0.3."""
    stride = int(0.05 * SR) // 4
    n = len(source())
    pat = source()[40000:40000 + stride]
    yb = np.resize(pat, n).astype(np.float32)
    ya = (yb + np.float32(0.1) * source()).astype(np.float32)
    return Case(ya, yb, 20, 0.05, 0.05)


def _cases():
    c = {}
    for ws in WINDOW_SECS:
        for nw in WINDOWS:
            c[f"speed_w{nw}_{ws}"] = Case(source(), faster(), nw, ws, 0.05)
        c[f"copy_{ws}"] = Case(source(), source(), 20, ws, 0.05)
    c["gated_three"] = gated(3)
    c["gated_two"] = gated(2)
    neg = (-source()).astype(np.float32)
    c["anti"] = Case(source(), neg, 20, 0.05, 0.05)
    # one candidate per window, the one before the aligned position: correlation near +1 / -1, so
    # every window matches / no window does (best <= 0)
    narrow = 1.5 / (0.8 * len(source()))
    c["narrow"] = Case(source(), source(), 20, 0.05, narrow)
    c["anti_narrow"] = Case(source(), neg, 20, 0.05, narrow)
    c["tied"] = tied()
    for k in c.values():
        for a in (k.ya, k.yb):
            a.setflags(write=False)
    return c


CASES = _cases()
NAMES = tuple(CASES)


@lru_cache(maxsize=None)
def oracle(name, f64=False):
    k = CASES[name]
    return search(k.ya, k.yb, SR, k.n_windows, k.window_sec, k.search_range, f64=f64)


def reference(name):
    """(ratio, quality) of refglue.estimate_speed_xcorr_arrays, the function the GPU replaces."""
    k = CASES[name]
    return refglue.estimate_speed_xcorr_arrays(k.ya, k.yb, SR, k.n_windows, k.window_sec, k.search_range)
