"""Inputs, a per-speed oracle and the yardstick for the tests of the intro-offset search
(csrc/align.hip behind nc_align_offsets: plan, half-band decimate, RMS envelope, stretch,
correlate, cosine select).  No GPU in here.

oracle() (evaluate_env on the case's envelopes) walks the speed grid exactly as oracle/refglue.py find_content_offset does, from the
same pieces (ncref.resample_half, ncref.rms_frames, np.interp, np.correlate), and keeps what
that function throws away: for every speed whether it was skipped, the stretch length, the lag
count, the peak, how far the peak stands above the next largest correlation, and the cosine
score.  Its winner is find_content_offset(detail=True)'s (test_align_cases_cpu.py).

oracle(exact=True) differs in one thing: the envelope's mean of squares is accumulated in f64
and rounded to f32 once, which is what align_env_kernel does; the oracle takes numpy's f32
mean.  Both are legitimate f32 envelopes.  The largest score difference between the two over
all cases is the yardstick(): what the rounding of the envelope alone moves the score by.  The
GPU is held to SCORE_MARGIN x that; the other differences (fused multiply-adds in the
decimator, f64 summation order) are orders of magnitude smaller, and the margin covers that the
yardstick samples one realisation of the envelope's rounding.

The decisions (peaks, the winning speed) are demanded exactly on the GPU, so the cases are
qualified on the CPU: every peak stands PEAK_MARGIN above the runner-up, relatively, and the
winner's score WIN_MARGIN above every other speed's unless the two speeds are bit-identical
(same stretch length, score difference exactly 0).  Both are some hundred times the yardstick.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from golden.cases import make_align_pair
from oracle import ncref, refglue
from nightcore_analyzer import synth

SR = 22050
HOP_SEC = refglue.ALIGN_HOP / refglue.ALIGN_SR
MAX_FRAMES = int(refglue.ALIGN_MAX_OFFSET / HOP_SEC)          # 2583: at most 2584 lags
GRID_REF = (refglue.ALIGN_SPEED_LO, refglue.ALIGN_SPEED_HI, refglue.ALIGN_N_SPEEDS)
GRID_WIDE = (0.8, 1.2, 9)       # speeds below 1: the nc envelope is stretched, not squeezed (golden60: all searchable)
GRID_MIXED = (0.6, 1.2, 9)      # golden60: the slowest speeds stretch the nc envelope beyond the source's and are skipped
PEAK_MARGIN = 1e-6
WIN_MARGIN = 1e-6
SCORE_MARGIN = 16.0
AL_TILE = 1024                  # csrc/align.hip: stretched samples per LDS tile of align_corr_kernel

Speed = namedtuple("Speed", "skipped n_st n_lag peak margin score all_zero denom")
Eval = namedtuple("Eval", "speeds winner")     # winner = (peak, speed_idx, score), speed_idx -1: none


def grid(g):
    return np.linspace(g[0], g[1], g[2])


# --------------------------------------------------------------------------- envelopes
def envelope(y, exact=False):
    """refglue.find_content_offset's envelope of one signal (f64 values of an f32 RMS).
    exact: ncref.rms_frames with the mean of the f32 squares accumulated in f64, rounded once."""
    d = ncref.resample_half(y)
    if not exact:
        return ncref.rms_frames(d, 2048, refglue.ALIGN_HOP).astype(np.float64)
    d = np.asarray(d, np.float32)
    T = 1 + len(d) // refglue.ALIGN_HOP
    fr = ncref._frames(d, 2048, refglue.ALIGN_HOP, 0, T)
    ms = np.mean(fr * fr, axis=-1, dtype=np.float64).astype(np.float32)
    return np.sqrt(ms).astype(np.float64)


def evaluate_env(src_env, nc_env, speeds):
    """The loop of refglue.find_content_offset over `speeds`, keeping every speed's figures."""
    out = []
    best = (0, -1, -1.0)
    for si, speed in enumerate(speeds):
        n_st = int(len(nc_env) / speed)
        search_len = min(MAX_FRAMES, len(src_env) - n_st)
        if n_st < 4 or n_st >= len(src_env) or search_len <= 0:
            out.append(Speed(True, n_st, 0, 0, 0.0, 0.0, False, 0.0))
            continue
        stretched = np.interp(np.linspace(0.0, 1.0, n_st), np.linspace(0.0, 1.0, len(nc_env)), nc_env)
        corr = np.correlate(src_env[:search_len + n_st], stretched, mode="valid")[:search_len + 1]
        peak = int(np.argmax(corr))
        peak_val = float(corr[peak])
        rest = np.delete(corr, peak)
        margin = (peak_val - float(rest.max())) / peak_val if len(rest) and peak_val > 0 else 0.0
        win_energy = float(np.sum(src_env[peak:peak + n_st] ** 2))
        query_energy = float(np.sum(stretched ** 2))
        denom = np.sqrt(win_energy * query_energy)
        score = peak_val / denom if denom > 1e-12 else 0.0
        out.append(Speed(False, n_st, len(corr), peak, margin, score, not corr.any(), float(denom)))
        if score > best[2]:
            best = (peak, si, score)
    return Eval(tuple(out), best)


# --------------------------------------------------------------------------- cases
@lru_cache(maxsize=None)
def _pair(seconds, seed, intro, up, down):
    nc, src = make_align_pair(synth, float(seconds), seed, float(intro), up, down)
    for a in (nc, src):
        a.setflags(write=False)
    return src, nc


_SHORT_NC = (30, 1031, 0.0, 4, 5)      # the source whose nc is cut to 1 s, 6 frames, 3 frames


def _golden60():
    return _pair(60, 1005, 7.3, 4, 5)


def _two_tiles():
    return _pair(70, 1021, 3.0, 4, 5)


def _other_ratio():
    return _pair(24, 1022, 12.5, 10, 13)


def _lag_cap():
    return _pair(40, 1024, 110.0, 4, 5)


def _short():
    return _pair(8, 1008, 0.0, 4, 5)


def _nc_cut(n):
    src, nc = _pair(*_SHORT_NC)
    return src, nc[:n]


def _nc_longer():
    return _pair(10, 1032, 0.0, 4, 5)[0], _pair(25, 1033, 0.0, 4, 5)[1]


def _silent_src():
    return np.zeros(10 * SR, np.float32), _pair(8, 1008, 0.0, 4, 5)[1][:5 * SR]


def _silent_nc():
    return _pair(24, 1022, 12.5, 10, 13)[0][:14 * SR], np.zeros(10 * SR, np.float32)


def _quiet():
    src, nc = _pair(40, 1034, 8.0, 4, 5)
    s = np.float32(1e-9)
    return (src[:40 * SR] * s).astype(np.float32), (nc[:20 * SR] * s).astype(np.float32)


CASES = {
    "golden60": _golden60,
    "two_tiles": _two_tiles,
    "other_ratio": _other_ratio,
    "lag_cap": _lag_cap,
    "short": _short,
    "nc_1s": lambda: _nc_cut(22050),
    "nc_6_frames": lambda: _nc_cut(5512),
    "nc_too_short": lambda: _nc_cut(3000),
    "nc_longer": _nc_longer,
    "silent_src": _silent_src,
    "silent_nc": _silent_nc,
    "quiet": _quiet,
}
NAMES = tuple(CASES)
ALL_SKIPPED = ("nc_too_short", "nc_longer")
SILENT = ("silent_src", "silent_nc")
# (case, grid) of every comparison: the reference's grid on every case, the other two on golden60
RUNS = tuple((n, GRID_REF) for n in NAMES) + (("golden60", GRID_WIDE), ("golden60", GRID_MIXED))


@lru_cache(maxsize=None)
def signals(name):
    """(src, nc) of a case, float32, read-only."""
    src, nc = CASES[name]()
    src, nc = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(nc, np.float32)
    for a in (src, nc):
        a.setflags(write=False)
    return src, nc


@lru_cache(maxsize=None)
def _envelopes(name, exact):
    src, nc = signals(name)
    return envelope(src, exact), envelope(nc, exact)


@lru_cache(maxsize=None)
def oracle(name, g=GRID_REF, exact=False):
    """Eval of a case on a speed grid; exact: with the envelope's mean accumulated in f64."""
    src_env, nc_env = _envelopes(name, exact)
    return evaluate_env(src_env, nc_env, grid(g))


def case_yardstick(name, g=GRID_REF):
    """Largest |score(f32 mean) - score(f64 mean)| over the speeds both evaluations search."""
    a, b = oracle(name, g), oracle(name, g, True)
    return max([abs(x.score - y.score) for x, y in zip(a.speeds, b.speeds) if not x.skipped and not y.skipped],
               default=0.0)


@lru_cache(maxsize=None)
def yardstick():
    """The largest case_yardstick over every (case, grid) the GPU is compared on."""
    return max(case_yardstick(n, g) for n, g in RUNS)


def score_tol():
    return SCORE_MARGIN * yardstick()
