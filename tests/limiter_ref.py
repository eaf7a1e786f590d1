"""The true-peak limiter's definition in numpy float64 ("True-peak limiter"),
evaluated directly, an independent 8x true-peak meter used only for checking, and the test
signals shared by tests/test_limiter_cpu.py and tests/test_gpu_limiter.py.

For the channels x_c[n], n < N, of one file (zero outside), L = 10^(limit_db / 20),
Wa = max(1, round(attack_ms sr / 1000)), Wr = max(1, round(release_ms sr / 1000)), beta = exp(-1 / Wr):
  h(u) = sinc(u) I0(9 sqrt(1 - (u / 12)^2)) / I0(9) for |u| < 12, else 0
  x_c(n + k/4) = sum_{i = -11..12} x_c[n + i] h(k/4 - i), k = 1, 2, 3
  t[n] = max_c max_k |x_c(n + k/4)|  (n = -1 included),  p[n] = max(max_c |x_c[n]|, t[n-1], t[n])
  r[n] = min(1, L / p[n]), 1 where p = 0 and outside the file
  hA[n] = min_{0 <= i < Wa} r[n + i],  a[n] = (1 / Wa) sum_{0 <= i < Wa} hA[n - i]
  d[n] = max(1 - a[n], beta d[n-1]), d[-1] = 0,  g[n] = 1 - d[n]
  y_c[n] = clamp(x_c[n] g[n], -L32, L32), L32 = L rounded to float32
1 - a is summed directly as the mean of 1 - hA, so it is exactly 0 (g exactly 1) wherever no
r < 1 lies within Wa - 1 samples.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TILE = 4096                      # a multiple of every tile of csrc/limiter.hip (LM_T = LM_PK_T = 2048):
                                 # each multiple of it is a tile boundary of every kernel
THRESHOLD = 2.0 ** -25           # float32(1 - d) < 1 exactly when d > 2^-25 (ties go to even: 1)
RATES = (22050, 48000)


def windows(sr: int, attack_ms: float = 5.0, release_ms: float = 50.0):
    """(Wa, Wr) in samples."""
    return max(1, int(round(attack_ms * sr / 1000.0))), max(1, int(round(release_ms * sr / 1000.0)))


def _kaiser_sinc(u, zeros: float, beta: float):
    u = np.asarray(u, np.float64)
    q = np.clip(1.0 - (u / zeros) ** 2, 0.0, None)
    return np.where(np.abs(u) < zeros, np.sinc(u) * np.i0(beta * np.sqrt(q)) / np.i0(beta), 0.0)


def h(u):
    """The inter-sample filter of the definition."""
    return _kaiser_sinc(u, 12.0, 9.0)


def _phases(x: np.ndarray, over: int, half: int, filt) -> np.ndarray:
    """[over - 1, N + 1]: |x(n + k / over)|, k = 1 .. over - 1, n = -1 .. N - 1 (column n + 1),
    by the 2 half taps i = -(half - 1) .. half of ``filt``; x one channel, zero outside."""
    n = len(x)
    xp = np.concatenate([np.zeros(half), np.asarray(x, np.float64), np.zeros(half)])
    i = np.arange(-(half - 1), half + 1)
    out = np.zeros((over - 1, n + 1))
    for a in range(0, n + 1, 16384):
        win = sliding_window_view(xp[a:a + 16384 + 2 * half - 1], 2 * half)[:n + 1 - a]   # x[m - 1 + i], m = a ..
        for k in range(1, over):
            out[k - 1, a:a + len(win)] = np.abs(win @ filt(k / over - i))
    return out


def sliding_min(v: np.ndarray, w: int) -> np.ndarray:
    """min(v[i : i + w]) for i <= len(v) - w."""
    return sliding_window_view(v, w).min(axis=1) if len(v) >= w else np.zeros(0)


@dataclass
class Limited:
    p: np.ndarray
    r: np.ndarray
    a1: np.ndarray        # 1 - a
    d: np.ndarray
    g: np.ndarray
    y: np.ndarray         # [channels, N]
    true_peak: float
    limited: int
    L: float
    Wa: int
    Wr: int


def limiter_ref(x, limit_db: float, Wa: int, Wr: int) -> Limited:
    """The definition on x [channels, N] (or [N]) in float64."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    C, N = x.shape
    L = 10.0 ** (limit_db / 20.0)
    if N == 0:
        z = np.zeros(0)
        return Limited(z, z, z, z, z, x.copy(), 0.0, 0, L, Wa, Wr)
    t = np.zeros(N + 1)
    for c in range(C):
        t = np.maximum(t, _phases(x[c], 4, 12, h).max(axis=0))
    p = np.maximum(np.abs(x).max(axis=0), np.maximum(t[:-1], t[1:]))
    r = np.where(p > 0.0, np.minimum(1.0, L / np.where(p > 0.0, p, 1.0)), 1.0)
    one = np.ones(Wa - 1)
    hA = sliding_min(np.concatenate([one, r, one]), Wa)                 # hA[n], n = -(Wa - 1) .. N - 1
    a1 = np.zeros(N)
    for s in range(0, N, 8192):
        a1[s:s + 8192] = sliding_window_view(1.0 - hA[s:s + 8192 + Wa - 1], Wa).sum(axis=1) / Wa
    beta = np.exp(-1.0 / Wr)
    d = np.empty(N)
    prev = 0.0
    for n, e in enumerate(a1.tolist()):
        prev = e if e > beta * prev else beta * prev
        d[n] = prev
    g = 1.0 - d
    L32 = float(np.float32(L))
    y = np.clip(x * g[None, :], -L32, L32)
    limited = int(np.count_nonzero((1.0 - d).astype(np.float32) < np.float32(1.0)))
    return Limited(p, r, a1, d, g, y, float(p.max()), limited, L, Wa, Wr)


def meter8(y) -> float:
    """An independent true-peak reading of y [channels, N]: 8x oversampling by a Kaiser
    (beta 12) windowed sinc of 32 zero crossings a side."""
    y = np.atleast_2d(np.asarray(y, np.float64))
    if y.shape[1] == 0:
        return 0.0
    filt = lambda u: _kaiser_sinc(u, 32.0, 12.0)  # noqa: E731
    return max(max(float(np.abs(c).max()), float(_phases(c, 8, 32, filt).max())) for c in y)


# ------------------------------------------------------------------ test signals
@dataclass
class Case:
    name: str
    sr: int
    x: np.ndarray            # float32 [channels, N]
    limit_db: float = -0.1
    peaks: tuple = ()        # positions of the over-peaks put in (sample indices)

    @property
    def wa_wr(self):
        return windows(self.sr)


def _bed(n: int, seed: int, amp: float = 0.2) -> np.ndarray:
    """A quiet bed well under any ceiling used here: two sines and a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return amp * (0.6 * np.sin(2 * np.pi * 0.0131 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 0.0717 * t)
                  + 0.1 * rng.uniform(-1.0, 1.0, n))


def _spiked(n: int, seed: int, spikes) -> np.ndarray:
    x = _bed(n, seed)
    for j, v in spikes:
        x[j] = v
    return x


L01 = 10.0 ** (-0.1 / 20.0)
LONG = 5 * TILE + 37


@lru_cache(maxsize=None)
def cases(sr: int):
    """The cases at one rate, in a fixed order."""
    Wa, Wr = windows(sr)
    N = LONG
    out = []

    def add(name, chans, **kw):
        out.append(Case(name, sr, np.stack([np.asarray(c, np.float32) for c in chans]), **kw))

    add("under", [_bed(N, 1)])
    add("first_last", [_spiked(N, 2, [(0, 1.7), (N - 1, -2.1)])], peaks=(0, N - 1))
    add("tile_edge", [_spiked(N, 3, [(TILE - 1, 1.5), (2 * TILE, -1.9), (4 * TILE - 1, 1.3), (4 * TILE, 1.4)])],
        peaks=(TILE - 1, 2 * TILE, 4 * TILE - 1, 4 * TILE))
    add("near_ends", [_spiked(N, 4, [(Wa // 2, 1.6), (N - 1 - Wa // 2, 2.2)])], peaks=(Wa // 2, N - 1 - Wa // 2))
    add("long_tail", [_spiked(N, 5, [(100, 4.0 * L01)])], peaks=(100,))
    # (f): a smaller over-peak inside the tail of the first (r = L/3 against a tail still above
    # 1 - L/1.05), then a larger one that overrides it
    add("tail_peaks", [_spiked(N, 6, [(3000, 3.0), (3000 + Wr // 4, 1.05), (3000 + Wr, -3.6)])],
        peaks=(3000, 3000 + Wr // 4, 3000 + Wr))
    # (g): full-scale sine at sr / 4, 45 degrees: sample peaks 0.7071, true peak near 1
    add("quarter_sine", [np.sin(2 * np.pi * 0.25 * np.arange(N) + np.pi / 4)], limit_db=20.0 * np.log10(0.9))
    add("stereo", [_bed(N, 7), _spiked(N, 8, [(TILE + 17, 2.5), (3 * TILE + 5, -1.2)])],
        peaks=(TILE + 17, 3 * TILE + 5))
    for n in (1, Wa - 1, 2 * Wa):
        add(f"short_{n}", [_spiked(n, 9 + n, [(n // 2, 1.8)])], peaks=(n // 2,))
    add("empty", [np.zeros(0)])
    return tuple(out)


@lru_cache(maxsize=None)
def reference(sr: int, name: str) -> Limited:
    """limiter_ref of a case, computed once."""
    c = next(c for c in cases(sr) if c.name == name)
    return limiter_ref(c.x, c.limit_db, *c.wa_wr)
