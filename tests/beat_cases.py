"""Case builder and oracle helpers for the beat-tracker tests (numpy only: no GPU, no torch).

The tracker (csrc/beat.hip, tempo_beat_kernel) is specified to equal oracle/ncref.beat_track in
its decisions (bpm, lag, beat frames), not in its floating-point intermediates.  Two differences
in intermediates are legitimate:

  * device exp / log may differ from the host libm's by an ulp, which moves entries of the
    Gaussian beat window and of the DP penalty table;
  * the kernel's onset norm (f64 sum -> f32 mean -> f64 sum of squares of the f32 residuals ->
    f32) may differ by a float32 ulp from numpy's float32 pairwise ``std(ddof=1)``.

A case is used for exact comparison only if the oracle's beats survive both (``qualifies``):
(a) every table entry moved one ulp in a random direction, for two seeds, and (b) the norm
computed the kernel's way.  ``beats_with`` is the oracle's beat_track body with the tables and
the norm passed in; with none passed it is ncref.beat_track itself (test_beat_cases_cpu.py
checks that).

The period is forced: P equals the chosen tempogram lag L, and a one-hot tempogram mean
(tg[L] = 1) makes ``log1p(1e6 tg) + logprior`` select L for any L whose tempo is below the
320 BPM cut-off of the prior.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import ncref
from nightcore_analyzer.engine import beat_needs_workspace

SR = 22050
START_BPM = 120.0
MAX_TEMPO = 320.0

KINDS = ("noise", "clicks", "impulse", "silence_mid")   # compared exactly with the oracle
WEAK_KINDS = ("const",)                                  # exact plateaus: invariants only

# group: grid group; kind: envelope generator; N frames; P forced period (= lag); hop, acw
Case = namedtuple("Case", "group kind N P hop acw")


def acw_of(hop: int) -> int:
    return ncref.ac_win_length(SR, hop)


def seed_of(case: Case) -> int:
    return 7 * case.N + case.P


def boundary(acw: int) -> tuple[int, int]:
    """(largest T that runs in LDS, smallest T that needs the workspace) for this acw."""
    lo, hi = 1, 1 << 20
    assert not beat_needs_workspace(lo, acw) and beat_needs_workspace(hi, acw)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if beat_needs_workspace(mid, acw):
            hi = mid
        else:
            lo = mid
    return lo, hi


# --------------------------------------------------------------------------- envelopes
def envelope(kind: str, N: int, P: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x = rng.random(N)
    elif kind in ("clicks", "silence_mid"):
        x = 0.2 * rng.random(N)
        Q = max(2, int(1.07 * P))           # clicks disagree with the forced period
        x[int(rng.integers(0, Q))::Q] += 1.0
        if kind == "silence_mid":           # first-beat threshold i0 and the trim
            x[:N // 4] = 0.0
            x[N - N // 5:] = 0.0
    elif kind == "impulse":
        x = np.zeros(N)
        x[N // 3] = 1.0
    elif kind == "fade":                    # scores fall over the last two fifths: see radix_cases
        x = rng.random(N)
        x[(3 * N) // 5:N - 2 * P] -= 3.0    # the last 2P frames stay positive: the trim ends there
    elif kind == "const":
        x = np.ones(N)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def case_onset(case: Case) -> np.ndarray:
    return envelope(case.kind, case.N, case.P, seed_of(case))


def forcible(P: int, hop: int) -> bool:
    return 60.0 * SR / (hop * P) < MAX_TEMPO


def one_hot_tg(acw: int, L: int) -> np.ndarray:
    tg = np.zeros(acw, dtype=np.float64)
    tg[L] = 1.0
    return tg


def case_tg(case: Case) -> np.ndarray:
    return one_hot_tg(case.acw, case.P)


# --------------------------------------------------------------------------- the grid
def _group(name, hop, Ps, Ns, kinds):
    acw = acw_of(hop)
    return [Case(name, k, N, P, hop, acw) for P in Ps for N in Ns for k in kinds
            if forcible(P, hop)]


@functools.lru_cache(maxsize=None)
def grid(weak: bool = False) -> tuple:
    """Every (group, envelope, N, P) case; weak=True gives the ``const`` envelopes instead."""
    kinds = WEAK_KINDS if weak else KINDS
    lds_max, ws_min = boundary(acw_of(512))
    lds_max_ibi, ws_min_ibi = boundary(acw_of(64))
    cases = []
    cases += _group("lds", 512, (9, 10, 13, 14, 15, 16, 17, 64, 127, 343),
                    (2, 3, 4, 5, 40, 431, lds_max), kinds)
    cases += _group("long", 512, (9, 17, 200, 343), (ws_min, 3500), kinds)
    ibi = _group("ibi", 64, (65, 168, 344, 700, 1022, 1023, 1024, 2755), (ws_min_ibi, 2600, 9000), kinds)
    # the oracle's DP takes ~0.6 s per run there: two envelopes are enough
    cases += [c for c in ibi if not (c.P >= 1024 and c.N == 9000 and c.kind not in ("noise", "clicks", "const"))]
    # the LDS side of the hop-64 boundary: the wave DP with long candidate ranges
    cases += _group("ibi_lds", 64, (65, 344, 1023, 2755), (lds_max_ibi,), kinds)
    # hop 2048 cannot force P = 2 (323 BPM is above the prior's cut-off); hop 4096 does
    cases += _group("tiny", 2048, (2, 3, 4, 5, 8), (300,), kinds)
    cases += _group("tiny", 4096, (2, 3, 4, 5, 8), (300,), kinds)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def radix_cases() -> tuple:
    """Cases with more cumulative-score peaks than the kernel has threads, both parities per
    path and envelope: the last-beat median runs the radix select (block_kth_flagged).  They
    are compared with trim on and off."""
    lds_max, _ = boundary(acw_of(512))
    a5, a64 = acw_of(512), acw_of(64)
    noise = (Case("radix_lds", "noise", lds_max, 9, 512, a5), Case("radix_lds", "noise", lds_max, 16, 512, a5),
             Case("radix_lds", "noise", 2000, 9, 512, a5),
             Case("radix_long", "noise", 4500, 9, 512, a5), Case("radix_long", "noise", 4500, 10, 512, a5),
             Case("radix_ibi", "noise", 12000, 65, 64, a64), Case("radix_ibi", "noise", 12000, 66, 64, a64))
    # On a non-negative envelope the scores never fall along a chain of beats, the last peak
    # clears half of any median and the select's value decides nothing.  On ``fade`` they fall
    # towards the end, so the last beat is where the peaks cross half the median
    # (median_decides): a wrong median moves it.  That shows with trim off only: the trim's RMS
    # threshold, raised by the negative scores, removes every beat (nbeats 0, also worth a run).
    fade = (Case("radix_lds", "fade", lds_max, 12, 512, a5), Case("radix_lds", "fade", lds_max, 10, 512, a5),
            Case("radix_lds", "fade", 2000, 10, 512, a5),
            Case("radix_long", "fade", 4500, 9, 512, a5), Case("radix_long", "fade", 4500, 11, 512, a5),
            Case("radix_long", "fade", 4500, 12, 512, a5),
            Case("radix_ibi", "fade", 15000, 65, 64, a64), Case("radix_ibi", "fade", 15000, 67, 64, a64))
    return noise + fade


@functools.lru_cache(maxsize=None)
def rank_cases() -> tuple:
    """``fade`` cases with at most as many peaks as the kernel has threads: the rank-count form of
    the median, where its value decides the last beat (compared with trim off, as above)."""
    _, ws_min = boundary(acw_of(512))
    a5, a64 = acw_of(512), acw_of(64)
    return (Case("rank_lds", "fade", 431, 13, 512, a5), Case("rank_lds", "fade", 431, 17, 512, a5),
            Case("rank_lds", "fade", 900, 16, 512, a5), Case("rank_lds", "fade", 1000, 64, 512, a5),
            Case("rank_long", "fade", ws_min, 17, 512, a5), Case("rank_long", "fade", 3500, 64, 512, a5),
            Case("rank_ibi", "fade", 2600, 65, 64, a64), Case("rank_ibi", "fade", 9000, 168, 64, a64))


MIXED_LAGS = {512: (13, 17), 64: (168, 220)}   # two hot lags per hop: the prior picks between them


@functools.lru_cache(maxsize=None)
def mixed_cases(hop: int) -> tuple:
    """Sequences of one mixed-length launch: N = 2, 3, 4, 5 and 40 next to workspace-length ones,
    alternating between the two periods of MIXED_LAGS[hop]."""
    acw = acw_of(hop)
    _, ws_min = boundary(acw)
    shapes = ((2, "noise"), (3, "clicks"), (4, "noise"), (5, "clicks"), (40, "noise"), (40, "clicks"),
              (ws_min, "noise"), (ws_min, "clicks"))
    return tuple(Case("mixed", kind, N, MIXED_LAGS[hop][j % 2], hop, acw) for j, (N, kind) in enumerate(shapes))


RADIX_NT = {"radix_lds": 256, "radix_long": 1024, "radix_ibi": 1024,    # threads of the path's kernel
            "rank_lds": 256, "rank_long": 1024, "rank_ibi": 1024}


def groups(cases) -> dict:
    out = {}
    for c in cases:
        out.setdefault(c.group, []).append(c)
    return out


# --------------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def oracle(case: Case, trim: bool = True):
    """ncref.beat_track as it stands -> (bpm, beat frames)."""
    bpm, beats = ncref.beat_track(case_onset(case), SR, case.hop, START_BPM, trim=trim, tg_mean=case_tg(case))
    beats.setflags(write=False)
    return bpm, beats


def numpy_norm(onset: np.ndarray) -> np.float32:
    """The norm of ncref.normalize_onsets."""
    return onset.std(ddof=1) + ncref.TINY32


def kernel_norm(onset: np.ndarray) -> np.float32:
    """The norm as tempo_beat_kernel takes it."""
    n = len(onset)
    mean32 = np.float32(onset.astype(np.float64).sum() / n)
    d = (onset - mean32).astype(np.float64)           # f32 residuals, squared and summed in f64
    std32 = np.float32(np.sqrt((d * d).sum() / (n - 1)))
    return np.float32(std32 + np.float32(ncref.TINY32))


def ulp_jitter(tab: np.ndarray, rng) -> np.ndarray:
    """Every finite entry moved one ulp up or down."""
    up = rng.random(tab.shape) < 0.5
    out = np.where(up, np.nextafter(tab, np.inf), np.nextafter(tab, -np.inf))
    return np.where(np.isfinite(tab), out, tab)


def _local_score(onset_norm, win):          # ncref.beat_local_score with the window passed in
    x = onset_norm.astype(np.float64)
    N, K = len(x), len(win)
    out = np.zeros(N, dtype=np.float64)
    i = np.arange(N)
    for k in range(K):
        j = i + K // 2 - k
        ok = (j >= 0) & (j < N)
        out[ok] += win[k] * x[j[ok]]
    return out


def _dp(localscore, P, pen):                # ncref.beat_track_dp with the penalty table passed in
    N = len(localscore)
    dmin = int(np.round(P / 2.0))
    dmax = int(2 * P)
    thr = 0.01 * localscore.max()
    backlink = np.full(N, -1, dtype=np.int64)
    cumscore = np.zeros(N, dtype=np.float64)
    first = True
    for i in range(N):
        hi = min(dmax, i)
        best_loc = -1
        best = -np.inf
        if hi >= dmin:
            d = np.arange(dmin, hi + 1)
            sc = cumscore[i - d] - pen[d]
            j = int(np.argmax(sc))
            best = sc[j]
            best_loc = i - int(d[j])
            if not (best > -np.inf):
                best_loc = -1
        cumscore[i] = localscore[i] + best if best_loc >= 0 else localscore[i]
        if first and localscore[i] < thr:
            backlink[i] = -1
        else:
            backlink[i] = best_loc
            first = False
    return backlink, cumscore


def beats_with(onset, P, trim=True, norm=None, win=None, pen=None) -> np.ndarray:
    """The body of ncref.beat_track after the tempo, with norm / window / penalty overridable."""
    onset = np.asarray(onset, dtype=np.float32)
    P = float(P)
    norm = numpy_norm(onset) if norm is None else norm
    win = ncref.gaussian_beat_window(P) if win is None else win
    pen = ncref.dp_penalty(P) if pen is None else pen
    ls = _local_score(onset / norm, win)
    backlink, cumscore = _dp(ls, P, pen)
    tail = ncref.last_beat(cumscore)
    beats = np.zeros(len(onset), dtype=bool)
    n = tail
    while n >= 0:
        beats[n] = True
        n = backlink[n]
    return np.flatnonzero(ncref.trim_beats(ls, beats, trim)).astype(np.int64)


def qualify(case: Case, trim: bool = True) -> dict:
    """Which of the allowed differences change the oracle's beats: {'a1', 'a2', 'b'} -> bool
    (True = unchanged), plus 'norm_differs'."""
    onset = case_onset(case)
    _, ref = oracle(case, trim)
    P = float(case.P)
    res = {}
    for tag, s in (("a1", 1), ("a2", 2)):
        rng = np.random.default_rng(1000003 * s + seed_of(case))
        got = beats_with(onset, P, trim=trim, win=ulp_jitter(ncref.gaussian_beat_window(P), rng),
                         pen=ulp_jitter(ncref.dp_penalty(P), rng))
        res[tag] = np.array_equal(got, ref)
    kn = kernel_norm(onset)
    res["norm_differs"] = bool(kn != numpy_norm(onset))
    # where the norms agree this run is the unperturbed copy: it pins beats_with to ncref.beat_track
    res["b"] = np.array_equal(beats_with(onset, P, trim=trim, norm=kn), ref)
    return res


def qualifies(case: Case, trim: bool = True) -> bool:
    r = qualify(case, trim)
    return r["a1"] and r["a2"] and r["b"]


def _cumscore(case: Case) -> np.ndarray:
    P = float(case.P)
    ls = ncref.beat_local_score(ncref.normalize_onsets(case_onset(case)), P)
    return ncref.beat_track_dp(ls, P)[1]


def peak_count(case: Case) -> int:
    """localmax(cumscore).sum() of the oracle: what selects the kernel's median form."""
    return int(ncref.localmax(_cumscore(case)).sum())


def median_decides(case: Case) -> tuple:
    """(peaks, last beat differs from the last peak, it also differs under the lower- and the
    upper-quartile score in the median's place): whether the median's value reaches the result."""
    cum = _cumscore(case)
    peaks = np.flatnonzero(ncref.localmax(cum))
    tail = ncref.last_beat(cum)
    vals = np.sort(cum[peaks])
    off = [int(peaks[cum[peaks] >= 0.5 * vals[k]].max()) != tail for k in (len(vals) // 4, (3 * len(vals)) // 4)]
    return len(peaks), tail != peaks[-1], all(off)


# --------------------------------------------------------------------------- invariants
def check_invariants(beats, N: int, P: int) -> None:
    """What any beat list of an N-frame sequence at period P satisfies, ties or not."""
    b = np.asarray(beats, dtype=np.int64)
    assert 0 <= len(b) <= N
    if len(b):
        assert b[0] >= 0 and b[-1] < N
    gaps = np.diff(b)
    assert np.all(gaps > 0)
    dmin = int(np.round(P / 2.0))
    assert np.all((gaps >= dmin) & (gaps <= 2 * P)), (gaps.min(), gaps.max(), dmin, 2 * P)
