"""Inputs, yardsticks and numpy emulations for the tests of the tempo features: the onset
envelope (stft_mel_kernel + wtg_onset / nc_ibi_onset) and the frame-averaged tempogram
(window_tg_kernel, window_tg_slide_kernel, nc_ibi_tempogram).  No GPU in here.

Signals are deterministic float32 at whatever rate the context under test runs at (the
samples of synth.make_source are simply read at that rate).  Envelopes feed the kernels that
take an onset directly.  mel_db_f32 is the oracle's mel_db with a single-precision FFT: the
distance between it and the f64 oracle is what any honest f32 implementation shows, so it is
the yardstick the GPU's f32 quantities are held to.  The two tempogram emulations restate
csrc/nc_slide.h and csrc/nc_tgcorr.h in f64 numpy; their distance to ncref.tempogram_mean on
one onset is the yardstick for the GPU tempogram on that onset."""
from functools import lru_cache

import numpy as np
import scipy.fft

from oracle import ncref
from nightcore_analyzer import synth

N_FFT = 2048
TILE = 2048                 # TG_TB of csrc/ibi.hip: frames per tile of tg_slide_kernel
RESEED = 2.0 ** -20         # SLIDE_RESEED of csrc/nc_slide.h
WTG_SPREAD = 2.0 ** 36      # WTG_SPREAD of csrc/window_stage.hip: beyond it window_tg_kernel slides
TOL_F64 = 1e-12             # tests/test_oracle_known_answers.py: identity vs the FFT autocorrelation
TOL_TG = 2e-5               # tests/test_gpu_window.py: tempogram mean vs the oracle
RATES = {16000: 250, 22050: 344, 44100: 689, 48000: 750}   # rate -> hop-512 tempogram window


# --------------------------------------------------------------------------- signals
@lru_cache(maxsize=None)
def _source(seed):
    y = synth.make_source(42.0, seed)
    y.setflags(write=False)
    return y


def music(n, seed=1001, start=0):
    y = _source(seed)[start:start + n]
    assert len(y) == n
    return y.copy()


def clicks(n, period=21 * 512, seed=5):
    y = np.random.default_rng(seed).standard_normal(n).astype(np.float32) * np.float32(1e-3)
    y[::period] += np.float32(1.0)
    return y


def scaled(y, s):
    return (y * np.float32(s)).astype(np.float32)


def half_silent(n, seed=1001):
    y = music(n, seed)
    y[:n // 2] = 0.0
    return y


def silent(n):
    return np.zeros(n, np.float32)


def gap(sr, a, g, b, n=None, seed=1001):
    """a s of music, a 0.5 s linear fade to exact zero, g s of zeros, b s of music; cut to n."""
    na, nf, ng, nb = int(a * sr), int(0.5 * sr), int(g * sr), int(b * sr)
    y = np.zeros(na + nf + ng + nb, np.float32)
    y[:na + nf] = music(na + nf, seed)
    y[na:na + nf] *= np.linspace(1.0, 0.0, nf).astype(np.float32)
    y[na + nf + ng:] = music(nb, seed, start=na + nf)
    assert y[na + nf - 1] == 0.0 and not y[na + nf:na + nf + ng].any()
    return y if n is None else y[:n]


def head(n, seed=1001):
    y = np.zeros(n, np.float32)
    y[:n // 8] = music(n // 8, seed)
    return y


def quiet_tail(n, seed=1001):
    y = music(n, seed)
    y[n // 2:] *= np.float32(1e-3)
    return y


def first_second(n, sr, seed=1001):
    y = np.zeros(n, np.float32)
    y[:sr] = music(sr, seed)
    return y


# --------------------------------------------------------------------------- envelopes
def env_sparse(T, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random(T) * (rng.random(T) > 0.6) * 8).astype(np.float32)


def env_periodic(T):
    o = np.zeros(T, np.float32)
    o[::21] = 5.0
    return o


def env_quiet_tail(T, seed=0):
    o = env_sparse(T, seed)
    o[T // 2:] *= np.float32(1e-3)
    return o


def env_head(T, seed=0):
    o = env_sparse(T, seed)
    o[max(1, T // 8):] = 0.0
    return o


def env_zero(T):
    return np.zeros(T, np.float32)


def env_gap_fits(T, N):
    return T >= N + 128


def env_gap(T, N, seed=0):
    """Two sparse stretches with at least N exact zeros between them (needs T >= N + 128)."""
    assert env_gap_fits(T, N)
    o = env_sparse(T, seed)
    a = (T - N) // 2
    o[a:T - a] = 0.0
    assert T - 2 * a >= N and o[:a].any() and o[T - a:].any()
    return o


WELL = ("sparse", "periodic")            # bounded dynamic range: the emulations reach 1e-12
ILL = ("head", "gap")                    # a loud stretch, then exact zeros
ENVELOPES = ("sparse", "periodic", "quiet_tail", "head", "zero", "gap")


def envelope(kind, T, N):
    if kind == "gap":
        return env_gap(T, N)
    return {"sparse": env_sparse, "periodic": env_periodic, "quiet_tail": env_quiet_tail, "head": env_head,
            "zero": env_zero}[kind](T)


# --------------------------------------------------------------------------- f32 yardstick
def mel_db_f32(y, sr=22050, hop=512, n_mels=128):
    """ncref.mel_db with the frames multiplied by an f32 Hann window and transformed by a
    single-precision FFT (scipy's pocketfft on float32 input)."""
    y = np.asarray(y, dtype=np.float32)
    T = 1 + len(y) // hop
    W = ncref.mel_filter(sr, N_FFT, n_mels, 0.0, sr / 2.0)
    win = ncref.hann(N_FFT).astype(np.float32)
    out = np.empty((n_mels, T), dtype=np.float32)
    blk = max(1, (1 << 21) // N_FFT)
    for b0 in range(0, T, blk):
        b1 = min(T, b0 + blk)
        fr = ncref._frames(y, N_FFT, hop, b0, b1) * win[None, :]
        assert fr.dtype == np.float32
        X = scipy.fft.rfft(fr, axis=-1)
        assert X.dtype == np.complex64
        P = (np.abs(X) ** np.float32(2.0)).T
        assert P.dtype == np.float32
        out[:, b0:b1] = 10.0 * np.log10(np.maximum(np.float32(1e-10), W @ P))
    return out


def clamp_db(S):
    """power_to_db's top_db = 80 clamp against the global maximum (ncref.onset_strength)."""
    return np.maximum(S, S.max() - np.float32(80.0))


def onset_from_db(S, hop=512, exact=False):
    """The tail of ncref.onset_strength on an unclamped (n_mels, T) mel dB matrix.  exact: the
    mean over the bands accumulated in f64 and rounded once, instead of numpy's f32 mean."""
    T = S.shape[1]
    S = clamp_db(S)
    d = np.maximum(np.float32(0.0), S[:, 1:] - S[:, :-1])
    od = np.mean(d, axis=0, dtype=np.float64 if exact else np.float32).astype(np.float32)
    pad = 1 + N_FFT // (2 * hop)
    return np.concatenate([np.zeros(pad, dtype=np.float32), od])[:T].astype(np.float32)


def onset_yardstick(ref_onset, S32, hop=512):
    """Largest distance between the oracle's onset and the two variants of it built on
    mel_db_f32: the band mean as numpy takes it (f32, the 128 bands added one after the other:
    the reduction runs along the strided axis, so it is not pairwise) and the band mean
    accumulated exactly.  An f32 implementation is free to add the bands in any order; the first
    variant shares the oracle's order, and with it the oracle's own accumulation error (up to 6
    ulps of the onset, measured), the second does not."""
    return max(float(np.max(np.abs(ref_onset - onset_from_db(S32, hop)))),
               float(np.max(np.abs(ref_onset - onset_from_db(S32, hop, exact=True)))))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def tol_f32(yardstick, magnitude):
    """f32 level: 8 x the f32-vs-f64 distance of the oracle itself, floored at 4 f32 ulps of
    the case's largest magnitude."""
    return max(4.0 * ulp32(magnitude), 8.0 * float(yardstick))


def tol_f64(d):
    """f64 level: 8 x the emulation's own distance to the oracle, within [1e-12, 2e-5]."""
    return min(TOL_TG, max(TOL_F64, 8.0 * float(d)))


# --------------------------------------------------------------------------- emulations
def _padded(o, N, extent):
    p = N // 2
    x = np.pad(np.asarray(o, np.float32), (p, p), mode="linear_ramp", end_values=(0, 0)).astype(np.float64)
    return np.concatenate([x, np.zeros(max(0, extent - len(x)))])


def frame_rinv(x, T, N):
    """1 / ac_t[0] per frame (1 where ac_t[0] is below tiny: tg_rinv of csrc/nc_slide.h)."""
    w2 = ncref.hann(N).astype(np.float64) ** 2
    y = x[:T + N] ** 2
    ac0 = np.lib.stride_tricks.sliding_window_view(y, N)[:T] @ w2
    return np.where(ac0 < np.finfo(np.float64).tiny, 1.0, 1.0 / np.where(ac0 == 0, 1, ac0)), ac0


def sliding_tempogram_mean(o, N, tile=None, reseed=None, seeds_out=None):
    """The engine's tempogram algorithm (csrc/nc_slide.h) in numpy: five sliding f64 sums per
    lag instead of one FFT autocorrelation per frame.  tile: the sums are recomputed directly
    every `tile` frames, as tg_slide_kernel does per 2048-frame tile.  reseed: the factor of
    slide_lag_sum2's re-seeding rule (the sums are recomputed at a frame whose ac_t[0] has
    fallen below reseed x the largest ac_t[0] since the last seed); None = plain recurrences."""
    T = len(o)
    x = _padded(o, N, T + N + 1)           # x[t + N] is read for every t < T (odd N: one past the pad)
    rinv, _ = frame_rinv(x, T, N)
    th = 2 * np.pi / N
    k = np.arange(N)
    L = N - k
    c, s = np.cos(th * k), np.sin(th * k)
    A, B, C, D, E = 0.25 + 0.125 * c, -0.25 - 0.25 * c, 0.25 * s, 0.125 * c, -0.125 * s
    j = np.arange(N)
    mask = j[:, None] < L[None, :]
    e1, e2 = np.exp(1j * th * j), np.exp(2j * th * j)

    def seed(t):
        P = x[t + j][:, None] * x[np.minimum(t + j[:, None] + k[None, :], len(x) - 1)] * mask   # p_k[t + j], j < L
        return P.sum(0), (e1.real @ P) + 1j * (e1.imag @ P), (e2.real @ P) + 1j * (e2.imag @ P)

    e1L, e2L = np.exp(-1j * th * k), np.exp(-2j * th * k)
    r1, r2 = np.exp(-1j * th), np.exp(-2j * th)
    acc = np.zeros(N)
    n_seeds = 0
    for t in range(T):
        r = rinv[t]
        if t == 0 or (tile and t % tile == 0):
            S0, Z1, Z2 = seed(t)
            rmin = np.inf
            n_seeds += 1
        if reseed is not None and r != 1.0:
            if r * reseed > rmin:
                S0, Z1, Z2 = seed(t)
                rmin = r
                n_seeds += 1
            else:
                rmin = min(rmin, r)
        ac = A * S0 + B * Z1.real + C * Z1.imag + D * Z2.real + E * Z2.imag
        acc += ac * r
        pt = x[t] * x[t + k]
        pl = x[t + L] * x[t + N]
        S0 = S0 - pt + pl
        Z1 = r1 * (Z1 - pt + e1L * pl)
        Z2 = r2 * (Z2 - pt + e2L * pl)
    if seeds_out is not None:
        seeds_out.append(n_seeds)
    return acc / T


def correlation_tempogram_mean(o, N):
    """The engine's window tempogram (csrc/nc_tgcorr.h) in numpy: prefix sums of the frame
    normalisers, six sequences, and per lag three Hankel minus three Toeplitz correlations
    weighted by (1, cos theta k, sin theta k)."""
    T = len(o)
    U = T + N
    x = _padded(o, N, U)
    r, _ = frame_rinv(x, T, N)
    th = 2 * np.pi / N
    t = np.arange(T)
    Q = [np.concatenate([[0.0], np.cumsum(r * f)])
         for f in (np.ones(T), np.cos(th * t), np.sin(th * t), np.cos(2 * th * t), np.sin(2 * th * t))]
    u = np.arange(U)
    cu, su, c2u, s2u = np.cos(th * u), np.sin(th * u), np.cos(2 * th * u), np.sin(2 * th * u)

    def g(at):
        P0, Qc1, Qs1, Qc2, Qs2 = (q[at] for q in Q)
        P1, P2 = cu * Qc1 + su * Qs1, su * Qc1 - cu * Qs1
        P3, P4 = c2u * Qc2 + s2u * Qs2, s2u * Qc2 - c2u * Qs2
        return [(P0 - P1) / 4, P0 / 8 - P1 / 4 + P3 / 8, P2 / 4 - P4 / 8]

    a = [x * v for v in g(np.minimum(T - 1, u) + 1)]
    b = [x * v for v in g(np.maximum(0, u - N + 1))]
    b[2] = -b[2]
    out = np.zeros(N)
    for k in range(N):
        n = U - k
        d = [np.dot(a[i][:n], x[k:]) - np.dot(b[i][k:], x[:n]) for i in range(3)]
        out[k] = d[0] + np.cos(th * k) * d[1] + np.sin(th * k) * d[2]
    return out / T


def ac0_spread(o, N):
    """Largest / smallest ac_t[0] at or above tiny over the frames (the window kernel's
    conditioning check), 1.0 when there is none."""
    T = len(o)
    _, ac0 = frame_rinv(_padded(o, N, T + N), T, N)
    v = ac0[ac0 >= np.finfo(np.float64).tiny]
    return float(v.max() / v.min()) if len(v) else 1.0


# --------------------------------------------------------------------------- kernel choice
WT_THREADS = 512
TGC_LB = 3
WIN_TG_LDS_CAP = 160 * 1024 - 1024


def win_tg_lds_doubles(T, acw):
    """WinTgLds(T, acw).total of csrc/window_stage.hip."""
    U = T + acw
    xoff = acw + TGC_LB + 1
    xlen = U + 2 * xoff
    blocks = (acw + TGC_LB - 1) // TGC_LB
    segs = max(1, WT_THREADS // blocks)
    pre = T + acw + 2 * acw + 5 * (T + 1)
    post = segs * blocks * TGC_LB
    return xlen + 6 * U + max(pre, post)


def uses_correlation(T, acw):
    return win_tg_lds_doubles(T, acw) * 8 <= WIN_TG_LDS_CAP


def corr_T_max(acw):
    """The longest window (in frames) that launch_window_stage gives to window_tg_kernel."""
    T = 1
    while uses_correlation(T + 1, acw):
        T += 1
    return T


# --------------------------------------------------------------------------- the GPU grid
WIN_LENS = (1, 511, 512, 1535, 3071, 3072, 3073, 4095, 16384, 33280, 220500)   # group a
WINDOW_T = {22050: (1, 2, 3, 8, 9, 63, 64, 65, 431, 1247, 1248, 1300),          # group b
            44100: (862, 929), 48000: (872, 873), 16000: (313,)}
IBI_LENS = (0, 1, 63, 64, 65, 2047 * 64, (2 * 2048 + 1) * 64)                   # group c
IBI_T = (1, 2, 2047, 2048, 2049, 4096, 4097)                                    # group d
IBI_N = {64: 2756, 512: 344}
