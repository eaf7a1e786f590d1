"""The phase-vocoder pitch shift's definition in numpy float64 ("Pitch shift"),
evaluated directly: the yardstick of tests/test_pvoc_cpu.py and tests/test_gpu_pvoc.py.

N = 2048, Hs = 512, Q = 10^6, W[j] = 0.5 - 0.5 cos(2 pi j / N), P = round(2^(S / 12) Q).
For x[0..n) (zero outside); every integer division is a floor division:
  Ns = ceil(n P / Q), J = ceil(Ns / Hs), K = J + 3 (0 for an empty file),
  c_k = (k - 1) Hs, u_k = (c_k Q) div P,
  A_k = rfft(x[u_k - N/2 + i] W[i]), B_k = the frame Hs samples earlier, mag_k = |A_k|,
  empty_k = every x[i] with u_k - N/2 < i < u_k + N/2 is zero, reset_k = (k == 0) or empty_{k-1},
  ph(z) = z / |z|, (1, 0) when |z| is 0 or not finite,
  V_k = ph(A_k) on a reset frame, else ph(A_k conj(B_k)),
  Phi_k = V_k on a reset frame, else ph(Phi_{k-1} V_k),
  f_k[i] = irfft(mag_k Phi_k)[i] W[i] 2/3,
  s[m] = sum_{k = j .. j+3} f_k[m - (k - 3) Hs], j = m div Hs, m < Ns, ascending k,
  y = speed_render(s, P)[0:n].
"""
import numpy as np

from speed_ref import speed_ref

N = 2048
HS = 512
Q = 1_000_000
BINS = N // 2 + 1
W = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def semitones_p(semitones: float) -> int:
    """P = round(2^(S / 12) Q), |S| <= 12."""
    if not abs(float(semitones)) <= 12.0:
        raise ValueError("pitch shift outside [-12, 12] semitones")
    return int(round(2.0 ** (float(semitones) / 12.0) * Q))


def plan(n: int, P: int):
    """(Ns, K) of an n-sample file at ratio P / Q."""
    if not Q // 2 <= P <= 2 * Q:
        raise ValueError("P outside [500000, 2000000]")
    n = int(n)
    if n <= 0:
        return 0, 0
    Ns = -(-n * P // Q)
    return Ns, -(-Ns // HS) + 3


def centres(K: int, P: int, k0: int = 0) -> np.ndarray:
    """u_k for k0 <= k < K (Python integers: c_k Q passes 2^40)."""
    return np.array([((k - 1) * HS * Q) // P for k in range(k0, K)], dtype=np.int64)


def _frames(x, starts, base=0):
    """x[start + i], i < N, zero outside the slice x = file[base : base + len(x)]."""
    x = np.asarray(x, np.float64)
    idx = np.asarray(starts, np.int64)[:, None] - base + np.arange(N)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, max(0, len(x) - 1))] if len(x) else 0.0, 0.0)


def ph(z):
    """z / |z|; (1, 0) where |z| is 0 or not finite."""
    z = np.asarray(z, np.complex128)
    a = np.abs(z)
    ok = (a > 0) & np.isfinite(a)
    return np.where(ok, z / np.where(ok, a, 1.0), 1.0 + 0.0j)


def analyze(x, P: int, k0: int = 0, base: int = 0, n=None):
    """(mag [K', 1025], V [K', 1025] complex, empty [K'] bool, A, B) of frames k0 .. K - 1.
    ``x`` holds samples base .. base + len(x) of a file of ``n`` samples (default: the whole
    file); with k0 > 0 the slice must cover frame k0 - 1's span as well (its empty flag decides
    frame k0's reset)."""
    x = np.asarray(x, np.float64)
    n = len(x) + base if n is None else int(n)
    _, K = plan(n, P)
    if K - k0 <= 0:
        z = np.zeros((0, BINS))
        return z, z.astype(np.complex128), np.zeros(0, bool), z.astype(np.complex128), z.astype(np.complex128)
    u = centres(K, P, k0)
    fa = _frames(x, u - N // 2, base)
    fb = _frames(x, u - N // 2 - HS, base)
    empty = ~np.any(fa[:, 1:] != 0.0, axis=1)
    if k0 == 0:
        reset = np.concatenate([[True], empty[:-1]])
    else:
        prev = _frames(x, centres(k0, P, k0 - 1) - N // 2, base)
        reset = np.concatenate([~np.any(prev[:, 1:] != 0.0, axis=1), empty[:-1]])
    A = np.fft.rfft(fa * W, axis=1)
    B = np.fft.rfft(fb * W, axis=1)
    V = np.where(reset[:, None], ph(A), ph(A * np.conj(B)))
    return np.abs(A), V, empty, A, B


def resets(empty) -> np.ndarray:
    empty = np.asarray(empty, bool)
    return np.concatenate([[True], empty[:-1]]) if len(empty) else np.zeros(0, bool)


def scan(V, empty) -> np.ndarray:
    """Phi [K, bins] (complex128), frame after frame."""
    V = np.asarray(V, np.complex128)
    out = np.empty_like(V)
    r = resets(empty)
    for k in range(len(V)):
        out[k] = V[k] if r[k] else ph(out[k - 1] * V[k])
    return out


def synth(mag, Phi, Ns: int) -> np.ndarray:
    """s[0..Ns) from K = ceil(Ns / Hs) + 3 frames."""
    Y = np.asarray(mag, np.float64) * np.asarray(Phi, np.complex128)
    K = len(Y)
    if Ns <= 0:
        return np.zeros(0)
    Y = Y.copy()
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    f = np.fft.irfft(Y, n=N, axis=1) * W * (2.0 / 3.0)
    J = K - 3
    s = np.zeros(J * HS)
    blocks = s.reshape(J, HS)
    for d in range(4):                      # frame k = j + d, ascending
        blocks += f[d:d + J, (3 - d) * HS:(4 - d) * HS]
    return s[:Ns]


def stretch(x, P: int) -> np.ndarray:
    """The time stretch by P / Q: Ns samples."""
    x = np.asarray(x, np.float64)
    Ns, K = plan(len(x), P)
    if K == 0:
        return np.zeros(0)
    mag, V, empty, _, _ = analyze(x, P)
    return synth(mag, scan(V, empty), Ns)


def pitch_shift(x, semitones: float = None, P: int = None) -> np.ndarray:
    """x shifted by ``semitones`` (or by the ratio P / Q), len(x) samples."""
    P = semitones_p(semitones) if P is None else int(P)
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros(0)
    return speed_ref(stretch(x, P), P / Q)[:len(x)]
