"""The speed renderer's definition in numpy float64 (render section), evaluated
directly: the yardstick of tests/test_render_cpu.py and tests/test_gpu_render.py.

For x[0..n) (zero outside) and a factor F in [0.25, 4]:
  P = round(F Q), n_out = ceil(n Q / P), c = ROLL min(1, Q / P),
  t_m = (m P div Q) + ((m P mod Q) / Q)                       (exact integer arithmetic),
  h(u) = c sinc(c u) I0(BETA sqrt(1 - (c u / Z)^2)) / I0(BETA)  for |c u| < Z, else 0,
  y[m] = sum_j x[j] h(t_m - j).
"""
import numpy as np

Q = 1_000_000
Z = 32
BETA = 10.06
ROLL = 0.9


def plan(n: int, F: float):
    """(P, n_out, c) of an n-sample input at factor F."""
    P = int(round(float(F) * Q))
    if not Q // 4 <= P <= 4 * Q:
        raise ValueError("factor outside [0.25, 4]")
    n_out = -(-int(n) * Q // P)
    return P, n_out, ROLL * min(1.0, Q / P)


def kernel(u: np.ndarray, c: float) -> np.ndarray:
    """h(u) of the definition (float64)."""
    v = c * np.asarray(u, np.float64)
    inside = np.abs(v) < Z
    w = np.i0(BETA * np.sqrt(np.clip(1.0 - (v / Z) ** 2, 0.0, None))) / np.i0(BETA)
    return np.where(inside, c * np.sinc(v) * w, 0.0)


def speed_ref(x, F: float, m0: int = 0, m1=None, base: int = 0, n=None) -> np.ndarray:
    """y[m0:m1] of the definition in float64.  ``x`` holds samples base .. base + len(x) of a
    file of ``n`` samples (default: the whole file); outputs whose taps reach outside the
    slice (but inside the file) are the caller's to avoid."""
    x = np.asarray(x, np.float64)
    n = len(x) + base if n is None else int(n)
    P, n_out, c = plan(n, F)
    m1 = n_out if m1 is None else min(int(m1), n_out)
    H = int(np.ceil(Z / c))
    q = np.arange(-H - 1, H + 2, dtype=np.int64)
    out = np.zeros(max(0, m1 - m0))
    for a in range(m0, m1, 8192):
        m = np.arange(a, min(m1, a + 8192), dtype=np.int64)
        pos = m * P
        i0, fr = pos // Q, (pos % Q) / Q
        j = i0[:, None] + q[None, :]
        h = kernel(fr[:, None] - q[None, :], c)              # t_m - j = (i0 - j) + fr
        k = j - base
        ok = (j >= 0) & (j < n) & (k >= 0) & (k < len(x))
        out[a - m0:a - m0 + len(m)] = np.sum(np.where(ok, x[np.clip(k, 0, max(0, len(x) - 1))], 0.0) * h, axis=1)
    return out
