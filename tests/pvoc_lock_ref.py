"""Identity phase locking with linked channels for the phase-vocoder stretch, in numpy float64 on
top of tests/pvoc_ref.py (DESIGN.md §4 "Phase locking"): the yardstick of
tests/test_pvoc_lock_cpu.py and tests/test_gpu_pvoc_lock.py.

All of pvoc_ref's definition stays; only the phase rule changes.  With U_k = ph(A_k):
  peaks   b is a peak of frame k iff mag[b] > mag[b-1], mag[b] > mag[b-2], mag[b] >= mag[b+1] and
          mag[b] >= mag[b+2], on the float32 magnitudes, neighbours outside 0..1024 ignored; a
          frame without one has the single peak 0,
  owners  for consecutive peaks p < q, bins b <= (p + q) div 2 belong to p, the rest to q; bins
          below the first peak belong to it, bins above the last to the last,
  scan    Phi_k = V_k on a reset frame, else Phi_k[b] = ph(Phi_{k-1}[o] M_k[b]), o = o_k[b],
          M_k[b] = V_k[b] when b == o, else V_k[o] U_k[b] conj(U_k[o]),
  linked  a group of C >= 2 equally long channels follows the scan Psi of its float32 sum m
          (channel order), analysed as a file of its own:
          Phi^c_k[b] = ph(Psi_k[b] U^c_k[b] conj(U^m_k[b])), with the channel's own mag.
"""
import numpy as np

import pvoc_ref as R
from speed_ref import speed_ref


def peaks(row) -> np.ndarray:
    """Ascending peak bins of one magnitude row (float32 comparisons)."""
    m = np.asarray(row, np.float32)
    n = len(m)
    pk = np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        pk[1:] &= m[1:] > m[:-1]
        pk[2:] &= m[2:] > m[:-2]
        pk[:-1] &= m[:-1] >= m[1:]
        pk[:-2] &= m[:-2] >= m[2:]
    idx = np.flatnonzero(pk)
    return idx if len(idx) else np.zeros(1, np.int64)


def owners(mag) -> np.ndarray:
    """o [K, bins] uint16 of magnitude rows [K, bins]."""
    mag = np.asarray(mag, np.float32)
    mag = mag.reshape(-1, mag.shape[-1])
    out = np.zeros(mag.shape, np.uint16)
    b = np.arange(mag.shape[1])
    for k, row in enumerate(mag):
        pk = peaks(row)
        cut = (pk[:-1] + pk[1:]) // 2                    # the last bin of each peak but the last
        out[k] = pk[np.searchsorted(cut, b, side="left")]
    return out


def phasors(A) -> np.ndarray:
    """U = ph(A)."""
    return R.ph(A)


def lock_scan(mag, U, V, empty, own=None) -> np.ndarray:
    """Phi [K, bins] (complex128), frame after frame; ``own``: owners to use instead of
    ``owners(mag)`` (the device's, say)."""
    U, V = np.asarray(U, np.complex128), np.asarray(V, np.complex128)
    own = owners(mag) if own is None else np.asarray(own)
    out = np.empty_like(V)
    r = R.resets(empty)
    b = np.arange(V.shape[1])
    for k in range(len(V)):
        if r[k]:
            out[k] = V[k]
            continue
        o = own[k].astype(np.int64)
        M = np.where(o == b, V[k], V[k][o] * U[k] * np.conj(U[k][o]))
        out[k] = R.ph(out[k - 1][o] * M)
    return out


def mid(xs) -> np.ndarray:
    """The float32 sum of equally long channels, in channel order."""
    xs = [np.asarray(x, np.float32) for x in xs]
    if any(len(x) != len(xs[0]) for x in xs):
        raise ValueError("linked channels must be equally long")
    m = xs[0].copy()
    for x in xs[1:]:
        m = (m + x).astype(np.float32)
    return m


def stretch_locked(xs, P: int, own=None):
    """The locked stretch of one group of channels ``xs`` (a list; one channel: rule 4), Ns
    samples each.  ``own``: the owners of the group's scan (of the channel itself, or of the sum)."""
    xs = [np.asarray(x, np.float32).astype(np.float64) for x in xs]
    Ns, K = R.plan(len(xs[0]), P)
    if K == 0:
        return [np.zeros(0) for _ in xs]
    if len(xs) == 1:
        mag, V, empty, A, _ = R.analyze(xs[0], P)
        return [R.synth(mag, lock_scan(mag.astype(np.float32), phasors(A), V, empty, own), Ns)]
    m = mid(xs).astype(np.float64)
    mag_m, V_m, empty_m, A_m, _ = R.analyze(m, P)
    U_m = phasors(A_m)
    psi = lock_scan(mag_m.astype(np.float32), U_m, V_m, empty_m, own)
    out = []
    for x in xs:
        mag, _, _, A, _ = R.analyze(x, P)
        out.append(R.synth(mag, R.ph(psi * phasors(A) * np.conj(U_m)), Ns))
    return out


def pitch_shift_locked(xs, semitones: float = None, P: int = None, own=None):
    """The group ``xs`` shifted by ``semitones`` (or by P / Q), len(x) samples each."""
    P = R.semitones_p(semitones) if P is None else int(P)
    n = len(xs[0])
    if n == 0:
        return [np.zeros(0) for _ in xs]
    return [speed_ref(s, P / R.Q)[:n] for s in stretch_locked(xs, P, own)]


# ------------------------------------------------------------------ the property tests' signals and measures
SR = 22050


def vibrato_tone():
    t = np.arange(2 * SR) / SR
    f = 440.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 5.5 * t))
    ph = 2 * np.pi * np.cumsum(f) / SR
    return sum(np.sin(h * ph) / h for h in range(1, 6))


def stereo_pair():
    rng = np.random.default_rng(3)
    t = np.arange(3 * SR) / SR
    f = 330.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(f) / SR
    s = 0.3 * sum(np.sin(h * ph) / h for h in range(1, 8)) + 0.05 * rng.standard_normal(len(t))
    left = s + 0.02 * rng.standard_normal(len(t))
    right = 0.7 * s + 0.02 * rng.standard_normal(len(t))
    return left, right


def rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, np.float64)))))


def running_rms_spread(v, w=512):
    """min / max of the rms over every window of ``w`` consecutive samples."""
    c = np.concatenate([[0.0], np.cumsum(np.square(np.asarray(v, np.float64)))])
    r = np.sqrt((c[w:] - c[:-w]) / w)
    return float(r.min() / r.max())


def unexplained(a, b):
    """The part of b that a gain times a does not explain."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = np.dot(a, b) / np.dot(a, a)
    return float(np.sqrt(np.mean(np.square(b - g * a)) / np.mean(np.square(b))))
