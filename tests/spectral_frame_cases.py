"""Inputs, per-frame references and derived bounds for the stage test of spectral_frames_kernel
(csrc/spectral.hip behind nc_spectral_stats): what the kernel writes for every frame, the dB row
and the record of centroid, rolloff, five band sums and max |X|, and the frame RMS.  No GPU in
here.

The reference is refglue.spectral_analyze(detail=True): librosa's f64 FFT rounded to complex64,
per-frame centroid, rolloff, rms and the magnitudes S[k, t].  Inputs are finite; NaN and Inf
samples are out of scope.

One number is measured, EPS_MEASURED: the largest |10^(row / 20) - S| / max_k S[:, t] over the
non-silent frames and the bins at or above the dB floor (S >= 1e-5), device dB rows against the
oracle's S over all cases on an MI355X (test_gpu_spectral_frames.py prints it).  It is the f32
FFT's rounding, a property of the input and the transform length, not of the code that follows
the FFT.  EPS = 4 x EPS_MEASURED is the tolerance, and everything else follows from it with no
further measured number (E = EPS * max_k S[:, t] is the error of one bin of frame t):

  magnitudes    |10^(row / 20) - S[k]| <= E + 2e-6 S[k]  (log10f and the f64 exponential)
  max |X|       |max - max S| <= E
  band sums     |sum - sum S[lo:hi]| <= (hi - lo) E + 2e-5 ref  (f32 partial sums of <= 17 terms)
  frame RMS     relative 2e-6, the figure of test_gpu_spectral.py
  centroid      c' - c = hz sum_k (k - c / hz) d_k / (l1 + sum_k d_k) with |d_k| <= E, so
                |c' - c| <= hz E sum_k |k - c / hz| / (l1 - 1025 E), where l1 > 2050 E; else the
                cruder hz E (sum k + 1024 * 1025) / l1.  Plus 2e-5 ref.
  rolloff       the device names the first bin k whose running sum c'[k] reaches 0.85 total'.
                With d_j the bin errors, c'[k] - 0.85 total' - (c[k] - 0.85 total) =
                0.15 sum_{j<=k} d_j - 0.85 sum_{j>k} d_j, at most E (0.15 (k + 1) + 0.85 (1024 - k))
                in size; the f32 running sum of 1025 terms and the threshold's product add at
                most 1025 * 2^-24 total.  With err[k] the sum of the two, bin k can be the first
                crossing only from the first k with c[k] + err[k] >= 0.85 total (f64 sums of S)
                up to the first k with c[k] - err[k] >= 0.85 total.  This is never wider than
                delta = 1025 * 2^-24 + 1025 EPS either side of 0.85 in units of the total.  The
                device bin must be admissible on every frame.

test_spectral_frame_cases_cpu.py shows that the rolloff condition is sharp: on at least three
quarters of each case's frames one bin only is admissible, and on no frame more than two.
Silent frames (all samples zero) are exact: every number 0, the dB row -100.0.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import refglue

EPS_MEASURED = 7.56e-7         # measured on an MI355X: 7.560e-7 (tone_quiet_noise; the other cases 1.4e-7 .. 7.4e-7)
EPS = 4.0 * EPS_MEASURED
EPS_CEILING = 1e-5             # a measured value above this is a finding, not a tolerance
ROLL = 0.85
NBINS = 1025
FLOOR = 1e-5                   # the dB row's floor: 10 log10(1e-10) = -100 dB
BANDS = ((20, 80), (80, 250), (250, 2000), (2000, 6000), (6000, 20000))     # spectral.py:70-74

Ref = namedtuple("Ref", "S centroid rolloff rms hz bands silent")


TONE = 0.06                    # beside noise at 0.05: the 85 % point lies among the noise bins, max S / total is small


def _tone_noise(n, sr, f0, noise, seed, amp=TONE):
    t = np.arange(n, dtype=np.float64) / sr
    y = amp * np.sin(2 * np.pi * f0 * t) + noise * np.random.default_rng(seed).standard_normal(n)
    return y.astype(np.float32)


def _gap():
    """Noise, half a second of exact zeros (silent frames inside a file), noise again."""
    y = _tone_noise(22050, 22050, 330.0, 0.05, 8113).copy()
    y[6000:17000] = 0.0
    return y


# the seeds of the short files are chosen so that every one of their few frames has a single
# admissible rolloff bin (test_spectral_frame_cases_cpu.py holds them to it)
CASES = {
    "tone_noise": lambda: (_tone_noise(2 * 22050, 22050, 220.0, 0.05, 8101), 22050),
    "noise": lambda: (_tone_noise(33075, 22050, 220.0, 0.1, 8102, amp=0.0), 22050),
    "tone_quiet_noise": lambda: (_tone_noise(2 * 22050, 22050, 440.0, 1e-3, 8103, amp=0.3), 22050),
    "short_1": lambda: (_tone_noise(1, 22050, 220.0, 0.05, 8111) + np.float32(0.1), 22050),
    "short_511": lambda: (_tone_noise(511, 22050, 440.0, 0.05, 8113), 22050),
    "short_512": lambda: (_tone_noise(512, 22050, 660.0, 0.05, 8112), 22050),
    "short_600": lambda: (_tone_noise(600, 22050, 880.0, 0.05, 8114), 22050),
    "short_2048": lambda: (_tone_noise(2048, 22050, 1100.0, 0.05, 8116), 22050),
    "zeros": lambda: (np.zeros(22050 // 4, np.float32), 22050),
    "rate_44100": lambda: (_tone_noise(44100, 44100, 220.0, 0.05, 8104), 44100),
    "rate_48000": lambda: (_tone_noise(48000, 48000, 220.0, 0.05, 8105), 48000),
    "gap": lambda: (_gap(), 22050),
}
NAMES = tuple(CASES)


@lru_cache(maxsize=None)
def signal(name):
    y, sr = CASES[name]()
    y = np.ascontiguousarray(y, np.float32)
    assert np.all(np.isfinite(y)) and len(y) <= 2 * sr
    y.setflags(write=False)
    return y, sr


def band_bins(sr):
    """[lo, hi) bins of each band mask (freqs >= lo) & (freqs < hi), (0, 0) for an empty one."""
    freqs = np.fft.rfftfreq(2048, 1.0 / sr)
    out = []
    for lo, hi in BANDS:
        idx = np.flatnonzero((freqs >= lo) & (freqs < hi))
        out.append((int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0))
    return tuple(out)


@lru_cache(maxsize=None)
def reference(name):
    """Per-frame reference of a case: S [1025, T] as f64, centroid, rolloff (Hz), rms, and which
    frames are silent (no non-zero sample under the centred 2048-sample frame)."""
    y, sr = signal(name)
    _, det = refglue.spectral_analyze(y, sr, detail=True)
    S = np.asarray(det["S"], np.float64)
    T = S.shape[1]
    assert T == 1 + len(y) // 512
    nz = np.concatenate([np.zeros(1024, bool), y != 0, np.zeros(1024 + 512, bool)])
    silent = np.array([not nz[512 * t:512 * t + 2048].any() for t in range(T)])
    assert np.array_equal(silent, S.max(axis=0) == 0.0)
    hz = float(np.fft.rfftfreq(2048, 1.0 / sr)[1])
    return Ref(S, np.asarray(det["centroid"], np.float64), np.asarray(det["rolloff"], np.float64),
               np.asarray(det["rms"], np.float32), hz, band_bins(sr), silent)


# --------------------------------------------------------------------------- derived bounds
def bin_error(S, eps=EPS):
    """E[t] = eps * max_k S[k, t]."""
    return eps * S.max(axis=0)


def rolloff_err(S, eps=EPS):
    """err[k, t]: how far c'[k] - 0.85 total' may stand from c[k] - 0.85 total (module docstring)."""
    k = np.arange(NBINS, dtype=np.float64)[:, None]
    return NBINS * 2.0 ** -24 * S.sum(axis=0)[None, :] + bin_error(S, eps)[None, :] * ((1 - ROLL) * (k + 1) + ROLL * (1024 - k))


def admissible_rolloff(S, eps=EPS):
    """(lo[t], hi[t]): the bins the device's rolloff may name on frame t, both inclusive."""
    cum = np.cumsum(S, axis=0)
    thr = ROLL * cum[-1][None, :]
    err = rolloff_err(S, eps)
    lo = np.argmax(cum + err >= thr, axis=0)
    hi = np.argmax(cum - err >= thr, axis=0)
    return lo, hi


def centroid_bound(S, hz, centroid, eps=EPS):
    """The largest |device centroid - reference| on each frame that bin errors of E allow."""
    E = bin_error(S, eps)
    l1 = S.sum(axis=0)
    k = np.arange(NBINS, dtype=np.float64)[:, None]
    spread = np.abs(k - centroid[None, :] / hz).sum(axis=0)
    crude = hz * E * (k.sum() + 1024.0 * 1025.0) / np.where(l1 > 0, l1, 1.0)
    fine = hz * E * spread / np.where(l1 > 2 * NBINS * E, l1 - NBINS * E, 1.0)
    return np.where(l1 > 2 * NBINS * E, np.minimum(fine, crude), crude) + 2e-5 * np.abs(centroid)


def band_bound(S, bands, eps=EPS):
    """(ref[5, T], bound[5, T]) of the band sums."""
    E = bin_error(S, eps)
    ref = np.array([S[lo:hi].sum(axis=0) for lo, hi in bands])
    return ref, np.array([(hi - lo) * E for lo, hi in bands]) + 2e-5 * ref
