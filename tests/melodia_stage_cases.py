"""Inputs and CPU references for the stage tests of melodia_salience_kernel (csrc/melodia.hip behind
nc_melodia_salience / nc_melodia_probe).  No GPU in here; test_melodia_stage_cases_cpu.py proves
from the oracle alone that every case does what it is here for, test_gpu_melodia_stages.py runs
them on the device.

Files are short (at most ~50 frames), 22050 Hz and hop 128 unless the name says otherwise; a case
is one launch: a tuple of files (all but ``batch`` hold one).  The whole-chain comparison needs
inputs on which an f32 spectrum decides what an f64 spectrum decides, and three things about the
files serve that (each explained where it is done): the tonal files fade in and out (_faded), the
constant of ``dc`` carries a weak tone (_dc), and ``threshold``, whose peaks straddle the 40 dB
threshold on purpose, is kept to the stage tests (WHOLE_CHAIN).

Per frame two CPU references, both through oracle/melodia_ref.py:
  * the f64 chain: the oracle's own spectrum (np.fft.rfft of the f64 product of frame and window);
  * the f32 chain: the same oracle stages on an f32 CPU spectrum, |scipy.fft.rfft| of the float32
    windowed, zero-padded frame (complex64 throughout).  It is what an f32 FFT that is not the
    device's does to the result, so its distance from the f64 chain is the yardstick for the
    device's: the device is allowed 4 x that distance (another butterfly order, table twiddles, an
    fmaf in the magnitude), in the spectrum and in the saliences at the end of the chain, case by
    case (yardsticks).

Frame classes, from the f32 windowed frame (the product the kernel forms):
  silent      no non-zero sample: every stage's output is exactly zero / empty;
  degenerate  exactly one non-zero sample: a flat spectrum whose local maxima, and every salience
              peak built on them, are rounding noise in the oracle and on the device alike.
              window()[0] == 0, so this is the last frame of a file whose length is 2 (mod hop)
              (two_tone_2, its copy in the batch, short_2) and every non-silent frame of a
              one-sample file (short_1 and its copy in the batch).  The stage-by-stage tests hold
              on these frames like on any other (each stage is checked on the device's own
              previous stage); only the comparison of the whole chain with the f64 oracle does not.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import scipy.fft

from oracle import melodia_ref as R

SR, HOP = 22050, 128
MIN_BIN = int(R.cent_bin(80.0))          # 65: the lower edge of the salience peaks


def _noise(n, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


RAMP = 256


def _faded(x):
    """x with sin^2 ramps of RAMP samples at both ends, never reaching zero.  A tone or a constant
    that is cut off abruptly leaves, on the file's first and last frames, a spectrum that runs
    flat towards Nyquist at -30 dB or so: no local maximum in f64, rounding-noise maxima within
    40 dB of the largest peak in any f32 FFT.  Such frames say nothing about the kernel (see the
    99 % condition in test_melodia_stage_cases_cpu.py), so the tonal files fade."""
    n = len(x)
    i = np.arange(n, dtype=np.float64)
    ramp = np.sin(0.5 * np.pi * np.minimum(1.0, np.minimum(i + 1, n - i) / (RAMP + 1))) ** 2
    return x * ramp


def _tones(n, sr, parts):
    t = np.arange(n, dtype=np.float64) / sr
    return _faded(sum(a * np.sin(2 * np.pi * f * t) for f, a in parts)).astype(np.float32)


def _two_tone(n, sr=SR):
    return _tones(n, sr, ((220.0, 0.5), (440.0, 0.2)))


def _dc(n):
    """A constant 0.5 under a 440 Hz sine of 0.1.  The constant's bin-0 maximum, ten times the
    tone's peak, is no candidate (were it one, the 40 dB threshold would rise tenfold and cut the
    tone's side lobes).  The constant alone leaves only its own side lobes as candidates, ripples
    at 1e-5 of the spectrum's maximum on the faded frames, where an f32 spectrum is good to a
    per cent of their height: a 28-frame device run lost three of them."""
    t = np.arange(n, dtype=np.float64) / SR
    return _faded(0.5 + 0.1 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)


def _threshold(n):
    """A 440 Hz tone of 0.5 and 24 weak tones, 150 Hz apart from 1000 Hz, at 0.94 % to 1.055 % of
    it in steps of 0.005 %-points: spectral peaks either side of the 40 dB threshold (1 % of the
    largest peak), so that a threshold off by a per cent keeps or drops another set of them."""
    parts = [(440.0, 0.5)] + [(1000.0 + 150.0 * i, 0.5 * (0.0094 + 0.00005 * i)) for i in range(24)]
    return _tones(n, SR, parts)


TONE_LEN = 2560                         # frames 8..12 lie wholly inside the file
SHORT = (1, 2, 127, 128, 129, 1023, 1024, 1025)

# name -> (samples, sample rate, hop)
FILES = {
    "silence": lambda: (np.zeros(3000, np.float32), SR, HOP),
    "zeros_300": lambda: (np.zeros(300, np.float32), SR, HOP),
    **{f"short_{n}": (lambda n=n: (_noise(n, 9100 + n), SR, HOP)) for n in SHORT},
    **{f"two_tone_{d}": (lambda d=d: (_two_tone(128 * 40 + d), SR, HOP)) for d in range(4)},
    "noise": lambda: (_noise(4096, 9001), SR, HOP),
    "low_tone": lambda: (_tones(TONE_LEN, SR, [(60.0 * (h + 1), 0.3 / (h + 1)) for h in range(9)]), SR, HOP),
    "edge_79": lambda: (_tones(TONE_LEN, SR, ((79.0, 0.5),)), SR, HOP),
    "edge_80": lambda: (_tones(TONE_LEN, SR, ((80.2, 0.5),)), SR, HOP),
    "high_tone": lambda: (_tones(TONE_LEN, SR, ((3000.0, 0.5),)), SR, HOP),
    "dc": lambda: (_dc(TONE_LEN), SR, HOP),
    "threshold": lambda: (_threshold(TONE_LEN), SR, HOP),
    "rate": lambda: (_two_tone(128 * 40, 44100), 44100, 256),
}
CASES = {name: (name,) for name in FILES if name != "zeros_300"}
CASES["batch"] = ("noise", "zeros_300", "two_tone_2", "short_1")
NAMES = tuple(CASES)
# the threshold case is for the stage tests alone: its frames are, by construction, the ones on
# which a spectrum error of 2e-7 of the largest peak can carry a 1 % peak across the 40 dB
# threshold (one peak per 0.5 % of it), and a peak kept on one side only moves the saliences by
# 1e-4.  An MI355X run had the f64 oracle's bin set on all its 28 frames and such a peak on one.
WHOLE_CHAIN = tuple(n for n in NAMES if n != "threshold")
# the whole chain must give the f64 oracle's bin set on every frame of these
EXACT_SET_CASES = tuple(f"two_tone_{d}" for d in range(4)) + ("edge_79", "edge_80", "high_tone", "dc", "silence")


@lru_cache(maxsize=None)
def signal(fname):
    y, sr, hop = FILES[fname]()
    y = np.ascontiguousarray(y, np.float32)
    assert np.all(np.isfinite(y))
    y.setflags(write=False)
    return y, sr, hop


def case_files(name):
    """The files of a case, and its (sample rate, hop) (one per launch)."""
    sigs = [signal(f) for f in CASES[name]]
    assert len({(sr, hop) for _, sr, hop in sigs}) == 1
    return [y for y, _, _ in sigs], sigs[0][1], sigs[0][2]


def frame_f32(y, t, hop):
    """The float32 windowed frame t, zero-padded to 8192: the kernel's stage-1 product."""
    win = R.window()
    s0 = t * hop - R.FRAME // 2
    fr = np.zeros(R.FFT, np.float32)
    a, b = max(0, s0), min(len(y), s0 + R.FRAME)
    if b > a:
        fr[a - s0:b - s0] = y[a:b] * win[a - s0:b - s0]
    return fr


def chain(mag, sr, key_dtype=np.float64):
    """The oracle's stages after the spectrum: (bins, saliences) of the salience peaks."""
    f, a = R.spectral_peaks(mag, sr, key_dtype=key_dtype)
    return R.salience_peaks(R.salience(f, a), MIN_BIN, key_dtype=key_dtype)


def frame_mag32(y, t, hop):
    """The f32 CPU spectrum of frame t, widened to f64 for the oracle's stages."""
    spec = scipy.fft.rfft(frame_f32(y, t, hop))
    assert spec.dtype == np.complex64
    return np.abs(spec).astype(np.float64)


# mag64 / mag32 [T, 4097] f64 (mag32: the f32 CPU spectrum, widened); peaks64 / peaks32: per frame
# (bins, saliences) of the two chains; silent / degenerate [T] bool
Ref = namedtuple("Ref", "T mag64 mag32 peaks64 peaks32 silent degenerate")


@lru_cache(maxsize=None)
def reference(fname):
    y, sr, hop = signal(fname)
    T = R.n_frames(len(y), hop)
    mag64 = np.zeros((T, R.FFT // 2 + 1))
    mag32 = np.zeros((T, R.FFT // 2 + 1))
    nz = np.zeros(T, np.int64)
    peaks64, peaks32 = [], []
    for t in range(T):
        fr = frame_f32(y, t, hop)
        nz[t] = np.count_nonzero(fr)
        mag64[t] = R.frame_mag(y, t, hop)
        mag32[t] = frame_mag32(y, t, hop)
        peaks64.append(chain(mag64[t], float(sr)))
        peaks32.append(chain(mag32[t], float(sr)))
    for arr in (mag64, mag32):
        arr.setflags(write=False)
    return Ref(T, mag64, mag32, tuple(peaks64), tuple(peaks32), nz == 0, nz == 1)


def spectrum_error(mag, ref64):
    """max_k |mag - mag64| / max_k mag64 of one frame."""
    return float(np.max(np.abs(np.asarray(mag, np.float64) - ref64)) / ref64.max())


def salience_deviation(got, ref):
    """(same bin set?, the largest |salience - reference| over the common bins / the reference
    frame's largest salience) of one frame; got and ref are (bins, saliences)."""
    gb, gs = np.asarray(got[0]).astype(np.int64), np.asarray(got[1], np.float64)
    rb, rs = np.asarray(ref[0]).astype(np.int64), np.asarray(ref[1], np.float64)
    same = sorted(gb.tolist()) == sorted(rb.tolist())
    r = dict(zip(rb.tolist(), rs.tolist()))
    dev = max((abs(s - r[b]) for b, s in zip(gb.tolist(), gs.tolist()) if b in r), default=0.0)
    return same, (dev / rs.max() if len(rs) else 0.0)


def as_output(peaks):
    """(bins, saliences) as the kernel hands them out: saliences rounded to float32."""
    return peaks[0], np.asarray(peaks[1], np.float64).astype(np.float32).astype(np.float64)


Yard = namedtuple("Yard", "spec sal agree frames")


@lru_cache(maxsize=None)
def yardsticks(fnames=tuple(FILES)):
    """What the f32 chain shows against the f64 chain over the frames of the files ``fnames``:
      spec    the largest spectrum_error of the f32 CPU spectrum on the non-silent frames;
      sal     the largest salience_deviation of the f32 chain's output (as_output: the kernel's
              output format is part of the comparison) on the non-degenerate frames where its bin
              set is the f64 chain's.  A frame on which the sets differ has another spectral peak
              kept, dropped or binned elsewhere, which moves the common bins by far more than
              rounding does; the agreement count is the check for those frames;
      agree, frames   non-degenerate frames with the same bin set, and all non-degenerate frames.
    The device is held to 4 x spec and 4 x sal over the same frames."""
    spec = sal = 0.0
    agree = frames = 0
    for fname in fnames:
        r = reference(fname)
        for t in range(r.T):
            if not r.silent[t]:
                spec = max(spec, spectrum_error(r.mag32[t], r.mag64[t]))
            if not r.degenerate[t]:
                same, d = salience_deviation(as_output(r.peaks32[t]), r.peaks64[t])
                agree += same
                frames += 1
                if same:
                    sal = max(sal, d)
    return Yard(spec, sal, agree, frames)
