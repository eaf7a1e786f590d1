"""Inputs and an exact reference for the stage tests of the silence trim and the window energies
(csrc/trim.hip behind nc_trim_bounds and nc_window_energy_blocks, window_energy_kernel of
csrc/glue.hip behind nc_window_energy).  No GPU in here.

exact_trim(y, top_db) restates the header of csrc/trim.hip in f64: the sums of squares of the
512-sample blocks by math.fsum (correctly rounded), a frame's mean as the f64 sum of its blocks
t-2 .. t+1 (zero outside the file) over 2048, dB and bounds from those.  It returns the bounds,
the block sums and the margin min_t |db[t] + top_db|: how far the closest frame stands from the
threshold.  The oracle (ncref.trim, librosa's f32 arithmetic) and the kernel (f64 sums rounded
to f32, sqrtf, log10f) both differ from it by f32 rounding only, below 1e-4 dB in all (sqrtf and
r * r about 5e-7 dB, 10 log10f at magnitudes up to 100 about 2e-5 dB, the subtraction about
4e-6 dB, librosa's pairwise f32 mean of 2048 terms about 3e-6 dB).  With every margin at least
MARGIN_DB = 1e-3 dB (test_trim_cases_cpu.py) no frame can fall on the other side of a threshold,
so the GPU tests demand the exact bounds of every case at every top_db.

Inputs are finite.  NaN and Inf samples are out of scope: librosa propagates them through the
maximum, and neither the reference nor the kernels promise anything for them.

Noise is Gaussian; an "amplitude" is its standard deviation.  Bodies are at 0.08 (-21.9 dB), so
that exact zeros (clamped to -100 dB, 78 dB below the body) stand clear of every top_db.
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

HOP = 512
FRAME = 2048
TOP_DBS = (20.0, 40.0, 60.0, 80.0)
MARGIN_DB = 1e-3
BODY = 0.08
TR_BPG = 16            # csrc/trim.hip: 512-sample blocks per workgroup tile of trim_blocks_kernel

Exact = namedtuple("Exact", "bounds blocks margin db")


# --------------------------------------------------------------------------- exact reference
def block_sums(y):
    """math.fsum of the f64 squares of each 512-sample block of y (the last one may be partial)."""
    sq = np.asarray(y, np.float32).astype(np.float64) ** 2
    return np.array([math.fsum(sq[b:b + HOP].tolist()) for b in range(0, len(sq), HOP)], np.float64)


def frame_db(blocks, n):
    """db[t] of the 1 + n // 512 centred frames of a file of n samples with these block sums."""
    T = 1 + n // HOP
    padded = np.concatenate([np.zeros(2), blocks, np.zeros(max(0, T + 2 - len(blocks)))])
    ms = np.array([(padded[t] + padded[t + 1] + padded[t + 2] + padded[t + 3]) for t in range(T)]) / float(FRAME)
    rms = np.sqrt(ms)
    ref = rms.max()
    return 10.0 * np.log10(np.maximum(1e-10, rms * rms)) - 10.0 * np.log10(max(1e-10, ref * ref))


def exact_trim(y, top_db):
    """-> Exact((start, end), block sums, margin in dB, db[t]) of one file, all in f64."""
    n = len(y)
    blocks = block_sums(y)
    db = frame_db(blocks, n)
    nz = np.flatnonzero(db > -top_db)
    bounds = (int(nz[0]) * HOP, min(n, (int(nz[-1]) + 1) * HOP)) if nz.size else (0, 0)
    return Exact(bounds, blocks, float(np.min(np.abs(db + top_db))), db)


def exact_energy_db(x):
    """io._rms_db of a window in f64 with a correctly rounded sum: 20 log10(max(sqrt(E / L), 1e-10))."""
    sq = np.asarray(x, np.float32).astype(np.float64) ** 2
    return 20.0 * math.log10(max(math.sqrt(math.fsum(sq.tolist()) / len(sq)), 1e-10))


def frame_base(lens):
    """Exclusive scan of the files' frame counts 1 + N // 512, [n + 1]."""
    lens = np.asarray(lens, np.int64)
    return np.concatenate([[0], np.cumsum(1 + lens // HOP)]).astype(np.int64)


def tile_base(lens):
    """Exclusive scan of the files' tile counts ceil(ceil(N / 512) / 16), [n + 1]."""
    nblk = (np.asarray(lens, np.int64) + HOP - 1) // HOP
    return np.concatenate([[0], np.cumsum((nblk + TR_BPG - 1) // TR_BPG)]).astype(np.int64)


# --------------------------------------------------------------------------- cases
def _noise(rng, n, amp):
    return (amp * rng.standard_normal(n)).astype(np.float32)


def _db(x):
    return 10.0 ** (x / 20.0)


LENGTHS = (0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 2047, 2048, 2049, 2560, 8191, 8192, 8193, 32775)
# 3000 + s: where the body starts.  51 and 52 put 21 and 20 body samples into frame 4, either
# side of the 1 % of a frame that top_db = 20 asks for
STEPS = (0, 1, 20, 21, 22, 51, 52, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 2047, 2048)


def _length(n):
    """A noise body of n samples whose first third is 50 dB down: top_db = 20 and 40 cut it off."""
    def make():
        y = _noise(np.random.default_rng(7000 + n), n, BODY)
        y[:n // 3] *= np.float32(_db(-50.0))
        return y
    return make


def _step(s):
    def make():
        rng = np.random.default_rng(7100 + s)
        return np.concatenate([np.zeros(3000 + s, np.float32), _noise(rng, 6000, BODY), np.zeros(3100, np.float32)])
    return make


def _fades():
    """30 frames linear in dB from -90 dB (3 dB a frame) into a short body and out again: the
    longest fades that keep the file below 33 k samples."""
    rng = np.random.default_rng(7201)
    n_fade = 30 * HOP + 137
    g = _db(np.linspace(-90.0, 0.0, n_fade))
    gain = np.concatenate([g, np.ones(1800), g[::-1]])
    return (gain * BODY * rng.standard_normal(len(gain))).astype(np.float32)


def _spike():
    y = np.zeros(5000, np.float32)
    y[2500] = 1.0
    return y


def _quiet():
    return _noise(np.random.default_rng(7202), 5000, 3e-6)


def _clamp():
    """The body's power (2e-10) is just above the 1e-10 clamp, the stretches around it (1e-12)
    below: 2.9 dB apart with the clamp, 23 dB without."""
    rng = np.random.default_rng(7203)
    return np.concatenate([_noise(rng, 4000, 1e-6), _noise(rng, 6000, 1.4e-5), _noise(rng, 4100, 1e-6)])


def _zeros():
    return np.zeros(5000, np.float32)


def _denormals():
    """A head of f32 denormals (1e-40 .. 1e-39), then a body."""
    rng = np.random.default_rng(7204)
    head = (rng.uniform(1e-40, 1e-39, 3000) * rng.choice([-1.0, 1.0], 3000)).astype(np.float32)
    assert np.all(head != 0) and np.all(np.abs(head) < np.finfo(np.float32).tiny)
    return np.concatenate([head, _noise(rng, 4000, BODY)])


CASES = {f"len_{n}": _length(n) for n in LENGTHS}
CASES.update({f"step_{s}": _step(s) for s in STEPS})
CASES.update(fades=_fades, spike=_spike, quiet=_quiet, clamp=_clamp, zeros=_zeros, denormals=_denormals)
NAMES = tuple(CASES)
SPIKE_BOUNDS = {20.0: (1536, 3584), 40.0: (1536, 3584), 60.0: (1536, 3584), 80.0: (0, 5000)}
WHOLE_FILE = ("quiet", "zeros", "clamp")


@lru_cache(maxsize=None)
def signal(name):
    y = np.ascontiguousarray(CASES[name](), np.float32)
    assert np.all(np.isfinite(y))
    y.setflags(write=False)
    return y


@lru_cache(maxsize=None)
def exact(name, top_db):
    return exact_trim(signal(name), top_db)


# --------------------------------------------------------------------------- batch layouts
def _batch_lengths(n, seed):
    """n random lengths in [0, 6000] with zero-length files first, last and in runs in the
    middle, several files of one sample and several multiples of 512."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6001, n)
    lens[[0, n - 1]] = 0
    lens[n // 3:n // 3 + 3] = 0
    lens[n // 2:n // 2 + 2] = 0
    lens[[1, n // 4, n - 2]] = 1
    for i, k in zip((2, 5, n // 5, n // 2 + 2, n - 3, n - 4), (512, 1024, 4096, 5632, 2048, 3072)):
        lens[i] = k
    return [int(v) for v in lens]


@lru_cache(maxsize=None)
def batch(name):
    """The files of a batch layout: noise bodies, a random head of each 50 dB down, a random tail zeros."""
    n, seed = {"batch_65": (65, 7301), "batch_300": (300, 7302)}[name]
    rng = np.random.default_rng(seed + 1)
    files = []
    for length in _batch_lengths(n, seed):
        y = _noise(rng, length, BODY)
        y[:int(rng.integers(0, length + 1)) // 2] *= np.float32(_db(-50.0))
        y[length - int(rng.integers(0, length + 1)) // 3:] = 0.0
        y.setflags(write=False)
        files.append(y)
    return tuple(files)


BATCHES = ("batch_65", "batch_300")


@lru_cache(maxsize=None)
def batch_exact(name, top_db):
    return tuple(exact_trim(y, top_db) for y in batch(name))


# --------------------------------------------------------------------------- window energies
WIN_LENGTHS = (1, 2, 63, 64, 65, 511, 512, 513, 1024, 1537, 5000)


@lru_cache(maxsize=None)
def energy_files():
    """Files for the window energies: lengths that are multiples of 512 (a last window ends on
    the boundary of the slot no block writes), lengths with a partial last block, and a file
    with a stretch of exact zeros."""
    rng = np.random.default_rng(7401)
    files = [_noise(rng, n, BODY) for n in (5120, 5000, 6144, 7777, 2048)]
    files[3][2000:4100] = 0.0
    for y in files:
        y.setflags(write=False)
    return tuple(files)


@lru_cache(maxsize=None)
def energy_windows():
    """{L: [(file, start)]} for every L of WIN_LENGTHS: starts 0, 1, 511, 512, 513, N - L and
    three random ones in every file that is long enough, and a window of zeros where one fits."""
    rng = np.random.default_rng(7402)
    out = {}
    for L in WIN_LENGTHS:
        wins = []
        for f, y in enumerate(energy_files()):
            n = len(y)
            if n < L:
                continue
            starts = {s for s in (0, 1, 511, 512, 513, n - L) if 0 <= s <= n - L}
            starts |= set(int(v) for v in rng.integers(0, n - L + 1, 3))
            wins += [(f, s) for s in sorted(starts)]
        if L <= 2100:
            wins.append((3, 2000))                  # all zeros: exactly -200.0
            if L < 512:
                wins.append((3, 2048 + 3))          # zeros wholly inside one block
        out[L] = tuple(wins)
    return out
