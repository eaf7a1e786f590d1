"""melodia_salience_kernel (csrc/melodia.hip) stage by stage, through nc_melodia_probe, on the cases
of tests/melodia_stage_cases.py.  Each stage's expected output is the oracle's
(oracle/melodia_ref.py) computed from the device's own previous stage, so that only the spectrum
carries a floating-point tolerance and a failure names its stage:

  spectrum        max_k |mag - mag64| / max_k mag64 <= 4 x what an f32 CPU FFT (scipy, complex64)
                  shows on the same case; silent frames exactly zero;
  spectral peaks  from f64(mag): the oracle's candidates ordered by (float32(value) descending, bin
                  ascending), the first 100: the same count and order, positions and values to
                  rtol 1e-12 (the same formula in the same operand order; only an FMA contraction
                  can move a last bit);
  salience        oracle.salience(device peaks) to 1e-12 of the frame's largest salience (at most
                  2000 f64 terms in another order, and pow's ulp: 2e-13);
  salience peaks  from the device's salience: bins, count, order exact, the output salience equal
                  to float32(salience[bin]) bit for bit.

Then the whole chain against the pure f64 oracle on every non-degenerate frame (the full bin set
on >= 99 % of all frames and on every frame of the tonal cases, saliences within 4 x the f32 CPU
chain's deviation), what little can be said about degenerate frames, independence of the grid
(one workgroup walking every frame reuses all of the kernel's LDS across frames), and exact
behaviour under scaling by a power of two.

Bounds are per case: 4 x what the f32 CPU chain shows on that case's frames.  Measured on an
MI355X (pytest -s prints every case), beside the bounds they were held to:
  spectrum error      1.42e-7 (short_1) .. 2.71e-7 (short_128); bounds 5.44e-7 (high_tone) ..
                      1.09e-6 (short_1023); the closest case is short_128, 2.71e-7 under 8.96e-7
  salience deviation  9.6e-8 (noise) .. 3.00e-7 (edge_79); bounds 2.95e-7 (short_1024) .. 2.62e-6
                      (edge_79); the closest case is short_1024, 1.28e-7 under 2.95e-7
  bin sets            the f64 oracle's on 616 of 616 non-degenerate frames (the f32 CPU chain: 614,
                      it misses two of short_2's two-sample frames)
Stages 2 to 4 held exactly as stated on all 663 frames, degenerate ones included.  The threshold
case (peaks within a per cent either side of the 40 dB threshold) takes part in the stage tests
only, see melodia_stage_cases.WHOLE_CHAIN.

That the checks bite was tried with five kernels changed in one place each (salience peaks
starting at bin 66; 99 spectral peaks kept; the 40 dB factor 0.0101; the left neighbour ignored at
bin 65; the sort keyed on the bin's magnitude instead of the interpolated one): each failed its
stage's test, on 1 to 23 cases.
"""
import numpy as np
import pytest
import torch

import melodia_stage_cases as MC
from nightcore_analyzer import engine as E
from nightcore_analyzer import melodia as M
from oracle import melodia_ref as R

pytestmark = pytest.mark.gpu

_PROBES = {}


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


def probe(eng, name):
    """One launch per case, kept for every test of this module (nobody writes to the arrays)."""
    if name not in _PROBES:
        files, sr, hop = MC.case_files(name)
        _PROBES[name] = M.salience_probe(eng, files, sr, hop)
    return _PROBES[name]


def frames_of(eng, name):
    """(file name, its probe, its reference, sample rate, frame) over every frame of a case."""
    _, sr, _ = MC.case_files(name)
    for fname, p in zip(MC.CASES[name], probe(eng, name)):
        ref = MC.reference(fname)
        assert len(p.npk) == ref.T == len(p.peaks.counts)
        for t in range(ref.T):
            yield fname, p, ref, float(sr), t


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("name", MC.NAMES)
def test_stage_spectrum(eng, name):
    bound = 4.0 * MC.yardsticks(MC.CASES[name]).spec
    worst = 0.0
    for fname, p, ref, sr, t in frames_of(eng, name):
        if ref.silent[t]:
            assert not p.mag[t].any() and p.npk[t] == 0 and not p.sal[t].any() and p.peaks.counts[t] == 0, (fname, t)
            continue
        assert np.all(np.isfinite(p.mag[t])) and np.all(p.mag[t] >= 0)
        worst = max(worst, MC.spectrum_error(p.mag[t], ref.mag64[t]))
    print(f"{name}: device spectrum error {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound, (name, worst, bound)


@pytest.mark.parametrize("name", MC.NAMES)
def test_stage_spectral_peaks(eng, name):
    cut = 0
    for fname, p, ref, sr, t in frames_of(eng, name):
        mag = p.mag[t].astype(np.float64)
        f, a = R.spectral_peaks(mag, sr, key_dtype=np.float32)
        n = int(p.npk[t])
        assert n == len(f) <= 100, (fname, t, n, len(f))
        np.testing.assert_allclose(p.pk_f[t, :n], f, rtol=1e-12, atol=0, err_msg=f"{fname} frame {t}")
        np.testing.assert_allclose(p.pk_a[t, :n], a, rtol=1e-12, atol=0, err_msg=f"{fname} frame {t}")
        assert not p.pk_f[t, n:].any() and not p.pk_a[t, n:].any()      # nothing written past the count
        cut += len(R.spectral_peaks(mag, sr, max_peaks=1 << 20)[0]) > 100
    if name in ("noise", "batch"):
        assert cut >= 30                                                # the 100-peak cut was exercised


@pytest.mark.parametrize("name", MC.NAMES)
def test_stage_salience(eng, name):
    for fname, p, ref, sr, t in frames_of(eng, name):
        n = int(p.npk[t])
        want = R.salience(p.pk_f[t, :n], p.pk_a[t, :n])
        err = float(np.max(np.abs(p.sal[t] - want)))
        assert err <= 1e-12 * want.max(), (fname, t, err, want.max())


@pytest.mark.parametrize("name", MC.NAMES)
def test_stage_salience_peaks(eng, name):
    for fname, p, ref, sr, t in frames_of(eng, name):
        bins, _ = R.salience_peaks(p.sal[t], MC.MIN_BIN, max_out=M.SALPK, key_dtype=np.float32)
        n = int(p.peaks.counts[t])
        assert n == len(bins), (fname, t, n, len(bins))
        assert np.array_equal(p.peaks.bins[t, :n], bins), (fname, t)
        assert np.array_equal(bits(p.peaks.sal[t, :n]), bits(p.sal[t, bins].astype(np.float32))), (fname, t)
        assert np.all((bins >= MC.MIN_BIN) & (bins < R.N_BINS))


def _whole_chain(eng, name):
    """(frames with the f64 oracle's bin set, non-degenerate frames, the largest salience
    deviation on the agreeing frames) of a case; asserts what holds on the degenerate frames."""
    agree = frames = 0
    worst = 0.0
    for fname, p, ref, sr, t in frames_of(eng, name):
        got = p.peaks.frame(t)
        if not ref.degenerate[t]:
            same, d = MC.salience_deviation(got, ref.peaks64[t])
            frames += 1
            agree += same
            if same:
                worst = max(worst, d)
            continue
        # one sample x under one window weight w: a flat spectrum of |x w|.  Nothing to compare,
        # but a salience is at most 100 peaks x sum_h 0.8^h < 500 |x w| (1e-5: the f32 spectrum
        # and the interpolation above a flat line), and behind a file that has real frames the
        # window weight 4.6e-9 keeps it far below them
        b, s = got
        y, _, hop = MC.signal(fname)
        xw = float(np.abs(MC.frame_f32(y, t, hop)).max())
        assert len(b) <= M.SALPK and np.all((b >= MC.MIN_BIN) & (b < R.N_BINS)), (fname, t)
        assert np.all(np.isfinite(s)) and np.all(s > 0) and np.all(s <= 500.0 * xw * (1 + 1e-5)), (fname, t)
        big = max((float(ref.peaks64[u][1].max()) for u in range(ref.T)
                   if not ref.degenerate[u] and len(ref.peaks64[u][1])), default=None)
        if big is not None:                                              # the oracle's largest salience of the file
            assert np.all(s < 1e-4 * big), (fname, t, s.max(), big)
    return agree, frames, worst


@pytest.mark.parametrize("name", MC.WHOLE_CHAIN)
def test_whole_chain_against_the_f64_oracle(eng, name):
    yard = MC.yardsticks(MC.CASES[name])
    agree, frames, worst = _whole_chain(eng, name)
    print(f"{name}: the oracle's bin set on {agree} of {frames} frames (f32 CPU chain: {yard.agree}); "
          f"salience deviation {worst:.3e}, bound {4 * yard.sal:.3e}")
    assert frames == yard.frames
    if name in MC.EXACT_SET_CASES:
        assert agree == frames, (name, agree, frames)
    assert worst <= 4.0 * yard.sal, (name, worst, 4.0 * yard.sal)


def test_whole_chain_bin_sets_on_99_percent_of_all_frames(eng):
    agree = frames = 0
    for name in MC.WHOLE_CHAIN:
        a, f, _ = _whole_chain(eng, name)
        agree, frames = agree + a, frames + f
    print(f"all cases: the oracle's bin set on {agree} of {frames} non-degenerate frames")
    assert frames >= 400 and agree >= 0.99 * frames, (agree, frames)


def _same(p, q, where):
    for field in ("mag", "npk", "pk_f", "pk_a", "sal"):
        assert np.array_equal(bits(getattr(p, field)), bits(getattr(q, field))), (where, field)
    for field in ("counts", "bins", "sal"):
        assert np.array_equal(bits(getattr(p.peaks, field)), bits(getattr(q.peaks, field))), (where, "peaks." + field)


def test_results_do_not_depend_on_the_grid_or_the_batch(eng):
    """max_blocks = 1 walks all 109 frames of the batch through one workgroup, 3 gives every
    workgroup some 36 of them: every LDS array is reused across frames of different files, with
    silent and degenerate frames in between.  Every stage must be bit-identical to the product's
    grid, to each file launched alone, and the product entry point to the probe."""
    files, sr, hop = MC.case_files("batch")
    base = probe(eng, "batch")
    assert sum(len(p.npk) for p in base) == 109
    for mb in (1, 3):
        for i, (p, q) in enumerate(zip(M.salience_probe(eng, files, sr, hop, max_blocks=mb), base)):
            _same(p, q, (mb, i))
    for i, (y, q) in enumerate(zip(files, base)):
        alone, = M.salience_probe(eng, [y], sr, hop)
        _same(alone, q, ("alone", i))
    for i, (pk, q) in enumerate(zip(M.salience_peaks(eng, files, sr, hop), base)):
        for field in ("counts", "bins", "sal"):
            assert np.array_equal(bits(getattr(pk, field)), bits(getattr(q.peaks, field))), ("product", i, field)


def test_scaling_by_a_power_of_two_is_exact(eng):
    """2^-20 x the noise: nothing under- or overflows, so every product, sum and rounding scales
    exactly: the same bins and counts, the output saliences 2^-20 x the unscaled ones bit for bit."""
    (y,), sr, hop = MC.case_files("noise")
    k = np.float32(2.0 ** -20)
    p, = probe(eng, "noise")
    q, = M.salience_probe(eng, [y * k], sr, hop)
    assert np.array_equal(q.npk, p.npk) and np.array_equal(q.peaks.counts, p.peaks.counts)
    assert p.peaks.counts.min() > 0
    assert np.array_equal(q.peaks.bins, p.peaks.bins)
    assert np.array_equal(bits(q.peaks.sal), bits(p.peaks.sal * k))
    assert np.array_equal(bits(q.mag), bits(p.mag * k))
