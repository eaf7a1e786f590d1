"""CPU qualification of tests/spectral_frame_cases.py: the cases are short and finite, the
per-frame reference is consistent with itself (its own rolloff bin is admissible, its centroid
and band sums are inside the bounds derived for the device), and the rolloff condition is sharp:
on at least three quarters of each case's frames a single bin is admissible, on no frame more
than two.  No GPU.  Figures are printed (pytest -s)."""
import numpy as np
import pytest

import spectral_frame_cases as SC


@pytest.mark.parametrize("name", SC.NAMES)
def test_rolloff_condition_is_sharp_and_holds_the_oracle(name):
    r = SC.reference(name)
    lo, hi = SC.admissible_rolloff(r.S)
    width = hi - lo + 1
    live = ~r.silent
    assert np.all(lo <= hi) and np.all(width[r.silent] == 1) and np.all(lo[r.silent] == 0)
    own = np.rint(r.rolloff / r.hz).astype(np.int64)
    assert np.all((lo <= own) & (own <= hi)), name
    single = float(np.mean(width[live] == 1)) if live.any() else 1.0
    print(f"{name}: {int(live.sum())} live frames of {len(live)}, single admissible bin on {100 * single:.0f} %, "
          f"widest {int(width.max())}")
    assert single >= 0.75, (name, single)
    assert width.max() <= 2, (name, int(width.max()))


def test_tolerance_comes_from_the_measured_value():
    assert SC.EPS == 4.0 * SC.EPS_MEASURED and 0.0 < SC.EPS_MEASURED <= SC.EPS_CEILING
    for name in SC.NAMES:
        S = SC.reference(name).S
        delta = SC.NBINS * 2.0 ** -24 + SC.NBINS * SC.EPS
        assert np.all(SC.rolloff_err(S) <= delta * S.sum(axis=0)[None, :])


def test_cases_are_short_and_reach_the_edges():
    rates = set()
    for name in SC.NAMES:
        y, sr = SC.signal(name)
        rates.add(sr)
        assert y.dtype == np.float32 and len(y) <= 2 * sr
    assert rates == {22050, 44100, 48000}
    assert [len(SC.signal(f"short_{n}")[0]) for n in (1, 511, 512, 600, 2048)] == [1, 511, 512, 600, 2048]
    assert SC.reference("zeros").silent.all() and len(SC.reference("zeros").silent) == 11
    g = SC.reference("gap").silent
    assert g.any() and not g[0] and not g[-1]                       # silent frames between live ones
    assert len({SC.band_bins(sr) for sr in rates}) == 3             # the band edges move with the rate
    assert SC.band_bins(22050)[4][1] == 1025 and SC.band_bins(48000)[4][1] < 1025
    # a frame whose l1 norm is below tiny(float32) does not occur outside the silent ones
    for name in SC.NAMES:
        r = SC.reference(name)
        assert np.all(r.S.sum(axis=0)[~r.silent] > 1e-30)


@pytest.mark.parametrize("name", SC.NAMES)
def test_reference_is_inside_its_own_bounds(name):
    """The f64 restatement of centroid and band sums from S against the oracle's own values: a
    bound that excluded the reference it was derived around would be wrong."""
    r = SC.reference(name)
    l1 = r.S.sum(axis=0)
    k = np.arange(SC.NBINS, dtype=np.float64)[:, None]
    cen = r.hz * np.divide((k * r.S).sum(axis=0), l1, out=np.zeros_like(l1), where=l1 > 0)
    assert np.all(np.abs(cen - r.centroid) <= SC.centroid_bound(r.S, r.hz, r.centroid)), name
    assert np.all(r.centroid[r.silent] == 0.0) and np.all(r.rolloff[r.silent] == 0.0) and np.all(r.rms[r.silent] == 0.0)
    ref, bound = SC.band_bound(r.S, r.bands)
    assert ref.shape == (5, r.S.shape[1]) and np.all(bound >= 0.0)
    # the fine centroid bound is the tighter one wherever it applies
    E = SC.bin_error(r.S)
    crude = r.hz * E * (k.sum() + 1024.0 * 1025.0) / np.where(l1 > 0, l1, 1.0) + 2e-5 * np.abs(r.centroid)
    assert np.all(SC.centroid_bound(r.S, r.hz, r.centroid) <= crude * (1 + 1e-12))
