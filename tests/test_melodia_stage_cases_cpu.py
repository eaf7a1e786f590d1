"""CPU qualification of tests/melodia_stage_cases.py: from the oracle alone, every case does what
it is there for, the degenerate rule names the frames it should and no other, and the inputs are
well conditioned: over all non-degenerate frames the oracle's salience-peak bins from its f64
spectrum and from an f32 CPU spectrum are the same set on at least 99 %.  No GPU.  Figures are
printed (pytest -s)."""
import numpy as np
import pytest

import melodia_stage_cases as MC
from oracle import melodia_ref as R


def _all_peaks(mag, sr):
    return R.spectral_peaks(mag, float(sr), max_peaks=1 << 20)


def _pow2(n):
    p = 2
    while p < n:
        p <<= 1
    return p


def test_cases_are_short_and_the_frame_counts_are_the_formula():
    for name in MC.NAMES:
        files, sr, hop = MC.case_files(name)
        for y, fname in zip(files, MC.CASES[name]):
            assert y.dtype == np.float32
            T = MC.reference(fname).T
            assert T == -(-(len(y) + 1024) // hop) and T <= 50, (fname, T)
    assert [len(MC.signal(f"short_{n}")[0]) for n in MC.SHORT] == list(MC.SHORT)
    assert [len(MC.signal(f"two_tone_{d}")[0]) for d in range(4)] == [5120, 5121, 5122, 5123]
    assert MC.signal("rate")[1:] == (44100, 256) and MC.MIN_BIN == 65
    assert MC.CASES["batch"] == ("noise", "zeros_300", "two_tone_2", "short_1")
    total = sum(MC.reference(f).T for name in MC.NAMES for f in MC.CASES[name])
    print(f"{len(MC.NAMES)} cases, {total} frames")


def test_silent_frames_are_the_all_zero_ones():
    for fname in MC.FILES:
        r = MC.reference(fname)
        assert np.array_equal(r.silent, r.mag64.max(axis=1) == 0.0), fname
        assert all(len(r.peaks64[t][0]) == 0 for t in np.flatnonzero(r.silent))
    assert MC.reference("silence").silent.all() and MC.reference("zeros_300").silent.all()
    # a frame that starts on the file's last sample sees it under window()[0] == 0
    assert R.window()[0] == 0.0 and R.window()[1] > 0.0
    for fname in ("short_1", "short_129", "short_1025", "two_tone_1"):
        assert np.flatnonzero(MC.reference(fname).silent).tolist() == [MC.reference(fname).T - 1], fname


def test_the_degenerate_rule_names_the_single_sample_frames_only():
    """Exactly one non-zero sample in the f32 windowed frame: the last frame of the files whose
    length is 2 (mod hop), and every non-silent frame of the one-sample file.  Nowhere else."""
    want = {"two_tone_2": [48], "short_2": [8], "short_1": list(range(8))}
    for fname in MC.FILES:
        got = np.flatnonzero(MC.reference(fname).degenerate).tolist()
        assert got == want.get(fname, []), (fname, got)
    # what makes them degenerate: a flat spectrum, and peaks that are rounding noise
    r = MC.reference("two_tone_2")
    m = r.mag64[48]
    assert m.min() / m.max() > 1 - 1e-12
    assert len(_all_peaks(m, 22050)[0]) > 100
    big = max(s.max() for t, (_, s) in enumerate(r.peaks64) if t != 48 and len(s))
    assert len(r.peaks64[48][1]) > 0 and r.peaks64[48][1].max() < 1e-4 * big


def test_noise_reaches_the_hundred_peak_cut_and_both_sort_sizes():
    r = MC.reference("noise")
    ncand = np.array([len(_all_peaks(r.mag64[t], 22050)[0]) for t in range(r.T)])
    inside = np.arange(8, 25)                      # frames wholly inside the 4096 samples
    print("noise candidates per frame:", ncand.tolist())
    assert np.all(ncand[inside] > 100) and np.sum(ncand > 100) >= 30
    assert {_pow2(n) for n in ncand[ncand > 128]} == {256, 512}          # the bitonic sort's sizes
    for t in inside:
        f, a = R.spectral_peaks(r.mag64[t], 22050.0)
        assert len(a) == 100 and a.min() > 0.01 * a.max()           # all kept peaks within 40 dB
    npk = [len(r.peaks64[t][0]) for t in inside]
    assert 20 <= min(npk) and max(npk) <= 40, npk


def test_low_tone_breaks_below_55_hz_and_has_salience_under_the_edge():
    r = MC.reference("low_tone")
    for t in range(8, 13):
        f, a = R.spectral_peaks(r.mag64[t], 22050.0)
        kept = f[a > 0.01 * a.max()]
        first_neg = [next((h for h in range(R.NH) if int(R.cent_bin(x / (h + 1))) < 0), None) for x in kept]
        assert any(h is not None and h > 0 for h in first_neg), t       # the hb < 0 break, after some harmonics
        sal = R.salience(f, a)
        assert sal[:MC.MIN_BIN].sum() > 0.1 * sal.sum()
        assert int(np.argmax(sal)) == int(R.cent_bin(60.0)) < MC.MIN_BIN   # the largest salience is no peak


def test_edge_tones_sit_either_side_of_bin_65():
    """79 Hz: the tone's salience maximum is at bin 63, the salience falls through bins 64, 65,
    66, so the lower edge must not produce a peak (the left neighbour sal[64] is the larger).  Its
    only peaks are those of the window's side lobes, a semitone and more above the edge.  80.2 Hz:
    the maximum is bin 65 itself, a peak because sal[64] < sal[65]."""
    for t in range(8, 13):
        r = MC.reference("edge_79")
        f, a = R.spectral_peaks(r.mag64[t], 22050.0)
        sal = R.salience(f, a)
        assert int(np.argmax(sal)) == 63 and sal[64] > sal[65] > sal[66] > 0
        assert all(b > MC.MIN_BIN + 2 * R.SEMI for b in r.peaks64[t][0]), r.peaks64[t][0]
        r = MC.reference("edge_80")
        f, a = R.spectral_peaks(r.mag64[t], 22050.0)
        sal = R.salience(f, a)
        assert int(np.argmax(sal)) == MC.MIN_BIN and 0 < sal[64] < sal[65] and sal[65] >= sal[66]
        assert int(r.peaks64[t][0][0]) == MC.MIN_BIN


def test_high_tone_skips_its_first_harmonic_bin_and_dc_has_no_bin_0_candidate():
    r = MC.reference("high_tone")
    for t in range(8, 13):
        f, a = R.spectral_peaks(r.mag64[t], 22050.0)
        assert abs(f[0] - 3000.0) < 2.0
        assert int(R.cent_bin(f[0])) >= R.N_BINS + R.SEMI               # h = 0 reaches no salience bin
        assert 0 <= int(R.cent_bin(f[0] / 2)) < R.N_BINS                # h = 1 does
        assert int(r.peaks64[t][0][0]) == int(R.cent_bin(f[0] / 2))
    r = MC.reference("dc")
    for t in range(r.T):
        assert int(np.argmax(r.mag64[t])) == 0                          # the maximum is bin 0 ...
        f, a = _all_peaks(r.mag64[t], 22050)
        assert len(f) > 0 and f.min() > 22050.0 / 8192                  # ... and no candidate is
        assert a.max() < 0.2 * r.mag64[t, 0]
        if 8 <= t <= 12:
            # as a candidate it would lift the 40 dB threshold above peaks that are kept now
            kept = a[a > 0.01 * a.max()]
            assert abs(f[0] - 440.0) < 2.0 and np.any(kept < 0.01 * r.mag64[t, 0])


def test_threshold_case_has_peaks_within_a_per_cent_either_side_of_40_db():
    """Not in the issue's list: none of its cases has a peak near the threshold (the noise keeps
    all 100), and a kernel with 0.0101 for 0.01 passed every stage test on them."""
    r = MC.reference("threshold")
    both = 0
    for t in range(r.T):
        f, a = R.spectral_peaks(r.mag64[t], 22050.0)
        ratio = a / a.max()
        just_in = np.any((ratio > 0.01) & (ratio <= 0.0101))
        just_out = np.any((ratio <= 0.01) & (ratio > 0.0099))
        both += bool(just_in and just_out)
        if 8 <= t <= 12:
            assert just_in and just_out, (t, np.sort(ratio)[::-1][:30])
            # and the salience differs by far more than the stage test's 1e-12 when one more is dropped
            a_wrong = np.where(ratio <= 0.0101, 0.0, a)
            assert np.max(np.abs(R.salience(f, a) - R.salience(f, a_wrong))) > 1e-6 * R.salience(f, a).max()
    print(f"threshold: peaks within 1 % either side of the threshold on {both} of {r.T} frames")
    assert both >= 20


def test_the_two_cpu_chains_agree_on_99_percent_of_the_frames():
    """A condition on the inputs: where an f32 FFT that is not the device's already changes the
    bin set, the frame says nothing about the kernel."""
    for name in MC.WHOLE_CHAIN:
        y = MC.yardsticks(MC.CASES[name])
        print(f"{name}: f32 spectrum error {y.spec:.2e}, salience deviation {y.sal:.2e}, "
              f"same bin set on {y.agree} of {y.frames} frames")
        if name in MC.EXACT_SET_CASES:
            assert y.agree == y.frames, name
    assert set(MC.NAMES) - set(MC.WHOLE_CHAIN) == {"threshold"}
    y = MC.yardsticks(tuple(dict.fromkeys(f for name in MC.WHOLE_CHAIN for f in MC.CASES[name])))
    print(f"all files: {y.spec:.2e}, {y.sal:.2e}, {y.agree} of {y.frames}")
    assert y.frames >= 400 and y.agree >= 0.99 * y.frames
    assert 1e-8 < y.spec < 1e-6


@pytest.mark.parametrize("key", (np.float64, np.float32))
def test_key_dtype_orders_by_the_rounded_value_then_by_bin(key):
    """The device's order contract, restated by the oracle's key_dtype: two values that round to
    the same float32 are ordered by bin under an f32 key, by value under the f64 key."""
    sal = np.zeros(R.N_BINS)
    sal[100], sal[200], sal[300] = 1.0, 1.0 + 1e-12, 0.5
    b, c = R.salience_peaks(sal, MC.MIN_BIN, key_dtype=key)
    assert b.tolist() == ([100, 200, 300] if key is np.float32 else [200, 100, 300])
    assert c.dtype == np.float64 and c.tolist() == [sal[i] for i in b]
    mag = np.zeros(4097)
    mag[1000], mag[2000] = 1.0, 1.0 + 1e-12
    f, a = R.spectral_peaks(mag, 8192.0, key_dtype=key)
    assert f.tolist() == ([1000.0, 2000.0] if key is np.float32 else [2000.0, 1000.0])
    # the default is the f64 order the oracle always had
    assert R.salience_peaks(sal, MC.MIN_BIN)[0].tolist() == [200, 100, 300]
