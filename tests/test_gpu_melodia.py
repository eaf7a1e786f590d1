"""The opt-in MELODIA front end on the device (nc_melodia_salience, csrc/melodia.hip) against the
CPU oracle (oracle/melodia_ref.py), and the device MELODIA through pitch.estimate_pitch_melodia
and pipeline.run.  PARITY UNPINNED: both sides restate essentia's PredominantPitchMelodia as the
reference calls it (pitch.py:210-215); essentia is not installed, so no essentia output pins them.
Tolerances: the device computes the 8192-point spectrum in f32 and (since round 5) the peak
interpolation, the harmonic binning and the salience sums in f64, the oracle all in f64, so only
two near-equal salience peaks (a spectrum 1e-7 apart) can order differently; the tests bound how
often.  The melody (contours and selection on the host, oracle/melodia_ref.py restating them
independently) must equal the whole-oracle melody on >= 99 % of the oracle's voiced frames."""
import numpy as np
import pytest
import torch

import melodia_stage_cases as MC
from nightcore_analyzer import engine as E
from nightcore_analyzer import melodia as M
from nightcore_analyzer import synth
from oracle import melodia_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


def test_salience_peaks_match_oracle(eng):
    y = synth.make_source(4.0, 1000)
    pk, = M.salience_peaks(eng, [y])
    T = R.n_frames(len(y))
    assert len(pk.counts) == T
    # every third frame (it was every ninth: with 81 frames a 99 % bar allows no miss at all, and
    # the file's last frame, 7 samples under the window's first weights, is one broad hump whose
    # maximum any f32 spectrum places 0.3 Hz off, across a 10-cent boundary: the f32 CPU chain
    # below misses the oracle's bins there exactly as the device does).  Measured on an MI355X:
    # the oracle's bin set on 234 of 235 frames, salience deviation 1.900e-6 under 4 x 1.887e-6
    frames = sorted(set(list(range(0, T, 3)) + [0, 1, T - 2, T - 1]))
    set_ok = cnt_ok = 0
    worst = yard = 0.0
    for t in frames:
        rb, rs = R.frame_salience_peaks(y, t)
        gb, gs = pk.frame(t)
        cnt_ok += abs(len(rb) - len(gb)) <= 1
        same, d = MC.salience_deviation((gb, gs), (rb, rs))     # the whole bin set, not the top bin only
        set_ok += same
        if same:
            worst = max(worst, d)
        # the yardstick: the oracle's stages on an f32 CPU spectrum of the same frame
        same32, d32 = MC.salience_deviation(MC.as_output(MC.chain(MC.frame_mag32(y, t, R.HOP), 22050.0)), (rb, rs))
        if same32:
            yard = max(yard, d32)
    print(f"bin sets {set_ok} of {len(frames)}, salience deviation {worst:.3e}, f32 CPU chain {yard:.3e}")
    assert set_ok >= 0.99 * len(frames), (set_ok, len(frames))
    assert cnt_ok >= 0.99 * len(frames), (cnt_ok, len(frames))
    assert worst <= 4.0 * yard, (worst, yard)


def test_device_melody_equals_the_oracle_melody(eng):
    """Front end on the device + contours / melody on the host against the whole oracle (front end,
    contours, melody; oracle/melodia_ref.py) on both files of a 1.25x melody pair: the same pitch
    on >= 99 % of the oracle's voiced frames, and voicing agreeing on >= 99 % of all frames."""
    nc, src = synth.make_melody_pair(3.0, 7)
    got = M.predominant_pitch_melodia([src, nc], 22050, eng)
    for y, hz in zip((src, nc), got):
        ref = R.predominant_pitch_ref(y)
        assert len(hz) == len(ref)
        voiced = ref > 0
        assert voiced.sum() > 0.3 * len(ref)
        same = np.isclose(hz, ref, rtol=1e-12, atol=0) & voiced
        assert same.sum() >= 0.99 * voiced.sum(), (same.sum(), voiced.sum())
        assert ((hz > 0) == voiced).mean() >= 0.99


def test_files_in_one_launch_equal_single_calls_and_repeat(eng):
    ys = [synth.make_source(2.3, 1001), synth.make_source(0.05, 1002), synth.make_source(3.1, 1003)[7:]]
    together = M.salience_peaks(eng, ys)
    for y, p in zip(ys, together):
        q, = M.salience_peaks(eng, [y])
        np.testing.assert_array_equal(p.counts, q.counts)
        for t in range(len(p.counts)):
            n = p.counts[t]
            np.testing.assert_array_equal(p.bins[t, :n], q.bins[t, :n])
            np.testing.assert_array_equal(p.sal[t, :n], q.sal[t, :n])


def test_device_melodia_tracks_a_nightcore_pair(eng):
    """A 1.25x pair with one clear melody line: nc frame t (time t hop / sr) shows src time
    1.25 t hop / sr, and where both are voiced the pitch ratio is the true 3.86 st within the
    10-cent bin grid.  (The voiced-median shift the reference uses depends on which frames are
    voiced: here 4.9 st on both the device and the oracle, one note off.)"""
    nc, src = synth.make_melody_pair(12.0, 7)
    hs, hn = M.predominant_pitch_melodia([src, nc], 22050, eng)
    ts = np.round(np.arange(len(hn)) * 1.25).astype(int)
    both = (ts < len(hs)) & (hn > 0)
    both[both] &= hs[ts[both]] > 0
    assert both.sum() > 0.35 * len(hn), both.sum()    # 790 of 1662 (the oracle front end: 790 too)
    r = 12.0 * np.log2(hn[both] / hs[ts[both]])
    assert np.mean(np.abs(r - 12.0 * np.log2(1.25)) < 0.15) > 0.95
    from nightcore_analyzer import pitch
    lines = []
    mel = pitch.estimate_pitch_melodia(src, nc, 22050, log=lines.append, backend="device")
    assert mel is not None, lines
    assert lines and lines[-1].startswith("    MELODIA: ") and "voiced frames" in lines[-1]
    assert len(mel[0]) == (hs > 0).sum() and len(mel[1]) == (hn > 0).sum()
    assert pitch.estimate_pitch_melodia(src, nc, 22050, backend="device") == mel      # deterministic


def test_run_with_device_melodia_keeps_the_reference_acceptance_rule(eng, monkeypatch):
    """pipeline.run with NC_MELODIA=device: the MELODIA shift (the true 3.86 st of a 1.25x pair)
    meets the chroma shift, which the reference's lag / 3 quirk reports as 1.33 st: 2.5 st apart,
    beyond MELODIA_AGREE_ST, so the reference's rule keeps chroma and logs the disagreement."""
    from nightcore_analyzer import pipeline
    monkeypatch.setenv("NC_MELODIA", "device")
    nc, src = synth.make_melody_pair(70.0, 8)
    lines = []
    res = pipeline.run(nc, src, log=lines.append)
    assert any(l.startswith("    MELODIA: ") for l in lines), lines
    assert any("disagrees with chroma" in l for l in lines), lines
    assert res.pitch_method == "chroma_xcorr"
