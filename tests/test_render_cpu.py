"""Host side of the speed render (no GPU): the renderer's definition (tests/speed_ref.py) is a
speed change and rejects what would alias; the factor, length and naming rules; the WAV
writer and the channel-preserving reader; the peak check and the native gain reduction."""
import math
from pathlib import Path

import numpy as np
import pytest

from nightcore_analyzer import io as nio
from nightcore_analyzer import loudness, ops, render
from speed_ref import Q, Z, plan, speed_ref

SR = 22050


def _edge(F):
    P, _, c = plan(SR, F)
    return math.ceil((Z / c + 1) / (P / Q)) + 1


# 3000 Hz at F = 4 lands above the Nyquist frequency (out of band by design): not a case
TONES = [(f0, F) for f0 in (440.0, 1000.0, 3000.0) for F in (0.25, 0.8, 1.0, 1.25, 1.234567, 4.0)
         if not (f0 == 3000.0 and F == 4.0)]


@pytest.mark.parametrize("f0,F", TONES)
def test_definition_is_a_speed_change(f0, F):
    """A tone at f0 comes out as the tone at f0 P / Q (away from the edges) within 1e-5.
    Measured: <= 1.2e-6 on every case."""
    P, n_out, _ = plan(SR, F)
    x = 0.5 * np.sin(2 * np.pi * f0 * np.arange(SR) / SR)
    y = speed_ref(x, F)
    assert len(y) == n_out
    E = _edge(F)
    m = np.arange(n_out)
    want = 0.5 * np.sin(2 * np.pi * f0 * (P / Q) * m / SR)
    err = float(np.max(np.abs(y - want)[E:n_out - E]))
    print(f"f0={f0} F={F} err={err:.3e}")
    assert n_out - 2 * E > 1000
    assert err <= 1e-5, err


@pytest.mark.parametrize("f0", [8900.0, 9500.0])
def test_definition_rejects_aliases(f0):
    """At F = 1.25 a tone that would land above the Nyquist frequency leaves <= -100 dB of
    its amplitude.  Measured: -101.8 dB (8900 Hz), -110.9 dB (9500 Hz)."""
    x = 0.5 * np.sin(2 * np.pi * f0 * np.arange(SR) / SR)
    y = speed_ref(x, 1.25)
    E = _edge(1.25)
    left = float(np.max(np.abs(y[E:len(y) - E])))
    db = 20 * math.log10(max(left, 1e-300) / 0.5)
    print(f"f0={f0} residue {db:.1f} dB")
    assert db <= -100.0, db


def test_quantize_factor():
    assert render.quantize_factor(1.25) == 1.25
    assert render.quantize_factor(1.2345674) == 1.234567
    assert render.quantize_factor(1.2345676) == 1.234568
    assert render.quantize_factor(0.25) == 0.25 and render.quantize_factor(4.0) == 4.0
    assert f"{render.quantize_factor(1.0447761194):.6f}" == "1.044776"
    for bad in (0.2, 4.1, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            render.quantize_factor(bad)


@pytest.mark.parametrize("n,F,want", [
    (1, 1.0, 1), (1, 4.0, 1), (1, 0.25, 4), (1, 0.8, 2), (2, 1.25, 2), (3, 1.234567, 3),
    (5000, 1.234567, 4051), (5000, 1.000001, 5000), (1_000_001, 1.000001, 1_000_000),
    (1_000_002, 1.000001, 1_000_001), (0, 1.25, 0),
    (3_000_000, 1.234567, -(-3_000_000 * Q // 1_234_567)), (1 << 40, 0.25, 4 << 40)])
def test_output_length(n, F, want):
    """n_out = ceil(n Q / P) in integers, from the library (nc_speed_out_len) and from the
    numpy definition alike."""
    P, n_out = ops.speed_plan(F, [n])
    assert P == int(round(F * Q))
    assert int(n_out[0]) == want
    assert plan(n, F)[:2] == (P, want)


def test_output_length_rejects_out_of_range_factor():
    from nightcore_analyzer import _native
    for bad in (0.2499994, 4.000001, float("nan")):
        with pytest.raises(_native.NativeError):
            ops.speed_plan(bad, [100])


def test_naming():
    assert render.hqnc_path("/m/Song.flac", 0) == Path("/m/Song [Nightcore].flac")
    assert render.hqnc_path(Path("/m/Song.wav")) == Path("/m/Song [Nightcore].wav")
    assert render.hqnc_path("/m/Song.wav", 1) == Path("/m/Song [Nightcore] UPD1.wav")
    assert render.hqnc_path("a.b.wav", 12) == Path("a.b [Nightcore] UPD12.wav")
    assert loudness.make_adj_path(Path("Song [Nightcore].flac"), 1) == Path("Song [Nightcore] ADJ1.flac")
    assert loudness.make_adj_path("/x/Song.wav", 2) == Path("/x/Song ADJ2.wav")


@pytest.fixture(scope="module")
def stereo():
    rng = np.random.default_rng(5)
    return rng.uniform(-1, 1, (2, 1001)).astype(np.float32)


def test_wav_float32_round_trip(tmp_path, stereo):
    p = tmp_path / "f.wav"
    nio.write_wav(p, stereo, 44100, "float32")
    back, sr, fmt = nio.read_wav_channels(p)
    assert (sr, fmt, back.dtype, back.shape) == (44100, "float32", np.float32, stereo.shape)
    assert np.array_equal(back.view(np.uint32), stereo.view(np.uint32))
    mono, msr = nio.load_audio(str(p), sr=None)
    assert msr == 44100
    assert np.array_equal(mono, stereo.T.mean(axis=1).astype(np.float32))
    nio.write_wav(p, stereo[0], 22050, "float32")                      # [frames] is one channel
    back, sr, _ = nio.read_wav_channels(p)
    assert sr == 22050 and back.shape == (1, 1001) and np.array_equal(back[0], stereo[0])
    assert np.array_equal(nio.load_audio(str(p))[0], stereo[0])


def test_wav_pcm16_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    q = rng.integers(-32768, 32768, (2, 777)).astype(np.int16)
    q[0, :4] = [-32768, 32767, 0, -1]
    p = tmp_path / "p.wav"
    nio.write_wav(p, q, 48000, "pcm16")                                # stored samples as they are
    back, sr, fmt = nio.read_wav_channels(p)
    assert (sr, fmt, back.shape) == (48000, "pcm16", (2, 777))
    assert np.array_equal(back, q.astype(np.float32) / 32768.0)
    p2 = tmp_path / "p2.wav"
    nio.write_wav(p2, back, sr, "pcm16")                               # float -> the same 16 bits
    assert p2.read_bytes() == p.read_bytes()
    assert np.array_equal(nio.load_audio(str(p), sr=None)[0], back.T.mean(axis=1).astype(np.float32))
    assert nio.decoded_length(str(p), None) == 777
    with pytest.raises(ValueError):
        nio.write_wav(p, q, 48000, "float32")
    with pytest.raises(ValueError):
        nio.write_wav(p, back, 48000, "pcm24")


def test_quantize_pcm16_rule():
    x = np.array([1.0, -1.0, 1 - 2.0 ** -16, -(1 - 2.0 ** -16), 0.5 / 32768, 1.5 / 32768, 2.5 / 32768,
                  -0.5 / 32768, -1.5 / 32768, 1.5, -1.5, 32767.5 / 32768, -32768.5 / 32768, 0.0], np.float32)
    q, clipped = nio.quantize_pcm16(x)
    assert q.tolist() == [32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 0]
    # clamped: 1.0 (32768), 1 - 2^-16 (32767.5 -> 32768), 1.5, -1.5, 32767.5 / 32768 (-> 32768);
    # -(1 - 2^-16) and -32768.5 / 32768 round (half to even) to -32768, which is in range
    assert clipped == 5


def test_detect_peak(tmp_path):
    n = 500
    quiet = (0.1 * np.sin(np.arange(n))).astype(np.float32)
    hot = quiet.copy()
    hot[123] = -1.25                                      # clips on one channel only
    p = tmp_path / "one_hot.wav"
    nio.write_wav(p, np.stack([quiet, hot]), 44100, "float32")
    db, clip = loudness.detect_peak(p)
    assert clip and db == pytest.approx(20 * math.log10(1.25), abs=1e-9)
    mono_peak = float(np.max(np.abs(nio.load_audio(str(p), sr=None)[0])))
    assert mono_peak < 1.0                                 # the mono mix would have hidden it
    nio.write_wav(p, np.stack([quiet, quiet]), 44100, "float32")
    db, clip = loudness.detect_peak(p)
    assert not clip and db == pytest.approx(20 * math.log10(float(np.max(np.abs(quiet)))), abs=1e-9)
    nio.write_wav(p, np.zeros((2, n), np.float32), 44100, "pcm16")
    assert loudness.detect_peak(p) == (-math.inf, False)
    full = np.zeros((2, n), np.int16)
    full[1, 7] = -32768                                    # full scale: exactly 0 dBFS
    nio.write_wav(p, full, 44100, "pcm16")
    assert loudness.detect_peak(p) == (0.0, True)
    full[1, 7] = 32767
    nio.write_wav(p, full, 44100, "pcm16")
    db, clip = loudness.detect_peak(p)
    assert not clip and db < 0.0
    with pytest.raises(NotImplementedError):
        loudness.detect_peak(tmp_path / "x.flac")


def test_gain_reduction(tmp_path, stereo):
    src, dst = tmp_path / "s.wav", tmp_path / "s ADJ1.wav"
    nio.write_wav(src, stereo, 44100, "float32")
    loudness.apply_gain_reduction(src, dst, -6.0206)
    back, sr, fmt = nio.read_wav_channels(dst)
    assert (sr, fmt) == (44100, "float32")
    half = stereo * np.float32(0.5)
    assert np.all(np.abs(back - half) <= np.spacing(np.abs(half)))      # within 1 ulp of half
    q = (stereo * 20000).astype(np.int16)
    nio.write_wav(src, q, 22050, "pcm16")
    loudness.apply_gain_reduction(src, dst, -6.0206)
    back, sr, fmt = nio.read_wav_channels(dst)
    assert (sr, fmt) == (22050, "pcm16")                                 # the source's sample format
    assert np.max(np.abs(back * 32768 - q.astype(np.float64) / 2)) <= 0.5 + 1e-3


def test_public_modules_import():
    from nightcore_analyzer import cli
    args = cli._build_parser().parse_args(["-n", "a", "-s", "b"])
    assert args.render_hqnc is None and args.refine is False
    assert {"speed", "speed_file", "refine_speed", "hqnc_path", "quantize_factor", "RenderInfo",
            "Refinement"} <= set(dir(render))
