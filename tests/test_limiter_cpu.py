"""The true-peak limiter's definition (tests/limiter_ref.py, numpy float64) held to what a
limiter must do, on the reference alone: no device.  The GPU kernels are compared with this
reference in tests/test_gpu_limiter.py.

Overshoot (h): a gain applied at the sample rate cannot bound the inter-sample values exactly.
The independent 8x meter (32 zero crossings a side) reads at most 1.00961 L on the limited
test signals (0.083 dB; the sr / 4 sine, whose limited samples sit at 0.707 L), measured on
the f64 definition over the cases below and recorded in DESIGN.md §2; OVERSHOOT holds it."""
import numpy as np
import pytest

import limiter_ref as R

OVERSHOOT = 0.0097        # largest (meter8(y) / L - 1) measured over the cases: 0.009610
GAIN_CAP = 1e-4           # the GPU test's cap on the gain deviation (0.001 dB)

ALL = [(sr, c.name) for sr in R.RATES for c in R.cases(sr)]


def _case(sr, name):
    return next(c for c in R.cases(sr) if c.name == name), R.reference(sr, name)


def test_windows():
    assert R.windows(22050) == (110, 1102) and R.windows(48000) == (240, 2400)
    assert R.windows(100, 0.0, 0.0) == (1, 1)
    assert abs(float(R.h(0.0)) - 1.0) < 1e-15 and np.all(np.abs(R.h(np.arange(1, 13))) < 1e-16)
    assert np.all(R.h(np.array([-12.0, 12.0, 12.5])) == 0.0) and float(R.h(11.75)) != 0.0


@pytest.mark.parametrize("sr", R.RATES)
def test_under_the_ceiling_is_untouched(sr):
    """(a) true peak <= L: g = 1 everywhere, y = x to the bit."""
    c, ref = _case(sr, "under")
    assert ref.true_peak <= ref.L
    assert np.all(ref.g == 1.0) and ref.limited == 0
    assert np.array_equal(ref.y, c.x.astype(np.float64))


@pytest.mark.parametrize("sr", R.RATES)
def test_one_over_peak(sr):
    """(b) one over-peak at j0: nothing before j0 - Wa + 1, the full reduction at j0, and an
    exponential release after it."""
    Wa, Wr = R.windows(sr)
    N, j0 = 3 * R.TILE, R.TILE + 300
    x = R._bed(N, 31, amp=0.02)
    x[j0] = 1.04 * R.L01        # the inter-sample values beside it stay under L: one r < 1
    ref = R.limiter_ref(x.astype(np.float32), -0.1, Wa, Wr)
    assert np.count_nonzero(ref.r < 1.0) == 1 and ref.r[j0] < 1.0
    assert np.all(ref.g[:j0 - Wa + 1] == 1.0) and ref.g[j0 - Wa + 1] < 1.0
    assert abs(ref.g[j0] - ref.r[j0]) <= 4e-16           # the mean of Wa equal deficits, summed
    beta = np.exp(-1.0 / Wr)
    n = np.arange(j0 + 1, N)
    bound = (1.0 - ref.r.min()) * beta ** (n - j0 - Wa + 1.0)
    assert np.all(1.0 - ref.g[n] <= bound * (1.0 + 1e-12))
    assert np.all(np.diff(ref.g[j0 + Wa:]) > 0.0)        # pure release once the box has passed


@pytest.mark.parametrize("sr,name", ALL)
def test_ceiling_and_gain_bound(sr, name):
    """(c) max |y| <= L and (d) g <= r everywhere, for every case."""
    c, ref = _case(sr, name)
    if c.x.shape[1] == 0:
        assert ref.true_peak == 0.0 and ref.limited == 0 and ref.y.shape == c.x.shape
        return
    assert np.abs(ref.y).max() <= float(np.float32(ref.L))
    assert np.all(ref.g <= ref.r + 1e-15)
    assert np.all((ref.g > 0.0) & (ref.g <= 1.0))
    # the clamp absorbs rounding only
    assert np.abs(c.x * ref.g[None, :]).max() <= ref.L * (1.0 + 1e-14)
    assert ref.true_peak == ref.p.max() >= np.abs(c.x).max()


@pytest.mark.parametrize("sr", R.RATES)
def test_channels_are_linked(sr):
    """(e) an over-peak on one channel turns both down alike."""
    c, ref = _case(sr, "stereo")
    solo = R.limiter_ref(c.x[0], c.limit_db, *c.wa_wr)
    assert solo.limited == 0 and ref.limited > 0
    ok = (c.x[0] != 0.0) & (c.x[1] != 0.0)
    q0, q1 = ref.y[0][ok] / c.x[0][ok], ref.y[1][ok] / c.x[1][ok]
    assert np.max(np.abs(q0 - q1)) <= 4e-16 and np.max(np.abs(q0 - ref.g[ok])) <= 4e-16
    assert np.min(q0) < 0.5


@pytest.mark.parametrize("sr", R.RATES)
def test_peaks_inside_a_release_tail(sr):
    """(f) a smaller over-peak inside the tail does not lift the gain off the tail; a larger
    one overrides it."""
    c, ref = _case(sr, "tail_peaks")
    Wa, Wr = c.wa_wr
    j0, j1, j2 = c.peaks
    beta = np.exp(-1.0 / Wr)
    lo, hi = j0 + Wa, j2 - Wa                             # from the end of j0's box to j2's attack
    tail = ref.d[lo] * beta ** (np.arange(len(ref.d)) - lo)
    assert ref.r[j0] < ref.r[j1] < 1.0 and 1.0 - ref.r[j1] < tail[j1] and lo < j1 - Wa and j1 + Wa < hi
    assert np.allclose(ref.d[lo:hi], tail[lo:hi], rtol=1e-12, atol=0.0)
    without = c.x.copy()
    without[0, j1] = without[0, j1 - 2]
    other = R.limiter_ref(without, c.limit_db, Wa, Wr)
    assert other.r[j1] == 1.0 and np.array_equal(other.d[:hi], ref.d[:hi])
    assert ref.r[j2] < ref.r[j0] and abs(ref.g[j2] - ref.r[j2]) <= 4e-16 and ref.d[j2] > 2.0 * tail[j2]


@pytest.mark.parametrize("sr", R.RATES)
def test_inter_sample_peak_of_a_quarter_rate_sine(sr):
    """(g) sample peaks 0.7071, true peak near 1: limited at L = 0.9 though no sample exceeds L."""
    c, ref = _case(sr, "quarter_sine")
    assert abs(np.abs(c.x).max() - np.sqrt(0.5)) < 1e-6 < ref.L - np.abs(c.x).max()
    mid = slice(100, -100)
    assert np.all(np.abs(ref.p[mid] - 1.0) < 3e-3)
    assert ref.limited == c.x.shape[1] and np.all(ref.g <= 0.9 + 1e-12) and np.all(ref.g > 0.8)
    deep = slice(3 * R.TILE, 4 * R.TILE)                  # far from the edge transients' release
    assert np.all(np.abs(ref.g[deep] - 0.9) < 3e-3)


def test_overshoot_of_the_limited_signal():
    """(h) the independent meter's reading of y against L, every case."""
    worst = 0.0
    for sr, name in ALL:
        c, ref = _case(sr, name)
        if c.x.shape[1] == 0:
            continue
        over = R.meter8(ref.y) / ref.L - 1.0
        print(f"{sr} {name}: meter8(y) / L - 1 = {over:+.6f}")
        worst = max(worst, over)
    print(f"largest overshoot {worst:.6f}")
    assert 0.0 < worst <= OVERSHOOT


def test_meter_agrees_with_the_definitions_estimate():
    """The 4x / 12-crossing estimate of step 1 against the 8x / 32-crossing meter on the inputs."""
    for sr, name in ALL:
        c, ref = _case(sr, name)
        if c.x.shape[1]:
            assert abs(ref.true_peak / R.meter8(c.x) - 1.0) < 0.02, (sr, name)


def limited_is_decidable(ref, bound=GAIN_CAP) -> bool:
    """No sample of d lies within ``bound`` of the float32 threshold 2^-25 (other than at
    exactly 0, which the device reproduces exactly: a window of ones sums to 0)."""
    return not np.any((ref.d > 0.0) & (ref.d <= R.THRESHOLD + bound))


@pytest.mark.parametrize("sr", R.RATES)
def test_cases_where_the_limited_count_must_be_exact(sr):
    """The signals whose `limited` the GPU test compares exactly: d is 0 or above the cap."""
    names = ["under", "tile_edge", "quarter_sine", "empty"] + [c.name for c in R.cases(sr) if c.name.startswith("short_")]
    if sr == 48000:
        names += ["long_tail", "stereo", "tail_peaks"]
    for name in names:
        assert limited_is_decidable(R.reference(sr, name)), name
    # and the long tail stays above float32 resolution for more than 10 Wr samples, across
    # at least three tile boundaries
    c, ref = _case(sr, "long_tail")
    Wr = c.wa_wr[1]
    j0 = c.peaks[0]
    seen = np.nonzero((1.0 - ref.d).astype(np.float32) < 1.0)[0]
    N = c.x.shape[1]
    assert seen.max() - j0 > min(10 * Wr, N - 2 - j0) and seen.max() // R.TILE - j0 // R.TILE >= 3
    assert np.all(np.diff(seen) == 1)


# ------------------------------------------------------------------ the host side of the package
def test_cli_rejects_limit_without_a_render(tmp_path, capsys):
    from nightcore_analyzer import cli
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    a.write_bytes(b"")
    b.write_bytes(b"")
    assert cli.main(["-n", str(a), "-s", str(b), "--limit"]) == 2
    assert "--limit needs --render-hqnc" in capsys.readouterr().err
    assert cli.main(["-n", str(a), "-s", str(b), "--render-hqnc", str(tmp_path / "o.wav"), "--limit", "0.5"]) == 2
    assert "--limit must be at or below 0 dBFS" in capsys.readouterr().err
    args = cli._build_parser().parse_args(["-n", "a", "-s", "b", "--render-hqnc", "o.wav", "--limit"])
    assert args.limit == -0.1
    assert cli._build_parser().parse_args(["-n", "a", "-s", "b", "--limit", "-1.5"]).limit == -1.5
    assert cli._build_parser().parse_args(["-n", "a", "-s", "b"]).limit is None


def test_host_side_of_the_package():
    from pathlib import Path

    from nightcore_analyzer import _native, loudness, ops, render
    for sr in (22050, 44100, 48000):
        assert ops.limiter_windows(sr) == R.windows(sr)
    assert ops.limiter_windows(8000, 0.01, 0.01) == (1, 1)
    info = render.RenderInfo(Path("x.wav"), 1.25, 10, 2, 44100, "pcm16", 0.5, -6.02, 0)
    assert (info.true_peak, info.limited_samples, info.limit_db) == (None, 0, None)
    assert loudness.LimitInfo(1.2, 1.58, 0.98, 7, -0.1, 221, 2205).limited_samples == 7
    with pytest.raises(NotImplementedError):
        loudness.apply_true_peak_limiter("song.flac", "out.wav")
    if not _native.lib_path().exists():
        pytest.skip("libncgpu.so not built")
    # the workspace layout (host only): r and the local release as float rows padded to 64, an
    # aggregate and a carry per 2048-sample tile, every file's region a multiple of 256 bytes
    frames = np.array([0, 1, 2048, 2049, 20517], np.int64)
    off = np.zeros(len(frames), np.int64)
    total = _native.load().nc_limiter_ws_bytes(frames.ctypes.data, len(frames), off.ctypes.data)
    need = [(-(-n // 64) * 64 * 8 + -(-n // 2048) * 16 + 255) // 256 * 256 for n in frames.tolist()]
    assert off.tolist() == np.concatenate([[0], np.cumsum(need)[:-1]]).tolist() and total == sum(need)
    assert _native.load().nc_limiter_ws_bytes(frames.ctypes.data, len(frames), None) == total
