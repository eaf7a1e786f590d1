"""The pitch shift's definition (tests/pvoc_ref.py, numpy float64) checked on its own: what
the phase vocoder must do whatever computes it.  No device, no library."""
import numpy as np
import pytest

import pvoc_ref as R
from nightcore_analyzer import synth
from oracle import refglue

SR = 22050
RATIOS = [500_000, 707_107, 840_896, 1_259_921, 2_000_000]


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def _tone(n, seed=5, hz=440.0):
    t = np.arange(n) / SR
    return np.sin(2 * np.pi * hz * t) + 0.01 * np.random.default_rng(seed).standard_normal(n)


def _peak_hz(y):
    """Frequency of the largest spectral peak of the steady part (Hann, 8x zero padding,
    parabolic interpolation on the log magnitude)."""
    y = np.asarray(y, np.float64)
    a = y[len(y) // 4: 3 * len(y) // 4]
    nfft = 8 * (1 << int(np.ceil(np.log2(len(a)))))
    m = np.abs(np.fft.rfft(a * np.hanning(len(a)), nfft))
    k = int(np.argmax(m))
    l0, l1, l2 = np.log(m[k - 1:k + 2])
    return (k + 0.5 * (l0 - l2) / (l0 - 2 * l1 + l2)) * SR / nfft


def _steady_rms(y):
    a = np.asarray(y)[len(y) // 4: 3 * len(y) // 4]
    return float(np.sqrt(np.mean(a * a)))


PLAN_TABLE = {
    (1, 500_000): (1, 4), (1, 943_874): (1, 4), (1, 1_000_000): (1, 4), (1, 1_000_001): (2, 4),
    (1, 1_059_463): (2, 4), (1, 2_000_000): (2, 4),
    (511, 500_000): (256, 4), (511, 943_874): (483, 4), (511, 1_000_000): (511, 4), (511, 1_000_001): (512, 4),
    (511, 1_059_463): (542, 5), (511, 2_000_000): (1022, 5),
    (513, 500_000): (257, 4), (513, 943_874): (485, 4), (513, 1_000_000): (513, 5), (513, 1_000_001): (514, 5),
    (513, 1_059_463): (544, 5), (513, 2_000_000): (1026, 6),
    (2048, 500_000): (1024, 5), (2048, 943_874): (1934, 7), (2048, 1_000_000): (2048, 7),
    (2048, 1_000_001): (2049, 8), (2048, 1_059_463): (2170, 8), (2048, 2_000_000): (4096, 11),
    (5000, 500_000): (2500, 8), (5000, 943_874): (4720, 13), (5000, 1_000_000): (5000, 13),
    (5000, 1_000_001): (5001, 13), (5000, 1_059_463): (5298, 14), (5000, 2_000_000): (10000, 23),
}


@pytest.mark.parametrize("case", sorted(PLAN_TABLE))
def test_plan_table(case):
    n, P = case
    Ns, K = R.plan(n, P)
    assert (Ns, K) == PLAN_TABLE[case]
    # the table's values restated: exact ceilings in integers
    assert Ns == (n * P + R.Q - 1) // R.Q and K == (Ns + R.HS - 1) // R.HS + 3


def test_plan_limits():
    assert R.plan(0, R.Q) == (0, 0)
    for P in (499_999, 2_000_001):
        with pytest.raises(ValueError):
            R.plan(10, P)
    assert R.semitones_p(12.0) == 2_000_000 and R.semitones_p(-12.0) == 500_000 and R.semitones_p(0.0) == R.Q
    with pytest.raises(ValueError):
        R.semitones_p(12.5)


def test_every_stretched_sample_has_four_frames():
    for (n, P), (Ns, K) in PLAN_TABLE.items():
        J = K - 3
        assert (J - 1) * R.HS < Ns <= J * R.HS
        # frame k covers [(k - 3) Hs, (k + 1) Hs): block j is inside frames j .. j + 3 and no other
        for j in (0, J - 1):
            cover = [k for k in range(K) if (k - 3) * R.HS <= j * R.HS and (j + 1) * R.HS <= (k + 1) * R.HS]
            assert cover == [j, j + 1, j + 2, j + 3]


def test_window_sums_to_three_halves():
    ola = sum(R.W[d * R.HS:(d + 1) * R.HS] ** 2 for d in range(4))
    assert np.max(np.abs(ola - 1.5)) < 1e-14


@pytest.mark.parametrize("n", [1, 511, 513, 2048, 5000, 20000])
def test_identity(n):
    x = _noise(n, n)
    s = R.stretch(x, R.Q)
    err = float(np.max(np.abs(s - x)))
    print(f"identity n={n}: {err:.2e}")
    assert len(s) == n and err <= 1e-12
    y = R.pitch_shift(x, 0.0)
    assert len(y) == n


@pytest.mark.parametrize("P", [840_896, 1_059_463, 1_259_921])
def test_stretch_keeps_pitch(P):
    x = _tone(4 * SR)
    s = R.stretch(x, P)
    hz, ratio = _peak_hz(s), _steady_rms(s) / _steady_rms(x)
    print(f"stretch P={P}: peak {hz:.4f} Hz, rms ratio {ratio:.3f}")
    assert len(s) == R.plan(len(x), P)[0]
    assert abs(hz - 440.0) <= 0.05
    assert 0.9 <= ratio <= 1.02


@pytest.mark.parametrize("st", [-2.0, 0.5, 3.0])
def test_shift_moves_pitch(st):
    x = _tone(4 * SR)
    y = R.pitch_shift(x, st)
    P = R.semitones_p(st)
    hz = _peak_hz(y)
    print(f"shift {st:+.1f} st: peak {hz:.4f} Hz, wanted {440.0 * P / R.Q:.4f}")
    assert len(y) == len(x)
    assert abs(hz / (440.0 * P / R.Q) - 1.0) <= 2e-4


def _stretch_without_reset_rule(x, P):
    Ns, K = R.plan(len(x), P)
    mag, _, _, A, B = R.analyze(x, P)
    V = R.ph(A * np.conj(B))
    V[0] = R.ph(A[0])
    return R.synth(mag, R.scan(V, np.zeros(K, bool)), Ns)


@pytest.mark.parametrize("P", RATIOS)
def test_reset_rule_keeps_the_onset_clean(P):
    x = _noise(20000, 11)
    s = R.stretch(x, P)
    head, whole = float(np.max(np.abs(s[:8 * R.HS]))), float(np.max(np.abs(s)))
    print(f"P={P}: first eight blocks {head:.3f}, whole {whole:.3f}")
    assert head <= 2.0


def test_reset_rule_matters():
    x = _noise(20000, 11)
    bad = _stretch_without_reset_rule(x, 500_000)
    good = R.stretch(x, 500_000)
    b, g = float(np.max(np.abs(bad[:8 * R.HS]))), float(np.max(np.abs(good[:8 * R.HS])))
    print(f"without the reset rule {b:.2f}, with it {g:.2f}")
    assert b > 2.0 >= g


def test_silence():
    for P in (500_000, 1_059_463, 2_000_000):
        s = R.stretch(np.zeros(3000), P)
        assert len(s) == R.plan(3000, P)[0] and not np.any(s)
        assert not np.any(R.pitch_shift(np.zeros(3000), P=P))
    x = _noise(30000, 3)
    x[9000:21000] = 0.0
    for P in (840_896, 1_259_921):
        s = R.stretch(x, P)
        # frames whose analysis span lies inside the gap are empty: their stretched blocks are zero
        # (centre in [9000 + N/2, 21000 - N/2]); a stretched sample's four frames have their
        # centres within N of it
        lo = -(-(9000 + R.N // 2) * P // R.Q) + R.N
        hi = (21000 - R.N // 2) * P // R.Q - R.N
        assert hi - lo > 1000
        assert not np.any(s[lo:hi])
        assert np.max(np.abs(s[hi + 4 * R.N:])) > 0.1


def test_host_plan_matches_the_definition():
    """nc_pv_plan (host only) against plan(): lengths, frame counts, bases, a workspace whose
    regions do not overlap; -2 outside the ratio range."""
    from nightcore_analyzer import _native, ops
    if not _native.lib_path().exists():
        pytest.skip("libncgpu.so not built")
    lengths = [1, 511, 513, 2048, 5000, 0, 3_000_000]
    for P in (500_000, 943_874, 1_000_000, 1_000_001, 1_059_463, 1_234_567, 2_000_000):
        p = ops.PvPlan(P, lengths)
        want = [R.plan(n, P) for n in lengths]
        assert p.ns.tolist() == [w[0] for w in want] and p.k.tolist() == [w[1] for w in want]
        assert p.frame_base.tolist() == np.concatenate([[0], np.cumsum(p.k)]).tolist()
        t = p.total_frames
        sizes = [t * 1025 * 4, t * 1025 * 8, t * 1025 * 8, t * 2048 * 4, t,
                 int(_native.load().nc_pv_scan_ws_bytes(t, len(lengths)))]
        ends = p.ws_off.tolist()[1:] + [p.ws_bytes]
        assert all(o % 256 == 0 and o + s <= e for o, s, e in zip(p.ws_off.tolist(), sizes, ends))
    for P in (499_999, 2_000_001):
        with pytest.raises(_native.NativeError, match="ratio outside"):
            ops.PvPlan(P, [10])
    assert ops.PvPlan(R.Q, []).total_frames == 0


def test_fft_kernels_do_not_spill(tmp_path):
    """pv_analysis / pv_synth read their FFT exchanges through the batched LDS loads of
    nc_device.h (outputs tied to registers only at their wait): no scratch, as for stft_mel
    (tests/test_kernel_resources_cpu.py)."""
    from test_kernel_resources_cpu import _kernels
    k = _kernels(tmp_path)
    for name in ("pv_analysis_kernel", "pv_synth_kernel"):
        hit = [v for n, v in k.items() if name in n]
        assert hit and all(v[0] == 0 for v in hit), (name, hit)


def test_semitone_quantisation_and_names():
    from nightcore_analyzer import ops, render
    for st in (-12.0, -2.0, 0.0, 0.5, 1.0, 3.0, 12.0):
        assert ops.pitch_p(st) == R.semitones_p(st)
        assert render.quantize_semitones(st) == R.semitones_p(st) / R.Q
    assert ops.pitch_p(1.0000004) == ops.pitch_p(1.0)            # six decimals, as `--pitch {S:+.6f}`
    for bad in (12.5, -13.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            render.quantize_semitones(bad)
    assert render.ps_path("/a/Song [Nightcore].wav", 2).name == "Song [Nightcore] PS2.wav"


def test_cli_flag_misuse_exits_2(tmp_path, capsys):
    from nightcore_analyzer import cli
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    a.write_bytes(b"")
    b.write_bytes(b"")
    assert cli.main(["-n", str(a), "-s", str(b), "--pitch-correct", str(tmp_path / "o.wav")]) == 2
    assert "--pitch-correct needs --semitones" in capsys.readouterr().err
    assert cli.main(["-n", str(a), "-s", str(b), "--semitones", "1"]) == 2
    assert "--semitones needs --pitch-correct" in capsys.readouterr().err
    assert cli.main(["-n", str(a), "-s", str(b), "--pitch-correct", str(tmp_path / "o.wav"), "--semitones", "13"]) == 2
    assert "--semitones must be within" in capsys.readouterr().err
    args = cli._build_parser().parse_args(["-n", "a", "-s", "b", "--pitch-correct", "o.wav", "--semitones", "-1.5",
                                           "--limit"])
    assert (args.pitch_correct, args.semitones, args.limit) == ("o.wav", -1.5, -0.1)


def test_chroma_lag_of_a_shifted_source():
    src = synth.make_source(20.0, 1000)
    assert refglue.chunk_lag(src, src) == 0
    shifted = R.pitch_shift(src, 2.0).astype(np.float32)
    assert len(shifted) == len(src)
    assert refglue.chunk_lag(src, shifted) == 2
