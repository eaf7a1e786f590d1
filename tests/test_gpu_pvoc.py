"""The phase-vocoder pitch shift on the MI355X (pvoc.hip: nc_pv_analyze / nc_pv_scan / nc_pv_synth /
nc_pv_stretch, then nc_speed_render) against its definition (tests/pvoc_ref.py, numpy float64),
stage by stage, and the layers on top: ops.pitch_shift_device, render.pitch_shift / pitch_file /
refine_pitch and the CLI's --pitch-correct.

Inputs are uniform +-1 noise unless stated: a bin far below its frame's maximum has a poorly
determined phase which the scan carries forward (the method's own conditioning), so
sample values are compared on broadband inputs.  Tolerances: 4x the largest deviation of the
first MI355X run (recorded in DESIGN.md §2), capped at 2e-5 for the stages and at 1e-3 max|x| for
the whole stretch (one bin of one frame with a wrong phase moves s by about 2e-2 on this noise;
f32 FFT rounding is predicted to move it by at most 6e-5)."""
import contextlib
import io as stdio
import math

import numpy as np
import pytest
import torch

import pvoc_ref as R
from nightcore_analyzer import cli, engine as E, io as nio, ops, pitch, render, synth
from oracle import refglue

pytestmark = pytest.mark.gpu

LENGTHS = [1, 511, 513, 2048, 5000]
RATIOS = [500_000, 943_874, 1_000_000, 1_000_001, 1_059_463, 2_000_000]
SR = 22050

# 4 x the largest deviation of the first MI355X run; none reaches its cap
T_MAG = 1.32e-6     # |mag - ref| / max_b ref per frame: one t for the analysis, 4 x 3.29e-7 (cap 2e-5)
T_PHASOR = 1.32e-6  # mag_A mag_B |V - V_ref| / (max|A| max|B|) (largest seen 2.36e-7)
T_SCAN = 2.4e-7     # |Phi - ref|: the f32 store of an f64 product (largest seen 4.2e-8)
T_SYNTH = 8.0e-7    # |s - ref| / max|s_ref|, synthesis alone: 4 x 1.99e-7 (cap 2e-5)
T_STRETCH = 2.0e-5  # |s - ref| / max|x|, the whole stretch: 4 x 5.01e-6 (cap 1e-3)
T_RENDER = 1e-5     # the speed render's own bound, per unit of max(1, max|s|) (tests/test_gpu_render.py)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def _gap_case():
    x = _noise(20000, 99)
    x[:3000] = 0.0
    x[9000:15000] = 0.0
    return x


def _c(t):
    """[.., 2] float32 device rows -> complex128 host."""
    h = t.cpu().numpy().astype(np.float64)
    return h[..., 0] + 1j * h[..., 1]


def _stretch(eng, xs, P):
    out, peak, plan = ops.pv_stretch_device(eng, xs, P)
    h = out.buf.cpu().numpy()
    return [h[o:o + n].copy() for o, n in zip(out.off, out.length)], peak.cpu().numpy(), plan


# ------------------------------------------------------------------ 1. analysis
@pytest.mark.parametrize("P", RATIOS)
def test_analysis(eng, P):
    xs = [_noise(n, 7 * n + P % 1000) for n in LENGTHS] + [_gap_case()]
    mag, v, empty, plan = ops.pv_analyze_device(eng, xs, P)
    mag, v, empty = mag.cpu().numpy().astype(np.float64), _c(v), empty.cpu().numpy()
    worst_m = worst_v = 0.0
    for f, x in enumerate(xs):
        Ns, K = R.plan(len(x), P)
        assert (int(plan.ns[f]), int(plan.k[f])) == (Ns, K)
        g0, g1 = int(plan.frame_base[f]), int(plan.frame_base[f + 1])
        assert g1 - g0 == K
        rm, rv, re, A, B = R.analyze(x, P)
        assert np.array_equal(empty[g0:g1].astype(bool), re), (f, P)
        reset = R.resets(re)
        top_a = np.maximum(np.max(np.abs(A), axis=1, keepdims=True), 1e-30)      # an all-zero frame: 0 / 1e-30
        top_b = np.where(reset[:, None], 1.0, np.maximum(np.max(np.abs(B), axis=1, keepdims=True), 1e-30))
        wb = np.where(reset[:, None], 1.0, np.abs(B))
        em = np.max(np.abs(mag[g0:g1] - rm) / top_a)
        ev = np.max(np.abs(A) * wb * np.abs(v[g0:g1] - rv) / (top_a * top_b))
        worst_m, worst_v = max(worst_m, em), max(worst_v, ev)
        # an empty frame is exactly zero, and its phasors are (1, 0)
        assert not np.any(mag[g0:g1][re]) and np.all(v[g0:g1][re] == 1.0)
    print(f"pv_analysis P={P}: mag {worst_m:.3e} phasor {worst_v:.3e}")
    assert worst_m <= T_MAG and worst_v <= T_PHASOR
    if P == RATIOS[0]:
        re = R.analyze(xs[-1], P)[2]
        assert re[:2].all() and re.sum() >= 5 and not re.all()     # the leading zeros and the gap are seen


# ------------------------------------------------------------------ 2. the scan alone
def test_scan_alone(eng):
    T = ops.PV_TILE
    Ks = [1, 2, T - 1, T, T + 1, 3 * T + 5]
    rng = np.random.default_rng(5)
    fb = np.concatenate([[0], np.cumsum(Ks)])
    total = int(fb[-1])
    ang = rng.uniform(-np.pi, np.pi, (total, ops.PV_BINS))
    v32 = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)
    empty = (rng.uniform(size=total) < 0.06).astype(np.uint8)
    empty[fb[5] + T - 1] = 1            # a reset on the first frame of a tile
    empty[fb[5] + 2 * T - 2] = 1        # ... and on the last
    v_d, e_d = torch.from_numpy(v32).to(eng.dev), torch.from_numpy(empty).to(eng.dev)
    phi = _c(ops.pv_scan_device(eng, v_d, e_d, fb))
    vc = v32[..., 0].astype(np.float64) + 1j * v32[..., 1].astype(np.float64)
    worst = 0.0
    for f, K in enumerate(Ks):
        a, b = int(fb[f]), int(fb[f + 1])
        ref = R.scan(vc[a:b], empty[a:b].astype(bool))
        worst = max(worst, float(np.max(np.abs(phi[a:b] - ref))))
        # a file alone: the same bits (the tiling follows the file's own frame index)
        one = _c(ops.pv_scan_device(eng, v_d[a:b], e_d[a:b], [0, K]))
        assert np.array_equal(one, phi[a:b]), K
    print(f"pv_scan: max |Phi - ref| {worst:.3e}")
    assert worst <= T_SCAN


# ------------------------------------------------------------------ 3. the synthesis alone
def test_synth_alone(eng):
    lengths = [300, 1000, 5000]                    # K = 4, 5, 13 at P = Q
    plan = ops.PvPlan(R.Q, lengths)
    assert plan.k.tolist() == [4, 5, 13]
    rng = np.random.default_rng(6)
    total = plan.total_frames
    mag32 = rng.uniform(0.0, 50.0, (total, ops.PV_BINS)).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, (total, ops.PV_BINS))
    phi32 = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)
    out, peak = ops.pv_synth_device(eng, torch.from_numpy(mag32).to(eng.dev), torch.from_numpy(phi32).to(eng.dev),
                                    lengths, R.Q)
    h, peak = out.buf.cpu().numpy(), peak.cpu().numpy()
    pc = phi32[..., 0].astype(np.float64) + 1j * phi32[..., 1].astype(np.float64)
    worst = 0.0
    for f, n in enumerate(lengths):
        a, b = int(plan.frame_base[f]), int(plan.frame_base[f + 1])
        ref = R.synth(mag32[a:b].astype(np.float64), pc[a:b], n)
        s = h[out.off[f]:out.off[f] + out.length[f]]
        assert len(s) == n
        worst = max(worst, float(np.max(np.abs(s - ref)) / np.max(np.abs(ref))))
        assert peak.dtype == np.float32 and float(peak[f]) == float(np.max(np.abs(s)))
    print(f"pv_synth: max |s - ref| / max|s_ref| {worst:.3e}")
    assert worst <= T_SYNTH


# ------------------------------------------------------------------ 4. the stretch
@pytest.mark.parametrize("P", RATIOS)
def test_stretch(eng, P):
    xs = [_noise(n, 13 * n + P % 1000) for n in LENGTHS]
    ss, peaks, plan = _stretch(eng, xs, P)
    worst = 0.0
    for x, s, pk in zip(xs, ss, peaks):
        ref = R.stretch(x, P)
        assert s.dtype == np.float32 and len(s) == len(ref) == R.plan(len(x), P)[0]
        worst = max(worst, float(np.max(np.abs(s - ref)) / np.max(np.abs(x))))
        assert float(pk) == float(np.max(np.abs(s)))
    print(f"pv_stretch P={P}: max |s - ref| / max|x| {worst:.3e}")
    assert worst <= T_STRETCH


@pytest.mark.parametrize("P", [500_000, 1_059_463, 2_000_000])
def test_stretch_40000(eng, P):
    x = _noise(40000, P % 977)
    (s,), _, _ = _stretch(eng, [x], P)
    ref = R.stretch(x, P)
    err = float(np.max(np.abs(s - ref)) / np.max(np.abs(x)))
    print(f"pv_stretch n=40000 P={P}: {err:.3e}")
    assert len(s) == len(ref) and err <= T_STRETCH


def test_stretch_edges(eng):
    """An empty file beside others, silence, and the argument errors."""
    xs = [_noise(700, 1), np.zeros(0, np.float32), np.zeros(3000, np.float32), _noise(64, 2)]
    ss, peaks, plan = _stretch(eng, xs, 1_059_463)
    assert plan.k.tolist() == [R.plan(len(x), 1_059_463)[1] for x in xs] and plan.k[1] == 0
    assert len(ss[1]) == 0 and float(peaks[1]) == 0.0
    assert len(ss[2]) == R.plan(3000, 1_059_463)[0] and not np.any(ss[2]) and float(peaks[2]) == 0.0
    for i in (0, 3):
        (one,), _, _ = _stretch(eng, [xs[i]], 1_059_463)
        assert np.array_equal(one.view(np.uint32), ss[i].view(np.uint32))
    from nightcore_analyzer import _native
    for P in (499_999, 2_000_001):
        with pytest.raises(_native.NativeError, match="ratio outside"):
            ops.PvPlan(P, [100])
    # a workspace below the plan's is refused before anything is launched
    sig = eng.upload_signals([xs[0]])
    p = ops.PvPlan(R.Q, sig.length)
    off = torch.zeros(1, dtype=torch.int64, device=eng.dev)
    ln = torch.tensor([700], dtype=torch.int64, device=eng.dev)
    fb = torch.from_numpy(p.frame_base).to(eng.dev)
    s = torch.zeros(1024, dtype=torch.float32, device=eng.dev)
    pk = torch.zeros(1, dtype=torch.float32, device=eng.dev)
    ws = torch.empty(p.ws_bytes, dtype=torch.uint8, device=eng.dev)
    with pytest.raises(_native.NativeError, match="workspace"):
        eng.call("nc_pv_stretch", sig.buf.data_ptr(), off.data_ptr(), ln.data_ptr(), fb.data_ptr(), 1, p.total_frames,
                 p.max_frames, p.P, p.max_ns, s.data_ptr(), off.data_ptr(), pk.data_ptr(), ws.data_ptr(),
                 p.ws_off.ctypes.data, p.ws_bytes - 1, eng.stream())


# ------------------------------------------------------------------ 5. batch
def test_batch_is_bit_identical(eng):
    xs = [_noise(5000, 1), _noise(1, 2), _noise(777, 3)]
    for P in (840_896, 1_259_921):
        ss, peaks, _ = _stretch(eng, xs, P)
        ss2, peaks2, _ = _stretch(eng, xs, P)
        for i, x in enumerate(xs):
            (one,), pk, _ = _stretch(eng, [x], P)
            assert np.array_equal(ss[i].view(np.uint32), one.view(np.uint32)), (P, i)
            assert np.array_equal(ss[i].view(np.uint32), ss2[i].view(np.uint32)), (P, i)
            assert float(peaks[i]) == float(pk[0]) == float(peaks2[i])


# ------------------------------------------------------------------ 6. long positions
def test_long_position_arithmetic(eng):
    """c_k Q passes 2^40 in a 3 000 000-sample file: the last 8 analysis frames against the
    definition evaluated on the matching input slice."""
    n, P, tail = 3_000_000, 1_234_567, 8
    x = _noise(n, 77)
    mag, v, empty, plan = ops.pv_analyze_device(eng, [x], P)
    Ns, K = R.plan(n, P)
    assert plan.total_frames == K and (K - 2) * R.HS * R.Q > 1 << 40
    k0 = K - tail
    base = int(R.centres(k0, P, k0 - 1)[0]) - R.N // 2 - R.HS - 8
    rm, rv, re, A, B = R.analyze(x[base:], P, k0=k0, base=base, n=n)
    gm, gv = mag[k0:].cpu().numpy().astype(np.float64), _c(v[k0:])
    # the last frame still reaches into the file: none of the eight is empty, none is a reset frame
    assert len(re) == tail and not re.any() and not empty[k0 - 1:].cpu().numpy().any()
    top_a, top_b = np.max(np.abs(A), axis=1, keepdims=True), np.max(np.abs(B), axis=1, keepdims=True)
    em = float(np.max(np.abs(gm - rm) / top_a))
    ev = float(np.max(np.abs(A) * np.abs(B) * np.abs(gv - rv) / (top_a * top_b)))
    print(f"pv_analysis tail of n={n}: mag {em:.3e} phasor {ev:.3e}")
    assert em <= T_MAG and ev <= T_PHASOR


# ------------------------------------------------------------------ 7. pitch_shift
def _tone(n, seed=5, hz=440.0):
    t = np.arange(n) / SR
    return (np.sin(2 * np.pi * hz * t) + 0.01 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _peak_hz(y):
    y = np.asarray(y, np.float64)
    a = y[len(y) // 4: 3 * len(y) // 4]
    nfft = 8 * (1 << int(np.ceil(np.log2(len(a)))))
    m = np.abs(np.fft.rfft(a * np.hanning(len(a)), nfft))
    k = int(np.argmax(m))
    l0, l1, l2 = np.log(m[k - 1:k + 2])
    return (k + 0.5 * (l0 - l2) / (l0 - 2 * l1 + l2)) * SR / nfft


def test_pitch_shift_moves_a_tone(eng):
    x = _tone(4 * SR)
    for st in (-2.0, 0.5, 3.0):
        y = render.pitch_shift(x, st)
        P = R.semitones_p(st)
        hz = _peak_hz(y)
        print(f"pitch_shift {st:+.1f} st: peak {hz:.4f} Hz, wanted {440.0 * P / R.Q:.4f}")
        assert y.dtype == np.float32 and len(y) == len(x)
        assert render.quantize_semitones(st) == P / R.Q
        assert abs(hz / (440.0 * P / R.Q) - 1.0) <= 2e-4


@pytest.fixture(scope="module")
def shifted20(eng):
    src = synth.make_source(20.0, 1000)
    return src, render.pitch_shift(src, 2.0)


def test_pitch_shift_chroma(eng, shifted20):
    src, shifted = shifted20
    assert len(shifted) == len(src)
    assert pitch._chroma_shift_for_chunk(src, shifted, SR) == 2 / 3.0
    assert pitch._chroma_shift_for_chunk(src, src, SR) == 0.0


def test_pitch_shift_device_form(eng):
    xs = [_noise(3000, 4), _noise(1000, 5)]
    sig = eng.upload_signals(xs)
    out, peak, P = ops.pitch_shift_device(eng, sig, 1.0)
    assert P == R.semitones_p(1.0) == 1_059_463 and out.buf.is_cuda
    assert out.length.tolist() == [3000, 1000] and all(int(o) % 64 == 0 for o in out.off)
    ys = ops.pitch_shift(eng, xs, 1.0)
    h = out.buf.cpu().numpy()
    for i, x in enumerate(xs):
        assert np.array_equal(h[out.off[i]:out.off[i] + len(x)], ys[i])
        ref = R.pitch_shift(x, P=P)
        assert np.max(np.abs(ys[i] - ref)) <= T_STRETCH + 2 * T_RENDER      # |s| stays below 2 on this noise
    with pytest.raises(ValueError):
        ops.pitch_shift_device(eng, sig, 12.5)


# ------------------------------------------------------------------ 8. pitch_file
def _speed_file_signals():
    rng = np.random.default_rng(21)
    t = np.arange(3001) / 44100.0
    return np.stack([0.6 * np.sin(2 * np.pi * 997.0 * t) + 0.2 * rng.uniform(-1, 1, len(t)),
                     0.3 * np.sin(2 * np.pi * 4001.0 * t) + 0.5 * rng.uniform(-1, 1, len(t))])


def test_pitch_file(eng, tmp_path):
    ch = _speed_file_signals()
    q = np.rint(ch * 32767).astype(np.int16)
    src = tmp_path / "Song.wav"
    dst = render.ps_path(src, 1)
    assert dst.name == "Song PS1.wav"
    nio.write_wav(src, q, 44100, "pcm16")
    info = render.pitch_file(src, dst, 1.0)
    P = R.semitones_p(1.0)
    assert (info.semitones, info.factor, info.n_out, info.channels, info.sample_rate, info.sample_format) == \
        (1.0, P / R.Q, 3001, 2, 44100, "pcm16")
    back, sr, fmt = nio.read_wav_channels(dst)
    assert (sr, fmt, back.shape) == (44100, "pcm16", (2, 3001))
    step = 1.0 / 32768
    over = 0
    for c in range(2):
        x = q[c].astype(np.float32) / 32768.0
        ref = R.pitch_shift(x, P=P)
        # the shifted second channel passes full scale by 0.0089 in one sample: a 16-bit file holds
        # the clamped value, and the clamp is counted
        v = np.rint(ref * 32768.0)
        over += int(np.count_nonzero((v > 32767) | (v < -32768)))
        err = float(np.max(np.abs(back[c] - np.clip(ref, -1.0, 32767.0 / 32768.0))))
        print(f"pitch_file channel {c}: {err:.3e}")
        assert err <= step + T_STRETCH * float(np.max(np.abs(x))), c
    assert over == 1 and info.clipped_samples == over and info.is_clipping and info.limit_db is None
    # a float file above full scale, limited on the resident result
    fsrc, fdst = tmp_path / "f.wav", tmp_path / "f out.wav"
    nio.write_wav(fsrc, (ch * 1.5).astype(np.float32), 48000, "float32")
    finfo = render.pitch_file(fsrc, fdst, -2.0, limit_db=-0.1)
    fback, sr, fmt = nio.read_wav_channels(fdst)
    L = float(np.float32(10 ** (-0.1 / 20)))
    assert (sr, fmt, fback.shape) == (48000, "float32", (2, 3001))
    assert float(np.max(np.abs(fback))) <= L and finfo.peak == float(np.max(np.abs(fback)))
    assert finfo.limit_db == -0.1 and finfo.limited_samples > 0 and finfo.true_peak > L
    with pytest.raises(ValueError):
        render.pitch_file(fsrc, fdst, 1.0, limit_db=0.5)


# ------------------------------------------------------------------ 9. refine_pitch
def test_refine_pitch_with_start(eng, shifted20):
    src, shifted = shifted20
    lines = []
    ref = render.refine_pitch(shifted, src, start=2.0, log=lines.append)
    print(f"refine_pitch: shifts {ref.shifts} residuals {ref.residuals} method {ref.method}")
    assert ref.shifts == [2.0] and ref.residuals == [0.0] and ref.converged and ref.corrections == 0
    assert isinstance(ref.render, nio.DeviceAudio) and ref.render.tensor.is_cuda and len(ref.render) == len(src)
    assert np.array_equal(ref.render.numpy(), shifted)
    assert any(line.startswith("Render 1: pitch +2.000000 st") for line in lines)
    # below the threshold nothing is rendered
    none = render.refine_pitch(shifted, src, start=0.3)
    assert none.converged and none.shifts == [] and none.render is None


def test_refine_pitch_first_shift_is_the_oracles(eng):
    nc, src = synth.make_pair(40.0, 1022, up=5, down=6)
    s_hz, n_hz = refglue.estimate_pitch_chroma(src, nc)[:2]
    want = 12.0 * math.log2(float(np.median(n_hz)) / float(np.median(s_hz)))
    ref = render.refine_pitch(nc, src)
    print(f"refine_pitch: initial {ref.initial!r} (oracle {want!r}) shifts {ref.shifts} residuals {ref.residuals}")
    assert ref.initial == want
    assert abs(want) >= 0.5 and ref.shifts[0] == round(want, 6) and len(ref.residuals) == len(ref.shifts) <= 4


# ------------------------------------------------------------------ 10. CLI
def _run_cli(argv):
    out, err = stdio.StringIO(), stdio.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = cli.main(argv)
    return rc, out.getvalue(), err.getvalue()


def test_cli_pitch_correct(eng, tmp_path):
    nc, src = synth.make_pair(40.0, 1022)
    ncp, srp, ps = tmp_path / "nc.wav", tmp_path / "src.wav", tmp_path / "src PS1.wav"
    nio.write_wav(ncp, nc, 22050, "pcm16")
    nio.write_wav(srp, src, 22050, "pcm16")
    rc, out, err = _run_cli(["-n", str(ncp), "-s", str(srp), "--pitch-correct", str(ps)])
    assert rc == 2 and "--pitch-correct needs --semitones" in err and out == ""
    rc, out, err = _run_cli(["-n", str(ncp), "-s", str(srp), "--semitones", "1.5"])
    assert rc == 2 and "--semitones needs --pitch-correct" in err and out == ""
    assert not ps.exists()
    rc, out, _ = _run_cli(["-n", str(ncp), "-s", str(srp), "--pitch-correct", str(ps), "--semitones", "-1.5",
                           "--limit"])
    assert rc == 0 and "Pitch-corrected file written to:" in out and "pitch -1.500000 st" in out
    assert "Limiter at -0.10 dBFS" in out
    back, sr, fmt = nio.read_wav_channels(ps)
    assert (sr, fmt, back.shape) == (22050, "pcm16", (1, len(src)))
    ps.unlink()
    rc, out, _ = _run_cli(["-n", str(ncp), "-s", str(srp), "-q", "-o", str(tmp_path / "a.json"),
                           "--pitch-correct", str(ps), "--semitones", "-1.5"])
    assert (rc, out) == (0, "") and nio.read_wav_channels(ps)[0].shape == (1, len(src))
