"""Identity phase locking with linked channels on the MI355X (pvoc.hip: nc_pv_analyze_u / nc_pv_lock /
nc_pv_mid_sum / nc_pv_rotate, then nc_pv_synth) against its definition (tests/pvoc_lock_ref.py,
numpy float64), stage by stage, and the layers on top: ops.pv_stretch_device(lock="identity"),
render.pitch_shift / pitch_file / refine_pitch(phase_lock=True) and the CLI's --phase-lock.

Inputs are uniform +-1 noise unless stated, as in tests/test_gpu_pvoc.py.  The reference of a
whole stretch is evaluated with the owners the device's lock stage returns for the same input: the
f32 / f64 near-ties of mag then cannot flip a region; the owners themselves are compared exactly on
the lock stage alone.  Tolerances: 4x the largest deviation of the first MI355X run (recorded in
DESIGN.md §2), capped at 2e-5 for the U and lock stages and at 1e-3 max|x| for a whole stretch."""
import contextlib
import io as stdio

import numpy as np
import pytest
import torch

import pvoc_lock_ref as L
import pvoc_ref as R
from nightcore_analyzer import cli, engine as E, io as nio, ops, pitch, render, synth
from pvoc_lock_ref import rms, running_rms_spread, stereo_pair, unexplained, vibrato_tone

pytestmark = pytest.mark.gpu

LENGTHS = [1, 511, 513, 2048, 5000]
RATIOS = [500_000, 943_874, 1_000_000, 1_000_001, 1_059_463, 2_000_000]
SR = 22050

# 4 x the largest deviation of the first MI355X run; none reaches its cap, and the caps are conditions
T_U = 7.3e-7        # |A| |U - ph(A)| / max_b |A| per frame: 4 x 1.812e-7 (cap 2e-5)
T_LOCK = 1.33e-6    # |Phi - ref| of the lock stage alone: 4 x 3.324e-7, M is stored in f32 (cap 2e-5)
T_STRETCH = 6.8e-6  # |s - ref| / max|x|, the whole locked or linked stretch: 4 x 1.682e-6 (cap 1e-3)


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
    h = t.cpu().numpy().astype(np.float64)
    return h[..., 0] + 1j * h[..., 1]


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _own(t):
    return t.cpu().numpy().view(np.uint16)


def _stretch(eng, xs, P, lock="identity", channels=1):
    out, peak, plan = ops.pv_stretch_device(eng, xs, P, lock=lock, channels=channels)
    h = out.buf.cpu().numpy()
    return [h[o:o + n].copy() for o, n in zip(out.off, out.length)], peak.cpu().numpy(), plan


def _device_owners(eng, xs, P):
    """The lock stage's owners of every file of ``xs``, by the stage ops."""
    mag, v, empty, plan, u = ops.pv_analyze_device(eng, xs, P, phasors=True)
    _, owner = ops.pv_lock_device(eng, mag, u, v, empty, plan.frame_base)
    owner = _own(owner)
    return [owner[int(a):int(b)] for a, b in zip(plan.frame_base[:-1], plan.frame_base[1:])]


# ------------------------------------------------------------------ 1. the analysis phasor U
@pytest.mark.parametrize("P", [500_000, 1_059_463, 2_000_000])
def test_analysis_u(eng, P):
    xs = [_noise(n, 7 * n + P % 1000) for n in LENGTHS] + [_gap_case()]
    mag, v, empty, plan, u = ops.pv_analyze_device(eng, xs, P, phasors=True)
    mag0, v0, empty0, plan0 = ops.pv_analyze_device(eng, xs, P)
    assert np.array_equal(_bits(mag), _bits(mag0)) and np.array_equal(_bits(v), _bits(v0))
    assert np.array_equal(empty.cpu().numpy(), empty0.cpu().numpy())
    assert np.array_equal(plan.frame_base, plan0.frame_base)
    ub, vb, uc = _bits(u), _bits(v), _c(u)
    worst, n_reset = 0.0, 0
    for f, x in enumerate(xs):
        g0, g1 = int(plan.frame_base[f]), int(plan.frame_base[f + 1])
        _, _, re, A, _ = R.analyze(x, P)
        reset = R.resets(re)
        top = np.maximum(np.max(np.abs(A), axis=1, keepdims=True), 1e-30)
        worst = max(worst, float(np.max(np.abs(A) * np.abs(uc[g0:g1] - R.ph(A)) / top)))
        assert np.array_equal(ub[g0:g1][reset], vb[g0:g1][reset]), (f, P)      # U == V bit for bit on a reset frame
        assert np.all(uc[g0:g1][re] == 1.0)                                     # an empty frame: (1, 0)
        n_reset += int(reset.sum())
    print(f"pv_analysis U P={P}: {worst:.3e} ({n_reset} reset frames)")
    assert n_reset > len(xs) and worst <= T_U


# ------------------------------------------------------------------ 2. the lock stage alone
KS = [1, 2, 63, 64, 65, 197]


def _lock_inputs(case):
    T = ops.PV_TILE
    rng = np.random.default_rng({"uniform": 11, "ties": 12, "rows": 13, "ridge": 14}[case])
    fb = np.concatenate([[0], np.cumsum(KS)])
    total = int(fb[-1])
    au, av = rng.uniform(-np.pi, np.pi, (2, total, ops.PV_BINS))
    u32 = np.stack([np.cos(au), np.sin(au)], axis=-1).astype(np.float32)
    v32 = np.stack([np.cos(av), np.sin(av)], axis=-1).astype(np.float32)
    empty = (rng.uniform(size=total) < (0.0 if case == "ridge" else 0.04)).astype(np.uint8)
    empty[fb[5] + T - 1] = 1            # a reset on the first frame of a tile
    empty[fb[5] + 2 * T - 2] = 1        # ... and on the last
    mag = rng.uniform(0.0, 1.0, (total, ops.PV_BINS)).astype(np.float32)
    if case == "ties":
        mag = rng.integers(0, 4, (total, ops.PV_BINS)).astype(np.float32)
    elif case == "rows":
        ramp = np.arange(ops.PV_BINS, dtype=np.float32)
        for f in range(len(KS)):
            for j, row in enumerate([np.zeros_like(ramp), ramp, ramp[::-1].copy(),
                                     np.where(ramp == 0, 2.0, mag[0]).astype(np.float32),
                                     np.where(ramp == 1024, 2.0, mag[0]).astype(np.float32)]):
                k = 3 * j + 1 + (60 if KS[f] > 80 else 0)      # in the long file: around the first tile boundary
                if k < KS[f]:
                    mag[fb[f] + k] = row
    elif case == "ridge":
        mag *= 0.05                      # a ridge that moves one bin per frame, across the tile boundaries
        for f in (4, 5):
            for k in range(KS[f]):
                for b0 in (100, 500, 800):
                    mag[fb[f] + k, b0 + k] = 1.0
                    mag[fb[f] + k, b0 + k + 1] = 0.8
    return fb, mag, u32, v32, empty


@pytest.mark.parametrize("case", ["uniform", "ties", "rows", "ridge"])
def test_lock_alone(eng, case):
    fb, mag, u32, v32, empty = _lock_inputs(case)
    d = [torch.from_numpy(a).to(eng.dev) for a in (mag, u32, v32, empty)]
    phi_d, own_d = ops.pv_lock_device(eng, d[0], d[1], d[2], d[3], fb)
    phi, own = _c(phi_d), _own(own_d)
    assert np.array_equal(own, L.owners(mag))
    if case == "rows":
        k = int(fb[2]) + 1
        assert not own[k].any() and np.all(own[k + 3] == 1024) and not own[k + 6].any()
        assert own[k + 9][0] == 0 and own[k + 12][1024] == 1024
    if case == "ridge":
        k = int(fb[5]) + 130
        assert own[k][500 + 130] == 630 and own[k - 1][630] == 629       # the chain moves with the ridge
    uc = u32[..., 0].astype(np.float64) + 1j * u32[..., 1].astype(np.float64)
    vc = v32[..., 0].astype(np.float64) + 1j * v32[..., 1].astype(np.float64)
    phi2_d, own2_d = ops.pv_lock_device(eng, d[0], d[1], d[2], d[3], fb)
    assert np.array_equal(_bits(phi_d), _bits(phi2_d)) and np.array_equal(own, _own(own2_d))
    worst = 0.0
    for f, K in enumerate(KS):
        a, b = int(fb[f]), int(fb[f + 1])
        ref = L.lock_scan(mag[a:b], uc[a:b], vc[a:b], empty[a:b].astype(bool), own=own[a:b])
        worst = max(worst, float(np.max(np.abs(phi[a:b] - ref))))
        r = R.resets(empty[a:b])
        assert np.array_equal(_bits(phi_d[a:b])[r], v32[a:b].view(np.uint32)[r])    # Phi == V on a reset frame
        # a file alone: the same bits (the tiling follows the file's own frame index)
        one, own1 = ops.pv_lock_device(eng, d[0][a:b], d[1][a:b], d[2][a:b], d[3][a:b], [0, K])
        assert np.array_equal(_bits(one), _bits(phi_d[a:b])) and np.array_equal(_own(own1), own[a:b]), K
    print(f"pv_lock {case}: max |Phi - ref| {worst:.3e}")
    assert worst <= T_LOCK


def test_lock_argument_errors(eng):
    from nightcore_analyzer import _native
    fb, mag, u32, v32, empty = _lock_inputs("uniform")
    a, b = int(fb[4]), int(fb[5])
    d = [torch.from_numpy(x[a:b].copy()).to(eng.dev) for x in (mag, u32, v32, empty)]
    K = b - a
    phi = torch.empty_like(d[2])
    fbd = torch.tensor([0, K], dtype=torch.int64, device=eng.dev)
    need = int(_native.load().nc_pv_lock_ws_bytes(K, 1))
    ws = torch.empty(need, dtype=torch.uint8, device=eng.dev)
    assert need > K * ops.PV_BINS * 10
    with pytest.raises(_native.NativeError, match="workspace"):
        eng.call("nc_pv_lock", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), fbd.data_ptr(), 1, K,
                 K, phi.data_ptr(), 0, ws.data_ptr(), need - 1, eng.stream())
    with pytest.raises(_native.NativeError, match="max_frames"):
        eng.call("nc_pv_lock", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), fbd.data_ptr(), 1, K,
                 K + 1, phi.data_ptr(), 0, ws.data_ptr(), need, eng.stream())
    with pytest.raises(ValueError):
        ops.pv_lock_device(eng, d[0], d[1], d[2], d[3], [0, K + 1])
    # a null owner: the stage keeps it in its workspace, and Phi is the same
    eng.call("nc_pv_lock", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), fbd.data_ptr(), 1, K, K,
             phi.data_ptr(), 0, ws.data_ptr(), need, eng.stream())
    ref, _ = ops.pv_lock_device(eng, d[0], d[1], d[2], d[3], [0, K])
    assert np.array_equal(_bits(phi), _bits(ref))


# ------------------------------------------------------------------ 3. the locked stretch, mono
@pytest.mark.parametrize("P", RATIOS)
def test_locked_stretch(eng, P):
    xs = [_noise(n, 13 * n + P % 1000) for n in LENGTHS] + [_gap_case()]
    ss, peaks, plan = _stretch(eng, xs, P)
    owners = _device_owners(eng, xs, P)
    worst = 0.0
    for x, s, pk, own in zip(xs, ss, peaks, owners):
        (ref,) = L.stretch_locked([x], P, own=own)
        assert s.dtype == np.float32 and len(s) == len(ref) == R.plan(len(x), P)[0]
        worst = max(worst, float(np.max(np.abs(s - ref)) / np.max(np.abs(x))))
        assert float(pk) == float(np.max(np.abs(s)))
    print(f"locked stretch P={P}: max |s - ref| / max|x| {worst:.3e}")
    assert worst <= T_STRETCH


def test_locked_stretch_edges(eng):
    """An empty file beside others, silence, batch against single."""
    P = 1_059_463
    xs = [_noise(700, 1), np.zeros(0, np.float32), np.zeros(3000, np.float32), _noise(64, 2), _noise(5000, 3)]
    ss, peaks, plan = _stretch(eng, xs, P)
    ss2, peaks2, _ = _stretch(eng, xs, P)
    assert plan.k.tolist() == [R.plan(len(x), P)[1] for x in xs] and plan.k[1] == 0
    assert len(ss[1]) == 0 and float(peaks[1]) == 0.0
    assert len(ss[2]) == R.plan(3000, P)[0] and not np.any(ss[2]) and float(peaks[2]) == 0.0
    for i in (0, 3, 4):
        (one,), pk, _ = _stretch(eng, [xs[i]], P)
        assert np.array_equal(one.view(np.uint32), ss[i].view(np.uint32)), i
        assert np.array_equal(ss2[i].view(np.uint32), ss[i].view(np.uint32)), i
        assert float(pk[0]) == float(peaks[i]) == float(peaks2[i])
    # the default is the plain stretch, bit for bit
    plain, _, _ = _stretch(eng, xs, P, lock=None)
    old = ops.pv_stretch_device(eng, xs, P)[0]
    assert all(np.array_equal(p, old.buf.cpu().numpy()[o:o + n]) for p, o, n in zip(plain, old.off, old.length))
    assert not np.array_equal(plain[4], ss[4])


# ------------------------------------------------------------------ 4. the linked stretch
def _mid32(group):
    m = np.asarray(group[0], np.float32).copy()
    for x in group[1:]:
        m = (m + np.asarray(x, np.float32)).astype(np.float32)
    return m


@pytest.mark.parametrize("P", [890_899, 1_122_462])
def test_linked_stretch(eng, P):
    groups = [[_noise(n, 100 * n + 7 * c + 1) for c in range(C)] for n in (513, 5000) for C in (2, 3)]
    x = _noise(5000, 8)
    groups += [[x, x.copy()], [x, -x], [_noise(700, 9)]]
    counts = [len(g) for g in groups]
    flat = [ch for g in groups for ch in g]
    ss, peaks, plan = _stretch(eng, flat, P, channels=counts)
    assert plan.n_files == len(flat)
    owners = _device_owners(eng, [_mid32(g) for g in groups], P)
    worst, i = 0.0, 0
    for g, own in zip(groups, owners):
        refs = L.stretch_locked(g, P, own=own)
        top = max(float(np.max(np.abs(ch))) for ch in g)
        for ref in refs:
            assert len(ss[i]) == len(ref) and np.all(np.isfinite(ss[i]))
            worst = max(worst, float(np.max(np.abs(ss[i] - ref)) / top))
            assert float(peaks[i]) == float(np.max(np.abs(ss[i])))
            i += 1
    print(f"linked stretch P={P}: max |s - ref| / max|x| {worst:.3e}")
    assert worst <= T_STRETCH
    first = np.concatenate([[0], np.cumsum(counts)])
    a = int(first[4])
    assert np.array_equal(ss[a].view(np.uint32), ss[a + 1].view(np.uint32))     # identical channels
    assert not np.any(_mid32(groups[5])) and np.max(np.abs(ss[a + 2])) > 0.1    # x and -x: a zero sum, a defined result
    assert np.array_equal(ss[a + 2], -ss[a + 3])
    # a group of one channel inside a linked batch is the mono locked stretch
    (mono,), _, _ = _stretch(eng, groups[6], P)
    assert np.array_equal(ss[a + 4].view(np.uint32), mono.view(np.uint32))
    # a group alone: the same bits as in the batch
    alone, _, _ = _stretch(eng, groups[3], P, channels=3)
    b = int(first[3])
    assert all(np.array_equal(alone[c].view(np.uint32), ss[b + c].view(np.uint32)) for c in range(3))


def test_linked_empty_and_silent_groups(eng):
    """A group of empty channels and a silent group beside a sounding one."""
    P = 1_059_463
    z0, z = np.zeros(0, np.float32), np.zeros(3000, np.float32)
    pair = [_noise(700, 31), _noise(700, 32)]
    ss, peaks, plan = _stretch(eng, [z0, z0, z, z] + pair, P, channels=2)
    assert plan.k[:2].tolist() == [0, 0] and len(ss[0]) == len(ss[1]) == 0
    assert len(ss[2]) == R.plan(3000, P)[0] and not np.any(ss[2]) and not np.any(ss[3])
    assert peaks[:4].tolist() == [0.0] * 4
    alone, pk, _ = _stretch(eng, pair, P, channels=2)
    for c in range(2):
        assert np.array_equal(alone[c].view(np.uint32), ss[4 + c].view(np.uint32))
        assert float(pk[c]) == float(peaks[4 + c]) > 0.0
    assert [len(s) for s in _stretch(eng, [], P, channels=2)[0]] == []


def test_linked_argument_errors(eng):
    from nightcore_analyzer import _native
    xs = [_noise(600, 1), _noise(601, 2)]
    with pytest.raises(ValueError, match="equally long"):
        ops.pv_stretch_device(eng, xs, R.Q, lock="identity", channels=2)
    with pytest.raises(ValueError):
        ops.pv_stretch_device(eng, xs + xs[:1], R.Q, lock="identity", channels=2)
    with pytest.raises(ValueError, match="lock"):
        ops.pv_stretch_device(eng, xs, R.Q, lock="loose")
    sig = eng.upload_signals(xs)
    lens, first = np.array([600, 601], np.int64), np.array([0, 2], np.int32)
    z = torch.zeros(1024, dtype=torch.int64, device=eng.dev)
    mid = torch.zeros(1024, dtype=torch.float32, device=eng.dev)
    with pytest.raises(_native.NativeError, match="equally long"):
        eng.call("nc_pv_mid_sum", sig.buf.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), lens.ctypes.data,
                 first.ctypes.data, 1, mid.data_ptr(), z.data_ptr(), eng.stream())


# ------------------------------------------------------------------ 5. what the mode buys, on the device output
def test_locked_keeps_the_level_of_a_voiced_tone(eng):
    x = vibrato_tone().astype(np.float32)
    P = 1_122_462
    (locked,), _, _ = _stretch(eng, [x], P)
    (plain,), _, _ = _stretch(eng, [x], P, lock=None)
    lk, pl = locked[4096:-4096], plain[4096:-4096]
    print(f"vibrato tone: locked rms ratio {rms(lk) / rms(x):.3f} spread {running_rms_spread(lk):.3f}, "
          f"plain rms ratio {rms(pl) / rms(x):.3f}")
    assert rms(lk) / rms(x) >= 0.95
    assert running_rms_spread(lk) >= 0.9
    assert rms(pl) / rms(x) <= 0.85


@pytest.mark.parametrize("P", [890_899, 1_122_462])
def test_linked_keeps_a_centred_source_centred(eng, P):
    left, right = (v.astype(np.float32) for v in stereo_pair())
    cut = slice(4096, -4096)
    (a, b), _, _ = _stretch(eng, [left, right], P, channels=2)
    (pa, pb), _, _ = _stretch(eng, [left, right], P, lock=None)
    linked, plain = unexplained(a[cut], b[cut]), unexplained(pa[cut], pb[cut])
    print(f"stereo pair P={P}: linked {linked:.3f} plain {plain:.3f}")
    assert linked <= 0.16
    assert plain >= 0.40


# ------------------------------------------------------------------ 6. the layers
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
        y = render.pitch_shift(x, st, phase_lock=True)
        P = R.semitones_p(st)
        hz = _peak_hz(y)
        print(f"locked pitch_shift {st:+.1f} st: peak {hz:.4f} Hz, wanted {440.0 * P / R.Q:.4f}")
        assert y.dtype == np.float32 and len(y) == len(x)
        assert abs(hz / (440.0 * P / R.Q) - 1.0) <= 2e-4
        assert not np.array_equal(y, render.pitch_shift(x, st))


def test_pitch_file_linked_flac(eng, tmp_path):
    rng = np.random.default_rng(21)
    t = np.arange(3001) / 44100.0
    ch = np.stack([0.6 * np.sin(2 * np.pi * 997.0 * t) + 0.2 * rng.uniform(-1, 1, len(t)),
                   0.3 * np.sin(2 * np.pi * 4001.0 * t) + 0.5 * rng.uniform(-1, 1, len(t))])
    q = np.rint(ch * 32767).astype(np.int16)
    src, dst = tmp_path / "Song.wav", tmp_path / "Song PS1.flac"
    nio.write_wav(src, q, 44100, "pcm16")
    info = render.pitch_file(src, dst, 1.0, phase_lock=True)
    P = R.semitones_p(1.0)
    assert info.phase_lock is True
    assert (info.semitones, info.factor, info.n_out, info.channels, info.sample_rate, info.sample_format) == \
        (1.0, P / R.Q, 3001, 2, 44100, "pcm16")
    back, sr, fmt = nio.read_audio_channels(dst)
    assert (sr, fmt, back.shape) == (44100, "pcm16", (2, 3001))
    xs = [q[c].astype(np.float32) / 32768.0 for c in range(2)]
    (own,) = _device_owners(eng, [_mid32(xs)], P)
    refs = L.pitch_shift_locked(xs, P=P, own=own)
    step, over = 1.0 / 32768, 0
    for c in range(2):
        v = np.rint(refs[c] * 32768.0)
        over += int(np.count_nonzero((v > 32767) | (v < -32768)))
        err = float(np.max(np.abs(back[c] - np.clip(refs[c], -1.0, 32767.0 / 32768.0))))
        print(f"linked pitch_file channel {c}: {err:.3e} (max |ref| {np.max(np.abs(refs[c])):.4f})")
        assert err <= step + T_STRETCH * float(np.max(np.abs(xs[c]))), c
    assert info.clipped_samples == over and info.is_clipping == (over > 0)
    plain = render.pitch_file(src, tmp_path / "plain.flac", 1.0)
    assert plain.phase_lock is False
    assert not np.array_equal(nio.read_audio_channels(tmp_path / "plain.flac")[0], back)


@pytest.fixture(scope="module")
def shifted20(eng):
    src = synth.make_source(20.0, 1000)
    return src, render.pitch_shift(src, 2.0, phase_lock=True)


def test_refine_pitch_locked(eng, shifted20):
    src, shifted = shifted20
    lines = []
    ref = render.refine_pitch(shifted, src, start=2.0, log=lines.append, phase_lock=True)
    print(f"locked refine_pitch: shifts {ref.shifts} residuals {ref.residuals} method {ref.method}")
    assert ref.shifts == [2.0] and ref.residuals == [0.0] and ref.converged and ref.corrections == 0
    assert np.array_equal(ref.render.numpy(), shifted)


def test_locked_pitch_shift_chroma(eng, shifted20):
    src, shifted = shifted20
    assert len(shifted) == len(src)
    assert pitch._chroma_shift_for_chunk(src, shifted, SR) == 2 / 3.0


def _run_cli(argv):
    out, err = stdio.StringIO(), stdio.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = cli.main(argv)
    return rc, out.getvalue(), err.getvalue()


def test_cli_phase_lock(eng, tmp_path):
    nc, src = synth.make_pair(40.0, 1022)
    ncp, srp, ps = tmp_path / "nc.wav", tmp_path / "src.wav", tmp_path / "src PS1.wav"
    nio.write_wav(ncp, nc, 22050, "pcm16")
    nio.write_wav(srp, src, 22050, "pcm16")
    rc, out, err = _run_cli(["-n", str(ncp), "-s", str(srp), "--phase-lock"])
    assert rc == 2 and "--phase-lock needs --pitch-correct" in err and out == ""
    assert not ps.exists()
    rc, out, _ = _run_cli(["-n", str(ncp), "-s", str(srp), "--pitch-correct", str(ps), "--semitones", "-1.5",
                           "--phase-lock"])
    assert rc == 0 and "Pitch-corrected file written to:" in out and "pitch -1.500000 st, phase-locked" in out
    back, sr, fmt = nio.read_wav_channels(ps)
    assert (sr, fmt, back.shape) == (22050, "pcm16", (1, len(src)))
    want = render.pitch_shift(nio.read_wav_channels(srp)[0][0], -1.5, phase_lock=True)
    assert np.max(np.abs(back[0] - np.clip(want, -1.0, 32767.0 / 32768.0))) <= 1.0 / 32768
