"""The true-peak limiter on the MI355X (csrc/limiter.hip behind nc_true_peak /
nc_true_peak_limit) against its definition (tests/limiter_ref.py, numpy float64), and the layers
on top of it: ops, loudness.apply_true_peak_limiter / detect_true_peak, render.speed_file's
limit_db and the CLI's --limit.

Tolerances.  The device computes p (3 x 24 taps) and r = L / p in float32, the box mean exactly
and the release in float64, and stores the local release and y in float32; the reference is
float64 throughout.  Largest deviations measured on an MI355X over the cases of limiter_ref.cases
at both rates (printed by test_against_reference):
    r 1.97e-7,  gain y / x 1.94e-7,  y 1.37e-7 (absolute),  true peak 1.54e-7 (relative).
The bounds are 4x those, rounded up, the gain's far inside the 1e-4 (0.001 dB) cap."""
import contextlib
import io as stdio
import math
import re

import numpy as np
import pytest
import torch

import limiter_ref as R
from nightcore_analyzer import _native, cli, engine as E, io as nio, loudness, ops, render, synth
from test_limiter_cpu import GAIN_CAP, limited_is_decidable

pytestmark = pytest.mark.gpu

R_BOUND = 8e-7            # 4 x 1.97e-7
GAIN_BOUND = 8e-7         # 4 x 1.94e-7
Y_BOUND = 5.5e-7          # 4 x 1.37e-7
TP_REL = 6.2e-7           # 4 x 1.54e-7
assert GAIN_BOUND <= GAIN_CAP

ALL = [(sr, c.name) for sr in R.RATES for c in R.cases(sr)]
_runs = {}


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


def _ws_layout(frames):
    frames = np.ascontiguousarray(frames, np.int64)
    off = np.zeros(len(frames), np.int64)
    total = int(_native.load().nc_limiter_ws_bytes(frames.ctypes.data, len(frames), off.ctypes.data))
    return total, off


def _limit(eng, files, limit_db, Wa, Wr, in_place=False):
    """One call over ``files`` ([channels, N] arrays): per file (y, true peak, peak out, limited, r)."""
    chans = [f.shape[0] for f in files]
    sig = eng.upload_signals([np.ascontiguousarray(ch) for f in files for ch in f])
    out, tp, pk, lim = ops.true_peak_limit_device(eng, sig, chans, limit_db, Wa, Wr, in_place=in_place)
    torch.cuda.synchronize()
    hy, tp, pk, lim = out.buf.cpu().numpy(), tp.cpu().numpy(), pk.cpu().numpy(), lim.cpu().numpy()
    _, ws_off = _ws_layout([f.shape[1] for f in files])
    ws = eng.workspace("limiter", 0).cpu().numpy()
    res, s = [], 0
    for i, f in enumerate(files):
        C, N = f.shape
        y = np.stack([hy[out.off[s + c]:out.off[s + c] + N] for c in range(C)])
        r = ws[ws_off[i]:ws_off[i] + 4 * N].view(np.float32).copy()
        res.append((y, float(tp[i]), float(pk[i]), int(lim[i]), r))
        s += C
    return res


def _run(eng, sr, name):
    if (sr, name) not in _runs:
        c = next(c for c in R.cases(sr) if c.name == name)
        _runs[sr, name] = _limit(eng, [c.x], c.limit_db, *c.wa_wr)[0]
    return _runs[sr, name]


def _case(sr, name):
    return next(c for c in R.cases(sr) if c.name == name), R.reference(sr, name)


def deviations(c, ref, got):
    """(r, gain, y, true peak relative) deviations of a device result from the reference."""
    y, tp, _, _, r = got
    if c.x.shape[1] == 0:
        return 0.0, 0.0, 0.0, 0.0
    ok = np.abs(c.x) > 1e-6
    gain = np.abs(y.astype(np.float64)[ok] / c.x.astype(np.float64)[ok] - np.broadcast_to(ref.g, c.x.shape)[ok])
    return (float(np.max(np.abs(r - ref.r))), float(gain.max()) if gain.size else 0.0,
            float(np.max(np.abs(y - ref.y))), abs(tp / ref.true_peak - 1.0))


@pytest.mark.parametrize("sr,name", ALL)
def test_against_reference(eng, sr, name):
    c, ref = _case(sr, name)
    got = _run(eng, sr, name)
    dr, dg, dy, dt = deviations(c, ref, got)
    print(f"limiter {sr} {name}: r {dr:.3e} gain {dg:.3e} y {dy:.3e} true peak {dt:.3e} limited {got[3]} / {ref.limited}")
    assert got[0].shape == c.x.shape and got[0].dtype == np.float32
    assert dr <= R_BOUND and dg <= GAIN_BOUND and dy <= Y_BOUND and dt <= TP_REL


@pytest.mark.parametrize("sr,name", ALL)
def test_exact_properties(eng, sr, name):
    """The ceiling holds in float32, the reported peak is the output's, and everything more than
    an attack ahead of the first over-peak comes back to the bit."""
    c, ref = _case(sr, name)
    y, tp, pk, lim, _ = _run(eng, sr, name)
    N = c.x.shape[1]
    if N == 0:
        assert (tp, pk, lim) == (0.0, 0.0, 0)
        return
    assert float(np.abs(y).max()) <= float(np.float32(ref.L))
    assert pk == float(np.abs(y).max())
    over = np.nonzero(ref.r < 1.0)[0]
    keep = N if len(over) == 0 else max(0, int(over[0]) - ref.Wa + 1)    # n <= j0 - Wa
    assert np.array_equal(y[:, :keep].view(np.uint32), c.x[:, :keep].view(np.uint32))
    if len(over) == 0:
        assert lim == 0 and tp <= ref.L
    else:
        assert keep == N or not np.array_equal(y[:, keep:], c.x[:, keep:])


@pytest.mark.parametrize("sr,name", ALL)
def test_limited_count(eng, sr, name):
    """limited = #{n : float32(1 - d[n]) < 1}: exact where no reference d lies within the gain
    bound of the threshold 2^-25, bracketed by the reference's counts otherwise."""
    _, ref = _case(sr, name)
    lim = _run(eng, sr, name)[3]
    if limited_is_decidable(ref, GAIN_BOUND):
        assert lim == ref.limited
    else:
        assert np.count_nonzero(ref.d > R.THRESHOLD + GAIN_BOUND) <= lim <= np.count_nonzero(ref.d > 0.0)
    if limited_is_decidable(ref, GAIN_CAP):
        assert lim == ref.limited


@pytest.mark.parametrize("sr", R.RATES)
def test_stereo_gain_is_shared(eng, sr):
    c, ref = _case(sr, "stereo")
    y = _run(eng, sr, "stereo")[0].astype(np.float64)
    ok = (np.abs(c.x[0]) > 1e-3) & (np.abs(c.x[1]) > 1e-3)
    q0, q1 = y[0][ok] / c.x[0][ok], y[1][ok] / c.x[1][ok]
    assert np.max(np.abs(q0 - q1)) <= 4e-7 and np.min(q0) < 0.5     # two float32 roundings of x g


@pytest.mark.parametrize("sr", R.RATES)
def test_fresh_workspace_same_bits(eng, sr):
    """Nothing is read from the workspace before it is written: two runs on workspaces of
    different contents give the same bits (and no float atomics but the bit-pattern maximum)."""
    names = ("tile_edge", "long_tail", "stereo")
    files = [_case(sr, n)[0].x for n in names]
    Wa, Wr = R.windows(sr)
    total, _ = _ws_layout([f.shape[1] for f in files])
    outs = []
    for fill in (0xFF, 0x3C):
        eng.workspace("limiter", total).fill_(fill)
        outs.append(_limit(eng, files, -0.1, Wa, Wr))
    for a, b in zip(*outs):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:4] == b[1:4]
        assert np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))


@pytest.mark.parametrize("sr", R.RATES)
def test_batch_of_unlike_files(eng, sr):
    """Three files of different lengths and channel counts (and an empty one) in one call give
    each file the bits of its own call; in place gives the same bits as to a second buffer."""
    Wa, Wr = R.windows(sr)
    names = ("stereo", f"short_{2 * Wa}", "empty", "tile_edge")
    trio = np.stack([_case(sr, "near_ends")[0].x[0][:3 * R.TILE + 1], _case(sr, "first_last")[0].x[0][:3 * R.TILE + 1],
                     R._bed(3 * R.TILE + 1, 77).astype(np.float32)])
    files = [_case(sr, n)[0].x for n in names] + [trio]
    got = _limit(eng, files, -0.1, Wa, Wr)
    again = _limit(eng, files, -0.1, Wa, Wr, in_place=True)
    for n, g, h in zip(names, got, again):
        one = _run(eng, sr, n)
        assert np.array_equal(g[0].view(np.uint32), one[0].view(np.uint32)) and g[1:4] == one[1:4], n
        assert np.array_equal(g[0].view(np.uint32), h[0].view(np.uint32)) and g[1:4] == h[1:4], n
    ref = R.limiter_ref(trio, -0.1, Wa, Wr)
    y, tp, pk, lim, r = got[-1]
    assert np.max(np.abs(y - ref.y)) <= Y_BOUND and np.max(np.abs(r - ref.r)) <= R_BOUND
    assert abs(tp / ref.true_peak - 1.0) <= TP_REL and pk == float(np.abs(y).max())
    # the meter alone: the same true peaks from one launch
    sig = eng.upload_signals([np.ascontiguousarray(ch) for f in files for ch in f])
    tps = ops.true_peak_device(eng, sig, [f.shape[0] for f in files]).cpu().numpy()
    assert tps.tolist() == [g[1] for g in got]


def test_other_ceilings_and_windows(eng):
    """Attack 1 (no look-ahead), 2 and the largest 2048; release 1; a 0 dBFS ceiling."""
    x = _case(22050, "tile_edge")[0].x
    for limit_db, Wa, Wr in ((-0.1, 1, 1), (-3.0, 2, 37), (0.0, 2048, 4000), (-6.0, 1023, 100000)):
        ref = R.limiter_ref(x, limit_db, Wa, Wr)
        (y, tp, pk, lim, r), = _limit(eng, [x], limit_db, Wa, Wr)
        dy = float(np.max(np.abs(y - ref.y)))
        print(f"limiter Wa {Wa} Wr {Wr} {limit_db} dB: y {dy:.3e} limited {lim} / {ref.limited}")
        assert dy <= Y_BOUND and np.max(np.abs(r - ref.r)) <= R_BOUND
        assert float(np.abs(y).max()) <= float(np.float32(ref.L))


def test_offsets_off_the_16_byte_grid(eng):
    """The C entry point with signals at odd sample offsets, to a second buffer at other odd
    offsets (upload_signals only makes 64-sample aligned ones): the kernels' scalar load and
    store paths give the bits of the aligned call."""
    c, _ = _case(22050, "stereo")
    N = c.x.shape[1]
    want = _run(eng, 22050, "stereo")
    lens, first = np.array([N, N], np.int64), np.array([0, 2], np.int32)
    x_off, y_off = np.array([1, N + 3], np.int64), np.array([N + 7, 2], np.int64)
    buf = np.zeros(2 * N + 16, np.float32)
    for ch, o in zip(c.x, x_off):
        buf[o:o + N] = ch
    total, ws_off = _ws_layout([N])
    d = {k: torch.tensor(v, device=eng.dev) for k, v in
         dict(off=x_off, len=lens, first=first, y_off=y_off, ws_off=ws_off).items()}
    x, y = torch.tensor(buf, device=eng.dev), torch.zeros(2 * N + 16, dtype=torch.float32, device=eng.dev)
    res = torch.zeros(3, dtype=torch.float32, device=eng.dev)
    ws = eng.workspace("limiter", total)
    eng.call("nc_true_peak_limit", x.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), d["first"].data_ptr(),
             lens.ctypes.data, first.ctypes.data, 1, c.limit_db, *c.wa_wr, y.data_ptr(), d["y_off"].data_ptr(),
             res[0:1].data_ptr(), res[1:2].data_ptr(), res[2:3].data_ptr(), ws.data_ptr(), d["ws_off"].data_ptr(),
             ws.numel(), eng.stream())
    hy, hr = y.cpu().numpy(), res.cpu().numpy()
    got = np.stack([hy[o:o + N] for o in y_off])
    assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
    assert (float(hr[0]), float(hr[1]), int(hr[2:3].view(np.int32)[0])) == want[1:4]
    assert np.count_nonzero(hy) == np.count_nonzero(got)          # nothing written beside the signals


def test_argument_checks(eng):
    x = [np.zeros(100, np.float32), np.zeros(100, np.float32), np.zeros(90, np.float32)]
    for kw, what in ((dict(limit_db=0.5), "ceiling"), (dict(attack=2049), "attack"), (dict(attack=0), "attack"),
                     (dict(channels=[2, 0, 1]), "channel"), (dict(channels=[1, 2]), "equally long")):
        args = dict(channels=[1, 1, 1], limit_db=-0.1, attack=110, release=1102)
        args.update(kw)
        with pytest.raises(_native.NativeError, match=r"\(-2\).*" + what):
            ops.true_peak_limit_device(eng, x, **args)
    with pytest.raises(_native.NativeError, match=r"\(-2\).*equally long"):
        ops.true_peak_device(eng, x, [1, 2])


# ------------------------------------------------------------------ the public surface
def _loud_source(n=30000, seed=5):
    """A 'mastered' 16-bit stereo source: flat-topped at full scale, so a band-limited
    resample of it overshoots."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    a = 1.6 * np.sin(2 * np.pi * 441.0 * t) + 0.5 * np.sin(2 * np.pi * 2917.0 * t + 1.0) + 0.2 * rng.uniform(-1, 1, n)
    b = 1.4 * np.sin(2 * np.pi * 331.0 * t + 0.5) + 0.6 * np.sin(2 * np.pi * 5003.0 * t) + 0.2 * rng.uniform(-1, 1, n)
    return np.rint(np.clip(np.stack([a, b]), -1.0, 1.0) * 32767).astype(np.int16)


@pytest.fixture(scope="module")
def clipping_render(eng, tmp_path_factory):
    d = tmp_path_factory.mktemp("limiter")
    src, dst = d / "Song.wav", d / "Song [Nightcore].wav"
    nio.write_wav(src, _loud_source(), 44100, "pcm16")
    info = render.speed_file(src, dst, 1.2345)
    return d, src, dst, info


def test_speed_file_without_a_ceiling_is_unchanged(eng, clipping_render):
    """limit_db=None: the bytes the renderer wrote before the limiter existed (the render, the
    16-bit epilogue and the WAV writer, composed here from their own entry points)."""
    d, src, dst, info = clipping_render
    data, sr, fmt = nio.read_wav_channels(src)
    out, peak, P = ops.speed_render_device(eng, list(data), render.quantize_factor(1.2345))
    q, _, clipped = ops.f32_to_pcm16_device(eng, out, interleave=True)
    n_out = int(out.length[0])
    nio.write_wav(d / "parent.wav", q[:2 * n_out].cpu().numpy().reshape(n_out, 2).T, sr, "pcm16")
    assert dst.read_bytes() == (d / "parent.wav").read_bytes()
    assert (info.peak, info.clipped_samples) == (float(peak.max().item()), int(clipped.sum().item()))
    assert info.is_clipping and info.clipped_samples > 0
    assert (info.true_peak, info.limited_samples, info.limit_db) == (None, 0, None)


def test_apply_true_peak_limiter_on_a_clipping_render(eng, clipping_render, capsys):
    d, _, dst, _ = clipping_render
    db, clip = loudness.detect_peak(dst)
    assert clip and db >= 0.0 or db > 20 * math.log10(32766.5 / 32768)
    adj = loudness.make_adj_path(dst, 1)
    info = loudness.apply_true_peak_limiter(dst, adj)
    assert capsys.readouterr().out == f"  Created: {adj}\n"
    data, sr, fmt = nio.read_wav_channels(dst)
    back, sr2, fmt2 = nio.read_wav_channels(adj)
    assert (sr2, fmt2, back.shape) == (sr, "pcm16", data.shape)
    db2, clip2 = loudness.detect_peak(adj)
    assert db2 < 0.0 and not clip2 and db2 <= -0.1 + 20 * math.log10(1 + 0.5 / 32768 / R.L01)
    Wa, Wr = R.windows(sr)
    ref = R.limiter_ref(data, -0.1, Wa, Wr)
    want = np.rint(ref.y * 32768.0)
    assert np.max(np.abs(back.astype(np.float64) * 32768.0 - want)) <= 1.0
    assert (info.attack_samples, info.release_samples, info.limit_db) == (Wa, Wr, -0.1)
    assert abs(info.true_peak / ref.true_peak - 1.0) <= TP_REL and info.true_peak > 1.0
    assert info.true_peak_dbfs == pytest.approx(20 * math.log10(info.true_peak))
    assert info.peak_out <= float(np.float32(ref.L)) and info.limited_samples > 0
    tdb, over = loudness.detect_true_peak(dst)
    assert over and tdb == pytest.approx(info.true_peak_dbfs, abs=1e-5)
    assert loudness.detect_true_peak(adj)[0] < 20 * math.log10(1.0 + 0.02)
    with pytest.raises(NotImplementedError):
        loudness.apply_true_peak_limiter(d / "x.flac", adj)
    with pytest.raises(ValueError):
        loudness.apply_true_peak_limiter(dst, adj, 0.5)
    # a float source stays float32, sample for sample the device's output
    fsrc, fdst = d / "f.wav", d / "f lim.wav"
    x = (data * np.float32(1.3)).astype(np.float32)
    nio.write_wav(fsrc, x, 48000, "float32")
    loudness.apply_true_peak_limiter(fsrc, fdst, -1.0, attack_ms=2.0, release_ms=20.0)
    fback, fsr, ffmt = nio.read_wav_channels(fdst)
    (y, *_), = _limit(eng, [x], -1.0, *R.windows(48000, 2.0, 20.0))
    assert (fsr, ffmt) == (48000, "float32") and np.array_equal(fback, y)


def test_speed_file_with_a_ceiling(eng, clipping_render):
    d, src, dst, plain = clipping_render
    out = d / "limited.wav"
    info = render.speed_file(src, out, 1.2345, limit_db=-0.1)
    assert info.clipped_samples == 0 and not info.is_clipping and info.limit_db == -0.1
    assert info.true_peak >= plain.peak > 1.0 and info.limited_samples > 0
    assert info.peak <= float(np.float32(R.L01))
    assert (info.n_out, info.channels, info.sample_format) == (plain.n_out, plain.channels, "pcm16")
    db, clip = loudness.detect_peak(out)
    assert not clip and db < 0.0
    # the limiter ran on the float render, not on the clamped 16-bit file
    data, sr, _ = nio.read_wav_channels(src)
    ys, _ = ops.speed_render(eng, list(data), render.quantize_factor(1.2345))
    ref = R.limiter_ref(np.stack(ys), -0.1, *R.windows(sr))
    back, _, _ = nio.read_wav_channels(out)
    assert np.max(np.abs(back.astype(np.float64) * 32768.0 - np.rint(ref.y * 32768.0))) <= 1.0


def _run_cli(argv):
    out, err = stdio.StringIO(), stdio.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = cli.main(argv)
    return rc, out.getvalue(), err.getvalue()


def test_cli_limit(eng, tmp_path):
    nc, src = synth.make_pair(40.0, 1022)
    loud = np.clip(src / np.max(np.abs(src)) * 1.5, -1.0, 1.0)
    ncp, srp = tmp_path / "nc.wav", tmp_path / "src.wav"
    nio.write_wav(ncp, nc, 22050, "pcm16")
    nio.write_wav(srp, loud, 22050, "pcm16")
    rc, out, err = _run_cli(["-n", str(ncp), "-s", str(srp), "--limit"])
    assert rc == 2 and "--limit needs --render-hqnc" in err and out == ""
    plain, lim = tmp_path / "plain.wav", tmp_path / "lim.wav"
    rc, out, _ = _run_cli(["-n", str(ncp), "-s", str(srp), "--render-hqnc", str(plain)])
    assert rc == 0 and "Limiter at" not in out
    assert int(re.search(r"(\d+) clipped samples", out).group(1)) > 0   # the plain render clips
    rc, out, _ = _run_cli(["-n", str(ncp), "-s", str(srp), "--render-hqnc", str(lim), "--limit"])
    assert rc == 0 and "Limiter at -0.10 dBFS: true peak +" in out and "0 clipped samples" in out
    db, clip = loudness.detect_peak(lim)
    assert not clip and db < 0.0
    assert nio.read_wav_channels(lim)[0].shape == nio.read_wav_channels(plain)[0].shape
