"""The speed renderer on the MI355X (nc_speed_render, nc_f32_to_pcm16) against its definition
(tests/speed_ref.py, numpy float64), and the layers on top of it: render.speed / speed_file,
the verify-and-correct loop, the peak check and the CLI's --render-hqnc.

Tolerance of the kernel: 1e-5 max(1, max|x|) — the filter's own -100 dB stop band, so a
device error below it is below the aliasing the definition already admits.  Largest error
seen on an MI355X over the cases below: 2.92e-6 ("Speed render")."""
import contextlib
import io as stdio
import json
import math

import numpy as np
import pytest
import torch

from nightcore_analyzer import cli, engine as E, io as nio, loudness, ops, pipeline, render, synth
from speed_ref import Q, Z, plan, speed_ref

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 257, 5000]
FACTORS = [0.25, 0.8, 1.0, 1.000001, 1.25, 1.234567, 4.0]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


@pytest.fixture(scope="module")
def pair60():
    return synth.make_pair(60.0, 1021)


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


@pytest.mark.parametrize("F", FACTORS)
@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_against_definition(eng, n, F):
    x = _noise(n, 1000 * n + int(F * 1000))
    (y,), peak = ops.speed_render(eng, [x], F)
    P, n_out, _ = plan(n, F)
    assert y.dtype == np.float32 and len(y) == n_out
    ref = speed_ref(x, F).astype(np.float32)
    err = float(np.max(np.abs(y - ref)))
    print(f"speed_render n={n} F={F}: max err {err:.3e}")
    assert err <= 1e-5 * max(1.0, float(np.max(np.abs(x)))), err
    assert peak.dtype == np.float32 and float(peak[0]) == float(np.max(np.abs(y)))


def test_batch_and_offsets(eng):
    xs = [_noise(5000, 1), _noise(1, 2), _noise(777, 3)]
    for F in (0.8, 1.234567):
        ys, peaks = ops.speed_render(eng, xs, F)
        ys2, peaks2 = ops.speed_render(eng, xs, F)
        for i, x in enumerate(xs):
            (one,), pk = ops.speed_render(eng, [x], F)
            assert np.array_equal(ys[i].view(np.uint32), one.view(np.uint32)), (F, i)
            assert np.array_equal(ys[i].view(np.uint32), ys2[i].view(np.uint32)), (F, i)
            assert float(peaks[i]) == float(pk[0]) == float(peaks2[i]) == float(np.max(np.abs(one)))


def test_device_resident_form(eng):
    """speed_render_device of signals already in HBM: the same bits, the result left in HBM
    with upload_signals' 64-sample aligned offsets."""
    xs = [_noise(300, 4), _noise(1000, 5)]
    sig = eng.upload_signals(xs)
    out, peak, P = ops.speed_render_device(eng, sig, 1.25)
    assert P == 1_250_000 and out.buf.is_cuda and out.n_files == 2
    assert out.length.tolist() == [240, 800] and all(int(o) % 64 == 0 for o in out.off)
    ys, peaks = ops.speed_render(eng, xs, 1.25)
    h = out.buf.cpu().numpy()
    for i in range(2):
        assert np.array_equal(h[out.off[i]:out.off[i] + out.length[i]], ys[i])
    assert np.array_equal(peak.cpu().numpy(), peaks)
    # and back into the engine's loaders without a host trip
    again = eng.upload_signals([xs[0], nio.DeviceAudio(out.buf[out.off[1]:out.off[1] + 800])])
    g = again.buf.cpu().numpy()
    assert again.length.tolist() == [300, 800]
    assert np.array_equal(g[again.off[0]:again.off[0] + 300], xs[0])
    assert np.array_equal(g[again.off[1]:again.off[1] + 800], ys[1])


def test_long_position_arithmetic(eng):
    """m P passes 2^31 and 2^40 in a 3 000 000-sample file: the last 4096 outputs against the
    definition evaluated on the matching input slice."""
    n, F, tail = 3_000_000, 1.234567, 4096
    x = _noise(n, 77)
    (y,), _ = ops.speed_render(eng, [x], F)
    P, n_out, c = plan(n, F)
    assert len(y) == n_out and (n_out - 1) * P > 1 << 40
    m0 = n_out - tail
    base = m0 * P // Q - math.ceil(Z / c) - 4
    ref = speed_ref(x[base:], F, m0=m0, m1=n_out, base=base, n=n).astype(np.float32)
    err = float(np.max(np.abs(y[m0:] - ref)))
    print(f"speed_render tail of n={n}: max err {err:.3e}")
    assert err <= 1e-5, err


def test_pcm16_epilogue(eng):
    a = np.array([1.0, -1.0, 1 - 2.0 ** -16, -(1 - 2.0 ** -16), 0.5 / 32768, 1.5 / 32768, 2.5 / 32768,
                  -0.5 / 32768, -1.5 / 32768, -2.5 / 32768, 1.5, -1.5, 32767.5 / 32768, -32768.5 / 32768,
                  -32769.5 / 32768, 0.0, 0.25], np.float32)
    b = np.concatenate([_noise(1000, 9) * np.float32(1.2), a])
    qs, clipped = ops.f32_to_pcm16(eng, [a, b, np.zeros(0, np.float32)])
    for x, q, k in zip((a, b), qs, clipped):
        v = np.rint(x * np.float32(32768.0))
        want = np.clip(v, -32768, 32767).astype(np.int16)
        assert q.dtype == np.int16 and np.array_equal(q, want)
        assert int(k) == int(np.count_nonzero((v > 32767) | (v < -32768)))
        assert (want.tolist(), int(k)) == (nio.quantize_pcm16(x)[0].tolist(), nio.quantize_pcm16(x)[1])
    assert qs[0][:4].tolist() == [32767, -32768, 32767, -32768] and int(clipped[0]) == 6
    assert len(qs[2]) == 0 and int(clipped[2]) == 0


def test_end_to_end(eng, pair60):
    nc, src = pair60
    y = render.speed(src, 1.25)
    assert y.dtype == np.float32 and len(y) == len(nc)
    res = pipeline.run(nc, y, compute_pitch=False, log=None)
    print(f"render vs nightcore: tempo_ratio {res.tempo_ratio!r} ibi_ratio {res.ibi_ratio!r}")
    assert abs(res.tempo_ratio - 1.0) < 0.005
    assert res.ibi_ratio is not None and abs(res.ibi_ratio - 1.0) < 0.005


def test_refinement(eng, pair60):
    nc, src = pair60
    lines = []
    ref = render.refine_speed(nc, src, start=1.2, log=lines.append)
    print(f"refine_speed: factors {ref.factors} residuals {ref.residuals}")
    assert ref.converged and ref.corrections <= 2
    assert ref.factors[0] == 1.2 and abs(ref.factor / 1.25 - 1.0) <= 0.005
    assert len(ref.results) == len(ref.factors) == len(ref.residuals)
    assert isinstance(ref.render, nio.DeviceAudio) and ref.render.tensor.is_cuda
    assert len(ref.render) == plan(len(src), ref.factor)[1]
    assert any(line.startswith("Render 1: speed 1.200000") for line in lines)


def test_speed_file(eng, tmp_path):
    rng = np.random.default_rng(21)
    t = np.arange(3001) / 44100.0
    ch = np.stack([0.6 * np.sin(2 * np.pi * 997.0 * t) + 0.2 * rng.uniform(-1, 1, len(t)),
                   0.3 * np.sin(2 * np.pi * 4001.0 * t) + 0.5 * rng.uniform(-1, 1, len(t))])
    q = np.rint(ch * 32767).astype(np.int16)
    src, dst = tmp_path / "Song.wav", render.hqnc_path(tmp_path / "Song.wav", 0)
    nio.write_wav(src, q, 44100, "pcm16")
    info = render.speed_file(src, dst, 1.2345674)
    P, n_out, _ = plan(q.shape[1], 1.234567)
    assert (info.factor, info.n_out, info.channels, info.sample_rate, info.sample_format) == \
        (1.234567, n_out, 2, 44100, "pcm16")
    back, sr, fmt = nio.read_wav_channels(dst)
    assert (sr, fmt, back.shape) == (44100, "pcm16", (2, n_out))
    step = 1.0 / 32768
    for c in range(2):
        ref = speed_ref(q[c].astype(np.float32) / 32768.0, 1.234567)
        assert np.max(np.abs(back[c] - ref)) <= step, c
    db, clip = loudness.detect_peak(dst)
    assert abs(info.peak - 10 ** (db / 20)) <= step and clip == info.is_clipping
    assert info.peak_dbfs == pytest.approx(20 * math.log10(info.peak))
    assert info.clipped_samples == 0
    # a float source stays float32, sample for sample the device render
    fsrc, fdst = tmp_path / "f.wav", tmp_path / "f out.wav"
    x = (ch * 1.5).astype(np.float32)
    nio.write_wav(fsrc, x, 48000, "float32")
    finfo = render.speed_file(fsrc, fdst, 0.8)
    fback, sr, fmt = nio.read_wav_channels(fdst)
    ys, peaks = ops.speed_render(eng, list(x), 0.8)
    assert (sr, fmt) == (48000, "float32") and np.array_equal(fback, np.stack(ys))
    assert finfo.peak == float(peaks.max()) and finfo.is_clipping
    assert finfo.clipped_samples == int(np.count_nonzero(np.abs(fback) >= 1.0)) > 0


def _run_cli(argv):
    out = stdio.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main(argv)
    return rc, out.getvalue()


def test_cli_render_hqnc(eng, tmp_path):
    nc, src = synth.make_pair(40.0, 1022)
    ncp, srp, hq = tmp_path / "nc.wav", tmp_path / "src.wav", tmp_path / "hq out.wav"
    nio.write_wav(ncp, nc, 22050, "pcm16")
    nio.write_wav(srp, src, 22050, "pcm16")
    # without the flag: exactly the log lines, the JSON and the result block, as before
    lines = []
    res = pipeline.run(str(ncp), str(srp), log=lines.append)
    today = "".join(line + "\n" for line in lines) + "\n" + json.dumps(cli.output_dict(res), indent=2) + "\n\n" \
        + str(res) + "\n"
    rc, plain = _run_cli(["-n", str(ncp), "-s", str(srp)])
    assert rc == 0 and plain == today
    rc, with_flag = _run_cli(["-n", str(ncp), "-s", str(srp), "--render-hqnc", str(hq)])
    assert rc == 0 and with_flag.startswith(today) and "HQNC written to:" in with_flag[len(today):]
    factor = res.ibi_ratio if res.ibi_ratio is not None else res.tempo_ratio
    back, sr, fmt = nio.read_wav_channels(hq)
    assert (sr, fmt, back.shape) == (22050, "pcm16", (1, plan(len(src), factor)[1]))
    # quiet, JSON to a file: nothing on stdout either way, the same JSON, and the render
    hq.unlink()
    rc, q0 = _run_cli(["-n", str(ncp), "-s", str(srp), "-q", "-o", str(tmp_path / "a.json")])
    rc2, q1 = _run_cli(["-n", str(ncp), "-s", str(srp), "-q", "-o", str(tmp_path / "b.json"),
                        "--render-hqnc", str(hq), "--refine"])
    assert (rc, rc2, q0, q1) == (0, 0, "", "")
    assert (tmp_path / "a.json").read_text() == (tmp_path / "b.json").read_text()
    assert nio.read_wav_channels(hq)[0].shape[0] == 1
    assert _run_cli(["-n", str(ncp), "-s", str(srp), "--refine"])[0] == 2
