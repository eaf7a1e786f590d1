"""FLAC encode on the device (nc_flac_encode + nc_flac_pack, flac_enc.hip): at level 0 the bytes
are those of the plain-Python choice rule (tests/flac_enc_ref.py), case by case and batched; at
both levels the device's own decoder and the Python decoder give back the input integer for
integer; a level 1 frame is never longer than its level 0 frame; float input is quantised as
nc_f32_to_pcm16 does; and the file writers write .flac files that read back as their .wav twins."""
import dataclasses
import struct

import numpy as np
import pytest
import torch

import flac_enc_ref as X
import flac_ref as R
from nightcore_analyzer import engine as E
from nightcore_analyzer import io as nio
from nightcore_analyzer import loudness, ops, render, synth

pytestmark = pytest.mark.gpu

SMALL = 5000        # cases up to this many samples also go through the Python decoder


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


@pytest.fixture(scope="module")
def encoded(eng):
    """name -> level -> (frame bytes, info): every case of the matrix, encoded once per level."""
    out = {}
    for name, (pcm, bps, rate, block) in X.cases().items():
        out[name] = {level: ops.flac_encode(eng, [pcm], bps, rate, block, level)[0] for level in (0, 1)}
    return out


def _file(pcm, bps, rate, block, blob, info) -> bytes:
    return nio.flac_stream_header(rate, pcm.shape[0], bps, pcm.shape[1], block, info["min_frame"], info["max_frame"],
                                  R.md5_of(pcm, bps)) + blob


def _wav(path, pcm: np.ndarray, bps: int, sr: int):
    ch, width = pcm.shape[0], bps // 8
    raw = np.ascontiguousarray(pcm.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width].tobytes()
    fmt = struct.pack("<HHIIHH", 1, ch, sr, sr * ch * width, ch * width, bps)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


@pytest.mark.parametrize("name", list(X.cases()))
def test_level0_bytes_equal_the_reference_rule(encoded, name):
    pcm, bps, rate, block = X.cases()[name]
    blob, info = encoded[name][0]
    want = X.encode_frames(pcm, bps, rate, block)
    assert info["frame_bytes"].tolist() == [len(f) for f in want]
    assert blob == b"".join(want)
    assert info["clipped"] == 0 and np.array_equal(info["pcm"], pcm)


def test_batched_call_equals_each_case_alone(eng, encoded):
    names = list(X.cases())
    arrays = [X.cases()[n][0] for n in names]
    bits = [X.cases()[n][1] for n in names]
    rates = [X.cases()[n][2] for n in names]
    by_block = {}
    for i, n in enumerate(names):
        by_block.setdefault(X.cases()[n][3], []).append(i)
    for block, idx in by_block.items():
        for level in (0, 1):
            got = ops.flac_encode(eng, [arrays[i] for i in idx], [bits[i] for i in idx], [rates[i] for i in idx],
                                  block, level)
            for (blob, info), i in zip(got, idx):
                alone_blob, alone = encoded[names[i]][level]
                assert blob == alone_blob, (names[i], level)
                assert np.array_equal(info["records"], alone["records"]) and info["clipped"] == alone["clipped"]


@pytest.mark.parametrize("level", [0, 1])
def test_both_decoders_return_the_input(eng, encoded, level):
    files, names = [], []
    for name, (pcm, bps, rate, block) in X.cases().items():
        blob, info = encoded[name][level]
        files.append(_file(pcm, bps, rate, block, blob, info))
        names.append(name)
        if pcm.size <= SMALL:
            assert np.array_equal(R.decode(files[-1]).pcm, pcm), name
    for name, (got, info) in zip(names, ops.flac_decode(eng, files, names=names, verify_md5=True)):
        pcm, bps, rate, _ = X.cases()[name]
        assert (info["rate"], info["channels"], info["bps"], info["total"]) == (rate, pcm.shape[0], bps, pcm.shape[1])
        assert np.array_equal(got, pcm), name


def test_level1_frames_are_never_longer_than_level0(encoded):
    for name in X.cases():
        a, b = encoded[name][0][1]["frame_bytes"], encoded[name][1][1]["frame_bytes"]
        assert len(a) == len(b) and np.all(b <= a), name


def test_records_describe_the_stream(encoded):
    for name, (pcm, bps, rate, block) in X.cases().items():
        if pcm.size > SMALL:
            continue
        for level in (0, 1):
            blob, info = encoded[name][level]
            desc = X.describe(_file(pcm, bps, rate, block, blob, info))
            for f, (assign, subs) in enumerate(desc):
                assert info["records"][f, 0] == assign
                for c, (typ, order, po, _) in enumerate(subs):
                    rec = info["records"][f, 1 + 3 * c:4 + 3 * c]
                    assert (ops.FLAC_SUBFRAME_TYPES[rec[0]], rec[1], rec[2]) == (typ, order, po), (name, f, c)
    # the spike in a one-partition block: k = 9, a unary run of 117 zeros
    pcm, bps, rate, block = X.cases()["spike_run117"]
    blob, info = encoded["spike_run117"][0]
    assert X.describe(_file(pcm, bps, rate, block, blob, info)) == [(0, [("fixed", 0, 0, [9])])]


def test_level1_takes_lpc_for_a_high_tone(eng):
    rng = np.random.default_rng(31)
    n = np.arange(3 * 4096)
    x = np.rint(8000 * np.sin(2 * np.pi * 0.31 * n) + rng.normal(0, 2, len(n))).astype(np.int64)[None, :]
    (b0, i0), = ops.flac_encode(eng, [x], 16, 44100, 4096, 0)
    (b1, i1), = ops.flac_encode(eng, [x], 16, 44100, 4096, 1)
    desc = X.describe(_file(x, 16, 44100, 4096, b1, i1))
    assert any(sub[0] == "lpc" for _, subs in desc for sub in subs)
    assert len(b1) < len(b0) and np.all(i1["frame_bytes"] <= i0["frame_bytes"])
    (got, _), = ops.flac_decode(eng, [_file(x, 16, 44100, 4096, b1, i1)], verify_md5=True)
    assert np.array_equal(got, x)


@pytest.mark.parametrize("bits", [16, 24])
def test_float_input_is_quantised_by_the_f32_to_pcm16_rule(eng, bits):
    rng = np.random.default_rng(bits)
    full = float(1 << (bits - 1))
    x = rng.uniform(-1.1, 1.1, (2, 700)).astype(np.float32)
    k = np.arange(-40, 40, dtype=np.float32)
    x[0, :80] = (k + np.float32(0.5)) / np.float32(full)                 # ties: round half to even
    x[1, :80] = (k * 400 + np.float32(0.5)) / np.float32(full)
    x[0, 80:88] = [1.0, -1.0, 1.5, -1.5, (full - 1) / full, -(full + 1) / full, (full - 0.5) / full, -(full + 0.5) / full]
    v = np.rint(x * np.float32(full))
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    want, clipped = np.clip(v, lo, hi).astype(np.int64), int(np.count_nonzero((v > hi) | (v < lo)))
    if bits == 16:
        q16, c16 = nio.quantize_pcm16(x)
        assert np.array_equal(want, q16) and clipped == c16
        (dev16,), devc = ops.f32_to_pcm16(eng, [x[0]])
        assert np.array_equal(dev16, want[0]) and int(devc[0]) == int(np.count_nonzero((v[0] > hi) | (v[0] < lo)))
    sig = eng.upload_signals([x[0], x[1]])
    (blob,), (info,) = ops.flac_encode_device(eng, sig, [2], bits, 48000, 256, 1)
    assert np.array_equal(info["pcm"].cpu().numpy(), want) and info["clipped"] == clipped and clipped > 0
    (got, _), = ops.flac_decode(eng, [_file(want, bits, 48000, 256, blob, info)], verify_md5=True)
    assert np.array_equal(got, want)


def test_write_flac_round_trips(eng, tmp_path):
    rng = np.random.default_rng(8)
    x = (0.5 * np.sin(np.arange(9000) * 0.02)[None, :] * np.array([[1.0], [-0.7]]) + rng.normal(0, 1e-3, (2, 9000)))
    x = x.astype(np.float32)
    info = nio.write_flac(tmp_path / "a.flac", x, 44100)
    data, sr, fmt = nio.read_flac_channels(tmp_path / "a.flac", verify_md5=True)
    assert (sr, fmt) == (44100, "pcm16") and np.array_equal(data, nio.quantize_pcm16(x)[0].astype(np.float32) / 32768.0)
    raw = (tmp_path / "a.flac").read_bytes()
    st = ops.flac_index(raw)[0]
    assert st["md5"] != bytes(16) and int.from_bytes(raw[8:10], "big") == int.from_bytes(raw[10:12], "big") == 4096
    assert (int.from_bytes(raw[12:15], "big"), int.from_bytes(raw[15:18], "big")) == (info["min_frame"], info["max_frame"])
    assert raw[4] == 0x80 and len(raw) == 42 + int(info["frame_bytes"].sum())
    # 24 bits, integer input, no MD5, a small block, mono; write_audio by suffix
    pcm = rng.integers(-(1 << 23), 1 << 23, 1000)
    nio.write_flac(tmp_path / "b.flac", pcm, 48000, 24, block=192, level=0, md5=False)
    raw = (tmp_path / "b.flac").read_bytes()
    assert raw[26:42] == bytes(16)
    data, sr, fmt = nio.read_audio_channels(tmp_path / "b.flac")
    assert (sr, fmt) == (48000, "pcm24") and np.array_equal(data[0], pcm.astype(np.float32) / float(1 << 23))
    nio.write_audio(tmp_path / "c.flac", x, 22050, "pcm16")
    nio.write_audio(tmp_path / "c.wav", x, 22050, "pcm16")
    assert np.array_equal(nio.read_audio_channels(tmp_path / "c.flac")[0], nio.read_wav_channels(tmp_path / "c.wav")[0])
    nio.write_audio(tmp_path / "d.flac", x, 22050, "float32")
    assert nio.read_audio_channels(tmp_path / "d.flac")[2] == "pcm24"


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """A 3 s stereo source whose left channel is a clipped sine, as a 16-bit and as a 24-bit WAV file."""
    d = tmp_path_factory.mktemp("flac_enc_src")
    rng = np.random.default_rng(77)
    t = np.arange(3 * 22050) / 22050.0
    y = np.stack([np.clip(1.6 * np.sin(2 * np.pi * 440 * t), -1, 1), 0.9 * np.sin(2 * np.pi * 557 * t + 1.0)])
    y += rng.normal(0, 0.002, y.shape)
    _wav(d / "s16.wav", np.clip(np.rint(y * 32768), -32768, 32767).astype(np.int64), 16, 22050)
    _wav(d / "s24.wav", np.clip(np.rint(y * 0.5 * (1 << 23)), -(1 << 23), (1 << 23) - 1).astype(np.int64), 24, 22050)
    return d


@pytest.mark.parametrize("limit", [None, -0.1])
def test_speed_file_to_flac_equals_speed_file_to_wav(eng, sources, tmp_path, limit):
    a = render.speed_file(sources / "s16.wav", tmp_path / "a.flac", 1.25, limit_db=limit)
    b = render.speed_file(sources / "s16.wav", tmp_path / "b.wav", 1.25, limit_db=limit)
    fa, sra, fmta = nio.read_flac_channels(tmp_path / "a.flac", verify_md5=True)
    fb, srb, fmtb = nio.read_wav_channels(tmp_path / "b.wav")
    assert (sra, fmta) == (srb, fmtb) == (22050, "pcm16") and np.array_equal(fa, fb)
    da, db = dataclasses.asdict(a), dataclasses.asdict(b)
    assert da.pop("path") == tmp_path / "a.flac" and db.pop("path") == tmp_path / "b.wav"
    assert da == db and a.sample_format == "pcm16"
    assert (tmp_path / "a.flac").stat().st_size < (tmp_path / "b.wav").stat().st_size
    if limit is None:
        assert a.clipped_samples > 0            # a clipped sine overshoots when resampled: the WAV path's count


def test_a_24_bit_source_gives_a_24_bit_flac(eng, sources, tmp_path):
    info = render.speed_file(sources / "s24.wav", tmp_path / "a.flac", 1.1)
    ref = render.speed_file(sources / "s24.wav", tmp_path / "a.wav", 1.1)
    data, sr, fmt = nio.read_flac_channels(tmp_path / "a.flac", verify_md5=True)
    assert (fmt, info.sample_format, ref.sample_format) == ("pcm24", "pcm24", "float32")
    want = np.clip(np.rint(nio.read_wav_channels(tmp_path / "a.wav")[0] * np.float32(1 << 23)), -(1 << 23), (1 << 23) - 1)
    assert np.array_equal(data, want.astype(np.float32) / float(1 << 23))
    assert (info.n_out, info.peak, info.factor) == (ref.n_out, ref.peak, ref.factor)


def test_other_writers_write_flac_files_that_load(eng, sources, tmp_path):
    p = render.pitch_file(sources / "s16.wav", tmp_path / "p.flac", 2.0, limit_db=-0.1)
    pw = render.pitch_file(sources / "s16.wav", tmp_path / "p.wav", 2.0, limit_db=-0.1)
    assert p.sample_format == "pcm16" and p.n_out == pw.n_out
    assert np.array_equal(nio.read_flac_channels(tmp_path / "p.flac", verify_md5=True)[0],
                          nio.read_wav_channels(tmp_path / "p.wav")[0])
    loudness.apply_true_peak_limiter(sources / "s16.wav", tmp_path / "l.flac", -1.0)
    loudness.apply_true_peak_limiter(sources / "s16.wav", tmp_path / "l.wav", -1.0)
    loudness.apply_gain_reduction(sources / "s16.wav", tmp_path / "g.flac", -3.0)
    loudness.apply_gain_reduction(sources / "s16.wav", tmp_path / "g.wav", -3.0)
    for stem in ("l", "g"):
        assert np.array_equal(nio.read_flac_channels(tmp_path / f"{stem}.flac", verify_md5=True)[0],
                              nio.read_wav_channels(tmp_path / f"{stem}.wav")[0]), stem
    for stem in ("p", "l", "g"):
        y, sr = nio.load_audio(str(tmp_path / f"{stem}.flac"))
        yw, _ = nio.load_audio(str(tmp_path / f"{stem}.wav"))
        assert sr == 22050 and len(y) == 3 * 22050 and np.array_equal(y, yw)
    with pytest.raises(NotImplementedError):
        loudness.apply_gain_reduction(sources / "s16.wav", tmp_path / "g.mp3", -3.0)


def test_cli_renders_to_a_flac_file(eng, tmp_path, capsys):
    from nightcore_analyzer import cli
    nc, src = synth.make_pair(30.0, 1021)
    for name, y in (("nc", nc), ("src", src)):
        _wav(tmp_path / f"{name}.wav", np.clip(np.round(y * 32768.0), -32768, 32767).astype(np.int64)[None, :], 16, 22050)
    hq = tmp_path / "Song [Nightcore].flac"
    rc = cli.main(["--nightcore", str(tmp_path / "nc.wav"), "--source", str(tmp_path / "src.wav"), "-o",
                   str(tmp_path / "r.json"), "--quiet", "--render-hqnc", str(hq)])
    assert rc == 0, capsys.readouterr().err
    assert hq.read_bytes()[:4] == b"fLaC"
    data, sr, fmt = nio.read_audio_channels(hq)
    assert (sr, fmt, data.shape[0]) == (22050, "pcm16", 1) and data.shape[1] > 0
    y, sr = nio.load_audio(str(hq))
    assert sr == 22050 and len(y) == data.shape[1]


def test_bad_arguments_raise_before_any_launch(eng, tmp_path):
    x = np.zeros((1, 100), np.int64)
    calls = []
    real = eng.call
    eng.call = lambda *a: calls.append(a[0])
    try:
        for kw in (dict(block=15), dict(block=16385), dict(bits=3), dict(bits=25)):
            args = dict(bits=16, block=4096)
            args.update(kw)
            with pytest.raises(ValueError):
                ops.flac_encode(eng, [x], args["bits"], 44100, args["block"], 1)
            with pytest.raises(ValueError):
                nio.write_flac(tmp_path / "bad.flac", x, 44100, args["bits"], block=args["block"])
        with pytest.raises(ValueError):
            ops.flac_encode(eng, [x], 16, 44100, 4096, 2)
        with pytest.raises(ValueError):
            ops.flac_encode(eng, [np.zeros((9, 10), np.int64)], 16, 44100)
    finally:
        eng.call = real
    assert calls == [] and not (tmp_path / "bad.flac").exists()
    with pytest.raises(ValueError, match=r"stream 0: frame 1 \(samples 64 \.\. 100\): sample outside the sample size"):
        big = x.copy()
        big[0, 70] = 40000
        ops.flac_encode(eng, [big], 16, 44100, 64)
