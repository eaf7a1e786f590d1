"""FLAC decode on the device (nc_flac_index + nc_flac_decode, flac.hip): the decoded PCM is the
expected PCM integer for integer — the RFC 9639 example streams, every case of the matrix in
tests/flac_ref.py, one by one and batched — a damaged frame is named, and a FLAC file is to
load_audio / read_audio_channels / pipeline.run / render.speed_file what the WAV file of the same
samples is."""
import dataclasses
import json
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

import flac_ref as R
from nightcore_analyzer import engine as E
from nightcore_analyzer import io as nio
from nightcore_analyzer import ops, pipeline, render, synth

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
RFC = json.loads((REPO / "tests" / "golden" / "flac_rfc9639.json").read_text())["streams"]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


@pytest.fixture(scope="module")
def cases():
    """name -> (bytes, expected int64 pcm): the RFC streams and the matrix."""
    out = {s["name"]: (bytes.fromhex(s["hex"]), np.array(s["pcm"], np.int64)) for s in RFC}
    out.update(R.matrix())
    return out


def _wav(path, pcm: np.ndarray, bps: int, sr: int):
    """pcm int [channels, n] as a 16- or 24-bit RIFF/WAVE file."""
    ch, width = pcm.shape[0], bps // 8
    raw = np.ascontiguousarray(pcm.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width].tobytes()
    fmt = struct.pack("<HHIIHH", 1, ch, sr, sr * ch * width, ch * width, bps)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


def _pcm(rng, ch: int, n: int, bps: int) -> np.ndarray:
    full = 1 << (bps - 1)
    x = rng.integers(-full, full, (ch, n))
    x[:, :2] = [[-full, full - 1]] * ch
    return x


def test_each_stream_decodes_to_the_expected_pcm(eng, cases):
    wrong = []
    for name, (data, pcm) in cases.items():
        (got, info), = ops.flac_decode(eng, [data], names=[name], verify_md5=True)
        s = R.decode(data)
        if not (got.dtype == np.int32 and got.shape == pcm.shape and np.array_equal(got, pcm)
                and (info["rate"], info["channels"], info["bps"], info["total"]) == (s.rate, s.channels, s.bps, s.total)):
            wrong.append(name)
    assert not wrong, wrong


def test_one_batched_call_decodes_every_stream(eng, cases):
    names = list(cases)
    sig, infos = ops.flac_decode_device(eng, [cases[n][0] for n in names], names=names, mono=True)
    assert sig.n_files == sum(cases[n][1].shape[0] for n in names) and np.all(sig.off % 64 == 0)
    hy = sig.buf.cpu().numpy()
    for name, info in zip(names, infos):
        pcm = cases[name][1]
        assert np.array_equal(info["pcm"].cpu().numpy(), pcm), name
        scale = np.float32(1.0 / (1 << (info["bps"] - 1)))
        f = np.stack([hy[o:o + pcm.shape[1]] for o in sig.off[info["first"]:info["first"] + pcm.shape[0]]])
        assert np.array_equal(f, pcm.astype(np.float32) * scale), name
        if pcm.shape[0] <= 2:            # the device mix is numpy's float32 mean over the channels
            want = np.ascontiguousarray(f.T).reshape(-1).reshape(-1, pcm.shape[0]).mean(axis=1).astype(np.float32)
            assert np.array_equal(info["mono"].cpu().numpy(), want), name
        else:
            assert info["mono"] is None


def test_a_flipped_payload_byte_names_its_frame(eng):
    rng = np.random.default_rng(5)
    pcm = _pcm(rng, 2, 5 * 64, 16)
    data = bytearray(R.encode_verbatim(pcm, 16, 44100, block=64))
    frames = R.decode(bytes(data)).frames
    start, end, _, _, _, _, hdr = frames[3]
    data[start + hdr + 40] ^= 0x10           # a VERBATIM sample byte: the frame still parses to its end
    with pytest.raises(ValueError, match="frame 3: CRC-16"):      # the reference agrees: only the CRC-16 fails
        R.decode(bytes(data))
    with pytest.raises(ValueError, match=r"clip\.flac: frame 3 \(samples 192 \.\. 256\): CRC-16 mismatch"):
        ops.flac_decode(eng, [bytes(data)], names=["clip.flac"])
    # the other streams of a batch are not blamed
    good = R.encode_verbatim(pcm, 16, 44100, block=64)
    with pytest.raises(ValueError, match=r"second: frame 3 "):
        ops.flac_decode(eng, [good, bytes(data)], names=["first", "second"])


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_read_flac_channels_equals_read_wav_channels(eng, tmp_path, bps, ch):
    pcm = _pcm(np.random.default_rng(10 * bps + ch), ch, 3 * 1152 + 7, bps)
    (tmp_path / "a.flac").write_bytes(R.encode_verbatim(pcm, bps, 48000, block=1152))
    _wav(tmp_path / "a.wav", pcm, bps, 48000)
    fa, fr, ff = nio.read_flac_channels(tmp_path / "a.flac", verify_md5=True)
    wa, wr, wf = nio.read_wav_channels(tmp_path / "a.wav")
    assert (fr, ff) == (wr, wf) == (48000, f"pcm{bps}")
    assert fa.dtype == wa.dtype and fa.shape == wa.shape and np.array_equal(fa, wa)
    ra, rr, rf = nio.read_audio_channels(tmp_path / "a.flac")
    assert np.array_equal(ra, wa) and (rr, rf) == (wr, wf)


@pytest.mark.parametrize("ch,bps", [(1, 16), (2, 16), (2, 24), (3, 16), (8, 24)])
def test_load_audio_of_flac_equals_load_audio_of_wav(eng, tmp_path, ch, bps):
    pcm = _pcm(np.random.default_rng(100 + ch), ch, 2 * 4096 + 333, bps)
    (tmp_path / "a.flac").write_bytes(R.encode_verbatim(pcm, bps, 44100))
    _wav(tmp_path / "a.wav", pcm, bps, 44100)
    for sr in (None, 44100, 22050):
        want, want_sr = nio.load_audio(str(tmp_path / "a.wav"), sr=sr)
        got, got_sr = nio.load_audio(str(tmp_path / "a.flac"), sr=sr)
        assert got_sr == want_sr and got.dtype == np.float32 and np.array_equal(got, want), sr
        dev, dev_sr = nio.load_audio(str(tmp_path / "a.flac"), sr=sr, device=True)
        assert isinstance(dev, nio.DeviceAudio) and dev.sr == dev_sr == want_sr and len(dev) == len(want)
        assert np.array_equal(dev.numpy(), want), sr
        assert nio.decoded_length(tmp_path / "a.flac", sr=sr) == len(want)


def test_verify_md5_passes_and_catches_an_altered_digest(eng):
    pcm = _pcm(np.random.default_rng(7), 2, 300, 24)
    data = bytearray(R.encode_verbatim(pcm, 24, 44100, block=128))
    ops.flac_decode(eng, [bytes(data)], verify_md5=True)
    data[4 + 4 + 18] ^= 0x01                      # STREAMINFO's MD5, first byte
    (got, _), = ops.flac_decode(eng, [bytes(data)], names=["m.flac"])            # unchecked by default
    assert np.array_equal(got, pcm)
    with pytest.raises(ValueError, match=r"m\.flac: MD5"):
        ops.flac_decode(eng, [bytes(data)], names=["m.flac"], verify_md5=True)
    data[4 + 4 + 18:4 + 4 + 34] = bytes(16)         # no digest stored: nothing to compare
    ops.flac_decode(eng, [bytes(data)], verify_md5=True)


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """A 30 s / 24 s synthetic pair as 16-bit mono FLAC (VERBATIM frames) and WAV files."""
    d = tmp_path_factory.mktemp("flac_pair")
    nc, src = synth.make_pair(30.0, 1021)
    for name, y in (("nc", nc), ("src", src)):
        q = np.clip(np.round(y * 32768.0), -32768, 32767).astype(np.int64)[None, :]
        (d / f"{name}.flac").write_bytes(R.encode_verbatim(q, 16, 22050))
        _wav(d / f"{name}.wav", q, 16, 22050)
    return d


def test_run_on_flac_files_equals_run_on_wav_files(eng, pair):
    la, lb = [], []
    ra = pipeline.run(str(pair / "nc.flac"), str(pair / "src.flac"), log=la.append)
    rb = pipeline.run(str(pair / "nc.wav"), str(pair / "src.wav"), log=lb.append)
    assert repr(dataclasses.asdict(ra)) == repr(dataclasses.asdict(rb))      # field for field (NaN-safe)
    assert str(ra) == str(rb) and repr(ra) == repr(rb)
    assert la == lb
    batch = pipeline.run_batch([(str(pair / "nc.flac"), str(pair / "src.flac"))])
    assert repr(batch[0]) == repr(rb)


def test_speed_file_from_flac_writes_the_bytes_it_writes_from_wav(eng, pair, tmp_path):
    a = render.speed_file(pair / "src.flac", tmp_path / "a.wav", 1.25, limit_db=-0.1)
    b = render.speed_file(pair / "src.wav", tmp_path / "b.wav", 1.25, limit_db=-0.1)
    assert a.sample_format == b.sample_format == "pcm16" and a.n_out == b.n_out
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    rng = np.random.default_rng(11)
    pcm = _pcm(rng, 2, 6000, 24) // 4
    (tmp_path / "s.flac").write_bytes(R.encode_verbatim(pcm, 24, 44100))
    _wav(tmp_path / "s.wav", pcm, 24, 44100)
    render.speed_file(tmp_path / "s.flac", tmp_path / "c.wav", 1.1)
    render.speed_file(tmp_path / "s.wav", tmp_path / "d.wav", 1.1)
    assert (tmp_path / "c.wav").read_bytes() == (tmp_path / "d.wav").read_bytes()


def test_cli_analyses_and_renders_from_flac_files(eng, pair, tmp_path, capsys):
    from nightcore_analyzer import cli
    out, hq = tmp_path / "r.json", tmp_path / "hq.wav"
    rc = cli.main(["--nightcore", str(pair / "nc.flac"), "--source", str(pair / "src.flac"), "-o", str(out),
                   "--quiet", "--render-hqnc", str(hq)])
    assert rc == 0, capsys.readouterr().err
    want = cli.output_dict(pipeline.run(str(pair / "nc.wav"), str(pair / "src.wav"), log=None))
    assert json.loads(out.read_text()) == json.loads(json.dumps(want))
    data, sr, fmt = nio.read_wav_channels(hq)
    assert (sr, fmt, data.shape[0]) == (22050, "pcm16", 1) and data.shape[1] > 0
