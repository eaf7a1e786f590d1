"""Audio I/O, windowing, energy gating and silence stripping
(drop-in for the reference's nightcore_analyzer/io.py).

* ``load_audio`` (io.py:44-55): WAV (PCM 8/16/24/32-bit, IEEE float, plain or
  WAVE_FORMAT_EXTENSIBLE) and ``.npy`` are parsed with numpy on the CPU and down-mixed to mono
  float32; FLAC (native streams, 1-8 channels, 4-24 bits) is decoded on the GPU: the host
  only lists the frames (``nc_flac_index``), ``nc_flac_decode`` decodes them one wave per
  frame and mixes one or two channels to mono in HBM (``device=True`` keeps the result
  there as a ``DeviceAudio``).  A file that is not at 22 050 Hz is resampled on the GPU by
  ``nc_resample_poly`` (bit-identical to scipy.signal.resample_poly; the reference uses
  librosa.load's soxr_hq, which is absent here — see DESIGN.md).  A FLAC file loads to
  exactly the array a WAV file of the same PCM does.  MP3 and Ogg are not decoded.
* ``read_flac_channels`` / ``read_audio_channels``: the channel-preserving read of a FLAC file
  (on the GPU) and the dispatch on the suffix the renderers use.
* ``strip_silence`` (io.py:58-79) runs ``nc_trim_bounds`` on the GPU.
* ``slice_windows`` (io.py:82-112) returns views like the reference, with the
  window energies computed by ``nc_window_energy`` on the GPU.
* ``energy_gate`` (io.py:115-126) is the same list filter.
* ``read_wav_channels`` / ``write_wav`` (no counterpart in the reference's io.py, which leaves
  this to soundfile and sox): the channel-preserving WAV read and the WAV writer behind
  ``render.speed_file`` and ``loudness``; ``DeviceAudio`` is a signal that is already in HBM.
* ``write_flac`` / ``write_flac_device`` / ``write_audio``: the FLAC writer (frames encoded on the
  GPU by ``nc_flac_encode``, one wave per frame; ``fLaC`` and STREAMINFO added on the host), its
  form for a signal already in HBM, and the dispatch on the suffix.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional

import numpy as np

SAMPLE_RATE: int = 22050
WINDOW_SEC: float = 10.0
HOP_SEC: float = 5.0
ENERGY_GATE_DB: float = -40.0
SILENCE_STRIP_DB: float = 60.0


@dataclass
class AudioWindow:
    """One time slice of an audio file (io.py:27-34)."""
    audio: np.ndarray
    sample_rate: int
    start_sec: float
    end_sec: float
    energy_db: float


def _rms_db(audio: np.ndarray) -> float:
    """20 log10(max(rms, 1e-10)) with float64 accumulation (io.py:38-40), on the GPU."""
    from .engine import get_engine
    from .ops import window_energies
    return float(window_energies(get_engine(), audio, np.array([0]), len(audio))[0])


_WAVE_PCM, _WAVE_FLOAT, _WAVE_EXTENSIBLE = 1, 3, 0xFFFE


class Pcm16(np.ndarray):
    """Mono 16-bit PCM as the file stores it: int16 sample k stands for k / 32768 (soundfile's
    scaling, exact in float32).  ``load_audio(..., keep_pcm16=True)`` returns one for a mono
    16-bit WAV at the requested rate; the engine uploads its 2-byte samples (half the host ->
    HBM bytes of float32) and widens them on the device (``nc_pcm16_to_f32``), so the analysis
    sees exactly the float32 array ``load_audio`` would have returned.  Slices stay Pcm16."""

    def f32(self) -> np.ndarray:
        return self.view(np.ndarray).astype(np.float32) / np.float32(32768.0)


class DeviceAudio:
    """A mono float32 signal already resident in HBM (``ops.speed_render_device``'s output): the
    engine's loaders (``pipeline.run``, ``Engine.upload_signals``) take it in place of a
    decoded array and copy it device to device, without a trip through the host."""

    def __init__(self, tensor, sr: int = SAMPLE_RATE):
        self.tensor, self.sr = tensor, int(sr)

    def __len__(self) -> int:
        return int(self.tensor.numel())

    def numpy(self) -> np.ndarray:
        return self.tensor.cpu().numpy()

    def __getitem__(self, key) -> "DeviceAudio":
        """A slice of the signal, still in HBM (the 20 s chunks of the pitch estimate)."""
        if not isinstance(key, slice):
            raise TypeError("DeviceAudio supports slices only")
        return DeviceAudio(self.tensor.reshape(-1)[key], self.sr)


def as_f32(a) -> np.ndarray:
    """The float32 samples of ``a``: a Pcm16 scaled by 1 / 32768, anything else as float32."""
    if isinstance(a, Pcm16):
        return a.f32()
    if isinstance(a, DeviceAudio):
        return a.numpy()
    return np.asarray(a, dtype=np.float32)


def _read_wav(path: Path, keep_pcm16: bool = False):
    """RIFF/WAVE -> (mono float32, rate): PCM 8 (unsigned) / 16 / 24 / 32-bit and IEEE float
    32 / 64-bit, plain or WAVE_FORMAT_EXTENSIBLE (the sub-format GUID's first two bytes
    carry the format tag), scaled to [-1, 1) as soundfile does and averaged over channels
    (librosa.load(mono=True)).  ``keep_pcm16``: a mono 16-bit PCM file comes back as its
    stored samples (Pcm16)."""
    data = Path(path).read_bytes()
    if len(data) < 12 or data[:4] not in (b"RIFF", b"RF64") or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = raw = None
    pos = 12
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            raw = body
        pos += 8 + size + (size & 1)
    if fmt is None or raw is None or len(fmt) < 16:
        raise ValueError(f"{path}: WAVE file without fmt/data chunks")
    tag, ch = int.from_bytes(fmt[0:2], "little"), int.from_bytes(fmt[2:4], "little")
    sr, bits = int.from_bytes(fmt[4:8], "little"), int.from_bytes(fmt[14:16], "little")
    if tag == _WAVE_EXTENSIBLE and len(fmt) >= 26:
        tag = int.from_bytes(fmt[24:26], "little")          # SubFormat GUID data1 (low 16 bits)
    block_align = int.from_bytes(fmt[12:14], "little")
    if ch <= 0 or block_align <= 0 or block_align % ch:
        raise ValueError(f"{path}: invalid WAVE header (channels={ch}, block_align={block_align})")
    # the container width, not bits // 8: 12- or 20-bit samples sit left-justified in 2 or 3
    # bytes, so the bytes split into samples at block_align / channels
    width = block_align // ch
    n = len(raw) // (width * ch) * width * ch
    raw = raw[:n]
    if tag == _WAVE_FLOAT and width in (4, 8):
        x = np.frombuffer(raw, "<f4" if width == 4 else "<f8").astype(np.float32)
    elif tag == _WAVE_PCM and width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif tag == _WAVE_PCM and width == 2:
        if keep_pcm16 and ch == 1:
            return np.frombuffer(raw, "<i2").astype(np.int16).view(Pcm16), sr
        x = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    elif tag == _WAVE_PCM and width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    elif tag == _WAVE_PCM and width == 4:
        x = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported WAVE format tag {tag} with {bits}-bit samples")
    return x.reshape(-1, ch).mean(axis=1).astype(np.float32), sr


def read_wav_channels(path) -> tuple[np.ndarray, int, str]:
    """RIFF/WAVE -> (float32[channels, frames], rate, sample format) with the channels kept
    (``_read_wav`` averages them): what the renderer and the peak check need (the reference
    reads ``soundfile.read(always_2d=True)``, loudness.py:60).  Same formats and scaling as
    ``_read_wav``; the format is "pcm8" / "pcm16" / "pcm24" / "pcm32" / "float32" / "float64"."""
    data = Path(path).read_bytes()
    if len(data) < 12 or data[:4] not in (b"RIFF", b"RF64") or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = raw = None
    pos = 12
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
        if cid == b"fmt ":
            fmt = data[pos + 8:pos + 8 + size]
        elif cid == b"data":
            raw = data[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    if fmt is None or raw is None or len(fmt) < 16:
        raise ValueError(f"{path}: WAVE file without fmt/data chunks")
    tag, ch = int.from_bytes(fmt[0:2], "little"), int.from_bytes(fmt[2:4], "little")
    sr, block_align = int.from_bytes(fmt[4:8], "little"), int.from_bytes(fmt[12:14], "little")
    if tag == _WAVE_EXTENSIBLE and len(fmt) >= 26:
        tag = int.from_bytes(fmt[24:26], "little")
    if ch <= 0 or block_align <= 0 or block_align % ch:
        raise ValueError(f"{path}: invalid WAVE header (channels={ch}, block_align={block_align})")
    width = block_align // ch
    raw = raw[:len(raw) // block_align * block_align]
    if tag == _WAVE_FLOAT and width in (4, 8):
        x, name = np.frombuffer(raw, "<f4" if width == 4 else "<f8").astype(np.float32), f"float{8 * width}"
    elif tag == _WAVE_PCM and width == 1:
        x, name = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0, "pcm8"
    elif tag == _WAVE_PCM and width == 2:
        x, name = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0, "pcm16"
    elif tag == _WAVE_PCM and width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x, name = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float32) / float(1 << 23), "pcm24"
    elif tag == _WAVE_PCM and width == 4:
        x, name = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32), "pcm32"
    else:
        raise ValueError(f"{path}: unsupported WAVE format tag {tag} with {8 * width}-bit samples")
    return np.ascontiguousarray(x.reshape(-1, ch).T, dtype=np.float32), sr, name


def _flac_streaminfo(path) -> tuple[int, int, int, int]:
    """(rate, channels, bits per sample, total samples or 0) from a FLAC file's first bytes:
    an optional ID3v2 tag, the ``fLaC`` marker and the STREAMINFO block."""
    with open(path, "rb") as fh:
        head = fh.read(10)
        pos = 0
        if head[:3] == b"ID3" and len(head) == 10:
            size = (head[6] & 0x7F) << 21 | (head[7] & 0x7F) << 14 | (head[8] & 0x7F) << 7 | (head[9] & 0x7F)
            pos = 10 + size + (10 if head[5] & 0x10 else 0)
        fh.seek(pos)
        head = fh.read(42)
    if head[:4] == b"OggS":
        raise ValueError(f"{path}: Ogg container (Ogg FLAC) is not supported; only native FLAC streams are")
    if len(head) < 42 or head[:4] != b"fLaC" or head[4] & 0x7F != 0:
        raise ValueError(f"{path}: not a FLAC stream (no fLaC marker and STREAMINFO block)")
    packed = int.from_bytes(head[18:26], "big")
    return packed >> 44, ((packed >> 41) & 7) + 1, ((packed >> 36) & 31) + 1, packed & ((1 << 36) - 1)


def read_flac_channels(path, verify_md5: bool = False) -> tuple[np.ndarray, int, str]:
    """FLAC -> (float32[channels, frames], rate, "pcm<bits>"), decoded on the GPU
    (``ops.flac_decode_device``): sample k stands for k / 2^(bits-1), the scaling of
    ``read_wav_channels``, so a FLAC file reads as the WAV file of the same PCM does."""
    from .engine import get_engine
    from .ops import flac_decode_device
    sig, (info,) = flac_decode_device(get_engine(), [Path(path).read_bytes()], names=[str(path)],
                                      verify_md5=verify_md5)
    ch, n = info["channels"], info["total"]
    hy = sig.buf.cpu().numpy()
    data = np.stack([hy[o:o + n] for o in sig.off[info["first"]:info["first"] + ch]])
    return np.ascontiguousarray(data, dtype=np.float32), info["rate"], f"pcm{info['bps']}"


def read_audio_channels(path) -> tuple[np.ndarray, int, str]:
    """(float32[channels, frames], rate, sample format) of a WAV or FLAC file, by its suffix."""
    if Path(path).suffix.lower() == ".flac":
        return read_flac_channels(path)
    return read_wav_channels(path)


def _load_flac(path: Path, sr: Optional[int], device: bool):
    """``load_audio`` of a FLAC file: decode and (for one or two channels) the mono mix in
    one launch, the load-time resampler on the resident result; three and more channels are
    mixed on the host by ``_read_wav``'s own numpy expression (an 8-channel numpy mean is not
    a left-to-right sum)."""
    import math
    from .engine import DeviceSignals, get_engine
    from .ops import flac_decode_device, resample_poly_device
    import torch
    eng = get_engine()
    sig, (info,) = flac_decode_device(eng, [path.read_bytes()], names=[str(path)], mono=True)
    file_sr, ch, n = info["rate"], info["channels"], info["total"]
    if info["mono"] is not None:
        y = info["mono"]
    else:
        hy = sig.buf.cpu().numpy()
        x = np.ascontiguousarray(np.stack([hy[o:o + n] for o in sig.off[:ch]]).T).reshape(-1)
        y = torch.from_numpy(x.reshape(-1, ch).mean(axis=1).astype(np.float32)).to(eng.dev)
    if sr is None:
        sr = file_sr
    if file_sr != sr:
        g = math.gcd(int(sr), int(file_sr))
        out = resample_poly_device(eng, DeviceSignals(y, np.zeros(1, np.int64), np.array([n], np.int64)),
                                   int(sr) // g, int(file_sr) // g)
        y = out.buf[:int(out.length[0])]
    if device:
        return DeviceAudio(y, sr), sr
    return np.ascontiguousarray(y.cpu().numpy(), dtype=np.float32), sr


def quantize_pcm16(x: np.ndarray) -> tuple[np.ndarray, int]:
    """(int16 clamp(rint(x 32768), -32768, 32767), samples clamped): the host statement of
    ``nc_f32_to_pcm16`` (round half to even; x 32768 is exact in float32)."""
    v = np.rint(np.asarray(x, np.float32) * np.float32(32768.0))
    clipped = int(np.count_nonzero((v > 32767.0) | (v < -32768.0)))
    return np.clip(v, -32768.0, 32767.0).astype(np.int16), clipped


def write_wav(path, data, sr: int, sample_format: str = "float32") -> None:
    """Write ``data`` ([channels, frames] or [frames]) as a RIFF/WAVE file of 16-bit PCM
    ("pcm16") or IEEE float32 ("float32").  int16 data is written as stored (the renderer
    quantises on the device, ``nc_f32_to_pcm16``); float data going to "pcm16" is quantised
    here by the same rule (``quantize_pcm16``).  The RIFF container is assembled on the CPU;
    ``write_flac`` is the compressed sibling and ``write_audio`` picks between them by suffix."""
    a = np.asarray(data)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[0] > 65535:
        raise ValueError("write_wav: data must be [frames] or [channels, frames]")
    if sample_format == "pcm16":
        q = a if a.dtype == np.int16 else quantize_pcm16(a)[0]
        body, tag, width = np.ascontiguousarray(q.T).astype("<i2").tobytes(), _WAVE_PCM, 2
    elif sample_format == "float32":
        if a.dtype == np.int16:
            raise ValueError("write_wav: int16 data is 16-bit PCM, not float32")
        body, tag, width = np.ascontiguousarray(a.T).astype("<f4").tobytes(), _WAVE_FLOAT, 4
    else:
        raise ValueError(f"write_wav: sample format {sample_format!r} is not supported (pcm16, float32)")
    ch = a.shape[0]
    if len(body) + 36 >= 1 << 32:
        raise ValueError("write_wav: more than 4 GiB of samples does not fit a RIFF file")
    fmt = (tag.to_bytes(2, "little") + ch.to_bytes(2, "little") + int(sr).to_bytes(4, "little")
           + (int(sr) * ch * width).to_bytes(4, "little") + (ch * width).to_bytes(2, "little")
           + (8 * width).to_bytes(2, "little"))
    head = b"RIFF" + (36 + len(body)).to_bytes(4, "little") + b"WAVE" + b"fmt " + (16).to_bytes(4, "little") + fmt
    Path(path).write_bytes(head + b"data" + len(body).to_bytes(4, "little") + body)


def flac_stream_header(sr: int, channels: int, bits: int, total: int, block: int, min_frame: int, max_frame: int,
                       md5: bytes = bytes(16)) -> bytes:
    """``fLaC`` and one STREAMINFO block, marked last: min_block = max_block = ``block``."""
    packed = (int(sr) << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | int(total)
    si = (int(block).to_bytes(2, "big") * 2 + int(min_frame).to_bytes(3, "big") + int(max_frame).to_bytes(3, "big")
          + packed.to_bytes(8, "big") + bytes(md5))
    return b"fLaC" + bytes([0x80]) + len(si).to_bytes(3, "big") + si


def write_flac_device(path, eng, sig, sr: int, bits: int = 16, *, block: int = 4096, level: int = 1,
                      md5: bool = True) -> dict:
    """Write the equally long channels ``sig`` (a ``DeviceSignals`` resident in HBM, float32 or
    int32) as one FLAC file, encoded on the device (``ops.flac_encode_device``); returns the
    stream's info dict.  ``md5``: STREAMINFO's MD5 is hashed on the host from a download of the
    quantised samples; without it the field is sixteen zero bytes and no sample is downloaded."""
    import hashlib
    import torch
    from .ops import flac_encode_device
    (blob,), (info,) = flac_encode_device(eng, sig, [sig.n_files], bits, sr, block, level, names=[str(path)])
    digest = bytes(16)
    if md5:
        width = (bits + 7) // 8        # interleaved little-endian samples of `width` bytes, cut on the device
        inter = info["pcm"].t().clone(memory_format=torch.contiguous_format).reshape(-1)
        inter = inter.view(torch.uint8).view(-1, 4)[:, :width].contiguous()
        digest = hashlib.md5(inter.cpu().numpy().tobytes()).digest()
    head = flac_stream_header(sr, info["channels"], bits, info["total"], block, info["min_frame"], info["max_frame"],
                              digest)
    Path(path).write_bytes(head + blob)
    return info


def write_flac(path, data, sr: int, bits: int = 16, *, block: int = 4096, level: int = 1, md5: bool = True) -> dict:
    """Write ``data`` ([channels, frames] or [frames], 1-8 channels) as a FLAC file of ``bits``
    (4-24) per sample, encoded on the GPU.  Float data is quantised on the device by
    clamp(rint(x 2^(bits-1))) (round half to even; ``quantize_pcm16`` at 16 bits); integer data
    is taken as the samples themselves and must fit ``bits``.  ``block`` (16 .. 16384) is the
    fixed block size, ``level`` 0 or 1 the encoder's effort.  Returns the stream's info dict
    (``clipped``: samples the quantiser clamped)."""
    import torch
    from .engine import _ALIGN, DeviceSignals, get_engine
    a = np.asarray(data)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or not 1 <= a.shape[0] <= 8:
        raise ValueError("write_flac: data must be [frames] or [channels, frames] with 1 .. 8 channels")
    if not 4 <= int(bits) <= 24:
        raise ValueError(f"write_flac: {bits} bits per sample outside 4 .. 24")
    if not 16 <= int(block) <= 16384:
        raise ValueError(f"write_flac: block size {block} outside 16 .. 16384")
    if not 0 < int(sr) < 1 << 20:
        raise ValueError(f"write_flac: sample rate {sr} outside 1 .. 2^20 - 1")
    integer = a.dtype.kind in "iu"
    if integer and a.size and (a.min() < -(1 << (bits - 1)) or a.max() >= 1 << (bits - 1)):
        raise ValueError(f"write_flac: integer samples outside {bits} bits")
    ch, n = a.shape
    stride = (n + _ALIGN - 1) // _ALIGN * _ALIGN
    host = torch.zeros(max(_ALIGN, ch * stride), dtype=torch.int32 if integer else torch.float32, pin_memory=True)
    host.numpy()[:ch * stride].reshape(ch, stride)[:, :n] = a
    eng = get_engine()
    sig = DeviceSignals(host.to(eng.dev, non_blocking=True), np.arange(ch, dtype=np.int64) * stride,
                        np.full(ch, n, np.int64))
    return write_flac_device(path, eng, sig, int(sr), int(bits), block=int(block), level=int(level), md5=md5)


def write_audio(path, data, sr: int, sample_format: str = "float32", **flac_kw) -> None:
    """``write_flac`` for a ``.flac`` path, else ``write_wav``.  A FLAC file gets 16 bits per
    sample for "pcm<b>" with b <= 16 and 24 bits for every other format (``flac_bits``)."""
    if Path(path).suffix.lower() == ".flac":
        write_flac(path, data, sr, flac_bits(sample_format), **flac_kw)
    else:
        write_wav(path, data, sr, sample_format)


def flac_bits(sample_format: str) -> int:
    """Bits per sample of the FLAC file written for a source of ``sample_format``: 16 for
    "pcm<b>" with b <= 16, else 24."""
    fmt = str(sample_format)
    return 16 if fmt.startswith("pcm") and fmt[3:].isdigit() and int(fmt[3:]) <= 16 else 24


def load_audio(path: str, sr: Optional[int] = SAMPLE_RATE, *, keep_pcm16: bool = False,
               device: bool = False) -> tuple[np.ndarray, int]:
    """Decode *path* to mono float32 at *sr* Hz (io.py:44-55; WAV and .npy on the CPU, FLAC on
    the GPU).  ``sr=None`` keeps the file's own rate (librosa.load(sr=None), spectral.py:52);
    a .npy file carries no rate and is taken to be at SAMPLE_RATE.  ``keep_pcm16`` (the
    engine's loaders, pipeline.run): a mono 16-bit WAV already at *sr* is returned as its
    stored samples (``Pcm16``: the same values as float32 once scaled by 1 / 32768, on the
    device).  ``device`` (FLAC only): the decoded, mixed and resampled signal stays in HBM and
    comes back as a ``DeviceAudio``."""
    p = Path(path)
    if p.suffix.lower() == ".flac":
        return _load_flac(p, sr, device)
    if p.suffix.lower() == ".npy":
        y, file_sr = np.load(p, allow_pickle=False).astype(np.float32), sr or SAMPLE_RATE
        if y.ndim > 1:
            y = y.mean(axis=0).astype(np.float32)
    elif p.suffix.lower() == ".wav":
        y, file_sr = _read_wav(p, keep_pcm16)
        if isinstance(y, Pcm16):
            if sr is None or file_sr == sr:
                return y, file_sr
            y = y.f32()
    else:
        raise NotImplementedError(
            f"{p.suffix} decoding is not implemented (WAV, FLAC and .npy are; the reference reads the rest "
            "through librosa.load/soundfile, not installed here); convert to WAV or FLAC first")
    if sr is None:
        sr = file_sr
    if file_sr != sr:                   # io.py:54 resamples at load: on the GPU (nc_resample_poly)
        import math
        from .engine import get_engine
        from .ops import resample_poly
        g = math.gcd(int(sr), int(file_sr))
        y, = resample_poly(get_engine(), [y], int(sr) // g, int(file_sr) // g)
    return np.ascontiguousarray(y, dtype=np.float32), sr


def decoded_length(x, sr: int = SAMPLE_RATE) -> int:
    """Samples ``load_audio(x, sr)`` returns, read from the file header alone (a decoded
    array: its length): the window-sharded runs plan every rank's items from the lengths
    of all files before each rank decodes only the files it touches."""
    if isinstance(x, np.ndarray):
        return len(x)
    p = Path(x)
    if p.suffix.lower() == ".npy":
        a = np.load(p, mmap_mode="r", allow_pickle=False)
        return int(a.shape[1] if a.ndim > 1 else a.shape[0])
    if p.suffix.lower() == ".flac":            # STREAMINFO alone; the frame index when it holds no total
        file_sr, _, _, n = _flac_streaminfo(p)
        if n == 0:
            from .ops import flac_index
            n = flac_index(p.read_bytes(), str(p))[0]["total"]
        if sr is None or file_sr == sr:
            return n
        import math
        g = math.gcd(int(sr), file_sr)
        return -(-n * (int(sr) // g) // (file_sr // g))
    if p.suffix.lower() != ".wav":
        return len(load_audio(x, sr)[0])          # raises the same NotImplementedError
    size = p.stat().st_size
    fmt = None
    frames = None
    with open(p, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
            raise ValueError(f"{p}: not a RIFF/WAVE file")
        pos = 12
        while pos + 8 <= size:
            fh.seek(pos)
            ck = fh.read(8)
            cid, n = ck[:4], int.from_bytes(ck[4:8], "little")
            if cid == b"fmt ":
                fmt = fh.read(n)
            elif cid == b"data":
                frames = min(n, size - pos - 8)
            pos += 8 + n + (n & 1)
    if fmt is None or frames is None or len(fmt) < 16:
        raise ValueError(f"{p}: WAVE file without fmt/data chunks")
    ch, block_align = int.from_bytes(fmt[2:4], "little"), int.from_bytes(fmt[12:14], "little")
    if ch <= 0 or block_align <= 0 or block_align % ch:
        raise ValueError(f"{p}: invalid WAVE header (channels={ch}, block_align={block_align})")
    n = frames // block_align
    file_sr = int.from_bytes(fmt[4:8], "little")
    if sr is None or file_sr == sr:
        return n
    import math
    g = math.gcd(int(sr), file_sr)
    up, down = int(sr) // g, file_sr // g
    return -(-n * up // down)                   # resample_poly's output length


def strip_silence(audio: np.ndarray, sr: int, top_db: float = SILENCE_STRIP_DB) -> tuple[np.ndarray, float, float]:
    """(trimmed view, leading_sec, trailing_sec) — librosa.effects.trim on the GPU."""
    from .engine import get_engine
    from .ops import trim_bounds
    (start, end), = trim_bounds(get_engine(), [audio], top_db)
    return audio[start:end], start / sr, (len(audio) - end) / sr


def slice_windows(audio: np.ndarray, sr: int, window_sec: float = WINDOW_SEC,
                  hop_sec: float = HOP_SEC) -> List[AudioWindow]:
    win_n, hop_n = int(window_sec * sr), int(hop_sec * sr)
    starts = []
    s = 0
    while s + win_n <= len(audio):
        starts.append(s)
        s += hop_n
    if not starts:
        return []
    from .engine import get_engine
    from .ops import window_energies
    en = window_energies(get_engine(), audio, np.asarray(starts, np.int64), win_n)
    return [AudioWindow(audio[s:s + win_n], sr, s / sr, (s + win_n) / sr, float(e)) for s, e in zip(starts, en)]


def energy_gate(windows: List[AudioWindow], threshold_db: float = ENERGY_GATE_DB) -> List[AudioWindow]:
    if not windows:
        return windows
    peak = max(w.energy_db for w in windows)
    return [w for w in windows if w.energy_db >= peak + threshold_db]
