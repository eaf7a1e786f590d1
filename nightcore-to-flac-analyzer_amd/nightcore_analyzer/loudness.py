"""Peak / clipping detection and uniform gain reduction (the reference's loudness.py).

* ``detect_peak`` (loudness.py:40-65): the largest |sample| over ALL channels of the file in
  dBFS (not of the mono mix: one clipping channel counts), ``-inf, False`` for silence,
  clipping when the peak is at or above 0 dBFS.
* ``make_adj_path`` (loudness.py:70-81): the ``… ADJ<n>`` name beside the source.
* ``apply_gain_reduction`` (loudness.py:139-191 runs ``sox gain``): done natively for WAV —
  every sample times 10^(gain_db / 20), written in the source's sample format (16-bit PCM
  stays 16-bit PCM, anything else becomes float32).
* ``apply_true_peak_limiter`` (loudness.py:86-134 runs ``ffmpeg -af alimiter=limit=L:attack=5:
  release=50:level=disabled``): done natively for WAV on the device (``nc_true_peak_limit``),
  channels linked, no make-up gain.  PARITY UNPINNED: ffmpeg is not installed and the reference
  holds no limiter, so the definition is this project's own ("True-peak limiter").
* ``detect_true_peak``: the inter-sample companion of ``detect_peak`` (the limiter's own 4x
  estimate, ``nc_true_peak``).

The source is a WAV file (io.read_wav_channels); the result is written as WAV (io.write_wav) or,
to a ``.flac`` name, as FLAC encoded on the device (io.write_flac); a render's own
peak and clamp count come from the device (render.speed_file's RenderInfo).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .io import flac_bits, read_wav_channels, write_flac, write_flac_device, write_wav


def _channels(path) -> tuple[np.ndarray, int, str]:
    p = Path(path)
    if p.suffix.lower() != ".wav":
        raise NotImplementedError(
            f"{p.suffix} decoding is outside the engine (the reference uses soundfile, not installed here); "
            "convert to WAV first")
    return read_wav_channels(p)


def detect_peak(path) -> tuple[float, bool]:
    """(peak_dbfs, is_clipping) of the audio file at ``path``."""
    data, _, _ = _channels(path)
    peak = float(np.max(np.abs(data))) if data.size else 0.0
    if peak == 0.0:
        return -math.inf, False
    db = 20.0 * math.log10(peak)
    return db, db >= 0.0


def make_adj_path(src, version: int) -> Path:
    """``Song ADJ<version>.wav`` beside ``src``."""
    src = Path(src)
    return src.with_name(f"{src.stem} ADJ{int(version)}{src.suffix}")


def apply_gain_reduction(src, dst, gain_db: float) -> None:
    """Write ``src`` scaled by ``gain_db`` decibels (negative reduces the level) to ``dst`` (WAV,
    or FLAC for a ``.flac`` name)."""
    data, sr, fmt = _channels(src)
    if Path(dst).suffix.lower() not in (".wav", ".flac"):
        raise NotImplementedError("only WAV and FLAC output is written")
    scaled = (data.astype(np.float64) * 10.0 ** (float(gain_db) / 20.0)).astype(np.float32)
    if Path(dst).suffix.lower() == ".flac":
        write_flac(dst, scaled, sr, flac_bits(fmt))
        return
    write_wav(dst, scaled, sr, "pcm16" if fmt == "pcm16" else "float32")


@dataclass
class LimitInfo:
    """What ``apply_true_peak_limiter`` did."""
    true_peak: float           # inter-sample peak of the source, linear
    true_peak_dbfs: float
    peak_out: float            # largest |sample| of the limited signal, before any 16-bit rounding
    limited_samples: int       # frames whose gain is below 1
    limit_db: float            # the ceiling, dBFS
    attack_samples: int        # Wa
    release_samples: int       # Wr


def _dbfs(peak: float) -> float:
    return -math.inf if peak <= 0.0 else 20.0 * math.log10(peak)


def detect_true_peak(path) -> tuple[float, bool]:
    """(true_peak_dbfs, over_ceiling_at_0dBFS) of the audio file at ``path``: the largest
    inter-sample magnitude over all channels (4x, the limiter's estimate), ``-inf, False`` for
    silence, over when the true peak is above 0 dBFS."""
    from .engine import get_engine
    from .ops import true_peak_device
    data, _, _ = _channels(path)
    if not data.size:
        return -math.inf, False
    peak = float(true_peak_device(get_engine(), list(data), data.shape[0])[0].item())
    return _dbfs(peak), peak > 1.0


def apply_true_peak_limiter(src, dst, limit_db: float = -0.1, *, attack_ms: float = 5.0,
                            release_ms: float = 50.0) -> LimitInfo:
    """Write ``src`` limited to a true-peak ceiling of ``limit_db`` dBFS to ``dst`` (WAV, the
    source's sample format: 16-bit PCM stays 16-bit PCM, quantised on the device; anything else
    becomes float32; or FLAC for a ``.flac`` name, encoded on the device: 16 bits for a source of
    at most 16 bits, else 24).  Attenuates only around the over-peaks; the channels share one gain."""
    from .engine import get_engine
    from .ops import f32_to_pcm16_device, limiter_windows, true_peak_limit_device
    if not float(limit_db) <= 0.0:
        raise ValueError(f"limiter ceiling {limit_db!r} dBFS is above full scale")
    data, sr, fmt = _channels(src)
    if Path(dst).suffix.lower() not in (".wav", ".flac"):
        raise NotImplementedError("only WAV and FLAC output is written")
    ch, n = data.shape
    wa, wr = limiter_windows(sr, attack_ms, release_ms)
    eng = get_engine()
    out, tp_d, pk_d, lim_d = true_peak_limit_device(eng, list(data), ch, float(limit_db), wa, wr, in_place=True)
    if Path(dst).suffix.lower() == ".flac":      # encoded from the resident result: no float download
        from .engine import DeviceSignals
        write_flac_device(dst, eng, DeviceSignals(out.buf, np.asarray(out.off[:ch], np.int64), np.full(ch, n, np.int64)),
                          sr, flac_bits(fmt))
    elif fmt == "pcm16":
        q, _, _ = f32_to_pcm16_device(eng, out, interleave=True)
        write_wav(dst, q[:ch * n].cpu().numpy().reshape(n, ch).T, sr, "pcm16")
    else:
        hy = out.buf.cpu().numpy()
        write_wav(dst, np.stack([hy[o:o + n] for o in out.off]), sr, "float32")
    print(f"  Created: {dst}")
    tp = float(tp_d[0].item())
    return LimitInfo(tp, _dbfs(tp), float(pk_d[0].item()), int(lim_d[0].item()), float(limit_db), wa, wr)
