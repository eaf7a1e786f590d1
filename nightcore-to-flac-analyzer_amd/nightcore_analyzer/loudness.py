"""Peak / clipping detection and uniform gain reduction (the reference's loudness.py).

* ``detect_peak`` (loudness.py:40-65): the largest |sample| over ALL channels of the file in
  dBFS (not of the mono mix: one clipping channel counts), ``-inf, False`` for silence,
  clipping when the peak is at or above 0 dBFS.
* ``make_adj_path`` (loudness.py:70-81): the ``… ADJ<n>`` name beside the source.
* ``apply_gain_reduction`` (loudness.py:139-191 runs ``sox gain``): done natively for WAV —
  every sample times 10^(gain_db / 20), written in the source's sample format (16-bit PCM
  stays 16-bit PCM, anything else becomes float32).
* The true-peak limiter (``ffmpeg alimiter``) is not provided.

File decode and encode stay on the CPU (io.read_wav_channels / io.write_wav); a render's own
peak and clamp count come from the device (render.speed_file's RenderInfo).
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np

from .io import read_wav_channels, write_wav


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
    """Write ``src`` scaled by ``gain_db`` decibels (negative reduces the level) to ``dst``."""
    data, sr, fmt = _channels(src)
    if Path(dst).suffix.lower() != ".wav":
        raise NotImplementedError("only WAV output is written")
    scaled = (data.astype(np.float64) * 10.0 ** (float(gain_db) / 20.0)).astype(np.float32)
    write_wav(dst, scaled, sr, "pcm16" if fmt == "pcm16" else "float32")
