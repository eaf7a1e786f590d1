"""Render the sped-up source on the device and verify it in place: the part of the
reference's workflow that shells out to ``sox SRC DST speed F`` (workflow.py:108-118),
re-analyses the result against the nightcore and corrects the factor until the residual is
inside tolerance (workflow.py:766-833), without its prompts and without a file round trip.

PARITY UNPINNED: sox is not installed and the reference holds no resampler, so the
renderer's definition is this project's own (``nc_speed_render`` in
include/ncgpu.h): a Kaiser-windowed sinc (beta 10.06, 32 zero crossings a side, cut-off at
0.9 of the lower Nyquist) evaluated at the exact rational position m P / 10^6 of every output.

* ``speed`` / ``speed_file`` — the render of an array / of every channel of a WAV or FLAC file,
  written as WAV or (destination ``.flac``) as FLAC encoded on the device
  (``limit_db``: with the true-peak limiter on the resident render, loudness.py).
* ``refine_speed`` — render, re-analyse, correct; the render stays in HBM between the two.
* ``quantize_factor`` / ``hqnc_path`` — the six-decimal factor and the output naming rule.
* ``pitch_shift`` / ``pitch_file`` / ``refine_pitch`` / ``quantize_semitones`` / ``ps_path`` — the
  same for the pitch-correction step (``rubberband --pitch S`` in the reference): a phase-vocoder
  stretch plus the speed render, also parity unpinned (second half of this module).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, List, Optional

import numpy as np

from .consensus import AnalysisResult
from .io import DeviceAudio, as_f32, read_audio_channels, write_wav

Q = 1_000_000            # the six decimals of `sox … speed {F:.6f}` (workflow.py:116)
MIN_FACTOR, MAX_FACTOR = 0.25, 4.0
IBI_TOLERANCE = 0.005    # |residual - 1| accepted when the IBI ratio is available (workflow.py:160)
BPM_TOLERANCE = 0.02     # … when only the windowed tempo ratio is (workflow.py:381)


def quantize_factor(factor: float) -> float:
    """The factor the renderer really applies: round(F 10^6) / 10^6."""
    f = float(factor)
    if not math.isfinite(f) or not MIN_FACTOR <= f <= MAX_FACTOR:
        raise ValueError(f"speed factor {factor!r} outside [{MIN_FACTOR}, {MAX_FACTOR}]")
    return int(round(f * Q)) / Q


def hqnc_path(hq, version: int = 0) -> Path:
    """``Song [Nightcore].wav`` (version 0) or ``Song [Nightcore] UPD<version>.wav`` beside
    ``hq`` (the reference's naming of the sped-up file and of its corrected re-renders)."""
    hq = Path(hq)
    tail = "" if int(version) == 0 else f" UPD{int(version)}"
    return hq.with_name(f"{hq.stem} [Nightcore]{tail}{hq.suffix}")


def _dbfs(peak: float) -> float:
    return -math.inf if peak <= 0.0 else 20.0 * math.log10(peak)


@dataclass
class RenderInfo:
    """What ``speed_file`` wrote."""
    path: Path
    factor: float              # the effective factor P / 10^6
    n_out: int                 # frames written
    channels: int
    sample_rate: int
    sample_format: str         # of the written file
    peak: float                # max |sample| over all channels, before any 16-bit clamp
    peak_dbfs: float
    clipped_samples: int       # samples at or beyond full scale (clamped, in a 16-bit file)
    # with ``speed_file(limit_db=...)``: ``peak`` / ``clipped_samples`` describe the limited file
    true_peak: Optional[float] = None      # inter-sample peak of the render before the limiter
    limited_samples: int = 0               # frames the limiter turned down
    limit_db: Optional[float] = None       # the ceiling, dBFS

    @property
    def is_clipping(self) -> bool:
        return self.peak_dbfs >= 0.0


def _write_flac_render(dst_path, eng, out, ch: int, n_out: int, sr: int, fmt: str):
    """The first ``n_out`` samples of the ``ch`` resident channels ``out`` as the FLAC file
    ``dst_path``, quantised and encoded on the device (no float download): a "pcm<b>" source with
    b <= 16 gives 16 bits, any other 24.  Returns (sample format, samples the quantiser clamped)."""
    from .engine import DeviceSignals
    from .io import flac_bits, write_flac_device
    bits = flac_bits(fmt)
    sig = DeviceSignals(out.buf, np.asarray(out.off[:ch], np.int64), np.full(ch, n_out, np.int64))
    info = write_flac_device(dst_path, eng, sig, sr, bits)
    return f"pcm{bits}", info["clipped"]


def speed(y: np.ndarray, factor: float, sr: Optional[int] = None) -> np.ndarray:
    """The mono signal ``y`` played ``factor`` times faster (float32, ceil(len / factor')
    samples at the same rate, factor' = ``quantize_factor(factor)``).  ``sr`` is accepted for
    symmetry with the other seams; the render does not depend on it."""
    from .engine import get_engine
    from .ops import speed_render
    quantize_factor(factor)
    (out,), _ = speed_render(get_engine(), [np.asarray(y, np.float32).reshape(-1)], factor)
    return out


def speed_file(src_path, dst_path, factor: float, limit_db: Optional[float] = None, *,
               attack_ms: float = 5.0, release_ms: float = 50.0) -> RenderInfo:
    """Render every channel of the WAV or FLAC file ``src_path`` at its own rate and write
    ``dst_path``: a 16-bit PCM source gives a 16-bit PCM file (quantised on the device,
    ``nc_f32_to_pcm16``), anything else a float32 file; a ``dst_path`` ending in ``.flac`` is
    written as FLAC, encoded on the device from the resident render (16 bits for a source of at
    most 16 bits, else 24; ``sample_format`` "pcm16" / "pcm24").  With a ceiling ``limit_db`` (dBFS,
    at most 0) the true-peak limiter (``nc_true_peak_limit``, channels linked) runs on the
    resident render before the quantisation; the render does not leave HBM in between."""
    from .engine import get_engine
    from .ops import f32_to_pcm16_device, limiter_windows, speed_render_device, true_peak_limit_device
    f = quantize_factor(factor)
    if limit_db is not None and not float(limit_db) <= 0.0:
        raise ValueError(f"limiter ceiling {limit_db!r} dBFS is above full scale")
    data, sr, fmt = read_audio_channels(src_path)
    eng = get_engine()
    out, peak_d, P = speed_render_device(eng, list(data), f)
    ch, n_out = data.shape[0], int(out.length[0])
    extra = {}
    if limit_db is not None and ch:
        wa, wr = limiter_windows(sr, attack_ms, release_ms)
        out, tp_d, pk_d, lim_d = true_peak_limit_device(eng, out, ch, float(limit_db), wa, wr, in_place=True)
        peak_d = pk_d
        extra = dict(true_peak=tp_d, limited_samples=lim_d, limit_db=float(limit_db))
    if Path(dst_path).suffix.lower() == ".flac":
        out_fmt, clipped = _write_flac_render(dst_path, eng, out, ch, n_out, sr, fmt)
    elif fmt == "pcm16":
        q, _, clipped_d = f32_to_pcm16_device(eng, out, interleave=True)
        frames = q[:ch * n_out].cpu().numpy().reshape(n_out, ch).T
        clipped = int(clipped_d.sum().item())
        out_fmt = "pcm16"
        write_wav(dst_path, frames, sr, out_fmt)
    else:
        hy = out.buf.cpu().numpy()
        frames = np.stack([hy[o:o + n_out] for o in out.off])
        clipped = int(np.count_nonzero(np.abs(frames) >= 1.0))
        out_fmt = "float32"
        write_wav(dst_path, frames, sr, out_fmt)
    peak = float(peak_d.max().item()) if ch else 0.0
    if extra:
        extra.update(true_peak=float(extra["true_peak"][0].item()),
                     limited_samples=int(extra["limited_samples"][0].item()))
    return RenderInfo(Path(dst_path), P / Q, n_out, ch, sr, out_fmt, peak, _dbfs(peak), clipped, **extra)


@dataclass
class Refinement:
    """The verify-and-correct loop's record."""
    factors: List[float] = field(default_factory=list)       # every factor rendered, in order
    results: List[AnalysisResult] = field(default_factory=list)   # nightcore against each render
    residuals: List[float] = field(default_factory=list)
    converged: bool = False
    estimator: str = "IBI"                                    # of the last residual: "IBI" or "BPM"
    initial: Optional[AnalysisResult] = None                  # nightcore against the source (no ``start``)
    render: Optional[DeviceAudio] = None                      # the last render, resident in HBM

    @property
    def factor(self) -> float:
        return self.factors[-1]

    @property
    def corrections(self) -> int:
        return max(0, len(self.factors) - 1)


def refine_speed(nightcore, source, *, start: Optional[float] = None, max_renders: int = 4,
                 log: Optional[Callable[[str], None]] = None) -> Refinement:
    """The workflow's create-verify-correct loop (workflow.py:766-833) on the 22 050 Hz mono
    analysis copies.  First factor: ``start``, else the IBI ratio of nightcore against source,
    else their tempo ratio.  Each pass renders the source at the factor on the device,
    analyses the nightcore against the render (``pipeline.run(compute_pitch=False)``; the
    render never leaves HBM) and takes the residual (IBI ratio, else tempo ratio); inside
    tolerance (0.5 % IBI, 2 % BPM) it stops, otherwise factor <- quantize(factor residual)."""
    from . import pipeline
    from .engine import get_engine
    from .ops import speed_render_device

    def _log(msg: str) -> None:
        if log is not None:
            log(msg)

    if max_renders < 1:
        raise ValueError("refine_speed: max_renders must be at least 1")
    nc = as_f32(pipeline._load(nightcore, _log, "nightcore"))
    src = as_f32(pipeline._load(source, _log, "source"))
    out = Refinement()
    if start is None:
        out.initial = pipeline.run(nc, src, compute_pitch=False, log=log)
        start = out.initial.ibi_ratio if out.initial.ibi_ratio is not None else out.initial.tempo_ratio
    factor = quantize_factor(start)
    eng = get_engine()
    resident = eng.upload_signals([src])
    for k in range(max_renders):
        _log(f"Render {k + 1}: speed {factor:.6f}×")
        rendered, _, _ = speed_render_device(eng, resident, factor)
        out.render = DeviceAudio(rendered.buf[:int(rendered.length[0])])
        out.factors.append(factor)
        res = pipeline.run(nc, out.render, compute_pitch=False, log=log)
        out.results.append(res)
        ibi = res.ibi_ratio is not None
        residual = float(res.ibi_ratio if ibi else res.tempo_ratio)
        out.residuals.append(residual)
        out.estimator = "IBI" if ibi else "BPM"
        _log(f"  residual ({out.estimator}): {residual:.6f}  ({(residual - 1.0) * 100:+.2f} %)")
        if abs(residual - 1.0) < (IBI_TOLERANCE if ibi else BPM_TOLERANCE):
            out.converged = True
            break
        if k + 1 < max_renders:
            factor = quantize_factor(factor * residual)
    return out


# ------------------------------------------------------------------ pitch shift (pvoc.hip + speed.hip)
# What the reference's workflow shells out to `rubberband --pitch S SRC DST` for
# (workflow.py:121-131) and the pitch-correction loop built on it (workflow.py:652-704).
# PARITY UNPINNED: rubberband is not installed and the reference holds no pitch shifter; the
# definition is this project's own (DESIGN.md §4 "Pitch shift", tests/pvoc_ref.py): a plain
# phase-vocoder time stretch by 2^(S/12) (no transient detection, no phase locking, channels
# independent) followed by the speed render at the same ratio.  ``phase_lock=True`` opts into
# identity phase locking with the channels of a file linked to the phases of their sum
# (DESIGN.md §4 "Phase locking", tests/pvoc_lock_ref.py); transients are still not handled.
PITCH_TOLERANCE_ST = 0.5   # |shift| below which the reference renders nothing (workflow.py:640, 697)


def quantize_semitones(semitones: float) -> float:
    """The pitch ratio P / 10^6 really applied for a shift by ``semitones``: S rounded to the
    six decimals the reference hands to rubberband (``--pitch {S:+.6f}``), P = round(2^(S/12) 10^6)."""
    from .ops import pitch_p
    return pitch_p(semitones) / Q


def ps_path(src, version: int) -> Path:
    """``Song PS<version>.wav`` beside ``src`` (workflow._make_ps_path)."""
    src = Path(src)
    return src.with_name(f"{src.stem} PS{int(version)}{src.suffix}")


def _lock_mode(phase_lock) -> Optional[str]:
    if not isinstance(phase_lock, (bool, np.bool_)):
        raise ValueError(f"phase_lock must be True or False, not {phase_lock!r}")
    return "identity" if phase_lock else None


def pitch_shift(y: np.ndarray, semitones: float, sr: Optional[int] = None, *, phase_lock: bool = False) -> np.ndarray:
    """The mono signal ``y`` shifted in pitch by ``semitones`` (float32, len(y) samples at the same
    rate).  ``sr`` is accepted for symmetry with the other seams; the shift does not depend on it.
    ``phase_lock``: identity phase locking (DESIGN.md §4 "Phase locking")."""
    from .engine import get_engine
    from . import ops
    quantize_semitones(semitones)
    lock = _lock_mode(phase_lock)
    return ops.pitch_shift(get_engine(), [np.asarray(y, np.float32).reshape(-1)], semitones, lock=lock)[0]


@dataclass
class PitchInfo(RenderInfo):
    """What ``pitch_file`` wrote: a ``RenderInfo`` whose ``factor`` is the pitch ratio P / 10^6
    and whose ``peak`` is that of the whole render (up to two samples longer than the file) when
    no limiter ran."""
    semitones: float = 0.0     # the shift applied (six decimals)
    phase_lock: bool = False   # identity phase locking, the file's channels linked


def pitch_file(src_path, dst_path, semitones: float, limit_db: Optional[float] = None, *,
               attack_ms: float = 5.0, release_ms: float = 50.0, phase_lock: bool = False) -> PitchInfo:
    """Shift every channel of the WAV or FLAC file ``src_path`` by ``semitones`` at its own rate and
    write ``dst_path`` (same rate, channels and length): a 16-bit PCM source gives a 16-bit PCM
    file (``nc_f32_to_pcm16``), anything else a float32 file; a ``.flac`` destination is encoded on
    the device as in ``speed_file``.  With a ceiling ``limit_db`` the
    true-peak limiter runs on the resident result first, as in ``speed_file``.  ``phase_lock``:
    identity phase locking with all channels of the file linked to the phases of their sum
    (DESIGN.md §4 "Phase locking")."""
    from .engine import get_engine
    from .ops import f32_to_pcm16_device, limiter_windows, pitch_shift_device, true_peak_limit_device
    ratio = quantize_semitones(semitones)
    lock = _lock_mode(phase_lock)
    if limit_db is not None and not float(limit_db) <= 0.0:
        raise ValueError(f"limiter ceiling {limit_db!r} dBFS is above full scale")
    data, sr, fmt = read_audio_channels(src_path)
    eng = get_engine()
    ch, n_out = data.shape[0], int(data.shape[1])
    out, peak_d, P = pitch_shift_device(eng, list(data), semitones, lock=lock, channels=max(1, ch))
    extra = {}
    if limit_db is not None and ch:
        wa, wr = limiter_windows(sr, attack_ms, release_ms)
        out, tp_d, pk_d, lim_d = true_peak_limit_device(eng, out, ch, float(limit_db), wa, wr, in_place=True)
        peak_d = pk_d
        extra = dict(true_peak=tp_d, limited_samples=lim_d, limit_db=float(limit_db))
    if Path(dst_path).suffix.lower() == ".flac":
        out_fmt, clipped = _write_flac_render(dst_path, eng, out, ch, n_out, sr, fmt)
    elif fmt == "pcm16":
        q, _, clipped_d = f32_to_pcm16_device(eng, out, interleave=True)
        frames = q[:ch * n_out].cpu().numpy().reshape(n_out, ch).T
        clipped = int(clipped_d.sum().item())
        out_fmt = "pcm16"
        write_wav(dst_path, frames, sr, out_fmt)
    else:
        hy = out.buf.cpu().numpy()
        frames = np.stack([hy[o:o + n_out] for o in out.off])
        clipped = int(np.count_nonzero(np.abs(frames) >= 1.0))
        out_fmt = "float32"
        write_wav(dst_path, frames, sr, out_fmt)
    peak = float(peak_d.max().item()) if ch else 0.0
    if extra:
        extra.update(true_peak=float(extra["true_peak"][0].item()),
                     limited_samples=int(extra["limited_samples"][0].item()))
    return PitchInfo(Path(dst_path), ratio, n_out, ch, sr, out_fmt, peak, _dbfs(peak), clipped,
                     semitones=round(float(semitones), 6), phase_lock=lock is not None, **extra)


@dataclass
class PitchRefinement:
    """The pitch-correction loop's record."""
    shifts: List[float] = field(default_factory=list)        # every shift rendered (semitones), in order
    residuals: List[float] = field(default_factory=list)     # nightcore against each render (semitones)
    converged: bool = False
    method: str = "chroma_xcorr"                             # of the last estimate
    initial: Optional[float] = None                          # nightcore against the source (no ``start``)
    render: Optional[DeviceAudio] = None                     # the last render, resident in HBM

    @property
    def total_shift(self) -> float:
        return float(sum(self.shifts))

    @property
    def corrections(self) -> int:
        return max(0, len(self.shifts) - 1)


def _pitch_shift_estimate(cur, nc, sr: int, log):
    """(12 log2(median nc_hz / median cur_hz), method) by ``pitch.estimate_pitch_combined``, or
    (None, method) without voiced values on either side (workflow.py:621-628)."""
    from . import pitch
    a_hz, n_hz, method = pitch.estimate_pitch_combined(cur, nc, sr, log=log)
    va = [v for v in a_hz if v is not None and v > 0]
    vn = [v for v in n_hz if v is not None and v > 0]
    if not va or not vn:
        return None, method
    return 12.0 * math.log2(float(np.median(vn)) / float(np.median(va))), method


def refine_pitch(nightcore, source, *, start: Optional[float] = None, max_renders: int = 4,
                 log: Optional[Callable[[str], None]] = None, phase_lock: bool = False) -> PitchRefinement:
    """The workflow's pitch-correction loop (workflow.py:652-704) without its prompts, on the
    22 050 Hz mono analysis copies.  First shift: ``start``, else
    12 log2(median nc_hz / median src_hz) of ``pitch.estimate_pitch_combined``; below 0.5 st
    nothing is rendered (converged, no shifts).  Each pass shifts the CURRENT render (the source
    at first) by the shift on the device, re-estimates the nightcore against it and makes the
    residual the next shift; it stops when the residual is below 0.5 st.  The render stays in
    HBM between the passes.  ``phase_lock``: every render uses identity phase locking.

    The chroma estimate keeps the reference's ``lag / 3`` (pitch.py: 36 bins per octave folded to
    12 chroma bins), so without MELODIA a true shift of S semitones is reported as
    S / 3, and the loop inherits that: it is the reference's loop, not a better one."""
    from . import pipeline, pitch
    from .engine import SR, get_engine
    from .ops import pitch_shift_device

    def _log(msg: str) -> None:
        if log is not None:
            log(msg)

    if max_renders < 1:
        raise ValueError("refine_pitch: max_renders must be at least 1")
    lock = _lock_mode(phase_lock)
    nc = as_f32(pipeline._load(nightcore, _log, "nightcore"))
    src = as_f32(pipeline._load(source, _log, "source"))
    out = PitchRefinement()
    if start is None:
        shift, out.method = _pitch_shift_estimate(src, nc, SR, log)
        out.initial = shift
        if shift is None:
            _log("Pitch analysis: insufficient voiced frames — no result.")
            return out
    else:
        shift = float(start)
    if abs(shift) < PITCH_TOLERANCE_ST:
        _log(f"Pitch shift {shift:+.6f} st is below the {PITCH_TOLERANCE_ST} st threshold: nothing rendered")
        out.converged = True
        return out
    eng = get_engine()
    resident = eng.upload_signals([src])
    host_estimate = pitch.melodia_backend() is not None   # MELODIA reads host arrays
    for k in range(max_renders):
        _log(f"Render {k + 1}: pitch {shift:+.6f} st")
        resident, _, _ = pitch_shift_device(eng, resident, shift, lock=lock)
        out.render = DeviceAudio(resident.buf[:int(resident.length[0])])
        out.shifts.append(round(float(shift), 6))
        cur = out.render.numpy() if host_estimate else out.render
        residual, out.method = _pitch_shift_estimate(cur, nc, SR, log)
        if residual is None:
            _log("  Verification: insufficient voiced frames — cannot confirm correction.")
            break
        out.residuals.append(residual)
        _log(f"  residual ({out.method}): {residual:+.6f} st")
        if abs(residual) < PITCH_TOLERANCE_ST:
            out.converged = True
            break
        shift = residual
    return out
