"""The launch of every device stage that more than one caller queues: the pipelined groups
(engine.py), the drop-in seams (ops.py) and the per-rank stages (sharded.py).  Each function is
the one place in the package that names its entry point(s) and owns what goes with the call:
argument order, placeholders and constants, derived sizes, the workspace (size query and name).

Device arrays may be tensors or ``engine._DevSpan``s: anything with ``data_ptr()``.  An output
that is given is used as it is (no view is built, nothing is allocated: the groups pass spans of
their arena); one that is omitted is allocated here.  Every launch goes through ``eng.call`` on the
current stream (``st``: its raw handle, where the caller has it), or on ``stream`` (a torch stream): the
workspace is then recorded on it, so the allocator does not hand it out again while the kernel is queued.
"""
from __future__ import annotations

import numpy as np
import torch

from . import consensus as C


def frames_of(n, hop: int):
    """Centred frames of n samples at this hop (n: an int or an array of lengths)."""
    return 1 + n // hop


def tempogram_window(sr: int, hop: int) -> int:
    """Tempogram lags: librosa's 8 s autocorrelation window in frames at this rate and hop."""
    return int(int(8.0 * sr) // hop)


def ibi_lists(vals: np.ndarray, nibi, fbase, min_n: int) -> list:
    """Per-file IBI arrays from the packed values (file i's start at fbase[i]); None under min_n."""
    return [vals[fbase[i]:fbase[i] + nibi[i]].copy() if nibi[i] >= min_n else None for i in range(len(nibi))]


def _ptr(x):
    return None if x is None else x.data_ptr()


def _stream(eng, ws, stream) -> int:
    """The raw stream of a launch that uses ``ws``: the current one, or ``stream`` with ws recorded on it."""
    if stream is None:
        return eng.stream()
    ws.record_stream(stream)
    return stream.cuda_stream


def window_stage(eng, buf, win_off, n_win: int, win_n: int, hop: int, sr: int, *, energy=None, tuning=None,
                 ws_tag: str = "win"):
    """Energy, onset envelope and tempogram mean of n_win windows of win_n samples at win_off
    -> (onset [n_win T] f32, tg [n_win acw] f64, T, acw).  ``energy=None``: the STFT skips its
    per-frame energies (the silence trim's block sums supply them).  ``tuning`` = (win_chunk, tf_base,
    tp, peak_pitch, peak_mag, npk, ev_stft): the windows' leading frames also give their chunks'
    tuning peaks, and ev_stft is recorded after the STFT."""
    T, acw = frames_of(win_n, hop), tempogram_window(sr, hop)
    onset = torch.empty(n_win * T, dtype=torch.float32, device=eng.dev)
    tg = torch.empty(n_win * acw, dtype=torch.float64, device=eng.dev)
    ws = eng.workspace(ws_tag, eng.ctx.lib.nc_window_stage_workspace_bytes(eng.ctx.h, n_win, win_n, hop))
    head = (buf.data_ptr(), win_off.data_ptr(), None, n_win, win_n, hop, onset.data_ptr(), tg.data_ptr(), _ptr(energy))
    if tuning is None:
        eng.call("nc_window_stage", *head, ws.data_ptr(), ws.numel(), eng.stream())
    else:
        win_chunk, tf_base, tp, peak_pitch, peak_mag, npk, ev_stft = tuning
        eng.call("nc_window_stage_tuning", *head, win_chunk.data_ptr(), tf_base.data_ptr(), tp, peak_pitch.data_ptr(),
                 peak_mag.data_ptr(), npk.data_ptr(), ev_stft.cuda_event, ws.data_ptr(), ws.numel(), eng.stream())
    return onset, tg, T, acw


def tempo_beats(eng, onset, off, length, n: int, max_len: int, tg, acw: int, start, hop: int, *, prior_idx=None,
                active=None, out=None, beats=None, total: int = 0, ws_tag: str = "beats", st=None):
    """beat_track of n onset sequences (sequence i: length[i] <= max_len frames at off[i], start
    bpm start[prior_idx[i]] or start[i], skipped where active[i] is 0) -> (bpm, lag, nbeats, margin):
    ``out``, or zero-filled tensors.  ``total``: the frames of ``onset``, and with them a global workspace; 0
    (none) only where engine.beat_needs_workspace allows.  ``beats`` (needs ``total``): the beat frames, at ``off``."""
    if out is None:
        out = tuple(torch.zeros(n, dtype=dt, device=eng.dev)
                    for dt in (torch.float64, torch.int32, torch.int32, torch.float64))
    bpm, lag, nbeats, margin = out
    ws = eng.workspace(ws_tag, eng.ctx.lib.nc_tempo_beats_workspace_bytes(total)) if total else None
    trim = 1                                            # beats after trimming, as beat_track(trim=True)
    eng.call("nc_tempo_beats", onset.data_ptr(), off.data_ptr(), length.data_ptr(), n, max_len, tg.data_ptr(), acw,
             start.data_ptr(), _ptr(prior_idx), _ptr(active), hop, trim, bpm.data_ptr(), lag.data_ptr(),
             nbeats.data_ptr(), margin.data_ptr(), _ptr(beats), total, _ptr(ws), ws.numel() if total else 0,
             eng.stream() if st is None else st)
    return out


def beats_to_ibis(eng, onset, fbase, lens, n: int, max_len: int, tg, acw: int, start, pidx, hop: int, min_ibis: int,
                  total: int, ws_tag: str, st=None) -> dict:
    """beat_track -> IBIs of n files whose onsets (``total`` frames) are packed at ``fbase``
    (tempo.py:158-172) -> bpm, lag, nbeats, margin, beats, ibis (packed at fbase), nibi."""
    st = eng.stream() if st is None else st
    beats = torch.empty(max(1, total), dtype=torch.int32, device=eng.dev)
    bpm, lag, nb, mg = tempo_beats(eng, onset, fbase, lens, n, max_len, tg, acw, start, hop, prior_idx=pidx,
                                   beats=beats, total=total, ws_tag=ws_tag, st=st)
    ibis = torch.empty(max(1, total), dtype=torch.float64, device=eng.dev)
    nibi = torch.zeros(n, dtype=torch.int32, device=eng.dev)
    eng.call("nc_ibi_from_beats", beats.data_ptr(), fbase.data_ptr(), nb.data_ptr(), n, hop, min_ibis,
             ibis.data_ptr(), nibi.data_ptr(), st)
    return dict(bpm=bpm, lag=lag, nbeats=nb, margin=mg, beats=beats, ibis=ibis, nibi=nibi)


def chroma_mean(eng, buf, off, length, n: int, total: int, max_len: int, *, chroma=None, tuning=None, tmargin=None,
                shared=None, ws_tag: str = "chroma", stream=None):
    """Mean CQT chroma and tuning of n chunks (``total`` samples, the longest max_len) -> (chroma
    [n 12] f32, tuning [n] f32, tmargin).  ``tmargin`` (the tuning decisions' count margins, int32 [n])
    is optional: None asks for none.  ``shared`` = (tf_skip, n_shared, peak_pitch, peak_mag, npk,
    ev_stft): the chunks' leading tuning frames come from the window stage's peak lists, complete at ev_stft."""
    chroma = torch.empty(n * 12, dtype=torch.float32, device=eng.dev) if chroma is None else chroma
    tuning = torch.empty(n, dtype=torch.float32, device=eng.dev) if tuning is None else tuning
    ws = eng.workspace(ws_tag, eng.ctx.lib.nc_chroma_workspace_bytes(eng.ctx.h, n, total))
    st = _stream(eng, ws, stream)
    head = (buf.data_ptr(), off.data_ptr(), length.data_ptr(), n, total, max_len, chroma.data_ptr(),
            tuning.data_ptr(), None, _ptr(tmargin))
    if shared is None:
        eng.call("nc_chroma_mean", *head, ws.data_ptr(), ws.numel(), st)
    else:
        tf_skip, n_shared, peak_pitch, peak_mag, npk, ev_stft = shared
        eng.call("nc_chroma_mean_shared", *head, tf_skip.data_ptr(), n_shared, peak_pitch.data_ptr(),
                 peak_mag.data_ptr(), npk.data_ptr(), ev_stft.cuda_event, ws.data_ptr(), ws.numel(), st)
    return chroma, tuning, tmargin


def chroma_lag_margin(eng, chroma, src_idx, nc_idx, n_pairs: int, *, lag=None, margin=None, stream=None):
    """Cyclic cross-correlation peak of n_pairs (src, nc) chroma rows -> (lag int32, the decision's relative margin f64)."""
    lag = torch.empty(n_pairs, dtype=torch.int32, device=eng.dev) if lag is None else lag
    margin = torch.empty(n_pairs, dtype=torch.float64, device=eng.dev) if margin is None else margin
    eng.call("nc_chroma_lag_margin", chroma.data_ptr(), src_idx.data_ptr(), nc_idx.data_ptr(), n_pairs,
             lag.data_ptr(), margin.data_ptr(), eng.stream() if stream is None else stream.cuda_stream)
    return lag, margin


def bootstrap_ratio(eng, vals, a_off, a_n, b_off, b_n, n_jobs: int, seed, pct, min_n: int, out, wsoff, cap,
                    ws_tag: str, ws_bytes: int, *, n_boot: int = C.N_BOOTSTRAP, stream=None) -> None:
    """n_jobs bootstraps of median(A) / median(B) (of median(A) with b_off = b_n = None) over samples
    of ``vals`` -> ``out`` (3 n_jobs doubles): the points, then the intervals' low and high ends.
    ``pct``: engine.percentile_params; a job with fewer than min_n values on a side gives NaN; job j's
    scratch is cap[j] values at byte wsoff[j] of the workspace (ws_bytes: engine._job_offsets)."""
    ws = eng.workspace(ws_tag, ws_bytes)
    p = out.data_ptr()
    eng.call("nc_bootstrap_ratio", vals.data_ptr(), a_off.data_ptr(), a_n.data_ptr(), _ptr(b_off), _ptr(b_n), n_jobs,
             n_boot, seed.data_ptr(), *pct, min_n, p, p + 8 * n_jobs, p + 16 * n_jobs, None, wsoff.data_ptr(),
             cap.data_ptr(), ws.data_ptr(), ws.numel(), _stream(eng, ws, stream))
