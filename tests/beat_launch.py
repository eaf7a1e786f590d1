"""Direct launches of nc_tempo_beats for the GPU tests: per-sequence off / len, acw, hop, trim,
active, prior_idx and the workspace.  Every output buffer is pre-filled with a sentinel, and the
helper itself asserts that the kernel wrote nothing outside what it reports."""
from collections import namedtuple

import numpy as np
import torch

from nightcore_analyzer import _dev

BeatOut = namedtuple("BeatOut", "bpm lag nbeats margin beats")

GAP_FILL = 3.25        # onset samples between sequences: non-zero, so a stray read changes results
NO_BEAT = -12345


def run_beats(ctx, onsets, tg, start_bpm, *, hop=512, trim=1, offs=None, active=None, prior_idx=None,
              max_len=None, workspace=True):
    """onsets: list of 1-D float32 arrays (sequence s at offs[s], default packed back to back);
    tg: (n, acw) float64; start_bpm: per sequence, or per prior when prior_idx is given.
    Returns BeatOut with beats as a list of int arrays (nbeats <= 0 -> empty)."""
    dev = _dev.device(0)
    n = len(onsets)
    lens = np.array([len(o) for o in onsets], np.int32)
    if offs is None:
        offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    offs = np.asarray(offs, np.int64)
    total = int(np.max(offs + lens))
    buf = np.full(total, GAP_FILL, np.float32)
    for o, x in zip(offs, onsets):
        buf[o:o + len(x)] = x
    tg = np.ascontiguousarray(tg, np.float64)
    assert tg.shape[0] == n
    acw = tg.shape[1]
    max_len = int(lens.max()) if max_len is None else max_len
    d_on = _dev.to_dev(buf, dev)
    d_tg = _dev.to_dev(tg.reshape(-1), dev)
    d_off = _dev.to_dev(offs, dev)
    d_len = _dev.to_dev(lens, dev)
    d_sb = _dev.to_dev(np.asarray(start_bpm, np.float64), dev)
    d_pi = None if prior_idx is None else _dev.to_dev(np.asarray(prior_idx, np.int32), dev)
    d_act = None if active is None else _dev.to_dev(np.asarray(active, np.uint8), dev)
    bpm = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    mg = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    lag = torch.full((n,), NO_BEAT, dtype=torch.int32, device=dev)
    nb = torch.full((n,), NO_BEAT, dtype=torch.int32, device=dev)
    beats = torch.full((total,), NO_BEAT, dtype=torch.int32, device=dev)
    wsb = ctx.lib.nc_tempo_beats_workspace_bytes(total) if workspace else 0
    ws = _dev.workspace(wsb, dev) if workspace else None
    ctx.call("nc_tempo_beats", d_on.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, max_len, d_tg.data_ptr(),
             acw, d_sb.data_ptr(), _dev.ptr(d_pi), _dev.ptr(d_act), hop, int(trim), bpm.data_ptr(), lag.data_ptr(),
             nb.data_ptr(), mg.data_ptr(), beats.data_ptr(), total, _dev.ptr(ws), wsb, _dev.stream_handle())
    torch.cuda.synchronize()
    b = beats.cpu().numpy()
    nbv = nb.cpu().numpy()
    assert np.all(nbv != NO_BEAT), "nbeats not written for every sequence"
    assert np.all(nbv <= lens), (nbv, lens)
    written = np.zeros(total, bool)
    out = []
    for s in range(n):
        k = max(0, int(nbv[s]))
        written[offs[s]:offs[s] + k] = True
        out.append(b[offs[s]:offs[s] + k].copy())
    assert np.all(b[~written] == NO_BEAT), "beats written outside [off, off + nbeats)"
    assert np.all(b[written] != NO_BEAT), "reported beats not written"
    return BeatOut(bpm.cpu().numpy(), lag.cpu().numpy(), nbv, mg.cpu().numpy(), out)
