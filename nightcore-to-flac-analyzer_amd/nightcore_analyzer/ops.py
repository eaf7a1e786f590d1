"""Device operations behind the reference's module-level functions (io / tempo /
pitch / xcorr), for callers that use those functions directly instead of
``pipeline.run`` (the reference's workflow does: workflow.py:617, 678, 797).
Every function uploads its arrays once and runs libncgpu kernels; results come
back in the reference's Python types.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native, launch
from .engine import _ALIGN, SR, DeviceSignals, Engine, Params, _Upload, h2d

HOP = 512


def _signals(eng: Engine, src, f32: bool = True) -> DeviceSignals:
    """``src`` if it is a ``DeviceSignals`` (already in HBM), else its arrays uploaded (``f32``: cast first)."""
    if isinstance(src, DeviceSignals):
        return src
    return eng.upload_signals([np.asarray(a, np.float32) for a in src] if f32 else list(src))


def _packed(lengths: np.ndarray) -> Tuple[np.ndarray, int]:
    """(offsets, total) of outputs of these lengths back to back, each on a 64-sample boundary."""
    pad = (lengths + _ALIGN - 1) // _ALIGN * _ALIGN
    off = np.zeros(len(lengths), np.int64)
    off[1:] = np.cumsum(pad)[:-1]
    return off, int(pad.sum())


def _read_back(buf: torch.Tensor, off, length) -> List[np.ndarray]:
    """The files of a device buffer as host arrays (one blocking copy of the buffer)."""
    h = buf.cpu().numpy()
    return [h[o:o + n].copy() for o, n in zip(off, length)]


def trim_bounds(eng: Engine, audios: Sequence[np.ndarray], top_db: float) -> List[Tuple[int, int]]:
    """librosa.effects.trim bounds (io.py:76) for each array."""
    sig = eng.upload_signals(audios)
    start, end = eng._trim_launch(sig, 0, sig.n_files, Params(silence_strip_db=top_db),
                                  torch.cuda.current_stream(eng.dev), pinned=False).bounds()
    return list(zip(start.tolist(), end.tolist()))


def window_energies(eng: Engine, audio: np.ndarray, starts: np.ndarray, win_len: int) -> np.ndarray:
    """io._rms_db (io.py:38-40) of audio[s:s+win_len] for every start."""
    if len(starts) == 0:
        return np.zeros(0)
    sig = eng.upload_signals([audio])
    off = torch.tensor(np.asarray(starts, np.int64) + sig.off[0], device=eng.dev)
    out = torch.empty(len(starts), dtype=torch.float64, device=eng.dev)
    eng.call("nc_window_energy", sig.buf.data_ptr(), off.data_ptr(), len(starts), int(win_len), out.data_ptr(),
             eng.stream())
    return out.cpu().numpy()


def window_tempos(eng: Engine, audios: Sequence[np.ndarray], start_bpms: Sequence[float],
                  details: Optional[list] = None) -> List[Optional[float]]:
    """tempo.estimate_tempo (tempo.py:27-77) for each window array."""
    res: List[Optional[float]] = [None] * len(audios)
    by_len: dict = {}
    for i, a in enumerate(audios):
        by_len.setdefault(len(a), []).append(i)
    for L, idx in by_len.items():
        if L == 0:
            continue
        n = len(idx)
        T = launch.frames_of(L, HOP)
        sig = eng.upload_signals([audios[i] for i in idx])
        up = _Upload()
        up.add("off", sig.off, np.int64)
        up.add("on_off", np.arange(n, dtype=np.int64) * T, np.int64)
        up.add("on_len", np.full(n, T), np.int32)
        up.add("start", [start_bpms[i] for i in idx], np.float64)
        d = up.commit(eng.dev)
        en = torch.empty(n, dtype=torch.float64, device=eng.dev)
        # the tempogram window of the engine's rate
        onset, tg, T, acw = launch.window_stage(eng, sig.buf, d["off"], n, L, HOP, eng.sr, energy=en)
        bpm, lag, nb, mg = launch.tempo_beats(eng, onset, d["on_off"], d["on_len"], n, T, tg, acw, d["start"], HOP,
                                              total=n * T)
        b_h, n_h = bpm.cpu().numpy(), nb.cpu().numpy()
        for k, i in enumerate(idx):
            res[i] = float(b_h[k]) if n_h[k] >= 4 else None
        if details is not None:
            details.append(dict(idx=idx, lag=lag.cpu().numpy(), nbeats=n_h, margin=mg.cpu().numpy()))
    return res


def ibis(eng: Engine, ys: Sequence[np.ndarray], start_bpms: Sequence[float], hop: int = 64,
         min_ibis: int = 4) -> List[Optional[np.ndarray]]:
    """tempo.estimate_ibis_global (tempo.py:120-173) for each signal."""
    sig = eng.upload_signals(ys)
    up = _Upload()
    up.add("off", sig.off, np.int64)
    up.add("len", sig.length, np.int64)
    up.add("start", list(start_bpms), np.float64)
    d = up.commit(eng.dev)
    core = eng.ibi_core(sig.buf, d["off"], d["len"], sig.length, d["start"],
                        torch.arange(len(ys), dtype=torch.int32, device=eng.dev), hop=hop, min_ibis=min_ibis)
    return launch.ibi_lists(core["ibis"].cpu().numpy(), core["nibi"].cpu().numpy(), core["fbase_h"], 1)


def chroma_means(eng: Engine, audios: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray, torch.Tensor]:
    """pitch._mean_chroma (pitch.py:55-64) of each array -> ([n,12] f32, tuning[n], device chroma)."""
    sig = eng.upload_signals(audios)
    n = sig.n_files
    up = _Upload()
    up.add("off", sig.off, np.int64)
    up.add("len", sig.length, np.int64)
    d = up.commit(eng.dev)
    out, tun, _ = launch.chroma_mean(eng, sig.buf, d["off"], d["len"], n, int(sig.length.sum()), int(sig.length.max()))
    return out.cpu().numpy().reshape(n, 12), tun.cpu().numpy(), out


def chroma_lags(eng: Engine, chroma_dev: torch.Tensor, src_idx: Sequence[int], nc_idx: Sequence[int]) -> List[int]:
    """pitch._cyclic_xcorr_peak (pitch.py:67-85) for each (src, nc) chroma row pair."""
    n = len(src_idx)
    si = torch.tensor(list(src_idx), dtype=torch.int32, device=eng.dev)
    ni = torch.tensor(list(nc_idx), dtype=torch.int32, device=eng.dev)
    lag = torch.empty(max(1, n), dtype=torch.int32, device=eng.dev)
    eng.call("nc_chroma_lag", chroma_dev.data_ptr(), si.data_ptr(), ni.data_ptr(), n, lag.data_ptr(), eng.stream())
    return lag.cpu().numpy()[:n].astype(int).tolist()


def xcorr_peaks(eng: Engine, src: np.ndarray, nc: np.ndarray) -> List[int]:
    """pitch._cyclic_xcorr_peak (pitch.py:67-85) for rows of [pairs, n] (any n >= 1)."""
    a = np.ascontiguousarray(src, np.float32)
    b = np.ascontiguousarray(nc, np.float32)
    n_pairs, n = a.shape
    d = torch.from_numpy(np.concatenate([a.reshape(-1), b.reshape(-1)])).to(eng.dev)
    lag = torch.empty(max(1, n_pairs), dtype=torch.int32, device=eng.dev)
    eng.call("nc_xcorr_peak", d[:a.size].data_ptr(), d[a.size:].data_ptr(), n, n_pairs, lag.data_ptr(), eng.stream())
    return lag.cpu().numpy()[:n_pairs].astype(int).tolist()


def xcorr_geometry(len_a: int, len_b: int, win: int, search: int, stride: int, n_windows: int):
    """The integer geometry of xcorr.estimate_speed_xcorr's search (xcorr.py:109-125) on the
    edge-trimmed lengths: [(pa, exp_pb, [candidate pb ...])] for every window with lo < hi."""
    out = []
    for pa in np.linspace(0, len_a - win, n_windows).astype(int):
        pa = int(pa)
        exp_pb = int(pa * len_b / len_a)
        lo, hi = max(0, exp_pb - search), min(len_b - win, exp_pb + search)
        if lo >= hi:
            continue
        out.append((pa, exp_pb, list(range(lo, hi, stride))))
    return out


def xcorr_speed(eng: Engine, ya: np.ndarray, yb: np.ndarray, sr: int = SR, n_windows: int = 20,
                window_sec: float = 3.0, search_range: float = 0.05,
                skip_edges: float = 0.10) -> Tuple[float, float]:
    """The search of xcorr.estimate_speed_xcorr (xcorr.py:95-162) on decoded arrays."""
    min_len = min(len(ya), len(yb))
    s, e = int(min_len * skip_edges), int(min_len * (1.0 - skip_edges))
    ya, yb = np.asarray(ya, np.float32)[s:e], np.asarray(yb, np.float32)[s:e]
    win = int(window_sec * sr)
    search = int(search_range * len(yb))
    stride = max(1, win // 4)
    if len(ya) < win or len(yb) < win:
        return 1.0, 0.0
    sig = eng.upload_signals([ya, yb])
    oa, ob = int(sig.off[0]), int(sig.off[1])
    ia, ib, sw, c0, c1, pa_l, pb_l, exp_l = [], [], [], [], [], [], [], []
    for pa, exp_pb, cands in xcorr_geometry(len(ya), len(yb), win, search, stride, n_windows):
        sw.append(len(ia))
        ia.append(oa + pa)
        ib.append(oa + pa)
        pb_l.append(pa)
        c0.append(len(ia))
        for pb in cands:
            ia.append(oa + pa)
            ib.append(ob + pb)
            pb_l.append(pb)
        c1.append(len(ia))
        pa_l.append(pa)
        exp_l.append(exp_pb)
    nw = len(sw)
    if nw == 0:
        return 1.0, 0.0
    up = _Upload()
    up.add("ia", ia, np.int64)
    up.add("ib", ib, np.int64)
    up.add("w0", [0], np.int32)
    up.add("w1", [nw], np.int32)
    up.add("sw", sw, np.int32)
    up.add("c0", c0, np.int32)
    up.add("c1", c1, np.int32)
    up.add("pa", pa_l, np.int64)
    up.add("pb", pb_l, np.int64)
    up.add("exp", exp_l, np.int64)
    d = up.commit(eng.dev)
    n_items = len(ia)
    scratch = torch.empty(2 * n_items + 2, dtype=torch.float64, device=eng.dev)
    out = torch.empty(2, dtype=torch.float64, device=eng.dev)
    eng.call("nc_xcorr_search", sig.buf.data_ptr(), d["ia"].data_ptr(), d["ib"].data_ptr(), n_items, win,
             scratch[:n_items].data_ptr(), scratch[n_items:2 * n_items].data_ptr(), d["w0"].data_ptr(),
             d["w1"].data_ptr(), d["sw"].data_ptr(), d["c0"].data_ptr(), d["c1"].data_ptr(), d["pa"].data_ptr(),
             d["pb"].data_ptr(), d["exp"].data_ptr(), 1, out[0:1].data_ptr(), out[1:2].data_ptr(), eng.stream())
    o = out.cpu().numpy()
    return float(o[0]), float(o[1])


def shift_bootstrap(eng: Engine, shifts: np.ndarray) -> Tuple[float, float]:
    """pitch.py:143-150: CI of the median chunk shift, rng = default_rng(0)."""
    (_, ci), = eng.bootstrap([(np.asarray(shifts, np.float64), None)], seed=0)
    return ci


# ------------------------------------------------------------------ load-time resampler
def poly_plan(up: int, down: int, max_in: int):
    """scipy.signal.resample_poly's filter and offsets for ratio up/down (reduced), sized for
    inputs up to max_in samples: (up, down, h padded to a multiple of up (f64), pre_remove).
    Trailing zero taps beyond what a shorter input needs leave every sum unchanged."""
    from scipy.signal import firwin
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    n_pre_pad = down - half_len % down
    pre_remove = (half_len + n_pre_pad) // down
    n_out = -(-max_in * up // down)

    def out_len(len_h, n_in):        # scipy.signal._upfirdn_apply._output_len
        n = n_in + (len_h + (-len_h % up)) // up - 1
        return -(-n * up // down)
    post = 0
    while out_len(len(h) + n_pre_pad + post, max_in) < n_out + pre_remove:
        post += 1
    h = np.concatenate([np.zeros(n_pre_pad), h, np.zeros(post)])
    h = np.concatenate([h, np.zeros(-len(h) % up)])
    return up, down, h, pre_remove


def resample_poly(eng: Engine, arrays: Sequence[np.ndarray], up: int, down: int) -> List[np.ndarray]:
    """float32(scipy.signal.resample_poly(float64(x), up, down)) for each array, on the GPU
    (nc_resample_poly; bit-identical to scipy).  The load-time resampler of io.load_audio."""
    arrays = [np.asarray(a, np.float32) for a in arrays]
    if not arrays:
        return []
    if int(up) == int(down):
        return [a.copy() for a in arrays]
    out = resample_poly_device(eng, eng.upload_signals(arrays), up, down)
    return _read_back(out.buf, out.off, out.length)


def resample_poly_device(eng: Engine, sig, up: int, down: int):
    """``resample_poly`` of signals already in HBM (``DeviceSignals``), the result left there
    (``DeviceSignals``, files back to back): the same launch, no host round trip and no
    synchronisation.  A 1:1 ratio returns ``sig`` itself."""
    n = sig.n_files
    lens = np.asarray(sig.length, np.int64)
    if n == 0 or int(up) == int(down):
        return sig
    up, down, h, pre = poly_plan(up, down, int(lens.max()))
    n_out = -(-lens * up // down)
    o_off = np.zeros(n, np.int64)
    o_off[1:] = np.cumsum(n_out)[:-1]
    up_ = _Upload()
    up_.add("in_off", sig.off, np.int64)
    up_.add("in_len", lens, np.int64)
    up_.add("out_off", o_off, np.int64)
    up_.add("out_len", n_out, np.int64)
    up_.add("h", h, np.float64)
    d = up_.commit(eng.dev)
    y = torch.empty(max(1, int(n_out.sum())), dtype=torch.float32, device=eng.dev)
    eng.call("nc_resample_poly", sig.buf.data_ptr(), d["in_off"].data_ptr(), d["in_len"].data_ptr(), n,
             y.data_ptr(), d["out_off"].data_ptr(), d["out_len"].data_ptr(), int(n_out.max()), d["h"].data_ptr(),
             len(h), up, down, pre, eng.stream())
    return DeviceSignals(y, o_off, n_out)


# ------------------------------------------------------------------ FLAC decode (nc_flac_index.cpp + flac.hip)
FLAC_STATUS = {1: "CRC-16 mismatch", 2: "bitstream ran past the frame's end", 3: "reserved or invalid field",
               4: "decoded length differs from the block size"}


def flac_index(data, name: str = "FLAC data"):
    """(info dict, int64 frame table [n, 8]) of one FLAC stream's bytes, from the library's host
    walk ``nc_flac_index`` (needs no device).  info: rate, channels, bps, total (samples per
    channel), md5 (STREAMINFO's 16 bytes).  The table's columns: byte start, byte end, first
    sample, block size, channel assignment, bits per sample, header bytes, 0.  ValueError
    (named after ``name``) for anything that is not a stream the decoder takes."""
    lib = _native.load()
    buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
    n_bytes = len(data)
    info, md5, n = np.zeros(8, np.int64), np.zeros(16, np.uint8), C.c_int64(0)

    def call(rows, cap):
        rc = lib.nc_flac_index(buf.ctypes.data, n_bytes, info.ctypes.data, md5.ctypes.data,
                               rows.ctypes.data if rows is not None else None, cap, C.byref(n))
        if rc != 0 and not (rc == -3 and rows is not None and cap < n.value):
            msg = lib.nc_last_error()
            raise ValueError(f"{name}: {msg.decode() if msg else rc}")
        return rc
    cap = max(1024, n_bytes // 256)          # one walk for frames of 256 bytes and more, else a second
    rows = np.zeros((cap, 8), np.int64)
    if call(rows, cap) == -3:
        rows = np.zeros((n.value, 8), np.int64)
        call(rows, n.value)
    return (dict(rate=int(info[0]), channels=int(info[1]), bps=int(info[2]), total=int(info[3]), md5=md5.tobytes()),
            rows[:n.value])


def flac_decode_device(eng: Engine, blobs: Sequence[bytes], *, names: Optional[Sequence[str]] = None,
                       mono: bool = False, verify_md5: bool = False):
    """Decode the FLAC streams ``blobs`` (the files' bytes) in one upload and one launch
    (``nc_flac_decode``, one wave per frame): (DeviceSignals, infos).  The DeviceSignals holds
    every channel of every file as float32 sample / 2^(bps-1) (exact; ``_read_wav``'s scaling),
    file by file, channel by channel; infos[f] is the index's info dict plus ``first`` (the
    file's first entry in the DeviceSignals), ``pcm`` (the file's device int32 samples
    [channels, total]) and, with ``mono`` and one or two channels, ``mono`` (the device float32
    mix f32(a + b) 0.5, what ``x.reshape(-1, ch).mean(axis=1)`` gives).  A frame whose status
    is not 0 raises ValueError naming the file, the frame and the reason (this reads the
    status words back: the one synchronisation).  ``verify_md5`` also downloads the samples
    and compares their MD5 with STREAMINFO's (skipped when that is all zeros)."""
    names = [f"FLAC stream {i}" for i in range(len(blobs))] if names is None else [str(n) for n in names]
    infos, tables, chunks = [], [], []
    files = np.zeros((max(1, len(blobs)), 8), np.int64)
    off, length = [], []
    byte_pos = pcm_len = mono_len = 0
    for f, blob in enumerate(blobs):
        info, rows = flac_index(blob, names[f])
        rows = rows.copy()
        rows[:, 0:2] += byte_pos
        rows[:, 7] = f
        if len(rows) and not np.all(rows[:, 5] == info["bps"]):
            raise ValueError(f"{names[f]}: the sample size changes inside the stream (unsupported)")
        tables.append(rows)
        chunks.append((byte_pos, blob))
        byte_pos += (len(blob) + 3) // 4 * 4
        ch, total = info["channels"], info["total"]
        stride = (total + _ALIGN - 1) // _ALIGN * _ALIGN
        want_mono = mono and ch <= 2
        files[f] = (pcm_len, stride, ch, info["bps"], total, mono_len if want_mono else -1, 0, 0)
        info.update(first=len(off), _out=pcm_len, _stride=stride, _mono=mono_len if want_mono else -1)
        off += [pcm_len + c * stride for c in range(ch)]
        length += [total] * ch
        pcm_len += ch * stride
        if want_mono:
            mono_len += stride
        infos.append(info)
    frames = np.concatenate(tables) if tables else np.zeros((0, 8), np.int64)
    host = torch.zeros(byte_pos + 16, dtype=torch.uint8, pin_memory=True)    # 8 bytes of padding and more
    hv = host.numpy()
    for pos, blob in chunks:
        hv[pos:pos + len(blob)] = np.frombuffer(blob, np.uint8)
    data = host.to(eng.dev, non_blocking=True)
    up = _Upload()
    up.add("frames", frames if len(frames) else np.zeros(8), np.int64)
    up.add("files", files, np.int64)
    d = up.commit(eng.dev)
    pcm = torch.zeros(max(_ALIGN, pcm_len), dtype=torch.int32, device=eng.dev)
    f32 = torch.zeros(max(_ALIGN, pcm_len), dtype=torch.float32, device=eng.dev)
    mix = torch.zeros(max(_ALIGN, mono_len), dtype=torch.float32, device=eng.dev) if mono else None
    status = torch.zeros(max(1, len(frames)), dtype=torch.int32, device=eng.dev)
    if len(frames):
        eng.call("nc_flac_decode", data.data_ptr(), data.numel(), d["frames"].data_ptr(), len(frames),
                 d["files"].data_ptr(), len(blobs), pcm.data_ptr(), f32.data_ptr(), pcm_len,
                 mix.data_ptr() if mix is not None else None, mono_len, status.data_ptr(), eng.stream())
        bad = np.flatnonzero(status.cpu().numpy()[:len(frames)])
        if len(bad):
            g = int(bad[0])
            f = int(frames[g, 7])
            k = g - sum(len(t) for t in tables[:f])
            code = int(status[g].item())
            raise ValueError(f"{names[f]}: frame {k} (samples {int(frames[g, 2])} .. "
                             f"{int(frames[g, 2] + frames[g, 3])}): {FLAC_STATUS.get(code, code)}")
    for f, info in enumerate(infos):
        o, s, ch, total = info.pop("_out"), info.pop("_stride"), info["channels"], info["total"]
        info["pcm"] = pcm[o:o + ch * s].view(ch, s)[:, :total]
        m = info.pop("_mono")
        info["mono"] = mix[m:m + total] if m >= 0 else None
        if verify_md5 and info["md5"] != bytes(16):
            import hashlib
            width = (info["bps"] + 7) // 8
            inter = np.ascontiguousarray(info["pcm"].cpu().numpy().T).astype("<i4")
            got = hashlib.md5(inter.view(np.uint8).reshape(-1, 4)[:, :width].tobytes()).digest()
            if got != info["md5"]:
                raise ValueError(f"{names[f]}: MD5 of the decoded samples {got.hex()} differs from STREAMINFO's "
                                 f"{info['md5'].hex()}")
    return DeviceSignals(f32, np.asarray(off, np.int64), np.asarray(length, np.int64)), infos


def flac_decode(eng: Engine, blobs: Sequence[bytes], **kw) -> List[Tuple[np.ndarray, dict]]:
    """[(int32 samples [channels, total], info)] of each stream, on the host (``flac_decode_device``)."""
    _, infos = flac_decode_device(eng, blobs, **kw)
    out = []
    for info in infos:
        info = dict(info)
        pcm = info.pop("pcm").cpu().numpy()
        info["mono"] = None if info["mono"] is None else info["mono"].cpu().numpy()
        out.append((pcm, info))
    return out


# ------------------------------------------------------------------ FLAC encode (flac_enc.hip)
FLAC_ENC_STATUS = {1: "table row outside the buffers or the format's limits", 2: "sample outside the sample size"}
FLAC_SUBFRAME_TYPES = ("constant", "verbatim", "fixed", "lpc")


def flac_slot_bytes(channels: int, block: int, bits: int) -> int:
    """Bytes of one frame's slot: the all-VERBATIM bound ``nc_flac_encode`` documents."""
    return (16 + (channels * (8 + block * (bits + 1)) + 7) // 8 + 2 + 3) // 4 * 4


def _per_stream(value, n: int, what: str) -> List[int]:
    vals = [int(value)] * n if isinstance(value, (int, np.integer)) else [int(v) for v in value]
    if len(vals) != n:
        raise ValueError(f"flac_encode: one {what} per stream is needed")
    return vals


def flac_encode_device(eng: Engine, src: DeviceSignals, streams, bits, rate, block: int = 4096, level: int = 1,
                       names: Optional[Sequence[str]] = None):
    """Encode streams resident in HBM as FLAC frames in one ``nc_flac_encode`` launch (one wave
    per frame) and one ``nc_flac_pack``: (frame bytes per stream, info dict per stream).

    ``src``: a ``DeviceSignals`` whose buffer is float32 (quantised by the kernel:
    clamp(rint(x 2^(bits-1))), round half to even, ``nc_f32_to_pcm16``'s rule) or int32 (samples
    already inside ``bits``).  ``streams``: the channel count of every stream (an int for all);
    stream s is that many consecutive, equally long, equally spaced signals of ``src``.  ``bits``
    (4-24) and ``rate`` (1 .. 2^20 - 1): an int for all streams or one per stream.  ``block``:
    16 .. 16384, the fixed block size; ``level`` 0 (CONSTANT / VERBATIM / FIXED) or 1 (plus LPC
    1-8; never longer than level 0).  info: ``frame_bytes`` (int32 per frame), ``min_frame`` /
    ``max_frame``, ``clipped`` (samples clamped by the quantiser), ``records`` (int32 [frames, 25]:
    assignment, then type / order / partition order per channel), ``pcm`` (the device int32
    samples [channels, total]), ``channels`` / ``bits`` / ``rate`` / ``total`` / ``block``.
    Only the packed bytes and the per-frame arrays are downloaded.  A frame whose status is not 0
    raises ValueError naming the stream and the frame."""
    n_sig = src.n_files
    chans = [int(streams)] * (n_sig // max(1, int(streams))) if isinstance(streams, (int, np.integer)) \
        else [int(c) for c in streams]
    n_streams = len(chans)
    if any(c < 1 or c > 8 for c in chans) or sum(chans) != n_sig:
        raise ValueError("flac_encode: every stream needs 1 .. 8 channels and the streams must use every signal")
    bits_s, rate_s = _per_stream(bits, n_streams, "sample size"), _per_stream(rate, n_streams, "sample rate")
    block, level = int(block), int(level)
    if not 16 <= block <= 16384:
        raise ValueError(f"flac_encode: block size {block} outside 16 .. 16384")
    if level not in (0, 1):
        raise ValueError(f"flac_encode: level {level} is not 0 or 1")
    for b, r in zip(bits_s, rate_s):
        if not 4 <= b <= 24:
            raise ValueError(f"flac_encode: {b} bits per sample outside 4 .. 24")
        if not 0 < r < 1 << 20:
            raise ValueError(f"flac_encode: sample rate {r} outside 1 .. 2^20 - 1")
    if src.buf.dtype not in (torch.float32, torch.int32):
        raise ValueError("flac_encode: the samples must be float32 or int32")
    names = [f"stream {i}" for i in range(n_streams)] if names is None else [str(n) for n in names]
    files = np.zeros((max(1, n_streams), 8), np.int64)
    rows, infos = [], []
    first_sig = slot_pos = 0
    for s, ch in enumerate(chans):
        off = np.asarray(src.off[first_sig:first_sig + ch], np.int64)
        lens = np.asarray(src.length[first_sig:first_sig + ch], np.int64)
        first_sig += ch
        total = int(lens[0])
        stride = int(off[1] - off[0]) if ch > 1 else max(total, 1)
        if np.any(lens != total) or (ch > 1 and (stride < total or np.any(np.diff(off) != stride))):
            raise ValueError(f"{names[s]}: the channels of a stream must be equally long and equally spaced")
        if total >= 1 << 36:
            raise ValueError(f"{names[s]}: {total} samples do not fit STREAMINFO")
        files[s] = (int(off[0]), stride, ch, bits_s[s], rate_s[s], total, 0, 0)
        n_fr = -(-total // block)
        need = flac_slot_bytes(ch, block, bits_s[s])
        t = np.zeros((n_fr, 8), np.int64)
        t[:, 0] = s
        t[:, 1] = np.arange(n_fr) * block
        t[:, 2] = np.minimum(block, total - t[:, 1])
        t[:, 3] = np.arange(n_fr)
        t[:, 4] = slot_pos + np.arange(n_fr) * need
        slot_pos += n_fr * need
        rows.append(t)
        infos.append(dict(channels=ch, bits=bits_s[s], rate=rate_s[s], total=total, block=block, _off=int(off[0]),
                          _stride=stride))
    frames = np.concatenate(rows) if rows else np.zeros((0, 8), np.int64)
    n_frames = len(frames)
    is_float = src.buf.dtype == torch.float32
    q = torch.empty(src.buf.numel(), dtype=torch.int32, device=eng.dev) if is_float else src.buf
    nf = max(1, n_frames)
    fb = torch.zeros(nf, dtype=torch.int32, device=eng.dev)
    rec = torch.zeros(nf * 25, dtype=torch.int32, device=eng.dev)
    clipped = torch.zeros(nf, dtype=torch.int32, device=eng.dev)
    status = torch.zeros(nf, dtype=torch.int32, device=eng.dev)
    packed_h = np.zeros(0, np.uint8)
    fb_h = cl_h = np.zeros(0, np.int32)
    rec_h = np.zeros((0, 25), np.int32)
    if n_frames:
        up = _Upload()
        up.add("frames", frames, np.int64)
        up.add("files", files, np.int64)
        d = up.commit(eng.dev)
        slots = torch.empty(slot_pos, dtype=torch.uint8, device=eng.dev)
        eng.call("nc_flac_encode", None if is_float else src.buf.data_ptr(), src.buf.data_ptr() if is_float else None,
                 q.data_ptr() if is_float else None, src.buf.numel(), d["frames"].data_ptr(), n_frames,
                 d["files"].data_ptr(), n_streams, level, slots.data_ptr(), slot_pos, fb.data_ptr(), rec.data_ptr(),
                 clipped.data_ptr(), status.data_ptr(), eng.stream())
        ends = torch.cumsum(fb, 0, dtype=torch.int64)
        offsets = ends - fb
        small = torch.cat([fb, status, clipped, rec]).cpu().numpy()      # the one synchronisation before the pack
        fb_h, st_h, cl_h, rec_h = small[:nf], small[nf:2 * nf], small[2 * nf:3 * nf], small[3 * nf:].reshape(nf, 25)
        bad = np.flatnonzero(st_h[:n_frames])
        if len(bad):
            g = int(bad[0])
            s = int(frames[g, 0])
            code = int(st_h[g])
            raise ValueError(f"{names[s]}: frame {int(frames[g, 3])} (samples {int(frames[g, 1])} .. "
                             f"{int(frames[g, 1] + frames[g, 2])}): {FLAC_ENC_STATUS.get(code, code)}")
        out_bytes = (int(fb_h.sum(dtype=np.int64)) + 3) // 4 * 4
        out = torch.empty(max(4, out_bytes), dtype=torch.uint8, device=eng.dev)
        eng.call("nc_flac_pack", slots.data_ptr(), slot_pos, d["frames"].data_ptr(), n_frames, fb.data_ptr(),
                 offsets.data_ptr(), out.data_ptr(), out_bytes, eng.stream())
        packed_h = out.cpu().numpy()
    blobs = []
    g = pos = 0
    for s, info in enumerate(infos):
        n_fr = len(rows[s])
        sizes = fb_h[g:g + n_fr] if n_fr else np.zeros(0, np.int32)
        n_bytes = int(sizes.sum(dtype=np.int64))
        blobs.append(packed_h[pos:pos + n_bytes].tobytes())
        o, stride, ch, total = info.pop("_off"), info.pop("_stride"), info["channels"], info["total"]
        info.update(frame_bytes=sizes.copy(), min_frame=int(sizes.min()) if n_fr else 0,
                    max_frame=int(sizes.max()) if n_fr else 0,
                    clipped=int(cl_h[g:g + n_fr].sum()) if n_fr else 0,
                    records=rec_h[g:g + n_fr].copy() if n_fr else np.zeros((0, 25), np.int32),
                    pcm=torch.as_strided(q, (ch, total), (stride, 1), o))
        g += n_fr
        pos += n_bytes
    return blobs, infos


def flac_encode(eng: Engine, arrays: Sequence[np.ndarray], bits, rate, block: int = 4096, level: int = 1):
    """[(frame bytes, info)] of integer arrays [channels, n] (or [n]), one stream each, by
    ``flac_encode_device``; ``info["pcm"]`` comes back as a host array."""
    arrs = [np.atleast_2d(np.asarray(a)) for a in arrays]
    for a in arrs:
        if a.dtype.kind not in "iu" or a.ndim != 2:
            raise ValueError("flac_encode: integer arrays [channels, n] are needed")
    off, length, pos = [], [], 0
    for a in arrs:
        stride = (a.shape[1] + _ALIGN - 1) // _ALIGN * _ALIGN
        off += [pos + c * stride for c in range(a.shape[0])]
        length += [a.shape[1]] * a.shape[0]
        pos += a.shape[0] * stride
    host = torch.zeros(max(_ALIGN, pos), dtype=torch.int32, pin_memory=True)
    hv = host.numpy()
    at = 0
    for a in arrs:
        if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
            raise ValueError("flac_encode: a sample does not fit 32 bits")
        for c in range(a.shape[0]):
            hv[off[at]:off[at] + a.shape[1]] = a[c]
            at += 1
    sig = DeviceSignals(host.to(eng.dev, non_blocking=True), np.asarray(off, np.int64), np.asarray(length, np.int64))
    blobs, infos = flac_encode_device(eng, sig, [a.shape[0] for a in arrs], bits, rate, block, level)
    out = []
    for blob, info in zip(blobs, infos):
        info = dict(info)
        info["pcm"] = info["pcm"].cpu().numpy()
        out.append((blob, info))
    return out


# ------------------------------------------------------------------ speed render (speed.hip)
def speed_plan(factor: float, lengths: Sequence[int]) -> Tuple[int, np.ndarray]:
    """(P, n_out[file]) of a speed render: P = round(factor 1e6), n_out = ceil(n 1e6 / P), from
    the library's own ``nc_speed_out_len`` (the formula the kernel uses).  Needs no device."""
    lib = _native.load()
    n_in = np.ascontiguousarray(lengths, np.int64).reshape(-1)
    n_out = np.zeros(len(n_in), np.int64)
    p = C.c_int64(0)
    _native.check(lib.nc_speed_out_len(float(factor), n_in.ctypes.data, len(n_in), C.byref(p), n_out.ctypes.data),
                  "nc_speed_out_len")
    return int(p.value), n_out


def speed_render_device(eng: Engine, src, factor: float):
    """Every file of ``src`` (arrays, or ``DeviceSignals`` already in HBM) played ``factor`` times
    faster (the renderer's definition: DESIGN.md, include/ncgpu.h R2), one launch, the result
    left in HBM: (DeviceSignals of the renders, device float32 peak[file] = max |y|, P).  No
    host synchronisation."""
    sig = _signals(eng, src, f32=False)
    n = sig.n_files
    P, n_out = speed_plan(factor, sig.length)
    o_off, total = _packed(n_out)
    up = _Upload()
    up.add("in_off", sig.off, np.int64)
    up.add("in_len", sig.length, np.int64)
    up.add("out_off", o_off, np.int64)
    d = up.commit(eng.dev)
    y = torch.zeros(max(_ALIGN, total), dtype=torch.float32, device=eng.dev)
    peak = torch.empty(max(1, n), dtype=torch.float32, device=eng.dev)
    if n:
        eng.call("nc_speed_render", sig.buf.data_ptr(), d["in_off"].data_ptr(), d["in_len"].data_ptr(), n, P,
                 y.data_ptr(), d["out_off"].data_ptr(), int(n_out.max()), peak.data_ptr(), eng.stream())
    return DeviceSignals(y, o_off, n_out), peak[:n], P


def speed_render(eng: Engine, arrays: Sequence[np.ndarray], factor: float) -> Tuple[List[np.ndarray], np.ndarray]:
    """(renders, peaks): each array played ``factor`` times faster, and max |y| of each."""
    out, peak, _ = speed_render_device(eng, [np.asarray(a, np.float32) for a in arrays], factor)
    return _read_back(out.buf, out.off, out.length), peak.cpu().numpy()


def f32_to_pcm16_device(eng: Engine, sig, interleave: bool = False):
    """16-bit PCM of the files of ``sig`` (DeviceSignals) by ``nc_f32_to_pcm16``: (device int16
    buffer, offsets, device int32 clamped-sample counts).  ``interleave``: the files are the
    equally long channels of one WAV file and come out frame-interleaved."""
    n = sig.n_files
    lens = np.asarray(sig.length, np.int64)
    if interleave:
        if n and not np.all(lens == lens[0]):
            raise ValueError("interleaved channels must be equally long")
        o_off, stride, total = np.arange(n, dtype=np.int64), max(1, n), int(lens.sum())
    else:
        stride, (o_off, total) = 1, _packed(lens)
    up = _Upload()
    up.add("in_off", sig.off, np.int64)
    up.add("in_len", lens, np.int64)
    up.add("out_off", o_off, np.int64)
    d = up.commit(eng.dev)
    q = torch.zeros(max(_ALIGN, total), dtype=torch.int16, device=eng.dev)
    clipped = torch.empty(max(1, n), dtype=torch.int32, device=eng.dev)
    if n:
        eng.call("nc_f32_to_pcm16", sig.buf.data_ptr(), d["in_off"].data_ptr(), d["in_len"].data_ptr(), n,
                 int(lens.max()), q.data_ptr(), d["out_off"].data_ptr(), stride, clipped.data_ptr(), eng.stream())
    return q, o_off, clipped[:n]


def f32_to_pcm16(eng: Engine, arrays: Sequence[np.ndarray]) -> Tuple[List[np.ndarray], np.ndarray]:
    """(int16 arrays, clamped-sample counts) of float32 arrays (``nc_f32_to_pcm16``)."""
    sig = eng.upload_signals([np.asarray(a, np.float32) for a in arrays])
    q, off, clipped = f32_to_pcm16_device(eng, sig)
    return _read_back(q, off, sig.length), clipped.cpu().numpy()


# ------------------------------------------------------------------ true-peak limiter (limiter.hip)
def limiter_windows(sr: int, attack_ms: float = 5.0, release_ms: float = 50.0) -> Tuple[int, int]:
    """(Wa, Wr): the limiter's attack and release in samples at rate ``sr``, at least 1 each."""
    return (max(1, int(round(float(attack_ms) * sr / 1000.0))),
            max(1, int(round(float(release_ms) * sr / 1000.0))))


def _limiter_files(eng: Engine, src, channels):
    """(DeviceSignals, first[file + 1], host lengths) of ``src`` grouped into files of
    ``channels`` consecutive signals (an int for every file, or one count per file)."""
    sig = _signals(eng, src)
    n_sig = sig.n_files
    if isinstance(channels, (int, np.integer)):
        if int(channels) < 1 or n_sig % int(channels):
            raise ValueError("the signals do not divide into files of that many channels")
        counts = np.full(n_sig // int(channels), int(channels), np.int64)
    else:
        counts = np.asarray(channels, np.int64).reshape(-1)
    first = np.zeros(len(counts) + 1, np.int32)
    first[1:] = np.cumsum(counts)
    if int(first[-1]) != n_sig:
        raise ValueError("the channel counts do not add up to the number of signals")
    return sig, first, np.ascontiguousarray(sig.length, np.int64)


def true_peak_device(eng: Engine, src, channels=1) -> torch.Tensor:
    """Inter-sample peak of every file of ``src`` (arrays, or ``DeviceSignals`` already in HBM;
    a file is ``channels`` consecutive signals of one length): device float32 [file], the
    limiter's step 1 (``nc_true_peak``).  One launch, no host synchronisation."""
    sig, first, lens = _limiter_files(eng, src, channels)
    n = len(first) - 1
    up = _Upload()
    up.add("off", sig.off, np.int64)
    up.add("len", lens, np.int64)
    up.add("first", first, np.int32)
    d = up.commit(eng.dev)
    tp = torch.empty(max(1, n), dtype=torch.float32, device=eng.dev)
    if n:
        eng.call("nc_true_peak", sig.buf.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), d["first"].data_ptr(),
                 lens.ctypes.data, first.ctypes.data, n, tp.data_ptr(), eng.stream())
    return tp[:n]


def true_peak_limit_device(eng: Engine, src, channels=1, limit_db: float = -0.1, attack: int = 221,
                           release: int = 2205, in_place: bool = False):
    """The linked true-peak limiter (``nc_true_peak_limit``) on every file of
    ``src`` (arrays, or ``DeviceSignals`` already in HBM; a file is ``channels`` consecutive
    signals of one length), ceiling ``limit_db`` dBFS, ``attack`` / ``release`` in samples
    (``limiter_windows``).  Returns (DeviceSignals of the limited signals — ``src``'s own buffer
    when ``in_place`` —, device float32 true peak in [file], device float32 sample peak out
    [file], device int32 limited frames [file]).  No host synchronisation."""
    sig, first, lens = _limiter_files(eng, src, channels)
    n = len(first) - 1
    frames = np.ascontiguousarray(lens[first[:-1]], np.int64) if n else np.zeros(0, np.int64)
    ws_off = np.zeros(n, np.int64)
    nbytes = int(_native.load().nc_limiter_ws_bytes(frames.ctypes.data, n, ws_off.ctypes.data))
    up = _Upload()
    up.add("off", sig.off, np.int64)
    up.add("len", lens, np.int64)
    up.add("first", first, np.int32)
    up.add("ws_off", ws_off, np.int64)
    d = up.commit(eng.dev)
    out = sig if in_place else DeviceSignals(torch.zeros_like(sig.buf), sig.off, sig.length)
    tp = torch.empty(max(1, n), dtype=torch.float32, device=eng.dev)[:n]
    pk = torch.empty(max(1, n), dtype=torch.float32, device=eng.dev)[:n]
    lim = torch.empty(max(1, n), dtype=torch.int32, device=eng.dev)[:n]
    if n:
        ws = eng.workspace("limiter", nbytes)
        eng.call("nc_true_peak_limit", sig.buf.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(),
                 d["first"].data_ptr(), lens.ctypes.data, first.ctypes.data, n, float(limit_db), int(attack),
                 int(release), out.buf.data_ptr(), d["off"].data_ptr(), tp.data_ptr(), pk.data_ptr(), lim.data_ptr(),
                 ws.data_ptr(), d["ws_off"].data_ptr(), ws.numel(), eng.stream())
    return out, tp, pk, lim


# ------------------------------------------------------------------ pitch shift (pvoc.hip + speed.hip)
PV_Q = 1_000_000
PV_BINS = 1025
PV_N = 2048
PV_TILE = 64             # frames per tile of the phase scan (pvoc.hip PV_TILE)
MAX_SEMITONES = 12.0


def pitch_p(semitones: float) -> int:
    """P = round(2^(S / 12) 10^6) of a shift by S semitones, S first rounded to the six decimals
    the reference hands to rubberband (``--pitch {S:+.6f}``, workflow.py:129-130); |S| <= 12."""
    s = float(semitones)
    if not math.isfinite(s) or not abs(round(s, 6)) <= MAX_SEMITONES:
        raise ValueError(f"pitch shift {semitones!r} outside [-{MAX_SEMITONES:g}, {MAX_SEMITONES:g}] semitones")
    return int(round(2.0 ** (round(s, 6) / 12.0) * PV_Q))


class PvPlan:
    """``nc_pv_plan`` of files of the given lengths at ratio P / 10^6 (host only): stretched
    lengths ``ns``, frame counts ``k``, ``frame_base`` [files + 1], the workspace layout
    ``ws_off`` [6] (mag, V, Phi, frame buffer, empty, scan) and ``ws_bytes``."""

    def __init__(self, P: int, lengths: Sequence[int]):
        lib = _native.load()
        n_in = np.ascontiguousarray(lengths, np.int64).reshape(-1)
        n = len(n_in)
        self.P, self.n_files = int(P), n
        self.ns, self.k = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.frame_base, self.ws_off = np.zeros(n + 1, np.int64), np.zeros(6, np.int64)
        nbytes = C.c_size_t(0)
        _native.check(lib.nc_pv_plan(int(P), n_in.ctypes.data, n, self.ns.ctypes.data, self.k.ctypes.data,
                                     self.frame_base.ctypes.data, self.ws_off.ctypes.data, C.byref(nbytes)),
                      "nc_pv_plan")
        self.ws_bytes = int(nbytes.value)
        self.total_frames = int(self.frame_base[-1])
        self.max_frames = int(self.k.max()) if n else 0
        self.max_ns = int(self.ns.max()) if n else 0


def _pv_analyze(eng: Engine, sig, plan: "PvPlan", want_u: bool, want_v: bool = True):
    """(mag, V or None, empty, U or None) of every frame of ``plan``: ``nc_pv_analyze``, or
    ``nc_pv_analyze_u`` with ``want_u`` (the same kernel body: mag, V and empty are bit-identical)."""
    T = max(1, plan.total_frames)
    up = _Upload()
    up.add("off", sig.off, np.int64)
    up.add("len", sig.length, np.int64)
    up.add("fb", plan.frame_base, np.int64)
    d = up.commit(eng.dev)
    mag = torch.empty((T, PV_BINS), dtype=torch.float32, device=eng.dev)
    v = torch.empty((T, PV_BINS, 2), dtype=torch.float32, device=eng.dev) if want_v else None
    empty = torch.empty(T, dtype=torch.uint8, device=eng.dev)
    head = (sig.buf.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), d["fb"].data_ptr(), plan.n_files,
            plan.total_frames, plan.P, mag.data_ptr(), v.data_ptr() if want_v else 0, empty.data_ptr())
    t = plan.total_frames
    if not want_u:
        eng.call("nc_pv_analyze", *head, eng.stream())
        return mag[:t], v[:t], empty[:t], None
    u = torch.empty((T, PV_BINS, 2), dtype=torch.float32, device=eng.dev)
    eng.call("nc_pv_analyze_u", *head, u.data_ptr(), eng.stream())
    return mag[:t], (v[:t] if want_v else None), empty[:t], u[:t]


def pv_analyze_device(eng: Engine, src, P: int, phasors: bool = False):
    """Stage 1 alone (``nc_pv_analyze``): (mag [frames, 1025] f32, V [frames, 1025, 2] f32,
    empty [frames] uint8, PvPlan), all on the device.  ``phasors``: the analysis phasors
    U = ph(A) [frames, 1025, 2] f32 as a fifth value (``nc_pv_analyze_u``; the first three are
    bit-identical)."""
    sig = _signals(eng, src)
    plan = PvPlan(P, sig.length)
    mag, v, empty, u = _pv_analyze(eng, sig, plan, bool(phasors))
    return (mag, v, empty, plan, u) if phasors else (mag, v, empty, plan)


def pv_lock_device(eng: Engine, mag: torch.Tensor, u: torch.Tensor, v: torch.Tensor, empty: torch.Tensor,
                   frame_base: Sequence[int]):
    """The phase-locked scan alone (``nc_pv_lock``; DESIGN.md §4 "Phase locking"): (Phi
    [frames, 1025, 2] f32, owner [frames, 1025] uint16 — viewed as int16 storage) from the
    magnitudes, analysis phasors U, V and empty flags of files whose frames start at
    ``frame_base`` [files + 1].  Four launches, no host synchronisation."""
    fb = np.ascontiguousarray(frame_base, np.int64).reshape(-1)
    n, total = len(fb) - 1, int(fb[-1])
    mag, u, v, empty = mag.contiguous(), u.contiguous(), v.contiguous(), empty.contiguous()
    if (tuple(mag.shape) != (total, PV_BINS) or tuple(u.shape) != (total, PV_BINS, 2) or
            tuple(v.shape) != (total, PV_BINS, 2) or tuple(empty.shape) != (total,)):
        raise ValueError("mag / U / V / empty do not match frame_base")
    phi = torch.empty_like(v)
    owner = torch.zeros((total, PV_BINS), dtype=torch.int16, device=eng.dev)
    if total == 0:
        return phi, owner
    ws = eng.workspace("pv_lock", int(_native.load().nc_pv_lock_ws_bytes(total, n)))
    d = h2d(fb, np.int64, eng.dev)
    eng.call("nc_pv_lock", mag.data_ptr(), u.data_ptr(), v.data_ptr(), empty.data_ptr(), d.data_ptr(), n, total,
             int(np.diff(fb).max()), phi.data_ptr(), owner.data_ptr(), ws.data_ptr(), ws.numel(), eng.stream())
    return phi, owner


def pv_scan_device(eng: Engine, v: torch.Tensor, empty: torch.Tensor, frame_base: Sequence[int]) -> torch.Tensor:
    """Stage 2 alone (``nc_pv_scan``): Phi [frames, 1025, 2] f32 from V and the empty flags of
    files whose frames start at ``frame_base`` [files + 1]."""
    fb = np.ascontiguousarray(frame_base, np.int64).reshape(-1)
    n, total = len(fb) - 1, int(fb[-1])
    v = v.contiguous()
    empty = empty.contiguous()
    if tuple(v.shape) != (total, PV_BINS, 2) or tuple(empty.shape) != (total,):
        raise ValueError("V / empty do not match frame_base")
    phi = torch.empty_like(v)
    if total == 0:
        return phi
    ws = eng.workspace("pv_scan", int(_native.load().nc_pv_scan_ws_bytes(total, n)))
    d = h2d(fb, np.int64, eng.dev)
    eng.call("nc_pv_scan", v.data_ptr(), empty.data_ptr(), d.data_ptr(), n, total, int(np.diff(fb).max()),
             phi.data_ptr(), ws.data_ptr(), ws.numel(), eng.stream())
    return phi


def pv_synth_device(eng: Engine, mag: torch.Tensor, phi: torch.Tensor, lengths: Sequence[int], P: int):
    """Stage 3 alone (``nc_pv_synth``): (DeviceSignals of the stretched signals, device peak[file])
    from mag / Phi rows laid out by ``PvPlan(P, lengths)``."""
    plan = PvPlan(P, lengths)
    mag, phi = mag.contiguous(), phi.contiguous()
    if tuple(mag.shape) != (plan.total_frames, PV_BINS) or tuple(phi.shape) != (plan.total_frames, PV_BINS, 2):
        raise ValueError("mag / Phi do not match the plan of these lengths")
    n = plan.n_files
    o_off, total = _packed(plan.ns)
    up = _Upload()
    up.add("len", np.asarray(lengths, np.int64), np.int64)
    up.add("fb", plan.frame_base, np.int64)
    up.add("out_off", o_off, np.int64)
    d = up.commit(eng.dev)
    s = torch.zeros(max(_ALIGN, total), dtype=torch.float32, device=eng.dev)
    peak = torch.empty(max(1, n), dtype=torch.float32, device=eng.dev)
    fbytes = plan.total_frames * PV_N * 4
    frames = eng.workspace("pv_frames", fbytes)
    if n:
        eng.call("nc_pv_synth", mag.data_ptr(), phi.data_ptr(), d["len"].data_ptr(), d["fb"].data_ptr(), n,
                 plan.total_frames, plan.P, plan.max_ns, frames.data_ptr(), frames.numel(), s.data_ptr(),
                 d["out_off"].data_ptr(), peak.data_ptr(), eng.stream())
    return DeviceSignals(s, o_off, plan.ns.copy()), peak[:n]


PV_LOCKS = (None, "identity")


def _pv_stretch_locked(eng: Engine, src, P: int, channels):
    """The locked stretch: every group of ``channels`` consecutive signals follows one locked scan
    (its own for a single channel, that of the channels' float32 sum otherwise)."""
    sig, first, lens = _limiter_files(eng, src, channels)
    counts = np.diff(first)
    for g in range(len(counts)):
        if np.any(lens[first[g]:first[g + 1]] != lens[first[g]]):
            raise ValueError("the channels of a linked group must be equally long")
    plan = PvPlan(P, lens)
    if plan.n_files == 0 or np.all(counts == 1):
        mag, v, empty, u = _pv_analyze(eng, sig, plan, True)
        phi, _ = pv_lock_device(eng, mag, u, v, empty, plan.frame_base)
    else:
        n_groups = len(counts)
        m_len = np.ascontiguousarray(lens[first[:-1]], np.int64)
        m_off, m_total = _packed(m_len)
        up = _Upload()
        up.add("off", sig.off, np.int64)
        up.add("len", lens, np.int64)
        up.add("first", first, np.int32)
        up.add("m_off", m_off, np.int64)
        d = up.commit(eng.dev)
        mid = DeviceSignals(torch.zeros(max(_ALIGN, m_total), dtype=torch.float32, device=eng.dev), m_off, m_len)
        eng.call("nc_pv_mid_sum", sig.buf.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), d["first"].data_ptr(),
                 lens.ctypes.data, first.ctypes.data, n_groups, mid.buf.data_ptr(), d["m_off"].data_ptr(),
                 eng.stream())
        m_plan = PvPlan(P, m_len)
        m_mag, m_v, m_empty, m_u = _pv_analyze(eng, mid, m_plan, True)
        psi, _ = pv_lock_device(eng, m_mag, m_u, m_v, m_empty, m_plan.frame_base)
        mag, _, _, u = _pv_analyze(eng, sig, plan, True, want_v=False)
        phi = torch.empty_like(u)
        up = _Upload()
        up.add("fb", plan.frame_base, np.int64)
        up.add("m_fb", m_plan.frame_base, np.int64)
        up.add("first", first, np.int32)
        d = up.commit(eng.dev)
        if plan.total_frames:
            eng.call("nc_pv_rotate", psi.data_ptr(), m_u.data_ptr(), d["m_fb"].data_ptr(), u.data_ptr(),
                     d["fb"].data_ptr(), d["first"].data_ptr(), plan.n_files, n_groups, plan.total_frames,
                     phi.data_ptr(), eng.stream())
    out, peak = pv_synth_device(eng, mag, phi, lens, P)
    return out, peak, plan


def pv_stretch_device(eng: Engine, src, P: int, lock: Optional[str] = None, channels=1):
    """Every file of ``src`` (arrays, or ``DeviceSignals`` already in HBM) stretched in time by
    P / 10^6 with its pitch kept (the phase vocoder of DESIGN.md §4 "Pitch shift";
    ``nc_pv_stretch``, six launches), the result left in HBM: (DeviceSignals of the stretched
    signals, device float32 peak[file] = max |s|, PvPlan).  No host synchronisation.
    ``lock="identity"``: identity phase locking (DESIGN.md §4 "Phase locking"), with every group of
    ``channels`` consecutive, equally long signals (an int, or one count per group, as for the
    limiter) linked to the phases of its sum; 7 launches unlinked, 10 linked."""
    if lock not in PV_LOCKS:
        raise ValueError(f"lock must be one of {PV_LOCKS!r}")
    if lock is not None:
        return _pv_stretch_locked(eng, src, P, channels)
    sig = _signals(eng, src)
    plan = PvPlan(P, sig.length)
    n = plan.n_files
    o_off, total = _packed(plan.ns)
    up = _Upload()
    up.add("off", sig.off, np.int64)
    up.add("len", sig.length, np.int64)
    up.add("fb", plan.frame_base, np.int64)
    up.add("out_off", o_off, np.int64)
    d = up.commit(eng.dev)
    s = torch.zeros(max(_ALIGN, total), dtype=torch.float32, device=eng.dev)
    peak = torch.empty(max(1, n), dtype=torch.float32, device=eng.dev)
    if n:
        ws = eng.workspace("pvoc", plan.ws_bytes)
        eng.call("nc_pv_stretch", sig.buf.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), d["fb"].data_ptr(), n,
                 plan.total_frames, plan.max_frames, plan.P, plan.max_ns, s.data_ptr(), d["out_off"].data_ptr(),
                 peak.data_ptr(), ws.data_ptr(), plan.ws_off.ctypes.data, ws.numel(), eng.stream())
    return DeviceSignals(s, o_off, plan.ns.copy()), peak[:n], plan


def pitch_shift_device(eng: Engine, src, semitones: float, lock: Optional[str] = None, channels=1):
    """Every file of ``src`` (arrays, or ``DeviceSignals`` already in HBM) shifted in pitch by
    ``semitones`` with its duration kept: the stretch by P / 10^6 (``pv_stretch_device``, with its
    ``lock`` and ``channels``), then the speed render at the same ratio (``speed_render_device``),
    cut to the input's length.
    Returns (DeviceSignals of length n per file, device float32 peak[file] of the render, P).
    The peak is that of the whole render, ceil(Ns 10^6 / P) >= n samples.  No host
    synchronisation."""
    if lock not in PV_LOCKS:
        raise ValueError(f"lock must be one of {PV_LOCKS!r}")
    sig = _signals(eng, src)
    P = pitch_p(semitones)
    stretched, _, _ = pv_stretch_device(eng, sig, P, lock=lock, channels=channels)
    out, peak, _ = speed_render_device(eng, stretched, P / PV_Q)
    return DeviceSignals(out.buf, out.off, np.asarray(sig.length, np.int64).copy()), peak, P


def pitch_shift(eng: Engine, arrays: Sequence[np.ndarray], semitones: float, lock: Optional[str] = None,
                channels=1) -> List[np.ndarray]:
    """Each array shifted by ``semitones`` (float32, the input's length)."""
    out, _, _ = pitch_shift_device(eng, [np.asarray(a, np.float32) for a in arrays], semitones, lock=lock,
                                   channels=channels)
    return _read_back(out.buf, out.off, out.length)
