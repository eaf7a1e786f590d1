#!/usr/bin/env python
"""Time the device FLAC decode against the 16-bit WAV path on the same PCM (no threshold; the
figures go into DESIGN.md §4 "FLAC decode").

The stream: about 10 s of 44.1 kHz stereo 16-bit frames from the tests' encoder (tests/flac_ref.py:
block 4096, FIXED order 2, Rice partitions of order 4 with per-partition parameters, left/side),
tiled to 3 minutes with the frame numbers and both CRCs rewritten (flac_ref.renumber).  The encode
is plain Python and takes a while; ``--cache`` keeps the 10 s of frames (tools/var/ is not tracked).

Reported, each the median of ``--reps`` runs after ``--warmup`` (host clock around work that ends
in a device synchronise; the launch alone by HIP events):
  flac   host index (nc_flac_index) / index + upload + decode (ops.flac_decode_device, status read
         back) / the nc_flac_decode launch alone; compressed MB/s of index + upload + decode
  wav    host parse of the RIFF file + pinned upload of the int16 samples + nc_pcm16_to_f32

    python tools/flac_decode_probe.py --build-only            # no device needed: fill the cache
    python tools/flac_decode_probe.py --json flac_probe.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import struct
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "nightcore-to-flac-analyzer_amd", REPO / "tests"):
    sys.path.insert(0, str(p))

import flac_ref as R  # noqa: E402

RATE, BLOCK = 44100, 4096


def ten_seconds(cache: Path):
    """(frames, pcm int64 [2, n]) of about 10 s; read from / written to ``cache``."""
    if cache.exists():
        z = np.load(cache)
        ends = np.cumsum(z["lengths"])
        blob = z["blob"].tobytes()
        return [blob[e - n:e] for e, n in zip(ends, z["lengths"])], z["pcm"]
    rng = np.random.default_rng(2026)
    n = 108 * BLOCK                                   # 10.03 s
    t = np.arange(n) / RATE
    left = 0.35 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 554.37 * t + 1) + 0.002 * rng.normal(size=n)
    right = 0.33 * np.sin(2 * np.pi * 220 * t + 0.3) + 0.18 * np.sin(2 * np.pi * 659.25 * t) + 0.002 * rng.normal(size=n)
    pcm = np.clip(np.rint(np.stack([left, right]) * 32768), -32768, 32767).astype(np.int64)
    sub = dict(type="fixed", order=2, po=4)
    frames = [R.encode_frame(pcm[:, i * BLOCK:(i + 1) * BLOCK].tolist(), 16, i, assign=8, subs=[sub, sub])
              for i in range(n // BLOCK)]
    cache.parent.mkdir(parents=True, exist_ok=True)
    np.savez(cache, blob=np.frombuffer(b"".join(frames), np.uint8), lengths=np.array([len(f) for f in frames]), pcm=pcm)
    return frames, pcm


def three_minutes(frames, pcm, seconds: float = 180.0):
    tiles = int(round(seconds * RATE / pcm.shape[1]))
    tiled = R.renumber(list(frames) * tiles, 16)
    full = np.tile(pcm, tiles)
    head = R.stream_header(RATE, 2, 16, full.shape[1], min_block=BLOCK, max_block=BLOCK, md5=R.md5_of(full, 16))
    return head + b"".join(tiled), full


def wav_bytes(pcm: np.ndarray) -> bytes:
    raw = np.ascontiguousarray(pcm.T).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 2, RATE, RATE * 4, 4, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw
    return b"RIFF" + struct.pack("<I", len(body)) + body


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cache", default=str(REPO / "tools" / "var" / "flac_probe_10s.npz"))
    ap.add_argument("--build-only", action="store_true", help="encode the 10 s of frames into the cache and stop")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.build_only and Path(args.cache).exists():
        Path(args.cache).unlink()                     # encode afresh
    frames, pcm10 = ten_seconds(Path(args.cache))
    if args.build_only:
        print(f"{len(frames)} frames, {sum(map(len, frames))} bytes for {pcm10.size * 2} PCM bytes -> {args.cache}")
        return 0
    import torch
    if not torch.cuda.is_available():
        print("flac_decode_probe: no HIP device (timings are taken on the GPU only)", file=sys.stderr)
        return 2
    from nightcore_analyzer import engine as E, ops
    eng = E.get_engine(0)
    blob, pcm = three_minutes(frames, pcm10)
    wav = wav_bytes(pcm)
    n_frames = len(frames) * (pcm.shape[1] // pcm10.shape[1])

    def sync():
        torch.cuda.synchronize(eng.dev)

    def flac_once():
        t0 = time.perf_counter()
        ops.flac_index(blob)
        t1 = time.perf_counter()
        eng.start_timers()
        _, infos = ops.flac_decode_device(eng, [blob])
        sync()
        t2 = time.perf_counter()
        launch = eng.stop_timers()["nc_flac_decode"][0]
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, launch, infos

    def wav_once():
        t0 = time.perf_counter()
        pos = wav.index(b"data") + 8
        x = np.frombuffer(wav, "<i2", offset=pos)
        host = torch.from_numpy(x.copy()).pin_memory()
        raw = host.to(eng.dev, non_blocking=True)
        out = torch.empty(raw.numel(), dtype=torch.float32, device=eng.dev)
        eng.call("nc_pcm16_to_f32", raw.data_ptr(), raw.numel(), out.data_ptr(), eng.stream())
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    # the decode is right before it is timed
    *_, infos = flac_once()
    assert np.array_equal(infos[0]["pcm"].cpu().numpy(), pcm), "decoded PCM differs from the encoder's input"
    _, out = wav_once()
    assert np.array_equal(out.cpu().numpy().reshape(-1, 2).T, (pcm / 32768.0).astype(np.float32))
    fl, wv = [], []
    for i in range(args.warmup + args.reps):             # alternate the two paths
        a, b = flac_once()[:3], wav_once()[0]
        if i >= args.warmup:
            fl.append(a)
            wv.append(b)
    med = statistics.median
    index_ms, e2e_ms, launch_ms = (med(x[k] for x in fl) for k in range(3))
    res = dict(seconds=pcm.shape[1] / RATE, frames=n_frames, flac_bytes=len(blob), pcm_bytes=pcm.size * 2,
               flac_index_ms=index_ms, flac_upload_decode_ms=e2e_ms, flac_decode_launch_ms=launch_ms,
               flac_upload_decode_compressed_MBps=len(blob) / 1e6 / (e2e_ms / 1e3),
               flac_upload_decode_min_max_ms=[min(x[1] for x in fl), max(x[1] for x in fl)],
               wav_parse_upload_widen_ms=med(wv), wav_min_max_ms=[min(wv), max(wv)], reps=args.reps)
    print(json.dumps(res))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
