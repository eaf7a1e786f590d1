#!/usr/bin/env python
"""Time the device FLAC encode against the 16-bit WAV path for the same resident render (no
threshold; the figures go into DESIGN.md §4 "FLAC encode").

The signal: 180 s of 44.1 kHz stereo float32 (two tones a channel plus a little noise, the
decode probe's signal), uploaded once and left in HBM as a render would be.  Reported, each the
median of ``--reps`` runs after ``--warmup`` (host clock around work that ends in a device
synchronise; the launches alone by HIP events):
  flac   the nc_flac_encode launch / the nc_flac_pack launch (levels 0 and 1) / the whole
         io.write_flac_device path to a file, with and without the MD5
  wav    ops.f32_to_pcm16_device + the download of the int16 samples + io.write_wav
  size   the file at level 0, at level 1, and all-VERBATIM (computed)

    python tools/flac_encode_probe.py --json flac_encode_probe.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "nightcore-to-flac-analyzer_amd", REPO / "tests"):
    sys.path.insert(0, str(p))

RATE, BLOCK = 44100, 4096


def signal(seconds: float) -> np.ndarray:
    rng = np.random.default_rng(2026)
    n = int(seconds * RATE)
    t = np.arange(n) / RATE
    left = 0.35 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 554.37 * t + 1) + 0.002 * rng.normal(size=n)
    right = 0.33 * np.sin(2 * np.pi * 220 * t + 0.3) + 0.18 * np.sin(2 * np.pi * 659.25 * t) + 0.002 * rng.normal(size=n)
    return np.stack([left, right]).astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("flac_encode_probe: no HIP device (timings are taken on the GPU only)", file=sys.stderr)
        return 2
    from nightcore_analyzer import engine as E, io as nio, ops
    eng = E.get_engine(0)
    x = signal(args.seconds)
    sig = eng.upload_signals(list(x))
    n = x.shape[1]
    tmp = Path(tempfile.mkdtemp(prefix="flac_encode_probe"))

    def sync():
        torch.cuda.synchronize(eng.dev)

    def launches(level):
        eng.start_timers()
        (blob,), (info,) = ops.flac_encode_device(eng, sig, [2], 16, RATE, BLOCK, level)
        t = eng.stop_timers()
        return t["nc_flac_encode"][0], t["nc_flac_pack"][0], len(blob), info

    def flac_file(md5):
        sync()
        t0 = time.perf_counter()
        nio.write_flac_device(tmp / "a.flac", eng, sig, RATE, 16, block=BLOCK, level=1, md5=md5)
        return (time.perf_counter() - t0) * 1e3

    def wav_file():
        sync()
        t0 = time.perf_counter()
        q, _, _ = ops.f32_to_pcm16_device(eng, sig, interleave=True)
        nio.write_wav(tmp / "a.wav", q[:2 * n].cpu().numpy().reshape(n, 2).T, RATE, "pcm16")
        return (time.perf_counter() - t0) * 1e3

    # the encode is right before it is timed: the file decodes to the quantised samples, MD5 checked
    flac_file(True)
    data, _, _ = nio.read_flac_channels(tmp / "a.flac", verify_md5=True)
    assert np.array_equal(data, nio.quantize_pcm16(x)[0].astype(np.float32) / 32768.0), "the file does not decode to the input"
    rows = []
    for i in range(args.warmup + args.reps):             # alternate the paths
        l0, l1 = launches(0), launches(1)
        row = dict(enc0=l0[0], pack0=l0[1], enc1=l1[0], pack1=l1[1], flac_md5=flac_file(True), flac_nomd5=flac_file(False),
                   wav=wav_file())
        if i >= args.warmup:
            rows.append(row)
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    span = {k: [min(r[k] for r in rows), max(r[k] for r in rows)] for k in rows[0]}
    n_frames = -(-n // BLOCK)
    import flac_ref as R
    hdr = sum(4 + len(R.utf8_number(f)) + {6: 1, 7: 2}.get(R.block_code(min(BLOCK, n - f * BLOCK)), 0) + 1
              for f in range(n_frames))
    verbatim = 42 + hdr + sum(2 * (1 + 2 * min(BLOCK, n - f * BLOCK)) + 2 for f in range(n_frames))
    lpc = int(np.count_nonzero(l1[3]["records"][:, 1::3] == 3))
    res = dict(seconds=n / RATE, frames=n_frames, pcm_bytes=4 * n, size_level0=42 + l0[2], size_level1=42 + l1[2],
               size_verbatim=verbatim, lpc_subframes_level1=lpc, subframes=2 * n_frames,
               encode_launch_level0_ms=med["enc0"], encode_launch_level1_ms=med["enc1"],
               pack_launch_level0_ms=med["pack0"], pack_launch_level1_ms=med["pack1"],
               write_flac_md5_ms=med["flac_md5"], write_flac_no_md5_ms=med["flac_nomd5"], wav_path_ms=med["wav"],
               min_max_ms=span, reps=args.reps)
    print(json.dumps(res))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
