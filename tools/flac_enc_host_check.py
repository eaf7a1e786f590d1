"""Drive tools/flac_enc_host.cpp (the encode kernels compiled for the host under ASan + UBSan; its
build line is in its header) over the encoder's test matrix:

    python tools/flac_enc_host_check.py /tmp/flac_enc_host [fuzz_rounds]

Level 0 must give tests/flac_enc_ref.py's bytes; level 1 must decode (tests/flac_ref.py) to the
input with no frame longer than at level 0; float input must quantise as io.quantize_pcm16 does.
The 2 100-frame case is cut to 140 frames here (a barrier between 64 threads per shuffle is slow).
Runs on the CPU only.
"""
from __future__ import annotations

import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "nightcore-to-flac-analyzer_amd")]

import flac_enc_ref as E   # noqa: E402
import flac_ref as R       # noqa: E402


def main() -> int:
    exe, fuzz = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "0")
    jobs = []
    for name, (pcm, bps, rate, block) in E.cases().items():
        if name == "frames_2100":
            pcm = pcm[:, :140 * 16]
        for level in (0, 1):
            jobs.append((name, np.asarray(pcm, np.int64), bps, rate, block, level, False))
    rng = np.random.default_rng(5)
    for bps in (16, 24):
        full = float(1 << (bps - 1))
        x = rng.uniform(-1.2, 1.2, (2, 300)).astype(np.float32)
        x[0, :64] = (np.arange(64, dtype=np.float32) - 32 + 0.5) / np.float32(full)       # ties
        x[1, :6] = [1.0, -1.0, 1.5, -1.5, (full - 1) / full, -(full + 1) / full]
        jobs.append((f"float{bps}", x, bps, 44100, 128, 1, True))
    with tempfile.TemporaryDirectory() as d:
        with open(Path(d) / "cases.bin", "wb") as fh:
            fh.write(np.int64(len(jobs)).tobytes())
            for name, x, bps, rate, block, level, is_float in jobs:
                fh.write(np.array([x.shape[0], bps, rate, x.shape[1], block, level, int(is_float), 0], np.int64).tobytes())
                fh.write(np.ascontiguousarray(x, np.float32 if is_float else np.int32).tobytes())
        r = subprocess.run([exe, str(Path(d) / "cases.bin"), str(Path(d) / "out.bin"), fuzz, "7"])
        if r.returncode != 0:
            print("the host program failed:", r.returncode)
            return 1
        blob = (Path(d) / "out.bin").read_bytes()
    pos = 0
    level0 = {}
    lpc_frames = 0
    for name, x, bps, rate, block, level, is_float in jobs:
        n_frames, n_bytes = np.frombuffer(blob, np.int64, 2, pos)
        pos += 16
        data = blob[pos:pos + n_bytes]
        pos += n_bytes
        fb = np.frombuffer(blob, np.int32, n_frames, pos)
        pos += 4 * n_frames
        rec = np.frombuffer(blob, np.int32, 25 * n_frames, pos).reshape(n_frames, 25)
        pos += 100 * n_frames
        clipped = np.frombuffer(blob, np.int32, n_frames, pos)
        pos += 4 * n_frames
        status = np.frombuffer(blob, np.int32, n_frames, pos)
        pos += 4 * n_frames
        q = np.frombuffer(blob, np.int32, x.size, pos).reshape(x.shape)
        pos += 4 * x.size
        assert not status.any(), (name, status)
        assert fb.sum() == n_bytes
        if is_float:
            v = np.rint(x * np.float32(1 << (bps - 1)))
            lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
            assert np.array_equal(q, np.clip(v, lo, hi).astype(np.int32)), name
            assert clipped.sum() == np.count_nonzero((v > hi) | (v < lo)), name
            if bps == 16:
                from nightcore_analyzer.io import quantize_pcm16
                assert np.array_equal(q, quantize_pcm16(x)[0]) and clipped.sum() == quantize_pcm16(x)[1]
            pcm = q.astype(np.int64)
        else:
            pcm = x
        head = E.stream_head(rate, pcm.shape[0], bps, pcm.shape[1], block, fb.tolist(), R.md5_of(pcm, bps))
        st = R.decode(head + data)
        assert np.array_equal(st.pcm, pcm), name
        if level == 0:
            want = b"".join(E.encode_frames(pcm, bps, rate, block))
            assert data == want, f"{name}: level 0 bytes differ from the reference's"
            level0[name] = fb
        elif name in level0:
            assert np.all(fb <= level0[name]), name
        lpc_frames += int(np.count_nonzero(rec[:, 1::3] == 3))
        desc = E.describe(head + data)
        for f, (assign, subs) in enumerate(desc):
            assert rec[f, 0] == assign, name
            for c, (typ, order, po, ks) in enumerate(subs):
                assert ["constant", "verbatim", "fixed", "lpc"][rec[f, 1 + 3 * c]] == typ and rec[f, 2 + 3 * c] == order \
                    and rec[f, 3 + 3 * c] == po, (name, f, c)
    assert pos == len(blob)
    print(f"{len(jobs)} jobs ok; {lpc_frames} LPC subframes at level 1")
    return 0


if __name__ == "__main__":
    sys.exit(main())
