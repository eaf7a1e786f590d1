"""The encoder's level 0 choice rule (DESIGN.md §4 "FLAC encode") in plain numpy and Python
integers, for the tests of ``nc_flac_encode``: every sum is exact, every tie is resolved in the
stated order, and the frames are written by ``flac_ref.encode_frame`` from the choices.

    choose(x, w, method)              -> (cost in bits, subframe spec for flac_ref)
    encode_frames(pcm, bps, ...)      -> [frame bytes] at level 0
    stream_head(...) / encode(...)    -> the file header / a whole file
    describe(data)                    -> per frame (assignment, [(type, order, po, ks)])
    cases()                           -> the case matrix shared by the CPU and GPU tests
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

import flac_ref as R

RATE_CODE = {v: k for k, v in R.RATE_TABLE.items()}
BITS_CODE = {v: k for k, v in R.BITS_TABLE.items()}


def fold(e: np.ndarray) -> np.ndarray:
    e = np.asarray(e, np.int64)
    return np.where(e >= 0, 2 * e, -2 * e - 1)


def max_po(block: int, order: int) -> int:
    """The largest p <= 6 with block % 2^p == 0 and (block >> p) > order."""
    p = 0
    while p < 6 and block % (2 << p) == 0 and (block >> (p + 1)) > order:
        p += 1
    return p


def rice_partition(u: Sequence[int], kmax: int) -> Tuple[int, int]:
    """(k, bits): the smallest k in 0..kmax minimising n (k + 1) + sum(u >> k)."""
    u = [int(v) for v in u]
    best = None
    for k in range(kmax + 1):
        c = len(u) * (k + 1) + sum(v >> k for v in u)
        if best is None or c < best[1]:
            best = (k, c)
    return best


def fixed_candidates(x: Sequence[int], w: int, method: int):
    """Every (cost, order, po, ks) of the FIXED predictors, in the rule's order."""
    x = np.asarray(x, np.int64)
    block = len(x)
    pbits, kmax = (4, 14) if method == 0 else (5, 30)
    out = []
    for o in range(min(4, block - 1) + 1):
        e = np.diff(x, n=o) if o else x
        u = fold(e)
        # cs[k][i] = sum(u[:i] >> k), exact in int64 (u < 2^33, at most 2^14 terms)
        cs = np.concatenate([np.zeros((kmax + 1, 1), np.int64),
                             np.cumsum(np.stack([u >> k for k in range(kmax + 1)]), axis=1)], axis=1)
        kp1 = np.arange(1, kmax + 2, dtype=np.int64)[:, None]
        for po in range(max_po(block, o) + 1):
            psize = block >> po
            a = np.maximum(np.arange(1 << po) * psize - o, 0)
            b = (np.arange(1 << po) + 1) * psize - o
            cost = (b - a)[None, :] * kp1 + cs[:, b] - cs[:, a]          # [k, partition]
            ks = np.argmin(cost, axis=0)                                 # the first (smallest) k of equals
            bits = int(cost[ks, np.arange(1 << po)].sum()) + pbits * (1 << po)
            out.append((8 + o * w + 6 + bits, o, po, [int(k) for k in ks]))
    return out


def choose(x: Sequence[int], w: int, method: int) -> Tuple[int, dict]:
    """The level 0 choice for one signal of width w: (cost, spec for flac_ref._write_subframe)."""
    x = [int(v) for v in x]
    block = len(x)
    cands = []                                          # (cost, class rank, order, po, spec)
    if all(v == x[0] for v in x):
        cands.append((8 + w, 0, 0, 0, dict(type="constant")))
    for cost, o, po, ks in fixed_candidates(x, w, method):
        cands.append((cost, 1, o, po, dict(type="fixed", order=o, po=po, method=method, params=ks)))
    cands.append((8 + block * w, 2, 0, 0, dict(type="verbatim")))
    cost, _, _, _, spec = min(cands, key=lambda c: c[:4])
    return cost, spec


def choose_frame(chans: np.ndarray, bps: int) -> Tuple[int, List[dict]]:
    """(assignment, subframe specs) of one frame's true samples int [channels, block]."""
    chans = np.asarray(chans, np.int64)
    method = 0 if bps <= 16 else 1
    if chans.shape[0] != 2:
        return chans.shape[0] - 1, [choose(c, bps, method)[1] for c in chans]
    left, right = chans
    cl, cr = choose(left, bps, method), choose(right, bps, method)
    cm, cs = choose((left + right) >> 1, bps, method), choose(left - right, bps + 1, method)
    options = [(cl[0] + cr[0], 1, [cl[1], cr[1]]), (cl[0] + cs[0], 8, [cl[1], cs[1]]),
               (cs[0] + cr[0], 9, [cs[1], cr[1]]), (cm[0] + cs[0], 10, [cm[1], cs[1]])]
    _, assign, subs = min(options, key=lambda t: t[0])   # min keeps the first of equals: 1, 8, 9, 10
    return assign, subs


def encode_frames(pcm, bps: int, rate: int = 44100, block: int = 4096) -> List[bytes]:
    pcm = np.asarray(pcm, np.int64)
    out = []
    for i, first in enumerate(range(0, pcm.shape[1], block)):
        fr = pcm[:, first:first + block]
        assign, subs = choose_frame(fr, bps)
        out.append(R.encode_frame(fr.tolist(), bps, i, assign=assign, subs=subs, rate_code=RATE_CODE.get(rate, 0),
                                  rate=rate, ss_code=BITS_CODE.get(bps, 0)))
    return out


def stream_head(rate: int, channels: int, bps: int, total: int, block: int, frame_sizes: Sequence[int],
                md5: bytes = bytes(16)) -> bytes:
    """``fLaC`` and one STREAMINFO block marked last: min_block = max_block = block, the true
    smallest and largest frame (0 for a stream without frames)."""
    lo, hi = (min(frame_sizes), max(frame_sizes)) if len(frame_sizes) else (0, 0)
    packed = (rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    si = (block.to_bytes(2, "big") * 2 + lo.to_bytes(3, "big") + hi.to_bytes(3, "big") + packed.to_bytes(8, "big") + md5)
    return b"fLaC" + bytes([0x80]) + len(si).to_bytes(3, "big") + si


def encode(pcm, bps: int, rate: int = 44100, block: int = 4096, md5: bool = True) -> bytes:
    pcm = np.asarray(pcm, np.int64)
    frames = encode_frames(pcm, bps, rate, block)
    head = stream_head(rate, pcm.shape[0], bps, pcm.shape[1], block, [len(f) for f in frames],
                       R.md5_of(pcm, bps) if md5 else bytes(16))
    return head + b"".join(frames)


def describe(data: bytes) -> List[Tuple[int, List[Tuple[str, int, int, List[int]]]]]:
    """Per frame of a stream: (assignment, [(type, order, partition order, Rice parameters)])."""
    st = R.decode(data)
    d = bytes(data)
    out = []
    for start, end, first, block, assign, bps, hdr in st.frames:
        br = R.BitReader(d, start + hdr)
        subs = []
        for c in range(st.channels):
            side = (assign == 8 and c == 1) or (assign == 9 and c == 0) or (assign == 10 and c == 1)
            w = bps + int(side)
            assert br.read(1) == 0
            t = br.read(6)
            assert br.read(1) == 0, "the encoder writes no wasted bits"
            if t == 0:
                br.read(w)
                subs.append(("constant", 0, 0, []))
            elif t == 1:
                for _ in range(block):
                    br.read(w)
                subs.append(("verbatim", 0, 0, []))
            else:
                lpc = t >= 32
                order = t - 31 if lpc else t - 8
                for _ in range(order):
                    br.read(w)
                if lpc:
                    prec = br.read(4) + 1
                    br.read(5)
                    for _ in range(order):
                        br.read(prec)
                method = br.read(2)
                po = br.read(4)
                ks = []
                for p in range(1 << po):
                    k = br.read(4 + method)
                    assert k != (1 << (4 + method)) - 1, "the encoder writes no escape partitions"
                    ks.append(k)
                    for _ in range((block >> po) - (order if p == 0 else 0)):
                        br.unary()
                        br.read(k)
                subs.append(("lpc" if lpc else "fixed", order, po, ks))
        out.append((assign, subs))
    return out


# ------------------------------------------------------------------ the case matrix
def spike_partition() -> np.ndarray:
    """64 samples, all zero but one 30000: FIXED order 0 at partition order 0 codes them with
    k = 9 (64 * 10 + (60000 >> 9) = 757 bits) and a unary run of 117 zeros."""
    x = np.zeros(64, np.int64)
    x[37] = 30000
    return x


_CASES = None


def cases() -> Dict[str, Tuple[np.ndarray, int, int, int]]:
    """name -> (pcm int64 [channels, n], bits, rate, block); built once.  About 150 k samples."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(1234)
    m: Dict[str, Tuple[np.ndarray, int, int, int]] = {}

    def full(bps):
        return 1 << (bps - 1)

    # channels x bits, block 64 with a final block of 37
    for nch in (1, 2, 3, 8):
        for bps in (8, 12, 16, 20, 24):
            m[f"ch{nch}_bps{bps}"] = (R._tone(rng, 101, bps, nch, 0.8), bps, 44100, 64)
    # block sizes (16, 64, 100: code 6, 192, 300: code 7, 576, 4096), final blocks of 1, 3 and 17, rates
    m["bs16_final1"] = (R._tone(rng, 49, 16, 2), 16, 22050, 16)
    m["bs64_final3"] = (R._tone(rng, 131, 16, 2), 16, 48000, 64)
    m["bs100_final17"] = (R._tone(rng, 217, 16, 2), 16, 12345, 100)
    m["bs192_exact"] = (R._tone(rng, 576, 16, 2), 16, 44100, 192)
    m["bs300_final17"] = (R._tone(rng, 617, 24, 1), 24, 48000, 300)
    m["bs576"] = (R._tone(rng, 1152 + 17, 16, 2), 16, 44100, 576)
    m["bs4096"] = (R._tone(rng, 8192 + 100, 16, 2), 16, 44100, 4096)
    m["bs4096_24bit"] = (R._tone(rng, 4096, 24, 2), 24, 96000, 4096)
    m["bs16384_mono"] = (R._tone(rng, 16384, 16, 1), 16, 44100, 16384)
    m["shorter_than_block"] = (R._tone(rng, 50, 16, 2), 16, 44100, 4096)
    m["frames_2100"] = (rng.integers(-128, 128, (1, 2100 * 16)), 8, 44100, 16)
    # signals
    m["silence"] = (np.zeros((2, 200), np.int64), 16, 44100, 64)
    m["dc"] = (np.stack([np.full(200, 1234), np.full(200, -77)]), 16, 44100, 64)
    m["white_noise_full_scale"] = (rng.integers(-32768, 32768, (2, 300)), 16, 44100, 100)
    m["white_noise_24"] = (rng.integers(-full(24), full(24), (1, 192)), 24, 44100, 192)
    alt = (full(24) - 1) * np.where(np.arange(256) % 2 == 0, 1, -1)
    m["alternating_24bit"] = (np.stack([alt, -alt]), 24, 44100, 64)
    t = R._tone(rng, 256, 16, 1)[0]
    m["left_equals_right"] = (np.stack([t, t]), 16, 44100, 64)
    m["left_equals_minus_right"] = (np.stack([t, -t]), 16, 44100, 64)
    m["spike_in_silence"] = (spike_partition()[None, :], 16, 44100, 64)
    # an odd block has partition order 0 only: the spike's partition is the whole block, k = 9
    # (65 * 10 + 117 = 767 bits) and the unary run is 117 zeros
    m["spike_run117"] = (np.concatenate([spike_partition(), [0]])[None, :], 16, 44100, 65)
    sp = np.zeros((2, 4096), np.int64)
    sp[0, 1000], sp[1, 3000] = 30000, -32768
    m["spikes_block4096"] = (sp, 16, 44100, 4096)
    m["bits_code0"] = (R._tone(rng, 150, 10, 2), 10, 44100, 64)        # sample-size code 0
    _CASES = m
    return m
