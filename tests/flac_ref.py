"""A plain-Python statement of the FLAC format (RFC 9639) for the tests: a decoder, the two
CRCs, and an encoder whose every choice is an argument, so that a test can put any legal
construct of the format in front of ``nc_flac_index`` / ``nc_flac_decode``.  Nothing here is
fast or clever; Python integers make every sum exact.

    decode(data)                 -> Stream (pcm int64[channels, n], frame table, STREAMINFO)
    encode_frame / build_stream  -> bytes, every header code and subframe choice given
    encode_verbatim              -> numpy fast path, all-VERBATIM 8/16/24-bit streams
    renumber(frames)             -> the same frames with new numbers and CRCs (tiling)
    matrix()                     -> the case matrix shared by the CPU and GPU tests
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np


def _table(poly: int, bits: int) -> List[int]:
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    out = []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def crc16_rows(rows: np.ndarray) -> np.ndarray:
    """crc16 of every row of a uint8 [frames, bytes] array (a loop over the byte columns)."""
    tab = np.array(_T16, np.uint32)
    c = np.zeros(rows.shape[0], np.uint32)
    for j in range(rows.shape[1]):
        c = ((c << 8) & 0xFFFF) ^ tab[(c >> 8) ^ rows[:, j]]
    return c


# ------------------------------------------------------------------ bits
class BitWriter:
    def __init__(self):
        self.done, self.acc, self.n = [], 0, 0      # finished bytes; the bits after them

    def write(self, v: int, n: int) -> None:
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc = (self.acc << n) | v
        self.n += n
        if self.n >= 4096:
            keep = self.n & 7
            self.done.append((self.acc >> keep).to_bytes(self.n >> 3, "big"))
            self.acc, self.n = self.acc & ((1 << keep) - 1), keep

    def signed(self, v: int, n: int) -> None:
        assert -(1 << (n - 1)) <= v < (1 << (n - 1)), (v, n)
        self.write(v & ((1 << n) - 1), n)

    def unary(self, q: int) -> None:
        self.write(1, q + 1)

    def align(self) -> None:
        self.write(0, -self.n % 8)

    def bytes(self) -> bytes:
        assert self.n % 8 == 0
        return b"".join(self.done) + self.acc.to_bytes(self.n // 8, "big")


class BitReader:
    def __init__(self, data: bytes, pos_bytes: int = 0):
        self.d, self.pos, self.nbits = data, 8 * pos_bytes, 8 * len(data)

    def read(self, n: int) -> int:
        if n == 0:
            return 0
        end = self.pos + n
        if end > self.nbits:
            raise ValueError("bitstream ran past the end of the data")
        b0, b1 = self.pos >> 3, (end + 7) >> 3
        v = int.from_bytes(self.d[b0:b1], "big") >> (b1 * 8 - end)
        self.pos = end
        return v & ((1 << n) - 1)

    def signed(self, n: int) -> int:
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self) -> int:
        q = 0
        while self.read(1) == 0:
            q += 1
        return q


# ------------------------------------------------------------------ frame header
RATE_TABLE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100,
              10: 48000, 11: 96000}
BITS_TABLE = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def utf8_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    n = 1
    while v >= 1 << (6 - n + 6 * n):      # n continuation bytes hold 6 n + (6 - n) bits
        n += 1
    out = [((0xFF << (7 - n)) & 0xFF) | (v >> (6 * n))]
    out += [0x80 | ((v >> (6 * (n - 1 - i))) & 0x3F) for i in range(n)]
    return bytes(out)


def block_code(block: int) -> int:
    if block == 192:
        return 1
    for c in range(2, 6):
        if block == 576 << (c - 2):
            return c
    for c in range(8, 16):
        if block == 256 << (c - 8):
            return c
    return 6 if block <= 256 else 7


def frame_header(block: int, bps: int, assign: int, number: int, *, variable: bool = False,
                 bs_code: Optional[int] = None, rate_code: int = 0, rate: int = 44100,
                 ss_code: Optional[int] = None) -> bytes:
    bs_code = block_code(block) if bs_code is None else bs_code
    ss_code = {v: k for k, v in BITS_TABLE.items()}[bps] if ss_code is None else ss_code
    h = bytes([0xFF, 0xF8 | int(variable), (bs_code << 4) | rate_code, (assign << 4) | (ss_code << 1)])
    h += utf8_number(number)
    if bs_code == 6:
        h += bytes([block - 1])
    elif bs_code == 7:
        h += (block - 1).to_bytes(2, "big")
    if rate_code == 12:
        h += bytes([rate // 1000])
    elif rate_code == 13:
        h += rate.to_bytes(2, "big")
    elif rate_code == 14:
        h += (rate // 10).to_bytes(2, "big")
    return h + bytes([crc8(h)])


def parse_frame_header(d: bytes, pos: int, stream_bps: int) -> dict:
    """The header at ``pos`` (ValueError unless it is one): variable, number, block, assign,
    bps, hdr_len, and the byte ranges of the number and of what follows it."""
    if d[pos] != 0xFF or d[pos + 1] & 0xFE != 0xF8:
        raise ValueError(f"no frame sync at byte {pos}")
    bs_code, sr_code = d[pos + 2] >> 4, d[pos + 2] & 15
    assign, ss_code = d[pos + 3] >> 4, (d[pos + 3] >> 1) & 7
    if d[pos + 3] & 1 or bs_code == 0 or sr_code == 15 or assign > 10 or ss_code in (3, 7):
        raise ValueError(f"reserved code in the frame header at byte {pos}")
    q = pos + 4
    b0 = d[q]
    extra = 0 if b0 < 0x80 else 8 - (b0 ^ 0xFF).bit_length() - 1
    if b0 >= 0x80 and (b0 < 0xC0 or b0 == 0xFF):
        raise ValueError("bad frame number")
    num = b0 if b0 < 0x80 else b0 & (0x3F >> extra)
    for i in range(extra):
        if d[q + 1 + i] & 0xC0 != 0x80:
            raise ValueError("bad frame number continuation")
        num = (num << 6) | (d[q + 1 + i] & 0x3F)
    num_end = q + 1 + extra
    q = num_end
    if bs_code == 1:
        block = 192
    elif bs_code <= 5:
        block = 576 << (bs_code - 2)
    elif bs_code == 6:
        block, q = d[q] + 1, q + 1
    elif bs_code == 7:
        block, q = int.from_bytes(d[q:q + 2], "big") + 1, q + 2
    else:
        block = 256 << (bs_code - 8)
    q += {12: 1, 13: 2, 14: 2}.get(sr_code, 0)
    if crc8(d[pos:q]) != d[q]:
        raise ValueError(f"frame header CRC-8 mismatch at byte {pos}")
    return dict(variable=d[pos + 1] & 1, number=num, block=block, assign=assign,
                bps=stream_bps if ss_code == 0 else BITS_TABLE[ss_code], hdr_len=q + 1 - pos,
                num_range=(pos + 4, num_end), tail_end=q)


# ------------------------------------------------------------------ decoder
@dataclass
class Stream:
    rate: int
    channels: int
    bps: int
    total: int                 # samples per channel (from the frames when STREAMINFO holds 0)
    stored_total: int
    md5: bytes
    pcm: np.ndarray            # int64 [channels, total]
    frames: List[Tuple[int, int, int, int, int, int, int]] = field(default_factory=list)
    # (byte start, byte end, first sample, block, assignment, bps, header bytes)


def _read_residual(br: BitReader, block: int, order: int) -> List[int]:
    method = br.read(2)
    if method > 1:
        raise ValueError("reserved residual coding method")
    pbits = 4 + method
    po = br.read(4)
    psize = block >> po
    if psize << po != block or psize < order:
        raise ValueError("partition order does not fit the block")
    out: List[int] = []
    for p in range(1 << po):
        cnt = psize - (order if p == 0 else 0)
        k = br.read(pbits)
        if k == (1 << pbits) - 1:
            nb = br.read(5)
            out += [br.signed(nb) for _ in range(cnt)]
        else:
            for _ in range(cnt):
                u = (br.unary() << k) | br.read(k)
                out.append((u >> 1) ^ -(u & 1))
    return out


def _read_subframe(br: BitReader, block: int, bps: int) -> List[int]:
    if br.read(1):
        raise ValueError("subframe padding bit set")
    t = br.read(6)
    w = br.unary() + 1 if br.read(1) else 0
    bps -= w
    if bps < 1:
        raise ValueError("wasted bits exceed the sample size")
    if t == 0:
        s = [br.signed(bps)] * block
    elif t == 1:
        s = [br.signed(bps) for _ in range(block)]
    elif 8 <= t <= 12 or t >= 32:
        order = t - 8 if t < 32 else t - 31
        if order > block:
            raise ValueError("predictor order above the block size")
        s = [br.signed(bps) for _ in range(order)]
        shift, coef = 0, FIXED.get(order, [])
        if t >= 32:
            prec = br.read(4) + 1
            shift = br.signed(5)
            if prec == 16 or shift < 0:
                raise ValueError("invalid LPC precision or shift")
            coef = [br.signed(prec) for _ in range(order)]
        for r in _read_residual(br, block, order):
            s.append(r + (sum(c * s[-1 - i] for i, c in enumerate(coef)) >> shift))
    else:
        raise ValueError("reserved subframe type")
    return [v << w for v in s]


def _skip_prefix(d: bytes) -> int:
    if d[:3] == b"ID3":
        size = (d[6] & 0x7F) << 21 | (d[7] & 0x7F) << 14 | (d[8] & 0x7F) << 7 | (d[9] & 0x7F)
        return 10 + size + (10 if d[5] & 0x10 else 0)
    return 0


def decode(data: bytes) -> Stream:
    d = bytes(data)
    pos = _skip_prefix(d)
    if d[pos:pos + 4] != b"fLaC":
        raise ValueError("no fLaC marker")
    pos += 4
    info = None
    while True:
        last, typ, ln = d[pos] >> 7, d[pos] & 0x7F, int.from_bytes(d[pos + 1:pos + 4], "big")
        body = d[pos + 4:pos + 4 + ln]
        if info is None:
            assert typ == 0 and ln >= 34
            packed = int.from_bytes(body[10:18], "big")
            info = dict(rate=packed >> 44, channels=((packed >> 41) & 7) + 1, bps=((packed >> 36) & 31) + 1,
                        total=packed & ((1 << 36) - 1), md5=body[18:34])
        pos += 4 + ln
        if last:
            break
    nch, bps = info["channels"], info["bps"]
    chans: List[List[int]] = [[] for _ in range(nch)]
    frames = []
    first = 0
    while pos < len(d):
        h = parse_frame_header(d, pos, bps)
        if h["number"] != (first if h["variable"] else len(frames)):
            raise ValueError(f"frame {len(frames)} is numbered {h['number']}")
        a, block = h["assign"], h["block"]
        if (a + 1 if a < 8 else 2) != nch:
            raise ValueError("channel assignment does not match STREAMINFO")
        br = BitReader(d, pos + h["hdr_len"])
        sub = []
        for c in range(nch):
            side = (a == 8 and c == 1) or (a == 9 and c == 0) or (a == 10 and c == 1)
            sub.append(_read_subframe(br, block, h["bps"] + int(side)))
        if a == 8:
            sub[1] = [l - s for l, s in zip(sub[0], sub[1])]
        elif a == 9:
            sub[0] = [s + r for s, r in zip(sub[0], sub[1])]
        elif a == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(sub[0], sub[1])]
            sub = [[(m + s) >> 1 for m, s in zip(mid, sub[1])], [(m - s) >> 1 for m, s in zip(mid, sub[1])]]
        end = (br.pos + 7) // 8
        if crc16(d[pos:end]) != int.from_bytes(d[end:end + 2], "big") or end + 2 > len(d):
            raise ValueError(f"frame {len(frames)}: CRC-16 mismatch")
        frames.append((pos, end + 2, first, block, a, h["bps"], h["hdr_len"]))
        for c in range(nch):
            chans[c] += sub[c]
        first += block
        pos = end + 2
    total = info["total"] or first
    if first != total:
        raise ValueError(f"{first} samples decoded, STREAMINFO says {total}")
    return Stream(info["rate"], nch, bps, total, info["total"], info["md5"],
                  np.array(chans, np.int64).reshape(nch, total), frames)


def md5_of(pcm: np.ndarray, bps: int) -> bytes:
    """MD5 of the interleaved little-endian samples, ceil(bps / 8) bytes each (STREAMINFO's)."""
    width = (bps + 7) // 8
    a = np.ascontiguousarray(np.asarray(pcm, np.int64).T).astype("<i8")
    return hashlib.md5(a.view(np.uint8).reshape(-1, 8)[:, :width].tobytes()).digest()


# ------------------------------------------------------------------ encoder
def _fold(v: int) -> int:
    return 2 * v if v >= 0 else -2 * v - 1


def _auto_param(part: Sequence[int], method: int) -> int:
    if not part:
        return 0
    mean = sum(_fold(v) for v in part) // len(part)
    return min(max(mean.bit_length() - 1, 0), (14 if method == 0 else 30))


def _write_residual(bw: BitWriter, res: Sequence[int], block: int, order: int, spec: dict) -> None:
    method, po, params = spec.get("method", 0), spec.get("po", 0), spec.get("params")
    pbits = 4 + method
    psize = block >> po
    assert psize << po == block and psize >= order, (block, po, order)
    bw.write(method, 2)
    bw.write(po, 4)
    at = 0
    for p in range(1 << po):
        cnt = psize - (order if p == 0 else 0)
        part = res[at:at + cnt]
        at += cnt
        prm = params[p] if params is not None else _auto_param(part, method)
        if isinstance(prm, tuple):                      # ("esc", width)
            bw.write((1 << pbits) - 1, pbits)
            bw.write(prm[1], 5)
            for v in part:
                if prm[1]:
                    bw.signed(v, prm[1])
                else:
                    assert v == 0
        else:
            assert prm < (1 << pbits) - 1
            bw.write(prm, pbits)
            for v in part:
                u = _fold(v)
                bw.unary(u >> prm)
                bw.write(u & ((1 << prm) - 1), prm)


def _write_subframe(bw: BitWriter, s: Sequence[int], bps: int, spec: dict) -> None:
    """spec: type "constant" | "verbatim" | "fixed" | "lpc"; order; precision, shift, coefs (lpc);
    wasted; method (0 | 1), po, params (per partition: a Rice parameter or ("esc", width))."""
    w = spec.get("wasted", 0)
    assert all(v % (1 << w) == 0 for v in s), "wasted bits need samples divisible by 2^wasted"
    s = [v >> w for v in s]
    bps -= w
    typ, order = spec.get("type", "verbatim"), spec.get("order", 0)
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[typ]
    bw.write(0, 1)
    bw.write(code, 6)
    if w:
        bw.write(1, 1)
        bw.unary(w - 1)
    else:
        bw.write(0, 1)
    if typ == "constant":
        assert all(v == s[0] for v in s)
        bw.signed(s[0], bps)
    elif typ == "verbatim":
        for v in s:
            bw.signed(v, bps)
    else:
        for v in s[:order]:
            bw.signed(v, bps)
        shift, coef = 0, FIXED.get(order, [])
        if typ == "lpc":
            prec, shift, coef = spec["precision"], spec["shift"], list(spec["coefs"])
            assert len(coef) == order
            bw.write(prec - 1, 4)
            bw.signed(shift, 5)
            for c in coef:
                bw.signed(c, prec)
        res = [s[n] - (sum(c * s[n - 1 - i] for i, c in enumerate(coef)) >> shift) for n in range(order, len(s))]
        assert all(-(1 << 31) <= r < (1 << 31) for r in res), "residual outside 32 bits"
        _write_residual(bw, res, len(s), order, spec)


def encode_frame(chans: Sequence[Sequence[int]], bps: int, number: int, *, variable: bool = False,
                 assign: Optional[int] = None, subs: Optional[Sequence[dict]] = None, bs_code: Optional[int] = None,
                 rate_code: int = 0, rate: int = 44100, ss_code: Optional[int] = None) -> bytes:
    """One frame of the true samples ``chans`` (per channel): the stereo transform of
    ``assign`` (8 left/side, 9 side/right, 10 mid/side) is applied here."""
    chans = [[int(v) for v in c] for c in chans]
    nch, block = len(chans), len(chans[0])
    assign = nch - 1 if assign is None else assign
    if assign >= 8:
        left, right = chans
        side = [l - r for l, r in zip(left, right)]
        chans = {8: [left, side], 9: [side, right], 10: [[(l + r) >> 1 for l, r in zip(left, right)], side]}[assign]
    bw = BitWriter()
    for c, s in enumerate(chans):
        wide = (assign == 8 and c == 1) or (assign == 9 and c == 0) or (assign == 10 and c == 1)
        _write_subframe(bw, s, bps + int(wide), subs[c] if subs else {})
    bw.align()
    body = frame_header(block, bps, assign, number, variable=variable, bs_code=bs_code, rate_code=rate_code,
                        rate=rate, ss_code=ss_code) + bw.bytes()
    return body + crc16(body).to_bytes(2, "big")


def stream_header(rate: int, channels: int, bps: int, total: int, *, min_block: int, max_block: int,
                  md5: bytes = bytes(16), metadata: Sequence[Tuple[int, bytes]] = (), id3: Optional[bytes] = None) -> bytes:
    packed = (rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    si = min_block.to_bytes(2, "big") + max_block.to_bytes(2, "big") + bytes(6) + packed.to_bytes(8, "big") + md5
    blocks = [(0, si)] + list(metadata)
    out = b"fLaC"
    for i, (typ, body) in enumerate(blocks):
        out += bytes([typ | (0x80 if i == len(blocks) - 1 else 0)]) + len(body).to_bytes(3, "big") + body
    if id3 is not None:
        n = len(id3)
        out = b"ID3\x04\x00\x00" + bytes([(n >> 21) & 0x7F, (n >> 14) & 0x7F, (n >> 7) & 0x7F, n & 0x7F]) + id3 + out
    return out


def build_stream(pcm, bps: int, blocks: Sequence[int], *, rate: int = 44100, variable: bool = False,
                 frame_args: Optional[Callable[[int], dict]] = None, store_total: bool = True,
                 store_md5: bool = True, metadata: Sequence[Tuple[int, bytes]] = (),
                 id3: Optional[bytes] = None) -> bytes:
    """pcm int [channels, n] cut into frames of ``blocks`` samples; ``frame_args(i)`` gives frame
    i's encode_frame keywords (assign, subs, bs_code, rate_code, ss_code)."""
    pcm = np.asarray(pcm, np.int64)
    assert sum(blocks) == pcm.shape[1]
    out, first = [], 0
    for i, b in enumerate(blocks):
        kw = dict(frame_args(i)) if frame_args else {}
        out.append(encode_frame(pcm[:, first:first + b].tolist(), bps, first if variable else i, variable=variable,
                                rate=rate, **kw))
        first += b
    head = stream_header(rate, pcm.shape[0], bps, pcm.shape[1] if store_total else 0, min_block=min(blocks),
                         max_block=max(blocks), md5=md5_of(pcm, bps) if store_md5 else bytes(16),
                         metadata=metadata, id3=id3)
    return head + b"".join(out)


def encode_verbatim_frames(pcm: np.ndarray, bps: int, block: int = 4096, first_number: int = 0) -> List[bytes]:
    """All-VERBATIM fixed-block-size frames of pcm int [channels, n] (8, 16 or 24 bits), with numpy."""
    assert bps in (8, 16, 24)
    pcm = np.asarray(pcm, np.int64)
    nch, n = pcm.shape
    width = bps // 8
    be = pcm.astype(">i8").view(np.uint8).reshape(nch, n, 8)[:, :, 8 - width:]      # big-endian sample bytes
    frames = []
    n_full = n // block
    if n_full:
        body = np.empty((n_full, nch, 1 + block * width), np.uint8)
        body[:, :, 0] = 0x02                                                         # VERBATIM, no wasted bits
        body[:, :, 1:] = be[:, :n_full * block].reshape(nch, n_full, block * width).transpose(1, 0, 2)
        body = body.reshape(n_full, -1)
        heads = [frame_header(block, bps, nch - 1, first_number + i) for i in range(n_full)]
        by_len: Dict[int, List[int]] = {}
        for i, h in enumerate(heads):
            by_len.setdefault(len(h), []).append(i)
        crcs = np.zeros(n_full, np.uint32)
        for ln, idx in by_len.items():
            rows = np.concatenate([np.frombuffer(b"".join(heads[i] for i in idx), np.uint8).reshape(len(idx), ln),
                                   body[idx]], axis=1)
            crcs[idx] = crc16_rows(rows)
        for i in range(n_full):
            frames.append(heads[i] + body[i].tobytes() + int(crcs[i]).to_bytes(2, "big"))
    if n % block:
        frames.append(encode_frame(pcm[:, n_full * block:].tolist(), bps, first_number + n_full))
    return frames


def encode_verbatim(pcm: np.ndarray, bps: int, rate: int, block: int = 4096, **header_kw) -> bytes:
    pcm = np.asarray(pcm, np.int64)
    frames = encode_verbatim_frames(pcm, bps, block)
    head = stream_header(rate, pcm.shape[0], bps, pcm.shape[1], min_block=block, max_block=block,
                         md5=md5_of(pcm, bps), **header_kw)
    return head + b"".join(frames)


def _gf_mul(a: int, b: int) -> int:
    """a b in GF(2)[x] mod x^16 + x^15 + x^2 + 1."""
    r = 0
    for i in range(15, -1, -1):
        r = ((r << 1) ^ (0x8005 if r & 0x8000 else 0)) & 0xFFFF
        if (b >> i) & 1:
            r ^= a
    return r


def crc16_concat(crc_a: int, crc_b: int, len_b: int) -> int:
    """crc16(A + B) from crc16(A), crc16(B) and len(B): crc(A) x^(8 len(B)) + crc(B) (init 0, no final xor)."""
    power, base, e = 1, 0x0100, len_b                   # x^8
    while e:
        if e & 1:
            power = _gf_mul(power, base)
        base = _gf_mul(base, base)
        e >>= 1
    return _gf_mul(crc_a, power) ^ crc_b


def renumber(frames: Sequence[bytes], bps: int, first_number: int = 0) -> List[bytes]:
    """Fixed-block-size frames numbered first_number, first_number + 1, ... with both CRCs
    recomputed.  A frame that occurs many times (tiling) has its payload's CRC computed once."""
    out = []
    seen: Dict[int, Tuple[int, int, bytes, dict]] = {}
    for i, f in enumerate(frames):
        if id(f) not in seen:
            h = parse_frame_header(f, 0, bps)
            payload = f[h["hdr_len"]:-2]
            seen[id(f)] = (crc16(payload), len(payload), payload, h)
        crc_p, len_p, payload, h = seen[id(f)]
        a, b = h["num_range"]
        head = f[:a] + utf8_number(first_number + i) + f[b:h["tail_end"]]
        head += bytes([crc8(head)])
        out.append(head + payload + crc16_concat(crc16(head), crc_p, len_p).to_bytes(2, "big"))
    return out


# ------------------------------------------------------------------ the case matrix
def _tone(rng, n: int, bps: int, nch: int, amp: float = 0.4) -> np.ndarray:
    """A smooth signal plus a little noise (small predictor residuals), odd and even values."""
    full = 1 << (bps - 1)
    t = np.arange(n)
    x = np.stack([np.sin(2 * np.pi * t * (0.013 + 0.004 * c) + c) for c in range(nch)]) * amp * full
    x = np.rint(x + rng.normal(0, max(1.0, full / 512), (nch, n))).astype(np.int64)
    return np.clip(x, -full, full - 1)


_MATRIX = None


def matrix() -> Dict[str, Tuple[bytes, np.ndarray]]:
    """name -> (stream bytes, expected pcm int64 [channels, n]); built once."""
    global _MATRIX
    if _MATRIX is not None:
        return _MATRIX
    rng = np.random.default_rng(9639)
    m: Dict[str, Tuple[bytes, np.ndarray]] = {}

    def add(name, pcm, bps, blocks, **kw):
        m[name] = (build_stream(pcm, bps, blocks, **kw), np.asarray(pcm, np.int64))

    fixed = lambda o, **kw: dict(type="fixed", order=o, **kw)          # noqa: E731
    # block sizes 16 / 17 / 192 / 4096 / 4608, header codes 6 and 7, final blocks of 1 and 3
    add("bs16_final1", _tone(rng, 33, 16, 2), 16, [16, 16, 1], frame_args=lambda i: dict(bs_code=6))
    add("bs17_final3", _tone(rng, 37, 16, 2), 16, [17, 17, 3], frame_args=lambda i: dict(subs=[fixed(2), fixed(1)]))
    add("bs192_fixed0to4", _tone(rng, 960, 16, 2), 16, [192] * 5,
        frame_args=lambda i: dict(subs=[fixed(i, po=5 if i else 6), fixed(4 - i, po=i)]))
    add("bs300_code7", _tone(rng, 500, 16, 1), 16, [300, 200], frame_args=lambda i: dict(bs_code=7 - i, subs=[fixed(3)]))
    lpc8 = dict(type="lpc", order=8, precision=12, shift=7, coefs=[230, -180, 90, -40, 20, -9, 4, -2], po=8)
    lpc12 = dict(type="lpc", order=12, precision=12, shift=0, coefs=[1, -1, 0, 1, -1, 0, 1, -1, 0, 0, 0, -1], po=3, method=1)
    add("bs4096_lpc8_lpc12_midside", _tone(rng, 8192, 16, 2), 16, [4096, 4096],
        frame_args=lambda i: dict(assign=10, subs=[lpc8, lpc12]))
    lpc32 = dict(type="lpc", order=32, precision=15, shift=14, method=1,
                 coefs=[int(v) for v in np.rint(8000 * np.cos(np.arange(32) * 0.7) / (1 + np.arange(32) / 4))])
    add("bs4608_lpc32_24bit", _tone(rng, 4608, 24, 1), 24, [4608], frame_args=lambda i: dict(subs=[lpc32]))
    # bits per sample by header code, and 16 by code 0
    for bps in (8, 12, 16, 20, 24):
        add(f"bps{bps}", _tone(rng, 101, bps, 2, 0.9), bps, [64, 37], frame_args=lambda i: dict(subs=[fixed(1), fixed(2)]))
    add("bps16_code0", _tone(rng, 101, 16, 1), 16, [64, 37], frame_args=lambda i: dict(ss_code=0, subs=[fixed(1)]))
    # channels 1 / 2 / 3 / 8
    for nch in (1, 3, 8):
        add(f"ch{nch}", _tone(rng, 96, 16, nch), 16, [48, 48],
            frame_args=lambda i, nch=nch: dict(subs=[fixed(c % 5) if (c + i) % 3 else {} for c in range(nch)]))
    # the four stereo modes, odd side values, wasted bits (1 on the left, 7 on a side channel)
    st = _tone(rng, 4 * 40, 16, 2)
    st[1] = st[0] - (2 * ((st[0] - st[1]) // 2) + 1)          # odd left - right everywhere
    add("stereo_modes", st, 16, [40] * 4, frame_args=lambda i: dict(assign=[1, 8, 9, 10][i], subs=[fixed(2), fixed(1)]))
    wl = 2 * rng.integers(-8000, 8000, 64)
    ws = 128 * rng.integers(-100, 100, 64)
    add("wasted_1_and_7_side", np.stack([wl, wl - ws]), 16, [64],
        frame_args=lambda i: dict(assign=8, subs=[fixed(1, wasted=1), dict(wasted=7)]))
    add("wasted_7_verbatim_mono", (128 * rng.integers(-256, 256, 50))[None, :], 16, [50],
        frame_args=lambda i: dict(subs=[fixed(0, wasted=7)]))
    # CONSTANT beside VERBATIM
    cpcm = np.stack([np.full(70, -1234), rng.integers(-32768, 32768, 70)])
    add("constant_verbatim", cpcm, 16, [35, 35], frame_args=lambda i: dict(subs=[dict(type="constant"), {}]))
    # LPC orders x precisions x shifts, predictions of both signs
    for order, prec, shift in ((1, 1, 0), (2, 12, 7), (8, 15, 14), (12, 12, 0), (32, 15, 14), (32, 1, 0), (2, 15, 0)):
        lim = 1 << (prec - 1)
        coefs = [int(v) for v in rng.integers(-lim, lim, order)]
        coefs[0] = -lim                                              # a large negative weight on s[n-1]
        x = _tone(rng, 200, 16 if prec > 1 or order < 32 else 12, 1, 0.1)
        bps = 16 if prec > 1 or order < 32 else 12
        add(f"lpc_o{order}_p{prec}_s{shift}", x, bps, [120, 80],
            frame_args=lambda i, o=order, p=prec, s=shift, cf=coefs: dict(
                subs=[dict(type="lpc", order=o, precision=p, shift=s, coefs=cf, method=1)]))
    # 64-bit accumulation: 24-bit alternating +-(2^23 - 1), order 32, precision 15: the sum is
    # 32 * 16383 * (2^23 - 1) ~ 2^42 before the shift by 14
    alt = ((1 << 23) - 1) * np.where(np.arange(96) % 2 == 0, 1, -1)
    add("lpc32_needs_64bit", alt[None, :], 24, [96], frame_args=lambda i: dict(subs=[dict(
        type="lpc", order=32, precision=15, shift=14, method=1, coefs=[16383 if k % 2 == 0 else -16383 for k in range(32)])]))
    # residual coding
    r0 = rng.integers(-3, 4, 64)
    r0[[3, 20, 41]] = -17                                            # unary runs of 33 zeros
    r0[[7, 30, 50]] = 35                                             # and of 70
    add("rice_k0_runs_33_70", r0[None, :], 16, [64], frame_args=lambda i: dict(subs=[fixed(0, params=[0])]))
    add("rice_k14", rng.integers(-32768, 32768, (1, 64)), 16, [64], frame_args=lambda i: dict(subs=[fixed(0, params=[14])]))
    add("rice5_k30", rng.integers(-(1 << 23), 1 << 23, (1, 48)), 24, [48],
        frame_args=lambda i: dict(subs=[fixed(0, method=1, params=[30])]))
    ramp = (np.arange(64) * 37 - 1000)[None, :]
    add("escape_width0", ramp, 16, [64], frame_args=lambda i: dict(subs=[fixed(2, po=1, params=[("esc", 0), ("esc", 0)])]))
    add("escape_width17", rng.integers(-32768, 32768, (1, 64)), 16, [64],
        frame_args=lambda i: dict(subs=[fixed(0, po=2, params=[("esc", 17), 13, ("esc", 17), ("esc", 17)])]))
    add("po12_block4096", _tone(rng, 4096, 16, 1), 16, [4096], frame_args=lambda i: dict(subs=[fixed(1, po=12)]))
    add("po15_block32768", _tone(rng, 32768, 8, 1), 8, [32768], frame_args=lambda i: dict(subs=[fixed(0, po=15)]))
    # sample-rate codes 0 / table / 12 / 13 / 14 and an ID3v2 prefix with every skippable block type
    meta = [(1, bytes(12)), (2, b"test" + bytes(range(8))), (3, bytes(18)), (4, (3).to_bytes(4, "little") + b"ref" + bytes(4)),
            (5, bytes(396)), (6, bytes(32) + b"\xff\xf8\xc9\x08\x00")]
    add("rate_codes_id3_metadata", _tone(rng, 5 * 32, 16, 2), 16, [32] * 5, rate=48000,
        frame_args=lambda i: dict(rate_code=[0, 10, 12, 13, 14][i], subs=[fixed(1), fixed(1)]),
        metadata=meta, id3=b"TIT2" + bytes(23) + b"\xff\xf8")
    # numbering: variable block size with 1-, 3- and 5-byte sample numbers (total 0 in STREAMINFO)
    vb = [100, 3000] + [65535] * 32 + [50, 7]
    vp = np.repeat(rng.integers(-128, 128, len(vb)), vb)[None, :]
    vp[0, :100] = rng.integers(-128, 128, 100)
    vp[0, -57:] = rng.integers(-128, 128, 57)
    add("variable_blocks", vp, 8, vb, variable=True, store_total=False,
        frame_args=lambda i: dict(subs=[dict(type="constant") if 1 <= i < 34 else fixed(0)]))
    # and a fixed-block-size stream of 2 100 frames of 16 samples (2- and 3-byte frame numbers)
    fp = rng.integers(-128, 128, (1, 2100 * 16))
    m["fixed_2100_frames"] = (encode_verbatim(fp, 8, 44100, block=16), fp.astype(np.int64))
    _MATRIX = m
    return m


def false_sync_stream() -> Tuple[bytes, np.ndarray]:
    """Mono 16-bit, three VERBATIM frames of 4 samples; frame 1's payload spells a frame header
    with a correct CRC-8 and the wrong number (5)."""
    fake = bytes([0xFF, 0xF8, 0x69, 0x08, 0x05])        # block code 6, 44.1 kHz, mono, 16-bit, number 5
    fake += bytes([3, crc8(fake + bytes([3]))])        # block size tail, CRC-8
    spell = np.frombuffer(fake + b"\x00", ">i2").astype(np.int64)
    pcm = np.concatenate([[11, -12, 13, -14], spell, [21, 22, -23, 24]])[None, :]
    return build_stream(pcm, 16, [4, 4, 4]), pcm
