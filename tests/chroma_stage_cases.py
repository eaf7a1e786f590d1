"""Inputs, per-stage f64 references and yardsticks for the stage tests of the chroma chain
(csrc/cqt.hip behind nc_chroma_mean: chroma_plan -> decimate3 x2 -> tuning_peaks ->
tuning_select -> cqt_mfma_low / cqt_mfma -> cqt_tail -> chroma_finalize).  No GPU in here.

Every reference is a function of the PREVIOUS stage's values, so the GPU file
(test_gpu_chroma_stages.py) feeds it the device's own previous stage and a failure names one
kernel; the CPU file (test_chroma_stage_cases_cpu.py) feeds it the oracle's and shows that the
reference alone stays inside every bar.  All pieces come from oracle/ncref.py:

  plan()            the octave lengths / offsets / frame counts, integers
  decimate          ncref.decimate2; level_bound() is the derived bar: a 25-term f32 FMA chain
                    on f32-rounded taps, x sqrt(2) through f64, one rounding, plus the
                    reference's own rounding: 27 * 2^-24 * sqrt(2) sum|h| * max|previous level|
  peaks()           ncref.piptrack's nonzero entries (f64=True: the same stencil on an f64
                    spectrum); compare_sorted() pairs two unordered lists by order statistics
  tuning_from_list  ncref.tuning_counts at np.median of the list's magnitudes
  octave_rows()     one octave of ncref.cqt_mag from that octave's level, folded to the 12
                    chroma columns with ncref.cq_to_chroma (f64=True: the same complex64
                    filter bank evaluated in f64 / complex128)
  tail()            the 7-octave f32 sum, ncref.chroma_cqt's inf-norm, the f64 mean

Yardsticks are the oracle's f32 / complex64 path against the f64 evaluation of the same
quantity; the device is held to MARGIN x that (the project's 16, align_cases.SCORE_MARGIN).
A chunk of a frame or two samples the rounding of a dozen values, so a chunk's row yardstick
is never taken below the median of its launch's chunks (the same arithmetic on the same kind
of signal).  The MFMA CQT's operands are f16 hi + lo halves at one scale per (chunk, octave):
its error follows the level's largest sample, not each bin as the oracle's complex64 path
does, so the row bar adds split_allowance() (derived from the formats) to the yardstick term;
ROW_CAP bounds the sum from above whatever the two say.

Lengths are placed by the tile constants the library reports (constants(), the host-only
nc_chroma_workspace_layout), never by literals."""
import ctypes as C
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import ncref
from nightcore_analyzer import _native, synth

SR = 22050
MARGIN = 16.0
ROW_FLOOR = 1e-3          # a frame's scale is never below this x the chunk's largest row value (-60 dB)
ROW_CAP = 1e-4            # no row bar above this: 100x under the 1 % errors the end-to-end test lets through
LAYOUT_NAMES = ("entries", "oct_off", "oct_len", "n_frames", "n_tframes", "chunk_npk", "tuning_idx", "tf_base",
                "oct_base", "ws_oct", "peak_pitch", "peak_mag", "partial", "tp_base", "xmax", "gpart", "oct_ex",
                "bytes", "D3_TILE", "kPeakSlots", "CH_FR", "C2_FR", "C2_NW", "CM_FR", "kHalfbandK", "head")

Chunk = namedtuple("Chunk", "name off len")
Launch = namedtuple("Launch", "name sig chunks")


def layout(n_chunks, total_len):
    """nc_chroma_workspace_layout as a dict (host only: needs the built library, no device)."""
    lib = _native.load()
    out = np.zeros(len(LAYOUT_NAMES), np.int64)
    got = lib.nc_chroma_workspace_layout(None, int(n_chunks), int(total_len), out.ctypes.data_as(C.c_void_p),
                                         len(out))
    assert got == len(LAYOUT_NAMES) == out[0], (got, out[0])
    return dict(zip(LAYOUT_NAMES, (int(v) for v in out)))


@lru_cache(maxsize=None)
def constants():
    lay = layout(1, 512)
    return {k: lay[k] for k in ("D3_TILE", "kPeakSlots", "CH_FR", "C2_FR", "C2_NW", "CM_FR", "kHalfbandK")}


def tile_extents():
    """Level-0 samples per tile of each kernel of the chain."""
    k = constants()
    return {"decimate3 base 0": 8 * k["D3_TILE"], "decimate3 base 3": 64 * k["D3_TILE"],
            "cqt high": k["CH_FR"] * 512, "cqt low pair": k["C2_FR"] * k["C2_NW"] * 512, "tail": k["CM_FR"] * 512}


# --------------------------------------------------------------------------- plan
def plan(lens):
    """chroma_plan_kernel restated: (oct_len [n,7], oct_off [n,7], n_frames, n_tframes, tf_base [n+1])."""
    n = len(lens)
    oct_len = np.zeros((n, 7), np.int64)
    oct_off = np.full((n, 7), -1, np.int64)
    n_frames = np.zeros(n, np.int64)
    acc = 0
    for c, L0 in enumerate(lens):
        L, hop, tmin = int(L0), 512, None
        for i in range(7):
            oct_len[c, i] = L
            if i:
                oct_off[c, i] = acc
                acc += (L + 63) & ~63
            t = 1 + L // hop
            tmin = t if tmin is None else min(tmin, t)
            hop >>= 1
            L = (L + 1) // 2
        n_frames[c] = tmin
    n_tframes = np.array([1 + int(L) // 512 for L in lens], np.int64)
    return oct_len, oct_off, n_frames, n_tframes, np.concatenate([[0], np.cumsum(n_tframes)])


# --------------------------------------------------------------------------- decimation
def taps_f32():
    return ncref.halfband_taps(constants()["kHalfbandK"]).astype(np.float32)


def level_gain():
    """g = sqrt(2) sum|h|: |level o+1| <= g max|level o| (the bound the f16 exponents rest on)."""
    return float(np.sqrt(2.0) * np.abs(taps_f32().astype(np.float64)).sum())


def level_bound(prev_max):
    return 27.0 * 2.0 ** -24 * level_gain() * float(prev_max)


def levels_oracle(y):
    """The oracle's own chain from level 0: [y, decimate2(y), ...] (7 levels, f32)."""
    out = [np.asarray(y, np.float32)]
    for _ in range(6):
        out.append(ncref.decimate2(out[-1]))
    return out


def levels_f64(y):
    """The same chain without the per-level rounding to f32."""
    taps = ncref.halfband_taps()
    K = (len(taps) - 1) // 2
    out = [np.asarray(y, np.float32).astype(np.float64)]
    for _ in range(6):
        x = out[-1]
        M = (len(x) + 1) // 2
        xp = np.pad(x, (K, K + 1))
        acc = np.zeros(M)
        for j, n in enumerate(range(-K, K + 1)):
            if taps[j] != 0.0:
                acc += taps[j] * xp[K - n: K - n + 2 * M: 2][:M]
        out.append(acc * np.sqrt(2.0))
    return out


def chain_bounds(level_max):
    """The per-level bound compounded from level 0: e_o = g e_{o-1} + level_bound(max|level o-1|)."""
    g, e, out = level_gain(), 0.0, [0.0]
    for o in range(1, 7):
        e = g * e + level_bound(level_max[o - 1])
        out.append(e)
    return out


# --------------------------------------------------------------------------- piptrack peaks
def peaks(y, f64=False):
    """(pitch, mag, peaks per frame): ncref.piptrack's nonzero entries, unordered.  f64: the
    same stencil, thresholds and parabolic shift on the f64 spectrum."""
    y = np.asarray(y, np.float32)
    if not f64:
        p, m = ncref.piptrack(y)
        nz = p > 0
        return p[nz].astype(np.float64), m[nz].astype(np.float64), nz.sum(axis=0)
    T = 1 + len(y) // 512
    fr = ncref._frames(y, 2048, 512, 0, T).astype(np.float64) * ncref.hann(2048)[None]
    S = np.abs(np.fft.rfft(fr, axis=-1).T)
    freqs = np.fft.rfftfreq(2048, 1.0 / SR)
    avg = np.gradient(S, axis=0)
    a = S[2:] + S[:-2] - 2 * S[1:-1]
    b = (S[2:] - S[:-2]) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        sh = np.where(np.abs(b) >= np.abs(a), 0.0, -b / a)
    shift = np.zeros_like(S)
    shift[1:-1] = sh
    Z = S * (S > 0.1 * S.max(axis=0, keepdims=True))
    Zp = np.pad(Z, ((1, 1), (0, 0)), mode="edge")
    lm = (Z > Zp[:-2]) & (Z >= Zp[2:]) & ((150.0 <= freqs) & (freqs < 4000.0))[:, None]
    idx = np.nonzero(lm)
    pitch = (idx[0] + shift[idx]) * float(SR) / 2048
    mag = S[idx] + 0.5 * avg[idx] * shift[idx]
    keep = pitch > 0
    return pitch[keep], mag[keep], lm.sum(axis=0)


def peak_cap(n):
    """Peaks that may stay unmatched on either side: threshold / plateau near-ties."""
    return max(2, int(0.002 * n))


def compare_sorted(a, b, tol):
    """Two unordered lists paired by order statistics (sorted against sorted minimises the
    largest pair distance, so it never invents an error): equal counts -> (0, 0, max |a_i - b_i|);
    else a greedy merge at `tol` -> (unmatched in a, unmatched in b, largest matched distance)."""
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    if len(a) == len(b):
        return 0, 0, float(np.max(np.abs(a - b))) if len(a) else 0.0
    i = j = ua = ub = 0
    worst = 0.0
    while i < len(a) and j < len(b):
        d = abs(a[i] - b[j])
        if d <= tol:
            worst = max(worst, d)
            i += 1
            j += 1
        elif a[i] < b[j]:
            ua += 1
            i += 1
        else:
            ub += 1
            j += 1
    return ua + len(a) - i, ub + len(b) - j, worst


def peak_yardstick(y):
    """(pitch Hz, magnitude relative to the largest) the oracle's f32 list moves against the
    f64 one; None where their decisions differ (the CPU file shows they do not)."""
    p32, m32, _ = peaks(y)
    p64, m64, _ = peaks(y, f64=True)
    if len(p32) != len(p64):
        return None
    if not len(p32):
        return 0.0, 0.0
    return (compare_sorted(p32, p64, 0)[2], compare_sorted(m32, m64, 0)[2] / float(m64.max()))


# --------------------------------------------------------------------------- tuning select
EDGE_EPS = 2e-4     # f32 residual 36 log2(p / 27.5) mod 1: |36 o| <= 260, a few ulps of it and of log2f < 5e-5


def tuning_from_list(pitch, mag):
    """estimate_tuning's tail on a given peak list: threshold np.median(mag), ncref.tuning_counts
    -> (index, margin, ambiguous): ambiguous = selected peaks whose residual lies within EDGE_EPS
    of a histogram edge, the only ones an f32 residual may put in the neighbouring bin."""
    pitch, mag = np.asarray(pitch, np.float32), np.asarray(mag, np.float32)
    if not len(pitch):
        return 50, 0, 0
    thr = np.median(mag)
    sel = pitch[(mag >= thr) & (pitch > 0)].astype(np.float64)
    counts = ncref.tuning_counts(sel, 0.01, 36)
    if counts is None:
        return 50, 0, 0
    r = np.mod(36 * np.log2(sel / 27.5), 1.0) * 100.0
    amb = int(np.sum(np.abs(r - np.round(r)) < EDGE_EPS * 100.0))
    best = int(np.argmax(counts))
    return best, int(counts[best] - np.max(np.delete(counts, best))), amb


def tuning_value(idx):
    return float(ncref.tuning_edges(0.01)[idx])


# --------------------------------------------------------------------------- CQT rows
@lru_cache(maxsize=128)
def _octave_filters(tuning):
    """Per device octave o (0 = the chunk itself, CQT bins 216..251): (the oracle's complex64
    bank, the same bank before its last rounding, 1 / sqrt(filter length))."""
    fmin = ncref.C1_HZ * 2.0 ** (tuning / 36)
    freqs = ncref.interval_frequencies(252, fmin, 36)
    alpha = ncref.relative_bandwidth(freqs)
    lengths, _ = ncref.wavelet_lengths(freqs, SR, alpha)
    out, my_sr = [], float(SR)
    for i in range(7):
        sl = slice(-36, None) if i == 0 else slice(-36 * (i + 1), -36 * i)
        fb, n_fft = ncref.vqt_filter_fft(my_sr, freqs[sl], alpha[sl])
        assert n_fft == 1024
        out.append(((fb * np.sqrt(SR / my_sr)).astype(np.complex64),
                    fb.astype(np.complex128) * np.sqrt(SR / my_sr), np.sqrt(lengths[sl])))
        my_sr /= 2.0
    return out


FOLD = ncref.cq_to_chroma(36, 36, 12).astype(np.float64)     # column j <- bins 3j-1, 3j, 3j+1 (mod 36)


def octave_mag(level, o, tuning, f64=False):
    """|C| [36, T_o] of device octave o from its level, scaled as ncref.cqt_mag scales it."""
    level = np.asarray(level, np.float32)
    fb32, fb128, sqlen = _octave_filters(float(tuning))[o]
    hop = 512 >> o
    if f64:
        T = 1 + len(level) // hop
        D = np.fft.rfft(ncref._frames(level, 1024, hop, 0, T).astype(np.float64), axis=-1).T
        return np.abs(fb128 @ D) / sqlen[:, None]
    V = (fb32 @ ncref.stft(level, 1024, hop, "ones")).astype(np.complex64)
    V /= sqlen[:, None]
    return np.abs(V).astype(np.float32)


def octave_rows(level, o, tuning, n_frames, f64=False):
    """[n_frames, 12]: the octave's 36 |C| folded to its chroma columns (one gpart octave)."""
    C_ = octave_mag(level, o, tuning, f64)[:, :n_frames]
    if f64:
        return (FOLD @ C_).T
    return (FOLD.astype(np.float32) @ C_).T.astype(np.float64)


def row_metric(G, R):
    """Per frame: max over the 12 columns of |G - R| over max(the frame's largest R,
    ROW_FLOOR x the chunk's largest R).  An all-zero reference asks for exact zeros (inf)."""
    G, R = np.asarray(G, np.float64), np.asarray(R, np.float64)
    top = R.max() if R.size else 0.0
    err = np.abs(G - R).max(axis=1)
    if top == 0.0:
        return np.where(err == 0.0, 0.0, np.inf)
    return err / np.maximum(R.max(axis=1), ROW_FLOOR * top)


def row_yardstick(levels, tuning, n_frames):
    """Per octave: the oracle's complex64 rows against the f64 evaluation, worst frame."""
    return np.array([row_metric(octave_rows(levels[o], o, tuning, n_frames),
                                octave_rows(levels[o], o, tuning, n_frames, f64=True)).max() for o in range(7)])


@lru_cache(maxsize=128)
def filter_l2_gain(tuning, o):
    """The gain from independent per-sample errors of a level to a gpart column, per unit of
    error: sqrt(sum_n |h_j[n]|^2) of the time-domain filters h_j[n] = sum_b fb[j][b]
    e^{-2 pi i b n / 1024}, scaled and folded like the rows, the largest of the 12 columns."""
    _, fb128, sqlen = _octave_filters(float(tuning))[o]
    full = np.zeros((36, 1024), np.complex128)
    full[:, :513] = fb128
    l2 = np.sqrt((np.abs(np.fft.fft(full, axis=1)) ** 2).sum(axis=1)) / sqlen
    return float((FOLD @ l2).max())


def split_allowance(level_max, ex, tuning, o):
    """What the f16 hi / lo split of the MFMA CQT may add to a gpart value (absolute): each
    operand keeps 22 significant bits (2^-22 of the sample and of the filter tap, truncated:
    2^-21 of a product) and a sample's lo half is an f16 whose subnormal spacing is 2^-24 at
    the per-chunk scale 2^ex, i.e. 2^-37 of the split's full scale 2^(13 - ex).  Errors of the
    1 024 taps are independent, so they reach a column through the filters' l2 gain.  This is
    a term in the level's LARGEST SAMPLE, where the oracle's complex64 path (an f64 FFT
    rounded bin by bin) errs relative to each bin: it matters where an octave's band holds
    far less than the level's amplitude, which the yardstick cannot see."""
    return filter_l2_gain(float(tuning), o) * (2.0 ** -21 * float(level_max) + 2.0 ** -37 * 2.0 ** (13 - int(ex)))


def row_bars(yards):
    """yards [chunks, 7] of one launch -> bars [chunks, 7] (module docstring)."""
    yards = np.asarray(yards, np.float64)
    return np.minimum(MARGIN * np.maximum(yards, np.median(yards, axis=0, keepdims=True)), ROW_CAP)


# --------------------------------------------------------------------------- tail
def tail(gpart):
    """gpart [T, 7, 12] (k = 0 the lowest octave) -> the chunk's mean chroma [12] (f64):
    cqt_tail's f32 sum over k ascending, ncref.chroma_cqt's inf-norm, the mean over frames."""
    g = np.asarray(gpart, np.float32)
    ch = np.zeros(g.shape[::2], np.float32)
    for k in range(7):
        ch = ch + g[:, k, :]
    mx = np.max(np.abs(ch), axis=1, keepdims=True).astype(np.float64)
    mx[mx < ncref.TINY32] = 1.0
    return (ch.astype(np.float64) / mx).astype(np.float32).astype(np.float64).mean(axis=0)


TAIL_BAR = 4.0 * 2.0 ** -24     # the mean is <= 1: f32 adds and one division restated exactly, the f64 mean's
                                # order and the f64 -> f32 rounding are what is left


# --------------------------------------------------------------------------- signals
@lru_cache(maxsize=None)
def _music():
    return synth.make_pair(30.0, 1007)[1].astype(np.float32)


def detuned(r, n, seed=7):
    """test_gpu_chroma.dense_peak_chunk's stack of sines, r 36ths of an octave off the A440
    grid, noise sigma 0.002."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = np.zeros(n)
    for m in range(0, 400, 3):
        f = 27.5 * 2 ** ((m + r) / 36)
        if 200 <= f <= 3900:
            y += 0.03 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))
    return (y + rng.normal(0, 0.002, n)).astype(np.float32)


def burst(freqs_amps, n=511, sigma=60.0):
    """Gaussian-windowed tones in a chunk of one tuning frame: a Gaussian spectrum has no side
    lobes, so every tone is exactly one piptrack peak.  A tone at 0.05 in the middle of each
    of the seven octaves stays under piptrack's threshold (0.1 of the largest bin) and gives
    every octave of the CQT something to measure."""
    t = np.arange(n) - (n - 1) / 2
    y = sum(a * np.cos(2 * np.pi * f * t / SR) for f, a in freqs_amps)
    y = y + sum(0.05 * np.cos(2 * np.pi * ncref.C1_HZ * 2.0 ** (k + 0.5) * t / SR + k) for k in range(7))
    return (y * np.exp(-0.5 * (t / sigma) ** 2)).astype(np.float32)


def adversarial(n, A=0.37, seed=11):
    """The +-A sign pattern of the half-band taps around one even sample, in noise below A:
    level 1 reaches sqrt(2) sum|h| A there, the bound the f16 exponents rest on."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-0.9 * A, 0.9 * A, n)
    h = taps_f32()
    K = (len(h) - 1) // 2
    m = (n // 4) * 2                                  # y[m - j] = A sign(h[j]), j = -K..K; zero taps keep the noise
    for j in range(-K, K + 1):
        if h[j + K] != 0.0:
            y[m - j] = A * np.sign(h[j + K])
    return y.astype(np.float32)


TUNING_INDICES = (0, 1, 25, 49, 50, 74, 98, 99)   # stacks at these bins' centres
EXTRA_DETUNE = -0.235     # the oracle puts the stack at bin 25's centre on 24 and this one on 25
SHORT_LENGTHS = (1, 2, 63, 511, 512, 513, 1023)


def _assemble(name, parts):
    """Chunks one after the other with 1 or 2 zeros before each (odd and even chunk_off); the
    last chunk ends with the buffer."""
    sig, chunks, pos = [], [], 0
    for i, (cname, y) in enumerate(parts):
        gap = np.zeros(1 + (i % 2), np.float32)
        sig += [gap, np.asarray(y, np.float32)]
        pos += len(gap)
        chunks.append(Chunk(cname, pos, len(y)))
        pos += len(y)
    return Launch(name, np.concatenate(sig), tuple(chunks))


@lru_cache(maxsize=None)
def launch(name):
    """edges: music chunks one sample either side of every tile extent, the short lengths between
    them, an all-zero chunk, a chunk whose middle third is digital silence, the adversarial chunk.
    tuning: the eight detuned stacks, white noise (two compaction passes), the 512-periodic
    signal (massive magnitude ties), one burst (N = 1) and two (N = 2, the weaker one in the
    lower histogram bin: the even-count median's upper middle decides the index).
    forced: two stacks whose peak lists are forced_lists() and one that keeps its own."""
    music, rng = _music(), np.random.default_rng(5)
    ext = tile_extents()
    if name == "edges":
        longs = [(f"{k} {d:+d}", e + d) for k, e in ext.items() for d in (-1, 1)]
        shorts = [(f"short {L}", (0.2 * rng.standard_normal(L)).astype(np.float32)) for L in SHORT_LENGTHS]
        parts, start = [], 5 * SR
        for i, (nm, L) in enumerate(longs):
            parts.append((nm, music[start:start + L]))
            start = (start + 7919 * (i + 1)) % (len(music) - max(ext.values()) - 2)
            if i < len(shorts):
                parts.append(shorts[i])
        gap = music[7 * SR:7 * SR + 3 * ext["cqt high"]].copy()
        gap[len(gap) // 3:2 * len(gap) // 3] = 0.0
        k = constants()                                # tail tiles: T = CM_FR - 1 (CM_FR, CM_FR + 1 are "tail -1 / +1")
        parts.append(("tail frames -1", music[9 * SR:9 * SR + (k["CM_FR"] - 2) * 512 + 5]))
        parts.insert(4, ("zero", np.zeros(ext["decimate3 base 0"] + 1301, np.float32)))
        parts.insert(9, ("silent middle", gap))
        parts.insert(12, ("adversarial", adversarial(ext["decimate3 base 0"] + 291)))
        # three samples that end with the buffer: no 16-byte piece of such a chunk lies inside it
        parts.append(("last 3", (0.2 * rng.standard_normal(3)).astype(np.float32)))
        return _assemble(name, parts)
    if name == "tuning":
        n = 2 * ext["cqt high"] + 2048 * 5 + 1
        parts = [(f"detuned {i}", detuned((i + 0.5) / 100 - 0.5, n)) for i in TUNING_INDICES]
        parts.append(("detuned extra", detuned(EXTRA_DETUNE, n)))
        parts.insert(2, ("burst 1", burst([(27.5 * 2 ** ((186 + 0.2) / 36), 1.0)])))
        parts.insert(5, ("burst 2", burst([(27.5 * 2 ** ((180 - 0.3) / 36), 0.5), (27.5 * 2 ** ((198 + 0.3) / 36), 1.0)])))
        parts.insert(7, ("noise", (0.3 * rng.standard_normal(2048 * 12 - 1)).astype(np.float32)))
        parts.append(("periodic 512", np.tile((0.1 * rng.standard_normal(512)).astype(np.float32), 84)[:n]))
        return _assemble(name, parts)
    if name == "forced":
        n = ext["cqt high"] + 2048 * 5 + 1
        return _assemble(name, [("bank 49", detuned(-0.005, n)), ("zero residual", detuned(0.0, n)),
                                ("own peaks", detuned(0.245, n))])
    raise KeyError(name)


def forced_lists():
    """Peak lists handed to nc_chroma_mean_shared in the caller's buffers (every tuning frame of
    the chunk skipped), so tuning_select and the CQT behind it run at a tuning no stack of sines
    reaches through piptrack: residuals of -0.005 bins (index 49), and pitches of 27.5 * 2^k Hz,
    whose f32 residual is exactly 0 (bin 50 of np.histogram: edge 50 is 0.0).  Magnitudes all
    equal: the median selects every peak."""
    p49 = np.float32([27.5 * 2 ** ((m - 0.005) / 36) for m in range(100, 260, 7)])
    p0 = np.float32([220.0, 440.0, 880.0, 1760.0, 3520.0])
    return {"bank 49": (p49, np.ones_like(p49)), "zero residual": (p0, np.ones_like(p0))}


LAUNCHES = ("edges", "tuning")


def chunk_signal(L, c):
    return L.sig[c.off:c.off + c.len]
