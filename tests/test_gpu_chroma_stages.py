"""GPU parity of the chroma chain stage by stage (csrc/cqt.hip behind nc_chroma_mean): every
intermediate nc_chroma_mean leaves in its workspace is read back through
nc_chroma_workspace_layout and compared with the f64 reference of tests/chroma_stage_cases.py
evaluated on the DEVICE's own previous stage (level o from the device's level o - 1, CQT rows
of octave o from the device's level o at the device's tuning index, the tail from the
device's rows), so a failure names one kernel.  Three launches (chroma_stage_cases.launch):
"edges" (chunks one sample either side of every kernel's tile extent, lengths 1 .. 1023
between them, silence, three samples that end with the buffer), "tuning" (the detuned stacks
over the filter banks, > 64 peaks per frame, massive magnitude ties, lists of one and two
peaks) and "forced" (peak lists handed over through nc_chroma_mean_shared: tuning index 49 and
pitches whose residual is exactly 0).

Each test prints its worst figure against its bar (pytest -s).  The bars are derived in
chroma_stage_cases.py; test_chroma_stage_cases_cpu.py shows the reference alone inside them.

Measured on an MI355X (edges and tuning, 35 chunks; forced where named):
  plan                 exact
  levels 1-6           worst error / bound 0.126 level by level, 0.107 for the chain from level 0
  f16 exponents        largest max|level| 2^ex / 2^13 = 0.973; the adversarial chunk's level 1 reaches
                       1.000000 of sqrt(2) sum|h| max|level 0|
  peak lists           every count equal to the f64 reference's (0 unmatched on either side); matched
                       pitch 0.110 of its bar, magnitude 0.115 (bars: 16x yardsticks of ~1e-4 Hz and
                       ~1e-7 of the largest magnitude)
  tuning select        every index and margin inside the ambiguity allowance; lists of 0, 1, 2 peaks exact
  filter banks         the stacks land on 0, 1, 24, 25, 48, 50, 74, 98, 99 like the oracle; the forced
                       lists on 49 (margin 23) and, the residuals of exactly 0, on 50 (margin 5)
  CQT rows             worst metric / bar per device octave 0..6:
                       edges  0.138 0.161 0.136 0.187 0.173 0.134 0.109
                       tuning 0.174 0.181 0.171 0.194 0.187 0.329 0.095
                       forced 0.155 0.176 0.131 0.160 0.141 0.285 0.039
                       against 16x the yardstick ALONE (2.0e-6 .. 4.6e-6, median per octave):
                       edges  0.92 0.73 0.29 0.27 0.25 1.19 0.20
                       tuning 0.27 0.28 0.25 0.27 0.24 6.82 0.24
                       forced 0.24 0.26 0.18 0.23 0.18 6.91 0.29
  tail / finalize      worst 2.98e-08 against 2.38e-07; the silent chunk exact zeros
  shared producer      4 139 peaks in the first 429 frames from the window stage (oracle 4 139), a
                       sub-multiset of the unfused 8 477, bit for bit; completed lists identical

The row bar is NOT 16x the yardstick alone, and that was set after a device measurement: the
device exceeded it in device octave 5 (65-130 Hz), 1.19x on one 8-frame chunk and 2.5e-5 ..
3.3e-5 (5 .. 6.8x) on every detuned stack, whose sines start at 200 Hz so that octave 5 holds
only the noise floor, 4 .. 10 % of its level's amplitude.  The cause is the operand format,
not the kernels' arithmetic: the MFMA CQT splits each sample into f16 hi + lo at one
power-of-two scale per (chunk, octave), 22 significant bits of the level's largest sample,
while the oracle's complex64 path rounds an f64 FFT bin by bin, so its error (the yardstick)
follows each bin and the device's follows the level.  In units of max|level| x the filters' l2
gain the device's worst error per octave is 1.8e-7 .. 6.0e-7 over all chunks of both launches:
the 2^-21 of two 22-bit operands.  chroma_stage_cases.split_allowance adds exactly that term (derived from
the formats, not fitted) to the yardstick bar; ROW_CAP = 1e-4 bounds the sum.  The 1 024-term
f32 accumulation stays inside the yardstick term (it is relative to the accumulated value,
like the oracle's f32 matrix product).  The Gaussian bursts carry a tone at 0.05 in every
octave for the same reason: with an octave at -280 dB of its level no f32 implementation
holds 1e-4 of that octave's own maximum (measured before the tones were added: 4.7e-3).

Mutations (arithmetic only, one scratch build each, not committed), the new tests that catch
them and what test_gpu_chroma.py (the 2e-5 end-to-end mean) does:
  top octave's scale x 1.01 in cqt_mfma_low   test_cqt_rows_per_frame_and_octave (both launches);
                                              test_gpu_chroma.py fails 6 of 19 (dense peaks, the four
                                              amplitude scales, ragged chunks) and passes
                                              test_chroma_mean_and_tuning_match_oracle and the lags
  tail's octave sum skips the lowest octave   test_tail_and_finalize_from_the_devices_rows (both);
                                              test_gpu_chroma.py fails 10 of 19
  even-count median takes the lower middle    test_tuning_select_on_the_devices_own_peak_list[tuning]
                                              (the two-peak list: index 22 instead of 79);
                                              test_gpu_chroma.py passes all 19
  the tuning grid contracted into an fma      test_tuning_select_on_the_devices_own_peak_list (both: tuning
  again (the first defect below)              1.04e-17 at index 50) and test_forced_peak_lists_... (the
                                              zero residuals land on 49, margin 5); test_gpu_chroma.py
                                              passes all 19

Two more deviations from "16x the yardstick per case and octave", both in the bars' favour of
short lists: a chunk's row yardstick is never taken below the median of its launch's chunks
(chroma_stage_cases.row_bars), and a chunk's pitch / magnitude yardstick never below the
median of its launch's chunks with peaks (_peak_yards).  A list of one or two peaks, or a
chunk of one frame, has a yardstick of 0 or of a single rounding; the floor loosens the bar of
the chunks under the median, and the figures above (0.1 .. 0.33 of the bars) show no pressure
on it.

Two defects found and fixed with these tests:
  * the tuning grid value i * 0.01 - 0.5 was contracted into one fma on the device, so index 50
    (and every chunk without a peak) reported a tuning of 1.04e-17 instead of 0.0, and a
    residual of exactly 0 fell into bin 49 (cqt.hip tuning_edge; the "zero residual" list);
  * cqt_mfma_low staged a level of 1 to 3 samples with one clamped 16-byte load, up to 12
    bytes past the level: past the caller's buffer for a chunk under 4 samples that ends with
    it.  chroma_plan_kernel now copies every chunk's first four samples (zeros past its end)
    into a head slot of the workspace and points the CQT of level 0 at that slot for a chunk
    under 4 samples; cqt_mfma_low itself is unchanged (it has no register to spare: selecting
    the slot inside it spilled 68 bytes, which tests/test_kernel_resources_cpu.py refuses).
    The "last 3" chunk ends with the buffer; lengths 1, 2 and 3 give the same rows as before.
"""
from collections import Counter

import numpy as np
import pytest
import torch

import chroma_stage_cases as S
from oracle import ncref
from nightcore_analyzer import _dev

pytestmark = pytest.mark.gpu


class Run:
    """One nc_chroma_mean launch with every workspace section read back.  forced: chunk name ->
    (pitch, magnitude) lists handed over in caller-owned buffers through nc_chroma_mean_shared,
    with every tuning frame of those chunks skipped."""

    def __init__(self, ctx, L, forced=None):
        dev = _dev.device(0)
        self.L, self.n = L, len(L.chunks)
        n = self.n
        off = np.array([c.off for c in L.chunks], np.int64)
        ln = np.array([c.len for c in L.chunks], np.int64)
        self.len, total = ln, int(ln.sum())
        d_sig = _dev.to_dev(L.sig, dev, np.float32)
        d_off, d_len = _dev.to_dev(off, dev), _dev.to_dev(ln, dev)
        out = torch.full((n * 12,), float("nan"), dtype=torch.float32, device=dev)
        tun = _dev.empty(n, torch.float32, dev)
        tidx = _dev.empty(n, torch.int32, dev)
        tmg = _dev.empty(n, torch.int32, dev)
        wsb = ctx.lib.nc_chroma_workspace_bytes(ctx.h, n, total)
        ws = torch.full((wsb,), 0xff, dtype=torch.uint8, device=dev)      # an unwritten float reads as NaN
        lay = self.lay = S.layout(n, total)
        tfr = total // 512 + n
        if forced is None:
            ctx.call("nc_chroma_mean", d_sig.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total, int(ln.max()),
                     out.data_ptr(), tun.data_ptr(), tidx.data_ptr(), tmg.data_ptr(), ws.data_ptr(), wsb,
                     _dev.stream_handle())
        else:
            ntf = 1 + ln // 512
            tfb = np.concatenate([[0], np.cumsum(ntf)])
            pp = np.full(tfr * lay["kPeakSlots"], np.nan, np.float32)
            pm, npk, skip = pp.copy(), np.zeros(n, np.int32), np.zeros(n, np.int32)
            for c, ch in enumerate(L.chunks):
                if ch.name in forced:
                    p, m = forced[ch.name]
                    a = int(tfb[c]) * lay["kPeakSlots"]
                    pp[a:a + len(p)], pm[a:a + len(p)], npk[c], skip[c] = p, m, len(p), ntf[c]
            d_pp, d_pm, d_npk, d_skip = (_dev.to_dev(v, dev) for v in (pp, pm, npk, skip))
            ctx.call("nc_chroma_mean_shared", d_sig.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total,
                     int(ln.max()), out.data_ptr(), tun.data_ptr(), tidx.data_ptr(), tmg.data_ptr(), d_skip.data_ptr(),
                     int(skip.sum()), d_pp.data_ptr(), d_pm.data_ptr(), d_npk.data_ptr(), None, ws.data_ptr(), wsb,
                     _dev.stream_handle())
        torch.cuda.synchronize()
        self.out = out.cpu().numpy().reshape(n, 12)
        self.tun, self.tidx, self.margin = tun.cpu().numpy(), tidx.cpu().numpy(), tmg.cpu().numpy()
        buf = ws.cpu().numpy().tobytes()
        assert lay["bytes"] <= wsb
        sec = lambda name, dt, count: np.frombuffer(buf, dt, int(count), lay[name])
        self.oct_off = sec("oct_off", np.int64, 7 * n).reshape(n, 7)
        self.oct_len = sec("oct_len", np.int64, 7 * n).reshape(n, 7)
        self.n_frames = sec("n_frames", np.int32, n)
        self.n_tframes = sec("n_tframes", np.int32, n)
        self.npk = sec("chunk_npk", np.int32, n)
        self.tf_base = sec("tf_base", np.int64, n + 1)
        self.oct_ex = sec("oct_ex", np.int32, 7 * n).reshape(n, 7)
        self.head = sec("head", np.float32, 4 * n).reshape(n, 4)
        self._ws_oct = sec("ws_oct", np.float32, total + 64 * 7 * n)
        self._pp = sec("peak_pitch", np.float32, tfr * lay["kPeakSlots"])
        self._pm = sec("peak_mag", np.float32, tfr * lay["kPeakSlots"])
        self._gpart = sec("gpart", np.float32, tfr * 84).reshape(tfr, 7, 12)
        if forced is not None:                       # the lists live in the caller's buffers
            self.npk, self._pp, self._pm = d_npk.cpu().numpy(), d_pp.cpu().numpy(), d_pm.cpu().numpy()
        self._yard = None

    def level(self, c, o):
        """Device level o of chunk c, its oct_len values (level 0: the chunk itself)."""
        if o == 0:
            return S.chunk_signal(self.L, self.L.chunks[c])
        a = int(self.oct_off[c, o])
        return self._ws_oct[a:a + int(self.oct_len[c, o])]

    def peak_list(self, c):
        a = int(self.tf_base[c]) * self.lay["kPeakSlots"]
        return self._pp[a:a + int(self.npk[c])], self._pm[a:a + int(self.npk[c])]

    def gpart(self, c):
        a = int(self.tf_base[c])
        return self._gpart[a:a + int(self.n_frames[c])]

    def row_yardsticks(self):
        """[chunks, 7] at the device's levels and tuning (computed once, shared)."""
        if self._yard is None:
            self._yard = np.array([S.row_yardstick([self.level(c, o) for o in range(7)], S.tuning_value(int(self.tidx[c])),
                                                   int(self.n_frames[c])) for c in range(self.n)])
        return self._yard


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    return {ln: Run(gpu_ctx, S.launch(ln)) for ln in S.LAUNCHES}


def _named(r):
    return [(i, c.name) for i, c in enumerate(r.L.chunks)]


# --------------------------------------------------------------------------- plan
@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_plan_is_the_restatement_exactly(runs, ln):
    r = runs[ln]
    oct_len, oct_off, n_frames, n_tf, tf_base = S.plan(r.len)
    assert np.array_equal(r.oct_len, oct_len)
    assert np.array_equal(r.oct_off, oct_off)
    assert np.array_equal(r.n_frames, n_frames) and np.array_equal(r.n_tframes, n_tf)
    assert np.array_equal(r.tf_base, tf_base)
    assert 1 in n_frames.tolist()                       # chunks under 512 samples: one frame
    for c, ch in enumerate(r.L.chunks):                 # the head slots a chunk under 4 samples is read from
        want = np.zeros(4, np.float32)
        want[:min(4, ch.len)] = r.level(c, 0)[:4]
        assert np.array_equal(r.head[c], want), ch.name


# --------------------------------------------------------------------------- decimated levels
@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_every_level_follows_from_the_devices_previous_level(runs, ln):
    """decimate3 level by level: ncref.decimate2 of the device's level o - 1, inside the derived
    27 * 2^-24 * sqrt(2) sum|h| * max|level o - 1|; then the chain from level 0 against the
    oracle's own chain inside that bound compounded."""
    r, worst, worst_chain = runs[ln], 0.0, 0.0
    for c, name in _named(r):
        lev = [r.level(c, o) for o in range(7)]
        mx = [float(np.max(np.abs(v))) for v in lev]
        assert all(np.isfinite(m) for m in mx), (name, mx)
        chain, bounds = S.levels_oracle(lev[0]), S.chain_bounds(mx)
        for o in range(1, 7):
            ref = ncref.decimate2(lev[o - 1]).astype(np.float64)
            err, bar = float(np.max(np.abs(lev[o] - ref))), S.level_bound(mx[o - 1])
            assert err <= bar, (name, "level", o, err, bar)
            e2 = float(np.max(np.abs(lev[o].astype(np.float64) - chain[o])))
            assert e2 <= bounds[o], (name, "chain to level", o, e2, bounds[o])
            if bar:
                worst, worst_chain = max(worst, err / bar), max(worst_chain, e2 / bounds[o])
    print(f"{ln}: level error / bound, worst {worst:.3f}; chain from level 0, worst {worst_chain:.3f}")


def _gpow():
    g = S.level_gain() * (1.0 + 1e-4)
    return [np.float32(g ** o * (1.0 + 1e-4)) for o in range(7)]


@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_f16_split_exponents(runs, ln):
    """2^oct_ex scales level o for the f16 hi / lo split.  With m0 = max|level 0| and
    G_o = (sqrt(2) sum|h| (1 + 1e-4))^o (1 + 1e-4) >= the level's gain: the exponent is the one
    that puts m0 G_o 2^ex in [2^12, 2^13), so no sample of the device's level reaches 2^13 (the
    hi half would lose bits above 2^16 = f16 overflow after 3 bits of headroom) and no more than
    the bound's own slack is given away; 0 for a silent chunk."""
    r, gp, tight = runs[ln], _gpow(), 0.0
    for c, name in _named(r):
        m0 = np.float32(np.max(np.abs(r.level(c, 0))))
        for o in range(7):
            ex = int(r.oct_ex[c, o])
            if m0 == 0:
                assert ex == 0, (name, o, ex)
                continue
            bound = float(np.float32(m0 * gp[o]))
            assert ex == 100 or 2.0 ** 12 <= bound * 2.0 ** ex < 2.0 ** 13, (name, o, ex, bound)
            top = float(np.max(np.abs(r.level(c, o)))) * 2.0 ** ex
            assert top < 2.0 ** 13, (name, o, ex, top)
            tight = max(tight, top / 2.0 ** 13)
    print(f"{ln}: largest max|level| 2^ex / 2^13 = {tight:.4f}")
    if ln == "edges":        # the adversarial chunk attains the gain the bound rests on
        c = [i for i, nm in _named(r) if nm == "adversarial"][0]
        ratio = float(np.max(np.abs(r.level(c, 1))) / (S.level_gain() * np.max(np.abs(r.level(c, 0)))))
        print(f"adversarial: max|level 1| / (g max|level 0|) = {ratio:.6f}")
        assert 1.0 - 1e-3 <= ratio <= 1.0 + 1e-6


# --------------------------------------------------------------------------- peak lists
def _peak_yards(r):
    ys = [S.peak_yardstick(r.level(c, 0)) for c in range(r.n)]
    assert all(y is not None for y in ys)
    ys = np.array(ys)
    med = np.median(ys[ys[:, 0] > 0], axis=0)            # lists of a peak or two sample too few roundings
    return np.maximum(ys, med[None])


@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_peak_lists_match_piptrack_as_multisets(runs, ln):
    """tuning_peaks' unordered lists against ncref.piptrack's nonzero entries (f64 spectrum):
    the count within max(2, 0.2 %), matched pitches and magnitudes (2 |X| on the device) within
    16x the oracle's own f32-against-f64 movement of the same quantity."""
    r, yards = runs[ln], _peak_yards(runs[ln])
    worst = [0.0, 0.0]
    for c, name in _named(r):
        p, m = r.peak_list(c)
        rp, rm, per_frame = S.peaks(r.level(c, 0), f64=True)
        assert per_frame.max(initial=0) <= r.lay["kPeakSlots"]
        cap = S.peak_cap(len(rp))
        assert np.isfinite(p).all() and np.isfinite(m).all() and (p > 0).all(), name
        bar_p, bar_m = S.MARGIN * yards[c, 0], S.MARGIN * yards[c, 1]
        top = float(rm.max()) if len(rm) else 1.0
        ua, ub, dp = S.compare_sorted(p, rp, bar_p)
        va, vb, dm = S.compare_sorted(m.astype(np.float64) / 2.0 / top, rm / top, bar_m)
        assert max(ua, ub, va, vb) <= cap, (name, "unmatched", (ua, ub), (va, vb), "cap", cap, len(p), len(rp))
        assert dp <= bar_p and dm <= bar_m, (name, "pitch", dp, bar_p, "mag", dm, bar_m)
        if len(rp):
            worst = [max(worst[0], dp / bar_p), max(worst[1], dm / bar_m)]
    print(f"{ln}: matched peaks, pitch error / bar worst {worst[0]:.3f}, magnitude error / bar worst {worst[1]:.3f}; "
          f"counts {[int(v) for v in r.npk]}")


# --------------------------------------------------------------------------- tuning select
@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_tuning_select_on_the_devices_own_peak_list(runs, ln):
    """The radix median, the histogram and its argmax in isolation: ncref.tuning_counts at
    np.median of the device's magnitudes.  The only legitimate difference is an f32 residual
    within EDGE_EPS of a histogram edge landing in the neighbouring bin, two counts of margin
    per such peak, never more than max(2, 0.2 %): lists without such a peak are exact."""
    r, counts = runs[ln], []
    for c, name in _named(r):
        p, m = r.peak_list(c)
        idx, margin, amb = S.tuning_from_list(p, m)
        tol = min(S.peak_cap(len(p)), 2 * amb)
        got = (int(r.tidx[c]), int(r.margin[c]))
        assert abs(got[1] - margin) <= tol, (name, got, (idx, margin), tol)
        if margin > 2 * tol:
            assert got[0] == idx, (name, got, (idx, margin), tol)
        assert r.tun[c] == np.float32(S.tuning_value(got[0])), (name, r.tun[c], got)
        if not len(p):
            assert got == (50, 0) and r.tun[c] == 0.0, (name, got)
        counts.append(len(p))
    print(f"{ln}: tuning (index, margin) {[(int(i), int(g)) for i, g in zip(r.tidx, r.margin)]}")
    if ln == "tuning":
        assert {1, 2} <= set(counts)
        assert any(n > 2 and n % 2 for n in counts) and any(n > 2 and not n % 2 for n in counts)


def test_detuned_stacks_land_on_the_oracles_filter_banks(runs):
    r = runs["tuning"]
    seen = set()
    for c, name in _named(r):
        if name.startswith("detuned"):
            _, idx, margin = ncref.estimate_tuning_detail(r.level(c, 0))
            assert int(r.tidx[c]) == idx, (name, int(r.tidx[c]), idx, margin)
            seen.add(idx)
    assert seen == {0, 1, 24, 25, 48, 50, 74, 98, 99}, seen


# --------------------------------------------------------------------------- CQT rows
def _check_rows(r, ln):
    """gpart against the f64 evaluation of the oracle's filter bank on the device's level o at
    the device's tuning index, every frame of every chunk (first and last frames, both sides of
    every tile edge), per octave.  Per frame: max over the 12 columns of |G - R| over
    max(the frame's largest R, 1e-3 x the chunk's largest R in the octave) must stay under
    16x the run-time yardstick (chroma_stage_cases.row_bars) plus the f16 split's allowance
    (chroma_stage_cases.split_allowance, on the same scale), and never above ROW_CAP."""
    yard_bars = S.row_bars(r.row_yardsticks())
    worst, worst_yard = np.zeros(7), np.zeros(7)
    fails = []
    for c, name in _named(r):
        T, tun, G = int(r.n_frames[c]), S.tuning_value(int(r.tidx[c])), r.gpart(c)
        for o in range(7):
            lev = r.level(c, o)
            R = S.octave_rows(lev, o, tun, T, f64=True)
            met = S.row_metric(G[:, 6 - o, :], R)
            if not R.max() > 0:
                assert not met.any(), (name, o)          # silence: exact zeros
                continue
            scale = np.maximum(R.max(axis=1), S.ROW_FLOOR * R.max())
            bar = np.minimum(yard_bars[c, o] + S.split_allowance(np.max(np.abs(lev)), r.oct_ex[c, o], tun, o) / scale,
                             S.ROW_CAP)
            worst[o] = max(worst[o], float(np.max(met / bar)))
            worst_yard[o] = max(worst_yard[o], float(met.max() / yard_bars[c, o]))
            if not (met <= bar).all():
                t = int(np.argmax(met / bar))
                fails.append((name, "octave", o, "frame", t, float(met[t]), float(bar[t]), float(yard_bars[c, o])))
    print(f"{ln}: row metric / bar, worst per device octave 0..6: {np.round(worst, 3).tolist()}\n"
          f"  against 16x the yardstick alone: {np.round(worst_yard, 2).tolist()}; "
          f"16x yardstick, median per octave {[float('%.2g' % v) for v in np.median(yard_bars, axis=0)]}")
    assert not fails, fails


@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_cqt_rows_per_frame_and_octave(runs, ln):
    _check_rows(runs[ln], ln)


def test_forced_peak_lists_reach_bank_49_and_the_zero_residual(gpu_ctx):
    """Tuning index 49 and a residual of exactly 0 (chroma_stage_cases.forced_lists): the select
    on lists given in the caller's buffers, exactly (no residual near an edge but the zeros,
    which np.histogram puts in bin 50), a chunk beside them that keeps its own peaks, and the
    CQT rows of all three at the banks so chosen."""
    forced = S.forced_lists()
    r = Run(gpu_ctx, S.launch("forced"), forced)
    want = {"bank 49": 49, "zero residual": 50}
    for c, name in _named(r):
        p, m = r.peak_list(c)
        idx, margin, amb = S.tuning_from_list(p, m)
        if name in forced:
            assert np.array_equal(p, forced[name][0]) and idx == want[name] and margin == len(p), (name, idx, margin)
            assert (int(r.tidx[c]), int(r.margin[c])) == (idx, margin), (name, int(r.tidx[c]), int(r.margin[c]))
        else:
            rp = S.peaks(r.level(c, 0), f64=True)[0]
            oracle = ncref.estimate_tuning_detail(r.level(c, 0))[1]
            assert abs(len(p) - len(rp)) <= S.peak_cap(len(rp)) and int(r.tidx[c]) == idx == oracle, (name, len(p), idx)
        assert r.tun[c] == np.float32(S.tuning_value(int(r.tidx[c])))
    print(f"forced: tuning (index, margin) {[(int(i), int(g)) for i, g in zip(r.tidx, r.margin)]}")
    _check_rows(r, "forced")


# --------------------------------------------------------------------------- tail and finalize
@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_tail_and_finalize_from_the_devices_rows(runs, ln):
    r, worst = runs[ln], 0.0
    Ts = set()
    for c, name in _named(r):
        ref = S.tail(r.gpart(c))
        err = float(np.max(np.abs(r.out[c].astype(np.float64) - ref)))
        assert err <= S.TAIL_BAR, (name, err, S.TAIL_BAR)
        if not r.level(c, 0).any():
            assert np.all(r.out[c] == 0.0), name
        worst = max(worst, err)
        Ts.add(int(r.n_frames[c]))
    print(f"{ln}: out_chroma against the tail of the device's rows, worst {worst:.2e} (bar {S.TAIL_BAR:.2e})")
    if ln == "edges":
        cm = r.lay["CM_FR"]
        assert {1, cm - 1, cm, cm + 1} <= Ts, sorted(Ts)


# --------------------------------------------------------------------------- shared-tuning producer
def test_window_stage_and_chroma_chain_produce_the_same_peaks(gpu_ctx):
    """The two producers of a chunk's leading tuning frames: nc_window_stage_tuning appends the
    peaks of the first tp_frames frames of a chunk that starts where a 10 s window starts;
    nc_chroma_mean_shared adds the remaining frames (every frame of a chunk that starts at no
    window).  The window stage's (pitch, magnitude) pairs are a sub-multiset of the unfused
    nc_chroma_mean list, bit for bit, and the completed lists are the same multisets."""
    ctx, dev = gpu_ctx, _dev.device(0)
    y = S._music()
    win, cl = 220500, 441000
    chunks = [(0, cl), (100001, cl)]                       # window 0 starts chunk 0; no window starts chunk 1
    n, tp = 2, (win - 1024) // 512 + 1
    off, ln = np.array([c[0] for c in chunks], np.int64), np.array([c[1] for c in chunks], np.int64)
    total = int(ln.sum())
    d_sig, d_off, d_len = _dev.to_dev(y, dev, np.float32), _dev.to_dev(off, dev), _dev.to_dev(ln, dev)
    slots = S.constants()["kPeakSlots"]
    tfb = np.concatenate([[0], np.cumsum(1 + ln // 512)]).astype(np.int64)

    def pairs(pp, pm, npk, c):
        a = int(tfb[c]) * slots
        v = np.stack([pp[a:a + int(npk[c])], pm[a:a + int(npk[c])]], axis=1).view(np.uint32)
        return sorted(map(tuple, v.tolist()))

    # unfused
    lay = S.layout(n, total)
    wsb = ctx.lib.nc_chroma_workspace_bytes(ctx.h, n, total)
    ws = torch.full((wsb,), 0xff, dtype=torch.uint8, device=dev)
    out, tun = _dev.empty(n * 12, torch.float32, dev), _dev.empty(n, torch.float32, dev)
    ctx.call("nc_chroma_mean", d_sig.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total, cl, out.data_ptr(),
             tun.data_ptr(), None, None, ws.data_ptr(), wsb, _dev.stream_handle())
    torch.cuda.synchronize()
    buf = ws.cpu().numpy().tobytes()
    tfr = total // 512 + n
    u_npk = np.frombuffer(buf, np.int32, n, lay["chunk_npk"])
    u_pp = np.frombuffer(buf, np.float32, tfr * slots, lay["peak_pitch"])
    u_pm = np.frombuffer(buf, np.float32, tfr * slots, lay["peak_mag"])
    assert np.array_equal(np.frombuffer(buf, np.int64, n + 1, lay["tf_base"]), tfb)
    unfused = [pairs(u_pp, u_pm, u_npk, c) for c in range(n)]
    out_u, tun_u = out.cpu().numpy(), tun.cpu().numpy()

    # the window stage's share, caller-owned lists
    n_win, T, acw = 2, 1 + win // 512, 344
    w_off = _dev.to_dev(np.array([0, win // 2], np.int64), dev)
    w_chunk = _dev.to_dev(np.array([0, -1], np.int32), dev)
    d_tfb = _dev.to_dev(tfb, dev)
    pp = torch.full((int(tfb[n]) * slots,), float("nan"), dtype=torch.float32, device=dev)
    pm = torch.full((int(tfb[n]) * slots,), float("nan"), dtype=torch.float32, device=dev)
    npk = torch.zeros(n, dtype=torch.int32, device=dev)
    onset = _dev.empty(n_win * T, torch.float32, dev)
    tg = _dev.empty(n_win * acw, torch.float64, dev)
    en = _dev.empty(n_win, torch.float64, dev)
    wwsb = ctx.lib.nc_window_stage_workspace_bytes(ctx.h, n_win, win, 512)
    wws = _dev.workspace(wwsb, dev)
    ctx.call("nc_window_stage_tuning", d_sig.data_ptr(), w_off.data_ptr(), None, n_win, win, 512, onset.data_ptr(),
             tg.data_ptr(), en.data_ptr(), w_chunk.data_ptr(), d_tfb.data_ptr(), tp, pp.data_ptr(), pm.data_ptr(),
             npk.data_ptr(), None, wws.data_ptr(), wwsb, _dev.stream_handle())
    torch.cuda.synchronize()
    s_npk = npk.cpu().numpy().copy()
    staged = pairs(pp.cpu().numpy(), pm.cpu().numpy(), s_npk, 0)
    ref_first = int(S.peaks(y[:cl])[2][:tp].sum())
    print(f"window stage: {s_npk[0]} peaks in the first {tp} frames (oracle {ref_first}); unfused lists {u_npk.tolist()}")
    assert s_npk[1] == 0 and abs(int(s_npk[0]) - ref_first) <= S.peak_cap(ref_first)
    assert not Counter(staged) - Counter(unfused[0])        # a sub-multiset, bit for bit
    # the chain completes the lists
    skip = _dev.to_dev(np.array([tp, 0], np.int32), dev)
    ws.fill_(0xff)
    ctx.call("nc_chroma_mean_shared", d_sig.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total, cl, out.data_ptr(),
             tun.data_ptr(), None, None, skip.data_ptr(), tp, pp.data_ptr(), pm.data_ptr(), npk.data_ptr(), None,
             ws.data_ptr(), wsb, _dev.stream_handle())
    torch.cuda.synchronize()
    f_npk, f_pp, f_pm = npk.cpu().numpy(), pp.cpu().numpy(), pm.cpu().numpy()
    assert f_npk.tolist() == u_npk.tolist()
    for c in range(n):
        assert pairs(f_pp, f_pm, f_npk, c) == unfused[c], c
    assert np.array_equal(out.cpu().numpy(), out_u) and np.array_equal(tun.cpu().numpy(), tun_u)
