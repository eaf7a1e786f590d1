"""GPU parity of the beat tracker's two inputs at rounding level: the onset envelope and the
frame-averaged tempogram, through all four chains that produce them
  a. stft_mel_kernel -> wtg_onset (nc_window_stage): mel dB, frame maxima, onsets, energies;
  b. window_tg_kernel (six correlations) and window_tg_slide_kernel (sliding sums);
  c. nc_ibi_onset (hop 64 and 512, ragged batches);
  d. nc_ibi_tempogram / _tiles / _reduce on injected onsets,
against oracle/ncref.py.  Cases, yardsticks and emulations: tests/tempo_feature_cases.py
(qualified on the CPU by tests/test_tempo_feature_cases_cpu.py).

Tolerances.  f32 level (mel dB, onsets): max(4 f32 ulps of the case's largest magnitude,
8 x |oracle - oracle with a single-precision FFT| on that case; for the onsets the larger of
two such variants, the band mean in numpy's order and accumulated exactly, see
tempo_feature_cases.onset_yardstick).  f64 level (tempogram on the
kernel's own onset): min(2e-5, max(1e-12, 8 x |emulation - oracle| on that onset)); where the
plain emulation itself misses 2e-5 (loud, then exact zeros) the kernel is held to 2e-5 and to
the oracle's tempo lag.

Largest differences seen on an MI355X (GPU vs oracle), with the yardstick of that case:
  a. mel dB   5.7e-5 (yardstick 4.6e-5, tolerance 3.7e-4; 220500-sample window);
     onset    1.5e-5 (yardstick 1.1e-5, tolerance 9.2e-5; peak 25); nearest to its tolerance
              2.4e-6 of 3.8e-6; energies within 1e-9; frame maxima and silent windows exact.
  b. window tempogram, bounded dynamic range: 1e-15 .. 3.7e-9 (emulation 1e-15 .. 1.5e-6),
     nearest 1.0e-12 of 7.5e-12; windows that fall to exact zero: at most 6.1e-7, held to 2e-5
     (before the re-seeding rule: 5.7e-3 head T = 1300, 2.4e-5 gap(12, 12, 12) on the sliding
     sums, 1.6e-4 gap(6, 12, 6) on the correlations -- the three that missed).
  c. nc_ibi_onset 4.8e-6 (yardstick 4.8e-6, tolerance 3.8e-5), batch = single file bit for bit.
  d. nc_ibi_tempogram, bounded dynamic range: at most 8.1e-10 (emulation 1.2e-9); head and gap
     envelopes: at most 1.5e-7, held to 2e-5 (before: 3.4e-4 .. 9.7e-4 head at hop 64 for every
     T >= 2047, 2.2e-3 / 4.3e-3 gap at hop 64, 2.1e-4 gap T = 2049 at hop 512).
The gap envelope needs T >= N + 128 frames (N exact zeros between two stretches), so it runs at
T = 4096, 4097 for hop 64 and at T >= 2047 for hop 512.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import tempo_feature_cases as C
from oracle import ncref, refglue
from nightcore_analyzer import _dev
from nightcore_analyzer import engine as E

pytestmark = pytest.mark.gpu

SR = 22050
HOP = 512


def _a256(n):
    return (n + 255) & ~255


def _ctx(gpu_ctx, sr):
    return gpu_ctx if sr == SR else E.get_engine(0, sr=sr).ctx


# --------------------------------------------------------------------------- launchers
def run_window_stage(ctx, sig, offs, win_len, active=None, energy=True, fill=None):
    """nc_window_stage -> onset [n, T], tg [n, acw], energy [n], sdb [n, T, 128], frame_max [n, T]."""
    dev = _dev.device(0)
    d_sig = _dev.to_dev(sig if len(sig) else np.zeros(1, np.float32), dev, np.float32)
    d_off = _dev.to_dev(np.asarray(offs, np.int64), dev)
    d_act = None if active is None else _dev.to_dev(np.asarray(active, np.uint8), dev)
    n, T, acw = len(offs), 1 + win_len // HOP, ncref.ac_win_length(ctx.sr, HOP)
    onset = torch.full((n * T,), np.nan if fill is None else fill, dtype=torch.float32, device=dev)
    tg = torch.full((n * acw,), np.nan if fill is None else fill, dtype=torch.float64, device=dev)
    en = torch.full((n,), np.nan if fill is None else fill, dtype=torch.float64, device=dev)
    wsb = ctx.lib.nc_window_stage_workspace_bytes(ctx.h, n, win_len, HOP)
    ws = _dev.workspace(wsb, dev)
    ctx.call("nc_window_stage", d_sig.data_ptr(), d_off.data_ptr(), None if d_act is None else d_act.data_ptr(), n,
             win_len, HOP, onset.data_ptr(), tg.data_ptr(), en.data_ptr() if energy else None, ws.data_ptr(), wsb,
             _dev.stream_handle())
    torch.cuda.synchronize()
    F = n * T  # workspace layout: window_stage_ws_bytes (csrc/window_stage.hip)
    o1 = _a256(F * 128 * 4)
    sdb = ws[:F * 128 * 4].cpu().numpy().view(np.float32).reshape(n, T, 128)
    fmax = ws[o1:o1 + F * 4].cpu().numpy().view(np.float32).reshape(n, T)
    return (onset.cpu().numpy().reshape(n, T), tg.cpu().numpy().reshape(n, acw), en.cpu().numpy(), sdb, fmax)


def run_ibi_onset(ctx, files, hop, lead=3):
    """nc_ibi_onset on a ragged batch (files at odd offsets of one buffer) -> onsets, frame_base."""
    dev = _dev.device(0)
    lens = np.array([len(f) for f in files], np.int64)
    offs, parts, pos = [], [], 0
    for f in files:
        parts.append(np.zeros(lead, np.float32))
        pos += lead
        offs.append(pos)
        parts.append(f)
        pos += len(f)
    buf = _dev.to_dev(np.concatenate(parts + [np.zeros(8, np.float32)]), dev, np.float32)
    frames = 1 + lens // hop
    total, n = int(frames.sum()), len(files)
    d_off, d_len = _dev.to_dev(np.asarray(offs, np.int64), dev), _dev.to_dev(lens, dev)
    onset = torch.full((total,), np.nan, dtype=torch.float32, device=dev)
    fbase = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    wsb = ctx.lib.nc_ibi_onset_workspace_bytes(ctx.h, n, total)
    ws = _dev.workspace(wsb, dev)
    ctx.call("nc_ibi_onset", buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total, hop, onset.data_ptr(),
             fbase.data_ptr(), ws.data_ptr(), ws.numel(), _dev.stream_handle())
    torch.cuda.synchronize()
    fb = fbase.cpu().numpy()
    on = onset.cpu().numpy()
    return [on[fb[i]:fb[i + 1]] for i in range(n)] if fb[-1] == total else None, fb


class IbiTg:
    """nc_ibi_tempogram and its tile / reduce split on injected onsets."""

    def __init__(self, ctx, onsets, hop):
        self.ctx, self.hop, self.dev = ctx, hop, _dev.device(0)
        self.N = C.IBI_N[hop]
        T = np.array([len(o) for o in onsets], np.int64)
        self.n, self.total, self.tmax = len(onsets), int(T.sum()), int(T.max())
        self.n_tblk = (self.tmax + C.TILE - 1) // C.TILE
        self.onset = _dev.to_dev(np.concatenate(onsets), self.dev, np.float32)
        self.fb = _dev.to_dev(np.concatenate([[0], np.cumsum(T)]).astype(np.int64), self.dev)
        self.wsb = ctx.lib.nc_ibi_tempogram_workspace_bytes(ctx.h, self.n, self.total, self.tmax, hop)
        self.ws = _dev.workspace(self.wsb, self.dev)

    def _tg(self):
        return torch.full((self.n * self.N,), np.nan, dtype=torch.float64, device=self.dev)

    def whole(self):
        tg = self._tg()
        self.ctx.call("nc_ibi_tempogram", self.onset.data_ptr(), self.fb.data_ptr(), self.n, self.total, self.tmax,
                      self.hop, tg.data_ptr(), self.ws.data_ptr(), self.ws.numel(), _dev.stream_handle())
        torch.cuda.synchronize()
        return tg.cpu().numpy().reshape(self.n, self.N)

    def split(self, shares):
        """Tiles [b0, b1) of every file per share into one NaN-filled slab, then the reduce."""
        slab = torch.full((self.n * self.n_tblk * self.N,), np.nan, dtype=torch.float64, device=self.dev)
        for b0, b1 in shares:
            d0 = _dev.to_dev(np.full(self.n, b0, np.int64), self.dev)
            d1 = _dev.to_dev(np.full(self.n, b1, np.int64), self.dev)
            self.ctx.call("nc_ibi_tempogram_tiles", self.onset.data_ptr(), self.fb.data_ptr(), self.n, self.total,
                          self.tmax, self.hop, d0.data_ptr(), d1.data_ptr(), slab.data_ptr(),
                          self.ws.data_ptr(), self.ws.numel(), _dev.stream_handle())
            torch.cuda.synchronize()
        tg = self._tg()
        self.ctx.call("nc_ibi_tempogram_reduce", slab.data_ptr(), self.fb.data_ptr(), self.n, self.tmax, self.hop,
                      tg.data_ptr(), _dev.stream_handle())
        torch.cuda.synchronize()
        return tg.cpu().numpy().reshape(self.n, self.N)


# --------------------------------------------------------------------------- a. mel dB, onset, energy
def _check_window(tag, y, sr, onset, en, sdb, fmax):
    """One window's mel dB rows, frame maxima, onset and energy against the oracle."""
    S64, S32 = ncref.mel_db(y, sr, 2048, HOP), C.mel_db_f32(y, sr, HOP)
    assert np.array_equal(fmax, sdb.max(axis=1)), tag
    ref_db = C.clamp_db(S64)
    got_db = np.maximum(sdb.T, sdb.max() - np.float32(80.0))
    y_db = float(np.max(np.abs(ref_db - C.clamp_db(S32))))
    d_db = float(np.max(np.abs(got_db - ref_db)))
    ref_on = ncref.onset_strength(y, sr, HOP)
    y_on = C.onset_yardstick(ref_on, S32, HOP)
    d_on = float(np.max(np.abs(onset - ref_on)))
    t_db, t_on = C.tol_f32(y_db, np.max(np.abs(ref_db))), C.tol_f32(y_on, np.max(ref_on))
    print(f"[a] {tag}: mel dB {d_db:.2e} (yardstick {y_db:.2e}, tol {t_db:.2e})  "
          f"onset {d_on:.2e} (yardstick {y_on:.2e}, tol {t_on:.2e}, peak {np.max(ref_on):.2f})")
    assert np.isfinite(sdb).all() and np.isfinite(onset).all(), tag
    assert d_db <= t_db, (tag, "mel dB", d_db, t_db)
    assert d_on <= t_on, (tag, "onset", d_on, t_on)
    assert abs(en - refglue.rms_db(y)) < 1e-9, (tag, en, refglue.rms_db(y))


def _contents(n):
    m, c = C.music(n), C.clicks(n)
    return {"music": m, "music_1e-4": C.scaled(m, 1e-4), "music_30": C.scaled(m, 30), "clicks": c,
            "clicks_1e-4": C.scaled(c, 1e-4), "clicks_30": C.scaled(c, 30), "half_silent": C.half_silent(n)}


@pytest.mark.parametrize("win_len", C.WIN_LENS)
def test_mel_onset_energy_one_window_per_launch(gpu_ctx, win_len):
    for name, y in _contents(win_len).items():
        onset, tg, en, sdb, fmax = run_window_stage(gpu_ctx, y, [0], win_len)
        assert np.isfinite(tg).all()
        _check_window(f"L={win_len} {name}", y, SR, onset[0], en[0], sdb[0], fmax[0])


@pytest.mark.parametrize("win_len", C.WIN_LENS)
def test_mel_onset_energy_17_overlapping_windows(gpu_ctx, win_len):
    """17 windows of one launch, overlapping, at odd sample offsets, across stretches of very
    different level: every window is clamped against its own maximum."""
    L = win_len
    sig = np.concatenate([C.music(L), C.scaled(C.clicks(L), 30), C.scaled(C.music(L), 1e-4), C.music(64)])
    offs = [((i * (2 * L + 40)) // 16) | 1 for i in range(17)]
    assert max(offs) + L <= len(sig) and all(o & 1 for o in offs)
    onset, tg, en, sdb, fmax = run_window_stage(gpu_ctx, sig, offs, L)
    assert np.isfinite(tg).all()
    for i, o in enumerate(offs):
        _check_window(f"L={L} window {i}@{o}", sig[o:o + L], SR, onset[i], en[i], sdb[i], fmax[i])


@pytest.mark.parametrize("win_len", [1, 512, 3073, 220500])
def test_silent_window_is_exact(gpu_ctx, win_len):
    onset, tg, en, sdb, fmax = run_window_stage(gpu_ctx, C.silent(win_len), [0], win_len)
    print(f"[a] silent L={win_len}: energy {en[0]!r}, mel dB in [{sdb.min()!r}, {sdb.max()!r}]")
    assert not onset.any() and not tg.any()
    assert en[0] == 20.0 * np.log10(1e-10)
    assert np.array_equal(fmax, sdb.max(axis=2)) and np.max(np.abs(sdb + 100.0)) <= 4 * C.ulp32(100.0)


@pytest.mark.parametrize("win_len", [3073, 220500])
def test_active_mask_and_null_energy(gpu_ctx, win_len):
    sig = C.music(win_len * 3 + 8)
    offs = [1 + i * (win_len // 2) for i in range(5)]
    mask = [1, 0, 1, 1, 0]
    full = run_window_stage(gpu_ctx, sig, offs, win_len)
    part = run_window_stage(gpu_ctx, sig, offs, win_len, active=mask)
    noen = run_window_stage(gpu_ctx, sig, offs, win_len, energy=False)
    for i, a in enumerate(mask):
        for q in range(3):
            if a:
                assert np.array_equal(part[q][i], full[q][i]), (i, q)
            else:
                assert np.isnan(part[q][i]).all(), (i, q)
    assert np.array_equal(noen[0], full[0]) and np.array_equal(noen[1], full[1])
    assert np.isnan(noen[2]).all() and np.isfinite(full[2]).all()


# --------------------------------------------------------------------------- b. window tempogram
def _check_window_tg(gpu_ctx, sr, tag, y, lag=False):
    """tg_out against the oracle's tempogram of the kernel's own onset (f64 level)."""
    ctx, acw = _ctx(gpu_ctx, sr), C.RATES[sr]
    win_len = len(y)
    T = 1 + win_len // HOP
    onset, tg, en, _, _ = run_window_stage(ctx, y, [0], win_len)
    onset, tg = onset[0], tg[0]
    assert np.isfinite(onset).all() and np.isfinite(tg).all(), tag
    ref = ncref.tempogram_mean(onset, acw)
    # the emulation of the path this window takes: window_tg_kernel's six correlations while they
    # fit in LDS and the normalisers span less than WTG_SPREAD, else the sliding sums (both near
    # the threshold, where the kernel's own sums decide)
    spread = C.ac0_spread(onset, acw)
    corr = C.uses_correlation(T, acw)
    d_emu = 0.0
    if corr and spread <= 4 * C.WTG_SPREAD:
        d_emu = float(np.max(np.abs(C.correlation_tempogram_mean(onset, acw) - ref)))
    if not corr or spread >= C.WTG_SPREAD / 4:
        d_emu = max(d_emu, float(np.max(np.abs(C.sliding_tempogram_mean(onset, acw, tile=C.TILE) - ref))))
    d = float(np.max(np.abs(tg - ref)))
    tol = C.tol_f64(d_emu)
    print(f"[b] {sr} Hz T={T} {'corr' if corr else 'slide'} {tag}: {d:.2e} (emulation {d_emu:.2e}, tol {tol:.2e}, "
          f"ac0 spread {spread:.1e})")
    assert d <= tol, (tag, d, tol, int(np.argmax(np.abs(tg - ref))))
    if lag:
        assert ncref.tempo_from_tg(tg, sr, HOP)[1] == ncref.tempo_from_tg(ref, sr, HOP)[1], tag


@pytest.mark.parametrize("sr,T", [(sr, T) for sr, Ts in C.WINDOW_T.items() for T in Ts])
def test_window_tempogram_matches_oracle_on_own_onset(gpu_ctx, sr, T):
    n = (T - 1) * HOP
    _check_window_tg(gpu_ctx, sr, "music", C.music(n), lag=T >= 431)
    if T >= 64:
        _check_window_tg(gpu_ctx, sr, "head", C.head(n), lag=True)
        _check_window_tg(gpu_ctx, sr, "quiet_tail", C.quiet_tail(n))


def test_window_tempogram_gap_24s_correlation_kernel(gpu_ctx):
    assert C.uses_correlation(1034, 344)
    _check_window_tg(gpu_ctx, SR, "gap(6, 12, 6)", C.gap(SR, 6, 12, 6, 1033 * HOP), lag=True)


def test_window_tempogram_gap_36s_slide_kernel(gpu_ctx):
    assert not C.uses_correlation(1551, 344)
    _check_window_tg(gpu_ctx, SR, "gap(12, 12, 12)", C.gap(SR, 12, 12, 12, 1550 * HOP), lag=True)


def test_window_tempogram_content_ends_after_one_second(gpu_ctx):
    _check_window_tg(gpu_ctx, SR, "first second", C.first_second(220500, SR), lag=True)


# --------------------------------------------------------------------------- c. nc_ibi_onset
def _ibi_files():
    scale = [1.0, 30.0, 1e-3, 1.0, 30.0, 1e-3, 1.0]
    return [C.scaled(C.music(n, start=1000 * i), s) for i, (n, s) in enumerate(zip(C.IBI_LENS, scale))]


@pytest.mark.parametrize("hop", [64, 512])
def test_ibi_onset_ragged_batch(gpu_ctx, hop):
    files = _ibi_files()
    ons, fb = run_ibi_onset(gpu_ctx, files, hop)
    assert np.array_equal(fb, np.concatenate([[0], np.cumsum([1 + len(f) // hop for f in files])]))
    for i, y in enumerate(files):
        S64, S32 = ncref.mel_db(y, SR, 2048, hop), C.mel_db_f32(y, SR, hop)
        ref = ncref.onset_strength(y, SR, hop)
        yard = C.onset_yardstick(ref, S32, hop)
        d, tol = float(np.max(np.abs(ons[i] - ref))), C.tol_f32(yard, np.max(ref))
        print(f"[c] hop {hop} file {i} len {len(y)}: onset {d:.2e} (yardstick {yard:.2e}, tol {tol:.2e}, "
              f"peak {np.max(ref):.2f})")
        assert ons[i].shape == ref.shape and np.isfinite(ons[i]).all()
        assert d <= tol, (i, d, tol)
        alone, fb1 = run_ibi_onset(gpu_ctx, [y], hop, lead=0)
        assert np.array_equal(fb1, [0, len(ref)]) and np.array_equal(alone[0], ons[i]), i


@pytest.mark.parametrize("hop", [64, 512])
def test_ibi_onset_short_files_between_long_ones(gpu_ctx, hop):
    """A 41-frame file first, so every wave of the STFT workgroup has looked its file up once; then
    six files of 1 to 4 frames, so a wave's next frame lies several files ahead and its segment
    cursor advances more than one step (with the tiny files first, as in the ragged batch above,
    every first lookup is the search); a second long file ends the batch."""
    lens = (40 * hop, 0, 1, hop, hop + 1, 0, 3 * hop, 40 * hop)
    scale = [1.0, 30.0, 1e-3, 1.0, 30.0, 1e-3, 1.0, 30.0]
    files = [C.scaled(C.music(n, start=1000 * i), s) for i, (n, s) in enumerate(zip(lens, scale))]
    ons, fb = run_ibi_onset(gpu_ctx, files, hop)
    assert np.array_equal(fb, np.concatenate([[0], np.cumsum([1 + n // hop for n in lens])]))
    for i, y in enumerate(files):
        ref = ncref.onset_strength(y, SR, hop)
        yard = C.onset_yardstick(ref, C.mel_db_f32(y, SR, hop), hop)
        d, tol = float(np.max(np.abs(ons[i] - ref))), C.tol_f32(yard, np.max(ref))
        print(f"[c] hop {hop} file {i} len {len(y)}: onset {d:.2e} (yardstick {yard:.2e}, tol {tol:.2e})")
        assert ons[i].shape == ref.shape and np.isfinite(ons[i]).all()
        assert d <= tol, (i, d, tol)
        alone, fb1 = run_ibi_onset(gpu_ctx, [y], hop, lead=0)
        assert np.array_equal(fb1, [0, len(ref)]) and np.array_equal(alone[0], ons[i]), i


def test_ibi_onset_short_files_deep_in_a_workgroup_range(gpu_ctx):
    """The same six short files between two of ~6 100 frames (hop 64): 12 299 frames, so that on a
    chip of up to 256 CUs a workgroup's share (48 frames) exceeds its 16 waves, and the short
    files start 24 frames into the share of the workgroup that meets them: each of its waves has
    a file already and steps its cursor up to seven files forward.  Batch = alone, bit for bit
    (the oracle comparison of such files is test_ibi_onset_ragged_batch's)."""
    hop = 64
    lens = (6167 * hop, 0, 1, hop, hop + 1, 0, 3 * hop, 6119 * hop)
    starts = (0, 1000, 2000, 3000, 4000, 5000, 6000, 400000)
    files = [C.music(n, start=s) for n, s in zip(lens, starts)]
    ons, fb = run_ibi_onset(gpu_ctx, files, hop)
    assert np.array_equal(fb, np.concatenate([[0], np.cumsum([1 + n // hop for n in lens])]))
    for i, y in enumerate(files):
        alone, _ = run_ibi_onset(gpu_ctx, [y], hop, lead=0)
        assert np.isfinite(ons[i]).all() and np.array_equal(alone[0], ons[i]), i


# --------------------------------------------------------------------------- d. nc_ibi_tempogram
@lru_cache(maxsize=None)
def _env_ref(kind, T, N):
    """(envelope, oracle tempogram, |tiled plain sliding emulation - oracle|), computed once."""
    o = C.envelope(kind, T, N)
    if kind == "zero":
        return o, np.zeros(N), 0.0
    ref = ncref.tempogram_mean(o, N)
    d = float(np.max(np.abs(C.sliding_tempogram_mean(o, N, tile=C.TILE) - ref)))
    for a in (o, ref):
        a.setflags(write=False)
    return o, ref, d


def _check_env(tag, kind, hop, tg, ref, d_emu):
    assert np.isfinite(tg).all(), tag
    if kind == "zero":
        assert not tg.any(), tag
        return
    d, tol = float(np.max(np.abs(tg - ref))), C.tol_f64(d_emu)
    print(f"[d] hop {hop} {tag}: {d:.2e} (emulation {d_emu:.2e}, tol {tol:.2e})")
    assert d <= tol, (tag, d, tol, int(np.argmax(np.abs(tg - ref))))
    if kind in C.ILL:
        assert ncref.tempo_from_tg(tg, SR, hop)[1] == ncref.tempo_from_tg(ref, SR, hop)[1], tag


def _d_cases():
    return [(hop, kind, T) for hop, N in C.IBI_N.items() for kind in C.ENVELOPES for T in C.IBI_T
            if kind != "gap" or C.env_gap_fits(T, N)]


@pytest.mark.parametrize("hop,kind,T", _d_cases())
def test_ibi_tempogram_one_file(gpu_ctx, hop, kind, T):
    o, ref, d_emu = _env_ref(kind, T, C.IBI_N[hop])
    tg = IbiTg(gpu_ctx, [o], hop).whole()
    _check_env(f"{kind} T={T}", kind, hop, tg[0], ref, d_emu)


@pytest.mark.parametrize("hop", [64, 512])
@pytest.mark.parametrize("kind", C.ENVELOPES)
def test_ibi_tempogram_ragged_batch(gpu_ctx, hop, kind):
    """T = 1 beside T = 4097 in one launch: the same bits as one file at a time."""
    N = C.IBI_N[hop]
    Ts = [T for T in (4097, 1, 2, 2047, 4096, 2049, 2048) if kind != "gap" or C.env_gap_fits(T, N)]
    cases = [_env_ref(kind, T, N) for T in Ts]
    tg = IbiTg(gpu_ctx, [c[0] for c in cases], hop).whole()
    for i, (T, (o, ref, d_emu)) in enumerate(zip(Ts, cases)):
        _check_env(f"batch {kind} T={T}", kind, hop, tg[i], ref, d_emu)
        assert np.array_equal(tg[i], IbiTg(gpu_ctx, [o], hop).whole()[0]), (kind, T)


@pytest.mark.parametrize("hop", [64, 512])
@pytest.mark.parametrize("kind", ["sparse", "head", "gap"])
def test_ibi_tempogram_tile_shares_reduce_to_the_same_bits(gpu_ctx, hop, kind):
    """The three tiles of T = 4097 computed by three separate calls into one slab, then the
    fixed-order reduce: bit-identical to nc_ibi_tempogram (a sharded run's contract), also
    where the sliding sums re-seed inside a tile."""
    o, _, _ = _env_ref(kind, 4097, C.IBI_N[hop])
    tg = IbiTg(gpu_ctx, [o, o[:2049]], hop)
    whole = tg.whole()
    assert np.isfinite(whole).all()
    assert np.array_equal(tg.split([(2, 3), (0, 1), (1, 2)]), whole)
