"""GPU parity of the intro-offset search (csrc/align.hip behind nc_align_offsets) against the
per-speed oracle of tests/align_cases.py (qualified on the CPU by test_align_cases_cpu.py), with
peak, speed index and score all read back.

Decisions (skipped or not, the peak of every speed, the winning speed) are demanded exactly: the
CPU qualification shows that each stands at least 1e-6 clear of the alternative, some hundred
times the yardstick.  Scores are held to 16 x the yardstick, the score difference between the
oracle's f32 envelope mean and the f64 one the kernel takes (align_cases.yardstick(), computed
at run time: 4.8e-9, so the bar is 7.6e-8).  Scores the 1e-12 denominator gate sets to 0.0, and
the -1.0 of a pair with no searchable speed, are demanded exactly.

Largest |GPU score - oracle score| seen on an MI355X (each test prints its figures, pytest -s):
per speed 4.78e-9 (nc_6_frames; every case lands on its own yardstick, 2.0e-9 .. 4.8e-9, to the
digits printed, so the GPU sits on the f64-mean evaluation), whole grid 2.63e-9, against the
yardstick 4.78e-9 and the bar 7.64e-8.  Peaks, skips and winners: all exact.  The distance to
the f64-mean evaluation, printed beside it, is at most 1.7e-15.

What these tests catch that the golden pairs and the pipeline golden do not (each change
built and run once on an MI355X, none of them caught by the earlier tests): the LDS tile of
align_corr_kernel staged one element short (the quiet case per speed, lag_cap in every batch);
'>=' over the speeds in align_select_kernel (nc_1s, whose first two speeds tie bit for bit); the
decimator's scalar branch reading in[i] for in[i + 1] (the sample-alignment test).  Not caught,
here or anywhere: al_lin without its exact end point.  It moves one stretched sample by an ulp
and every printed figure, down to 1e-16, stays as it is, so no tolerance that allows for the
envelope's own rounding can see it through this entry point.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import align_cases as A
from nightcore_analyzer import _dev
from nightcore_analyzer import engine as E

pytestmark = pytest.mark.gpu

UNTOUCHED = (-77, -78, -79.0)       # what the outputs hold before a call


class Batch:
    """(src, nc) pairs in one device buffer, every file `shift` samples past a 64-sample boundary."""

    def __init__(self, pairs, shift=0):
        self.dev = _dev.device(0)
        files = [a for p in pairs for a in p]
        off, pos = [], 0
        for a in files:
            off.append(pos + shift)
            pos += (len(a) + shift + 63) // 64 * 64
        host = np.zeros(pos + 64, np.float32)
        for a, o in zip(files, off):
            host[o:o + len(a)] = a
        self.n = len(pairs)
        self.buf = _dev.to_dev(host, self.dev, np.float32)
        self.off = np.array(off, np.int64)
        self.len = np.array([len(a) for a in files], np.int64)
        self.d = {k: _dev.to_dev(v, self.dev) for k, v in
                  (("so", self.off[0::2]), ("sl", self.len[0::2]), ("no", self.off[1::2]), ("nl", self.len[1::2]))}
        self.tot, self.mx = int(self.len.sum()), int(max(1, self.len.max()))

    def ws_bytes(self, ctx, n_speeds):
        return int(ctx.lib.nc_align_workspace_bytes(ctx.h, self.n, n_speeds, self.tot, self.mx, A.MAX_FRAMES))

    def run(self, ctx, speeds, ws=None, ws_bytes=None, n_pairs=None, n_speeds=None):
        """-> (rc, peak[n], speed_idx[n], score[n]); ws: a uint8 tensor (default: a fresh one)."""
        speeds = np.atleast_1d(np.asarray(speeds, np.float64))
        ns = len(speeds) if n_speeds is None else n_speeds
        d_sp = _dev.to_dev(speeds, self.dev)
        peak = torch.full((self.n,), UNTOUCHED[0], dtype=torch.int32, device=self.dev)
        idx = torch.full((self.n,), UNTOUCHED[1], dtype=torch.int32, device=self.dev)
        score = torch.full((self.n,), UNTOUCHED[2], dtype=torch.float64, device=self.dev)
        if ws is None:
            ws = _dev.workspace(self.ws_bytes(ctx, max(1, ns)), self.dev)
        rc = ctx.lib.nc_align_offsets(ctx.h, self.buf.data_ptr(), self.d["so"].data_ptr(), self.d["sl"].data_ptr(),
                                      self.d["no"].data_ptr(), self.d["nl"].data_ptr(),
                                      self.n if n_pairs is None else n_pairs, d_sp.data_ptr(), ns, A.MAX_FRAMES,
                                      self.tot, self.mx, peak.data_ptr(), idx.data_ptr(), score.data_ptr(),
                                      ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                      _dev.stream_handle())
        torch.cuda.synchronize()
        return rc, peak.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()


def _check_score(tag, got, ref):
    """Scores the gate or the all-skipped path sets are exact; the others within the tolerance."""
    if ref in (0.0, -1.0):
        assert got == ref, (tag, got, ref)
        return 0.0
    d = abs(got - ref)
    assert d <= A.score_tol(), (tag, got, ref, d, A.score_tol())
    return d


@lru_cache(maxsize=None)
def _all_pairs():
    return tuple(A.signals(n) for n in A.NAMES)


def _check_winners(tag, names, got, g=A.GRID_REF):
    rc, peak, idx, score = got
    assert rc == 0, tag
    worst = 0.0
    for i, n in enumerate(names):
        w = A.oracle(n, g).winner
        assert (int(peak[i]), int(idx[i])) == w[:2], (tag, n, int(peak[i]), int(idx[i]), w)
        worst = max(worst, _check_score((tag, n), float(score[i]), float(w[2])))
    return worst


# --------------------------------------------------------------------------- per speed
@pytest.mark.parametrize("name,g", A.RUNS)
def test_every_speed_alone(gpu_ctx, name, g):
    """One call per speed of the grid with n_speeds = 1: that speed's own peak and score."""
    b = Batch([A.signals(name)])
    ev, ex = A.oracle(name, g), A.oracle(name, g, True)
    ws = _dev.workspace(b.ws_bytes(gpu_ctx, 1), b.dev)
    worst, worst_ex, n_cmp = 0.0, 0.0, 0
    for i, (speed, s) in enumerate(zip(A.grid(g), ev.speeds)):
        rc, peak, idx, score = b.run(gpu_ctx, [speed], ws=ws)
        assert rc == 0
        got = (int(peak[0]), int(idx[0]), float(score[0]))
        if s.skipped:
            assert got == (0, -1, -1.0), (name, i, got)
        else:
            assert got[:2] == (s.peak, 0), (name, i, got, s)
            worst = max(worst, _check_score((name, i), got[2], s.score))
            worst_ex = max(worst_ex, abs(got[2] - ex.speeds[i].score))
        n_cmp += 1
    assert n_cmp == g[2]
    print(f"[per speed] {name} {g}: largest score difference {worst:.2e} (case yardstick "
          f"{A.case_yardstick(name, g):.2e}, yardstick {A.yardstick():.2e}, tolerance {A.score_tol():.2e}); "
          f"from the evaluation with the f64 envelope mean {worst_ex:.2e}")


# --------------------------------------------------------------------------- whole grid
def test_whole_grid_ragged_batch_and_reversed(gpu_ctx):
    """All cases in one call (strides and grids from the longest file), then in reverse order."""
    pairs = _all_pairs()
    speeds = A.grid(A.GRID_REF)
    fwd = Batch(pairs).run(gpu_ctx, speeds)
    worst = _check_winners("batch", A.NAMES, fwd)
    rev = Batch(pairs[::-1]).run(gpu_ctx, speeds)
    _check_winners("reversed", A.NAMES[::-1], rev)
    for q in (1, 2, 3):
        assert np.array_equal(rev[q][::-1], fwd[q]), q
    print(f"[whole grid] largest score difference {worst:.2e} (yardstick {A.yardstick():.2e}, "
          f"tolerance {A.score_tol():.2e})")


@pytest.mark.parametrize("g", [A.GRID_WIDE, A.GRID_MIXED])
def test_whole_grid_other_speed_grids(gpu_ctx, g):
    worst = _check_winners(f"grid {g}", ["golden60"], Batch([A.signals("golden60")]).run(gpu_ctx, A.grid(g)), g)
    print(f"[whole grid] golden60 {g}: score difference {worst:.2e}")


def test_engine_maps_peak_and_speed_index(gpu_ctx):
    """Engine.align_offsets on the same batch: (peak * hop_sec, speeds[idx]), and the reference's
    (0.0, (lo + hi) / 2) where no speed is searchable."""
    eng = E.get_engine(0)
    b = Batch(_all_pairs())
    got = eng.align_offsets(b.buf, b.off[0::2], b.len[0::2], b.off[1::2], b.len[1::2])
    speeds = A.grid(A.GRID_REF)
    exp = []
    for n in A.NAMES:
        w = A.oracle(n).winner
        exp.append((0.0, (A.GRID_REF[0] + A.GRID_REF[1]) / 2.0) if w[1] < 0 else (w[0] * A.HOP_SEC, float(speeds[w[1]])))
    assert got == exp
    mid = (A.GRID_REF[0] + A.GRID_REF[1]) / 2.0
    assert [got[A.NAMES.index(n)] for n in A.ALL_SKIPPED] == [(0.0, mid)] * 2


def test_sample_alignment_does_not_change_a_bit(gpu_ctx):
    """Files 1, 2 and 3 samples past a 64-sample boundary (2 keeps the decimator's float2 loads,
    1 and 3 take its scalar branch): the same bits as the aligned batch."""
    pairs = _all_pairs()
    speeds = A.grid(A.GRID_REF)
    ref = Batch(pairs).run(gpu_ctx, speeds)
    _check_winners("aligned", A.NAMES, ref)
    for shift in (1, 2, 3):
        got = Batch(pairs, shift).run(gpu_ctx, speeds)
        assert got[0] == 0
        for q in (1, 2, 3):
            assert np.array_equal(got[q], ref[q]), (shift, q, got[q], ref[q])


# --------------------------------------------------------------------------- workspace and refusals
def test_workspace_contents_size_and_refusals(gpu_ctx):
    pairs = _all_pairs()
    speeds = A.grid(A.GRID_REF)
    b = Batch(pairs)
    need = b.ws_bytes(gpu_ctx, len(speeds))
    lead, guard = 256, 4096
    slab = torch.empty(lead + need + guard + 256, dtype=torch.uint8, device=b.dev)
    ws = slab[lead:lead + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    ref = None
    for fill in (0x00, 0xFF, 0x7F):
        slab.fill_(0xA5)
        ws.fill_(fill)
        got = b.run(gpu_ctx, speeds, ws=ws)
        _check_winners(f"fill {fill:#x}", A.NAMES, got)
        after = slab.cpu().numpy()
        assert (after[:lead] == 0xA5).all() and (after[lead + need:] == 0xA5).all(), fill
        if ref is None:
            ref = got
        for q in (1, 2, 3):
            assert np.array_equal(got[q], ref[q]), (fill, q)
    untouched = ([UNTOUCHED[0]] * b.n, [UNTOUCHED[1]] * b.n, [UNTOUCHED[2]] * b.n)

    def refused(rc_exp, **kw):
        rc, peak, idx, score = b.run(gpu_ctx, speeds, ws=ws, **kw)
        assert rc == rc_exp, (kw, rc)
        assert (peak.tolist(), idx.tolist(), score.tolist()) == untouched, kw

    refused(-3, ws_bytes=need - 1)
    assert b"workspace" in gpu_ctx.lib.nc_last_error()
    refused(-2, n_speeds=0)
    refused(0, n_pairs=0)
    # and the exact size is enough
    _check_winners("exact size", A.NAMES, b.run(gpu_ctx, speeds, ws=ws, ws_bytes=need))
