"""GPU parity of the waveform speed search (csrc/xcorr.hip behind nc_xcorr_search) against
refglue.estimate_speed_xcorr_arrays on the cases of tests/xcorr_search_cases.py (qualified on
the CPU by test_xcorr_search_cases_cpu.py): 3 to 200 windows per search at two window lengths
that are no multiple of 256, both gates, fewer than 3 matches, best <= 0, exact ties, and 130
jobs of different window counts in one launch.

Bars: those of test_gpu_components.test_xcorr_speed_matches_oracle, ratio within 1e-9 and
quality within 1e-5; results the reference sets to (1.0, 0.0) are demanded exactly.  The CPU
qualification shows every candidate decision standing at least 3.6e-5 clear, against 7.7e-8
between the reference's f32 dot products and f64 ones.

Seen on an MI355X: largest ratio difference 6.7e-16, largest quality difference 7.7e-8
(figures printed by each test, pytest -s).  Before xcorr_finalize_kernel kept every
correspondence (it held at most 64 per job), the 65-, 80- and 200-window cases missed the ratio
bar by 1.8e-3 .. 3.0e-2 at both window lengths (the device returned exactly the fit through
the first 64 correspondences, as test_xcorr_search_cases_cpu.py computes it).  '>=' for the
strict '>' over a window's candidates fails the tied case here (ratio off by 2.3e-7) and
passes test_gpu_components.test_xcorr_speed_matches_oracle.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import xcorr_search_cases as X
from nightcore_analyzer import _dev, ops, xcorr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from nightcore_analyzer import engine as E
    return E.get_engine(0)


def _check(tag, got, ref):
    if ref == (1.0, 0.0):
        assert got == ref, (tag, got, ref)
        return 0.0, 0.0
    dr, dq = abs(got[0] - ref[0]), abs(got[1] - ref[1])
    print(f"[xcorr] {tag}: ratio {got[0]:.9f} (oracle {ref[0]:.9f}, difference {dr:.1e}), "
          f"quality difference {dq:.1e}")
    assert dr < X.RATIO_TOL and dq < X.QUALITY_TOL, (tag, got, ref)
    return dr, dq


@lru_cache(maxsize=None)
def _reference(name):
    return X.reference(name)


@pytest.mark.parametrize("name", X.NAMES)
def test_drop_in_matches_oracle(eng, name):
    k = X.CASES[name]
    got = xcorr.estimate_speed_xcorr_arrays(k.ya, k.yb, X.SR, k.n_windows, k.window_sec, k.search_range)
    _check(name, got, _reference(name))


# --------------------------------------------------------------------------- many jobs, one launch
class Jobs:
    """nc_xcorr_search on a list of cases (all of one window length) as one launch: the
    geometry of ops.xcorr_speed per job, every job with items of its own."""

    def __init__(self, names):
        win = {int(X.CASES[n].window_sec * X.SR) for n in names}
        assert len(win) == 1
        self.win, self.names = win.pop(), list(names)
        parts, where, pos = [], {}, 0
        for n in dict.fromkeys(names):
            k = X.CASES[n]
            m = min(len(k.ya), len(k.yb))
            s, e = int(m * 0.10), int(m * 0.90)
            where[n] = []
            for y in (k.ya[s:e], k.yb[s:e]):
                where[n].append((pos + 3, len(y)))            # odd sample offsets
                parts += [np.zeros(3, np.float32), y]
                pos += 3 + len(y)
        self.sig = np.concatenate(parts + [np.zeros(8, np.float32)])
        ia, ib, w0, w1, sw, c0, c1, pa_l, pb_l, exp_l = ([] for _ in range(10))
        for n in names:
            k = X.CASES[n]
            (oa, la), (ob, lb) = where[n]
            w0.append(len(sw))
            geo = ops.xcorr_geometry(la, lb, self.win, int(k.search_range * lb), max(1, self.win // 4), k.n_windows)
            for pa, exp_pb, cands in geo:
                assert 0 <= pa <= la - self.win and all(0 <= pb <= lb - self.win for pb in cands)
                sw.append(len(ia))
                ia.append(oa + pa)
                ib.append(oa + pa)
                pb_l.append(pa)
                c0.append(len(ia))
                ia += [oa + pa] * len(cands)
                ib += [ob + pb for pb in cands]
                pb_l += cands
                c1.append(len(ia))
                pa_l.append(pa)
                exp_l.append(exp_pb)
            w1.append(len(sw))
        assert max(max(ia), max(ib)) + self.win <= len(self.sig)
        self.n_items = len(ia)
        self.arrays = [(ia, np.int64), (ib, np.int64), (w0, np.int32), (w1, np.int32), (sw, np.int32), (c0, np.int32),
                       (c1, np.int32), (pa_l, np.int64), (pb_l, np.int64), (exp_l, np.int64)]

    def run(self, ctx):
        dev = _dev.device(0)
        sig = _dev.to_dev(self.sig, dev, np.float32)
        ia, ib, w0, w1, sw, c0, c1, pa, pb, ex = (_dev.to_dev(np.asarray(a, t), dev) for a, t in self.arrays)
        n = len(self.names)
        scratch = torch.full((2 * self.n_items,), np.nan, dtype=torch.float64, device=dev)
        out = torch.full((2 * n,), np.nan, dtype=torch.float64, device=dev)
        ctx.call("nc_xcorr_search", sig.data_ptr(), ia.data_ptr(), ib.data_ptr(), self.n_items, self.win,
                 scratch[:self.n_items].data_ptr(), scratch[self.n_items:].data_ptr(), w0.data_ptr(), w1.data_ptr(),
                 sw.data_ptr(), c0.data_ptr(), c1.data_ptr(), pa.data_ptr(), pb.data_ptr(), ex.data_ptr(), n,
                 out[:n].data_ptr(), out[n:].data_ptr(), _dev.stream_handle())
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        return [(float(o[j]), float(o[n + j])) for j in range(n)]


@pytest.mark.parametrize("window_sec", X.WINDOW_SECS)
def test_130_jobs_in_one_launch_equal_their_single_job_results(gpu_ctx, window_sec):
    """The cases of one window length repeated in turn, so neighbouring jobs differ in window
    count (3 next to 200) and the jobs fill three 64-thread blocks of the finalize kernel, the
    last one partly.  Every job: the bits of the same job launched alone, and the oracle."""
    mine = [n for n in X.NAMES if X.CASES[n].window_sec == window_sec]
    assert len(mine) >= 9 and {X.CASES[n].n_windows for n in mine} >= {3, 20, 64, 65, 80, 200}
    names = [mine[j % len(mine)] for j in range(130)]
    got = Jobs(names).run(gpu_ctx)
    alone = {n: Jobs([n]).run(gpu_ctx)[0] for n in mine}
    worst = [0.0, 0.0]
    for j, n in enumerate(names):
        assert got[j] == alone[n], (j, n, got[j], alone[n])
    for n in mine:
        d = _check(f"alone {n}", alone[n], _reference(n))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print(f"[xcorr] 130 jobs, window {window_sec} s: largest ratio difference {worst[0]:.1e}, "
          f"largest quality difference {worst[1]:.1e}")
