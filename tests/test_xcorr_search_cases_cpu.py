"""CPU qualification of tests/xcorr_search_cases.py: the windowed oracle is refglue's, the cases
reach the branches of xcorr_finalize_kernel they are meant to reach, and every decision the GPU
test depends on (which candidate wins, whether a window matches, either gate) stands clear of
the f32 / f64 difference between the reference's np.dot and the device's f64 sums.  No GPU."""
import numpy as np
import pytest

import xcorr_search_cases as X
from nightcore_analyzer import ops


@pytest.mark.parametrize("name", X.NAMES)
def test_windowed_oracle_is_refglues(name):
    o = X.oracle(name)
    assert (o.ratio, o.quality) == X.reference(name)


def test_window_lengths_and_counts():
    for ws in X.WINDOW_SECS:
        win = int(ws * X.SR)
        assert win % 256 != 0 and win % 64 != 0
    assert int(0.05 * X.SR) == 1102 and int(0.05 * X.SR) // 4 == 275 and int(0.1 * X.SR) == 2205
    for ws in X.WINDOW_SECS:
        for nw in X.WINDOWS:
            o = X.oracle(f"speed_w{nw}_{ws}")
            n_match = sum(w.matched for w in o.windows)
            print(f"speed_w{nw}_{ws}: windows {len(o.windows)}, matched {n_match}, candidates "
                  f"{min(w.n_cand for w in o.windows)}..{max(w.n_cand for w in o.windows)}, "
                  f"ratio {o.ratio:.5f}, quality {o.quality:.4f}")
            assert len(o.windows) == nw and nw - 2 <= n_match <= nw
            assert n_match > 64 or nw <= 64                   # 65, 80, 200: more than 64 correspondences
    assert max(w.n_cand for w in X.oracle("speed_w20_0.05").windows) == 39
    # the fit moves with the windows past the 64th: a search that stops there misses the 1e-9 bar
    for ws in X.WINDOW_SECS:
        r64 = X.oracle(f"speed_w64_{ws}").ratio
        for nw in (65, 80, 200):
            o = X.oracle(f"speed_w{nw}_{ws}")
            first = [(w.pa, w.best_pb) for w in o.windows if w.matched][:64]
            cut = float(np.polyfit(*np.array(first, float).T, 1)[0])
            print(f"window_sec {ws}, {nw} windows: ratio {o.ratio:.6f}, from the first 64 only {cut:.6f}")
            assert abs(cut - o.ratio) > 1e-6, (ws, nw)
        assert np.isfinite(r64)


def test_gates_ties_and_signs_reach_their_branches():
    for name, n in (("gated_three", 3), ("gated_two", 2)):
        o = X.oracle(name)
        gates = [w.gate for w in o.windows]
        assert gates == ["rms", "rms", None, "norm", "norm", "norm", None, None if n == 3 else "norm"], (name, gates)
        assert [w.matched for w in o.windows] == [g is None for g in gates]
        k = X.CASES[name]
        win, geo = X._trimmed_geometry(len(k.ya), len(k.yb), 8, 0.1)
        rms = [float(np.sqrt(np.mean(k.ya[a0:a0 + win].astype(np.float64) ** 2))) for a0, _, _ in geo]
        print(name, "window rms", [f"{r:.2e}" for r in rms], "result", (o.ratio, o.quality))
        assert all(abs(r / 5e-4 - 1) < 1e-3 for r in rms[:2]) and abs(rms[2] / 2e-3 - 1) < 1e-3
        assert all(r > 4e-3 for r in rms[3:])
    assert (X.oracle("gated_two").ratio, X.oracle("gated_two").quality) == (1.0, 0.0)
    assert X.oracle("gated_three").quality > 0.1 and X.oracle("gated_three").ratio != 1.0
    # anti-correlated: the aligned candidate is at -1; with one candidate per window nothing matches
    o = X.oracle("anti_narrow")
    assert len(o.windows) == 20 and all(w.n_cand == 1 and w.best < -0.5 and not w.matched for w in o.windows)
    assert (o.ratio, o.quality) == (1.0, 0.0)
    o = X.oracle("narrow")
    assert all(w.n_cand == 1 and w.best > 0.5 and w.matched for w in o.windows) and o.quality > 0.5
    o = X.oracle("anti")
    print("anti: best per window", [f"{w.best:.3f}" for w in o.windows], (o.ratio, o.quality))
    assert all(w.best_pb != w.pa for w in o.windows if w.matched)
    # exact ties: every candidate of a window gives the same bits, the first one wins
    for f64 in (False, True):
        o = X.oracle("tied", f64)
        assert len(o.windows) == 20
        assert all(w.matched and w.best_pb == w.lo and w.runner_up == w.best and w.n_cand >= 20 and w.best > 0.3
                   for w in o.windows), f64
    k = X.CASES["tied"]
    assert np.array_equal(k.yb[275:275 + 5000], k.yb[:5000])


def test_decisions_stand_clear_of_f32_against_f64():
    """For every window of every case: the f64 search makes the same decisions as the reference's
    f32 one; the winner beats the runner-up by RUNNER_UP (ties apart), the best correlation and
    the window's RMS stand clear of their thresholds."""
    worst_q, worst_margin = 0.0, np.inf
    for name in X.NAMES:
        a, b = X.oracle(name), X.oracle(name, True)
        assert [(w.pa, w.gate, w.best_pb, w.matched, w.n_cand) for w in a.windows] == \
               [(w.pa, w.gate, w.best_pb, w.matched, w.n_cand) for w in b.windows], name
        assert abs(a.ratio - b.ratio) < 1e-12, name
        worst_q = max(worst_q, abs(a.quality - b.quality))
        for e in (a, b):
            for w in e.windows:
                if w.gate is not None:
                    continue
                assert abs(w.best) >= X.RUNNER_UP, (name, w)
                if name != "tied" and w.n_cand > 1:
                    assert w.best - w.runner_up >= X.RUNNER_UP, (name, w)
                    worst_margin = min(worst_margin, w.best - w.runner_up)
    print(f"largest |quality f32 - quality f64| {worst_q:.2e}; smallest lead over the runner-up {worst_margin:.2e}")
    assert worst_q < X.QUALITY_TOL / 10


def test_product_geometry_is_the_oracles():
    """ops.xcorr_geometry (what ops.xcorr_speed and the many-jobs GPU test plan with) gives the
    oracle's windows and candidate counts."""
    for name in X.NAMES:
        k = X.CASES[name]
        n = int(min(len(k.ya), len(k.yb)) * 0.9) - int(min(len(k.ya), len(k.yb)) * 0.1)
        win = int(k.window_sec * X.SR)
        geo = ops.xcorr_geometry(n, n, win, int(k.search_range * n), max(1, win // 4), k.n_windows)
        o = X.oracle(name)
        assert [(pa, ex, c[0]) for pa, ex, c in geo] == [(w.pa, w.exp_pb, w.lo) for w in o.windows], name
        assert all(len(c) >= w.n_cand for (_, _, c), w in zip(geo, o.windows))
