"""CPU qualification of tests/align_cases.py: the cases reach the paths of csrc/align.hip they
are meant to reach, the per-speed oracle agrees with refglue.find_content_offset, and every
decision the GPU test demands exactly is safe from the envelope's rounding (the yardstick).
No GPU.  Figures measured here are printed (pytest -s) next to each condition."""
import numpy as np
import pytest

import align_cases as A
from oracle import refglue


def _searchable(ev):
    return [(i, s) for i, s in enumerate(ev.speeds) if not s.skipped]


@pytest.mark.parametrize("name,g", A.RUNS)
def test_per_speed_oracle_winner_is_refglues(name, g):
    src, nc = A.signals(name)
    off, speed, best = refglue.find_content_offset(src, nc, A.SR, speed_lo=g[0], speed_hi=g[1], n_speeds=g[2],
                                                   detail=True)
    ev = A.oracle(name, g)
    assert len(ev.speeds) == g[2]
    assert ev.winner == best
    if best[1] < 0:
        assert (off, speed) == (0.0, (g[0] + g[1]) / 2.0)
    else:
        assert (off, speed) == (best[0] * A.HOP_SEC, float(A.grid(g)[best[1]]))


def test_signals_are_short_and_cases_cheap():
    for name in A.NAMES:
        src, nc = A.signals(name)
        assert src.dtype == nc.dtype == np.float32
        assert max(len(src), len(nc)) <= 150 * A.SR, name


def test_cases_reach_what_they_are_for():
    ev = {n: A.oracle(n) for n in A.NAMES}
    st = {n: [s.n_st for _, s in _searchable(ev[n])] for n in A.NAMES}
    lag = {n: [s.n_lag for _, s in _searchable(ev[n])] for n in A.NAMES}
    for n in A.NAMES:
        print(f"{n}: searchable {len(st[n])}/30, n_st {min(st[n], default=0)}..{max(st[n], default=0)}, "
              f"n_lag {min(lag[n], default=0)}..{max(lag[n], default=0)}, winner {ev[n].winner}")
    # more than one 256-lag block of align_corr_kernel, every speed searched
    assert len(st["golden60"]) == 30 and min(lag["golden60"]) > 256 and max(lag["golden60"]) > 512
    # the 1024-element LDS tile is crossed inside the grid
    assert len(st["two_tiles"]) == 30 and min(st["two_tiles"]) < A.AL_TILE < max(st["two_tiles"])
    assert A.AL_TILE in range(min(st["two_tiles"]), max(st["two_tiles"]))
    # a winner that is neither end of the grid
    assert 5 <= ev["other_ratio"].winner[1] <= 24
    # the lag cap max_offset_frames + 1 is reached and not reached within one grid; peaks in the last blocks
    assert max(lag["lag_cap"]) == A.MAX_FRAMES + 1 == 2584 and min(lag["lag_cap"]) < 2584
    assert lag["lag_cap"].count(2584) >= 5
    assert all(s.peak >= 2304 for _, s in _searchable(ev["lag_cap"]))
    assert len(st["short"]) == 30
    # several speeds share a stretch length: bit-identical stretches, correlations and scores
    s1 = st["nc_1s"]
    assert len(s1) == 30 and len(set(s1)) < 30
    w = ev["nc_1s"].winner
    tied = [i for i, s in _searchable(ev["nc_1s"]) if s.score == w[2]]
    print("nc_1s: n_st", s1, "speeds at the winning score", tied)
    assert len(tied) >= 2 and w[1] == tied[0]
    assert len({ev["nc_1s"].speeds[i].n_st for i in tied}) == 1
    # the smallest searchable stretch lengths
    assert sorted(set(st["nc_6_frames"])) == [4, 5] and len(st["nc_6_frames"]) == 30
    # nothing searchable: too short a query, then too long a query
    for n in A.ALL_SKIPPED:
        assert not st[n] and ev[n].winner == (0, -1, -1.0), n
    assert all(s.n_st < 4 for s in ev["nc_too_short"].speeds)
    src_frames = 1 + ((len(A.signals("nc_longer")[0]) + 1) // 2) // 512
    assert all(s.n_st >= src_frames for s in ev["nc_longer"].speeds)
    # exact zeros: every correlation 0, denom 0, the first speed and the first lag win with score 0.0
    for n in A.SILENT:
        assert len(st[n]) == 30 and ev[n].winner == (0, 0, 0.0), n
        assert all(s.all_zero and s.peak == 0 and s.score == 0.0 for _, s in _searchable(ev[n])), n
    # real peaks below the denominator gate: every score 0.0, speed 0 wins with its own peak
    q = ev["quiet"]
    assert len(st["quiet"]) == 30 and all(s.score == 0.0 and not s.all_zero for _, s in _searchable(q))
    assert q.winner == (q.speeds[0].peak, 0, 0.0) and q.speeds[0].peak > 0
    # the gate itself is far from every case: no rounding moves a denominator across 1e-12
    assert all(0.0 < s.denom < 1e-15 for _, s in _searchable(q))
    loud = [n for n in A.NAMES if n not in A.SILENT + A.ALL_SKIPPED + ("quiet",)]
    assert all(s.denom > 1e-6 for n in loud for _, s in _searchable(ev[n]))
    # the mixed grid: skipped and searchable speeds within one pair
    m = A.oracle("golden60", A.GRID_MIXED)
    sk = [s.skipped for s in m.speeds]
    print("golden60 on the mixed grid: skipped", sk, "winner", m.winner)
    assert any(sk) and not all(sk) and sk[0] and not sk[-1] and m.winner[1] > sk.index(False)
    wd = A.oracle("golden60", A.GRID_WIDE)
    assert not any(s.skipped for s in wd.speeds)
    assert wd.speeds[0].n_st > len(A._envelopes("golden60", False)[1]) > wd.speeds[-1].n_st


def test_decisions_are_safe_from_the_yardstick():
    """For every searchable (case, speed): both evaluations find the same peak, and it stands
    PEAK_MARGIN above the runner-up (exact zeros apart: there every correlation is 0 in any
    implementation, and the first lag wins).  The winner beats every other speed by WIN_MARGIN
    or ties it bit for bit at the same stretch length.  No (case, speed) is left out."""
    yard = A.yardstick()
    print(f"yardstick {yard:.2e}, score tolerance {A.score_tol():.2e}")
    assert 0.0 < yard < 1e-7
    assert min(A.PEAK_MARGIN, A.WIN_MARGIN) > 16 * yard
    compared = 0
    for name, g in A.RUNS:
        a, b = A.oracle(name, g), A.oracle(name, g, True)
        assert [s.skipped for s in a.speeds] == [s.skipped for s in b.speeds]
        assert [(s.n_st, s.n_lag) for s in a.speeds] == [(s.n_st, s.n_lag) for s in b.speeds]
        assert a.winner[:2] == b.winner[:2]
        margins, leads = [], []
        for i, s in _searchable(a):
            compared += 1
            assert s.peak == b.speeds[i].peak, (name, i)
            if s.all_zero:
                assert name in A.SILENT and b.speeds[i].all_zero
                continue
            for e in (s, b.speeds[i]):
                assert e.margin >= A.PEAK_MARGIN, (name, g, i, e.margin)
            margins.append(min(s.margin, b.speeds[i].margin))
        for e in (a, b):
            w = e.winner
            for i, s in _searchable(e):
                if i == w[1]:
                    continue
                lead = w[2] - s.score
                if lead == 0.0 and (s.n_st == e.speeds[w[1]].n_st or w[2] == 0.0):
                    assert i > w[1], (name, i)        # a bit-tie: the strict '>' keeps the first
                    continue
                assert lead >= A.WIN_MARGIN, (name, g, i, lead)
                leads.append(lead)
        print(f"{name} {g}: yardstick {A.case_yardstick(name, g):.2e}, smallest peak margin "
              f"{min(margins, default=float('nan')):.2e}, smallest lead of the winner {min(leads, default=float('nan')):.2e}")
    n_search = sum(len(_searchable(A.oracle(n, g))) for n, g in A.RUNS)
    assert compared == n_search            # the share of comparisons left out is zero
