"""The beat-tracker case grid (tests/beat_cases.py) on the CPU: every case that the GPU tests
compare exactly with the oracle must be robust to the differences in intermediates that the
kernel is allowed (table entries an ulp off, the kernel's form of the onset norm), the
radix-select cases must really have more peaks than the kernel has threads, and the grid must
straddle the LDS / workspace boundary of the engine."""
import numpy as np
import pytest

import beat_cases as bc
from oracle import ncref
from nightcore_analyzer.engine import beat_needs_workspace

GROUPS = bc.groups(bc.grid() + bc.radix_cases() + bc.rank_cases() + bc.mixed_cases(512) + bc.mixed_cases(64))


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_case_qualifies(group):
    """Allowed share of unqualified cases: zero.  If a future case fails, change its seed."""
    bad, norm_differs = [], 0
    for c in GROUPS[group]:
        # the median cases are compared with trim off as well (where ``fade`` keeps its beats)
        for trim in (True, False) if group.startswith(("radix", "rank")) else (True,):
            r = bc.qualify(c, trim)
            norm_differs += r["norm_differs"] and trim
            if not (r["a1"] and r["a2"] and r["b"]):
                bad.append((c, trim, r))
    print(f"{group}: {len(GROUPS[group])} cases, kernel-form norm differs in {norm_differs}, unqualified {len(bad)}")
    assert not bad, bad


def test_perturbable_oracle_is_the_oracle():
    """beats_with() with nothing overridden is ncref.beat_track, trim on and off."""
    for c in (bc.Case("x", "clicks", 431, 17, 512, 344), bc.Case("x", "silence_mid", 1500, 168, 64, 2756),
              bc.Case("x", "noise", 300, 3, 4096, 43), bc.Case("x", "const", 40, 9, 512, 344)):
        for trim in (True, False):
            _, ref = bc.oracle(c, trim)
            np.testing.assert_array_equal(bc.beats_with(bc.case_onset(c), c.P, trim=trim), ref)


def test_one_hot_tempogram_forces_the_period():
    seen = set()
    for c in bc.grid() + bc.grid(weak=True) + bc.radix_cases() + bc.rank_cases():
        if (c.hop, c.P) in seen:
            continue
        seen.add((c.hop, c.P))
        assert 0 < c.P < c.acw and c.acw == ncref.ac_win_length(bc.SR, c.hop)
        bpm, lag = ncref.tempo_from_tg(bc.case_tg(c), bc.SR, c.hop, bc.START_BPM)
        assert lag == c.P and bpm == 60.0 * bc.SR / (c.hop * c.P)
        assert float(np.round(bc.SR / c.hop * 60.0 / bpm)) == c.P


def test_no_case_is_all_zero_or_single_frame():
    for c in bc.grid() + bc.grid(weak=True) + bc.radix_cases() + bc.rank_cases():
        assert c.N >= 2 and bc.case_onset(c).any()


def test_radix_select_conditions():
    """More peaks than threads (256 in LDS, 1024 through the workspace) and both parities of the
    count on each path, so that the odd and the even form of the median both run."""
    parities = {}
    for c in bc.radix_cases() + bc.rank_cases():
        cnt, threshold_active, decides = bc.median_decides(c)
        nt = bc.RADIX_NT[c.group]
        long_path = beat_needs_workspace(c.N, c.acw)
        assert long_path == (nt == 1024)
        if c.group.startswith("radix"):
            assert cnt > nt, (c, cnt)
            parities.setdefault((nt, c.kind), set()).add(cnt & 1)
        else:                       # the rank-count form, with a median that matters
            assert 0 < cnt <= nt and c.kind == "fade", (c, cnt)
            parities.setdefault((nt, "rank"), set()).add(cnt & 1)
        # fade: the last beat is set by the median (and would move with a quartile in its place)
        # and, with trim off, is the last beat reported; with trim on no beat is left
        if c.kind == "fade":
            assert threshold_active and decides, c
            assert len(bc.oracle(c, True)[1]) == 0 or c.group.startswith("rank")
            assert bc.oracle(c, False)[1][-1] == ncref.last_beat(bc._cumscore(c)) < c.N - 3 * c.P
        print(c, "peaks", cnt)
    assert parities == {(nt, k): {0, 1} for nt in (256, 1024) for k in ("noise", "fade", "rank")}


def test_ordinary_cases_use_the_rank_count_median():
    """The other side of the threshold: a case of each path with at most NT peaks."""
    for c, nt in ((bc.Case("lds", "clicks", 431, 17, 512, 344), 256),
                  (bc.Case("long", "clicks", 3500, 17, 512, 344), 1024)):
        assert c in bc.grid()
        assert 0 < bc.peak_count(c) <= nt


@pytest.mark.parametrize("hop", [512, 64])
def test_grid_straddles_the_workspace_boundary(hop):
    acw = bc.acw_of(hop)
    lo, hi = bc.boundary(acw)
    assert hi == lo + 1 and not beat_needs_workspace(lo, acw) and beat_needs_workspace(hi, acw)
    ns = {c.N for c in bc.grid() if c.acw == acw}
    assert lo in ns and hi in ns
