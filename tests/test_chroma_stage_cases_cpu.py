"""CPU qualification of tests/chroma_stage_cases.py: the cases reach the paths of csrc/cqt.hip
they are meant to reach, the per-stage references agree with the oracle's end-to-end functions,
and the reference alone (the oracle's f32 / complex64 roundings against the f64 evaluation)
stays inside every bar the GPU file holds the device to.  No GPU.  Figures are printed
(pytest -s) next to each condition."""
import numpy as np
import pytest

import chroma_stage_cases as S
from oracle import ncref


def _chunk_signals(ln):
    L = S.launch(ln)                      # built on first use, never at collection
    return [(c, S.chunk_signal(L, c)) for c in L.chunks]


def test_lengths_come_from_the_library_and_straddle_every_tile():
    k, ext = S.constants(), S.tile_extents()
    assert all(v > 0 for v in k.values()) and k["kHalfbandK"] == (len(ncref.halfband_taps()) - 1) // 2
    L = S.launch("edges")
    lens = {c.len for c in L.chunks}
    for name, e in ext.items():
        assert {e - 1, e + 1} <= lens, name
    assert set(S.SHORT_LENGTHS) <= lens
    assert {c.off & 1 for c in L.chunks} == {0, 1}                    # odd and even chunk_off
    names = [c.name for c in L.chunks]
    for s in S.SHORT_LENGTHS:                                         # short ones between long ones
        i = names.index(f"short {s}")
        assert 0 < i < len(names) - 1 and L.chunks[i - 1].len > 2048 and L.chunks[i + 1].len > 2048
    assert max(len(S.launch(ln).sig) for ln in S.LAUNCHES) <= 25 * S.SR  # the launches stay small
    z = S.chunk_signal(L, L.chunks[names.index("zero")])
    g = S.chunk_signal(L, L.chunks[names.index("silent middle")])
    assert not z.any() and not g[len(g) // 3:2 * len(g) // 3].any() and g[:len(g) // 3].any() and g[-len(g) // 3:].any()


def test_layout_query_is_consistent_with_the_workspace_size():
    from nightcore_analyzer import _native
    lib = _native.load()
    for n, total in ((1, 1), (3, 70000), (224, 224 * 441000)):
        lay = S.layout(n, total)
        offs = [lay[k] for k in S.LAYOUT_NAMES[1:17]]
        assert offs[0] == 0 and offs == sorted(offs) and all(o % 256 == 0 for o in offs)
        assert offs[-1] < lay["head"] and lay["head"] + 24 * n <= lay["bytes"] <= lib.nc_chroma_workspace_bytes(None, n, total)
        tfr = total // 512 + n
        assert lay["peak_mag"] - lay["peak_pitch"] >= 4 * tfr * lay["kPeakSlots"]
        assert lay["oct_ex"] - lay["gpart"] >= 4 * tfr * 84
        assert lay["peak_pitch"] - lay["ws_oct"] >= 4 * (total + 64 * 7 * n)
    out = np.zeros(4, np.int64)
    assert lib.nc_chroma_workspace_layout(None, 1, 512, out.ctypes.data, 4) == -2   # too small a cap


def test_plan_restatement_matches_the_oracles_shapes():
    for L in (1, 2, 63, 511, 512, 513, 1023, 3807, 65537):
        y = np.ones(L, np.float32)
        oct_len, oct_off, n_frames, n_tf, tf_base = S.plan([L, L])
        lev = S.levels_oracle(y)
        assert [len(v) for v in lev] == oct_len[0].tolist()
        assert n_frames[0] == ncref.cqt_mag(y, tuning=0.0).shape[1]
        assert n_tf[0] == ncref.piptrack(y)[0].shape[1] and tf_base.tolist() == [0, n_tf[0], 2 * n_tf[0]]
        assert oct_off[1, 1] == sum((v + 63) & ~63 for v in oct_len[0, 1:]) and oct_off[0, 0] == -1


@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_decimation_reference_is_inside_its_bound(ln):
    """The oracle's chain (f64 sums rounded to f32 per level) against the unrounded f64 chain:
    inside the compounded bound the device chain is held to, with room to spare."""
    worst = 0.0
    for c in S.launch(ln).chunks:
        y = S.chunk_signal(S.launch(ln), c)
        a, b = S.levels_oracle(y), S.levels_f64(y)
        bounds = S.chain_bounds([float(np.max(np.abs(v))) if len(v) else 0.0 for v in a])
        for o in range(1, 7):
            err = float(np.max(np.abs(a[o] - b[o])))
            assert err <= bounds[o], (c.name, o, err, bounds[o])
            if bounds[o]:
                worst = max(worst, err / bounds[o])
    print(f"{ln}: oracle f32 chain against f64 chain, worst error / bound {worst:.3f}")


def test_adversarial_chunk_attains_the_level_gain():
    L = S.launch("edges")
    y = S.chunk_signal(L, [c for c in L.chunks if c.name == "adversarial"][0])
    l1 = ncref.decimate2(y)
    ratio = float(np.max(np.abs(l1)) / (S.level_gain() * np.max(np.abs(y))))
    print(f"adversarial: max|level 1| / (g max|level 0|) = {ratio:.6f}")
    assert 1.0 - 1e-3 <= ratio <= 1.0 + 1e-6


@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_peak_lists_f32_and_f64_agree(ln):
    for c, y in _chunk_signals(ln):
        p32, m32, pf = S.peaks(y)
        p64, m64, _ = S.peaks(y, f64=True)
        cap = S.peak_cap(len(p64))
        ua, ub, _ = S.compare_sorted(p32, p64, 1e-2)
        assert ua <= cap and ub <= cap, (c.name, ua, ub, cap)
        assert pf.max(initial=0) <= S.constants()["kPeakSlots"]
        yard = S.peak_yardstick(y)
        print(f"{c.name}: {len(p32)} peaks, unmatched {ua}/{ub} (cap {cap}), most per frame {pf.max(initial=0)}, "
              f"yardstick {yard}")
        assert yard is not None                  # equal counts on every case: measured 0 differing decisions


def test_forced_lists_select_bank_49_and_the_zero_residual():
    f = S.forced_lists()
    assert S.tuning_from_list(*f["bank 49"]) == (49, len(f["bank 49"][0]), 0)
    idx, margin, amb = S.tuning_from_list(*f["zero residual"])
    assert (idx, margin) == (50, len(f["zero residual"][0]))
    p = f["zero residual"][0]
    assert np.all(np.float32(36.0) * np.log2(p / np.float32(27.5)) % np.float32(1.0) == 0.0)   # exactly 0 in f32 too
    assert {c.name for c in S.launch("forced").chunks} >= set(f)
    L = S.launch("edges")
    assert L.chunks[-1].len == 3 and L.chunks[-1].off + 3 == len(L.sig)      # ends with the buffer


def test_peak_cases_reach_their_paths():
    T = S.launch("tuning")
    by = {c.name: S.chunk_signal(T, c) for c in T.chunks}
    E = S.launch("edges")
    assert S.peaks(by["noise"])[2].max() > 64                       # two compaction passes
    pn, mn, _ = S.peaks(by["periodic 512"])
    assert len(np.unique(mn)) * 8 < len(mn)                         # massive ties in the radix median
    assert len(S.peaks(by["burst 1"])[0]) == 1 and len(S.peaks(by["burst 2"])[0]) == 2
    assert len(S.peaks(S.chunk_signal(E, [c for c in E.chunks if c.name == "zero"][0]))[0]) == 0
    counts = [len(S.peaks(S.chunk_signal(L, c))[0]) for L in (T, E) for c in L.chunks]
    assert any(n > 2 and n % 2 == 0 for n in counts) and any(n > 2 and n % 2 == 1 for n in counts)
    # burst 2: the weaker peak sits in the lower histogram bin and both are far from a bin edge,
    # so the even-count median (the upper middle included) decides the index
    p, m, _ = S.peaks(by["burst 2"])
    lo, hi = np.argsort(m)
    one = lambda q: S.tuning_from_list(np.float32([p[q]]), np.float32([m[q]]))
    assert one(lo)[0] < one(hi)[0] and one(lo)[2] == 0 and one(hi)[2] == 0
    assert S.tuning_from_list(p.astype(np.float32), m.astype(np.float32))[:2] == (one(hi)[0], 1)
    assert S.tuning_from_list(p.astype(np.float32), np.float32([1.0, 1.0]))[0] == one(lo)[0]   # were the median the lower middle


def test_detuned_stacks_sample_the_filter_banks():
    """The stacks at the bin centres of indices 0, 1, 25, 49, 50, 74, 98, 99: the oracle lands
    them on 0, 1, 24, 48, 50, 74, 98, 99 (piptrack's parabolic shift is biased low by up to a
    bin), and the extra stack on 25; every decision is far from a tie."""
    T = S.launch("tuning")
    got = {}
    for c in T.chunks:
        if c.name.startswith("detuned"):
            _, idx, margin = ncref.estimate_tuning_detail(S.chunk_signal(T, c))
            p, m, _ = S.peaks(S.chunk_signal(T, c))
            assert S.tuning_from_list(p.astype(np.float32), m.astype(np.float32))[0] == idx
            assert margin > 4 * S.peak_cap(len(p)), (c.name, idx, margin)
            got[c.name] = idx
    print(got)
    assert [got[f"detuned {i}"] for i in S.TUNING_INDICES] == [0, 1, 24, 48, 50, 74, 98, 99]
    assert got["detuned extra"] == 25


@pytest.mark.parametrize("ln", S.LAUNCHES)
def test_octave_rows_restate_cqt_mag_and_the_yardsticks_fit_the_cap(ln):
    L = S.launch(ln)
    yards = []
    for c in L.chunks:
        y = S.chunk_signal(L, c)
        tun = ncref.estimate_tuning(y)
        lev = S.levels_oracle(y)
        T = int(S.plan([c.len])[2][0])
        Cq = ncref.cqt_mag(y, tuning=tun)
        for o in range(7):                                            # device octave o = CQT bins 252 - 36 (o + 1) ..
            assert np.array_equal(S.octave_mag(lev[o], o, tun)[:, :T], Cq[252 - 36 * (o + 1):252 - 36 * o]), (c.name, o)
        rows = np.stack([S.octave_rows(lev[6 - k], 6 - k, tun, T) for k in range(7)], axis=1)   # a gpart
        ref = ncref.chroma_cqt(y, tuning=tun).mean(axis=1)
        assert np.max(np.abs(S.tail(rows) - ref)) <= 4e-7, c.name    # f32 sums in another order, T frames
        yards.append(S.row_yardstick(lev, tun, T))
    yards = np.array(yards)
    bars = S.row_bars(yards)
    print(f"{ln}: row yardstick per octave, median {np.median(yards, axis=0)} max {yards.max(axis=0)}\n"
          f"  bars max {bars.max(axis=0)}")
    assert np.isfinite(yards).all() and yards.max() <= S.ROW_CAP
    assert (bars <= S.ROW_CAP).all() and (bars[yards.max(axis=1) > 0] > 0).all()
