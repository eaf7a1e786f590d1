"""The cases of tests/test_gpu_tempo_features.py, qualified on the CPU: which kernel each
window length reaches, how far an honest f32 mel/onset chain is from the f64 oracle (the
yardstick of the GPU tests), that the well-conditioned envelopes of the grid are ones on
which both tempogram emulations reach f64 rounding level, and that the plain sliding sums
do NOT on envelopes that fall from loud to exact zero (the finding behind slide_lag_sum2's
re-seeding rule, csrc/nc_slide.h)."""
import numpy as np
import pytest

import tempo_feature_cases as C
from oracle import ncref

SR = 22050


def test_corr_T_max_matches_the_launcher():
    assert {sr: C.corr_T_max(acw) for sr, acw in C.RATES.items()} == {16000: 1333, 22050: 1247, 44100: 928,
                                                                     48000: 872}
    assert (1 + 638975 // 512, 1 + 638976 // 512) == (1248, 1249)  # win_len < 638 976 is T <= 1248 ...
    assert C.uses_correlation(1247, 344) and not C.uses_correlation(1248, 344)
    for sr, acw in C.RATES.items():
        assert acw == ncref.ac_win_length(sr, 512)


@pytest.mark.parametrize("sr", [22050, 44100, 48000])
def test_window_grid_straddles_the_kernel_boundary(sr):
    acw, Ts = C.RATES[sr], C.WINDOW_T[sr]
    tmax = C.corr_T_max(acw)
    assert any(T <= tmax for T in Ts) and any(T > tmax for T in Ts)
    if sr == 22050:
        assert tmax in Ts and tmax + 1 in Ts
    # the gap windows of group b: 24 s on the correlation kernel, 36 s on the sliding sums
    assert C.uses_correlation(1034, 344) and not C.uses_correlation(1551, 344)


AUDIO = {
    "music": lambda n: C.music(n),
    "music_1e-4": lambda n: C.scaled(C.music(n), 1e-4),
    "music_30": lambda n: C.scaled(C.music(n), 30),
    "clicks": lambda n: C.clicks(n),
    "clicks_1e-4": lambda n: C.scaled(C.clicks(n), 1e-4),
    "clicks_30": lambda n: C.scaled(C.clicks(n), 30),
    "half_silent": lambda n: C.half_silent(n),
    "head": lambda n: C.head(n),
    "quiet_tail": lambda n: C.quiet_tail(n),
    "first_second": lambda n: C.first_second(n, SR),
    "gap_6_12_6": lambda n: C.gap(SR, 6, 12, 6),
}


@pytest.mark.parametrize("name", sorted(AUDIO))
def test_f32_yardsticks_are_below_the_old_tolerances(name):
    """The distance between the oracle and its own single-precision restatement: finite, and
    far below the tolerances test_gpu_window.py uses (1e-4 max(1, peak) and 2e-5)."""
    y = AUDIO[name](220500)
    S64, S32 = ncref.mel_db(y, SR, 2048, 512), C.mel_db_f32(y, SR, 512)
    o64, o32 = ncref.onset_strength(y, SR, 512), C.onset_from_db(S32, 512)
    assert np.array_equal(o64, C.onset_from_db(S64, 512))
    d_db = float(np.max(np.abs(C.clamp_db(S64) - C.clamp_db(S32))))
    d_on = C.onset_yardstick(o64, S32, 512)
    d_tg = float(np.max(np.abs(ncref.tempogram_mean(o64, 344) - ncref.tempogram_mean(o32, 344))))
    print(f"{name}: mel dB {d_db:.2e}  onset {d_on:.2e} (peak {o64.max():.1f})  tg {d_tg:.2e}")
    assert np.isfinite([d_db, d_on, d_tg]).all()
    assert d_db < 1e-3
    assert d_on < 1e-4 * max(1.0, float(o64.max()))
    assert d_tg < C.TOL_TG


def test_silent_yardstick_is_exact():
    y = C.silent(33280)
    assert np.array_equal(ncref.mel_db(y), C.mel_db_f32(y)) and not ncref.onset_strength(y).any()
    assert not ncref.tempogram_mean(ncref.onset_strength(y), 344).any()


def _music_env(T, hop):
    n = (T - 1) * hop
    src = C.music(900000)
    return ncref.onset_strength(np.tile(src, 1 + n // len(src))[:n], SR, hop)


def _well(kind, T, N, hop):
    return _music_env(T, hop) if kind == "music" else C.envelope(kind, T, N)


GRID = sorted({(T, C.RATES[sr], 512) for sr, Ts in C.WINDOW_T.items() for T in Ts} |
              {(T, N, hop) for hop, N in C.IBI_N.items() for T in C.IBI_T})


@pytest.mark.parametrize("kind", C.WELL + ("music",))
@pytest.mark.parametrize("T,N,hop", GRID)
def test_well_conditioned_cases_reach_f64_level(T, N, hop, kind):
    """Both emulations agree with the FFT autocorrelation within 1e-12 on the random, periodic
    and music envelopes at every (T, N) of the GPU grid, so a GPU difference above that on
    them is the kernel's, not the algorithm's."""
    o = _well(kind, T, N, hop)
    ref = ncref.tempogram_mean(o, N)
    assert np.max(np.abs(C.sliding_tempogram_mean(o, N, tile=C.TILE) - ref)) < C.TOL_F64
    assert np.max(np.abs(C.sliding_tempogram_mean(o, N, tile=C.TILE, reseed=C.RESEED) - ref)) < C.TOL_F64
    assert np.max(np.abs(C.correlation_tempogram_mean(o, N) - ref)) < C.TOL_F64


@pytest.mark.parametrize("N", [689, 345])
def test_sliding_emulation_handles_an_odd_window(N):
    o = C.env_sparse(130, 3)
    assert np.max(np.abs(C.sliding_tempogram_mean(o, N) - ncref.tempogram_mean(o, N))) < C.TOL_F64


ILL_CASES = [("head", T, 2756) for T in (2047, 2048, 2049, 4096, 4097)] + \
            [("gap", T, 2756) for T in (4096, 4097)] + [("gap", 2049, 344)]


@pytest.mark.parametrize("kind,T,N", ILL_CASES)
def test_plain_sliding_sums_lose_precision_after_a_fall_to_zero(kind, T, N):
    """Loud, then exact zeros: the frames that see only the last samples under the far tail of
    the Hann window have a huge 1 / ac_t[0], and sums slid down from the loud passage carry its
    rounding residue.  The plain recurrences miss 2e-5 there; re-seeded at a 2^-20 drop of
    ac_t[0] they keep it, with a handful of extra seeds.  The oracle itself stays finite and
    normalised."""
    o = C.envelope(kind, T, N)
    ref = ncref.tempogram_mean(o, N)
    assert np.isfinite(ref).all() and np.max(np.abs(ref)) <= 1.0
    plain, fixed, seeds = [], [], []
    d0 = np.max(np.abs(C.sliding_tempogram_mean(o, N, tile=C.TILE, seeds_out=plain) - ref))
    d1 = np.max(np.abs(C.sliding_tempogram_mean(o, N, tile=C.TILE, reseed=C.RESEED, seeds_out=fixed) - ref))
    print(f"{kind} T={T} N={N}: plain {d0:.2e}, re-seeded {d1:.2e} ({fixed[0] - plain[0]} extra seeds), "
          f"ac0 spread {C.ac0_spread(o, N):.1e}")
    assert not d0 <= C.TOL_TG
    assert d1 < 1e-6 and fixed[0] - plain[0] <= 4


def test_gap_audio_through_the_emulations():
    """The issue's audio gaps at hop 512 on the oracle's own onsets: 36 s (12 s of zeros) through
    the sliding sums, 24 s through the correlations."""
    o36 = ncref.onset_strength(C.gap(SR, 12, 12, 12, 1550 * 512), SR, 512)
    ref = ncref.tempogram_mean(o36, 344)
    d0 = np.max(np.abs(C.sliding_tempogram_mean(o36, 344, tile=C.TILE) - ref))
    fix = C.sliding_tempogram_mean(o36, 344, tile=C.TILE, reseed=C.RESEED)
    o24 = ncref.onset_strength(C.gap(SR, 6, 12, 6, 1033 * 512), SR, 512)
    dc = np.max(np.abs(C.correlation_tempogram_mean(o24, 344) - ncref.tempogram_mean(o24, 344)))
    print(f"36 s: plain {d0:.2e}, re-seeded {np.max(np.abs(fix - ref)):.2e}; 24 s correlations {dc:.2e}, "
          f"ac0 spreads {C.ac0_spread(o36, 344):.1e} / {C.ac0_spread(o24, 344):.1e}")
    assert not d0 <= C.TOL_TG
    assert np.max(np.abs(fix - ref)) < 1e-6
    assert ncref.tempo_from_tg(fix)[1] == ncref.tempo_from_tg(ref)[1]
    assert np.isfinite(dc)
