"""Identity phase locking with linked channels (DESIGN.md §4 "Phase locking") without a GPU: the
peak and owner rule on hand-made rows, tests/pvoc_lock_ref.py against a brute-force walk of each
bin's predecessor chain, the identities of the definition, what the mode buys on a sustained
voiced tone and on a stereo pair, and the host-side argument checks of the layers above."""
import contextlib
import io as stdio

import numpy as np
import pytest

import pvoc_lock_ref as L
import pvoc_ref as R
from pvoc_lock_ref import rms, running_rms_spread, stereo_pair, unexplained, vibrato_tone

SR = 22050
BINS = R.BINS


# ------------------------------------------------------------------ peaks and owners
def _row(**at):
    m = np.zeros(BINS, np.float32)
    for b, v in at.items():
        m[int(b[1:])] = v
    return m


def _owners_slow(row):
    """The rule, bin by bin."""
    pk = [int(p) for p in L.peaks(row)]
    out = []
    for b in range(len(row)):
        below = [p for p in pk if p <= b]
        above = [p for p in pk if p >= b]
        if not below:
            out.append(above[0])
        elif not above:
            out.append(below[-1])
        else:
            p, q = below[-1], above[0]
            out.append(p if b <= (p + q) // 2 else q)
    return np.array(out, np.uint16)


def test_peaks_on_hand_made_rows():
    assert L.peaks(np.zeros(BINS)).tolist() == [0]                       # an all-zero row: bin 0 alone
    assert L.peaks(np.arange(BINS)).tolist() == [BINS - 1]               # monotone rows
    assert L.peaks(-np.arange(BINS, dtype=np.float64)).tolist() == [0]
    assert L.peaks(np.full(BINS, np.nan)).tolist() == [0]                # nothing qualifies: the single peak 0
    assert L.peaks(_row(b0=2.0, b1024=3.0)).tolist()[0] == 0 and L.peaks(_row(b0=2.0, b1024=3.0)).tolist()[-1] == 1024
    # a plateau: its first bin is the peak (> to the left, >= to the right)
    assert L.peaks(_row(b10=1.0, b11=1.0, b12=1.0)).tolist() == [0, 10]
    # exact ties two bins apart: the left one wins, the right one fails mag[b] > mag[b - 2]
    assert L.peaks(_row(b10=1.0, b12=1.0)).tolist() == [0, 10]
    # ... three bins apart both are peaks
    assert L.peaks(_row(b10=1.0, b13=1.0)).tolist() == [0, 10, 13]
    # the comparison is made on float32 values: a difference below half an ulp is a tie
    assert L.peaks(_row(b10=1.0) + _row(b11=1.0) * np.float64(1.0 + 1e-9)).tolist() == [0, 10]


def test_owners_on_hand_made_rows():
    o = L.owners(_row(b10=1.0, b13=1.0, b20=5.0))[0]
    assert o.dtype == np.uint16
    # peaks 0, 10, 13, 20: cuts at 5, 11, 16
    assert o[:6].tolist() == [0] * 6 and o[6:12].tolist() == [10] * 6
    assert o[12:17].tolist() == [13] * 5 and o[17:].tolist() == [20] * (BINS - 17)
    assert not L.owners(np.zeros((2, BINS))).any()
    assert np.all(L.owners(np.arange(BINS)[None, :]) == BINS - 1)
    assert not L.owners(np.full((1, BINS), np.nan)).any()
    o = L.owners(_row(b0=2.0, b1024=3.0))[0]
    assert o[:513].tolist() == [0] * 513 and o[513:].tolist() == [1024] * 512
    rng = np.random.default_rng(1)
    rows = np.concatenate([rng.uniform(0, 1, (4, BINS)), rng.integers(0, 4, (4, BINS)).astype(np.float64)])
    got = L.owners(rows)
    for k, row in enumerate(rows):
        assert np.array_equal(got[k], _owners_slow(row.astype(np.float32))), k
        pk = L.peaks(row)
        assert np.array_equal(got[k][pk], pk)                            # a peak owns itself


# ------------------------------------------------------------------ the scan against its chains
def _synthetic(K, seed, empties=0.1):
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0, 1, (K, BINS)).astype(np.float32)
    au, av = rng.uniform(-np.pi, np.pi, (2, K, BINS))
    empty = rng.uniform(size=K) < empties
    return mag, np.exp(1j * au), np.exp(1j * av), empty


def test_lock_scan_is_the_chain_walk():
    K = 40
    mag, U, V, empty = _synthetic(K, 2)
    own = L.owners(mag).astype(np.int64)
    phi = L.lock_scan(mag, U, V, empty)
    r = R.resets(empty)
    assert r[0] and r[1:].sum() >= 2
    rng = np.random.default_rng(3)
    for k, b in zip(rng.integers(0, K, 300), rng.integers(0, BINS, 300)):
        chain, kk, bb = [], int(k), int(b)
        while not r[kk]:                      # the one predecessor of (frame, bin)
            o = own[kk, bb]
            chain.append(V[kk, bb] if o == bb else V[kk, o] * U[kk, bb] * np.conj(U[kk, o]))
            kk, bb = kk - 1, int(o)
        z = V[kk, bb]
        for m in reversed(chain):
            z = z * m
        assert abs(phi[k, b] - z / abs(z)) <= 1e-12, (k, b)
    assert np.array_equal(phi[r], V[r])       # a reset frame is V itself
    # handed-in owners are used as they are
    assert np.array_equal(L.lock_scan(mag, U, V, empty, own=L.owners(mag)), phi)
    one = np.zeros_like(own)
    ref = L.lock_scan(mag, U, V, np.zeros(K, bool), own=one)
    assert abs(ref[5, 7] - R.ph(ref[4, 0] * V[5, 0] * U[5, 7] * np.conj(U[5, 0]))) <= 1e-15


# ------------------------------------------------------------------ identities
def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def test_identity_at_unit_ratio():
    x = _noise(6000, 4)
    (s,) = L.stretch_locked([x], R.Q)
    assert len(s) == len(x) and np.max(np.abs(s[R.N:-R.N] - x[R.N:-R.N])) <= 1e-12
    y = _noise(6000, 5)
    a, b = L.stretch_locked([x, y], R.Q)
    assert np.max(np.abs(a[R.N:-R.N] - x[R.N:-R.N])) <= 1e-12
    assert np.max(np.abs(b[R.N:-R.N] - y[R.N:-R.N])) <= 1e-12


def test_identical_channels_linked_equal_mono_locked():
    x = (0.5 * _noise(9000, 6)).astype(np.float32)          # x + x is exact in float32
    for P in (890_899, 1_122_462):
        (mono,) = L.stretch_locked([x], P)
        a, b = L.stretch_locked([x, x], P)
        assert np.array_equal(a, b)
        assert np.max(np.abs(a - mono)) <= 1e-12
    with pytest.raises(ValueError):
        L.stretch_locked([x, x[:-1]], R.Q)
    assert [len(s) for s in L.stretch_locked([x[:0], x[:0]], R.Q)] == [0, 0]
    ys = L.pitch_shift_locked([x, x], 1.0)
    assert [len(y) for y in ys] == [len(x)] * 2 and np.array_equal(ys[0], ys[1])


# ------------------------------------------------------------------ what the mode buys
def test_locked_keeps_the_level_of_a_voiced_tone():
    x = vibrato_tone()
    P = 1_122_462
    (locked,) = L.stretch_locked([x], P)
    plain = R.stretch(x.astype(np.float32), P)
    lk, pl = locked[4096:-4096], plain[4096:-4096]
    print(f"vibrato tone: locked rms ratio {rms(lk) / rms(x):.3f} spread {running_rms_spread(lk):.3f}, "
          f"plain rms ratio {rms(pl) / rms(x):.3f}")
    assert rms(lk) / rms(x) >= 0.95
    assert running_rms_spread(lk) >= 0.9
    assert rms(pl) / rms(x) <= 0.85


@pytest.mark.parametrize("P", [890_899, 1_122_462])
def test_linked_keeps_a_centred_source_centred(P):
    left, right = stereo_pair()
    cut = slice(4096, -4096)
    a, b = L.stretch_locked([left, right], P)
    pa, pb = R.stretch(left.astype(np.float32), P), R.stretch(right.astype(np.float32), P)
    (ia,), (ib,) = L.stretch_locked([left], P), L.stretch_locked([right], P)
    res = [unexplained(left, right), unexplained(pa[cut], pb[cut]), unexplained(ia[cut], ib[cut]),
           unexplained(a[cut], b[cut])]
    print(f"stereo pair P={P}: input {res[0]:.3f} plain {res[1]:.3f} locked {res[2]:.3f} linked {res[3]:.3f}")
    assert res[3] <= 0.16
    assert res[1] >= 0.40
    assert res[3] < res[2] < res[1]


# ------------------------------------------------------------------ host-side checks
def test_host_side_argument_checks(tmp_path):
    from nightcore_analyzer import cli, ops, render
    x = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="phase_lock"):
        render.pitch_shift(x, 1.0, phase_lock="identity")
    with pytest.raises(ValueError, match="phase_lock"):
        render.pitch_file(tmp_path / "a.wav", tmp_path / "b.wav", 1.0, phase_lock=1)
    with pytest.raises(ValueError, match="phase_lock"):
        render.refine_pitch(x, x, start=2.0, phase_lock=None)
    with pytest.raises(ValueError):                       # the shift is still checked first
        render.pitch_shift(x, 12.5, phase_lock=True)
    with pytest.raises(ValueError, match="lock"):
        ops.pv_stretch_device(None, [x], R.Q, lock="laroche")
    with pytest.raises(ValueError, match="lock"):
        ops.pitch_shift_device(None, [x], 1.0, lock=True)
    assert ops.PV_LOCKS == (None, "identity")
    info = render.PitchInfo(tmp_path / "b.wav", 1.0, 0, 1, 44100, "pcm16", 0.0, 0.0, 0)
    assert info.phase_lock is False
    assert render.PitchInfo(tmp_path / "b.wav", 1.0, 0, 1, 44100, "pcm16", 0.0, 0.0, 0, phase_lock=True).phase_lock
    from nightcore_analyzer.engine import Engine
    assert set(Engine.PV_LOCK_TAGS) >= {"pv_lock_prep", "pv_lock_tile", "pv_lock_carry", "pv_lock_apply",
                                        "pv_mid_sum", "pv_rotate"}
    assert not set(Engine.PV_LOCK_TAGS) & {"pv_scan_tile", "pv_scan_carry", "pv_scan_apply"}

    ncp, srp = tmp_path / "nc.wav", tmp_path / "src.wav"
    ncp.write_bytes(b"")
    srp.write_bytes(b"")
    out, err = stdio.StringIO(), stdio.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = cli.main(["-n", str(ncp), "-s", str(srp), "--phase-lock"])
    assert rc == 2 and "--phase-lock needs --pitch-correct" in err.getvalue() and out.getvalue() == ""
    assert err.getvalue().count("needs") == 1
