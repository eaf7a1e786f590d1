"""GPU parity of the beat tracker (csrc/beat.hip) across periods, lengths and both memory paths,
and of the small kernels around it (nc_tempo_prior, nc_ibi_from_beats, nc_energy_gate,
nc_collect_valid), each against the CPU oracle or plain numpy on the same inputs.

The cases come from tests/beat_cases.py; tests/test_beat_cases_cpu.py establishes that every one
compared exactly here is robust to the differences in intermediates the kernel is allowed."""
import numpy as np
import pytest
import torch

import beat_cases as bc
from beat_launch import run_beats
from oracle import ncref
from nightcore_analyzer import _dev
from nightcore_analyzer.engine import beat_needs_workspace

pytestmark = pytest.mark.gpu

SR = bc.SR


def _launch(ctx, cases, trim=1, extra=()):
    """One launch of same-(hop, acw) cases, packed back to back; extra: onsets appended after
    them (with a one-hot tg at lag 17), e.g. a long one that puts the whole launch on the
    workspace path."""
    hop, acw = cases[0].hop, cases[0].acw
    assert all(c.hop == hop and c.acw == acw for c in cases)
    onsets = [bc.case_onset(c) for c in cases] + list(extra)
    tg = np.stack([bc.case_tg(c) for c in cases] + [bc.one_hot_tg(acw, 17 if hop >= 512 else 168)] * len(extra))
    return run_beats(ctx, onsets, tg, [bc.START_BPM] * len(onsets), hop=hop, trim=trim)


def _compare_exact(cases, out, trim=True):
    bad = []
    for s, c in enumerate(cases):
        _, ref = bc.oracle(c, trim)
        what = []
        if out.lag[s] != c.P:
            what.append(("lag", int(out.lag[s])))
        if out.bpm[s] != 60.0 * SR / (c.hop * c.P):
            what.append(("bpm", float(out.bpm[s])))
        if out.nbeats[s] != len(ref):
            what.append(("nbeats", int(out.nbeats[s]), len(ref)))
        if not np.array_equal(out.beats[s], ref):
            k = min(len(ref), len(out.beats[s]))
            diff = np.flatnonzero(out.beats[s][:k] != ref[:k])
            what.append(("beats differ from index", int(diff[0]) if len(diff) else k))
        if what:
            bad.append((c, what))
        bc.check_invariants(out.beats[s], c.N, c.P)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from the oracle: {bad[:8]}"


def _by(cases, *keys):
    out = {}
    for c in cases:
        out.setdefault(tuple(getattr(c, k) for k in keys), []).append(c)
    return out


def _exact_key(c):       # one launch per (group, hop, N); the oracle is slow at long periods: those apart
    return (c.group, c.hop, c.N, "P>=1000" if c.P >= 1000 and c.N >= 2600 else "all")


EXACT = {}
for _c in bc.grid() + bc.radix_cases() + bc.rank_cases():
    EXACT.setdefault(_exact_key(_c), []).append(_c)


@pytest.mark.parametrize("key", sorted(EXACT), ids=lambda k: "-".join(map(str, k)))
def test_beats_equal_oracle(gpu_ctx, key):
    """lag, bpm, nbeats and the beat frames, bit for bit, for every case of the grid (trim on)."""
    cases = EXACT[key]
    long_path = beat_needs_workspace(key[2], cases[0].acw)
    assert long_path == key[0].endswith(("long", "ibi"))
    _compare_exact(cases, _launch(gpu_ctx, cases))


def _mid_p(cases):
    ps = sorted({c.P for c in cases})
    return ps[len(ps) // 2]


NOTRIM = {k: [c for c in v if c.P == _mid_p(v)] for k, v in _by(bc.grid(), "group", "hop").items()}
NOTRIM.update(_by(bc.radix_cases() + bc.rank_cases(), "group", "hop"))   # ``fade`` keeps its beats only here


@pytest.mark.parametrize("key", sorted(NOTRIM), ids=lambda k: "-".join(map(str, k)))
def test_beats_equal_oracle_without_trim(gpu_ctx, key):
    """trim = 0 for one period of every grid group, and for every median case: only here does the
    last beat that the median selects on a ``fade`` envelope reach the output."""
    cases = NOTRIM[key]
    for sub in _by(cases, "N").values():        # one launch per length: LDS and workspace lengths apart
        _compare_exact(sub, _launch(gpu_ctx, sub, trim=0), trim=False)


def test_sequence_longer_than_max_len_is_a_capacity_error(gpu_ctx):
    """A sequence longer than the max_len the launch was sized for: the tempo is still reported,
    nbeats is -1 and no beat is written; its neighbours are unaffected."""
    cases = [bc.Case("lds", k, N, 13, 512, 344) for N in (40, 431) for k in ("noise", "clicks")]
    assert all(c in bc.grid() for c in cases)
    onsets = [bc.case_onset(c) for c in cases]
    out = run_beats(gpu_ctx, onsets, np.stack([bc.case_tg(c) for c in cases]), [bc.START_BPM] * 4, max_len=40)
    for s, c in enumerate(cases):
        assert out.lag[s] == c.P and out.bpm[s] == 60.0 * SR / (512 * c.P)
        if c.N > 40:
            assert out.nbeats[s] == -1
        else:
            np.testing.assert_array_equal(out.beats[s], bc.oracle(c)[1])


# --------------------------------------------------------------------------- mixed batches
@pytest.mark.parametrize("hop", [512, 64])
@pytest.mark.parametrize("with_long", [False, True])
def test_mixed_batch(gpu_ctx, hop, with_long):
    """Different lengths in one launch at unequal offsets with gaps, an all-zero sequence, an
    inactive one and two priors behind prior_idx.  with_long adds workspace-length sequences,
    so that max_len puts every sequence, the 2-frame one included, on the workspace path."""
    acw = bc.acw_of(hop)
    cases = [c for c in bc.mixed_cases(hop) if with_long or not beat_needs_workspace(c.N, acw)]
    assert any(beat_needs_workspace(c.N, acw) for c in cases) == with_long
    L1, L2 = bc.MIXED_LAGS[hop]
    priors = [60.0 * SR / (hop * L1), 60.0 * SR / (hop * L2)]
    tg2 = np.zeros(acw)
    tg2[[L1, L2]] = 1.0
    onsets = [bc.case_onset(c) for c in cases]
    pidx = [(L1, L2).index(c.P) for c in cases]
    active = [1] * len(cases)
    # an all-zero sequence in the middle, an inactive one (non-zero onset) at the end
    zero_at = 3
    onsets.insert(zero_at, np.zeros(40, np.float32))
    pidx.insert(zero_at, 1)
    active.insert(zero_at, 1)
    onsets.append(bc.envelope("noise", 40, L1, 99))
    pidx.append(0)
    active.append(0)
    n = len(onsets)
    gaps = [(5 * s) % 7 + (s % 3 == 0) * 11 for s in range(n)]
    offs, o = [], 3
    for s in range(n):
        offs.append(o)
        o += len(onsets[s]) + gaps[s]
    out = run_beats(gpu_ctx, onsets, np.tile(tg2, (n, 1)), priors, hop=hop, offs=offs, active=active,
                    prior_idx=pidx)
    for s in (zero_at, n - 1):
        assert (out.bpm[s], out.lag[s], out.nbeats[s], out.margin[s]) == (0.0, 0, 0, 0.0)
    live = [s for s in range(n) if s not in (zero_at, n - 1)]
    for s, c in zip(live, cases):
        prior = priors[pidx[s]]
        rbpm, rlag = ncref.tempo_from_tg(tg2, SR, hop, prior)
        assert rlag == c.P                                  # the prior picks this case's period
        rb, rbeats = ncref.beat_track(onsets[s], SR, hop, prior, tg_mean=tg2)
        assert (out.bpm[s], out.lag[s], out.nbeats[s]) == (rb, rlag, len(rbeats)), c
        np.testing.assert_array_equal(out.beats[s], rbeats, err_msg=str(c))
    if with_long:
        for s, c in zip(live, cases):
            if not beat_needs_workspace(c.N, acw):
                continue
            alone = run_beats(gpu_ctx, [onsets[s]], tg2[None], [priors[pidx[s]]], hop=hop)
            assert (alone.bpm[0], alone.lag[0], alone.nbeats[0]) == (out.bpm[s], out.lag[s], out.nbeats[s])
            assert alone.margin[0] == out.margin[s]
            np.testing.assert_array_equal(alone.beats[0], out.beats[s])


# --------------------------------------------------------------------------- the two paths agree
SHORT = _by([c for c in bc.grid() + bc.grid(weak=True) if not beat_needs_workspace(c.N, c.acw)], "group", "hop")


@pytest.mark.parametrize("key", sorted(SHORT), ids=lambda k: "-".join(map(str, k)))
def test_lds_and_workspace_paths_agree(gpu_ctx, key):
    """Scores and back-pointers of the two paths are specified bit-identical, so every output
    is, ``const`` (whose plateaus the oracle comparison leaves out) included: the same
    sequences alone, and in a launch that a longer sequence puts on the workspace path."""
    cases = SHORT[key]
    acw = cases[0].acw
    _, ws_min = bc.boundary(acw)
    short = _launch(gpu_ctx, cases)
    forced = _launch(gpu_ctx, cases, extra=[bc.envelope("noise", ws_min, 17, 5)])
    bad = []
    for s, c in enumerate(cases):
        bc.check_invariants(short.beats[s], c.N, c.P)
        bc.check_invariants(forced.beats[s], c.N, c.P)
        same = (short.bpm[s] == forced.bpm[s] and short.lag[s] == forced.lag[s] == c.P
                and short.nbeats[s] == forced.nbeats[s] >= 0 and short.margin[s] == forced.margin[s]
                and np.array_equal(short.beats[s], forced.beats[s]))
        if not same:
            bad.append(c)
    assert not bad, f"{len(bad)} of {len(cases)} differ between the paths: {bad[:8]}"


LONG_WEAK = _by([c for c in bc.grid(weak=True) if beat_needs_workspace(c.N, c.acw)], "group", "hop", "N")


@pytest.mark.parametrize("key", sorted(LONG_WEAK), ids=lambda k: "-".join(map(str, k)))
def test_const_invariants_on_the_workspace_path(gpu_ctx, key):
    cases = LONG_WEAK[key]
    out = _launch(gpu_ctx, cases)
    for s, c in enumerate(cases):
        assert out.lag[s] == c.P and out.nbeats[s] >= 0
        bc.check_invariants(out.beats[s], c.N, c.P)


# --------------------------------------------------------------------------- tempo stage
def _oracle_margin(tg, hop, prior):
    score = np.log1p(1e6 * tg) + ncref.tempo_logprior(len(tg), SR, hop, prior)
    top = np.sort(score)[-2:]
    return float(top[1] - top[0])


@pytest.mark.parametrize("hop", [512, 64])
@pytest.mark.parametrize("long_path", [False, True])
def test_tempo_stage(gpu_ctx, hop, long_path):
    """Random non-negative tempogram means at several scales (so the prior weighs in more or
    less) and an all-zero one (prior-only argmax) under four priors: lag and bpm equal
    tempo_from_tg, margin_out equals best minus runner-up within 1e-12 (scores are below 32, an
    f64 ulp there is 7e-15: a handful of log1p / log2 ulps stays far under it)."""
    acw = bc.acw_of(hop)
    rng = np.random.default_rng(400 + hop)
    tgs, priors = [], []
    for prior in (60.0, 120.0, 153.80859375, 240.0):
        for scale in (1.0, 1e-3, 1e-6, 1e-9, 0.0):
            tgs.append(rng.random(acw) * scale)
            priors.append(prior)
    n = len(tgs)
    onsets = [bc.envelope("noise", 40, 17, 11)] * n
    if long_path:
        _, ws_min = bc.boundary(acw)
        onsets = onsets + [bc.envelope("noise", ws_min, 17, 5)]
        tgs = tgs + [bc.one_hot_tg(acw, 17 if hop == 512 else 168)]
        priors = priors + [120.0]
    out = run_beats(gpu_ctx, onsets, np.stack(tgs), priors, hop=hop)
    for s in range(n):
        rbpm, rlag = ncref.tempo_from_tg(tgs[s], SR, hop, priors[s])
        m = _oracle_margin(tgs[s], hop, priors[s])
        assert m > 1e-9, (s, m)
        assert (out.lag[s], out.bpm[s]) == (rlag, rbpm), (s, priors[s])
        assert abs(out.margin[s] - m) <= 1e-12, (s, out.margin[s], m)


# --------------------------------------------------------------------------- nc_tempo_prior
def _prior_ref(bpm, nbeats, active, w0, w1, src_len, nc_len):
    """pipeline.py:174-183 with tempo.py:54-55's four-beat rule."""
    valid = [bpm[w] for w in range(w0, w1) if (active is None or active[w]) and nbeats[w] >= 4]
    nc_dur, src_dur = nc_len / SR, src_len / SR
    if valid and nc_dur > 0 and src_dur > 0:
        return float(np.median(valid)) * (src_dur / nc_dur)
    return 120.0


@pytest.mark.parametrize("with_active", [True, False])
def test_tempo_prior(gpu_ctx, with_active):
    rng = np.random.default_rng(77)
    dev = _dev.device(0)
    sizes = [7, 8, 5, 6, 300, 301, 1, 0, 9, 2]
    w0 = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int32) + 2      # two unused windows first
    w1 = (w0 + np.array(sizes)).astype(np.int32)
    nw = int(w1[-1]) + 3
    lags = rng.integers(9, 41, nw)
    bpm = 60.0 * SR / (512.0 * lags)                     # few distinct tempos: the select meets ties
    bpm = np.where(rng.random(nw) < 0.3, rng.uniform(40, 300, nw), bpm)
    nbeats = rng.integers(0, 30, nw).astype(np.int32)
    nbeats[rng.random(nw) < 0.2] = rng.integers(0, 4)
    active = (rng.random(nw) < 0.7).astype(np.uint8)
    nbeats[w0[2]:w1[2]] = 3                              # pair 2: no window with four beats
    active[w0[3]:w1[3]] = 0                              # pair 3: every window inactive
    nbeats[w0[3]:w1[3]] = 9
    src_len = rng.integers(10 * SR, 300 * SR, len(sizes)).astype(np.int64)
    nc_len = (src_len / rng.uniform(1.1, 1.4, len(sizes))).astype(np.int64)
    nc_len[8] = 0                                        # no duration: the default prior
    act = active if with_active else None
    ref = [_prior_ref(bpm, nbeats, act, int(a), int(b), int(sl), int(nl))
           for a, b, sl, nl in zip(w0, w1, src_len, nc_len)]
    counts = [sum(1 for w in range(a, b) if (act is None or act[w]) and nbeats[w] >= 4) for a, b in zip(w0, w1)]
    assert {c & 1 for c in counts if c} == {0, 1} and counts[2] == 0 and counts[7] == 0
    assert {counts[4] & 1, counts[5] & 1} == {0, 1} and min(counts[4:6]) > 100    # 300 windows > 256 threads
    assert with_active == (counts[3] == 0)
    out = torch.full((len(sizes),), float("nan"), dtype=torch.float64, device=dev)
    t = [_dev.to_dev(x, dev) for x in (bpm, nbeats, w0, w1, src_len, nc_len)]
    d_act = _dev.to_dev(active, dev) if with_active else None
    gpu_ctx.call("nc_tempo_prior", t[0].data_ptr(), t[1].data_ptr(), _dev.ptr(d_act), t[2].data_ptr(),
                 t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), len(sizes), out.data_ptr(),
                 _dev.stream_handle())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.tolist() == ref
    assert got[2] == 120.0 and got[7] == 120.0 and got[8] == 120.0


# --------------------------------------------------------------------------- nc_ibi_from_beats
def _ibi_ref(frames, hop, min_ibis):
    """tempo.py:165-172."""
    if len(frames) < min_ibis + 1:
        return None
    ibis = np.diff(ncref.frames_to_time(frames, SR, hop))
    ibis = ibis[ibis > 0.05]
    return None if len(ibis) < min_ibis else ibis


def test_ibi_from_beats(gpu_ctx):
    hop, min_ibis = 64, 4
    assert 17 * hop / SR < 0.05 < 18 * hop / SR          # 17-frame gaps are glitches, 18-frame ones kept
    rng = np.random.default_rng(31)
    dev = _dev.device(0)
    seqs = []
    for nb in (0, 4, 5, 257, 1000, 1000):
        gaps = rng.choice([17, 18, 19, 150, 151, 400], size=max(0, nb - 1))
        seqs.append(np.concatenate([[rng.integers(0, 50)], gaps]).cumsum()[:nb].astype(np.int32))
    seqs.append(np.cumsum([5, 18, 18, 18, 18]).astype(np.int32))           # 5 beats, 4 kept: the minimum
    seqs.append(np.cumsum([5, 17, 18, 17, 18, 17, 17]).astype(np.int32))   # 7 beats, 2 kept: below it
    seqs.append(np.cumsum([5] + [17] * 40).astype(np.int32))               # nothing kept
    seqs.append((np.cumsum([3] + [400] * 300) + 2_000_000).astype(np.int32))   # frame x hop beyond 2^27
    n = len(seqs)
    offs, o = [], 5
    for s, q in enumerate(seqs):
        offs.append(o)
        o += len(q) + (3 * s) % 5 + 1
    total = o
    buf = np.full(total, -1, np.int32)
    for of, q in zip(offs, seqs):
        buf[of:of + len(q)] = q
    d_b, d_off, d_nb = (_dev.to_dev(x, dev) for x in (buf, np.asarray(offs, np.int64),
                                                      np.asarray([len(q) for q in seqs], np.int32)))
    ibi = torch.full((total,), float("nan"), dtype=torch.float64, device=dev)
    n_ibi = torch.full((n,), -7, dtype=torch.int32, device=dev)
    gpu_ctx.call("nc_ibi_from_beats", d_b.data_ptr(), d_off.data_ptr(), d_nb.data_ptr(), n, hop, min_ibis,
                 ibi.data_ptr(), n_ibi.data_ptr(), _dev.stream_handle())
    torch.cuda.synchronize()
    got, cnt = ibi.cpu().numpy(), n_ibi.cpu().numpy()
    may_write = np.zeros(total, bool)
    kept_some = dropped_some = 0
    for s, q in enumerate(seqs):
        ref = _ibi_ref(q, hop, min_ibis)
        may_write[offs[s]:offs[s] + max(0, len(q) - 1)] = True
        if ref is None:
            assert cnt[s] == 0, (s, cnt[s])
            continue
        assert cnt[s] == len(ref), (s, cnt[s], len(ref))
        assert np.array_equal(got[offs[s]:offs[s] + cnt[s]], ref), s
        kept_some += 1
        dropped_some += len(ref) < len(q) - 1
    assert kept_some >= 5 and dropped_some >= 3
    assert np.all(np.isnan(got[~may_write]))


# --------------------------------------------------------------------------- glue
def _groups(sizes, lead=2, gap_every=4):
    w0, o = [], lead
    for i, s in enumerate(sizes):
        w0.append(o)
        o += s + (1 if i % gap_every == 0 else 0)      # some windows belong to no group
    w0 = np.asarray(w0, np.int32)
    return w0, (w0 + np.asarray(sizes)).astype(np.int32), o + 1


GLUE_SIZES = [0, 1, 63, 64, 65, 200] + [3] * 70        # > 64 groups: collect_valid's second workgroup


def test_energy_gate(gpu_ctx):
    """io.py:115-126: active = energy >= max(group) + gate, a tie at exactly max + gate kept."""
    gate = -40.0
    rng = np.random.default_rng(5)
    dev = _dev.device(0)
    w0, w1, nw = _groups(GLUE_SIZES)
    en = rng.uniform(-90.0, -10.0, nw)
    for a, b in zip(w0, w1):
        if b - a >= 3:
            k = a + int(rng.integers(0, b - a - 2))
            en[k] = -8.5                                 # the group's maximum
            en[k + 1] = -8.5 + gate                      # exactly on the gate: kept
            en[k + 2] = np.nextafter(-8.5 + gate, -np.inf)   # one ulp under it: dropped
    assert -8.5 + gate == -48.5
    act = torch.full((nw,), 7, dtype=torch.uint8, device=dev)
    t = [_dev.to_dev(x, dev) for x in (en, w0, w1)]
    gpu_ctx.call("nc_energy_gate", t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(w0), gate,
                 act.data_ptr(), _dev.stream_handle())
    torch.cuda.synchronize()
    got = act.cpu().numpy()
    ref = np.full(nw, 7, np.uint8)
    for a, b in zip(w0, w1):
        if b > a:
            peak = max(en[a:b])
            ref[a:b] = [e >= peak + gate for e in en[a:b]]
    assert np.array_equal(got, ref)
    assert (ref == 1).sum() > 100 and (ref == 0).sum() > 100 and (ref == 7).sum() >= 3


@pytest.mark.parametrize("with_active", [True, False])
def test_collect_valid(gpu_ctx, with_active):
    """consensus.py:236-240 over tempo.py:54-55: ordered compaction of the active windows with
    at least min_beats beats and a finite positive tempo, and their count per group."""
    rng = np.random.default_rng(6)
    dev = _dev.device(0)
    w0, w1, nw = _groups(GLUE_SIZES)
    bpm = rng.uniform(40.0, 300.0, nw)
    odd = rng.random(nw)
    bpm[odd < 0.08] = np.nan
    bpm[(odd >= 0.08) & (odd < 0.16)] = np.inf
    bpm[(odd >= 0.16) & (odd < 0.20)] = -np.inf
    bpm[(odd >= 0.20) & (odd < 0.28)] = 0.0
    bpm[(odd >= 0.28) & (odd < 0.32)] = -0.0
    bpm[(odd >= 0.32) & (odd < 0.40)] = -120.0
    nbeats = rng.integers(0, 9, nw).astype(np.int32)
    nbeats[rng.random(nw) < 0.05] = -1                   # the tracker's capacity error
    active = (rng.random(nw) < 0.75).astype(np.uint8)
    vals = torch.full((nw,), -777.0, dtype=torch.float64, device=dev)
    cnt = torch.full((len(w0),), -7, dtype=torch.int32, device=dev)
    t = [_dev.to_dev(x, dev) for x in (bpm, nbeats, w0, w1)]
    d_act = _dev.to_dev(active, dev) if with_active else None
    gpu_ctx.call("nc_collect_valid", t[0].data_ptr(), t[1].data_ptr(), _dev.ptr(d_act), t[2].data_ptr(),
                 t[3].data_ptr(), len(w0), 4, vals.data_ptr(), cnt.data_ptr(), _dev.stream_handle())
    torch.cuda.synchronize()
    got, n = vals.cpu().numpy(), cnt.cpu().numpy()
    ref = np.full(nw, -777.0)
    for g, (a, b) in enumerate(zip(w0, w1)):
        keep = [bpm[w] for w in range(a, b) if (not with_active or active[w]) and nbeats[w] >= 4
                and np.isfinite(bpm[w]) and bpm[w] > 0]
        assert n[g] == len(keep), (g, n[g], len(keep))
        ref[a:a + len(keep)] = keep
    assert np.array_equal(got, ref)                      # kept values in order, nothing else written
    assert n[0] == 0 and n.max() > 40
