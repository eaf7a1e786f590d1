"""The launchers on workspaces of exactly the size their query reports (csrc/nc_ws.h: one carve
function gives the size and the pointers).

* ``test_context_bound_sizes``: the two size queries that read a live context's tables return
  what tests/golden/workspace_sizes.json records under ``context_bound`` (taken from the library
  of the commit before the carve functions, on an MI355X).  Nothing is launched.
* ``test_exact_fit_is_enough_and_stays_inside``: every converted launcher runs once on a
  workspace that is a view, 256 bytes into a larger buffer, of exactly the queried size; the
  buffer holds a byte pattern before the run, with 4096 bytes of it after the view.  The outputs
  equal those of the same call on the engine's ordinary (1.1 x, named) workspace and both margins
  come back untouched.  With one byte less the launcher returns the status it has always
  returned and launches nothing: the whole of the short workspace still holds the pattern, so no
  kernel of the stage ran and no output was written (trim, called directly, also shows its
  outputs unwritten).  The beat tracker is the exception: a workspace it cannot use selects its
  LDS path, with equal results.

The workspaces are swapped in where the package asks for them (``Engine.workspace``), so the
launches are the package's own.  Shapes are the smallest at which every section is non-empty and
every kernel of the stage launches; the smallest phase-vocoder file (one sample) has four frames,
the fewest a file can have.
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from golden import make_workspace_sizes as W
from nightcore_analyzer import _native, engine as E, launch, ops

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "workspace_sizes.json").read_text())
SR = 22050
PATTERN = 0xA5
FRONT, BACK = 256, 4096


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


def test_context_bound_sizes(gpu_ctx):
    lib, rec = _native.load(), GOLDEN["context_bound"]
    assert set(rec) == set(W.CONTEXT_CALLS) and {n: [a for a, _ in c] for n, c in rec.items()} == W.context_inputs()
    for name, cases in rec.items():
        assert {a[-1] for a, _ in cases} == {64, 512}, name                  # both hops
        bad = [(a, got, want) for a, want in cases for got in [W.CONTEXT_CALLS[name](lib, gpu_ctx.h, *a)]
               if got != want]
        assert not bad, (name, bad[:5])


# ----------------------------------------------------------------------------- guarded workspaces
class Guarded:
    """Stands in for ``Engine.workspace``: every workspace asked for is a view of exactly the
    bytes asked for (one less for the one named ``short``), FRONT bytes into a pattern-filled buffer."""

    def __init__(self, eng, short=None):
        self.eng, self.short, self.given = eng, short, []

    def __enter__(self):
        self.eng.workspace = self.workspace          # shadows the method on this instance
        return self

    def __exit__(self, *exc):
        del self.eng.workspace
        torch.cuda.synchronize()

    def workspace(self, name, nbytes):
        n = int(nbytes) - (1 if name == self.short else 0)
        buf = torch.full((FRONT + n + BACK,), PATTERN, dtype=torch.uint8, device=self.eng.dev)
        self.given.append((name, buf, n))
        return buf[FRONT:FRONT + n]

    def check_margins(self, expect):
        assert [g[0] for g in self.given] == list(expect), [g[0] for g in self.given]
        for name, buf, n in self.given:
            assert bool((buf[:FRONT] == PATTERN).all()) and bool((buf[FRONT + n:] == PATTERN).all()), name

    def untouched(self, name):
        return all(bool((buf == PATTERN).all()) for nm, buf, _ in self.given if nm == name)


def _noise(n, seed, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    clicks = (t % 5513 < 300) * rng.standard_normal(n)                      # a 4 Hz pulse train of noise bursts
    return (amp * (0.2 * rng.standard_normal(n) + clicks + 0.5 * np.sin(2 * np.pi * 440.0 * t / SR))).astype(np.float32)


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if isinstance(x, E.DeviceSignals):
        return [x.buf.cpu().numpy(), np.asarray(x.off), np.asarray(x.length)]
    if isinstance(x, dict):
        return {k: _host(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    return x


def _up(eng, **arrays):
    up = E._Upload()
    for k, (a, dt) in arrays.items():
        up.add(k, a, dt)
    return up.commit(eng.dev)


# ----------------------------------------------------------------------------- the stages
# name -> (run(eng) -> outputs, [(workspace name, status with one byte less or None), ...] in the
# order the stage asks for them); the statuses are those of the launchers before the carve functions
def _align(eng):
    sig = eng.upload_signals([_noise(4 * SR, 1), _noise(2 * SR, 2)])        # 1 pair: src, nc
    return eng.align_offsets(sig.buf, sig.off[:1], sig.length[:1], sig.off[1:], sig.length[1:], n_speeds=2)


def _spectral(eng):
    return eng.spectral([(_noise(100, 3), SR), (_noise(1100, 4), SR)])     # 1 and 3 frames


def _ibi_core(eng):
    ys = [_noise(25000, 5), _noise(20000, 6)]                               # 391 and 313 hop-64 frames
    sig = eng.upload_signals(ys)
    d = _up(eng, off=(sig.off, np.int64), len=(sig.length, np.int64), start=([120.0, 120.0], np.float64))
    core = eng.ibi_core(sig.buf, d["off"], d["len"], sig.length, d["start"],
                        torch.arange(2, dtype=torch.int32, device=eng.dev), ws_tag="t_")
    out = {k: core[k].cpu().numpy() for k in ("onset", "fbase", "tg", "bpm", "lag", "nbeats", "margin", "nibi")}
    fb = out["fbase"]                                   # beats and ibis are written up to each file's count only
    out["beats"] = [core["beats"].cpu().numpy()[fb[f]:fb[f] + out["nbeats"][f]] for f in range(2)]
    out["ibis"] = [core["ibis"].cpu().numpy()[fb[f]:fb[f] + out["nibi"][f]] for f in range(2)]
    return out


def _ibi_range(eng):
    from nightcore_analyzer.sharded import IBI_TILE, DeviceStages
    ys = [_noise(25000, 7), _noise(20000, 8)]
    sig = eng.upload_signals(ys)
    st = DeviceStages(eng, sig)
    T = 1 + sig.length // 64
    mx = st.ibi_mel(sig.off, sig.length, [0, 10], T)                        # a whole file and a tail share
    on = st.ibi_onset(mx)
    onsets = [on[:T[0]], np.concatenate([np.zeros(10, np.float32), on[T[0]:]])]
    tiles = st.ibi_tiles(onsets, [0, 0], [-(-int(t) // IBI_TILE) for t in T])
    return mx, on, tiles


def _window(eng):
    sig = eng.upload_signals([_noise(12 * SR, 9)])
    off = torch.tensor([0, 30000], dtype=torch.int64, device=eng.dev)       # 2 windows of 10 s
    en = torch.empty(2, dtype=torch.float64, device=eng.dev)
    onset, tg, T, acw = launch.window_stage(eng, sig.buf, off, 2, 220500, 512, SR, energy=en, ws_tag="t_win")
    return onset, tg, en, T, acw


def _chroma(eng):
    out = np.zeros(32, np.int64)
    assert _native.load().nc_chroma_workspace_layout(None, 1, 512, out.ctypes.data, 32) == 26
    d3_tile = int(out[18])                                                  # level-3 outputs per decimate3 workgroup
    ys = [_noise(3, 10), _noise(8 * d3_tile + 200, 11)]                     # under 4 samples; two D3_TILE tiles
    ch, tun, _ = ops.chroma_means(eng, ys)
    return ch, tun


def _pv_stretch(eng):
    return ops.pv_stretch_device(eng, [_noise(1, 12), _noise(9000, 13)], 1059463)[:2]


def _pv_lock(eng):
    return ops.pv_stretch_device(eng, [_noise(1, 14), _noise(9000, 15)], 1059463, lock="identity")[:2]


def _pv_scan(eng):
    mag, v, empty, plan = ops.pv_analyze_device(eng, [_noise(1, 16), _noise(9000, 17)], 943874)
    return ops.pv_scan_device(eng, v, empty, plan.frame_base)


def _limiter(eng):
    return ops.true_peak_limit_device(eng, [3.0 * _noise(5000, 18), 3.0 * _noise(300, 19)], limit_db=-1.0)


STAGES = {
    "align": (_align, [("align", -3)]),
    "spectral": (_spectral, [("spectral", -2)]),
    "ibi onset, tempogram, beat": (_ibi_core, [("t_ibi_on", -3), ("t_ibi_tg", -3), ("t_ibi_beats", None)]),
    "ibi mel range, tiles": (_ibi_range, [("sp_ibi_rng", -3), ("sp_ibi_tg", -3)]),
    "window stage": (_window, [("t_win", -3)]),
    "chroma": (_chroma, [("chroma", -3)]),
    "pvoc stretch": (_pv_stretch, [("pvoc", -2)]),
    "pvoc lock": (_pv_lock, [("pv_lock", -2), ("pv_frames", None)]),
    "pvoc scan": (_pv_scan, [("pv_scan", -2)]),
    "limiter": (_limiter, [("limiter", -2)]),
}


@pytest.mark.parametrize("stage", sorted(STAGES) + ["trim"])
def test_exact_fit_is_enough_and_stays_inside(eng, stage):
    if stage == "trim":
        return _trim(eng)
    run, spaces = STAGES[stage]
    want = _host(run(eng))                                                  # the engine's ordinary workspaces
    torch.cuda.synchronize()
    with Guarded(eng) as g:
        got = _host(run(eng))
    np.testing.assert_equal(got, want)
    g.check_margins([s for s, _ in spaces])
    for name, status in spaces:
        if name == "pv_frames":                                             # a buffer the caller sizes, not a carved workspace
            continue
        with Guarded(eng, short=name) as g:
            if status is None:                                              # beat: its LDS path, equal results
                np.testing.assert_equal(_host(run(eng)), want)
            else:
                with pytest.raises(_native.NativeError, match=rf"failed \({status}\)"):
                    run(eng)
                assert g.untouched(name), name                              # nothing of the stage was launched
        names = [s for s, _ in spaces]
        g.check_margins(names if status is None else names[:names.index(name) + 1])


def _trim(eng):
    """nc_trim_bounds allocates a fresh workspace per launch (its block sums outlive the call), so
    it is called directly: 2 files, one empty."""
    lib, h = _native.load(), eng.ctx.h
    sig = eng.upload_signals([np.zeros(0, np.float32), np.concatenate([np.zeros(3000, np.float32), _noise(6000, 20)])])
    want = _host(eng._trim_all(sig, E.Params())[:2])
    lens = np.ascontiguousarray(sig.length, np.int64)
    d = _up(eng, off=(sig.off, np.int64), len=(lens, np.int64))
    nbytes, frames = int(lib.nc_trim_workspace_bytes(lens.ctypes.data, 2)), int(np.sum(1 + lens // 512))
    need = nbytes - 256                                                      # the launcher does not ask for the slack

    def call(n):
        buf = torch.full((FRONT + n + BACK,), PATTERN, dtype=torch.uint8, device=eng.dev)
        se = torch.full((4,), -77, dtype=torch.int64, device=eng.dev)
        rc = lib.nc_trim_bounds(h, sig.buf.data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), 2, frames,
                                float(E.Params().silence_strip_db), se[:2].data_ptr(), se[2:].data_ptr(),
                                buf[FRONT:].data_ptr(), n, eng.stream())
        torch.cuda.synchronize()
        return rc, se.cpu().numpy(), buf

    for n in (nbytes, need):
        rc, se, buf = call(n)
        assert rc == 0 and np.array_equal(se[:2], want[0]) and np.array_equal(se[2:], want[1]), (n, rc, se, want)
        assert bool((buf[:FRONT] == PATTERN).all()) and bool((buf[FRONT + n:] == PATTERN).all())
    rc, se, buf = call(need - 1)
    assert rc == -3 and (se == -77).all() and bool((buf == PATTERN).all())
