"""nightcore_analyzer.launch without a device: every launcher in each of its modes against a fake
engine that records what would be launched.  Checks what the ABI's arity test cannot see: the
entry point chosen, every argument's kind against its ctypes type, and every pointer's place.
Shapes: n = 2, T = 3, acw = 4 (win_n 1024, hop 512 at a rate of 256), two chunks, two jobs."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nightcore_analyzer import consensus as C
from nightcore_analyzer import launch
from nightcore_analyzer._native import SIGNATURES
from nightcore_analyzer.engine import _DevSpan, percentile_params

_empty, _zeros = torch.empty, torch.zeros
STREAM, WS_BYTES = 7, 4096
HOP, WIN_N, RATE, N, T, ACW = 512, 1024, 256, 2, 3, 4
_ISZ = {torch.float64: 8, torch.float32: 4, torch.int64: 8, torch.int32: 4, torch.uint8: 1, torch.uint64: 8}


class _Ws:
    """A workspace: CPU bytes, and the streams recorded on it."""

    def __init__(self, nbytes):
        self.t, self.streams = _empty(nbytes, dtype=torch.uint8), []

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return self.t.numel()

    def record_stream(self, s):
        self.streams.append(s)


class _Lib:
    """ctx.lib: every nc_*_workspace_bytes returns WS_BYTES and records its arguments."""

    def __init__(self):
        self.queries = []

    def __getattr__(self, name):
        assert name.startswith("nc_") and name.endswith("_workspace_bytes"), name

        def query(*args):
            self.queries.append((name, args))
            return WS_BYTES
        return query


class FakeEngine:
    dev = torch.device("cpu")

    def __init__(self):
        self.ctx = SimpleNamespace(lib=_Lib(), h=ctypes.c_void_p(1))
        self.calls, self.ws, self.stream_queries = [], {}, 0

    def stream(self):
        self.stream_queries += 1
        return STREAM

    def workspace(self, name, nbytes):
        assert name not in self.ws, "one workspace per launch"
        self.ws[name] = (_Ws(max(1, nbytes)), nbytes)
        return self.ws[name][0]

    def call(self, name, *args):
        self.calls.append((name, args))


class _Carver:
    """_DevSpans carved from one CPU byte buffer, as the groups' uploads and arenas are."""

    def __init__(self):
        self.buf, self.pos = _zeros(1 << 14, dtype=torch.uint8), 0

    def __call__(self, n, dtype):
        self.pos = (self.pos + 15) & ~15
        s = _DevSpan(self.buf, self.buf.data_ptr() + self.pos, n, dtype, _ISZ[dtype])
        self.pos += n * _ISZ[dtype]
        return s


@pytest.fixture
def eng():
    return FakeEngine()


@pytest.fixture
def span():
    return _Carver()


@pytest.fixture
def allocs(monkeypatch):
    """Counts torch.empty / torch.zeros calls made from here on."""
    count = []
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (count.append("empty"), _empty(*a, **k))[1])
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (count.append("zeros"), _zeros(*a, **k))[1])
    return count


def check_abi(name, args):
    """Arity and every argument's kind against the entry point's ctypes signature."""
    types = SIGNATURES[name][1][1:]                 # Context.call prepends the context handle
    assert len(args) == len(types), (name, len(args), len(types))
    for i, (a, t) in enumerate(zip(args, types)):
        if t is ctypes.c_void_p:
            assert a is None or type(a) is int, (name, i, a)
        elif t in (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t):
            assert type(a) is int, (name, i, a)
        else:
            assert t in (ctypes.c_float, ctypes.c_double) and type(a) is float, (name, i, a)


def only_call(eng, name):
    (got, args), = eng.calls
    assert got == name
    check_abi(name, args)
    return args


def ws_of(eng, tag, nbytes=WS_BYTES):
    (name, (ws, asked)), = eng.ws.items()
    assert name == tag and asked == nbytes
    return ws


class _Stream:
    cuda_stream = 99


EV = SimpleNamespace(cuda_event=1234)


# ------------------------------------------------------------------------------ window_stage
@pytest.mark.parametrize("with_energy", [True, False])
@pytest.mark.parametrize("with_tuning", [True, False])
def test_window_stage(eng, span, allocs, with_energy, with_tuning):
    buf, win_off = span(4096, torch.float32), span(N, torch.int64)
    energy = span(N, torch.float64) if with_energy else None
    tuning = (span(N, torch.int32), span(3, torch.int64), 1, span(8, torch.float32), span(8, torch.float32),
              span(N, torch.int32), EV) if with_tuning else None
    tag = "sp_win" if with_tuning else "win"
    onset, tg, t, acw = launch.window_stage(eng, buf, win_off, N, WIN_N, HOP, RATE, energy=energy, tuning=tuning,
                                            **({"ws_tag": tag} if with_tuning else {}))
    assert allocs == ["empty", "empty"]             # onset and tg, nothing else
    assert (t, acw) == (T, ACW)
    assert (onset.dtype, onset.numel(), tg.dtype, tg.numel()) == (torch.float32, N * T, torch.float64, N * ACW)
    ws = ws_of(eng, tag)
    assert eng.ctx.lib.queries == [("nc_window_stage_workspace_bytes", (eng.ctx.h, N, WIN_N, HOP))]
    args = only_call(eng, "nc_window_stage_tuning" if with_tuning else "nc_window_stage")
    head = (buf.data_ptr(), win_off.data_ptr(), None, N, WIN_N, HOP, onset.data_ptr(), tg.data_ptr(),
            energy.data_ptr() if with_energy else None)
    mid = tuple(x.data_ptr() for x in tuning[:2]) + (1,) + tuple(x.data_ptr() for x in tuning[3:6]) + (1234,) \
        if with_tuning else ()
    assert args == head + mid + (ws.data_ptr(), WS_BYTES, STREAM)
    assert ws.streams == [] and eng.stream_queries == 1


# ------------------------------------------------------------------------------ tempo_beats
@pytest.mark.parametrize("long_windows", [False, True])
def test_tempo_beats_group_mode(eng, span, allocs, long_windows):
    """The groups' second launch: spans sliced past the source windows, outputs given, the stream's
    handle passed on (no query here); a workspace for all the windows' frames only when they are long."""
    k = 1                                           # n_src_w
    total = (N + k) * T if long_windows else 0
    onset, tg = span((N + k) * T, torch.float32), _zeros((N + k) * ACW, dtype=torch.float64)
    off, length = span(N + k, torch.int64), span(N + k, torch.int32)
    start, pidx, active = span(N, torch.float64), span(N, torch.int32), span(N + k, torch.uint8)
    res = [span(N + k, dt) for dt in (torch.float64, torch.int32, torch.int32, torch.float64)]
    del allocs[:]
    out = launch.tempo_beats(eng, onset, off[k:], length[k:], N, T, tg[k * ACW:], ACW, start, HOP, prior_idx=pidx,
                             active=active[k:], out=[x[k:] for x in res], total=total, st=55)
    assert allocs == [] and eng.stream_queries == 0
    if long_windows:
        ws = ws_of(eng, "beats")
        assert ws.streams == [] and eng.ctx.lib.queries == [("nc_tempo_beats_workspace_bytes", (total,))]
    else:
        assert eng.ws == {} and eng.ctx.lib.queries == []
    assert [a.data_ptr() for a in out] == [x.data_ptr() + k * x.isz for x in res]
    assert only_call(eng, "nc_tempo_beats") == (
        onset.data_ptr(), off.data_ptr() + 8 * k, length.data_ptr() + 4 * k, N, T, tg.data_ptr() + 8 * k * ACW, ACW,
        start.data_ptr(), pidx.data_ptr(), active.data_ptr() + k, HOP, 1, res[0].data_ptr() + 8 * k,
        res[1].data_ptr() + 4 * k, res[2].data_ptr() + 4 * k, res[3].data_ptr() + 8 * k, None, total,
        *((ws.data_ptr(), WS_BYTES) if long_windows else (None, 0)), 55)


def test_tempo_beats_seam_mode(eng, span, allocs):
    """The seams: outputs omitted (zero-filled), no prior index, no active flags, always a workspace."""
    onset, tg = span(N * T, torch.float32), span(N * ACW, torch.float64)
    off, length, start = span(N, torch.int64), span(N, torch.int32), span(N, torch.float64)
    bpm, lag, nb, mg = launch.tempo_beats(eng, onset, off, length, N, T, tg, ACW, start, HOP, total=N * T,
                                          ws_tag="sp_beats")
    assert allocs == ["zeros"] * 4 and eng.stream_queries == 1
    assert [(x.dtype, x.numel()) for x in (bpm, lag, nb, mg)] == \
        [(torch.float64, N), (torch.int32, N), (torch.int32, N), (torch.float64, N)]
    assert not any(x.any() for x in (bpm, lag, nb, mg))
    ws = ws_of(eng, "sp_beats")
    assert eng.ctx.lib.queries == [("nc_tempo_beats_workspace_bytes", (N * T,))]
    assert only_call(eng, "nc_tempo_beats") == (
        onset.data_ptr(), off.data_ptr(), length.data_ptr(), N, T, tg.data_ptr(), ACW, start.data_ptr(), None, None,
        HOP, 1, bpm.data_ptr(), lag.data_ptr(), nb.data_ptr(), mg.data_ptr(), None, N * T, ws.data_ptr(), WS_BYTES,
        STREAM)


@pytest.mark.parametrize("stream", [None, 55])
def test_beats_to_ibis(eng, span, stream):
    """Both launches on one stream: the caller's handle, or the current stream asked for once."""
    total, st = 2 * T, stream or STREAM
    onset, fbase, lens = span(total, torch.float32), span(N + 1, torch.int64), span(N, torch.int32)
    tg, start, pidx = span(N * ACW, torch.float64), span(N, torch.float64), span(N, torch.int32)
    r = launch.beats_to_ibis(eng, onset, fbase, lens, N, T, tg, ACW, start, pidx, 64, 4, total, "sp_ibi_beats",
                             st=stream)
    assert eng.stream_queries == (stream is None)
    assert sorted(r) == ["beats", "bpm", "ibis", "lag", "margin", "nbeats", "nibi"]
    assert (r["beats"].dtype, r["beats"].numel()) == (torch.int32, total)
    assert (r["ibis"].dtype, r["ibis"].numel()) == (torch.float64, total)
    assert (r["nibi"].dtype, r["nibi"].numel(), int(r["nibi"].sum())) == (torch.int32, N, 0)
    ws = ws_of(eng, "sp_ibi_beats")
    assert eng.ctx.lib.queries == [("nc_tempo_beats_workspace_bytes", (total,))]
    assert [name for name, _ in eng.calls] == ["nc_tempo_beats", "nc_ibi_from_beats"]
    for name, args in eng.calls:
        check_abi(name, args)
    assert eng.calls[0][1] == (
        onset.data_ptr(), fbase.data_ptr(), lens.data_ptr(), N, T, tg.data_ptr(), ACW, start.data_ptr(),
        pidx.data_ptr(), None, 64, 1, r["bpm"].data_ptr(), r["lag"].data_ptr(), r["nbeats"].data_ptr(),
        r["margin"].data_ptr(), r["beats"].data_ptr(), total, ws.data_ptr(), WS_BYTES, st)
    assert eng.calls[1][1] == (r["beats"].data_ptr(), fbase.data_ptr(), r["nbeats"].data_ptr(), N, 64, 4,
                               r["ibis"].data_ptr(), r["nibi"].data_ptr(), st)


def test_ibi_lists_and_sizes():
    vals, fbase = np.arange(10.0), np.array([0, 5, 7, 10])
    got = launch.ibi_lists(vals, np.array([4, 1, 0], np.int32), fbase, 4)
    assert got[0].tolist() == [0.0, 1.0, 2.0, 3.0] and got[1] is None and got[2] is None
    got = launch.ibi_lists(vals, np.array([4, 1, 0], np.int32), fbase, 1)
    assert got[1].tolist() == [5.0] and got[2] is None
    got[0][0] = -1.0
    assert vals[0] == 0.0                            # copies
    assert launch.frames_of(WIN_N, HOP) == T and launch.tempogram_window(RATE, HOP) == ACW
    assert launch.frames_of(np.array([220500, 511]), 512).tolist() == [431, 1]
    assert (launch.tempogram_window(22050, 512), launch.tempogram_window(22050, 64)) == (344, 2756)
    assert type(launch.tempogram_window(22050, 512)) is int


# ------------------------------------------------------------------------------ chroma
@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("with_shared", [True, False])
def test_chroma_mean(eng, span, allocs, given, with_shared):
    buf, off, length = span(4096, torch.float32), span(2, torch.int64), span(2, torch.int64)
    outs = dict(chroma=span(24, torch.float32), tuning=span(2, torch.float32), tmargin=span(2, torch.int32)) \
        if given else {}
    shared = (span(2, torch.int32), 5, span(8, torch.float32), span(8, torch.float32), span(2, torch.int32), EV) \
        if with_shared else None
    s = _Stream() if given else None                 # the groups' side stream; the seams' current stream
    tag = "chroma" if given else "sp_chroma"
    chroma, tuning, tmargin = launch.chroma_mean(eng, buf, off, length, 2, 3000, 2000, shared=shared, stream=s,
                                                 ws_tag=tag, **outs)
    if given:
        assert allocs == [] and (chroma, tuning, tmargin) == (outs["chroma"], outs["tuning"], outs["tmargin"])
    else:
        assert allocs == ["empty", "empty"] and tmargin is None
        assert (chroma.dtype, chroma.numel(), tuning.dtype, tuning.numel()) == (torch.float32, 24, torch.float32, 2)
    ws = ws_of(eng, tag)
    assert ws.streams == ([s] if given else [])
    assert eng.ctx.lib.queries == [("nc_chroma_workspace_bytes", (eng.ctx.h, 2, 3000))]
    args = only_call(eng, "nc_chroma_mean_shared" if with_shared else "nc_chroma_mean")
    mid = (shared[0].data_ptr(), 5, shared[2].data_ptr(), shared[3].data_ptr(), shared[4].data_ptr(), 1234) \
        if with_shared else ()
    assert args == (buf.data_ptr(), off.data_ptr(), length.data_ptr(), 2, 3000, 2000, chroma.data_ptr(),
                    tuning.data_ptr(), None, tmargin.data_ptr() if given else None) + mid + \
        (ws.data_ptr(), WS_BYTES, 99 if given else STREAM)


@pytest.mark.parametrize("given", [True, False])
def test_chroma_lag_margin(eng, span, allocs, given):
    chroma, si, ni = span(24, torch.float32), span(1, torch.int32), span(1, torch.int32)
    outs = dict(lag=span(1, torch.int32), margin=span(1, torch.float64), stream=_Stream()) if given else {}
    lag, margin = launch.chroma_lag_margin(eng, chroma, si, ni, 1, **outs)
    if given:
        assert allocs == [] and (lag, margin) == (outs["lag"], outs["margin"])
    else:
        assert allocs == ["empty", "empty"]
        assert (lag.dtype, lag.numel(), margin.dtype, margin.numel()) == (torch.int32, 1, torch.float64, 1)
    assert only_call(eng, "nc_chroma_lag_margin") == (chroma.data_ptr(), si.data_ptr(), ni.data_ptr(), 1,
                                                      lag.data_ptr(), margin.data_ptr(), 99 if given else STREAM)
    assert eng.ws == {}


# ------------------------------------------------------------------------------ bootstrap_ratio
@pytest.mark.parametrize("mode", ["group", "tensor"])
def test_bootstrap_ratio(eng, span, allocs, mode):
    nj = 2
    vals, a_off, a_n = span(16, torch.float64), span(nj, torch.int64), span(nj, torch.int32)
    seed, wsoff, cap = span(4 * nj, torch.uint64), span(nj, torch.int64), span(nj, torch.int32)
    pct = percentile_params(C.N_BOOTSTRAP, C.CI_LEVEL)
    if mode == "group":                             # a span of the arena, both sides, the tail stream
        b_off, b_n, out = span(nj, torch.int64), span(nj, torch.int32), span(3 * nj, torch.float64)
        s, kw, n_boot = _Stream(), {}, C.N_BOOTSTRAP
    else:                                           # a tensor, one array per job, the current stream
        b_off, b_n, out, s, kw, n_boot = None, None, _empty(3 * nj, dtype=torch.float64), None, dict(n_boot=500), 500
        pct = percentile_params(500, 0.9)
    del allocs[:]
    assert launch.bootstrap_ratio(eng, vals, a_off, a_n, b_off, b_n, nj, seed, pct, 3, out, wsoff, cap, "boot_s", 1234,
                                  stream=s, **kw) is None
    assert allocs == []
    ws = ws_of(eng, "boot_s", 1234)
    assert ws.streams == ([s] if s else []) and eng.ctx.lib.queries == []
    args = only_call(eng, "nc_bootstrap_ratio")
    assert args == (vals.data_ptr(), a_off.data_ptr(), a_n.data_ptr(), b_off.data_ptr() if b_off is not None else None,
                    b_n.data_ptr() if b_n is not None else None, nj, n_boot, seed.data_ptr(), *pct, 3,
                    out[0:nj].data_ptr(), out[nj:2 * nj].data_ptr(), out[2 * nj:3 * nj].data_ptr(), None,
                    wsoff.data_ptr(), cap.data_ptr(), ws.data_ptr(), ws.numel(), 99 if s else STREAM)
    assert args[13] == out.data_ptr() and args[14] - args[13] == args[15] - args[14] == 8 * nj
