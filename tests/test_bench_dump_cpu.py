"""bench.py's --dump-outputs writer and its options, on the CPU (no device): the arrays a caller of
the timed path received, one value per pair for every result figure and the per-window / per-chunk
detail arrays concatenated in batch order, as float64 .npy files of finite values; --full and
--dump-outputs are off by default."""
import sys

import numpy as np

import bench
from nightcore_analyzer import consensus as C
from nightcore_analyzer import engine as E
from nightcore_analyzer.sharded import RES_FIELDS


def _outcome(i, n_win, n_chunks):
    r = C.AnalysisResult(tempo_ratio=1.25 + i, pitch_ratio=1.2, tempo_ci=(1.2, 1.3), pitch_ci=(1.1, 1.3),
                         classification="x", n_source_pitch_windows=n_chunks, n_nc_pitch_windows=n_chunks,
                         n_source_tempo_windows=n_win, n_nc_tempo_windows=n_win, nc_duration=144.0,
                         src_duration=180.0, nc_median_bpm=150.0, src_median_bpm=120.0)
    d = dict(energy_src=np.arange(n_win, dtype=np.float32) + i, energy_nc=np.ones(n_win + 1, np.float32),
             src_tempos=[120.0, None, 121.0][:n_win], nc_tempos=[150.0] * n_win, nc_start_bpm=np.float64(150.0),
             tempo_margin_src=np.zeros(n_win), tempo_margin_nc=np.zeros(n_win),
             chunk_lags=np.arange(n_chunks, dtype=np.int64), chunk_lag_margin=np.full(n_chunks, 0.5),
             tuning=np.zeros(2 * n_chunks, np.float32), tuning_margin=None,
             chroma=np.arange(24 * n_chunks, dtype=np.float32).reshape(-1, 12))
    return E.PairOutcome(result=r, detail=d)


def test_dump_outputs_writes_rows_and_detail(tmp_path):
    outs = [_outcome(0, 3, 2), _outcome(1, 2, 1), E.PairOutcome(error=RuntimeError("gated"))]
    bench.dump_outputs(tmp_path / "d", outs)
    arrays = {f.name[:-4]: np.load(f) for f in (tmp_path / "d").iterdir()}
    absent = {"ibi_ratio", "ibi_lo", "ibi_hi", "intro_offset_sec"}     # None in every pair: no file
    computed = [f for f in RES_FIELDS if f not in absent]
    data = {f"result_{f}" for f in computed} | set(bench.DUMP_DETAIL)
    masks = {f"result_{f}_missing" for f in computed if f != "ok"} | {"src_tempos_missing"}
    assert set(arrays) == data | masks | {f"{n}_count" for n in bench.DUMP_DETAIL}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) < 64 << 20
    assert arrays["result_ok"].tolist() == [1.0, 1.0, 0.0]
    assert arrays["result_tempo_ratio"].tolist() == [1.25, 2.25, 0.0]  # the failed pair: 0.0, marked missing
    assert arrays["result_tempo_ratio_missing"].tolist() == [0.0, 0.0, 1.0]
    assert arrays["result_tempo_lo"].tolist() == [1.2, 1.2, 0.0]
    assert arrays["energy_src"].tolist() == [0.0, 1.0, 2.0, 1.0, 2.0]
    assert arrays["energy_src_count"].tolist() == [3.0, 2.0, 0.0]
    assert arrays["src_tempos"].tolist() == [120.0, 0.0, 121.0, 120.0, 0.0]      # None -> 0.0 + mask
    assert arrays["src_tempos_missing"].tolist() == [0.0, 1.0, 0.0, 0.0, 1.0]
    assert arrays["nc_start_bpm"].tolist() == [150.0, 150.0]
    assert arrays["chunk_lags"].tolist() == [0.0, 1.0, 0.0]
    assert arrays["chroma_count"].tolist() == [48.0, 24.0, 0.0]
    assert arrays["tuning_margin"].size == 0 and arrays["tuning_margin_count"].tolist() == [0.0, 0.0, 0.0]


def test_dump_outputs_marks_infinities(tmp_path):
    o = _outcome(0, 3, 2)
    o.detail["energy_src"] = np.array([-np.inf, 1.0, np.inf], np.float32)
    bench.dump_outputs(tmp_path / "d", [o])
    assert np.load(tmp_path / "d" / "energy_src.npy").tolist() == [0.0, 1.0, 0.0]
    assert np.load(tmp_path / "d" / "energy_src_missing.npy").tolist() == [3.0, 0.0, 2.0]
    assert not (tmp_path / "d" / "energy_nc_missing.npy").exists()


def test_dump_outputs_is_repeatable(tmp_path):
    outs = [_outcome(0, 3, 2), _outcome(1, 2, 1)]
    bench.dump_outputs(tmp_path / "a", outs)
    bench.dump_outputs(tmp_path / "b", outs)
    for f in (tmp_path / "a").iterdir():
        assert f.read_bytes() == (tmp_path / "b" / f.name).read_bytes()


def test_full_and_dump_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert (a.full, a.dump_outputs) == (True, "out")
