"""CPU qualification of tests/trim_cases.py: on every case and every top_db the oracle
(ncref.trim, librosa's f32 arithmetic) returns exactly the bounds of the exact f64 reference, and
no frame stands within MARGIN_DB = 1e-3 dB of a threshold, ten times what the f32 steps of the
oracle and of the kernel can move a frame by (trim_cases' docstring).  With that the GPU tests
(test_gpu_trim_stages.py) demand exact bounds with no case left out.  The cases reach the paths
they are meant for.  No GPU.  Figures are printed (pytest -s) next to each condition.

If a changed seed lands a frame inside the band, change the seed, never the band."""
import numpy as np
import pytest

import trim_cases as TC
from oracle import ncref, refglue


def _oracle(y, top_db):
    return tuple(int(v) for v in ncref.trim(y, top_db)[1])


@pytest.mark.parametrize("name", TC.NAMES)
def test_oracle_equals_exact_and_margins_hold(name):
    y = TC.signal(name)
    assert y.dtype == np.float32 and len(y) <= 33_000
    for top_db in TC.TOP_DBS:
        ex = TC.exact(name, top_db)
        assert _oracle(y, top_db) == ex.bounds, (name, top_db)
        assert ex.margin >= TC.MARGIN_DB, (name, top_db, ex.margin)
    print(f"{name}: N {len(y)}, bounds {[TC.exact(name, t).bounds for t in TC.TOP_DBS]}, "
          f"smallest margin {min(TC.exact(name, t).margin for t in TC.TOP_DBS):.3g} dB")


@pytest.mark.parametrize("name", TC.BATCHES)
def test_batch_files_oracle_equals_exact_and_margins_hold(name):
    files = TC.batch(name)
    worst = np.inf
    for top_db in TC.TOP_DBS:
        for i, (y, ex) in enumerate(zip(files, TC.batch_exact(name, top_db))):
            assert _oracle(y, top_db) == ex.bounds, (name, i, top_db)
            assert ex.margin >= TC.MARGIN_DB, (name, i, top_db, ex.margin)
            worst = min(worst, ex.margin)
    print(f"{name}: {len(files)} files, smallest margin {worst:.3g} dB")


def test_smallest_margin_over_everything():
    m = min(TC.exact(n, t).margin for n in TC.NAMES for t in TC.TOP_DBS)
    print(f"smallest margin over {len(TC.NAMES)} cases x {len(TC.TOP_DBS)} top_db: {m:.3g} dB")
    assert len(TC.NAMES) == len(TC.LENGTHS) + len(TC.STEPS) + 6 and m >= TC.MARGIN_DB


def test_exact_reference_on_known_answers():
    """The spike: one sample of 1.0 puts 1 / 2048 into the four frames that hold it, 66.9 dB above
    the clamp that every other frame sits on."""
    for top_db, b in TC.SPIKE_BOUNDS.items():
        assert TC.exact("spike", top_db).bounds == b, top_db
    db = TC.exact("spike", 60.0).db
    assert np.flatnonzero(db == 0.0).tolist() == [3, 4, 5, 6]
    assert np.allclose(db[[0, 1, 2, 7, 8, 9]], -100.0 + 10.0 * np.log10(2048.0), rtol=0, atol=1e-12)
    for name in TC.WHOLE_FILE:
        for top_db in TC.TOP_DBS:
            assert TC.exact(name, top_db).bounds == (0, len(TC.signal(name))), (name, top_db)
    assert np.all(TC.exact("zeros", 60.0).db == 0.0) and np.all(TC.exact("quiet", 60.0).db == 0.0)
    assert TC.exact_trim(np.zeros(0, np.float32), 60.0).bounds == (0, 0)
    # block sums: fsum against a f64 dot product, and the frame count
    y = TC.signal("len_8193")
    ex = TC.exact("len_8193", 60.0)
    assert len(ex.blocks) == 17 and len(ex.db) == 17
    assert np.allclose(ex.blocks[:16], (y[:8192].astype(np.float64).reshape(16, 512) ** 2).sum(1), rtol=1e-13)
    assert ex.blocks[16] == float(y[8192]) ** 2


def test_cases_reach_what_they_are_for():
    # every top_db cuts the fades at another frame; the thirds of the length cases separate 40 from 60
    assert len({TC.exact("fades", t).bounds for t in TC.TOP_DBS}) == 4
    assert TC.exact("len_32775", 40.0).bounds[0] > 0 and TC.exact("len_32775", 60.0).bounds == (0, 32775)
    # the 20 dB threshold falls among the steps that leave about 1 % of a frame to the body
    assert len({TC.exact(f"step_{s}", 20.0).bounds[0] for s in (20, 21, 22, 51, 52)}) == 2
    # without the clamp on the frames the clamp case would lose its ends at top_db = 20
    y = TC.signal("clamp")
    db_unclamped = 10.0 * np.log10(ncref.rms_frames(y).astype(np.float64) ** 2)
    assert (db_unclamped - db_unclamped.max()).min() < -20.0 and TC.exact("clamp", 20.0).bounds == (0, len(y))
    # the denormal head is not zero in f64: its blocks have sums a flush to zero would lose
    assert 0.0 < TC.exact("denormals", 60.0).blocks[0] < 1e-70
    for name in TC.BATCHES:
        lens = [len(y) for y in TC.batch(name)]
        assert len(lens) == {"batch_65": 65, "batch_300": 300}[name] and max(lens) <= 6000
        assert lens[0] == lens[-1] == 0 and lens.count(0) >= 7 and lens.count(1) >= 3
        assert any(a == b == c == 0 for a, b, c in zip(lens[1:], lens[2:], lens[3:-1]))
        assert sum(1 for v in lens if v and v % 512 == 0) >= 6
        tb = TC.tile_base(lens)
        assert np.any(np.diff(tb) == 0) and tb[-1] == sum(((v + 511) // 512 + 15) // 16 for v in lens)
    assert len(TC.batch("batch_65")) > 64 and len(TC.batch("batch_300")) > 256


def test_energy_windows_cover_the_block_edges():
    files = TC.energy_files()
    wins = TC.energy_windows()
    assert set(wins) == set(TC.WIN_LENGTHS)
    assert sum(1 for y in files if len(y) % 512 == 0) >= 2 and any(len(y) % 512 for y in files)
    for L, ws in wins.items():
        assert len(ws) > 4 and all(0 <= s and s + L <= len(files[f]) for f, s in ws)
        ends = [(f, s) for f, s in ws if s + L == len(files[f])]
        assert any(len(files[f]) % 512 == 0 for f, _ in ends) and any(len(files[f]) % 512 for f, _ in ends)
        if L <= 2100:
            assert TC.exact_energy_db(files[3][2000:2000 + L]) == -200.0
    assert any(len(ws) % 4 for ws in wins.values())
    # windows wholly inside one block: no full block between the partial ones (b1 < b0 in the kernel)
    assert any((s + 511) // 512 > (s + L) // 512 for L, ws in wins.items() for _, s in ws)
    y = files[0]
    assert TC.exact_energy_db(y[7:1031]) == pytest.approx(refglue.rms_db(y[7:1031]), abs=1e-11)
