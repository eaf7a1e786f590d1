"""The window -> file index the trim's block-sum energies are looked up with, on the CPU: the
plan form (engine.window_files, from BatchPlan.w0 / w1) and the offset form
(engine.window_files_by_offset, the window-sharded stages') against a brute-force loop."""
import numpy as np
import pytest

from nightcore_analyzer import engine as E

SR = E.SR


def _plan(secs, p, trim=0):
    """plan_batch over files of these lengths (seconds) laid out as upload_signals does
    (64-sample aligned offsets), each trimmed by ``trim`` samples at both ends."""
    length = np.array([int(s * SR) for s in secs], np.int64)
    off = np.concatenate([[0], np.cumsum((length + 63) // 64 * 64)[:-1]]).astype(np.int64)
    start = np.minimum(trim, length // 2)
    return off, E.plan_batch(off, length, start, length - start, p)


def _brute(pl, first=0):
    idx = np.full(pl.n_win, -1, np.int32)
    for f in range(pl.nF):
        for k in range(pl.w0[f], pl.w1[f]):
            idx[k] = f + first
    assert (idx >= 0).all()
    return idx


CASES = {
    # 3 pairs, the second pair's nightcore shorter than a window (no windows of its own)
    "short_file": ([31.0, 40.0, 7.5, 25.0, 22.0, 28.0], E.Params(), 0, 0),
    "src_trim": ([33.0, 41.0], E.Params(src_trim_sec=6.5), 1234, 0),
    "first_file": ([24.0, 30.0, 12.0, 15.0], E.Params(window_sec=2.0, hop_sec=1.0), 777, 6),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_window_files_equal_the_brute_force_loop(name):
    secs, p, trim, first = CASES[name]
    off, pl = _plan(secs, p, trim)
    assert pl.n_win > 0
    if name == "short_file":
        assert pl.w0[2] == pl.w1[2] and pl.f_len[2] < pl.win_n
    got = E.window_files(pl.w0, pl.w1, first)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, _brute(pl, first))
    # ascending offsets: the offset form finds the same files
    by_off = E.window_files_by_offset(off, pl.win_abs)
    assert by_off.dtype == np.int32
    np.testing.assert_array_equal(by_off, _brute(pl))


def test_window_files_by_offset_refuses_unsorted_offsets():
    off, pl = _plan([24.0, 30.0, 12.0, 15.0], E.Params())
    swapped = off[[0, 2, 1, 3]]
    with pytest.raises(ValueError):
        E.window_files_by_offset(swapped, pl.win_abs)
    with pytest.raises(ValueError):                       # equal offsets are not ascending either
        E.window_files_by_offset(np.array([0, 64, 64]), pl.win_abs)
