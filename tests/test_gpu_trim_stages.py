"""GPU stage tests of the silence trim and the window energies: what trim_blocks_kernel,
frame_base_kernel, trim_bounds_kernel and window_energy_blocks_kernel (csrc/trim.hip) and
window_energy_kernel (csrc/glue.hip) write, against the exact f64 reference of
tests/trim_cases.py (qualified on the CPU by test_trim_cases_cpu.py).

Bounds are demanded exactly on every case at every top_db of 20, 40, 60 and 80: the CPU
qualification shows that no frame stands within 1e-3 dB of a threshold, ten times the f32
rounding of the kernel and of the oracle together.  The two tables at the head of the trim's
workspace (frame_base: exclusive scan of 1 + N // 512, tile_base: of ceil(ceil(N / 512) / 16))
are exact.  Every block sum the trim writes is within relative 1e-12 of the correctly rounded
(math.fsum) sum: 512 f64 fused multiply-adds of non-negative terms and the wave tree lose at
most 520 * 2^-53 = 6e-14; a block of zeros gives exactly 0.0.  Window energies are within 1e-9 dB
of 20 log10(max(sqrt(fsum(x^2) / L), 1e-10)), the project's figure
(test_gpu_components.test_window_energy_from_trim_blocks), in both forms and between them; a
window of zeros gives exactly -200.0.

Offsets off the 4-sample grid: trim_blocks_kernel's scalar branch gives each lane the samples
lane + 64 q of a block, its float4 branch the samples 4 lane + 256 q .. + 3, so the two sum a
block in different orders and their f64 sums differ in the last bits: on an MI355X 39 of the
197 block sums of this test do.  The test therefore holds the block sums of the shifted files to
relative 1e-12 of the aligned run's (both are within 6e-14 of the exact sum) and prints how many
differ at all; the bounds are demanded equal.  Blocks that take the scalar branch in both runs
(a file's last tile) are demanded bit for bit.
"""
import numpy as np
import pytest
import torch

import trim_cases as TC
from nightcore_analyzer import engine as E
from nightcore_analyzer import ops

pytestmark = pytest.mark.gpu

BLOCK_RTOL = 1e-12
ENERGY_TOL_DB = 1e-9


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return E.get_engine(0)


# --------------------------------------------------------------------------- helpers
def _read_ws(ws, lens):
    """(frame_base [n + 1], tile_base [n + 1], block sums [frames]) of a finished trim workspace."""
    n = len(lens)
    frames = int(np.sum(1 + np.asarray(lens, np.int64) // 512))
    raw = ws.cpu().numpy()
    head = 8 * (n + 1)
    return (raw[:head].view(np.int64).copy(), raw[head:2 * head].view(np.int64).copy(),
            raw[2 * head:2 * head + 8 * frames].view(np.float64).copy())


def _check_tables_and_blocks(tag, ws, files, exact):
    """The tables exactly; every slot with a block against the fsum value; -> the largest relative error."""
    lens = [len(y) for y in files]
    fb, tb, blk = _read_ws(ws, lens)
    assert np.array_equal(fb, TC.frame_base(lens)), tag
    assert np.array_equal(tb, TC.tile_base(lens)), tag
    worst = 0.0
    for f, ex in enumerate(exact):
        got = blk[fb[f]:fb[f] + len(ex.blocks)]
        assert len(ex.blocks) == (lens[f] + 511) // 512
        zero = ex.blocks == 0.0
        assert np.all(got[zero] == 0.0), (tag, f)
        if (~zero).any():
            rel = np.abs(got[~zero] - ex.blocks[~zero]) / ex.blocks[~zero]
            assert rel.max() <= BLOCK_RTOL, (tag, f, float(rel.max()))
            worst = max(worst, float(rel.max()))
    return worst


class Packed:
    """Files in one hand-packed device buffer at the given sample offsets, for direct calls of
    nc_trim_bounds, nc_window_energy_blocks and nc_window_energy."""

    def __init__(self, eng, files, offsets):
        self.eng, self.files = eng, files
        self.off = np.asarray(offsets, np.int64)
        self.len = np.array([len(y) for y in files], np.int64)
        assert np.all(self.off[1:] >= (self.off + self.len)[:-1])           # no two files overlap
        host = np.zeros(int((self.off + self.len).max()) + 64, np.float32)
        for y, o in zip(files, self.off):
            host[o:o + len(y)] = y
        self.buf = torch.from_numpy(host).to(eng.dev)
        self.d_off = torch.from_numpy(self.off).to(eng.dev)
        self.d_len = torch.from_numpy(self.len).to(eng.dev)
        self.n = len(files)
        self.frames = int(np.sum(1 + self.len // 512))
        self.ws_bytes = int(eng.ctx.lib.nc_trim_workspace_bytes(self.len.ctypes.data, self.n))

    def trim(self, top_db, fill=None):
        """-> (start, end, workspace); fill: the byte the workspace holds before the call."""
        eng = self.eng
        ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=eng.dev)
        if fill is not None:
            ws.fill_(fill)
        se = torch.full((2 * self.n,), -7, dtype=torch.int64, device=eng.dev)
        eng.call("nc_trim_bounds", self.buf.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n,
                 self.frames, float(top_db), se[:self.n].data_ptr(), se[self.n:].data_ptr(), ws.data_ptr(),
                 ws.numel(), eng.stream())
        h = se.cpu().numpy()
        return h[:self.n].copy(), h[self.n:].copy(), ws

    def energies_from_blocks(self, ws, wins, L):
        """nc_window_energy_blocks of the windows [(file, start)] of L samples from a trim workspace."""
        eng = self.eng
        d_off = torch.tensor([int(self.off[f]) + s for f, s in wins], dtype=torch.int64, device=eng.dev)
        d_file = torch.tensor([f for f, _ in wins], dtype=torch.int32, device=eng.dev)
        out = torch.full((len(wins),), 777.0, dtype=torch.float64, device=eng.dev)
        eng.call("nc_window_energy_blocks", self.buf.data_ptr(), ws.data_ptr(), self.n, self.d_off.data_ptr(),
                 d_off.data_ptr(), d_file.data_ptr(), len(wins), int(L), out.data_ptr(), eng.stream())
        return out.cpu().numpy()

    def energies_direct(self, wins, L):
        """nc_window_energy of the same windows: f64 sums over the samples themselves."""
        eng = self.eng
        d_off = torch.tensor([int(self.off[f]) + s for f, s in wins], dtype=torch.int64, device=eng.dev)
        out = torch.full((len(wins),), 777.0, dtype=torch.float64, device=eng.dev)
        eng.call("nc_window_energy", self.buf.data_ptr(), d_off.data_ptr(), len(wins), int(L), out.data_ptr(),
                 eng.stream())
        return out.cpu().numpy()


def _aligned_offsets(files):
    off, pos = [], 0
    for y in files:
        off.append(pos)
        pos += (len(y) + 63) // 64 * 64
    return off


def _launch(eng, sig, f0, f1, top_db):
    return eng._trim_launch(sig, f0, f1, E.Params(silence_strip_db=top_db), torch.cuda.current_stream(eng.dev),
                            pinned=False)


# --------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("name", TC.NAMES)
def test_single_file_bounds_equal_exact_reference(eng, name):
    y = TC.signal(name)
    for top_db in TC.TOP_DBS:
        got, = ops.trim_bounds(eng, [y], top_db)
        assert got == TC.exact(name, top_db).bounds, (name, top_db, got)
        if name == "spike":
            assert got == TC.SPIKE_BOUNDS[top_db]


@pytest.mark.parametrize("layout", TC.BATCHES)
def test_batch_in_one_launch_equals_per_file_results(eng, layout):
    """65 files (the second round of the wave-ballot file search) and 300 files (the second tile
    of the prefix tables), empty files first, last and in runs between the others."""
    files = list(TC.batch(layout))
    for top_db in TC.TOP_DBS:
        got = ops.trim_bounds(eng, files, top_db)
        assert got == [ex.bounds for ex in TC.batch_exact(layout, top_db)], (layout, top_db)
    # a few of them alone: one launch per file gives what the batch gave
    top_db = 40.0
    exp = TC.batch_exact(layout, top_db)
    for f in (0, 1, 2, len(files) // 3, len(files) // 2 + 2, len(files) - 5, len(files) - 1):
        assert ops.trim_bounds(eng, [files[f]], top_db) == [exp[f].bounds], (layout, f)


# --------------------------------------------------------------------------- block sums and tables
@pytest.mark.parametrize("layout", ("cases",) + TC.BATCHES)
def test_block_sums_and_tables(eng, layout):
    if layout == "cases":
        files = [TC.signal(n) for n in TC.NAMES]
        exact = [TC.exact(n, 60.0) for n in TC.NAMES]
    else:
        files, exact = list(TC.batch(layout)), TC.batch_exact(layout, 60.0)
    sig = eng.upload_signals(files)
    tr = _launch(eng, sig, 0, len(files), 60.0)
    start, end = tr.bounds()
    assert list(zip(start.tolist(), end.tolist())) == [ex.bounds for ex in exact]
    worst = _check_tables_and_blocks(layout, tr.ws, files, exact)
    print(f"[block sums] {layout}: {len(files)} files, largest relative error {worst:.2e} (bound {BLOCK_RTOL:.0e})")


# --------------------------------------------------------------------------- offsets off the grid
OFF_GRID = ("len_8193", "len_2049", "step_513", "len_32775", "len_513", "fades", "len_2048", "denormals")


def test_offsets_off_the_four_sample_grid(eng):
    """Files at offsets 1, 2 and 3 past a multiple of 4 (the scalar branch on every tile) and one
    on the grid, packed with no more than 3 samples between them, so that a read past a file's
    end meets its neighbour's samples, not padding."""
    files = [TC.signal(n) for n in OFF_GRID]
    shift = [1, 2, 3, 0, 3, 1, 2, 1]
    off, pos = [], 0
    for y, s in zip(files, shift):
        o = (pos + 3) // 4 * 4 + s
        off.append(o)
        pos = o + len(y)
    assert [o % 4 for o in off] == shift and all(b - (a + len(y)) <= 6 for a, b, y in zip(off, off[1:], files))
    a = Packed(eng, files, _aligned_offsets(files))
    p = Packed(eng, files, off)
    n_diff = n_blocks = 0
    for top_db in TC.TOP_DBS:
        sa, ea, wa = a.trim(top_db)
        sp, ep, wp = p.trim(top_db)
        exp = [TC.exact(n, top_db).bounds for n in OFF_GRID]
        assert list(zip(sa.tolist(), ea.tolist())) == exp, top_db
        assert list(zip(sp.tolist(), ep.tolist())) == exp, top_db
    exact = [TC.exact(n, 60.0) for n in OFF_GRID]
    _check_tables_and_blocks("aligned", wa, files, exact)
    _check_tables_and_blocks("shifted", wp, files, exact)
    fb, _, ba = _read_ws(wa, a.len)
    _, _, bp = _read_ws(wp, p.len)
    for f, ex in enumerate(exact):
        nblk = len(ex.blocks)
        ga, gp = ba[fb[f]:fb[f] + nblk], bp[fb[f]:fb[f] + nblk]
        assert np.all(np.abs(ga - gp) <= BLOCK_RTOL * ex.blocks), f
        # a wave's 4 blocks take the scalar branch in both runs when they reach past the file's end
        n_vec = len(files[f]) // 2048 * 4
        assert np.array_equal(ga[n_vec:], gp[n_vec:]), f
        if shift[f] == 0:
            assert np.array_equal(ga, gp), f
        n_diff += int(np.sum(ga != gp))
        n_blocks += nblk
    print(f"[off grid] {n_diff} of {n_blocks} block sums differ in their last bits between the two load branches")


# --------------------------------------------------------------------------- stale workspace, window energies
@pytest.fixture(scope="module")
def energy_setup(eng):
    """The window-energy files, trimmed twice by the same direct call: into a workspace of zeros
    and into one filled with 0xFF bytes (NaN doubles, -1 in the tables).  The energies of part B
    are fed from the second."""
    files = list(TC.energy_files())
    p = Packed(eng, files, _aligned_offsets(files))
    clean = p.trim(60.0, fill=0x00)
    stale = p.trim(60.0, fill=0xFF)
    return p, clean, stale


def test_stale_workspace_bytes_reach_no_result(eng, energy_setup):
    p, (s0, e0, w0), (s1, e1, w1) = energy_setup
    exact = [TC.exact_trim(y, 60.0) for y in p.files]
    assert list(zip(s0.tolist(), e0.tolist())) == [ex.bounds for ex in exact]
    assert np.array_equal(s0, s1) and np.array_equal(e0, e1)
    _check_tables_and_blocks("stale", w1, p.files, exact)
    fb0, tb0, b0 = _read_ws(w0, p.len)
    fb1, tb1, b1 = _read_ws(w1, p.len)
    assert np.array_equal(fb0, fb1) and np.array_equal(tb0, tb1)
    written = np.zeros(len(b0), bool)
    for f, n in enumerate(p.len):
        written[fb0[f]:fb0[f] + (n + 511) // 512] = True
    assert np.array_equal(b0[written], b1[written])
    # the slots no block writes (the last one of a file of a multiple of 512 samples) keep what they held
    assert (~written).sum() == sum(1 for n in p.len if n % 512 == 0) >= 2
    assert np.all(b0[~written] == 0.0) and np.all(np.isnan(b1[~written]))
    # and the same with files of 0 and 512 samples in the batch: single slots that stay unwritten
    files = [np.zeros(0, np.float32), TC.signal("len_512"), np.zeros(0, np.float32), TC.signal("len_1025")]
    q = Packed(eng, files, _aligned_offsets(files))
    for top_db in TC.TOP_DBS:
        sa, ea, _ = q.trim(top_db, fill=0x00)
        sb, eb, wb = q.trim(top_db, fill=0xFF)
        exp = [TC.exact_trim(y, top_db).bounds for y in files]
        assert list(zip(sa.tolist(), ea.tolist())) == exp and list(zip(sb.tolist(), eb.tolist())) == exp, top_db
    assert np.isnan(_read_ws(wb, q.len)[2]).sum() == 3


@pytest.mark.parametrize("L", TC.WIN_LENGTHS)
def test_window_energies_both_forms(eng, energy_setup, L):
    """Every window of trim_cases.energy_windows at this length in one launch of each form; the
    block-sum form reads the workspace that held 0xFF bytes before the trim."""
    p, _, (_, _, ws) = energy_setup
    wins = TC.energy_windows()[L]
    ref = np.array([TC.exact_energy_db(p.files[f][s:s + L]) for f, s in wins])
    blocks = p.energies_from_blocks(ws, wins, L)
    direct = p.energies_direct(wins, L)
    zero = ref == -200.0
    assert zero.any() == (L <= 2100)
    for tag, got in (("blocks", blocks), ("direct", direct)):
        assert np.all(np.isfinite(got)), (tag, L)
        assert np.all(got[zero] == -200.0), (tag, L)
        assert np.max(np.abs(got - ref)) <= ENERGY_TOL_DB, (tag, L, float(np.max(np.abs(got - ref))))
    assert np.max(np.abs(blocks - direct)) <= ENERGY_TOL_DB
    print(f"[window energy] L {L}: {len(wins)} windows, largest difference blocks {np.max(np.abs(blocks - ref)):.2e}, "
          f"direct {np.max(np.abs(direct - ref)):.2e} dB (tolerance {ENERGY_TOL_DB:.0e})")
    # fewer than four windows, and a count that is no multiple of four: four waves share a workgroup
    for k in (1, 3, 5):
        assert np.array_equal(p.energies_from_blocks(ws, wins[:k], L), blocks[:k]), (L, k)


# --------------------------------------------------------------------------- sub-range
SUB_RANGE = ("len_2049", "step_0", "len_8192", "fades", "len_2560", "step_2047", "denormals")


def test_sub_range_trim_and_its_window_energies(eng):
    """Engine._trim_launch over files [2, 7) of a 7-file batch: those files' bounds and block
    sums, and _Trim.window_energies with win_file counted from file 2 gives bit for bit what the
    trim of the whole batch gives with win_file counted from file 0."""
    files = [TC.signal(n) for n in SUB_RANGE]
    sig = eng.upload_signals(files)
    f0, L = 2, 1537
    wins = [(f, s) for f in range(f0, len(files)) for s in (0, 1, 511, 513, len(files[f]) - L)]
    ref = np.array([TC.exact_energy_db(files[f][s:s + L]) for f, s in wins])
    d_off = torch.tensor([int(sig.off[f]) + s for f, s in wins], dtype=torch.int64, device=eng.dev)
    got = {}
    for first in (f0, 0):
        for top_db in ((20.0, 60.0) if first else (60.0,)):
            tr = _launch(eng, sig, first, len(files), top_db)
            assert (tr.f0, tr.f1) == (first, len(files))
            start, end = tr.bounds()
            exact = [TC.exact(n, top_db) for n in SUB_RANGE[first:]]
            assert list(zip(start.tolist(), end.tolist())) == [ex.bounds for ex in exact], (first, top_db)
            _check_tables_and_blocks(f"files [{first}, 7)", tr.ws, files[first:], exact)
        d_file = torch.tensor([f - first for f, _ in wins], dtype=torch.int32, device=eng.dev)
        out = torch.full((len(wins),), 777.0, dtype=torch.float64, device=eng.dev)
        tr.window_energies(d_off, d_file, len(wins), L, out.data_ptr())
        got[first] = out.cpu().numpy()
        assert np.max(np.abs(got[first] - ref)) <= ENERGY_TOL_DB, first
    assert np.array_equal(got[f0], got[0])
