"""The plain-Python statement of the encoder's level 0 choice rule (tests/flac_enc_ref.py), which
the GPU tests compare the device's bytes with: it must itself be a lossless FLAC encoder with
the right headers, and give the hand-computed answers.  No GPU."""
import numpy as np
import pytest

import flac_enc_ref as E
import flac_ref as R


@pytest.mark.parametrize("name", list(E.cases()))
def test_reference_encoder_round_trips(name):
    pcm, bps, rate, block = E.cases()[name]
    data = E.encode(pcm, bps, rate, block)
    st = R.decode(data)
    assert np.array_equal(st.pcm, pcm)
    assert (st.rate, st.channels, st.bps, st.stored_total) == (rate, pcm.shape[0], bps, pcm.shape[1])
    assert st.md5 == R.md5_of(pcm, bps)
    sizes = [end - start for start, end, *_ in st.frames]
    n_frames = -(-pcm.shape[1] // block)
    assert len(sizes) == n_frames
    assert data[:4] == b"fLaC" and data[4] == 0x80 and int.from_bytes(data[5:8], "big") == 34      # STREAMINFO, last
    assert int.from_bytes(data[8:10], "big") == int.from_bytes(data[10:12], "big") == block
    assert int.from_bytes(data[12:15], "big") == min(sizes) and int.from_bytes(data[15:18], "big") == max(sizes)
    for i, (start, end, first, blk, assign, fbps, hdr) in enumerate(st.frames):
        assert first == i * block and blk == min(block, pcm.shape[1] - first)
        h = R.parse_frame_header(data, start, bps)
        assert h["number"] == i and not h["variable"]
        assert (data[start + 2] >> 4) == R.block_code(blk)
        assert (data[start + 2] & 15) == E.RATE_CODE.get(rate, 0)
        assert ((data[start + 3] >> 1) & 7) == E.BITS_CODE.get(bps, 0)
        # never longer than all-VERBATIM with the widest header
        assert end - start <= 16 + (pcm.shape[0] * (8 + blk * (bps + 1)) + 7) // 8 + 2


def test_spike_partition_takes_k9_and_a_run_of_117():
    x = E.spike_partition()
    u = E.fold(x)
    assert sorted(set(u.tolist())) == [0, 60000]
    assert E.rice_partition(u, 14) == (9, 64 * 10 + 117) and 60000 >> 9 == 117
    # by hand: k = 8 costs 64 * 9 + 234 = 810, k = 10 costs 64 * 11 + 58 = 762, k = 9 costs 757
    assert [64 * (k + 1) + (60000 >> k) for k in (8, 9, 10)] == [810, 757, 762]
    # an odd block has one partition: the rule keeps that k, and the stream holds the run
    pcm, bps, rate, block = E.cases()["spike_run117"]
    data = E.encode(pcm, bps, rate, block)
    (assign, (sub,)), = E.describe(data)
    assert assign == 0 and sub == ("fixed", 0, 0, [9])
    # subframe header, residual header, k, 37 codes of zero, then 117 zeros before the spike's stop bit
    br = R.BitReader(data, 42 + R.parse_frame_header(data, 42, 16)["hdr_len"])
    assert (br.read(8), br.read(6), br.read(4)) == (8 << 1, 0, 9)
    assert all((br.unary(), br.read(9)) == (0, 0) for _ in range(37))
    assert (br.unary(), br.read(9)) == (117, 60000 & 511)


def test_constant_block():
    cost, spec = E.choose([-5] * 4096, 16, 0)
    assert (cost, spec) == (24, dict(type="constant"))
    # a block of one zero sample: FIXED order 0 (8 + 6 + 4 + 1 = 19 bits) beats CONSTANT (8 + 24 = 32)
    cost, spec = E.choose([0], 24, 1)
    assert cost == 8 + 6 + 5 + 1 and spec["type"] == "fixed" and spec["params"] == [0]
    data = E.encode(np.full((1, 100), 77), 8, 8000, 64)
    assert [f for f in E.describe(data)] == [(0, [("constant", 0, 0, [])])] * 2
    # per frame: header 4 + number 1 + block size tail 1 + CRC-8 1, subframe (8 + 8 bits) 2, CRC-16 2
    assert len(data) == 42 + 2 * (7 + 2 + 2)


def test_equal_channels_take_left_side_with_a_constant_side():
    pcm, bps, rate, block = E.cases()["left_equals_right"]
    for assign, subs in E.describe(E.encode(pcm, bps, rate, block)):
        assert assign == 8 and subs[1] == ("constant", 0, 0, [])
    pcm, bps, rate, block = E.cases()["left_equals_minus_right"]
    for assign, subs in E.describe(E.encode(pcm, bps, rate, block)):
        assert assign in (1, 8, 9, 10) and len(subs) == 2


def _search(width: int, n: int, lo: int, hi: int, want):
    """The first random signal (seeded) for which ``want(candidates)`` holds."""
    rng = np.random.default_rng(3)
    for _ in range(5000):
        x = rng.integers(lo, hi, n)
        if want(E.fixed_candidates(x, width, 0)):
            return x
    raise AssertionError("no such signal found")


def test_ties_resolve_in_the_stated_order():
    # k: four residuals of u = 2 cost 4 (k + 1) + 4 (2 >> k) = 12 bits at k = 0, 1 and 2: the smallest k
    assert E.rice_partition([2, 2, 2, 2], 14) == (0, 12)
    # (order, partition order): two candidates share the smallest cost; the smaller order, then the
    # smaller partition order is kept

    def shared_minimum(cands):
        best = min(c[0] for c in cands)
        return sum(c[0] == best for c in cands) > 1 and best < 8 + 16 * 8
    x = _search(8, 16, -3, 4, shared_minimum)
    cands = E.fixed_candidates(x, 8, 0)
    ties = [c for c in cands if c[0] == min(c[0] for c in cands)]
    cost, spec = E.choose(x, 8, 0)
    assert len(ties) > 1 and (spec["order"], spec["po"]) == min((c[1], c[2]) for c in ties) and cost == ties[0][0]
    # silence in two channels: every assignment costs the same, 1 (left, right) is kept
    assign, subs = E.choose_frame(np.zeros((2, 64), np.int64), 16)
    assert assign == 1 and [s["type"] for s in subs] == ["constant", "constant"]
    # FIXED before VERBATIM: a 4-bit signal whose best FIXED cost is exactly 8 + 17 * 4 bits
    x = _search(4, 17, -4, 4, lambda cands: min(c[0] for c in cands) == 8 + 17 * 4)
    cost, spec = E.choose(x, 4, 0)
    assert cost == 8 + 17 * 4 and spec["type"] == "fixed"
    # CONSTANT before FIXED: one 4-bit sample of 0 costs 8 + 4 as CONSTANT; FIXED order 0 costs 8 + 6 + 4 + 1
    assert E.choose([0], 4, 0) == (12, dict(type="constant"))
