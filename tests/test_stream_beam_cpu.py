"""CPU checks of the carried CTC prefix beam search: the float64 restatement of the carried state (tests/stream_beam_ref.py) against the
whole-utterance restatement (tests/ctc_prefix_beam_ref.py) under every chunk schedule tests/test_gpu_stream_beam.py uses, the row
behaviours the interface states, and what the library answers without a device (the state's size, the argument checks)."""
import pytest
import torch

import ctc_prefix_beam_ref as R
import stream_beam_ref as SB

PAIRS = [(name, W, spec) for (name, W) in R.CASES for spec in SB.SCHEDULES[(name, W)]]


def test_every_case_has_a_schedule():
    assert sorted(SB.SCHEDULES) == sorted(R.CASES)
    assert SB.calls(70, [1, 64, 5]) == [(0, 1), (1, 64), (65, 5)] and SB.calls(6, 4) == [(0, 4), (4, 2)]
    assert len(SB.calls(400, 64)) == 7
    assert SB.frames_of([6, 4, 0], 4, 2) == [2, 0, 0]


@pytest.mark.parametrize('name,W,spec', PAIRS, ids=[f'{n}-{w}-{s}' for n, w, s in PAIRS])
def test_chunked_restatement_equals_the_whole(name, W, spec):
    e, il, capacity = R.inputs(name)
    T, N, _ = e.shape
    e64 = e.double()
    carried = SB.CarriedBeam(N, W, capacity)
    for i, (off, size) in enumerate(SB.calls(T, spec)):
        carried.advance(e64[off:off + size], SB.frames_of(il.tolist(), off, size), [i == 0] * N)
    for n in range(N):
        want, _, _ = R.beam_row(e64[:, n], int(il[n]), capacity, W)
        got = carried.nbest(n)
        assert [y for y, _ in got] == [y for y, _ in want]
        assert all(abs(a - b) <= 1e-12 for (_, a), (_, b) in zip(got, want))


def test_rows_without_frames_begins_and_re_begins():
    e, il, capacity = R.inputs('small')
    e64 = e.double()
    c = SB.CarriedBeam(3, 4, capacity)
    assert c.nbest(0) == []                                             # never begun: no hypothesis
    c.advance(e64[:2], [2, 0, 0], [True, True, False])
    assert c.nbest(1) == [((), 0.0)] and c.nbest(2) == []               # a begin with 0 frames: the empty hypothesis alone, score 0
    before = [list(r) if r is not None else None for r in c.rows]
    c.advance(e64[2:4], [0, 2, 0], None)                                # row 0 gets 0 frames: unchanged
    assert c.rows[0] == before[0] and c.rows[2] is None
    assert c.nbest(1) == R.beam_row(e64[2:4, 1], 2, capacity, 4)[0]
    c.advance(e64[:3], [3, 9, -1], [True, False, True])                 # row 0 begins again; n_frames clamps to [0, T]
    assert c.nbest(0) == R.beam_row(e64[:, 0], 3, capacity, 4)[0]
    assert c.nbest(1) == R.beam_row(torch.cat([e64[2:4, 1], e64[:3, 1]]), 5, capacity, 4)[0]
    assert c.nbest(2) == [((), 0.0)]


def test_state_bytes_and_limits():
    from haloop_amd import _lib, ops
    size = _lib.lib().halo_ctc_prefix_beam_state_bytes
    assert ops.PREFIX_BEAM_MAX_CAPACITY == 8192 >= 1024
    assert size(32, 4, 256) == 512 + 2 * 4 * 256                        # token rows worked on in LDS: one copy of 16-bit tokens
    assert size(32, 16, 384) == 512 + 2 * 16 * 384                      # 2 W capacity = 12288 still fits
    assert size(32, 16, 385) == 512 + 8 * 16 * 385                      # ... above it both copies of 32-bit tokens live in the state
    assert size(70000, 2, 2) == 512 + 8 * 2 * 2                         # tokens above 16 bits
    assert size(5, 1, 3) == 512 + 16                                    # rounded up to 16 bytes
    assert size(32, 16, 1024) > 0 and size(32, 16, 8192) == 512 + 8 * 16 * 8192
    for V, beam, capacity in ((1, 4, 8), (2 ** 26 + 1, 4, 8), (32, 0, 8), (32, 17, 8), (32, 4, 0), (32, 4, 8193)):
        assert size(V, beam, capacity) == 0


def test_argument_checks():
    from haloop_amd import _lib, ctc
    for kwargs in (dict(beam=0), dict(beam=17), dict(capacity=0), dict(capacity=8193)):
        with pytest.raises(ValueError):
            ctc.PrefixBeamStream(2, 5, **kwargs)
    with pytest.raises(ValueError):
        ctc.PrefixBeamStream(0, 5)
    with pytest.raises(ValueError):
        ctc.PrefixBeamStream(2, 1)
    with pytest.raises(_lib.HaloError):
        ctc.PrefixBeamStream(2, 5, device='cpu')                        # no CPU path
