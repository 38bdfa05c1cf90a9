"""CPU checks of tests/resample_ref.py, the float64 restatement the GPU resampling tests compare against, and of the host-side tables of
haloop_amd.features (the packed taps, the stream id): what can be verified of them without torchaudio (parity with it is unpinned).

Figures measured on the restatement: polyphase against the direct sum 4.1e-9 .. 2.3e-8 (the fp32 rounding of the taps), tap sums
1.00004 .. 1.00088, the 1 kHz tone 4.9e-4 .. 7.4e-4 on the interior."""
import os

import numpy as np
import pytest

import resample_ref as R
from haloop_amd import features

SPEED_RATIOS = [(19, 20), (49, 50), (51, 50), (21, 20)]
FILE_RATIOS = [(441, 320), (2, 1), (441, 160), (3, 1)]
RATIOS = SPEED_RATIOS + FILE_RATIOS
PAIRS = [(0, 0), (1, 0), (1, 1), (7, 3), (1234, 5), (2 ** 40 + 17, 9), (2 ** 63 + 5, 2 ** 31 + 1), (99, 10 ** 6)]   # test_gpu_frontend.py's


def _wave(n, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * g.standard_normal(n)


def test_ratios_and_tap_shapes_are_the_stated_ones():
    assert [R.speed_ratio(f) for f in R.FACTORS] == [(19, 20), (49, 50), (1, 1), (51, 50), (21, 20)]
    assert [R.ratio(r, 16000) for r in (22050, 32000, 44100, 48000)] == FILE_RATIOS
    assert [R.ratio(r, 16000) for r in (15200, 15680, 16320, 16800)] == SPEED_RATIOS
    shapes = {(19, 20): (7, 33), (49, 50): (7, 63), (51, 50): (7, 65), (21, 20): (7, 35), (441, 320): (9, 459), (2, 1): (13, 28),
              (441, 160): (17, 475), (3, 1): (19, 41)}
    counts = {(441, 320): {16, 17}, (2, 1): {25}, (441, 160): {33, 34}, (3, 1): {37}}
    for ratio in RATIOS:
        h, width = R.taps(*ratio)
        assert (width, h.shape[1]) == shapes[ratio] and h.shape[0] == ratio[1] and h.dtype == np.float32
        nz = (h != 0).sum(axis=1)
        assert set(nz.tolist()) <= counts.get(ratio, {12, 13}), (ratio, set(nz.tolist()))


@pytest.mark.parametrize('ratio', RATIOS)
def test_polyphase_equals_the_direct_sum(ratio):
    orig, new = ratio
    x = _wave(1000 + orig, orig)
    got, want = R.resample(x, orig, new), R.direct(x, orig, new)
    assert got.shape == want.shape == (R.out_length(1000 + orig, orig, new),)
    print(f'[resample] polyphase vs direct {ratio}: {np.abs(got - want).max():.3e}')
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-7)


def test_output_lengths():
    for orig, new in RATIOS + [(1, 1)]:
        for n in (0, 1, orig - 1, orig, orig + 1, 7 * orig, 7 * orig + 1):
            want = -(-new * n // orig)
            assert R.out_length(n, orig, new) == want
            assert R.resample(np.ones(n), orig, new).shape == (want,)
    # 64-bit: 441 x a minute of 48 kHz audio is past 2^31
    assert R.out_length(48000 * 60 * 10, 441, 160) == -(-160 * 48000 * 600 // 441)


def test_every_phase_sums_to_one():
    for ratio in RATIOS:
        sums = R.taps(*ratio)[0].astype(np.float64).sum(axis=1)
        print(f'[resample] tap sums {ratio}: {sums.min():.5f} .. {sums.max():.5f}')
        np.testing.assert_allclose(sums, 1.0, rtol=0, atol=1e-3)


def test_a_tone_is_resampled_to_the_same_tone():
    for orig, new in SPEED_RATIOS:
        src_rate = 16000.0 * orig / new                      # the rate the waveform is taken to be sampled at
        x = np.sin(2 * np.pi * 1000.0 * np.arange(4000) / src_rate)
        got = R.resample(x, orig, new)
        want = np.sin(2 * np.pi * 1000.0 * np.arange(got.shape[0]) / 16000.0)
        print(f'[resample] 1 kHz tone {(orig, new)}: {np.abs(got - want)[40:-40].max():.3e}')
        np.testing.assert_allclose(got[40:-40], want[40:-40], rtol=0, atol=1e-3)
    x = _wave(777, 3)
    assert np.array_equal(R.resample(x, 1, 1), x)            # equal rates: a copy


def test_factor_draws_and_the_stream_constant():
    from haloop_amd import _lib
    assert R.SPEED_STREAM == _lib.HALO_SPEED_STREAM == 0x53504544
    assert len({_lib.HALO_SPEED_STREAM, _lib.HALO_SPECMASK_STREAM, _lib.HALO_MLM_STREAM, _lib.HALO_GPT_SAMPLE_STREAM}) == 4
    assert _lib.HALO_SPEED_STREAM > 4096 + 4096             # dropout sites: small integers; LoRA sites: 4096 + layer
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'halo.h')).read()
    assert f'#define HALO_SPEED_STREAM 0x{_lib.HALO_SPEED_STREAM:08X}u' in text
    assert f'#define HALO_RESAMPLE_MAX_RATIOS {_lib.HALO_RESAMPLE_MAX_RATIOS}' in text
    for seed, step in PAIRS:
        draws = [R.speed_index(n, seed, step) for n in range(64)]
        assert all(0 <= d < 5 for d in draws) and len(set(draws)) >= 3
        assert draws == [R.speed_index(n, seed, step) for n in range(64)]
    seen = np.bincount([R.speed_index(n, 7, 3) for n in range(4096)], minlength=5)
    assert (seen > 0).all() and seen.sum() == 4096
    assert [R.speed_index(n, 7, 3) for n in range(64)] != [R.speed_index(n, 7, 4) for n in range(64)]
    assert all(R.speed_index(n, 7, 3, 1) == 0 for n in range(16))


def test_packed_tables_are_the_dense_taps():
    """haloop_amd.features.resample_taps: first non-zero tap, count and the packed run of every phase reproduce the restatement's dense
    [new, K] table (to one float32 rounding: the two are evaluated by different float64 libraries), the zeros exactly."""
    for ratio in RATIOS:
        dense, width = R.taps(*ratio)
        w, stride, phases, packed = features.resample_taps(*ratio)
        phases, packed = phases.numpy(), packed.numpy()
        assert w == width and stride % 2 == 1 and packed.shape == (ratio[1], stride) and phases.shape == (2, ratio[1])
        rebuilt = np.zeros_like(dense)
        for p in range(ratio[1]):
            lo, cnt = phases[:, p]
            assert 0 <= lo and 1 <= cnt <= stride and lo + cnt <= dense.shape[1]
            assert packed[p, 0] != 0 and packed[p, cnt - 1] != 0 and (packed[p, cnt:] == 0).all()
            rebuilt[p, lo:lo + cnt] = packed[p, :cnt]
        assert np.array_equal(rebuilt != 0, dense != 0)
        np.testing.assert_allclose(rebuilt, dense, rtol=0, atol=2.0 ** -24)
    assert max(s * n for (_, n), s in ((r, features.resample_taps(*r)[1]) for r in RATIOS)) <= 5600       # 22.4 KB: every table fits LDS
    w, stride, phases, packed = features.resample_taps(1, 1)
    assert (w, stride, phases.tolist(), packed.tolist()) == (0, 1, [[0], [1]], [[1.0]])


def test_lds_budget_is_checked_on_the_host():
    """The LDS a ratio needs is host arithmetic of the library; a ratio that does not fit is refused before any launch."""
    import ctypes
    from haloop_amd import _lib
    for ratio in RATIOS + [(1, 1)]:
        w, stride, _, _ = features.resample_taps(*ratio)
        need = _lib.lib().halo_resample_lds_bytes((ctypes.c_int * 6)(ratio[0], ratio[1], w, stride, 0, 0), 1)
        assert 0 < need <= 40 * 1024, (ratio, need)
    assert _lib.lib().halo_resample_lds_bytes((ctypes.c_int * 6)(0, 1, 0, 1, 0, 0), 1) == -1
    with pytest.raises(ValueError, match='LDS'):
        features._resample_tables(((999, 1000),), 'cpu')     # the factor 0.999: 1000 phases of 13 taps
