"""CPU checks of tests/frontend_ref.py, the restatement the GPU front-end tests compare against, and of the host-side tables of
haloop_amd.features (kaldi's DCT and lifter, the packed mel filters, the stream id): what can be verified of them without vectors."""
import numpy as np

import frontend_ref as R
from haloop_amd import features


def _wave(n, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * g.standard_normal(n) + 0.01).astype(np.float32)


def test_dct_rows_are_orthonormal_and_the_tables_agree():
    full = R.dct_matrix(23, 23)
    np.testing.assert_allclose(full @ full.T, np.eye(23), atol=1e-13)
    np.testing.assert_allclose(R.dct_matrix(13, 23), full[:13], atol=0)
    assert R.lifter()[0] == 1.0 and np.all(R.lifter()[1:] > 1.0)
    np.testing.assert_allclose(features.dct_lifter(13, 23, 22.0).numpy(), R.dct_matrix() * R.lifter()[:, None], atol=1e-15)


def test_c0_is_the_scaled_sum_of_the_log_mels():
    from oracle import fbank_ref
    wav = _wave(4000, 0)
    mel = fbank_ref.fbank(wav, num_mel_bins=23).astype(np.float64)
    got = R.mfcc(wav)
    assert got.shape == (R.n_frames(4000), 13) and got.dtype == np.float32
    np.testing.assert_allclose(got[:, 0], np.sqrt(1.0 / 23.0) * mel.sum(axis=1), rtol=1e-6)


def test_cmvn_gives_zero_mean_and_unit_unbiased_std():
    x = R.mfcc(_wave(8000, 1))
    y = R.cmvn(x).astype(np.float64)
    np.testing.assert_allclose(y.mean(axis=0), 0.0, atol=1e-6)
    np.testing.assert_allclose(y.std(axis=0, ddof=1), 1.0, atol=1e-6)
    assert np.isnan(R.cmvn(x[:1])).all() and R.cmvn(x[:0]).shape == (0, 13)


def test_packed_filters_are_the_dense_matrix():
    from oracle import fbank_ref
    for bins in (80, 23):
        ranges, weights = features.mel_filters(bins, 512, 16000.0, 20.0, 0.0)
        ranges, weights = ranges.numpy(), weights.numpy()
        dense = np.zeros((bins, 257))
        for b in range(bins):
            lo, count, off = ranges[:, b]
            assert 0 <= lo and lo + count <= 256 and off + count <= weights.size
            dense[b, lo:lo + count] = weights[off:off + count]
        np.testing.assert_allclose(dense, fbank_ref.mel_banks(bins, 512, 16000.0), atol=1e-15)


def test_spec_mask_properties_over_1000_seeds():
    from haloop_amd import _lib
    assert R.SPECMASK_STREAM == _lib.HALO_SPECMASK_STREAM
    assert len({_lib.HALO_SPECMASK_STREAM, _lib.HALO_MLM_STREAM, _lib.HALO_GPT_SAMPLE_STREAM}) == 3 and _lib.HALO_SPECMASK_STREAM > 4096 + 4096
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'halo.h')).read()
    assert f'#define HALO_SPECMASK_STREAM 0x{_lib.HALO_SPECMASK_STREAM:08X}u' in text
    lengths = np.array([98, 1, 0, 75, 2, 80])
    feats = np.ones((6, 98, 80), dtype=np.float32)
    widths = set()
    for seed in range(1000):
        for n, m in enumerate(lengths):
            (cs, cw), (ts, tw) = R.spec_mask_bands(n, 80, int(m), seed, 3)
            assert 0 <= cw < 13 and 0 <= cs and cs + cw <= 80
            assert 0 <= tw < max(min(7, m), 1) and 0 <= ts and ts + tw <= m
            widths.add((cw, tw))
        if seed < 50:
            zero = R.spec_mask(feats, lengths, seed, 3)
            for n, m in enumerate(lengths):
                assert not zero[n, m:].any()                                   # frames past m_n untouched
            (cs, cw), (_, tw) = R.spec_mask_bands(1, 80, 1, seed, 3)
            assert tw == 0 and zero[1, 0].sum() == cw and zero[1, 0, cs:cs + cw].all()   # one frame: P = 1, int(u) = 0: columns only
            assert not zero[2].any()                                           # no frame: nothing
            assert np.array_equal(zero, R.spec_mask(feats, lengths, seed, 3))  # a function of (seed, step)
            assert not np.array_equal(zero, R.spec_mask(feats, lengths, seed, 4))
            assert not np.array_equal(zero, R.spec_mask(feats, lengths, seed + 1000, 3))
    assert {w for w, _ in widths} == set(range(13)) and {t for _, t in widths} == set(range(7))
    # MFCC width: D // 6 = 2 columns at most, and an explicit parameter above the axis is clamped to it
    for seed in range(200):
        (cs, cw), (ts, tw) = R.spec_mask_bands(0, 13, 5, seed, 0, freq_param=100, time_param=100)
        assert cw < 13 and cs + cw <= 13 and tw < 5 and ts + tw <= 5
        assert R.spec_mask_bands(0, 13, 98, seed, 0)[0][1] < 2
