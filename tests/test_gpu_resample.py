"""GPU checks of the waveform stage (haloop_amd.features.resample_batch / speed_perturb / FrontEnd('...:speed'), csrc/resample.hip)
against tests/resample_ref.py, the float64 restatement of torchaudio.functional.resample's defaults (parity with torchaudio itself is
unpinned: it is not installed where this project is built).

Bound.  Derived, not measured: the kernel's output is an fp32 dot product of the same fp32 taps and fp32 samples the restatement sums in
float64, so for any summation order |got - ref| <= n u / (1 - n u) * max_p sum_k |taps[p, k]| * max |x| with u = 2^-24 and n one more
than the largest count of non-zero taps in a phase (resample_ref.tolerance; |x| <= 0.5 here).  It comes to 7.7e-7 .. 7.8e-7 for the
speed ratios and 8.7e-7 / 1.13e-6 / 1.65e-6 / 1.72e-6 for 22050 / 32000 / 44100 / 48000 Hz.  Lengths, padding, draws and every
"bit-identical" below are exact.  The measured maxima are printed and recorded in DESIGN.md 3.3u.

The batch: 8 rows of padded width 3037 -- 3000 samples cross several 1024-sample tiles, rows of 0 / 1 / 6 samples sit below the filter's
width, 950 and 951 hit the ceil of the 19/20 ratio exactly, 1323 = 3 * 441 that of the 441 ratios -- with NaN behind every length, so a
stray read shows."""
import math

import numpy as np
import pytest
import torch

import resample_ref as R
from haloop_amd import features

pytestmark = pytest.mark.gpu

LENGTHS = [3000, 0, 1, 6, 19 * 50, 19 * 50 + 1, 441 * 3, 2999]
L = 3000 + 37
RATES = [15200, 15680, 16320, 16800, 22050, 32000, 44100, 48000]
PAIRS = [(0, 0), (1, 0), (1, 1), (7, 3), (1234, 5), (2 ** 40 + 17, 9), (2 ** 63 + 5, 2 ** 31 + 1), (99, 10 ** 6)]   # test_gpu_frontend.py's
FACTOR_RATES = [int(f * 16000) for f in R.FACTORS]


def report(name, value):
    print(f'[resample] {name}: {value:.3e}')


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def make_batch(lengths, width, seed=0):
    """Tone + uniform noise + offset, |x| <= 0.41, NaN past the length."""
    wav = torch.full((len(lengths), width), float('nan'))
    for n, ln in enumerate(lengths):
        g = torch.Generator().manual_seed(seed + n)
        t = torch.arange(ln) / 16000.0
        wav[n, :ln] = 0.3 * torch.sin(2 * np.pi * (220.0 + 110.0 * n) * t) + 0.1 * (2.0 * torch.rand(ln, generator=g) - 1.0) + 0.01
    return wav


@pytest.fixture(scope='module')
def base():
    wav = make_batch(LENGTHS, L)
    assert float(wav[~wav.isnan()].abs().max()) <= 0.5
    w = wav.numpy().astype(np.float64)
    refs = {rate: R.resample_batch(w, LENGTHS, *R.ratio(rate, 16000)) for rate in RATES}
    return dict(wav=wav.cuda(), lengths=torch.tensor(LENGTHS).cuda(), refs=refs, single={})


def own_ratio(base, n, index):
    """Row n resampled alone at the ratio of factor `index` (cached): what a row of speed_perturb must equal bit for bit."""
    key = (n, index)
    if key not in base['single']:
        base['single'][key] = features.resample_batch(base['wav'][n:n + 1], base['lengths'][n:n + 1], FACTOR_RATES[index])
    return base['single'][key]


@pytest.mark.parametrize('rate', RATES)
def test_resample_batch_matches_the_restatement(base, rate):
    orig, new = R.ratio(rate, 16000)
    got, got_len = features.resample_batch(base['wav'], base['lengths'], rate)
    ref, ref_len = base['refs'][rate]
    assert got.shape == (8, math.ceil(L * new / orig)) == ref.shape and got.dtype == torch.float32 and got_len.dtype == torch.int64
    assert got_len.tolist() == ref_len.tolist() == [-(-new * n // orig) for n in LENGTHS]
    g = got.cpu().numpy()
    assert not np.isnan(g).any()
    atol = R.tolerance(orig, new, 0.5)
    worst = 0.0
    for n, m in enumerate(ref_len):
        assert (g[n, m:] == 0).all()                         # padding: exact zeros
        if m:
            worst = max(worst, float(np.abs(g[n, :m] - ref[n, :m]).max()))
    report(f'{rate} -> 16000 vs float64 restatement, max abs (bound {atol:.3e})', worst)
    assert worst <= atol


def test_rows_are_independent_and_runs_are_bit_identical(base):
    for rate in (15200, 44100):
        a, a_len = features.resample_batch(base['wav'], base['lengths'], rate)
        b, b_len = features.resample_batch(base['wav'], base['lengths'], rate)
        assert np.array_equal(bits(a), bits(b)) and torch.equal(a_len, b_len)
        one, one_len = features.resample_batch(base['wav'][:1], base['lengths'][:1], rate)
        assert np.array_equal(bits(one[0]), bits(a[0])) and int(one_len[0]) == int(a_len[0])
        last, _ = features.resample_batch(base['wav'][[7, 3, 0]], base['lengths'][[7, 3, 0]], rate)
        assert np.array_equal(bits(last), bits(a[[7, 3, 0]]))
    same, same_len = features.resample_batch(base['wav'], base['lengths'], 16000)          # equal rates: a copy
    assert same.data_ptr() != base['wav'].data_ptr() and same_len.tolist() == LENGTHS
    for n, ln in enumerate(LENGTHS):
        assert np.array_equal(bits(same[n, :ln]), bits(base['wav'][n, :ln])) and (same[n, ln:] == 0).all()


def test_new_times_len_past_32_bits():
    """Five minutes of 22050 Hz audio: 320 * len is past 2^31, so the output length and a tile's first input sample need the 64-bit
    arithmetic.  The last 100 blocks of 441 samples are compared against the restatement of that segment alone (it starts on a multiple of
    orig, so only its first few outputs see the missing left context: one block of 320 is skipped)."""
    orig, new = 441, 320
    n = orig * 15300 + 17
    assert new * n > 2 ** 31
    wav = torch.rand(1, n + 5, device='cuda') - 0.5
    wav[0, n:] = float('nan')
    out, out_len = features.resample_batch(wav, torch.tensor([n]).cuda(), 22050)
    m = -(-new * n // orig)
    assert out.shape == (1, -(-new * (n + 5) // orig)) and out_len.tolist() == [m]
    q = 15200
    ref = R.resample(wav[0, q * orig:n].cpu().numpy().astype(np.float64), orig, new)
    got = out[0, q * new:].cpu().numpy()
    assert ref.shape[0] == m - q * new and (got[ref.shape[0]:] == 0).all() and not np.isnan(got).any()
    worst = float(np.abs(got[new:ref.shape[0]] - ref[new:]).max())
    report('22050 -> 16000 at 6.7 M samples, last 100 blocks, max abs', worst)
    assert worst <= R.tolerance(orig, new, 0.5)
    assert torch.isfinite(out).all() and float(out[0, :m].abs().max()) > 0.1


def test_speed_perturb_draws_and_rows(base):
    wav, lengths = base['wav'], base['lengths']
    L_out = (20 * L + 18) // 19
    for seed, step in PAIRS:
        out, out_len, indices = features.speed_perturb(wav, lengths, seed=seed, step=step)
        assert out.shape == (8, L_out) and out.dtype == torch.float32 and out_len.dtype == torch.int64 and indices.dtype == torch.int32
        want = [R.speed_index(n, seed, step) for n in range(8)]
        assert indices.tolist() == want
        assert not torch.isnan(out).any()
        for n, idx in enumerate(want):
            one, one_len = own_ratio(base, n, idx)
            assert int(out_len[n]) == int(one_len[0]) == R.out_length(LENGTHS[n], *R.speed_ratio(R.FACTORS[idx]))
            w = one.shape[1]
            assert np.array_equal(bits(out[n, :w]), bits(one[0])) and (out[n, w:] == 0).all()
            if R.FACTORS[idx] == 1.0:
                assert int(out_len[n]) == LENGTHS[n] and np.array_equal(bits(out[n, :LENGTHS[n]]), bits(wav[n, :LENGTHS[n]]))
    a = features.speed_perturb(wav, lengths, seed=7, step=3)
    b = features.speed_perturb(wav, lengths, seed=7, step=3)
    assert np.array_equal(bits(a[0]), bits(b[0])) and torch.equal(a[2], b[2])
    # the caller's own indices override the draw
    given = torch.tensor([4, 3, 2, 1, 0, 0, 2, 1], dtype=torch.int32).cuda()
    out, out_len, indices = features.speed_perturb(wav, lengths, seed=7, step=3, indices=given)
    assert torch.equal(indices, given)
    for n, idx in enumerate(given.tolist()):
        one, one_len = own_ratio(base, n, idx)
        assert int(out_len[n]) == int(one_len[0]) and np.array_equal(bits(out[n, :one.shape[1]]), bits(one[0]))
    # 64 short rows: the draw is per row
    short = make_batch([40 + n for n in range(64)], 128, seed=100).cuda()
    short_len = torch.tensor([40 + n for n in range(64)]).cuda()
    for seed, step in PAIRS:
        out, out_len, indices = features.speed_perturb(short, short_len, seed=seed, step=step)
        want = [R.speed_index(n, seed, step) for n in range(64)]
        assert indices.tolist() == want and len(set(want)) >= 3
        assert out_len.tolist() == [R.out_length(40 + n, *R.speed_ratio(R.FACTORS[i])) for n, i in enumerate(want)]
        assert not torch.isnan(out).any()


def test_front_end_over_speed(base):
    from haloop_amd import _lib, rnn
    wav, lengths = base['wav'], base['lengths']
    plain, flen = features.FrontEnd('fbank')(wav, lengths)
    front = features.FrontEnd('fbank:speed')
    assert front.training and not list(front.parameters())
    got, glen = front.eval()(wav, lengths, seed=11, step=4)
    assert np.array_equal(bits(got), bits(plain)) and torch.equal(glen, flen)
    full = features.FrontEnd('mask:fbank:speed')
    got, glen = full.eval()(wav, lengths, seed=11, step=4)
    assert np.array_equal(bits(got), bits(plain)) and torch.equal(glen, flen)
    got, glen = full.train()(wav, lengths, seed=11, step=4)
    x, xl = features.fbank_batch(*features.speed_perturb(wav, lengths, seed=11, step=4)[:2])
    want = features.spec_mask_(x, xl, seed=11, step=4)
    assert got.shape == (8, 1 + ((20 * L + 18) // 19 - 400) // 160, 80)
    assert np.array_equal(bits(got), bits(want)) and torch.equal(glen, xl)
    assert [R.speed_index(n, 11, 4) for n in range(8)] != [2] * 8 and glen.tolist() != flen.tolist()       # the stage did something
    enc = rnn.Encoder(80, 16, 32, num_layers=1).cuda().eval()
    out, out_len, _ = enc(got, glen)
    assert out.shape[0] == 8 and out.shape[2] == 32 and torch.isfinite(out).all()
    assert torch.equal(out_len.cpu(), enc.subsampled_lengths(glen.cpu()))
    for spec, dim in (('mfcc:speed', 13), ('mask:mfcc:speed', 13)):
        y, yl = features.FrontEnd(spec)(wav[[0, 6, 7]], lengths[[0, 6, 7]], seed=5, step=1)
        assert y.shape[0] == 3 and y.shape[2] == dim and torch.isfinite(y).all() and (yl > 1).all()
    with pytest.raises(ValueError, match='mask:mfcc'):
        features.FrontEnd('speed:fbank')
    with pytest.raises(_lib.HaloError):
        features.resample_batch(wav.cpu(), lengths.cpu(), 48000)
    with pytest.raises(_lib.HaloError):
        features.speed_perturb(wav.cpu(), lengths, seed=1)
    with pytest.raises(_lib.HaloError):
        full(wav.cpu(), lengths.cpu())
    with pytest.raises(ValueError):
        features.speed_perturb(wav, lengths, seed=1, factors=[0.9 + 0.02 * i for i in range(9)])
    with pytest.raises(ValueError, match='LDS'):
        features.speed_perturb(wav, lengths, seed=1, factors=(0.999, 1.0))
    with pytest.raises(NotImplementedError):
        features.resample_batch(wav, lengths, 48000, resampling_method='sinc_interp_kaiser')
    with pytest.raises(NotImplementedError):
        features.resample_batch(wav, lengths, 48000, lowpass_filter_width=16)


def test_front_end_over_speed_replays_from_a_captured_graph(base):
    """No host read on the path: 'mask:fbank:speed' in training mode captures into a graph (three sequential launches, no parallel
    branches) and replays to the eager result, also on other samples and lengths in the same buffers.  ``step`` is a launch argument,
    so the replay is compared against eager at the captured step."""
    front = features.FrontEnd('mask:fbank:speed').train()
    wav, lengths = base['wav'].clone(), base['lengths'].clone()
    front(wav, lengths, seed=21, step=2)                      # tables built before the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out, out_len = front(wav, lengths, seed=21, step=2)
    seen = []
    for order in ([0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1, 0], [0, 0, 7, 7, 6, 6, 4, 5]):
        wav.copy_(base['wav'][order]); lengths.copy_(base['lengths'][order])
        graph.replay()
        torch.cuda.synchronize()
        want, want_len = front(wav, lengths, seed=21, step=2)
        assert np.array_equal(bits(out), bits(want)) and torch.equal(out_len, want_len)
        seen.append(out_len.tolist())
    assert seen[0] != seen[1]
