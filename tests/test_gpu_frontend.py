"""GPU checks of the batched feature front-end (haloop_amd.features, csrc/frontend.hip) against tests/frontend_ref.py -- the numpy
restatement on oracle/fbank_ref.py and oracle/philox.py -- against the per-utterance fbank.fbank, and against g11_fbank, the vectors of
the Hugging Face transformers port of torchaudio.compliance.kaldi.fbank.

Bounds.  Log-mels: 1e-4 abs, the project's own bound for this front-end (test_gpu_fbank.py: framing in fp32, everything behind it in
float64).  MFCC without CMVN: the same 1e-4 -- a coefficient is a sum of 23 log-mels with orthonormal weights times a lifter <= 12.
CMVN: rtol = atol = 1e-4.  The masks: exact.  Measured on an MI355X: 80 log-mels 9.3e-5 (the fp32 framing on the
filters beside DC, bit-identical to fbank.fbank), 23 log-mels 9.5e-6, MFCC 2.5e-5, MFCC + CMVN 8.0e-6.  The base batch holds utterances of 98 / 1 / 0 / 75 / 2 / 80 frames, and every
sample past an utterance's length is NaN, so a stray read shows."""
import numpy as np
import pytest
import torch

import frontend_ref as R
from haloop_amd import features

pytestmark = pytest.mark.gpu

LENGTHS = [16000, 400, 399, 12345, 560, 13040]
FRAMES = [98, 1, 0, 75, 2, 80]
L = 16000 + 37
PAIRS = [(0, 0), (1, 0), (1, 1), (7, 3), (1234, 5), (2 ** 40 + 17, 9), (2 ** 63 + 5, 2 ** 31 + 1), (99, 10 ** 6)]


def report(name, value):
    print(f'[frontend] {name}: {value:.3e}')


@pytest.fixture(scope='module')
def base():
    """waveforms [6, L] (tone + noise + offset, NaN past the length), lengths, and the references computed once."""
    wav = torch.full((len(LENGTHS), L), float('nan'))
    for n, ln in enumerate(LENGTHS):
        g = torch.Generator().manual_seed(n)
        t = torch.arange(ln) / 16000.0
        wav[n, :ln] = 0.3 * torch.sin(2 * np.pi * (220.0 + 110.0 * n) * t) + 0.05 * torch.randn(ln, generator=g) + 0.01
    lengths = torch.tensor(LENGTHS)
    w = wav.numpy()
    keep = [0, 2, 3, 4, 5]                                   # without the one-frame utterance
    return dict(wav=wav.cuda(), lengths=lengths.cuda(), keep=keep,
                fbank80=R.fbank_batch(w, LENGTHS, 80), fbank23=R.fbank_batch(w, LENGTHS, 23),
                mfcc=R.mfcc_batch(w, LENGTHS, apply_cmvn=False), mfcc_cmvn=R.mfcc_batch(w[keep], [LENGTHS[i] for i in keep]))


def valid_rows(x, frames=FRAMES):
    return np.concatenate([x[n, :m] for n, m in enumerate(frames)])


def padding_rows(x, frames=FRAMES):
    return np.concatenate([x[n, m:].reshape(-1) for n, m in enumerate(frames)])


def test_fbank_batch_matches_restatement_and_per_utterance_fbank(base):
    from haloop_amd import fbank
    got, flen = features.fbank_batch(base['wav'], base['lengths'], num_mel_bins=80)
    assert got.shape == (6, 98, 80) and got.dtype == torch.float32 and flen.dtype == torch.int64
    assert flen.tolist() == FRAMES
    g = got.cpu().numpy()
    ref, ref_len = base['fbank80']
    assert ref_len.tolist() == FRAMES
    assert not np.isnan(g).any()
    assert (padding_rows(g) == 0).all()
    report('fbank80 vs fbank_ref, max abs', np.abs(valid_rows(g) - valid_rows(ref)).max())
    np.testing.assert_allclose(valid_rows(g), valid_rows(ref), rtol=0, atol=1e-4)
    single = [fbank.fbank(base['wav'][n, :ln][None], num_mel_bins=80).cpu().numpy() for n, ln in enumerate(LENGTHS)]
    assert [s.shape[0] for s in single] == FRAMES
    report('fbank80 vs fbank.fbank, max abs', np.abs(valid_rows(g) - np.concatenate(single)).max())
    np.testing.assert_allclose(valid_rows(g), np.concatenate(single), rtol=0, atol=1e-4)


def test_fbank_batch_matches_the_transformers_port_vectors():
    from conftest import load_golden
    g = load_golden('g11_fbank')
    keys = ('tone', 'noise', 'chirp', 'one_frame')
    lens = [g[f'{k}.wav'].shape[0] for k in keys]
    wav = torch.full((4, max(lens) + 3), float('nan'))
    for n, k in enumerate(keys):
        wav[n, :lens[n]] = torch.from_numpy(g[f'{k}.wav'])
    got, flen = features.fbank_batch(wav.cuda(), torch.tensor(lens).cuda(), num_mel_bins=80)
    got = got.cpu().numpy().astype(np.float64)
    for n, k in enumerate(keys):
        ref = g[f'{k}.fbank'].astype(np.float64)
        assert int(flen[n]) == ref.shape[0]
        x = got[n, :ref.shape[0]]
        assert (got[n, ref.shape[0]:] == 0).all()
        # the two criteria of test_gpu_fbank.py::test_fbank_matches_the_transformers_port_vectors
        peak = np.exp(ref).max(axis=1, keepdims=True)
        report(f'g11 {k} energies / peak', (np.abs(np.exp(x) - np.exp(ref)) / peak).max())
        assert (np.abs(np.exp(x) - np.exp(ref)) / peak).max() <= 5e-6, k
        near = ref >= ref.max(axis=1, keepdims=True) - 12.0
        report(f'g11 {k} logs within 12 nepers', np.abs(x - ref)[near].max())
        assert np.abs(x - ref)[near].max() <= 1e-4, k


def test_fbank23_and_mfcc_match_restatement(base):
    got, flen = features.fbank_batch(base['wav'], base['lengths'], num_mel_bins=23)
    assert got.shape == (6, 98, 23) and flen.tolist() == FRAMES
    g = got.cpu().numpy()
    report('fbank23 vs fbank_ref, max abs', np.abs(valid_rows(g) - valid_rows(base['fbank23'][0])).max())
    np.testing.assert_allclose(valid_rows(g), valid_rows(base['fbank23'][0]), rtol=0, atol=1e-4)
    assert (padding_rows(g) == 0).all()
    got, flen = features.mfcc_batch(base['wav'], base['lengths'], cmvn=False)
    assert got.shape == (6, 98, 13) and got.dtype == torch.float32 and flen.tolist() == FRAMES
    g = got.cpu().numpy()
    assert not np.isnan(g).any() and (padding_rows(g) == 0).all()
    report('mfcc vs frontend_ref, max abs', np.abs(valid_rows(g) - valid_rows(base['mfcc'][0])).max())
    np.testing.assert_allclose(valid_rows(g), valid_rows(base['mfcc'][0]), rtol=0, atol=1e-4)
    # the single-utterance form under torchaudio's signature is a batch of one
    one = features.mfcc(base['wav'][3, :LENGTHS[3]][None])
    assert one.shape == (75, 13) and torch.equal(one, got[3, :75])


def test_mfcc_cmvn(base):
    keep = base['keep']
    frames = [FRAMES[i] for i in keep]
    got, flen = features.mfcc_batch(base['wav'][keep], base['lengths'][keep])
    assert got.shape == (5, 98, 13) and flen.tolist() == frames
    g = got.cpu().numpy()
    ref = base['mfcc_cmvn'][0]
    assert (padding_rows(g, frames) == 0).all()
    report('mfcc + cmvn vs frontend_ref, max abs', np.abs(valid_rows(g, frames) - valid_rows(ref, frames)).max())
    np.testing.assert_allclose(valid_rows(g, frames), valid_rows(ref, frames), rtol=1e-4, atol=1e-4)
    # the base batch holds the one-frame utterance: NaN in exactly its valid row (0 / 0, as frames.std(dim=0) of one frame)
    full = features.mfcc_batch(base['wav'], base['lengths'])[0].cpu().numpy()
    want = np.zeros((6, 98, 13), dtype=bool)
    want[1, 0] = True
    assert np.array_equal(np.isnan(full), want)
    assert np.array_equal(full[keep], g)


@pytest.mark.parametrize('kind', ['fbank', 'mfcc'])
def test_spec_mask_is_the_restatements_exactly(base, kind):
    x, flen = features.fbank_batch(base['wav'], base['lengths']) if kind == 'fbank' else features.mfcc_batch(base['wav'], base['lengths'], cmvn=False)
    x = x + 100.0                                           # no element of a valid row is 0 before the mask
    x[:, :, :] = torch.where(torch.arange(98, device='cuda')[None, :, None] < flen[:, None, None], x, torch.zeros_like(x))
    before = x.cpu().numpy()
    for seed, step in PAIRS:
        y = x.clone()
        assert features.spec_mask_(y, flen, seed=seed, step=step) is y
        got = y.cpu().numpy()
        want = R.spec_mask(before, FRAMES, seed, step)
        valid = np.arange(98)[None, :, None] < np.array(FRAMES)[:, None, None]
        zeroed = (got == 0) & valid
        assert np.array_equal(zeroed, want)                                                  # the two boolean masks, exactly
        assert np.array_equal(got[~want].view(np.uint32), before[~want].view(np.uint32))     # everything else: the same bits
        assert not want[2].any() and not want[1, 1:].any()                                   # 0 frames: nothing; 1 frame: its columns only
        assert want[1, 0].sum() < 80 // 6 + 1 and want[4, :2].all(axis=1).sum() <= 1         # 2 frames: at most one whole frame
    a = R.spec_mask(before, FRAMES, 7, 3)
    assert not np.array_equal(a, R.spec_mask(before, FRAMES, 7, 4))
    # explicit parameters, above the axis sizes: clamped to them
    y = x.clone()
    features.spec_mask_(y, flen, seed=5, step=1, freq_param=1000, time_param=1000)
    assert np.array_equal((y.cpu().numpy() == 0) & (before != 0), R.spec_mask(before, FRAMES, 5, 1, freq_param=1000, time_param=1000))


def test_launches_are_bit_reproducible(base):
    for fn in (lambda: features.fbank_batch(base['wav'], base['lengths'])[0], lambda: features.mfcc_batch(base['wav'], base['lengths'], cmvn=False)[0],
               lambda: features.mfcc_batch(base['wav'], base['lengths'])[0],
               lambda: features.spec_mask_(features.fbank_batch(base['wav'], base['lengths'])[0], torch.tensor(FRAMES).cuda(), seed=3, step=2)):
        a, b = fn().cpu().numpy(), fn().cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_front_end_module(base):
    from haloop_amd import _lib, rnn
    wav, lengths = base['wav'], base['lengths']
    plain, flen = features.FrontEnd('fbank')(wav, lengths)
    masked = features.FrontEnd('mask:fbank')
    assert masked.training and not list(masked.parameters())
    got, glen = masked.eval()(wav, lengths, seed=11, step=4)
    assert torch.equal(got, plain) and torch.equal(glen, flen)
    got, _ = masked.train()(wav, lengths, seed=11, step=4)
    want = features.spec_mask_(features.fbank_batch(wav, lengths)[0], flen, seed=11, step=4)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    for spec, dim in (('mask:fbank', 80), ('mfcc', 13)):
        front = features.FrontEnd(spec)
        keep = base['keep']                                  # (CMVN of one frame is NaN by definition: leave that utterance out)
        x, xl = front(wav[keep], lengths[keep], seed=1)
        assert x.shape == (5, 98, dim)
        enc = rnn.Encoder(input_dim=dim, subsample_dim=16, hidden_dim=32, num_layers=1).cuda().eval()
        out, out_len, _ = enc(x, xl)
        assert out.shape[0] == 5 and out.shape[1] == int(enc.subsampled_lengths(torch.tensor([98]))[0]) and out.shape[2] == 32
        assert torch.equal(out_len.cpu(), enc.subsampled_lengths(torch.tensor([FRAMES[i] for i in keep])))
        assert torch.isfinite(out).all()
    with pytest.raises(ValueError, match='mask:mfcc'):
        features.FrontEnd('speed:fbank')
    with pytest.raises(_lib.HaloError):
        features.fbank_batch(wav.cpu(), lengths.cpu())
    with pytest.raises(_lib.HaloError):
        features.FrontEnd('mfcc')(wav.cpu(), lengths)
    with pytest.raises(NotImplementedError):
        features.fbank_batch(wav, lengths, dither=1.0)
    with pytest.raises(NotImplementedError):
        features.mfcc_batch(wav, lengths, use_energy=True)


def test_front_end_replays_from_a_captured_graph(base):
    """No host read on the path: 'mask:fbank' in training mode captures into a graph (two sequential launches) and replays to the eager
    result, also on other samples and lengths in the same buffers."""
    front = features.FrontEnd('mask:fbank').train()
    wav, lengths = base['wav'].clone(), base['lengths'].clone()
    front(wav, lengths, seed=21, step=2)                      # tables built before the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out, out_len = front(wav, lengths, seed=21, step=2)
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]):
        wav.copy_(base['wav'][order]); lengths.copy_(base['lengths'][order])
        graph.replay()
        torch.cuda.synchronize()
        want, want_len = front(wav, lengths, seed=21, step=2)
        assert torch.equal(out, want) and torch.equal(out_len, want_len) and out_len.tolist() == [FRAMES[i] for i in order]
