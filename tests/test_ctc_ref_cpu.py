"""tests/ctc_ref.py, the float64 yardstick of tests/test_gpu_ctc_f64.py, held to float64 torch on the CPU: ``ctc`` against
``F.ctc_loss`` with autograd, ``head`` (exact operands) against autograd through F.linear, log_softmax and ctc_loss with the Philox
mask applied, to 1e-9 in every loss and every gradient element, on the GPU test's own cases at their own sizes (none is slow on a CPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_f64_cases as K
import ctc_ref

TOL = 1e-9


@pytest.mark.parametrize('name', list(K.CTC))
def test_ctc_equals_float64_torch(name):
    c = K.CTC[name][0]()
    lp64 = c['lp'].double()
    nll, dlp = ctc_ref.ctc(lp64.numpy(), c['tg'], c['il'], c['tl'])
    x = lp64.clone().requires_grad_(True)
    want = F.ctc_loss(x.permute(1, 0, 2), c['tg'], c['il'], c['tl'], reduction='none')
    fin = torch.isfinite(want)
    want[fin].sum().backward()
    fin = fin.numpy()
    assert np.array_equal(np.isfinite(nll), fin) and (nll[~fin] == np.inf).all()
    assert np.abs(nll[fin] - want.detach().numpy()[fin]).max(initial=0) <= TOL
    ok = np.isfinite(lp64.numpy()) & fin[:, None, None]       # torch gives NaN where lp = -inf; infeasible rows promise nothing
    err = np.abs(dlp - x.grad.numpy())[ok].max()
    print(f'{name}: max|nll| {np.abs(nll[fin]).max(initial=0):.1f}  gradient error {err:.2e}')
    assert err <= TOL
    for n in range(len(nll)):
        assert not dlp[n, int(c['il'][n]):].any(), 'rows at and beyond il are zero'
    if name == 'masked':
        inf = ~np.isfinite(lp64.numpy())
        assert inf.any() and not dlp[inf].any(), 'lp = -inf: occupancy 0, gradient 0'
    if name == 'corners':
        assert list(fin) == [True, True, True, True, False, True]


def test_cases_reach_their_paths():
    """The shapes against the dispatch rule quoted in ctc_f64_cases.py."""
    for name, (_, shape, want) in K.CTC.items():
        assert K.ctc_paths(*shape) == want, name
    T, C, S = K.CTC['wave_lds_edge'][1]
    assert T * C * 4 == K.WAVE_LDS and K.ctc_paths(T + 1, C, S)[0] == 'general'
    assert K.ctc_paths(32, 32, 31)[:2] == ('wave', 'wave') and K.ctc_paths(32, 32, 32)[:2] == ('general', 'general')     # 2S+1 = 63 / 65
    for name, (_, (B, T, H, V, S, p), slices) in K.HEAD.items():
        assert K.train_slices(B, H) == slices, name
        assert (H // slices) % 32 == 0


def _torch_head(c, mask):
    feats = c['feats'].double().requires_grad_(True)
    W = c['W'].double().requires_grad_(True)
    b = c['b'].double().requires_grad_(True)
    x = feats if mask is None else feats * torch.from_numpy(mask).double()
    lp = F.linear(x, W, b).log_softmax(-1)
    flen = torch.from_numpy(ctc_ref.feature_lengths(c['il'].numpy(), feats.shape[1]))
    nll = F.ctc_loss(lp.permute(1, 0, 2), c['tg'], flen, c['tl'], reduction='none')
    loss = (nll / c['tl'].clamp(min=1)).mean()
    fin = torch.isfinite(nll)
    (nll[fin] / c['tl'].clamp(min=1)[fin]).sum().div(len(nll)).backward()
    return dict(flen=flen.numpy(), lp=lp.detach().numpy(), nll=nll.detach().numpy(), loss=loss.item(), dW=W.grad.numpy(), db=b.grad.numpy(),
                dfeats=feats.grad.numpy())


@pytest.mark.parametrize('name', list(K.HEAD))
def test_head_equals_float64_torch(name):
    c = K.HEAD[name][0]()
    assert list(ctc_ref.feature_lengths(c['il'].numpy(), c['feats'].shape[1])) == c['flen']
    mask = K.head_mask(c)
    if mask is not None:
        kept = (mask != 0).mean()
        assert set(np.unique(mask)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(c['p']))} and abs(kept - (1 - c['p'])) < 0.05
    got = ctc_ref.head(c['feats'].numpy(), c['W'].numpy(), c['b'].numpy(), mask, c['il'].numpy(), c['tg'].numpy(), c['tl'].numpy())
    want = _torch_head(c, mask)
    fin = np.isfinite(want['nll'])
    assert np.array_equal(got['flen'], want['flen'])
    assert np.abs(got['lp'] - want['lp']).max() <= TOL
    assert np.array_equal(np.isfinite(got['nll']), fin) and np.abs(got['nll'][fin] - want['nll'][fin]).max() <= TOL
    assert np.abs(got['dfeats'][fin] - want['dfeats'][fin]).max() <= TOL
    if fin.all():
        assert abs(got['loss'] - want['loss']) <= TOL
        for k in ('dW', 'db'):
            assert np.abs(got[k] - want[k]).max() <= TOL, k
    else:
        assert name == 'with_infeasible' and list(fin) == [True, False, True, True] and not np.isfinite(got['loss'])


def test_split_model_is_the_three_term_bf16_product():
    """bf16_round against torch's bfloat16 cast; hi + lo carries 16 bits of the operand; the modelled product misses the exact one by
    the lo*lo term only (<= 2^-16 |a| |b| per term)."""
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(4096, generator=g) * 3, torch.tensor([0.0, 1.0, -1.0, 1.00390625, 1.01171875, 3.3895314e38])])
    assert np.array_equal(ctc_ref.bf16_round(x.numpy()), x.bfloat16().float().numpy())
    hi, lo = ctc_ref._split(x.numpy()[:4096], np.dtype('float64'))
    assert (np.abs(hi + lo - x.numpy()[:4096].astype(np.float64)) <= 2.0 ** -16 * np.abs(x.numpy()[:4096])).all()
    a, b = torch.randn(5, 64, generator=g).numpy(), torch.randn(64, 7, generator=g).numpy()
    exact = a.astype(np.float64) @ b.astype(np.float64)
    model = ctc_ref._product(a, b, 'bf16x3', np.dtype('float64'))
    assert 0 < np.abs(model - exact).max() <= 2.0 ** -16 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)).max()


@pytest.mark.parametrize('split', [None, 'bf16x3'])
def test_greedy_cases_have_no_near_ties(split):
    """The GPU test demands exact alignments and hypotheses of every utterance whose float64 top-two margins all exceed 8 e32(lp), and
    lets at most 2 % of the utterances fall under that: with these seeds none does, so no near-tie filter can hide a broken collapse."""
    for name in K.GREEDY:
        c = K.HEAD[name][0]()
        args = (c['feats'].numpy(), c['W'].numpy(), c['b'].numpy(), None, c['il'].numpy(), c['tg'].numpy(), c['tl'].numpy())
        lp64 = ctc_ref.head(*args, split=split)['lp']
        lp32 = ctc_ref.head(*args, split=split, dtype='float32')['lp']
        e32 = float(np.abs(lp32.astype(np.float64) - lp64).max())
        under = ctc_ref.top_two_margin(lp64) <= 8 * e32
        assert under.mean() <= 0.02, (name, e32)
        ali, scores, hyp, hyp_len = ctc_ref.greedy(lp64)
        a32 = ctc_ref.greedy(lp32)
        assert np.array_equal(ali, a32[0]) and hyp == a32[2]
        if name == 'tile_full':
            assert 0 < hyp_len.min() and hyp_len.max() < ali.shape[1], 'the collapse has repeats or blanks to drop'


def test_greedy_collapse():
    lp = np.log(np.array([[[.1, .6, .3], [.1, .6, .3], [.5, .2, .3], [.1, .6, .3], [.2, .4, .4], [.2, .2, .6], [.6, .2, .2]]]))
    ali, scores, hyp, hyp_len = ctc_ref.greedy(lp)
    assert ali.tolist() == [[1, 1, 0, 1, 1, 2, 0]] and hyp == [[1, 1, 2]] and hyp_len.tolist() == [3]      # ties: the lowest index
    assert np.allclose(scores[0], np.log([.6, .6, .5, .6, .4, .6, .6]))
