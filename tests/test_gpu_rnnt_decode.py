"""GPU tests of greedy transducer decoding (haloop_amd.transducer.GreedyDecoder, recognizer.Transducer.decode, csrc/rnnt_decode.hip)
against the float64 restatement on the CPU (tests/rnnt_greedy_ref.py), in `bf16x3` unless said otherwise.

Tokens, lengths, frames and the truncated flags must equal the restatement exactly: tests/test_rnnt_greedy_cpu.py asserts on the CPU
that every free argmax of the fixtures has a gap of at least 1e-3, ten times the project's fp32-grade tolerance on features.  Scores:
rtol 1e-5 / atol 1e-4, the lattice tests' tolerance for sums of log-probabilities (tests/test_gpu_lattice.py).
"""
import contextlib

import numpy as np
import pytest
import torch

import rnnt_greedy_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@contextlib.contextmanager
def math_mode(mode):
    from haloop_amd import _lib
    _lib.lib()
    prev = _lib.get_math_mode()
    _lib.set_math_mode(mode)
    try:
        yield
    finally:
        _lib.set_math_mode(prev)


@pytest.fixture(autouse=True)
def bf16x3():
    with math_mode('bf16x3'):
        yield


def head_of(sd):
    from haloop_amd import recognizer
    head = recognizer.Transducer(sd['classifier.weight'].shape[1], sd['classifier.weight'].shape[0]).eval()
    head.load_state_dict(sd)
    return head.to(DEV)


def check(got, ref, what):
    tokens, lengths, frames, scores, truncated = (x.cpu() for x in got)
    print(what, 'lengths', lengths.tolist(), 'max |score error|', float((scores.double() - ref['scores']).abs().max()))
    assert tokens.dtype == torch.int64 and frames.dtype == torch.int64 and lengths.dtype == torch.int64
    assert scores.dtype == torch.float32 and truncated.dtype == torch.bool
    assert torch.equal(lengths, ref['lengths']), what
    assert torch.equal(tokens, ref['tokens']), what
    assert torch.equal(frames, ref['frames']), what
    assert torch.equal(truncated, ref['truncated']), what
    np.testing.assert_allclose(scores.numpy(), ref['scores'].numpy(), rtol=1e-5, atol=1e-4, err_msg=what)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run_fixture(name):
    from haloop_amd import transducer
    sd, features, il, capacity, ref = R.fixture(name)
    dec = transducer.GreedyDecoder(head_of(sd), features.shape[0], capacity, R.MAX_SYMBOLS)
    return dec, features.to(DEV), il.to(DEV), ref


def test_small_ragged_case():
    """N = 3 (one partial row group), V = 20 (below one wave), T = 12 (no multiple of the waves' stride), a one-frame row."""
    dec, x, il, ref = run_fixture('small')
    assert dec.fused
    check(dec.decode(x, il), ref, 'small')


@pytest.mark.parametrize('name', ['rows17', 'rows17_long'])
def test_two_row_groups(name):
    """N = 17: a second row group holding a single row; V = 67: no multiple of 16 or 64; a row of length 0.  rows17_long: capacity
    2 T, so no row truncates and every row ends by its length."""
    dec, x, il, ref = run_fixture(name)
    assert dec.fused
    check(dec.decode(x, il), ref, name)


def test_padding_is_never_read():
    dec, x, il, ref = run_fixture('small')
    clean = dec.decode(x, il)
    poisoned = x.clone()
    for n, L in enumerate(il.tolist()):
        poisoned[n, L:] = float('nan')
    assert same(dec.decode(poisoned, il), clean)
    check(clean, ref, 'small')


def test_fused_path_equals_general_path():
    dec, x, il, ref = run_fixture('small')
    fused = dec.decode(x, il)
    with math_mode('f32'):
        assert not dec.fused
        general = dec.decode(x, il)
    assert dec.fused
    check(general, ref, 'general path')
    assert torch.equal(fused[0], general[0]) and torch.equal(fused[2], general[2])
    np.testing.assert_allclose(fused[3].cpu().numpy(), general[3].cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_state_carries_nothing_over():
    """One GreedyDecoder: N = 17, N = 3, N = 17 again -- the first and third results are identical; then a parameter changed in place:
    the next decode equals the restatement on the new weights (a stale decode image fails it)."""
    from haloop_amd import transducer
    sd, x17, il17, capacity, ref17 = R.fixture('rows17')
    _, x3, il3, _, _ = R.fixture('small')
    head = head_of(sd)
    dec = transducer.GreedyDecoder(head, 17, capacity, R.MAX_SYMBOLS)
    x17d, il17d = x17.to(DEV), il17.to(DEV)
    first = dec.decode(x17d, il17d)
    feat = x17.shape[2]
    x3w = torch.zeros(3, x3.shape[1], feat)
    x3w[:, :, :x3.shape[2]] = x3                                       # (the small case's frames, widened to this head's features)
    dec.decode(x3w.to(DEV), il3.to(DEV))
    third = dec.decode(x17d, il17d)
    assert same(first, third)
    check(first, ref17, 'rows17')
    with torch.no_grad():
        head.lm.rnn.weight_hh_l0.mul_(0.5)
    sd2 = {k: v.detach().cpu().clone() for k, v in head.state_dict().items()}
    ref2 = R.greedy(sd2, x17, il17, capacity, R.MAX_SYMBOLS)
    assert ref2['gap'] >= 1e-3, ref2['gap']                             # (the changed weights' own fixture condition)
    assert not torch.equal(ref2['tokens'], ref17['tokens'])
    check(dec.decode(x17d, il17d), ref2, 'rows17, weight_hh_l0 halved')


def test_decodable_protocol():
    sd, features, il, capacity, ref = R.fixture('small')
    head = head_of(sd)
    x, ild = features.to(DEV), il.to(DEV)
    ct = torch.tensor([capacity - 1, 2, 1])                             # capacity = condtarget_lengths.max() + 1
    ref10 = R.greedy(sd, features, il, capacity, 10)                    # the protocol call's cap of 10 symbols per frame
    assert ref10['gap'] >= 1e-3
    out = head.decode(x, ild, ct)
    assert len(out) == 5
    hypotheses, output_lengths, frames, scores, sum_entropies = out
    assert sum_entropies is None
    assert hypotheses.is_nested
    assert output_lengths.tolist() == ref10['lengths'].tolist()
    for n, hyp in enumerate(hypotheses.unbind()):
        assert torch.equal(hyp.cpu(), ref10['tokens'][n, :ref10['lengths'][n]])
    assert torch.equal(frames.cpu(), ref10['frames'])
    np.testing.assert_allclose(scores.cpu().numpy(), ref10['scores'].numpy(), rtol=1e-5, atol=1e-4)
    with pytest.raises(NotImplementedError):
        head.decode(x, ild)
    with pytest.raises(NotImplementedError):
        head.decode(x, ild, ct, prompt=torch.zeros(3, 1, dtype=torch.long))
    head.train()
    with pytest.raises(NotImplementedError):
        head.decode(x, ild, ct)
    head.eval()


def test_score_is_below_the_lattice_total_on_the_device():
    """The module's own training-path operators: for the rows of the 17-row fixture that are not truncated,
    -transducer_forward_score(log_softmax(joint of the head's lm.forward_batch_first on [0 | hyp]), hyp) >= score - 1e-4."""
    from haloop_amd import functional as HF, transducer
    dec, x, il, ref = run_fixture('rows17')
    head = dec.head
    tokens, lengths, frames, scores, truncated = dec.decode(x, il)
    keep = (~truncated & (il > 0)).nonzero().view(-1)
    assert keep.numel() >= 8
    with torch.no_grad():
        hyp = tokens[keep].clamp(min=0)                                  # (-1 past a row's length: never read by the lattice)
        U = int(lengths[keep].max())
        hyp = hyp[:, :max(U, 1)]
        lm_in = torch.cat([hyp.new_zeros((len(keep), 1)), hyp], dim=1)
        lm_out, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(len(keep)))
        f = HF.linear(x[keep].float(), head.classifier.weight, head.classifier.bias)
        joint = HF.log_softmax((f[:, :, None, :] + lm_out[:, None, :, :]).contiguous())
        losses = transducer.transducer_forward_score(joint, hyp, il[keep], lengths[keep])
    print('lattice totals', (-losses).tolist(), 'scores', scores[keep].tolist())
    assert bool((-losses >= scores[keep] - 1e-4).all())
