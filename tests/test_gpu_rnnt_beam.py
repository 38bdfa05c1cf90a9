"""GPU tests of transducer beam search (haloop_amd.transducer.BeamDecoder, recognizer.Transducer.decode(beam_size=...),
csrc/rnnt_beam.hip) against the float64 restatement on the CPU (tests/rnnt_beam_ref.py), in `bf16x3` unless said otherwise.

Tokens, lengths and counts must equal the restatement exactly on every row the fixture does not leave out:
tests/test_rnnt_beam_cpu.py asserts on the CPU that every prune and every final ranking of those rows was decided by a gap of at least
1e-3, ten times the project's fp32-grade tolerance on features.  Scores: rtol 1e-5 / atol 1e-4, the tolerance of
tests/test_gpu_rnnt_decode.py.
"""
import contextlib

import numpy as np
import pytest
import torch

import rnnt_beam_ref as R

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


def check(got, ref, rows, what):
    tokens, lengths, scores, counts = (x.cpu() for x in got)
    assert tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and counts.dtype == torch.int64 and scores.dtype == torch.float32
    assert tokens.shape == ref['tokens'].shape and lengths.shape == ref['lengths'].shape and scores.shape == ref['scores'].shape
    rows = list(rows)
    present = ref['lengths'][rows] >= 0
    err = (scores[rows].double() - ref['scores'][rows])[present].abs().max()
    print(what, 'best lengths', lengths[:, 0].tolist(), 'counts', counts.tolist(), 'max |score error|', float(err))
    assert torch.equal(counts[rows], ref['counts'][rows]), what
    assert torch.equal(lengths[rows], ref['lengths'][rows]), what
    assert torch.equal(tokens[rows], ref['tokens'][rows]), what
    np.testing.assert_allclose(scores[rows].numpy(), ref['scores'][rows].numpy(), rtol=1e-5, atol=1e-4, err_msg=what)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run_fixture(name, W):
    from haloop_amd import transducer
    sd, features, il, capacity, ref = R.fixture(name, W)
    dec = transducer.BeamDecoder(head_of(sd), features.shape[0], capacity, W)
    return dec, features.to(DEV), il.to(DEV), ref


def test_small_ragged_case():
    """N = 3, V = 20 (below one wave), T = 12, a one-frame row."""
    dec, x, il, ref = run_fixture('small', 4)
    assert dec.fused
    check(dec.decode(x, il), ref, R.compared_rows('small', 4), 'small W=4')


@pytest.mark.parametrize('W', [4, 8])
def test_two_row_groups(W):
    """N = 17: a second row group of slots; V = 67: no multiple of 16 or 64; a row of length 0."""
    dec, x, il, ref = run_fixture('rows17', W)
    assert dec.fused
    check(dec.decode(x, il), ref, R.compared_rows('rows17', W), f'rows17 W={W}')


def test_width_one():
    dec, x, il, ref = run_fixture('small', 1)
    assert dec.fused
    check(dec.decode(x, il), ref, R.compared_rows('small', 1), 'small W=1')


def test_wide_vocabulary():
    """V = 1031: several passes per thread and a ragged tail; W = 3 (the row's W V logits fit the step kernel's LDS cache)."""
    dec, x, il, ref = run_fixture('wide', 3)
    assert dec.fused
    check(dec.decode(x, il), ref, R.compared_rows('wide', 3), 'wide W=3')


def test_vocabulary_streamed_from_l2():
    """V = 4099, W = 3: W V is above what the step kernel keeps in LDS, so every selection round recomputes the logits."""
    dec, x, il, ref = run_fixture('stream', 3)
    assert dec.fused
    check(dec.decode(x, il), ref, R.compared_rows('stream', 3), 'stream W=3')


def test_without_pruning_scores_equal_the_training_loss():
    """N = 2, T = 5, V = 4, cap = 2, W = 16: nothing is pruned, so every score is -transducer_loss of the head's own training-path
    operators on f and the teacher-forced g of the returned tokens."""
    from haloop_amd import functional as HF, transducer
    dec, x, il, ref = run_fixture('tiny', 16)
    assert dec.fused
    got = dec.decode(x, il)
    check(got, ref, R.compared_rows('tiny', 16), 'tiny W=16')
    tokens, lengths, scores, counts = got
    head = dec.head
    assert counts.tolist() == [13, 13]
    with torch.no_grad():
        hyp = tokens[:, :13].reshape(26, -1).clamp(min=0)                 # (-1 past a hypothesis's length: never read by the lattice)
        hl = lengths[:, :13].reshape(26)
        rows = torch.arange(2, device=DEV).repeat_interleave(13)
        lm_in = torch.cat([hyp.new_zeros((26, 1)), hyp], dim=1)
        g, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(26))
        f = HF.linear(x[rows].float(), head.classifier.weight, head.classifier.bias)
        losses = transducer.transducer_loss(f, g, hyp, il[rows], hl)
    print('max |score + loss|', float((scores[:, :13].reshape(26) + losses).abs().max()))
    np.testing.assert_allclose(scores[:, :13].reshape(26).cpu().numpy(), -losses.cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_padding_is_never_read():
    dec, x, il, ref = run_fixture('small', 4)
    clean = dec.decode(x, il)
    poisoned = x.clone()
    for n, L in enumerate(il.tolist()):
        poisoned[n, L:] = float('nan')
    assert same(dec.decode(poisoned, il), clean)
    check(clean, ref, R.compared_rows('small', 4), 'small W=4')


def test_fused_path_equals_general_path():
    dec, x, il, ref = run_fixture('small', 4)
    fused = dec.decode(x, il)
    with math_mode('f32'):
        assert not dec.fused
        general = dec.decode(x, il)
    assert dec.fused
    check(general, ref, R.compared_rows('small', 4), 'general path')
    assert torch.equal(fused[0], general[0]) and torch.equal(fused[1], general[1]) and torch.equal(fused[3], general[3])
    np.testing.assert_allclose(fused[2].cpu().numpy(), general[2].cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_state_carries_nothing_over():
    """One BeamDecoder: N = 17, N = 3, N = 17 again -- the first and third results are identical; then a parameter changed in place:
    the next decode follows it (a stale decode image would repeat the old result)."""
    from haloop_amd import transducer
    sd, x17, il17, capacity, ref17 = R.fixture('rows17', 4)
    head = head_of(sd)
    dec = transducer.BeamDecoder(head, 17, capacity, 4)
    x17d, il17d = x17.to(DEV), il17.to(DEV)
    first = dec.decode(x17d, il17d)
    dec.decode(x17d[3:6, :12].contiguous(), torch.tensor([12, 9, 1], device=DEV), capacity=6)
    third = dec.decode(x17d, il17d)
    assert same(first, third)
    check(first, ref17, R.compared_rows('rows17', 4), 'rows17 W=4')
    with torch.no_grad():
        head.lm.rnn.weight_hh_l0.mul_(0.5)
    sd2 = {k: v.detach().cpu().clone() for k, v in head.state_dict().items()}
    ref2 = R.beam_search(sd2, x17, il17, capacity, 4)
    rows = [n for n in range(17) if float(ref2['gaps'][n]) >= R.GAP]    # (the changed weights' own fixture condition)
    assert len(rows) >= 13
    assert not torch.equal(ref2['tokens'], ref17['tokens'])
    check(dec.decode(x17d, il17d), ref2, rows, 'rows17 W=4, weight_hh_l0 halved')


def test_transducer_decode_beam_size():
    from haloop_amd import transducer
    sd, features, il, capacity, ref = R.fixture('small', 4)
    head = head_of(sd)
    x, ild = features.to(DEV), il.to(DEV)
    ct = torch.tensor([capacity - 1, 2, 1])                             # capacity = condtarget_lengths.max() + 1
    assert head.beam_size == 0
    greedy = transducer.GreedyDecoder(head, 3, capacity).decode(x, ild)
    out = head.decode(x, ild, ct)                                       # no keyword: the greedy route, as before
    assert head.last_nbest is None
    assert torch.equal(out[1], greedy[1].cpu()) and torch.equal(out[2], greedy[2]) and torch.equal(out[3], greedy[3])
    for n, hyp in enumerate(out[0].unbind()):
        assert torch.equal(hyp, greedy[0][n, :int(greedy[1][n])])
    out = head.decode(x, ild, ct, beam_size=4)
    assert len(out) == 5
    hypotheses, output_lengths, alignments, scores, sum_entropies = out
    assert sum_entropies is None and alignments == [None] * 3 and hypotheses.is_nested
    assert output_lengths.tolist() == ref['lengths'][:, 0].tolist()
    for n, hyp in enumerate(hypotheses.unbind()):
        assert torch.equal(hyp.cpu(), ref['tokens'][n, 0, :ref['lengths'][n, 0]])
    np.testing.assert_allclose(scores.cpu().numpy(), ref['scores'][:, 0].numpy(), rtol=1e-5, atol=1e-4)
    check(head.last_nbest, ref, R.compared_rows('small', 4), 'last_nbest')
    head.beam_size = 4                                                  # the attribute, without the keyword
    again = head.decode(x, ild, ct)
    assert torch.equal(again[3], scores) and again[1].tolist() == output_lengths.tolist()
