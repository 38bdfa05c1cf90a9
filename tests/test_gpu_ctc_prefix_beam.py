"""GPU tests of the CTC prefix beam search (haloop_amd.ctc.ctc_prefix_beam_search, recognizer.TemporalClassifier.decode(beam_size=...)
and mwer_forward, csrc/ctc_prefix_beam.hip) against the float64 restatement on the CPU (tests/ctc_prefix_beam_ref.py), in fp32.

Tokens, lengths and counts must equal the restatement exactly on every row the fixture does not leave out:
tests/test_ctc_prefix_beam_cpu.py asserts on the CPU that every prune and every final ranking of those rows was decided by a gap of at
least 1e-3.  Scores: rtol 1e-5 / atol 1e-4, the tolerance of tests/test_gpu_rnnt_beam.py.
"""
import numpy as np
import pytest
import torch

import ctc_prefix_beam_ref as R
import edit_distance_ref as ED

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -23


def search(emissions, il, W, capacity):
    from haloop_amd import ctc
    return ctc.ctc_prefix_beam_search(emissions, il, W, capacity)


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
    e, il, capacity, ref = R.fixture(name, W)
    return search(e.to(DEV), il.to(DEV), W, capacity), ref


@pytest.mark.parametrize('name,W', R.CASES)
def test_fixture_equals_the_restatement(name, W):
    """small: ragged rows, the row of no frames, width one.  rows17: more rows than any grouping, merges in every row; rows17cap:
    extensions refused at the capacity.  wide: V above the workgroup size and no multiple of 64.  long: the frame loop past 64, both
    parities of the double buffers, long prefixes.  tiny: nothing pruned.  stream: V above what LDS stages, the emissions read from L2.
    deep: 2 W capacity above what LDS holds, the token rows in the workspace.  huge: both, with tokens above 16 bits."""
    got, ref = run_fixture(name, W)
    check(got, ref, R.compared_rows(name, W), f'{name} W={W}')


def test_without_pruning_scores_equal_the_training_loss():
    """N = 2, T = 4, V = 3, cap = 3, W = 16: nothing is pruned, so every score is -functional.ctc_loss(reduction='none') of its
    hypothesis, the project's own training loss on the device."""
    from haloop_amd import functional as HF
    e, il, capacity, ref = R.fixture('tiny', 16)
    ed, ild = e.to(DEV), il.to(DEV)
    tokens, lengths, scores, counts = search(ed, ild, 16, capacity)
    assert counts.tolist() == [13, 13]
    hyp = tokens[:, :13].reshape(26, -1).clamp(min=0)                   # (-1 past a hypothesis's length: never read by the lattice)
    rows = torch.arange(2, device=DEV).repeat_interleave(13)
    losses = HF.ctc_loss(ed[:, rows].contiguous(), hyp, ild[rows], lengths[:, :13].reshape(26), reduction='none')
    print('max |score + loss|', float((scores[:, :13].reshape(26) + losses).abs().max()))
    np.testing.assert_allclose(scores[:, :13].reshape(26).cpu().numpy(), -losses.cpu().numpy(), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('name,W', [('small', 4), ('rows17', 4)])
def test_padding_is_never_read(name, W):
    e, il, capacity, ref = R.fixture(name, W)
    ed, ild = e.to(DEV), il.to(DEV)
    clean = search(ed, ild, W, capacity)
    check(clean, ref, R.compared_rows(name, W), f'{name} W={W}')
    T, N, V = e.shape
    poisoned = ed.clone()
    for n, L in enumerate(il.tolist()):
        poisoned[L:, n] = float('nan')                                  # frames at or past the row's length
    assert same(search(poisoned, ild, W, capacity), clean)
    big = torch.full((N + 1, T + 2, V + 3), float('nan'), device=DEV)   # the gaps of a strided view: rows, frames and classes beyond it
    big[:N, :T, :V] = poisoned.permute(1, 0, 2)
    view = big[:N, :T, :V].permute(1, 0, 2)
    assert view.stride(2) == 1 and not view.is_contiguous()
    assert same(search(view, ild, W, capacity), clean)


def test_nothing_carries_over_and_calls_repeat_bit_for_bit():
    e3, il3, cap3, ref3 = R.fixture('small', 4)
    e17, il17, cap17, ref17 = R.fixture('rows17', 8)
    first = search(e3.to(DEV), il3.to(DEV), 4, cap3)
    between = search(e17.to(DEV), il17.to(DEV), 8, cap17)
    third = search(e3.to(DEV), il3.to(DEV), 4, cap3)
    assert same(first, third)
    check(first, ref3, R.compared_rows('small', 4), 'small W=4')
    check(between, ref17, R.compared_rows('rows17', 8), 'rows17 W=8')


@pytest.mark.parametrize('name,W', [('long', 16), ('deep', 16)])
def test_two_identical_calls_are_bit_equal(name, W):
    e, il, capacity, ref = R.fixture(name, W)
    ed, ild = e.to(DEV), il.to(DEV)
    assert same(search(ed, ild, W, capacity), search(ed, ild, W, capacity))


def test_lengths_default_to_every_frame():
    e, il, capacity, ref = R.fixture('small', 4)
    full = R.beam_search(e, None, e.shape[0], 4)
    rows = [n for n in range(3) if float(full['gaps'][n]) >= R.GAP]
    assert len(rows) >= 2
    check(search(e.to(DEV), None, 4, None), full, rows, 'small W=4, no lengths, default capacity')


def tiny_head(seed=5):
    from haloop_amd import recognizer
    torch.manual_seed(seed)
    head = recognizer.TemporalClassifier(16, 5)
    head.dropout.p = 0.0
    head.beam_size, head.mwer_beam = 0, 0
    return head


def head_inputs(seed=5, scale=3.0):
    """Features at which the float64 search on tiny_head's log-probabilities decides by gaps of 5e-2 at W = 4 (capacity 6 and 4), a list
    holds the empty hypothesis, and width one agrees with greedy on all three rows with more than the greedy path's mass."""
    g = torch.Generator().manual_seed(seed)
    features = scale * torch.randn(3, 6, 16, generator=g)
    return features, torch.tensor([6, 4, 2])


def float64_log_probs(head, features):
    w, b = head.classifier.weight.detach().cpu().double(), head.classifier.bias.detach().cpu().double()
    return torch.nn.functional.linear(features.cpu().double(), w, b).log_softmax(-1)


def test_temporal_classifier_decode_beam_size():
    from haloop_amd import ops
    head = tiny_head().to(DEV).eval()
    features, il = head_inputs()
    x, ild = features.to(DEV), il.to(DEV)
    lp64 = float64_log_probs(head, features)
    ref = R.beam_search(lp64.permute(1, 0, 2), il, 6, 4)
    print('gaps', ref['gaps'].tolist())
    assert float(ref['gaps'].min()) >= R.GAP                            # (this test's own fixture condition)

    # beam_size = 0 and the default: today's greedy output, bit for bit
    with torch.no_grad():
        want = ops.ctc_greedy(head.log_probs(x).contiguous())
    for out in (head.decode(x, ild, None), head.decode(x, ild, None, beam_size=0)):
        hypotheses, output_lengths, alignments, scores, nothing = out
        assert nothing is None and torch.equal(alignments, want[0]) and torch.equal(scores, want[1])
        assert output_lengths.tolist() == want[3].tolist()
        for n, hyp in enumerate(hypotheses.unbind()):
            assert torch.equal(hyp, want[2][n, :int(want[3][n])])
    assert head.last_nbest is None

    out = head.decode(x, ild, None, beam_size=4)
    assert len(out) == 5
    hypotheses, output_lengths, alignments, scores, nothing = out
    assert nothing is None and alignments == [None] * 3 and hypotheses.is_nested
    assert output_lengths.tolist() == ref['lengths'][:, 0].tolist()
    for n, hyp in enumerate(hypotheses.unbind()):
        assert torch.equal(hyp.cpu(), ref['tokens'][n, 0, :ref['lengths'][n, 0]])
    np.testing.assert_allclose(scores.cpu().numpy(), ref['scores'][:, 0].numpy(), rtol=1e-5, atol=1e-4)
    assert head.last_nbest[0].shape == (3, 4, 6)
    check(head.last_nbest, ref, range(3), 'last_nbest')
    head.beam_size = 4                                                  # the attribute, without the keyword
    again = head.decode(x, ild, None)
    assert torch.equal(again[3], scores) and again[1].tolist() == output_lengths.tolist()
    head.beam_size = 0

    # width one against greedy, both over every frame (greedy ignores input_lengths): where they spell the same tokens, the prefix's
    # score holds the greedy alignment's and more
    one = head.decode(x, None, None, beam_size=1)
    assert head.last_nbest[0].shape == (3, 1, 6)
    agree = 0
    for n in range(3):
        if torch.equal(one[0].unbind()[n], want[2][n, :int(want[3][n])]):
            agree += 1
            print('row', n, 'beam 1', float(one[3][n]), 'greedy path', float(want[1][n].sum()))
            assert float(one[3][n]) >= float(want[1][n].sum())
    assert agree >= 1
    head.train()
    with pytest.raises(NotImplementedError):
        head.decode(x, ild, None, beam_size=4)


def test_mwer_forward_against_float64():
    """N = 3, T = 6, V = 5 ('small''s shape), feat_dim 16, W = 4, no dropout: loss and gradients against a float64 restatement on the
    restatement's own n-best list.  Tolerance: that of tests/test_gpu_mwer.py, (W + 8) * 2^-23 * max(1, max err), taken absolutely for
    the loss and for every gradient entry; the worst error is printed as a fraction of it before it is asserted."""
    W, mle = 4, 0.01
    head = tiny_head().to(DEV).train()
    features, il = head_inputs()
    targets, tl = torch.tensor([[1, 3, 2], [4, 4, 0], [2, 0, 0]]), torch.tensor([3, 2, 1])
    cap = 4                                                             # min(T, target_lengths.max() + 1)

    # float64, CPU
    x64 = features.double().requires_grad_(True)
    w64 = head.classifier.weight.detach().cpu().double().requires_grad_(True)
    b64 = head.classifier.bias.detach().cpu().double().requires_grad_(True)
    lp64 = torch.nn.functional.linear(x64, w64, b64).log_softmax(-1)
    ref = R.beam_search(lp64.detach().permute(1, 0, 2), il, cap, W)
    print('gaps', ref['gaps'].tolist(), 'lengths', ref['lengths'].tolist())
    assert float(ref['gaps'].min()) >= R.GAP                            # (this test's own fixture condition)
    assert bool((ref['lengths'] == 0).any(1).any())                     # a list with the empty hypothesis
    want_errors, _ = ED.batch(ref['tokens'].view(3 * W, -1).tolist(), ref['lengths'].view(-1).tolist(), targets.tolist(), tl.tolist(), group=W)
    errors = torch.tensor(want_errors).view(3, W)
    rows = lp64[:, None].expand(3, W, 6, 5).reshape(3 * W, 6, 5)
    losses = torch.nn.functional.ctc_loss(rows.permute(1, 0, 2), ref['tokens'].clamp(min=0).view(3 * W, -1), il.repeat_interleave(W),
                                          ref['lengths'].clamp(min=0).view(-1), reduction='none').view(3, W)
    want = ED.nbest_risk(losses, errors).mean() + mle * torch.nn.functional.ctc_loss(lp64.permute(1, 0, 2), targets, il, tl)
    want.backward()

    x = features.to(DEV).requires_grad_(True)
    outs = []
    for _ in range(2):
        x.grad = None
        head.zero_grad(set_to_none=True)
        loss, info = head.mwer_forward(x, targets, il, tl, beam_size=W, mle_weight=mle)
        loss.backward()
        outs.append((loss.detach().clone(), x.grad.clone(), head.classifier.weight.grad.clone(), head.classifier.bias.grad.clone(), info))
    assert head.training
    loss, gx, gw, gb, info = outs[0]
    check(info['nbest'], ref, range(3), 'mwer n-best')
    assert info['errors'].dtype == torch.int32 and info['errors'].cpu().view(-1).tolist() == want_errors
    assert not info['risk'].requires_grad and not info['nbest_losses'].requires_grad
    tol = (W + 8) * EPS * max(1, max(want_errors))
    report = {'loss': float((loss.cpu().double() - want.detach()).abs()) / tol,
              'features': float((gx.cpu().double() - x64.grad).abs().max()) / tol,
              'classifier.weight': float((gw.cpu().double() - w64.grad).abs().max()) / tol,
              'classifier.bias': float((gb.cpu().double() - b64.grad).abs().max()) / tol}
    print('loss', float(loss), 'float64', float(want.detach()), 'errors as fractions of the tolerance', tol, report)
    assert bool(x64.grad.any()) and bool(w64.grad.any())
    assert all(v <= 1.0 for v in report.values()), report
    again = outs[1]
    assert torch.equal(again[0], loss) and torch.equal(again[1], gx) and torch.equal(again[2], gw) and torch.equal(again[3], gb)
    assert same(again[4]['nbest'], info['nbest'])


def test_mwer_beam_switch():
    head = tiny_head().to(DEV).train()
    features, il = head_inputs()
    x = features.to(DEV)
    targets, tl = torch.tensor([[1, 3, 2], [4, 4, 0], [2, 0, 0]]), torch.tensor([3, 2, 1])
    plain, stats = head(x, targets, il, tl)
    assert stats == {}
    head.mwer_beam = 3
    a, info_a = head(x, targets, il, tl)
    b, info_b = head.mwer_forward(x, targets, il, tl, beam_size=3)
    assert torch.equal(a.detach(), b.detach()) and same(info_a['nbest'], info_b['nbest']) and info_a['nbest'][1].shape == (3, 3)
    head.eval()
    c, stats = head(x, targets, il, tl)
    assert stats == {} and torch.equal(c.detach(), plain.detach())
