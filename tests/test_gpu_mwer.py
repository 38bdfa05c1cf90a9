"""GPU checks of minimum-word-error-rate training on n-best lists: transducer.nbest_risk (csrc/edit_distance.hip) against the float64
yardstick tests/edit_distance_ref.py, and recognizer.Transducer.mwer_forward / mwer_beam against a composition of the library's own
calls written here.  Every launch on that path is deterministic, so the comparison is torch.equal -- the prediction network's embedding
gradient included, which both sides take in token order (``ordered_grad``): the ordinary one scatter-adds with float atomics, and
with it the gradient of lm.embedding.weight alone differed between two evaluations, by one unit in the last place (9.3e-10).

Tolerance of the risk and of every gradient entry of a row: (W + 8) * 2^-23 * max(1, max_w err_w) -- W roundings in the sums, a few
ulp for each exponential and the division, and the rounding of an exponent d = loss_w - min loss, which moves its term by at most
d e^-d 2^-24 <= 0.37 * 2^-24.  The worst error is printed as a fraction of it before it is asserted."""
import pytest
import torch

import edit_distance_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -23


@pytest.mark.parametrize('W', [1, 3, 16])
def test_nbest_risk_matches_the_float64_formula(W):
    from haloop_amd import transducer
    N = 5
    g = torch.Generator().manual_seed(40 + W)
    losses = (20 + 5 * torch.randn(N, W, generator=g)).float()
    errors = torch.randint(0, 9, (N, W), generator=g, dtype=torch.int32)
    errors[3, :] = -1                                       # a row with everything absent
    if W > 1:
        errors[1, 1] = -1                                   # rows with absent entries
        errors[2, 1:] = -1                                  # ... down to a single hypothesis
        errors[4, 0] = -1
    l = losses.to(DEV).requires_grad_(True)
    risk = transducer.nbest_risk(l, errors.to(DEV))
    assert risk.shape == (N,) and risk.dtype == torch.float32
    weights = torch.tensor([1.0, -2.0, 0.5, 3.0, 1.5])
    (risk * weights.to(DEV)).sum().backward()
    want = R.nbest_risk(losses, errors)
    want_grad = R.nbest_risk_grad(losses, errors) * weights.double()[:, None]
    tol = (W + 8) * EPS * errors.max(1).values.clamp(min=1).double()
    err_risk = (risk.detach().cpu().double() - want).abs() / tol
    err_grad = (l.grad.cpu().double() - want_grad).abs() / (tol * weights.abs().double())[:, None]
    print(f'W = {W}: worst risk error {float(err_risk.max()):.3f}, worst gradient error {float(err_grad.max()):.3f} of the tolerance')
    assert float(err_risk.max()) <= 1.0
    assert float(err_grad.max()) <= 1.0
    assert float(risk.detach()[3]) == 0.0 and not l.grad[3].any()
    assert not l.grad.cpu()[errors < 0].any()
    if W == 1:
        assert not risk.detach().any() and not l.grad.any()  # one hypothesis: expected error = mean error
    again = transducer.nbest_risk(l.detach(), errors.to(DEV))
    assert torch.equal(again, risk.detach())


def test_ordered_embedding_gradient():
    """functional.embedding(..., ordered_grad=True): the gradient of the atomic scatter-add up to the order of its sums, the same bits on
    every call, rows no token names zero.  Many tokens share a row here (ids over 5 of 8 symbols), which is where the order shows."""
    from haloop_amd import functional as HF
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(0, 5, (9, 7), generator=g).to(DEV)
    weight = torch.randn(8, 512, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(9, 7, 512, generator=g).to(DEV)
    out = {}
    for ordered in (False, True, True):
        weight.grad = None
        y = HF.embedding(ids, weight, ordered)
        assert torch.equal(y, weight.detach()[ids])
        y.backward(dy)
        out.setdefault(ordered, []).append(weight.grad.clone())
    want = torch.zeros(8, 512, dtype=torch.float64).index_add_(0, ids.view(-1).cpu(), dy.view(-1, 512).cpu().double())
    assert torch.equal(out[True][0], out[True][1])
    assert not out[True][0][5:].any()
    # 63 addends of magnitude ~1 a row at most: 64 roundings of partial sums below 64 * 5
    assert float((out[True][0].cpu().double() - want).abs().max()) <= 64 * 320 * 2.0 ** -24
    assert float((out[False][0].cpu().double() - want).abs().max()) <= 64 * 320 * 2.0 ** -24


def make_head(seed=3):
    from haloop_amd import recognizer
    torch.manual_seed(seed)
    head = recognizer.Transducer(feat_dim=32, vocab_size=8)
    head.dropout.p = 0.0
    head.lm.rnn.dropout = 0.0
    head.fused_loss, head.mwer_beam = False, 0
    return head.to(DEV).train()


def small_batch(N=3, T=6, U=3, seed=9):
    g = torch.Generator().manual_seed(seed)
    features = torch.randn(N, T, 32, generator=g).to(DEV)
    targets = torch.randint(1, 8, (N, U), generator=g).to(DEV)
    il = torch.tensor([T, T - 2, T - 1, T][:N]).to(DEV)
    tl = torch.tensor([U, U - 1, 1, U][:N]).to(DEV)
    return features, targets, il, tl


def nbest_losses(head, feats, il, nbest):
    """-log P(hypothesis | x) of every hypothesis of an n-best list, on the expand + reshape rows of feats: [N, W]."""
    from haloop_amd import transducer
    tokens, lengths = nbest[0], nbest[1]
    N, W, _ = tokens.shape
    T, V = feats.shape[1], feats.shape[2]
    hyps = tokens.clamp(min=0).view(N * W, -1)
    lm_in = torch.cat([hyps.new_zeros((N * W, 1)), hyps], dim=1)
    g, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(N * W), ordered_grad=True)
    rows = feats[:, None].expand(N, W, T, V).reshape(N * W, T, V)
    return transducer.transducer_loss(rows, g, hyps, il[:, None].expand(N, W).reshape(-1), lengths.clamp(min=0).view(-1)).view(N, W)


def composition(head, features, targets, il, tl, nbest, mle_weight):
    from haloop_amd import functional as HF, transducer, wer
    N, W = nbest[1].shape
    errors, _ = wer.edit_distance(nbest[0], nbest[1], targets, tl, group=W)
    feats = HF.linear(features.float(), head.classifier.weight, head.classifier.bias)
    losses = nbest_losses(head, feats, il, nbest)
    loss = transducer.nbest_risk(losses, errors.view(N, W)).mean()
    if mle_weight != 0:
        lm_in = torch.cat([targets.new_zeros((N, 1)), targets], dim=1)
        g, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(N), ordered_grad=True)
        loss = loss + mle_weight * transducer.transducer_loss(feats, g, targets, il, tl).mean()
    return loss, losses.detach()


def checked_parameters(head):
    return [('classifier.weight', head.classifier.weight), ('classifier.bias', head.classifier.bias)] + \
        [('lm.' + k, p) for k, p in head.lm.named_parameters()]


def grads(head):
    out = {k: p.grad.clone() for k, p in checked_parameters(head)}
    head.zero_grad(set_to_none=True)
    return out


def test_mwer_forward_equals_the_composition():
    head = make_head()
    features, targets, il, tl = small_batch()
    loss, info = head.mwer_forward(features, targets, il, tl, beam_size=3, mle_weight=0.01)
    loss.backward()
    got = grads(head)
    assert head.training and all(m.training for m in head.modules())
    tokens, lengths, scores, counts = info['nbest']
    assert tokens.shape == (3, 3, int(tl.max()) + 1) and lengths.shape == (3, 3)
    want_errors, _ = R.batch(tokens.view(9, -1).tolist(), lengths.view(-1).tolist(), targets.tolist(), tl.tolist(), group=3)
    assert info['errors'].dtype == torch.int32 and info['errors'].view(-1).tolist() == want_errors
    assert not info['risk'].requires_grad and not info['nbest_losses'].requires_grad

    ref_loss, ref_losses = composition(head, features, targets, il, tl, info['nbest'], 0.01)
    ref_loss.backward()
    want = grads(head)
    assert torch.equal(info['nbest_losses'], ref_losses)
    assert torch.equal(loss.detach(), ref_loss.detach()), (float(loss), float(ref_loss))
    differing = {k: float((got[k] - want[k]).abs().max()) for k in want if not torch.equal(got[k], want[k])}
    print(f'parameters whose gradients differ between mwer_forward and the composition: {differing}')
    assert all(want[k].any() for k in want)
    assert not differing


def test_one_hypothesis_without_the_mle_term_is_exactly_zero():
    head = make_head()
    features, targets, il, tl = small_batch()
    loss, info = head.mwer_forward(features, targets, il, tl, beam_size=1, mle_weight=0)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not info['risk'].any()
    for k, p in checked_parameters(head):
        assert p.grad is None or not p.grad.any(), k


@pytest.mark.parametrize('fused', [False, True])
def test_mwer_beam_switch(fused):
    from haloop_amd import functional as HF, transducer
    head = make_head()
    head.fused_loss = fused
    features, targets, il, tl = small_batch()
    # 0: forward is the head's ordinary loss, by the fused or the dense route
    loss, stats = head(features, targets, il, tl)
    assert stats == {}
    lm_in = torch.cat([targets.new_zeros((3, 1)), targets], dim=1)
    g, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(3))
    feats = HF.linear(features.float(), head.classifier.weight, head.classifier.bias)
    if fused:
        want = transducer.transducer_loss(feats, g, targets, il, tl).mean()
    else:
        want = transducer.transducer_forward_score(HF.log_softmax(feats[:, :, None, :] + g[:, None, :, :]), targets, il, tl).mean()
    assert torch.equal(loss.detach(), want.detach())
    # 3, training: forward is mwer_forward at that width; in eval mode it stays the ordinary loss
    head.mwer_beam = 3
    a, info_a = head(features, targets, il, tl)
    b, info_b = head.mwer_forward(features, targets, il, tl, beam_size=3)
    assert torch.equal(a.detach(), b.detach()) and torch.equal(info_a['nbest'][0], info_b['nbest'][0])
    assert info_a['nbest'][1].shape == (3, 3)
    head.eval()
    c, stats = head(features, targets, il, tl)
    assert stats == {} and torch.equal(c.detach(), loss.detach())


def test_training_flag_is_restored_when_the_search_raises():
    head = make_head()
    features, targets, il, tl = small_batch()
    head.lm.eval()                                          # a mode of a submodule that differs from the head's
    with pytest.raises(ValueError):
        head.mwer_forward(features, targets, torch.cat([il, il[:1]]), tl, beam_size=3)
    assert head.training and head.classifier.training and not head.lm.training and not head.lm.rnn.training
    head.train()
    head.mwer_forward(features, targets, il, tl, beam_size=2)
    assert all(m.training for m in head.modules())


def test_ten_steps_lower_the_expected_error_of_the_first_nbest_list():
    from haloop_amd import functional as HF
    head = make_head(seed=21)
    features, targets, il, tl = small_batch(N=4, T=8, U=3, seed=22)
    opt = torch.optim.AdamW(head.parameters(), lr=1e-3)

    def expected_error(nbest, errors):
        with torch.no_grad():
            feats = HF.linear(features.float(), head.classifier.weight, head.classifier.bias)
            losses = nbest_losses(head, feats, il, nbest)
        present = errors >= 0
        p = torch.softmax(torch.where(present, -losses.double(), torch.full_like(losses, float('-inf'), dtype=torch.float64)), 1)
        return float((p * errors.clamp(min=0)).sum(1).mean())

    first = None
    for step in range(10):
        opt.zero_grad(set_to_none=True)
        loss, info = head.mwer_forward(features, targets, il, tl, beam_size=4, mle_weight=0)
        if first is None:
            first = (info['nbest'], info['errors'])
            before = expected_error(*first)
        loss.backward()
        opt.step()
    after = expected_error(*first)
    print(f'expected error of the step-0 n-best list: {before:.6f} before, {after:.6f} after ten AdamW steps')
    assert after < before
