"""GPU checks of the transducer loss over the additive joint (haloop_amd.transducer.transducer_loss, csrc/rnnt_loss.hip) against the
float64 yardstick tests/rnnt_loss_ref.py (pinned to the oracle lattice by tests/test_rnnt_loss_cpu.py).  Inputs are seeded randn
logits scaled by 3.  Tolerances are the project's lattice tolerances (tests/test_gpu_lattice.py): losses rtol 1e-5 / atol 1e-4,
gradients rtol 1e-4 / atol 5e-6.  Where a gradient misses that bound the existing dense route (HF.log_softmax +
transducer_forward_score + autograd) runs on the same inputs and the fused route is allowed twice ITS maximum error against the
yardstick: a sum in another order cannot be asked to beat the route it replaces.  Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import rnnt_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = {
    # N, T, U1, V, f_lengths, target_lengths, seed, repeat_label
    'ragged': (3, 7, 5, 37, [7, 1, 4], [4, 0, 2], 41, True),          # a single-frame row, an empty target, a full row; V % 4 != 0
    'tile_tu': (2, 33, 18, 256, None, None, 43, False),               # T and U + 1 one past a power of two
    'tile_v': (2, 5, 3, 1030, None, None, 44, False),                 # V: more than one pass of a 256-thread workgroup, with a tail
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the float64 reference of a case, computed once and shared (nothing writes to them)."""
    inputs = R.make_case(*CASES[name])
    f, g, tg, fl, tl, w = inputs
    return inputs, R.transducer_loss_ref(f, g, tg, fl, tl, w)


def run_fused(f, g, tg, fl, tl, w):
    from haloop_amd import transducer
    fd, gd = f.to(DEV).requires_grad_(True), g.to(DEV).requires_grad_(True)
    losses = transducer.transducer_loss(fd, gd, tg.to(DEV), fl.to(DEV), tl.to(DEV))
    (losses * w.to(DEV)).sum().backward()
    return losses.detach().cpu(), fd.grad.cpu(), gd.grad.cpu()


def run_dense(f, g, tg, fl, tl, w):
    from haloop_amd import functional as HF, transducer
    fd, gd = f.to(DEV).requires_grad_(True), g.to(DEV).requires_grad_(True)
    joint = fd[:, :, None, :] + gd[:, None, :, :]
    losses = transducer.transducer_forward_score(HF.log_softmax(joint), tg.to(DEV), fl.to(DEV), tl.to(DEV))
    (losses * w.to(DEV)).sum().backward()
    return losses.detach().cpu(), fd.grad.cpu(), gd.grad.cpu()


def within(got, want, rtol, atol):
    return bool((torch.abs(got.double() - want) <= atol + rtol * torch.abs(want)).all())


def check_case(name, got=None):
    inputs, (ref_l, ref_df, ref_dg) = case(name)
    losses, df, dg = got if got is not None else run_fused(*inputs)
    err = lambda a, b: float((a.double() - b).abs().max())
    print(f'{name}: fused max abs error  losses {err(losses, ref_l):.3e}  df {err(df, ref_df):.3e}  dg {err(dg, ref_dg):.3e}')
    np.testing.assert_allclose(losses.numpy(), ref_l.numpy(), rtol=1e-5, atol=1e-4)
    if not (within(df, ref_df, 1e-4, 5e-6) and within(dg, ref_dg, 1e-4, 5e-6)):
        _, ddf, ddg = run_dense(*inputs)
        print(f'{name}: dense max abs error  df {err(ddf, ref_df):.3e}  dg {err(ddg, ref_dg):.3e}')
        assert err(df, ref_df) <= 2 * err(ddf, ref_df), 'df: more than twice the dense route\'s error'
        assert err(dg, ref_dg) <= 2 * err(ddg, ref_dg), 'dg: more than twice the dense route\'s error'
    return inputs, (losses, df, dg)


def test_ragged_case_weighted_backward():
    (f, g, tg, fl, tl, w), (losses, df, dg) = check_case('ragged')
    for n in range(f.shape[0]):
        assert not df[n, int(fl[n]):].any(), 'df rows at t >= T_n must be exactly zero'
        assert not dg[n, int(tl[n]) + 1:].any(), 'dg rows at u > U_n must be exactly zero'
    assert df[0].any() and dg[1, 0].any()


@pytest.mark.parametrize('name', ['tile_tu', 'tile_v'])
def test_tile_edges(name):
    check_case(name)


def test_strided_operands_are_read_and_written_in_place():
    """g as the transpose of a time-major [U + 1, N, V] tensor (what Decoder.forward_batch_first returns), f as [:, :, :V] of a wider
    buffer: bit-identical to the contiguous copies' results, and g.grad arrives with the right values."""
    from haloop_amd import transducer
    (f, g, tg, fl, tl, w), (ref_l, ref_df, ref_dg) = case('ragged')
    l0, df0, dg0 = run_fused(f, g, tg, fl, tl, w)
    N, T, V = f.shape
    wide = torch.randn(N, T, V + 11).to(DEV)
    wide[:, :, :V] = f.to(DEV)
    wide.requires_grad_(True)
    g_tm = g.transpose(0, 1).contiguous().to(DEV).requires_grad_(True)          # [U + 1, N, V]
    fv, gv = wide[:, :, :V], g_tm.transpose(0, 1)
    assert not fv.is_contiguous() and not gv.is_contiguous()
    losses = transducer.transducer_loss(fv, gv, tg.to(DEV), fl.to(DEV), tl.to(DEV))
    (losses * w.to(DEV)).sum().backward()
    assert torch.equal(losses.detach().cpu(), l0)
    assert torch.equal(wide.grad[:, :, :V].cpu(), df0) and not wide.grad[:, :, V:].any()
    assert torch.equal(g_tm.grad.transpose(0, 1).cpu(), dg0)
    check_case('ragged', (losses.detach().cpu(), wide.grad[:, :, :V].cpu(), g_tm.grad.transpose(0, 1).cpu()))


def test_backward_is_reproducible():
    inputs, _ = case('ragged')
    _, df0, dg0 = run_fused(*inputs)
    _, df1, dg1 = run_fused(*inputs)
    assert torch.equal(df0, df1) and torch.equal(dg0, dg1)


def test_no_joint_sized_tensor_is_allocated():
    """N = 4, T = 200, U + 1 = 50, V = 512: ONE dense [N, T, U + 1, V] fp32 tensor is 81.9 MB (the dense route holds several); the fused
    route needs df + dg + lse + lp2 + alpha + the lattice gradient = about 2.3 MB.  The bound is that one tensor."""
    from haloop_amd import transducer
    N, T, U1, V = 4, 200, 50, 512
    f, g, tg, fl, tl, w = (x.to(DEV) for x in R.make_case(N, T, U1, V, [200, 150, 200, 37], [49, 30, 0, 49], 45))
    f.requires_grad_(True); g.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    losses = transducer.transducer_loss(f, g, tg, fl, tl)
    (losses * w).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f'peak rise {rise / 1e6:.2f} MB')
    assert rise < N * T * U1 * V * 4
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(f.grad).all()) and bool(torch.isfinite(g.grad).all())


@functools.lru_cache(maxsize=None)
def head_case():
    """The construction and CPU composition of test_transducer_head_matches_cpu_composition (tests/test_gpu_lattice.py)."""
    from haloop_amd import recognizer
    from oracle import star_ref
    g = torch.Generator().manual_seed(31)
    N, T, H, V, U = 3, 12, 48, 20, 5
    feats = torch.randn(N, T, H, generator=g)
    tg = torch.randint(1, V, (N, U), generator=g)
    il, tl = torch.tensor([12, 9, 12]), torch.tensor([5, 3, 4])
    torch.manual_seed(5)
    head = recognizer.Transducer(H, V).eval()
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    E = 512
    lstm = torch.nn.LSTM(E, E, 2)
    lstm.load_state_dict({k[len('lm.rnn.'):]: v for k, v in sd.items() if k.startswith('lm.rnn.')})
    emb = sd['lm.embedding.weight'].clone().requires_grad_(True)
    ob = sd['lm.out_layer.bias'].clone().requires_grad_(True)
    cw, cb = sd['classifier.weight'].clone().requires_grad_(True), sd['classifier.bias'].clone().requires_grad_(True)
    lm_in = torch.cat([tg.new_zeros((N, 1)), tg], dim=1)
    out, _ = lstm(torch.nn.functional.embedding(lm_in, emb).transpose(0, 1))
    lm_out = torch.nn.functional.linear(out, emb, ob).transpose(0, 1)
    f = torch.nn.functional.linear(feats, cw, cb)
    joint = (f[:, :, None, :] + lm_out[:, None, :, :]).log_softmax(-1)
    jl, tl32 = il.to(torch.int32), tl.to(torch.int32)
    ref_losses = star_ref.transducer_forward_score(joint.detach(), tg, jl, tl32)
    joint.backward(gradient=star_ref.transducer_grad(joint.detach(), tg, jl, tl32) / N)
    ref = dict(loss=float(ref_losses.mean()), cw=cw.grad, cb=cb.grad, emb=emb.grad, lstm={k: p.grad for k, p in lstm.named_parameters()})
    return head.to(DEV), feats, tg, il, tl, ref


@pytest.mark.parametrize('fused', [True, False])
def test_head_matches_cpu_composition(fused):
    """recognizer.Transducer with fused_loss on: the loss and every parameter gradient against the CPU composition; with it off the
    head gives what it gives today (the same composition, the same tolerances)."""
    head, feats, tg, il, tl, ref = head_case()
    head.zero_grad(set_to_none=True)
    head.fused_loss = fused
    try:
        loss, stats = head(feats.to(DEV), tg, il, tl)
        loss.backward()
    finally:
        head.fused_loss = False
    assert stats == {}
    np.testing.assert_allclose(float(loss.detach()), ref['loss'], rtol=2e-5)
    np.testing.assert_allclose(head.classifier.weight.grad.cpu().numpy(), ref['cw'].numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(head.classifier.bias.grad.cpu().numpy(), ref['cb'].numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(head.lm.embedding.weight.grad.cpu().numpy(), ref['emb'].numpy(), rtol=2e-3, atol=2e-5)
    for k, p_ in head.lm.rnn.named_parameters():
        np.testing.assert_allclose(p_.grad.cpu().numpy(), ref['lstm'][k].numpy(), rtol=2e-3, atol=2e-5, err_msg=k)


def test_argument_errors_are_raised_before_any_launch():
    from haloop_amd import transducer
    (f, g, tg, fl, tl, w), _ = case('ragged')
    fd, gd, V, T = f.to(DEV), g.to(DEV), f.shape[2], f.shape[1]
    bad = tg.clone(); bad[0, 0] = V
    with pytest.raises(ValueError):
        transducer.transducer_loss(fd, gd, bad.to(DEV), fl.to(DEV), tl.to(DEV))
    with pytest.raises(ValueError):
        transducer.transducer_loss(fd, gd, tg.to(DEV), (fl + T).to(DEV), tl.to(DEV))
    with pytest.raises(ValueError):
        transducer.transducer_loss(fd, gd, tg[:, :3].to(DEV), fl.to(DEV), tl.to(DEV))
