"""The vectorised float64 lattice yardstick (tests/lattice_ref.py) against everything that already pins these lattices on the CPU: the
reference-generated fixtures g8_star.npz / g9_transducer.npz / g8_star_edges.npz (losses and the reference's autograd gradients, at
the tolerances tests/test_oracle_golden.py holds oracle/star_ref.py to) and oracle/star_ref.py itself on the two seeded cases of
tests/test_gpu_lattice.py.  The float32 mode must land near the float64 one: it is the measure of fp32 loss in
tests/test_gpu_lattice_f64.py."""
import numpy as np
import pytest
import torch

import lattice_ref as L
from conftest import load_golden
from test_oracle_golden import STAR_CASES, STAR_EDGE_CASES, TRANSDUCER_CASES, star_case_from_golden


@pytest.mark.parametrize('name', STAR_CASES + ['demo'] + STAR_EDGE_CASES)
def test_star_reference_reproduces_the_fixtures(name):
    g = load_golden('g8_star_edges' if name in STAR_EDGE_CASES else 'g8_star')
    em, tg, il, tl, pen = star_case_from_golden(g, name)
    losses, grad = L.star_ctc(em, tg, il, tl, pen, 'float64')
    np.testing.assert_allclose(losses, g[name + '.losses'], rtol=2e-6, atol=1e-5)
    l32, g32 = L.star_ctc(em, tg, il, tl, pen, 'float32')
    assert l32.dtype == np.float32 and g32.dtype == np.float32
    np.testing.assert_allclose(l32, losses, rtol=2e-6, atol=1e-5)
    if name == 'demo':
        return
    np.testing.assert_allclose(grad, g[name + '.grad'], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(g32, grad, rtol=1e-4, atol=2e-6)
    for n in range(em.shape[1]):
        assert not grad[int(il[n]):, n].any(), 'frames past the emission length carry no gradient'


@pytest.mark.parametrize('name', TRANSDUCER_CASES)
def test_transducer_reference_reproduces_the_fixtures(name):
    g = load_golden('g9_transducer')
    t = lambda k: torch.from_numpy(g[name + '.' + k])
    joint, tg, jl, tl = t('joint'), t('targets'), t('jl'), t('tl')
    losses, grad = L.transducer(joint, tg, jl, tl, 'float64')
    np.testing.assert_allclose(losses.numpy(), g[name + '.losses'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad.numpy(), g[name + '.grad'], rtol=1e-4, atol=2e-6)
    l32, g32 = L.transducer(joint, tg, jl, tl, 'float32')
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32
    np.testing.assert_allclose(l32.numpy(), losses.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g32.numpy(), grad.numpy(), rtol=1e-4, atol=2e-6)


def test_star_reference_agrees_with_the_oracle_on_the_seeded_case():
    """tests/test_gpu_lattice.py test_star_ctc_weighted_backward_time_strided_and_helpers' inputs (seed 11)."""
    from oracle import star_ref
    g = torch.Generator().manual_seed(11)
    T, N, C, S = 30, 6, 40, 9
    em = torch.randn(N, T, C, generator=g).log_softmax(-1).permute(1, 0, 2)
    tg = torch.randint(1, C, (N, S), generator=g)
    il = torch.randint(20, T + 1, (N,), generator=g)
    tl = torch.randint(1, S + 1, (N,), generator=g)
    losses, grad = L.star_ctc(em, tg, il, tl, -1.25, 'float64')
    np.testing.assert_allclose(star_ref.star_ctc_forward_score(em, tg, il, tl, star_penalty=-1.25).numpy(), losses, rtol=2e-6, atol=1e-5)
    np.testing.assert_allclose(star_ref.star_ctc_grad(em, tg, il, tl, star_penalty=-1.25).numpy(), grad, rtol=1e-4, atol=2e-6)


def test_transducer_reference_agrees_with_the_oracle_on_the_seeded_case():
    """tests/test_gpu_lattice.py test_transducer_any_length_against_oracle's inputs (seed 3): T = 21, labels that are 0, an empty target."""
    from oracle import star_ref
    g = torch.Generator().manual_seed(3)
    N, T, U, K = 4, 21, 6, 12
    joint = (torch.randn(N, T, 1, K, generator=g) + torch.randn(N, 1, U + 1, K, generator=g)).log_softmax(-1)
    tg = torch.randint(0, K, (N, U), generator=g)
    jl, tl = torch.tensor([21, 20, 9, 1], dtype=torch.int32), torch.tensor([6, 3, 0, 2], dtype=torch.int32)
    w = torch.rand(N, generator=g) + 0.5
    losses, grad = L.transducer(joint, tg, jl, tl, 'float64', weights=w)
    np.testing.assert_allclose(star_ref.transducer_forward_score(joint, tg, jl, tl).numpy(), losses.numpy(), rtol=1e-5, atol=1e-5)
    ref_g = star_ref.transducer_grad(joint, tg, jl, tl) * w[:, None, None, None]
    np.testing.assert_allclose(ref_g.numpy(), grad.numpy(), rtol=1e-4, atol=2e-6)


def test_additive_joint_form_is_the_dense_yardstick():
    """transducer_additive against tests/rnnt_loss_ref.py's own dense transducer_loss_ref on its 'ragged' shape: the same float64 numbers."""
    import rnnt_loss_ref as R
    f, g, tg, fl, tl, w = R.make_case(3, 7, 5, 37, [7, 1, 4], [4, 0, 2], 41, True)
    want = R.transducer_loss_ref(f, g, tg, fl, tl, w)
    got = L.transducer_additive(f, g, tg, fl, tl, 'float64', weights=w)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=1e-13)


def test_star_reference_is_finite_where_every_star_is_log_zero():
    """C = 2: <star\\1> = log 0 in every frame; the alpha-beta gradient has no 0 * inf."""
    g = torch.Generator().manual_seed(5)
    em = torch.randn(8, 2, 2, generator=g).log_softmax(-1)
    tg = torch.ones(2, 3, dtype=torch.int64)
    for dtype in ('float64', 'float32'):
        losses, grad = L.star_ctc(em, tg, torch.tensor([8, 5]), torch.tensor([3, 1]), -0.5, dtype)
        assert np.isfinite(losses).all() and np.isfinite(grad).all() and grad[:5].any()
