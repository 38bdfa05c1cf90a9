"""The star-CTC and transducer lattices (csrc/lattice.hip; csrc/rnnt_loss.hip around them for the fused route) against the float64
yardstick tests/lattice_ref.py, at the sizes where their strided loops take a second trip -- more than 256 lattice states, more than
64 and more than 256 symbols, more than 256 cells on an anti-diagonal -- and at the edges of the arithmetic: losses of thousands of
nats, peaked posteriors (cancellation in <star\\s>), -inf log-probabilities, C = 2 (every <star\\s> is log 0), empty targets, labels equal
to the blank.  Every case runs (losses * w).sum().backward() with w in [0.5, 1.5] and compares the losses and EVERY gradient element.

Tolerance.  The kernels are fp32, so a case is allowed what fp32 arithmetic itself loses on it: with e32 = max|ref(float32) - ref(float64)|
(the yardstick's own float32 run, computed on the CPU, separately for losses and gradients), an element may be off by

    max(floor, 4 * e32)        floor = 1e-5 |loss| + 1e-4 (losses), 1e-4 |g| + 5e-6 (gradients): what tests/test_gpu_lattice.py grants

The 4 covers another, equally valid order of the same sums (the wave reduction of star_complete, anti-diagonals against rows, the LDS
atomics).  It is never taken from the kernel's own error.

Observed (e32 on the CPU; kernel = max |kernel - float64| on an MI355X), losses / gradients:

    case                              e32 loss   kernel loss  e32 grad   kernel grad
    star states_two_trips             3.5e-05    3.5e-05      3.7e-05    8.0e-05
    star states_edge_63               1.2e-05    1.1e-05      1.5e-05    5.0e-05
    star states_edge_64               6.4e-06    6.4e-06      2.9e-05    3.1e-05
    star symbols_two_trips            2.6e-06    1.0e-05      4.1e-06    5.9e-06
    star symbols_edge_2               2.2e-06    2.2e-06      2.1e-06    2.5e-06
    star symbols_edge_64              3.4e-06    2.6e-06      3.1e-06    1.5e-06
    star symbols_edge_65              3.3e-06    5.2e-06      3.5e-06    4.2e-06
    star symbols_edge_257             3.2e-06    3.5e-06      3.5e-06    3.7e-06
    star repeats_long                 2.5e-05    2.5e-05      3.1e-05    2.7e-05
    star long                         9.1e-04    1.1e-03      1.3e-03    2.9e-03
    star peaked                       2.0e-05    2.0e-05      2.4e-05    3.5e-05
    star masked                       5.4e-06    5.4e-06      6.5e-06    6.4e-06
    star empty_target                 9.3e-07    1.9e-06      6.3e-07    2.1e-06
    star time_major_view              4.7e-05    4.7e-05      5.5e-05    6.5e-05
    transducer diag_two_trips         4.9e-05    4.9e-05      1.6e-05    1.6e-05
    transducer diag_edge_256          6.0e-05    6.0e-05      2.7e-06    2.6e-06
    transducer diag_edge_257          1.2e-04    1.5e-04      1.3e-05    6.6e-06
    transducer long                   2.2e-03    2.2e-03      5.5e-07    6.1e-07
    transducer label_is_blank         9.9e-07    9.9e-07      2.9e-07    3.0e-07
    transducer fused_route_wide_u df                          3.1e-04    3.1e-04
    transducer fused_route_wide_u dg  1.1e-03    1.1e-03      1.2e-04    1.2e-04

The star yardstick's float32 run is the same alpha-beta formulation as star_beta_grad_kernel (occupancies exp(alpha + beta - logZ)).  At
'star long' that is not what costs the 1.3e-3: a float32 run that hands the state posteriors back through the local weights of every
logaddexp, as autograd would, is off by 2.9e-3 there -- 2000 frames of fp32 rounding in the forward lattice itself.  The transducer is
different: its yardstick's float32 run is autograd through the recurrence and loses 5.5e-7 at 'transducer long' (2242 nats), while the
kernel, which formed its occupancies the alpha-beta way, was off by 3.4e-3 there, 1.3e-4 at diag_two_trips and 1.0e-2 in df of the fused
route -- outside the bound -- until it carried the cell posteriors through local arc weights (the kernel column is from after that change).
"""
import functools

import numpy as np
import pytest
import torch

import lattice_ref as L
import rnnt_loss_ref as R
from conftest import load_golden
from test_oracle_golden import star_case_from_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------------------------------------------------------------- star-CTC
def _star_inputs(T, C, S, il, tl, seed, scale=1.0, N=3, masked=()):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, T, C, generator=g) * scale
    if masked:
        logits[:, :, list(masked)] = float('-inf')
    hi = min(masked) if masked else C
    tg = torch.ones(N, S, dtype=torch.int64) if C == 2 else torch.randint(1, hi, (N, S), generator=g)
    w = torch.rand(N, generator=g) + 0.5
    return logits.log_softmax(-1), tg, torch.tensor(il), torch.tensor(tl), -0.5, w          # lp is [N, T, C]


def _repeats(seed, S, C, N=3):
    """Runs of one to three equal labels, neighbouring runs distinct; row 0 ends inside a run, row 1 at a change of label."""
    g = torch.Generator().manual_seed(seed)
    tg = torch.zeros(N, S, dtype=torch.int64)
    for n in range(N):
        k, last = 0, 0
        while k < S:
            lab = int(torch.randint(1, C, (1,), generator=g))
            if lab == last:
                continue
            run = int(torch.randint(1, 4, (1,), generator=g))
            tg[n, k:k + run] = lab
            k, last = k + run, lab
    tg[0, S - 1] = tg[0, S - 2]
    tg[1, S - 1] = tg[1, S - 2] % (C - 1) + 1
    return tg


def _repeats_long():
    lp, _, il, tl, pen, w = _star_inputs(120, 9, 40, [120, 101, 120], [40, 37, 22], 109)
    tg = _repeats(109, 40, 9)
    tg[2, 22:] = 0                                                          # target padding past tl
    return lp, tg, il, tl, pen, w


def _empty_target():
    """The inputs of the reference-generated fixture (tests/golden/make_golden_star_edges.py): tl = 0, 4, 0; il = 15, 15, 1."""
    em, tg, il, tl, pen = star_case_from_golden(load_golden('g8_star_edges'), 'empty_target')
    return em.permute(1, 0, 2).contiguous(), tg, il, tl, pen, torch.tensor([0.75, 1.25, 1.5])


STAR = {
    # 4S+3 = 283: a second trip of the state loops (tail 27); C = 70: a second 64-lane trip of star_complete (tail 5).  tl = 64 reads
    # out states 255 .. 258, across the trip boundary; tl = 70 reads the last states of the second trip.
    'states_two_trips': lambda: _star_inputs(160, 70, 70, [160, 151, 160], [70, 64, 33], 101),
    'states_edge_63': lambda: _star_inputs(80, 12, 63, [80, 77, 80], [63, 62, 31], 102),            # 4S+3 = 255
    'states_edge_64': lambda: _star_inputs(80, 12, 64, [80, 77, 80], [64, 63, 31], 103),            # 4S+3 = 259
    'symbols_two_trips': lambda: _star_inputs(40, 300, 5, [40, 29, 40], [5, 3, 5], 104),            # the gradient's symbol loops: 256 + 44
    'symbols_edge_2': lambda: _star_inputs(24, 2, 3, [24, 17, 24], [3, 2, 1], 105),                 # every <star\\s> is log 0
    'symbols_edge_64': lambda: _star_inputs(24, 64, 3, [24, 17, 24], [3, 2, 1], 106),               # c = 1 + lane: the last lane
    'symbols_edge_65': lambda: _star_inputs(24, 65, 3, [24, 17, 24], [3, 2, 1], 107),               # ... and the first of a second trip
    'symbols_edge_257': lambda: _star_inputs(24, 257, 3, [24, 17, 24], [3, 2, 1], 108),
    'repeats_long': _repeats_long,
    'long': lambda: _star_inputs(2000, 32, 30, [2000, 1337, 1], [30, 12, 1], 110),                  # losses of thousands of nats
    'peaked': lambda: _star_inputs(60, 20, 8, [60, 47, 60], [8, 5, 8], 111, scale=8.0),
    'masked': lambda: _star_inputs(30, 40, 6, [30, 22, 30], [6, 4, 6], 112, masked=range(30, 40)),
    'empty_target': _empty_target,
    # states_two_trips' S; 40 frames reach no further than 40 labels, so the targets read out are shorter
    'time_major_view': lambda: _star_inputs(40, 70, 70, [40, 33, 40], [35, 20, 7], 113),
}


@functools.lru_cache(maxsize=None)
def star_case(name):
    """Inputs and the float64 / float32 yardsticks of a case, computed once and shared (nothing writes to them)."""
    lp, tg, il, tl, pen, w = STAR[name]()
    wn = w.double().numpy()[None, :, None]
    ref = {}
    for dtype in ('float64', 'float32'):
        losses, grad = L.star_ctc(lp.permute(1, 0, 2), tg, il, tl, pen, dtype)
        ref[dtype] = (losses.astype(np.float64), grad.astype(np.float64) * wn)
    assert np.isfinite(ref['float64'][0]).all() and ref['float64'][0].max() < 1e5, 'the case must be a reachable lattice'
    return (lp, tg, il, tl, pen, w), ref


def run_star(lp, tg, il, tl, pen, w, time_major_copy=True):
    """-> (losses [N], grad [T, N, C]) from the HIP path.  ``time_major_copy``: hand the kernel a contiguous [T, N, C] tensor; otherwise the
    [N, T, C] buffer viewed time-major (what recognizer.py passes)."""
    from haloop_amd import star
    x = (lp.permute(1, 0, 2).contiguous() if time_major_copy else lp.contiguous()).to(DEV).requires_grad_(True)
    em = x if time_major_copy else x.permute(1, 0, 2)
    assert em.is_contiguous() == time_major_copy
    losses = star.star_ctc_forward_score(em, tg.to(DEV), il.to(DEV), tl.to(DEV), star_penalty=pen)
    (losses * w.to(DEV)).sum().backward()
    grad = x.grad if time_major_copy else x.grad.permute(1, 0, 2)
    return losses.detach().cpu().double().numpy(), grad.cpu().double().numpy()


def within(name, what, got, ref, rtol, atol):
    """|got - ref64| <= max(floor, 4 e32) for every element; the figures are printed first."""
    r64, r32 = ref['float64'], ref['float32']
    got, r64, r32 = (np.asarray(a, dtype=np.float64) for a in (got, r64, r32))
    e32 = float(np.abs(r32 - r64).max())
    err = np.abs(got - r64)
    bound = np.maximum(atol + rtol * np.abs(r64), 4 * e32)
    print(f'{name}: {what}  e32 {e32:.3e}  kernel {float(err.max()):.3e}  max|ref| {float(np.abs(r64).max()):.4e}  '
          f'worst err/bound {float((err / bound).max()):.3f}')
    assert np.isfinite(got).all(), f'{name}: {what} not finite'
    assert (err <= bound).all(), f'{name}: {what} off by {float(err.max()):.3e}, allowed max(floor, 4 * {e32:.3e})'


def check_case(name, got, ref):
    within(name, 'losses', got[0], {k: v[0] for k, v in ref.items()}, 1e-5, 1e-4)
    within(name, 'grad', got[1], {k: v[1] for k, v in ref.items()}, 1e-4, 5e-6)


@pytest.mark.parametrize('name', list(STAR))
def test_star_ctc_against_float64(name):
    inputs, ref = star_case(name)
    lp, tg, il, tl, pen, w = inputs
    got = run_star(*inputs, time_major_copy=name != 'time_major_view')
    check_case(name, got, ref)
    for n in range(lp.shape[0]):
        assert not got[1][int(il[n]):, n].any(), 'frames past the emission length carry no gradient'
    if name == 'masked':
        assert np.isinf(lp[:, :, 30:].numpy()).all() and not got[1][:, :, 30:].any(), 'masked symbols: the gradient is exactly 0'
    if name == 'empty_target':
        g = load_golden('g8_star_edges')                                    # the reference's own numbers for the empty targets
        np.testing.assert_allclose(got[0], g[name + '.losses'], rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(got[1], g[name + '.grad'] * w.numpy()[None, :, None], rtol=1e-4, atol=5e-6)


# -------------------------------------------------------------------------------------------------------------- transducer
def _transducer_inputs(T, U1, K, jl, tl, seed, N=2, zeros=False):
    g = torch.Generator().manual_seed(seed)
    joint = (torch.randn(N, T, 1, K, generator=g) + torch.randn(N, 1, U1, K, generator=g)).log_softmax(-1)
    tg = torch.randint(0 if zeros else 1, K, (N, U1 - 1), generator=g)
    if zeros:
        tg[:, ::3] = 0                                                      # the label of these cells is the blank
    w = torch.rand(N, generator=g) + 0.5
    return joint, tg, torch.tensor(jl, dtype=torch.int32), torch.tensor(tl, dtype=torch.int32), w


TRANSDUCER = {
    # U+1 = 300: a second trip over the anti-diagonal in alpha and in beta (u <= U_n); U_n = 299: the whole tail, 256: one cell past a trip
    'diag_two_trips': lambda: _transducer_inputs(12, 300, 4, [12, 7], [299, 256], 201),
    'diag_edge_256': lambda: _transducer_inputs(9, 256, 3, [9, 5], [255, 254], 202),
    'diag_edge_257': lambda: _transducer_inputs(9, 257, 3, [9, 5], [256, 255], 203),
    'long': lambda: _transducer_inputs(1500, 6, 8, [1500, 1], [5, 0], 204),
    'label_is_blank': lambda: _transducer_inputs(10, 8, 5, [10, 6], [7, 4], 205, zeros=True),
}


@functools.lru_cache(maxsize=None)
def transducer_case(name):
    inputs = TRANSDUCER[name]()
    joint, tg, jl, tl, w = inputs
    ref = {}
    for dtype in ('float64', 'float32'):
        losses, grad = L.transducer(joint, tg, jl, tl, dtype, weights=w)
        ref[dtype] = (losses.double().numpy(), grad.double().numpy())
    return inputs, ref


def run_transducer(joint, tg, jl, tl, w):
    from haloop_amd import transducer
    x = joint.to(DEV).requires_grad_(True)
    losses = transducer.transducer_forward_score(x, tg.to(DEV), jl.to(DEV), tl.to(DEV))
    (losses * w.to(DEV)).sum().backward()
    return losses.detach().cpu().numpy(), x.grad.cpu().numpy()


@pytest.mark.parametrize('name', list(TRANSDUCER))
def test_transducer_against_float64(name):
    inputs, ref = transducer_case(name)
    got = run_transducer(*inputs)
    check_case(name, got, ref)
    if name == 'label_is_blank':
        assert (inputs[1] == 0).any()


@functools.lru_cache(maxsize=None)
def fused_case():
    """tests/rnnt_loss_ref.py's case construction (randn logits scaled by 3) at U + 1 = 300, V = 64."""
    inputs = R.make_case(2, 20, 300, 64, [20, 13], [299, 256], 206)
    f, g, tg, fl, tl, w = inputs
    return inputs, {dtype: tuple(a.double().numpy() for a in L.transducer_additive(f, g, tg, fl, tl, dtype, weights=w))
                    for dtype in ('float64', 'float32')}


def test_fused_route_wide_u():
    """transducer_loss (rnnt_joint_fwd / bwd around the lattice at K = 2): tests/test_gpu_rnnt_loss.py stops at U + 1 = 18."""
    from haloop_amd import transducer
    (f, g, tg, fl, tl, w), ref = fused_case()
    fd, gd = f.to(DEV).requires_grad_(True), g.to(DEV).requires_grad_(True)
    losses = transducer.transducer_loss(fd, gd, tg.to(DEV), fl.to(DEV), tl.to(DEV))
    (losses * w.to(DEV)).sum().backward()
    name = 'fused_route_wide_u'
    within(name, 'losses', losses.detach().cpu().numpy(), {k: v[0] for k, v in ref.items()}, 1e-5, 1e-4)
    within(name, 'df', fd.grad.cpu().numpy(), {k: v[1] for k, v in ref.items()}, 1e-4, 5e-6)
    within(name, 'dg', gd.grad.cpu().numpy(), {k: v[2] for k, v in ref.items()}, 1e-4, 5e-6)


# --------------------------------------------------------------------------------------------------------- reproducibility
def test_backward_twice():
    """The transducer gradient has one writer per element: two runs are bit-identical.  The star gradient is NOT asserted bit-identical:
    star_beta_grad_kernel accumulates the occupancies of a frame with atomicAdd into LDS, all 2S+2 blank states into g[0] and every
    occurrence of a label into that label's g[c], from four waves in whatever order they arrive, and fp32 addition does not associate.
    Its two runs must agree to within the yardstick of test_star_ctc_against_float64 (max(floor, 4 e32)), element by element (observed on an
    MI355X: not bit-identical, at most 2.4e-7 apart)."""
    inputs, ref = transducer_case('diag_two_trips')
    l0, g0 = run_transducer(*inputs)
    l1, g1 = run_transducer(*inputs)
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    inputs, ref = star_case('states_two_trips')
    l0, g0 = run_star(*inputs)
    l1, g1 = run_star(*inputs)
    assert np.array_equal(l0, l1), 'the star forward has one writer per state'
    r64, r32 = ref['float64'][1], ref['float32'][1]
    bound = np.maximum(5e-6 + 1e-4 * np.abs(r64), 4 * np.abs(r32 - r64).max())
    print(f'states_two_trips: two backward runs differ by at most {float(np.abs(g0 - g1).max()):.3e}, bit-identical: {np.array_equal(g0, g1)}')
    assert (np.abs(g0 - g1) <= bound).all()
