"""The CTC loss (csrc/ctc.hip) and the fused CTC head (csrc/head.hip) against the float64 yardstick tests/ctc_ref.py (itself held to
float64 torch by tests/test_ctc_ref_cpu.py), at the edges of their kernel choice and of their tiles.  The cases and the dispatch rule
they are chosen from are in tests/ctc_f64_cases.py.

Tolerance, for every comparison.  The kernels are fp32, so a case is allowed what fp32 arithmetic itself loses on it: with
e32 = max|ref(float32) - ref(float64)| (the yardstick's own float32 run on the CPU; separately for losses and gradients, for the head
separately per output and under the same operand model), an element may be off by

    max(floor, 4 * e32)     floor = 1e-5 |loss| + 1e-5 (losses), 1e-5 (log-probs and their gradients),
                                    2e-4 |ref| + 1e-6 + 2e-5 max|ref| (dW, db, dfeats)

The floors are what tests/test_gpu_parity.py and tests/test_gpu_head.py already grant; the 4 is tests/test_gpu_lattice_f64.py's, for
the same reason (another valid order of the same sums, the hardware exp / log of the wave kernels).  It is never taken from the
kernel's own error.

A. ops.ctc_fwd + ops.ctc_bwd with grad_out in [0.5, 1.5], every loss and every gradient element, each case batch-major and as a
   time-major view of a wider buffer; the forward flag variants (ctc.ctc_forward_score1/2/3) against oracle.lattice fed float64.
B. the head on its three routes -- ctc_head_fwd + ctc_head_bwd in the 'f32' mode (exact operands), ctc_head_train in 'bf16x3' and in
   'bf16' (both run the three-term split of ctc_ref.head(split='bf16x3'): see its docstring) -- and ctc_head_greedy on both kernels.

Observed (e32 on the CPU; kernel = max |kernel - float64| on an MI355X), losses / gradients:

    CTC loss                 e32 loss   kernel loss  e32 grad   kernel grad
    wave_full                1.4e-05    1.4e-05      2.0e-05    2.0e-05
    wave_lds_edge            6.6e-04    6.6e-04      1.6e-03    1.6e-03
    general_just_over        1.7e-03    1.7e-03      9.4e-04    9.4e-04
    states_two_trips         1.1e-03    1.1e-03      1.8e-03    1.8e-03
    classes_two_trips        8.5e-06    8.5e-06      1.9e-05    1.9e-05
    classes_wave             4.1e-06    4.1e-06      6.7e-06    6.7e-06
    long_peaked              2.1e-03    2.1e-03      1.6e-02    1.6e-02
    repeats                  1.4e-05    1.4e-05      1.8e-05    1.8e-05
    corners                  1.1e-06    1.1e-06      1.8e-06    1.7e-06
    corners_n1               3.0e-07    3.0e-07      1.7e-06    1.8e-06
    masked                   7.1e-07    7.1e-07      1.9e-06    1.9e-06

    forward flags            score1 e32 / kernel    score2 e32 / kernel    score3 e32 / kernel
    wave_full                1.4e-05 / 1.4e-05    1.4e-05 / 1.4e-05    1.4e-05 / 1.4e-05
    general_just_over        9.0e-04 / 9.0e-04    1.8e-04 / 1.8e-04    1.7e-03 / 1.7e-03

    head, e32 / kernel            nll                lp                 dfeats             dW                 db
    tile_full f32                 1.0e-05 / 1.0e-05  6.5e-07 / 8.6e-07  7.5e-08 / 1.3e-07  1.0e-06 / 1.6e-06  9.0e-07 / 1.6e-06
    tile_full_drop f32            9.6e-06 / 1.7e-05  8.6e-07 / 8.1e-07  1.1e-07 / 1.2e-07  1.6e-06 / 1.3e-06  1.1e-06 / 6.3e-07
    row16 f32                     1.1e-06 / 1.1e-06  5.7e-07 / 6.1e-07  7.2e-08 / 9.2e-08  8.4e-07 / 1.1e-06  4.5e-07 / 5.4e-07
    smallest f32                  4.5e-08 / 7.6e-08  4.5e-08 / 7.9e-08  1.1e-08 / 9.1e-09  4.5e-08 / 3.7e-08  2.0e-08 / 2.0e-08
    odd_tiles f32                 4.1e-06 / 3.6e-06  8.0e-07 / 7.6e-07  6.5e-08 / 6.7e-08  1.3e-06 / 1.2e-06  3.6e-07 / 1.6e-07
    odd_tiles_5 f32               7.0e-06 / 4.8e-06  1.4e-06 / 6.7e-07  8.2e-08 / 3.8e-08  1.7e-06 / 1.3e-06  1.4e-06 / 1.3e-06
    eight_slices f32              3.0e-06 / 6.9e-06  6.2e-07 / 7.1e-07  4.1e-08 / 6.6e-08  1.3e-06 / 2.1e-06  4.6e-07 / 8.1e-07
    one_slice_wide f32            2.2e-06 / 3.9e-06  1.4e-06 / 8.3e-07  1.1e-09 / 1.1e-09  2.5e-07 / 1.3e-07  6.7e-08 / 5.3e-08
    peaked f32                    2.5e-05 / 4.1e-05  2.4e-05 / 1.1e-05  1.3e-05 / 2.5e-05  1.2e-05 / 2.8e-05  8.8e-06 / 1.6e-05
    with_infeasible f32           1.5e-06 / 1.5e-06  3.4e-07 / 5.8e-07  3.2e-07 / 3.1e-07  -                  -
    tile_full bf16x3 = bf16       1.0e-05 / 1.0e-05  5.4e-07 / 6.6e-07  1.5e-07 / 9.1e-08  2.1e-06 / 1.3e-06  1.9e-06 / 1.2e-06
    tile_full_drop bf16x3 = bf16  1.4e-05 / 1.3e-05  7.6e-07 / 7.4e-07  2.2e-07 / 1.6e-07  3.0e-06 / 1.7e-06  1.9e-06 / 5.5e-07
    row16 bf16x3 = bf16           5.0e-06 / 5.0e-06  5.1e-07 / 3.6e-07  1.6e-07 / 2.6e-07  2.7e-06 / 3.3e-06  1.8e-06 / 1.8e-06
    smallest bf16x3 = bf16        9.2e-08 / 3.2e-08  9.2e-08 / 3.2e-08  3.7e-09 / 3.7e-09  1.5e-08 / 1.5e-08  1.3e-08 / 1.3e-08
    odd_tiles bf16x3 = bf16       1.6e-06 / 2.2e-06  6.1e-07 / 6.7e-07  1.8e-07 / 1.8e-07  2.9e-06 / 5.3e-06  1.8e-06 / 4.4e-06
    odd_tiles_5 bf16x3 = bf16     6.3e-06 / 2.5e-06  6.2e-07 / 6.1e-07  7.6e-08 / 8.4e-08  1.8e-06 / 2.0e-06  1.3e-06 / 1.3e-06
    eight_slices bf16x3 = bf16    6.3e-06 / 5.1e-06  6.5e-07 / 6.4e-07  7.7e-08 / 7.4e-08  3.4e-06 / 2.8e-06  1.5e-06 / 1.4e-06
    one_slice_wide bf16x3 = bf16  2.8e-06 / 2.8e-06  6.8e-07 / 8.5e-07  3.4e-09 / 3.5e-09  3.0e-07 / 2.5e-07  2.1e-07 / 2.9e-08
    peaked bf16x3 = bf16          5.3e-05 / 2.2e-05  1.5e-05 / 9.6e-06  1.6e-05 / 1.6e-05  9.0e-06 / 1.5e-05  4.9e-06 / 1.5e-05
    with_infeasible bf16x3 = bf16 3.0e-06 / 1.0e-05  3.8e-07 / 3.8e-07  5.7e-07 / 6.0e-07  -                  -

    greedy, e32 / kernel     lp                 scores
    tile_full greedy f32     6.5e-07 / 8.6e-07  3.1e-07 / 3.9e-07
    tile_full greedy bf16x3  5.4e-07 / 6.6e-07  2.6e-07 / 3.9e-07
    smallest greedy f32      4.5e-08 / 7.9e-08  4.5e-08 / 7.6e-08
    smallest greedy bf16x3   9.2e-08 / 8.7e-08  9.2e-08 / 8.7e-08
    row16 greedy f32         5.5e-07 / 4.7e-07  1.6e-07 / 2.1e-07
    row16 greedy bf16x3      5.2e-07 / 4.8e-07  3.2e-07 / 2.5e-07

(The 'bf16' math mode runs the same kernel and the same split as 'bf16x3': its figures are the same to every printed digit.  The time-major
view gives the figures of the batch-major run.  with_infeasible: dW / db are not compared, loss is not finite.)
"""
import functools

import numpy as np
import pytest
import torch

import ctc_f64_cases as K
import ctc_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def within(name, what, got, r64, r32, rtol, atol, where=None):
    """|got - ref64| <= max(atol + rtol |ref64|, 4 e32) for every element (of ``where``); the figures are printed first."""
    got, r64, r32 = (np.asarray(a, dtype=np.float64) for a in (got, r64, r32))
    if where is not None:
        got, r64, r32 = got[where], r64[where], r32[where]
    if got.size == 0:
        return
    assert np.isfinite(r64).all() and np.isfinite(r32).all(), f'{name}: {what}: the yardstick is not finite here'
    e32 = float(np.abs(r32 - r64).max())
    err = np.abs(got - r64)
    bound = np.maximum(atol + rtol * np.abs(r64), 4 * e32)
    print(f'{name}: {what}  e32 {e32:.1e}  kernel {float(np.nanmax(err)):.1e}  max|ref| {float(np.abs(r64).max()):.4e}  '
          f'worst err/bound {float(np.nanmax(err / bound)):.3f}')
    assert np.isfinite(got).all(), f'{name}: {what} not finite'
    assert (err <= bound).all(), f'{name}: {what} off by {float(err.max()):.3e}, allowed max(floor, 4 * {e32:.3e})'


def wide(name, what, got, r64, r32, where=None):
    """The floor of dW, db, dfeats: 2e-4 |ref| + 1e-6 + 2e-5 max|ref| (tests/test_gpu_head.py)."""
    ref = np.asarray(r64, dtype=np.float64)
    ref = ref[where] if where is not None else ref
    within(name, what, got, r64, r32, 2e-4, 1e-6 + 2e-5 * float(np.abs(ref).max(initial=0)), where)


# ------------------------------------------------------------------------------------------------------------ A. the CTC loss
@functools.lru_cache(maxsize=None)
def ctc_case(name):
    """Inputs and the float64 / float32 yardsticks of a case, computed once and shared (nothing writes to them)."""
    c = K.CTC[name][0]()
    ref = {dt: ctc_ref.ctc(c['lp'].numpy(), c['tg'], c['il'], c['tl'], dt) for dt in ('float64', 'float32')}
    return c, ref


def run_ctc(c, time_major_view):
    """-> (nll [N], grad [N,T,C]) from halo_ctc_fwd / halo_ctc_bwd; ``time_major_view``: the log-probs as the first C columns of a
    [T, N, C + 3] buffer (row strides that are not the packed ones)."""
    from haloop_amd import ops
    lp = c['lp']
    N, T, C = lp.shape
    if time_major_view:
        buf = torch.full((T, N, C + 3), float('nan'), device=DEV)
        buf[:, :, :C] = lp.permute(1, 0, 2).to(DEV)
        x = buf[:, :, :C]
        assert not x.is_contiguous()
    else:
        x = lp.contiguous().to(DEV)
    nll, alpha, saved = ops.ctc_fwd(x, time_major_view, c['tg'].to(DEV), c['il'].to(DEV), c['tl'].to(DEV))
    grad = ops.ctc_bwd(x, time_major_view, saved, alpha, nll, c['w'].to(DEV))
    if time_major_view:
        grad = grad.permute(1, 0, 2)
    return nll.cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize('time_major_view', [False, True], ids=['batch_major', 'time_major_view'])
@pytest.mark.parametrize('name', list(K.CTC))
def test_ctc_against_float64(name, time_major_view):
    c, ref = ctc_case(name)
    assert K.ctc_paths(*K.CTC[name][1]) == K.CTC[name][2], 'the case no longer reaches the kernels it was chosen for'
    assert tuple(c['lp'].shape[1:]) == K.CTC[name][1][:2] and c['tg'].shape[1] == K.CTC[name][1][2]
    nll, grad = run_ctc(c, time_major_view)
    (n64, g64), (n32, g32) = ref['float64'], ref['float32']
    fin = np.isfinite(n64)
    assert np.array_equal(np.isfinite(n32), fin)
    assert (nll[~fin] == np.inf).all(), 'an infeasible row: nll = +inf exactly'
    within(name, 'losses', nll, n64, n32, 1e-5, 1e-5, where=fin)
    w = c['w'].double().numpy()[:, None, None]
    ok = np.isfinite(c['lp'].numpy()) & fin[:, None, None]          # infeasible rows and lp = -inf entries are unconstrained
    within(name, 'grad', grad, g64 * w, g32.astype(np.float64) * w, 0.0, 1e-5, where=ok)
    for n in range(len(nll)):
        assert not grad[n, int(c['il'][n]):].any(), 'frames at and beyond il carry no gradient'
    if name == 'corners':
        assert list(fin) == [True, True, True, True, False, True]
    if name == 'masked':
        assert (~np.isfinite(c['lp'].numpy())).any() and fin.all()


def _flag_inputs(name):
    c, _ = ctc_case(name)
    return c['lp'].permute(1, 0, 2).contiguous(), c['tg'], c['il'], c['tl']           # emissions [T, N, C]


@functools.lru_cache(maxsize=None)
def flag_reference(name):
    """oracle.lattice (torch on the CPU; it computes in the dtype of its input) in float64 and float32: score1 / score2 of utterance 0
    over all T frames and S labels, score3 of the batch."""
    from oracle import lattice
    em, tg, il, tl = _flag_inputs(name)
    out = {}
    for dt in (torch.float64, torch.float32):
        e = em.to(dt)
        out[dt] = dict(score1=lattice.ctc_forward_score1(e[:, 0], tg[0]).reshape(1).double().numpy(),
                       score2=lattice.ctc_forward_score2(e[:, 0], tg[0]).reshape(1).double().numpy(),
                       score3=lattice.ctc_forward_score3(e, tg, il, tl).double().numpy())
        assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in out[dt].values())
    return out


@pytest.mark.parametrize('name', ['wave_full', 'general_just_over'])
def test_ctc_flag_variants_against_float64(name):
    """The full-lattice, finite-min, no-lead-blank-loop and wrap-skip flags of halo_ctc_fwd, through ctc.ctc_forward_score1/2/3, on the
    single-wave and on the general kernel."""
    from haloop_amd import ctc
    assert K.ctc_paths(*K.CTC[name][1])[0] == ('wave' if name == 'wave_full' else 'general')
    em, tg, il, tl = _flag_inputs(name)
    ref = flag_reference(name)
    e = em.to(DEV)
    got = dict(score1=ctc.ctc_forward_score1(e[:, 0], tg[0].to(DEV)).reshape(1), score2=ctc.ctc_forward_score2(e[:, 0], tg[0].to(DEV)).reshape(1),
               score3=ctc.ctc_forward_score3(e, tg.to(DEV), il.to(DEV), tl.to(DEV)))
    for k, v in got.items():
        within(name, k, v.cpu().numpy(), ref[torch.float64][k], ref[torch.float32][k], 1e-5, 1e-5)


# ------------------------------------------------------------------------------------------------------------------ B. the head
@functools.lru_cache(maxsize=None)
def head_case(name, split):
    c = K.HEAD[name][0]()
    mask = K.head_mask(c)
    args = (c['feats'].numpy(), c['W'].numpy(), c['b'].numpy(), mask, c['il'].numpy(), c['tg'].numpy(), c['tl'].numpy())
    ref = {dt: ctc_ref.head(*args, dtype=dt, split=split) for dt in ('float64', 'float32')}
    return c, ref


def check_head(name, got, ref):
    """got: dict(flen, lp, nll, loss, dW, db, dfeats) of numpy arrays from a HIP route."""
    r64, r32 = ref['float64'], ref['float32']
    assert np.array_equal(got['flen'], r64['flen'])
    fin = np.isfinite(r64['nll'])
    assert np.array_equal(np.isfinite(r32['nll']), fin)
    within(name, 'lp', got['lp'], r64['lp'], r32['lp'], 0.0, 1e-5)
    assert (got['nll'][~fin] == np.inf).all()
    within(name, 'nll', got['nll'], r64['nll'], r32['nll'], 1e-5, 1e-5, where=fin)
    wide(name, 'dfeats', got['dfeats'], r64['dfeats'], r32['dfeats'], where=np.broadcast_to(fin[:, None, None], r64['dfeats'].shape))
    if fin.all():
        within(name, 'loss', got['loss'], r64['loss'], r32['loss'], 1e-5, 1e-5)
        wide(name, 'dW', got['dW'], r64['dW'], r32['dW'])
        wide(name, 'db', got['db'], r64['db'], r32['db'])
    else:
        assert name.startswith('with_infeasible') and not np.isfinite(got['loss'])      # dW / db: F.ctc_loss itself gives NaN there


def _device_inputs(c):
    from haloop_amd import ops
    drop = ops.Dropout(c['p'], K.SEED, K.OFFSET) if c['p'] > 0 else ops.NO_DROPOUT
    return [c[k].to(DEV) for k in ('feats', 'W', 'b', 'il', 'tg', 'tl')] + [drop]


@pytest.mark.parametrize('name', list(K.HEAD))
def test_head_two_launches_against_float64(name):
    """halo_ctc_head_fwd + halo_ctc_head_bwd in the exact-f32 mode against the yardstick with exact operands."""
    from haloop_amd import _lib, ops
    _lib.lib(); _lib.lend_scratch()
    c, ref = head_case(name, None)
    B, T, H, V, S, p = K.HEAD[name][1]
    assert tuple(c['feats'].shape) == (B, T, H) and tuple(c['W'].shape) == (V, H) and c['tg'].shape[1] == S and ops.ctc_head_supported(T, H, V, S)
    feats, W, b, il, tg, tl, drop = _device_inputs(c)
    prev = _lib.get_math_mode()
    _lib.set_math_mode('f32')
    try:
        loss = torch.full((), -1.0, device=DEV)
        ticket = torch.zeros(1, device=DEV, dtype=torch.int32)
        dW, db = torch.empty_like(W), torch.empty_like(b)
        for rep in range(2):
            lp, alpha, nll, flen, grad_out, (tg64, tl64) = ops.ctc_head_fwd(feats, W, b, drop, K.STREAM, il, tg, tl, loss, ticket)
            dfeats = ops.ctc_head_bwd(feats, W, drop, K.STREAM, flen, tg64, tl64, lp, alpha, nll, grad_out, dW, db)
            assert int(ticket.item()) == 0, 'the loss ticket is back at zero'
            got = dict(flen=flen, lp=lp, nll=nll, loss=loss, dW=dW, db=db, dfeats=dfeats)
            check_head(f'{name} f32 run {rep}', {k: v.cpu().numpy() for k, v in got.items()}, ref)
    finally:
        _lib.set_math_mode(prev)


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('name', list(K.HEAD))
def test_head_one_launch_against_float64(name, mode):
    """halo_ctc_head_train against the yardstick under the three-term bf16 split that kernel applies in both modes."""
    from haloop_amd import _lib, ops
    _lib.lib(); _lib.lend_scratch()
    c, ref = head_case(name, 'bf16x3')
    B, T, H, V, S, p = K.HEAD[name][1]
    feats, W, b, il, tg, tl, drop = _device_inputs(c)
    prev = _lib.get_math_mode()
    _lib.set_math_mode(mode)
    try:
        ticket = ops.ctc_head_train_ticket(B, H, DEV)
        want_slices = K.HEAD[name][2]
        slices = (ticket.numel() - 2) // (B * 2048) if ticket.numel() > 2 else 1
        if slices != want_slices:
            pytest.skip(f'this device slices B = {B}, H = {H} {slices} ways; the case is built for {want_slices} (a 256-CU MI355X)')
        loss = torch.full((), -1.0, device=DEV)
        dW, db = torch.empty_like(W), torch.empty_like(b)
        for rep in range(2):
            dfeats, nll, flen, lp = ops.ctc_head_train(feats, W, b, drop, K.STREAM, il, tg, tl, loss, ticket, dW, db, want_lp=True)
            assert ticket[:2].tolist() == [0, rep + 1], 'the loss ticket back at zero, the launches counted'
            got = dict(flen=flen, lp=lp, nll=nll, loss=loss, dW=dW, db=db, dfeats=dfeats)
            check_head(f'{name} {mode} run {rep}', {k: v.cpu().numpy() for k, v in got.items()}, ref)
    finally:
        _lib.set_math_mode(prev)


def test_head_one_launch_refuses_a_slice_wider_than_2048():
    """B = 300 utterances are more than half of any gfx950's CUs, so H = 2112 stays one slice of 2112 columns: not supported, no result."""
    from haloop_amd import _lib, ops
    _lib.lib()
    B, T, H, V = 300, 1, 2112, 2
    assert ops.ctc_head_supported(T, H, V, 1)
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16x3')
    try:
        ticket = ops.ctc_head_train_ticket(B, H, DEV)
        assert ticket.numel() == 2, 'one slice per utterance'
        feats, W, b = torch.zeros(B, T, H, device=DEV), torch.zeros(V, H, device=DEV), torch.zeros(V, device=DEV)
        il, tg, tl = (torch.ones(B, dtype=torch.int64, device=DEV), torch.ones(B, 1, dtype=torch.int64, device=DEV),
                      torch.ones(B, dtype=torch.int64, device=DEV))
        loss = torch.full((), -1.0, device=DEV)
        dW, db = torch.full_like(W, -1.0), torch.full_like(b, -1.0)
        with pytest.raises(_lib.HaloError, match=r'\(-95\)'):                # HALO_ENOTSUP (include/halo.h)
            ops.ctc_head_train(feats, W, b, ops.NO_DROPOUT, K.STREAM, il, tg, tl, loss, ticket, dW, db)
        assert loss.item() == -1.0 and (dW == -1.0).all() and ticket.tolist() == [0, 0], 'nothing ran'
    finally:
        _lib.set_math_mode(prev)


@pytest.mark.parametrize('mode', ['f32', 'bf16x3'])
@pytest.mark.parametrize('name', K.GREEDY)
def test_head_greedy_against_float64(name, mode):
    """halo_ctc_head_greedy on ctc_head_fwd_kernel<true> ('f32') and on ctc_head_greedy2_kernel (every other mode): log-probs to the
    tolerance above; alignments, hypotheses and lengths exactly ctc_ref.greedy's for every utterance whose frames all have a float64
    top-two margin above 8 e32(lp) -- with these seeds all of them (tests/test_ctc_ref_cpu.py asserts the cap of 2 % on the CPU)."""
    from haloop_amd import _lib, ops
    _lib.lib()
    c, ref = head_case(name, None if mode == 'f32' else 'bf16x3')
    lp64, lp32 = ref['float64']['lp'], ref['float32']['lp']
    # the greedy launch has no dropout: the case's reference is reused only where the case has none, else computed without the mask
    if c['p'] > 0:
        args = (c['feats'].numpy(), c['W'].numpy(), c['b'].numpy(), None, c['il'].numpy(), c['tg'].numpy(), c['tl'].numpy())
        lp64, lp32 = (ctc_ref.head(*args, dtype=dt, split=None if mode == 'f32' else 'bf16x3')['lp'] for dt in ('float64', 'float32'))
    e32 = float(np.abs(lp32.astype(np.float64) - lp64).max())
    clear = ctc_ref.top_two_margin(lp64) > 8 * e32
    assert (~clear).mean() <= 0.02
    ali64, scores64, hyp64, len64 = ctc_ref.greedy(lp64)
    feats, W, b = (c[k].to(DEV) for k in ('feats', 'W', 'b'))
    prev = _lib.get_math_mode()
    _lib.set_math_mode(mode)
    try:
        ali, scores, hyp, hyp_len, lp = (t.cpu().numpy() for t in ops.ctc_head_greedy(feats, W, b, want_lp=True))
    finally:
        _lib.set_math_mode(prev)
    within(f'{name} greedy {mode}', 'lp', lp, lp64, lp32, 0.0, 1e-5)
    within(f'{name} greedy {mode}', 'scores', scores, scores64, ctc_ref.greedy(lp32)[1], 0.0, 1e-5)
    for n in np.flatnonzero(clear):
        assert np.array_equal(ali[n], ali64[n]), n
        assert hyp_len[n] == len64[n] and hyp[n, :len64[n]].tolist() == hyp64[n] and not hyp[n, len64[n]:].any(), n
