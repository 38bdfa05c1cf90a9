"""The tiled attention kernels (csrc/attn.hip, attn_mx.hip, attn_b16.hip) against the float64 reference of tests/attention_ref.py, where the
rest of the suite does not reach: dropout on the probabilities beyond one key tile and one query tile, and the softmax reference point
moving after the first tile.  tests/test_attention_ref_cpu.py holds the CPU side: the reference itself, the teeth of the gates below, the
re-reference counts of the peaked inputs and the probe algebra.

A. Mask probes.  q = 0 makes the probabilities uniform; one-hot v / k / dy make single dropout multipliers come out as single elements
   of y (forward), dq (dQ sweep) and dv (dK/dV sweep).  Thresholded at half the kept value they must EQUAL oracle.philox's multipliers on
   every visible (query, key), in every mode and in every forced form of the backward -- sharp in bf16 as well.
B. Unit-scale randn operands with dropout against the reference with the same multipliers.  Gates (attention_ref.fwd_gate / lse_gate /
   bwd_gate): f32 and bf16x3 the project's gates for such operands times 1 / (1 - p); bf16 against the reference on the operands as the
   single-pass kernels round them, forward 2^-8 max|v| / (1 - p) (2^-9 per probability, a factor two), backward the project's 1e-1 times
   1 / (1 - p) -- test_attention_ref_cpu.py shows that every wrong dropout index moves y, dq, dk and dv past these gates, each on its own.
C. Peaked scores (attention_ref.peaked_inputs), no dropout: every 16-query block re-references on later tiles with half of its lanes
   moving ('ramp', 'spike'), or the later tiles underflow ('descend').  Errors relative to max|reference| of the tensor; f32 / bf16x3
   gates are the project's times max(1, A / A0), A = max scale * sum_d |q_d k_d| of the peaked input and A0 of its randn baseline (the
   score error grows with that sum at a fixed operand precision); bf16 and attn_b16 use the gates of B at p = 0.

Measured on an MI355X: the largest error over the cases of each row, and in brackets the largest share of a gate that any element used
(each test prints its figures on lines beginning with ATTNERR):
    section   mode     y                lse              dq               dk               dv
    B         f32      8.38e-07 (0.12)  7.66e-07 (0.02)  1.74e-06 (0.04)  2.64e-06 (0.06)  3.13e-06 (0.05)
    B         bf16x3   2.61e-05 (0.50)  1.05e-05 (0.09)  4.56e-05 (0.29)  7.26e-05 (0.42)  7.21e-05 (0.35)
    B         bf16     8.17e-03 (0.38)  8.45e-07 (0.02)  2.09e-02 (0.19)  3.88e-02 (0.35)  4.47e-02 (0.36)
    C         f32      2.92e-06 (0.27)  2.81e-07 (0.00)  3.70e-06 (0.04)  1.99e-06 (0.02)  1.48e-06 (0.02)
    C         bf16x3   2.29e-05 (0.22)  3.80e-06 (0.01)  6.67e-05 (0.14)  6.49e-05 (0.14)  4.78e-05 (0.10)
    C         bf16     2.94e-03 (0.17)  1.16e-07 (0.00)  3.09e-02 (0.31)  2.57e-02 (0.26)  3.60e-02 (0.36)
    C attn_b16 bf16    2.99e-03 (0.17)  1.09e-07 (0.00)  1.87e-02 (0.19)  1.26e-02 (0.13)  1.51e-02 (0.15)
B: absolute errors; C: relative to max|reference| (y in bf16 mode and attn_b16: absolute).  No gate needed a margin beyond those derived
above.  A: every multiplier of every probe equal.
"""
import functools

import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops
    _lib.lib()
    return dict(ops=ops, lib=_lib)


@pytest.fixture
def math_mode(request, hal):
    prev = hal['lib'].get_math_mode()
    hal['lib'].set_math_mode(request.param)
    yield request.param
    hal['lib'].set_math_mode(prev)


def _set_form(monkeypatch, qb, lf):
    """The backward's dispatch switches (read per call); None leaves the default rule in charge."""
    for name, val in (('HALO_ATTN_BWD_QB', qb), ('HALO_ATTN_DKV_LF', lf)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _forms(modes=R.MODES):
    return [pytest.param(m, qb, lf, id='%s-qb%s-lf%s' % (m, qb or 'x', lf or 'x')) for m in modes for qb, lf in R.BWD_FORMS[m]]


MODE_PARAM = pytest.mark.parametrize('math_mode', R.MODES, indirect=True)
FORM_PARAM = pytest.mark.parametrize('math_mode,qb,lf', _forms(), indirect=['math_mode'])


def _lens_dev(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def _forward(ops, q, k, v, N, heads, hd, Tq, Tk, causal, lens, drop, stream_id):
    y, lse, _ = ops.attention_fwd(q, k, v, N, heads, hd, Tq, Tk, causal=causal, key_lengths=_lens_dev(lens), want_lse=True, drop=drop,
                                  stream_id=stream_id)
    return y, lse


def _backward(ops, q, k, v, y, dy, lse, N, heads, hd, Tq, Tk, causal, lens, drop, stream_id):
    """dq, dk, dv written into NaN-filled buffers (dk | dv packed, as the models hold them)."""
    C = heads * hd
    dq = torch.full_like(q, float('nan'))
    dkv = torch.full((N * Tk, 2 * C), float('nan'), device=DEV)
    ops.attention_bwd(q, k, v, y, dy, lse, dq, dkv[:, :C], dkv[:, C:], N, heads, hd, Tq, Tk, causal=causal, key_lengths=_lens_dev(lens),
                      drop=drop, stream_id=stream_id)
    return dq, dkv[:, :C], dkv[:, C:]


def _report(tag, name, got, ref, atol, rtol=0.0, relative_to=None):
    """Prints the measured error and its share of the gate, then asserts.  relative_to: errors as a fraction of this scale."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), (tag, name)
    scale = 1.0 if relative_to is None else relative_to
    err = np.abs(got - ref) / scale
    bound = atol + rtol * np.abs(ref) / scale
    print('ATTNERR %s %s err %.3e gate %.3e share %.3f' % (tag, name, err.max(), atol, (err / bound).max()))
    assert (err <= bound).all(), (tag, name, float(err.max()), atol)


# ------------------------------------------------------------------------------------------------------------------- A. mask probes
@functools.lru_cache(maxsize=None)
def _probe_mult(N, heads, Tq, Tk, offset):
    return R.drop_mult(N, heads, Tq, Tk, R.PROBE_P, R.SEED, R.STREAM_ID, offset)


def _run_probe(ops, which, case, drop, want_offset):
    N, heads, Tq, Tk, causal, lens = case
    want = _probe_mult(N, heads, Tq, Tk, want_offset)
    est = np.full(want.shape, np.nan, dtype=np.float32)
    for tile in R.probe_tiles(which, Tq, Tk):                     # one launch per tile
        q, k, v, dy = (t.to(DEV) for t in R.probe_inputs(which, N, heads, Tq, Tk, tile))
        y, lse = _forward(ops, q, k, v, N, heads, R.PROBE_HD, Tq, Tk, causal, lens, drop, R.STREAM_ID)
        out = y
        if which != 'fwd':
            dq, dk, dv = _backward(ops, q, k, v, y, dy, lse, N, heads, R.PROBE_HD, Tq, Tk, causal, lens, drop, R.STREAM_ID)
            out = dq if which == 'dq' else dv
        R.probe_decode(which, out.cpu(), y.cpu(), N, heads, Tq, Tk, causal, lens, R.PROBE_P, tile, est)
    vis = np.broadcast_to(R.visible(N, Tq, Tk, causal, lens).numpy(), want.shape)
    np.testing.assert_array_equal(est[vis], want[vis])


PROBE_CASE_PARAM = pytest.mark.parametrize('case', R.PROBE_CASES, ids=lambda c: '%dx%d' % (c[2], c[3]))


@PROBE_CASE_PARAM
@MODE_PARAM
def test_forward_draws_the_oracle_multipliers_on_every_tile(hal, math_mode, case):
    _run_probe(hal['ops'], 'fwd', case, hal['ops'].Dropout(R.PROBE_P, R.SEED, R.OFFSET), R.OFFSET)


@pytest.mark.parametrize('which', ['dq', 'dkv'])
@PROBE_CASE_PARAM
@FORM_PARAM
def test_backward_sweeps_draw_the_oracle_multipliers_on_every_tile(hal, monkeypatch, math_mode, qb, lf, case, which):
    _set_form(monkeypatch, qb, lf)
    _run_probe(hal['ops'], which, case, hal['ops'].Dropout(R.PROBE_P, R.SEED, R.OFFSET), R.OFFSET)


@pytest.mark.parametrize('which', ['fwd', 'dq', 'dkv'])
@MODE_PARAM
def test_attention_dropout_adds_the_device_step_counter(hal, math_mode, which):
    """Dropout(offset=3, counter=[5]) draws the multipliers of offset 8 (graph replays advance the counter, not the argument)."""
    counter = torch.tensor([5], dtype=torch.int32, device=DEV)
    _run_probe(hal['ops'], which, R.PROBE_CASES[1], hal['ops'].Dropout(R.PROBE_P, R.SEED, 3, counter=counter), 8)
    assert counter.item() == 5


# ------------------------------------------------------------------------------------- B. random data with dropout against the reference
@functools.lru_cache(maxsize=None)
def _drop_reference(case, p, rounded):
    """(inputs, y, lse, dq, dk, dv) of a dropout case: float64 on the CPU, computed once per (case, p, operand rounding)."""
    hd, heads, N, Tq, Tk, causal, lens = case
    q, k, v, dy = R.case_inputs(hd, heads, N, Tq, Tk)
    mult = R.drop_mult(N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET)
    qr, kr, vr, dyr, l2 = R.reference_operands('bf16' if rounded else 'f32', hd, q, k, v, dy)
    y, lse = R.attention_ref(qr, kr, vr, N, heads, hd, Tq, Tk, causal, lens, mult, l2)
    grads = R.attention_grads_ref(qr, kr, vr, N, heads, hd, Tq, Tk, causal, lens, dyr, mult, l2)
    return (q, k, v, dy), float(torch.as_tensor(vr).abs().max()), y.numpy(), lse.numpy(), tuple(g.numpy() for g in grads)


def _case_id(c):
    return 'hd%d-%dx%d' % (c[0], c[3], c[4])


def _check_forward(tag, mode, hd, p, vmax, y, lse, y_ref, lse_ref):
    _report(tag, 'y', y.cpu(), y_ref, *R.fwd_gate(mode, hd, p, vmax))
    _report(tag, 'lse', lse.cpu(), lse_ref, *R.lse_gate(mode, hd))


def _check_backward(tag, mode, hd, p, got, ref):
    for name, g, r in zip(('dq', 'dk', 'dv'), got, ref):
        _report(tag, name, g.float().cpu(), r, *R.bwd_gate(mode, hd, p))


@pytest.mark.parametrize('p', R.DROPOUT_PS)
@pytest.mark.parametrize('case', R.DROPOUT_CASES, ids=_case_id)
@MODE_PARAM
def test_dropout_forward_against_float64(hal, math_mode, case, p):
    hd, heads, N, Tq, Tk, causal, lens = case
    inputs, vmax, y_ref, lse_ref, _ = _drop_reference(case, p, R.kernel_class(math_mode, hd) == 'bf16')
    q, k, v, _ = (t.to(DEV) for t in inputs)
    y, lse = _forward(hal['ops'], q, k, v, N, heads, hd, Tq, Tk, causal, lens, hal['ops'].Dropout(p, R.SEED, R.OFFSET), R.STREAM_ID)
    _check_forward('B %s %s p%.1f' % (math_mode, _case_id(case), p), math_mode, hd, p, vmax, y, lse, y_ref, lse_ref)


def _backward_cases():
    """Every form of every mode on the matrix-core shapes; head dimension 16 runs the exact-f32 kernels, which have one form."""
    return [pytest.param(m, qb, lf, case, id='%s-qb%s-lf%s-%s' % (m, qb or 'x', lf or 'x', _case_id(case)))
            for m in R.MODES for case in R.DROPOUT_CASES for qb, lf in (R.BWD_FORMS[m] if case[0] != 16 else R.BWD_FORMS[m][:1])]


@pytest.mark.parametrize('p', R.DROPOUT_PS)
@pytest.mark.parametrize('math_mode,qb,lf,case', _backward_cases(), indirect=['math_mode'])
def test_dropout_backward_against_float64(hal, monkeypatch, math_mode, qb, lf, case, p):
    hd, heads, N, Tq, Tk, causal, lens = case
    _set_form(monkeypatch, qb, lf)
    ops = hal['ops']
    inputs, _, _, _, grads_ref = _drop_reference(case, p, R.kernel_class(math_mode, hd) == 'bf16')
    q, k, v, dy = (t.to(DEV) for t in inputs)
    drop = ops.Dropout(p, R.SEED, R.OFFSET)
    y, lse = _forward(ops, q, k, v, N, heads, hd, Tq, Tk, causal, lens, drop, R.STREAM_ID)
    got = _backward(ops, q, k, v, y, dy, lse, N, heads, hd, Tq, Tk, causal, lens, drop, R.STREAM_ID)
    _check_backward('B %s qb%s lf%s %s p%.1f' % (math_mode, qb, lf, _case_id(case), p), math_mode, hd, p, got, grads_ref)


def _one_bf16_rounding(b16, f32):
    """|bf16 - fp32| <= 2^-8 |fp32| (a normal number moves by less than one unit of its 8-bit significand)."""
    b, f = b16.float(), f32.float()
    assert torch.isfinite(b).all()
    return bool(((b - f).abs() <= 2.0 ** -8 * f.abs() + 1e-37).all())


@pytest.mark.parametrize('p', R.DROPOUT_PS)
@pytest.mark.parametrize('math_mode,qb,lf', _forms(('bf16x3', 'bf16')), indirect=['math_mode'])
def test_dropout_bf16_outputs_against_float64(hal, monkeypatch, math_mode, qb, lf, p):
    """attention_fwd_bf16 / attention_bwd_bf16 (the outputs also / instead as row-major bf16) on the first shape."""
    case = R.DROPOUT_CASES[0]
    hd, heads, N, Tq, Tk, causal, lens = case
    C = heads * hd
    _set_form(monkeypatch, qb, lf)
    ops = hal['ops']
    inputs, vmax, y_ref, lse_ref, grads_ref = _drop_reference(case, p, math_mode == 'bf16')
    q, k, v, dy = (t.to(DEV) for t in inputs)
    drop = ops.Dropout(p, R.SEED, R.OFFSET)
    tag = 'B-bf16out %s qb%s lf%s p%.1f' % (math_mode, qb, lf, p)
    y, lse, yb = ops.attention_fwd_bf16(q, k, v, N, heads, hd, Tq, Tk, causal=causal, drop=drop, stream_id=R.STREAM_ID)
    _check_forward(tag, math_mode, hd, p, vmax, y, lse, y_ref, lse_ref)
    assert _one_bf16_rounding(yb, y)
    d = torch.full((N * Tq, 3 * C), float('nan'), device=DEV, dtype=torch.bfloat16)
    ops.attention_bwd_bf16(q, k, v, y, dy, lse, d[:, :C], d[:, C:2 * C], d[:, 2 * C:], N, heads, hd, Tq, Tk, causal=causal, drop=drop,
                           stream_id=R.STREAM_ID)
    f32 = _backward(ops, q, k, v, y, dy, lse, N, heads, hd, Tq, Tk, causal, lens, drop, R.STREAM_ID)
    _check_backward(tag, math_mode, hd, p, f32, grads_ref)
    for i, (name, g32) in enumerate(zip(('dq', 'dk', 'dv'), f32)):
        assert _one_bf16_rounding(d[:, i * C:(i + 1) * C], g32), name


@pytest.fixture(scope='module')
def big_reference():
    """The 257-token case: multipliers (19 x 9 x 257 x 5 tiles x 64 Philox elements) and float64 reference, once per module."""
    hd, heads, N, Tq, Tk, causal, lens = R.BIG_CASE
    q, k, v, dy = R.case_inputs(hd, heads, N, Tq, Tk)
    mult = R.drop_mult(N, heads, Tq, Tk, R.BIG_P, R.SEED, R.STREAM_ID, R.OFFSET)
    qr, kr, vr, dyr, l2 = R.reference_operands('bf16', hd, q, k, v, dy)
    y, lse = R.attention_ref(qr, kr, vr, N, heads, hd, Tq, Tk, causal, lens, mult, l2)
    grads = R.attention_grads_ref(qr, kr, vr, N, heads, hd, Tq, Tk, causal, lens, dyr, mult, l2)
    return (q, k, v, dy), float(vr.abs().max()), y.numpy(), lse.numpy(), tuple(g.numpy() for g in grads)


@pytest.mark.parametrize('math_mode', ['bf16'], indirect=True)
def test_dropout_on_the_default_dispatch_with_two_query_blocks(hal, monkeypatch, math_mode, big_reference):
    """hd 32, 9 heads, N = 19, T = 257, causal, p = 0.1 in bf16 mode: T >= 256 and ceil(T / 128) * heads * N = 513 >= 512 workgroups, so the
    launchers' own rules pick the two-query-block forward and dQ sweep (and the paired dK/dV sweep) -- no switch is set."""
    for name in ('HALO_ATTN_BWD_QB', 'HALO_ATTN_DKV_LF'):
        monkeypatch.delenv(name, raising=False)
    hd, heads, N, Tq, Tk, causal, lens = R.BIG_CASE
    assert Tq >= 256 and (Tq + 127) // 128 * heads * N >= 512
    ops = hal['ops']
    inputs, vmax, y_ref, lse_ref, grads_ref = big_reference
    q, k, v, dy = (t.to(DEV) for t in inputs)
    drop = ops.Dropout(R.BIG_P, R.SEED, R.OFFSET)
    y, lse = _forward(ops, q, k, v, N, heads, hd, Tq, Tk, causal, lens, drop, R.STREAM_ID)
    _check_forward('B-big bf16', 'bf16', hd, R.BIG_P, vmax, y, lse, y_ref, lse_ref)
    got = _backward(ops, q, k, v, y, dy, lse, N, heads, hd, Tq, Tk, causal, lens, drop, R.STREAM_ID)
    _check_backward('B-big bf16', 'bf16', hd, R.BIG_P, got, grads_ref)


# ---------------------------------------------------------------------------------------------------- C. peaked scores, no dropout
def _peaked_id(c):
    return '%s-hd%d-%dx%d-%s' % (c[0], c[1], c[2], c[3], 'causal' if c[4] else 'full')


@functools.lru_cache(maxsize=None)
def _peaked_reference(case, rounded, from_bf16=False):
    """(inputs, vmax, A / A0 factor, y, lse, grads).  from_bf16: the operands are first rounded to bf16 rows (attn_b16's inputs)."""
    kind, hd, Tq, Tk, causal, lens = case
    N, heads = R.PEAKED_N, R.PEAKED_HEADS
    q, k, v = R.peaked_inputs(kind, N, heads, Tq, Tk, hd, R.PEAKED_SEED)
    q0, k0, _ = R.peaked_inputs('randn', N, heads, Tq, Tk, hd, R.PEAKED_SEED)
    dy = torch.randn(N * Tq, heads * hd, generator=torch.Generator().manual_seed(R.PEAKED_SEED + 1))
    if from_bf16:
        q, k, v, dy = (t.bfloat16().float() for t in (q, k, v, dy))
    factor = max(1.0, R.score_magnitude(q, k, hd, causal, lens, N) / R.score_magnitude(q0, k0, hd, causal, lens, N))
    qr, kr, vr, dyr, l2 = R.reference_operands('bf16' if rounded else 'f32', hd, q, k, v, dy)
    y, lse = R.attention_ref(qr, kr, vr, N, heads, hd, Tq, Tk, causal, lens, None, l2)
    grads = R.attention_grads_ref(qr, kr, vr, N, heads, hd, Tq, Tk, causal, lens, dyr, None, l2)
    return (q, k, v, dy), float(torch.as_tensor(vr).abs().max()), factor, y.numpy(), lse.numpy(), tuple(g.numpy() for g in grads)


def _check_peaked_forward(tag, mode, hd, vmax, factor, y, lse, y_ref, lse_ref):
    if mode == 'bf16':                                           # the derived bound of B at p = 0 is absolute
        _report(tag, 'y', y.cpu(), y_ref, R.fwd_gate(mode, hd, 0.0, vmax)[0])
    else:
        _report(tag, 'y', y.cpu(), y_ref, R.fwd_gate(mode, hd, 0.0, vmax)[0] * factor, relative_to=np.abs(y_ref).max())
    _report(tag, 'lse', lse.cpu(), lse_ref, R.lse_gate(mode, hd)[0] * factor, relative_to=np.abs(lse_ref).max())


def _check_peaked_backward(tag, mode, hd, factor, got, ref):
    for name, g, r in zip(('dq', 'dk', 'dv'), got, ref):
        _report(tag, name, g.float().cpu(), r, R.bwd_gate(mode, hd, 0.0)[0] * (1.0 if mode == 'bf16' else factor), relative_to=np.abs(r).max())


@pytest.mark.parametrize('case', R.PEAKED_CASES, ids=_peaked_id)
@MODE_PARAM
def test_peaked_scores_forward_and_backward_against_float64(hal, monkeypatch, math_mode, case):
    kind, hd, Tq, Tk, causal, lens = case
    N, heads = R.PEAKED_N, R.PEAKED_HEADS
    for name in ('HALO_ATTN_BWD_QB', 'HALO_ATTN_DKV_LF'):
        monkeypatch.delenv(name, raising=False)
    ops = hal['ops']
    inputs, vmax, factor, y_ref, lse_ref, grads_ref = _peaked_reference(case, math_mode == 'bf16')
    q, k, v, dy = (t.to(DEV) for t in inputs)
    tag = 'C %s %s' % (math_mode, _peaked_id(case))
    y, lse = _forward(ops, q, k, v, N, heads, hd, Tq, Tk, causal, lens, ops.NO_DROPOUT, 0)
    _check_peaked_forward(tag, math_mode, hd, vmax, factor, y, lse, y_ref, lse_ref)
    got = _backward(ops, q, k, v, y, dy, lse, N, heads, hd, Tq, Tk, causal, lens, ops.NO_DROPOUT, 0)
    _check_peaked_backward(tag, math_mode, hd, factor, got, grads_ref)


@pytest.mark.parametrize('case', R.PEAKED_CASES, ids=_peaked_id)
@pytest.mark.parametrize('math_mode', ['bf16x3', 'bf16'], indirect=True)
def test_peaked_scores_forward_with_bf16_output_against_float64(hal, math_mode, case):
    kind, hd, Tq, Tk, causal, lens = case
    N, heads = R.PEAKED_N, R.PEAKED_HEADS
    inputs, vmax, factor, y_ref, lse_ref, _ = _peaked_reference(case, math_mode == 'bf16')
    q, k, v, _ = (t.to(DEV) for t in inputs)
    y, lse, yb = hal['ops'].attention_fwd_bf16(q, k, v, N, heads, hd, Tq, Tk, causal=causal, key_lengths=_lens_dev(lens))
    _check_peaked_forward('C-bf16out %s %s' % (math_mode, _peaked_id(case)), math_mode, hd, vmax, factor, y, lse, y_ref, lse_ref)
    assert _one_bf16_rounding(yb, y)


@pytest.mark.parametrize('case', [c for c in R.PEAKED_CASES if c[1] == 64 and c[5] is None], ids=_peaked_id)     # attn_b16: hd 64, no key lengths
@pytest.mark.parametrize('math_mode', ['bf16'], indirect=True)
def test_peaked_scores_from_bf16_rows_against_float64(hal, math_mode, case):
    """attention_fwd_b16 / attention_bwd_b16 on operands already rounded to bf16: the reference reads the same bf16 values."""
    kind, hd, Tq, Tk, causal, lens = case
    N, heads = R.PEAKED_N, R.PEAKED_HEADS
    C = heads * hd
    ops = hal['ops']
    inputs, vmax, factor, y_ref, lse_ref, grads_ref = _peaked_reference(case, True, from_bf16=True)
    q, k, v, dy = (t.to(DEV).bfloat16() for t in inputs)
    tag = 'C-b16 %s' % _peaked_id(case)
    y, lse, yb = ops.attention_fwd_b16(q, k, v, N, heads, hd, Tq, Tk, causal=causal, want_y=True, want_lse=True)
    _check_peaked_forward(tag, 'bf16', hd, vmax, factor, y, lse, y_ref, lse_ref)
    assert _one_bf16_rounding(yb, y)
    d = torch.full((N * Tq, 3 * C), float('nan'), device=DEV, dtype=torch.bfloat16)
    ops.attention_bwd_b16(q, k, v, yb, dy, lse, d[:, :C], d[:, C:2 * C], d[:, 2 * C:], N, heads, hd, Tq, Tk, causal=causal)
    _check_peaked_backward(tag, 'bf16', hd, factor, (d[:, :C], d[:, C:2 * C], d[:, 2 * C:]), grads_ref)
