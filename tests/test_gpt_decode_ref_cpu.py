"""tests/gpt_decode_ref.py before anything is tied to it: the references against torch where torch has the operation, every stand-in inside
its own bound, every mutant leaving the float64 reference by at least twice the bound a device is held to (the draw mutants: fewer than half
of the stand-in's draws accepted), the stand-in's draws accepted on every line at that line's delta, and the restated dispatches naming every
instantiation tests/test_gpu_gpt_decode_f64.py is there for.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpt_decode_ref as R

F32, F64 = torch.float32, torch.float64
LIN_MODES = [(c.name, m) for c in R.LINEAR_CASES for m in R.MODES]


# ---- linear ------------------------------------------------------------------------------------------------------------------------
def test_layer_norm_and_product_agree_with_torch():
    case = R.LINEAR_BY_NAME['33x1024x100_L']
    inp = R.linear_inputs(case.name)
    x, w, lnw = inp['x'], inp['w'], inp['lnw']
    want = F.layer_norm(x.double(), (case.K,), lnw.double(), None, R.EPS)
    xn = R.layer_norm64(x, lnw)
    assert (xn - want).abs().max().item() < 1e-13
    assert (R.layer_norm32(x, lnw).double() - want).abs().max().item() < 2e-6
    S = R.linear_scale(case, inp)
    plain = want @ w.double().T
    # the rounding models against the plain float64 product: bf16 rounds each operand to 2^-9 relative, x3 leaves 2^-16 and lo lo
    assert R.deviation(R.linear_reference(case.name, 'bf16'), plain, S) < 2.0 ** -8
    assert R.deviation(R.linear_reference(case.name, 'bf16x3'), plain, S) < 2.0 ** -15
    a = torch.tensor([[1.0 + 2.0 ** -8, 3.0]]); b = torch.tensor([[1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0]])
    assert [tuple(t[0].flatten().tolist()) for t in R.linear_terms(a, b, 'bf16x3')] == [(2.0 ** -8, 0.0), (1.0, 3.0), (1.0, 3.0)]
    assert sum(p @ q.T for p, q in R.linear_terms(a.double(), b, 'bf16')).item() == 1.0 * (1.0 + 2.0 ** -6) + 3.0
    # the epilogue: GELU of the product, then the addend
    c = R.LINEAR_BY_NAME['6x256x24_A_G']
    i2 = R.linear_inputs(c.name)
    acc = sum(p @ q.T for p, q in R.linear_terms(i2['x'].double(), i2['w'], 'bf16x3'))
    assert torch.equal(R.linear_reference(c.name, 'bf16x3'), F.gelu(acc, approximate='tanh') + i2['out0'][:, :24].double())


def test_lane_order_of_the_statistics():
    """_lanes restates which elements a lane holds: wave w, k-step i, lane group g, slot j <-> k = (w * ksw + i) * 32 + 8 g + j."""
    K = 768
    v = R._lanes(torch.arange(K, dtype=F32)[None])
    assert v.shape == (1, 4, 4, 48)
    for w, g, i, j in ((0, 0, 0, 0), (1, 2, 3, 5), (3, 3, 5, 7)):
        assert v[0, w, g, i * 8 + j].item() == (w * 6 + i) * 32 + 8 * g + j


@pytest.mark.parametrize('name,mode', LIN_MODES, ids=[f'{n}-{m}' for n, m in LIN_MODES])
def test_linear_stand_in_and_mutants(name, mode):
    """The stand-in inside its own bound (a factor 8 to spare by construction) and inside a rail of 2^-22 S sqrt(K); behind a LayerNorm no
    normalised element within reach of a bf16 rounding boundary, and none rounded another way by the fp32 statistics; every applicable
    mutant at least twice the bound away."""
    case, inp = R.LINEAR_BY_NAME[name], R.linear_inputs(name)
    noise, bound = R.linear_noise(name, mode), R.linear_bound(name, mode)
    print(f'{name} {mode} stand-in {noise:.2e} bound {bound:.2e}')
    assert noise <= bound / R.FACTOR or bound == R.FLOOR
    assert noise <= 2.0 ** -22 * case.K ** 0.5
    if case.ln:
        dist, margin = R.tie_distance(inp['x'], inp['lnw'])
        assert bool((dist >= margin).all())
        assert torch.equal(R.rb(R.layer_norm32(inp['x'], inp['lnw'])).double(), R.rb(R.layer_norm64(inp['x'], inp['lnw'])))
        assert 0.05 < inp['x'][-1].std().item() < 0.15 and 1.3 < inp['x'][0].std().item() < 1.7
    S, ref = R.linear_scale(case, inp), R.linear_reference(name, mode)
    for mutant in R.LINEAR_MUTANTS:
        if not R.linear_mutant_applies(mutant, case, mode):
            continue
        dev = R.deviation(R.linear_reference(name, mode, mutant), ref, S)
        print(f'{name} {mode} {mutant} {dev:.2e} = {dev / bound:.1f} x bound')
        assert dev >= 2.0 * bound, (mutant, dev, bound)


def test_every_linear_mutant_is_reached():
    for mutant in R.LINEAR_MUTANTS:
        assert any(R.linear_mutant_applies(mutant, c, m) for c in R.LINEAR_CASES for m in R.MODES), mutant


def test_plan_names_every_instantiation_the_entry_can_launch():
    labels = {R.plan(c.rows, c.K, c.n_out, c.ln).label(m) for c in R.LINEAR_CASES for m in R.MODES}
    assert labels == {f'NT{nt} LN{ln} P{p}' for nt in (1, 2) for ln in (0, 4, 6, 8) for p in (1, 3)}
    walks = {c.K: R.plan(c.rows, c.K, c.n_out, c.ln).walk for c in R.LINEAR_CASES if not c.ln}
    assert walks == {256: (2,), 768: (4, 2), 1280: (4, 4, 2), 2048: (8, 8), 3072: (8, 8, 8)}
    p = R.plan(130, 512, 904, True)
    assert (p.NT, p.n_tiles, p.row_groups, p.ksw_ln) == (2, 57, 9, 4) and 904 % 16 == 8
    p = R.plan(4, 1024, 8200, True)
    assert (p.NT, p.n_tiles, p.row_groups) == (2, 513, 1)
    assert R.plan(33, 1024, 100, True).NT == 1 and R.plan(*R.BITCHECK, False).NT == 1
    # what the model-level tests reach: C = 768 and lm_head at 50304, an even tile count
    assert R.plan(8, 768, 50304, True).NT == 2 and R.plan(8, 768, 50304, True).n_tiles % 2 == 0 and R.plan(8, 768, 2304, True).NT == 1
    assert not R.linear_supported(640, True) and not R.linear_supported(384, False) and R.linear_supported(1280, False)


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def test_attention_table_names_all_four_kernels():
    assert {R.attention_plan(c.B, c.heads, c.Tc) for c in R.ATTENTION_CASES} == {(1024, 16), (1024, 4), (8192, 16), (8192, 4)}
    assert R.attention_plan(16, 8, 1024) == (1024, 16) and R.attention_plan(43, 3, 1024) == (1024, 4)      # 128 pairs: still sixteen waves
    c = R.ATTENTION_BY_NAME['17x8x320']
    assert len(c.pos) == c.B and R.clamped(c)[11].item() == 0 and R.clamped(c)[12].item() == 319
    sharp = R.attention_inputs(c.name)
    C = c.heads * 64
    s = torch.einsum('hd,hjd->hj', sharp['qkv'][c.sharp_row, :C].view(8, 64), sharp['ck'][c.sharp_row, :, :200]) / 8
    assert 40 < s.abs().max().item() < 120
    assert bool((sharp['ck'][c.equal_row] == sharp['ck'][c.equal_row, :, :1]).all())


def test_attention_reference_agrees_with_torch_on_a_full_cache():
    case = R.ATTENTION_BY_NAME['1x2x8192']
    inp = R.attention_inputs(case.name)
    C = case.heads * 64
    qkv = inp['qkv'].double()
    k, v = inp['ck'].double().clone(), inp['cv'].double().clone()
    k[0, :, -1] = qkv[0, C:2 * C].view(2, 64)
    v[0, :, -1] = qkv[0, 2 * C:].view(2, 64)
    want = F.scaled_dot_product_attention(qkv[:, :C].view(1, 2, 1, 64), k, v).reshape(1, C)
    got, S = R.attention_reference(case.name)
    assert ((got - want).abs() / S).max().item() < 1e-13
    # a row whose keys are all equal attends uniformly
    c = R.ATTENTION_BY_NAME['17x8x320']
    i2 = R.attention_inputs(c.name)
    v = i2['cv'][c.equal_row, :, :301].double().clone()
    v[:, 300] = i2['qkv'][c.equal_row, 2 * 512:].view(8, 64).double()
    assert (R.attention_reference(c.name)[0][c.equal_row] - v.mean(1).reshape(-1)).abs().max().item() < 1e-13


@pytest.mark.parametrize('name', [c.name for c in R.ATTENTION_CASES])
def test_attention_stand_in_and_mutants(name):
    case = R.ATTENTION_BY_NAME[name]
    noise, bound = R.attention_noise(name), R.attention_bound(name)
    print(f'{name} stand-in {noise.max().item():.2e} bound per row {bound.min().item():.2e} .. {bound.max().item():.2e}')
    assert bool((noise <= bound / R.FACTOR).logical_or(bound == R.FLOOR).all())
    ref, S = R.attention_reference(name)
    assert bool(torch.isfinite(ref).all()) and bool((S > 0).all())
    for mutant in R.ATTENTION_MUTANTS:
        if not R.attention_mutant_applies(mutant, case):
            continue
        dev = (R.row_deviation(R.attention_reference(name, mutant)[0], ref, S) / bound).max().item()
        print(f'{name} {mutant} {dev:.1f} x bound')
        assert dev >= 2.0, (mutant, dev)
    assert R.attention_mutant_applies('pass_tail_dropped', case) == (name != '1x2x8192')


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [d.name for d in R.DRAW_LINES])
def test_stand_in_draws_are_accepted_and_the_mutants_are_not(name):
    """That the definition in fp32 is accepted on every draw is the condition under which the GPU test's "no draw left out" can be met."""
    line = R.DRAW_BY_NAME[name]
    tokens = R.stand_in_draw(name)
    delta, worst = R.draw_delta(name)
    keep = R.kept(R.draw_logits(name), line)
    print(f'{name} delta {delta:.2e} (stand-in |cdf32 - cdf64| / total {worst:.2e}) kept per row {keep.sum(1).tolist()}')
    assert tokens.min() >= 0 and tokens.max() < line.V
    ok = R.draws_accepted(name, tokens)
    assert bool(ok.all()), int((~ok).sum())
    assert len(np.unique(tokens)) > ROWS_DISTINCT
    for mutant in R.DRAW_MUTANTS:
        if not R.draw_mutant_applies(mutant, line):
            continue
        frac = float(R.draws_accepted(name, tokens, mutant).mean())
        print(f'{name} {mutant} accepted {frac:.2f}')
        assert frac < 0.5, (mutant, frac)


ROWS_DISTINCT = 8


def test_draw_lines_are_what_they_say():
    keep = lambda n: R.kept(R.draw_logits(n), R.DRAW_BY_NAME[n])
    assert keep('v1000_k100_zeros').sum(1).tolist() == [430] * R.ROWS
    assert R.kept(R.draw_logits('v1000_k100_zeros'), R.DRAW_BY_NAME['v1000_k100_zeros'], 'signed_zero_split').sum(1).tolist() == [230] * R.ROWS
    assert R.kept(R.draw_logits('v1000_k100_zeros'), R.DRAW_BY_NAME['v1000_k100_zeros'], 'threshold_strict').sum(1).tolist() == [30] * R.ROWS
    assert bool((keep('v2048_k100_quarter').sum(1) > 100).all())
    assert bool(keep('v4100_kV').all()) and bool(keep('v4100_kVp5').all()) and keep('v4100_kVm1').sum(1).tolist() == [4099] * R.ROWS
    lg = R.draw_logits('v2048_k40_ninf')
    assert (np.isinf(lg).sum(1) == 512).all() and not (keep('v2048_k40_ninf') & np.isinf(lg)).any()
    assert keep('v40_k20').sum(1).tolist() == [20] * R.ROWS
    for mutant in R.DRAW_MUTANTS:
        assert any(R.draw_mutant_applies(mutant, d) for d in R.DRAW_LINES), mutant
    assert [d.name for d in R.DRAW_LINES if R.draw_mutant_applies('signed_zero_split', d)] == ['v1000_k100_zeros']
    assert {d.name for d in R.DRAW_LINES if R.draw_mutant_applies('threshold_strict', d)} == {'v1000_k100_zeros', 'v2048_k100_quarter'}
    # an independent uniform accepts a draw with probability sum p^2 >= 1 / kept: two lines cannot lose half their draws to foreign uniforms
    assert [d.name for d in R.DRAW_LINES if R.collision(d.name) > R.COLLISION_CAP] == ['v4100_k2_t5', 'v50257_k40_t0.05']
    assert R.collision('v4100_k2_t5') >= 0.5 and R.rejections_wanted('v4100_k2_t5', 512) > 100 and R.rejections_wanted('v40_k20', 512) == 256
    # the sharp line: inv_t is 1 / T rounded to float32, and l is formed in float32
    assert R.inv_temperature(0.05) == np.float32(20.0) and R.inv_temperature(0.7) == np.float32(1.0 / 0.7)
