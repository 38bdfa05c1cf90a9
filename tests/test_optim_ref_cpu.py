"""tests/optim_ref.py checked on the CPU: its float64 step equals torch.optim.AdamW + clip_grad_norm_ in float64 over the trainer's chain
(skipped step included); the gates of tests/test_gpu_optim.py are 4x the float32 restatement's own error; and on the inputs the GPU tests
use, every mutant is rejected by the comparison those tests use while the float32 restatement passes it."""
import functools

import numpy as np
import pytest
import torch

import optim_ref as R
from optim_ref import GATES


def test_float64_steps_equal_torch_adamw_and_clip_grad_norm_over_the_chain():
    ref, want = R.chain_run(), R.torch_chain()
    clipped = [r['coef'] < 1.0 for r in ref if r['coef'] == r['coef']]
    assert sum(clipped) >= 5 and len(clipped) - sum(clipped) >= 5          # some steps clip, some do not
    assert ref[R.CHAIN_INF_STEP]['coef'] != ref[R.CHAIN_INF_STEP]['coef']
    for k in range(R.CHAIN_STEPS):
        assert ref[k]['applied'] == want[k]['applied'] == (k + 1 if k < R.CHAIN_INF_STEP else k)
        errs = R.state_err([ref[k][x] for x in 'pmv'], [want[k][x] for x in 'pmv'], ref[k]['scales'])
        assert R.within(errs, (1e-14, 1e-14, 1e-14)), (k, errs)             # float64 rounding: a few ulp of 1.1e-16 over 25 steps
    k = R.CHAIN_INF_STEP
    for x in 'pmv':
        assert np.array_equal(ref[k][x], ref[k - 1][x])                      # the skipped step changes nothing


def _adamw_errs(step_fn, n, betas, scale):
    """max over the 12 steps of the (p, m, v) errors of step_fn's run against adamw_step's, and the errors after the last step."""
    p, g, _ = R.adamw_inputs(n)
    b1, b2 = R.BETAS[betas]
    ref = R.run_steps(R.adamw_step, p, g, R.LR, b1, b2, R.EPS, R.WD, scale)
    with np.errstate(all='ignore'):
        got = list(R.run_steps(step_fn, p, g, R.LR, b1, b2, R.EPS, R.WD, scale))
    mabs, worst = np.zeros(n), (0.0, 0.0, 0.0)
    for k, want in enumerate(ref):
        mabs = R.mabs_next(mabs, g[k], b1, scale)
        last = R.state_err(got[k], want, R.step_scales(mabs))
        worst = tuple(max(a, b) for a, b in zip(worst, last))
    return worst, last


@pytest.mark.parametrize('betas', list(R.BETAS))
def test_adamw_gates_are_four_times_the_float32_restatements_error(betas):
    """Measured where the maximum runs over the most elements (the largest size of the GPU test), after the last step, per output."""
    worst, last = _adamw_errs(R.f32_restatement, R.GATE_N, betas, None)
    print(f'adamw {betas}: f32 restatement vs float64 after step {R.ADAMW_STEPS}: p {last[0]:.4e} m {last[1]:.4e} v {last[2]:.4e}; '
          f'worst step p {worst[0]:.4e} m {worst[1]:.4e} v {worst[2]:.4e}')
    for gate, e in zip(GATES['adamw_' + betas], last):
        assert gate == pytest.approx(4.0 * e, rel=5e-3), (gate, 4.0 * e)
    assert R.within(worst, GATES['adamw_' + betas])                          # and it passes at every step, not only the last


def test_chain_gates_are_four_times_the_float32_restatements_error():
    ref, got = R.chain_run(), R.chain_run(single=True)
    errs = [R.state_err([got[k][x] for x in 'pmv'], [ref[k][x] for x in 'pmv'], ref[k]['scales']) for k in range(R.CHAIN_STEPS)]
    print('chain: f32 restatement vs float64 after the last step: p %.4e m %.4e v %.4e' % errs[-1])
    for gate, e in zip(GATES['chain'], errs[-1]):
        assert gate == pytest.approx(4.0 * e, rel=5e-3), (gate, 4.0 * e)
    assert all(R.within(e, GATES['chain']) for e in errs)


def test_sumsq_gate_is_positive_at_every_size_of_the_gpu_test():
    for n in R.SUMSQ_SIZES:
        x, want, rtol = R.sumsq_case(n)
        assert 2.0 ** -26 <= rtol < 1e-6 and want > 0, (n, rtol)           # a seed on which the float32 sum is exact by luck gates nothing sensibly


PER_ELEMENT = [k for k in R.MUTANTS if k not in R.RANGE_MUTANTS and not k.startswith('f_')]      # (f) needs a changing lr, see below


@pytest.mark.parametrize('betas', list(R.BETAS))
def test_every_per_element_mutant_fails_the_adamw_comparison_and_the_restatement_passes(betas):
    """The 12-step halo_adamw test's inputs at n = 4097 with grad_scale 0.5 (mutant g needs a scale that is not 1)."""
    gates = GATES['adamw_' + betas]
    for n in (1023, 4097):
        for scale in (None, 0.5):
            assert R.within(_adamw_errs(R.f32_restatement, n, betas, scale)[0], gates)
    for name in PER_ELEMENT:
        worst, _ = _adamw_errs(R.MUTANTS[name], 4097, betas, 0.5)
        assert not R.within(worst, gates), (name, worst)
    # a NaN scale: nothing moves, in the reference and in the restatement
    p, g, _ = R.adamw_inputs(5)
    for fn in (R.adamw_step, R.f32_restatement):
        out = fn(p, g[0], p * 0.5, p * p, R.LR, *R.BETAS[betas], R.EPS, R.WD, 3, float('nan'))
        assert all(np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64)) for a, b in zip(out, (p, p * 0.5, p * p)))


@pytest.mark.parametrize('t', R.LATE_STEPS)
def test_late_single_steps_pass_for_the_restatement_and_fail_for_mutants(t):
    """(The mutants of the bias corrections are the reference itself once b^t has underflowed; they are judged on the first 12 steps.)"""
    for betas, (b1, b2) in R.BETAS.items():
        p, g, s = R.adamw_inputs(4097)
        m, v = R.make_moments(s, g[0], 5)
        want = R.adamw_step(p, g[0], m, v, R.LR, b1, b2, R.EPS, R.WD, t, 0.5)
        scales = R.step_scales(R.mabs_next(np.abs(m), g[0], b1, 0.5))
        got = R.f32_restatement(p, g[0], m, v, R.LR, b1, b2, R.EPS, R.WD, t, 0.5)
        assert R.within(R.state_err(got, want, scales), GATES['adamw_' + betas])
        for name in ('d_coupled_l2_decay', 'e_decay_after_step', 'g_scale_on_m_only', 'h_b2_swapped_in_v'):
            bad = R.MUTANTS[name](p, g[0], m, v, R.LR, b1, b2, R.EPS, R.WD, t, 0.5)
            assert not R.within(R.state_err(bad, want, scales), GATES['adamw_' + betas]), (name, betas)


def test_ranges_mutants_fail_on_the_eight_range_buffer_and_the_restatement_passes():
    """Mutant (i) (a range takes its neighbour's wd and scale) and, through ranges_step, two per-element ones, on the 8-range inputs."""
    p, g, _, ranges, inside = R.ranges_inputs()
    b1, b2 = R.BETAS['b95']
    gates = GATES['adamw_b95']
    runs = {'ref': lambda *a: R.ranges_step(*a), 'f32': lambda *a: R.ranges_step(*a, step_fn=R.f32_restatement),
            'i': R.MUTANTS['i_neighbours_wd_and_scale'], 'c': lambda *a: R.ranges_step(*a, step_fn=R.MUTANTS['c_no_second_moment_correction'])}
    state = {k: (p, np.zeros_like(p), np.zeros_like(p)) for k in runs}
    mabs, ok = np.zeros(len(p)), {k: True for k in runs}
    for k in range(R.RANGES_STEPS):
        gk = np.where(inside, g[k], 0.0)                 # (the NaN canaries of the gaps are never read; ranges_step slices them away too)
        mabs = R.ranges_mabs(mabs, gk, ranges, b1)
        with np.errstate(all='ignore'):
            state = {name: fn(*state[name][:1], gk, *state[name][1:], ranges, R.LR, b1, b2, R.EPS, k + 1) for name, fn in runs.items()}
        for name in runs:
            ok[name] &= R.within(R.state_err(state[name], state['ref'], R.ranges_scales(mabs, ranges)), gates)
    assert ok['f32'] and not ok['i'] and not ok['c'], ok
    nan_range = [r for r in ranges if r[3] is not None and r[3] != r[3]][0]
    assert np.array_equal(state['ref'][0][nan_range[0]:nan_range[1]], p[nan_range[0]:nan_range[1]].astype(np.float64))
    assert np.array_equal(state['ref'][0][~inside], p[~inside].astype(np.float64))


def test_stale_decay_mutant_fails_under_a_changing_lr_and_the_restatement_passes():
    """Mutant (f) is invisible under a constant lr; the halo_adamw_ranges_dev test changes lr between launches."""
    ref = R.changing_lr_run(R.adamw_step)
    f32 = R.changing_lr_run(R.f32_restatement)
    bad = R.changing_lr_run(R.MUTANTS['f_decay_from_previous_lr'], stale=True)
    _, g, _, _ = R.dev_inputs()
    b1 = R.BETAS['b95'][0]
    mabs, ok_f32, ok_bad = np.zeros(R.DEV_N), True, True
    for k in range(len(R.DEV_LRS)):
        mabs = R.ranges_mabs(mabs, g[k], R.DEV_RANGES, b1)
        scales = R.ranges_scales(mabs, R.DEV_RANGES)
        ok_f32 &= R.within(R.state_err(f32[k], ref[k], scales), GATES['adamw_b95'])
        ok_bad &= R.within(R.state_err(bad[k], ref[k], scales), GATES['adamw_b95'])
    assert ok_f32 and not ok_bad
    # under a constant lr the mutant IS the reference: that is why the other tests cannot see it
    p, g, _ = R.adamw_inputs(5)
    a = list(R.run_steps(R.adamw_step, p, g, R.LR, *R.BETAS['b95'], R.EPS, R.WD))[-1]
    b = list(R.run_steps(R.MUTANTS['f_decay_from_previous_lr'], p, g, R.LR, *R.BETAS['b95'], R.EPS, R.WD))[-1]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_chain_rejects_mutants_too():
    ref = R.chain_run()
    for name in ('i_neighbours_wd_and_scale', 'g_scale_on_m_only', 'b_bias_correction_at_t_minus_1'):
        fn = R.MUTANTS[name]
        got = R.chain_run(fn if name in R.RANGE_MUTANTS else functools.partial(R.ranges_step, step_fn=fn))
        ok = all(R.within(R.state_err([got[k][x] for x in 'pmv'], [ref[k][x] for x in 'pmv'], ref[k]['scales']), GATES['chain'])
                 for k in range(R.CHAIN_STEPS))
        assert not ok, name


def test_clip_coef_reference():
    assert R.clip_coef(0.0, 1.0) == (1.0, 1.0, 0.0)
    assert R.clip_coef(4.0, 3.0)[0] == 1.0
    assert R.clip_coef(16.0, 1.0)[0] == pytest.approx(1.0 / (4.0 + 1e-6), rel=1e-15)
    for bad in (float('inf'), float('nan')):
        c0, c1, _ = R.clip_coef(bad, 1.0)
        assert c0 != c0 and c1 != c1
