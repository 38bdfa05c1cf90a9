"""CPU checks of tests/asr_lm_beam_ref.py, the float64 restatement of the attention decoder's beam search with LM shallow fusion
(DESIGN.md 3.3ab), and of the fixture conditions tests/test_gpu_asr_lm_beam.py relies on: which rows of every case are left out (a
decision below GAP), that lm_weight = 0 restates the searches without the LM, that every returned lm is the teacher-forced LM score of
its tokens, and that the LM changes the best hypothesis (so the cases cannot pass on the unfused search)."""
import pytest
import torch

import asr_beam_ref as A
import asr_joint_beam_ref as J
import asr_lm_beam_ref as R

ETX = R.ETX


def _id(case):
    return '-'.join(str(x) for x in case[:8])


def test_gap_is_the_derived_figure():
    assert max(case[4] for case in R.CASES) <= 0.7
    assert 2 * (2e-3 + 0.7 * 1e-4) <= R.GAP == 4.5e-3


@pytest.mark.parametrize('case', R.CASES, ids=_id)
def test_left_out_rows_are_the_listed_ones(case):
    N = A.CASES[R.base_case(case[0])][5]
    assert R.left_out(case) == list(case[8])
    assert 3 * len(case[8]) <= N
    assert R.compared_rows(case) == [n for n in range(N) if n not in case[8]]


def test_left_out_rows_overall():
    assert sum(len(case[8]) for case in R.CASES) <= R.MAX_LEFT_OUT
    assert sum(A.CASES[R.base_case(case[0])][5] for case in R.CASES) == 125


@pytest.mark.parametrize('case', R.CASES, ids=_id)
def test_weight_zero_restates_the_search_without_the_lm(case):
    name, W, c, Ll, a, bonus, start, eos, _ = case
    base = R.base_case(name)
    heads, T = A.CASES[base][2], A.CASES[base][11]
    pd, feats, flen, _ = R.case_inputs(name)
    got = R.case_result(case, 0.0)
    if c > 0.0:
        want = J.joint_beam_search(pd, feats, flen, J.ctc_log_probs(name), heads, W, T, bonus, c)
    else:
        want = A.beam_search(pd, feats, flen, heads, W, T, bonus)
    for key in want:
        assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize('case', R.CASES, ids=_id)
def test_lm_scores_are_the_teacher_forced_ones(case):
    name, W, c, Ll, a, bonus, start, eos, _ = case
    res = R.case_result(case)
    lm64 = R.language_model(case)[1]
    N = res['lengths'].shape[0]
    for n in range(N):
        for w in range(int(res['counts'][n])):
            y = res['tokens'][n, w, :int(res['lengths'][n, w])].tolist()
            want = lm64.score(y, start)
            if bool(res['finished'][n, w]) and eos is not None:
                want += _eos_term(lm64, y, start, eos)
            assert abs(float(res['lm'][n, w]) - want) <= 1e-13 * max(1.0, abs(want)), (n, w)
        assert bool((res['lm'][n, int(res['counts'][n]):] == R.NINF).all())
    # the rank is the sum of its parts
    present = res['lengths'] >= 0
    base = (1.0 - c) * res['attention'] + c * res['ctc'] if c > 0.0 else res['attention']
    assert torch.allclose(res['ranks'][present], (base + a * res['lm'])[present], rtol=0, atol=1e-12)


def _eos_term(lm64, y, start, eos):
    """log P(eos | start, y): the LM's price of closing."""
    return lm64.score(list(y) + [eos], start) - lm64.score(y, start)


@pytest.mark.parametrize('case', R.CASES, ids=_id)
def test_the_lm_changes_the_best_hypothesis(case):
    rows = R.compared_rows(case)
    with_lm, without = R.case_result(case), R.case_result(case, 0.0)
    changed = sum(not torch.equal(with_lm['tokens'][n, 0], without['tokens'][n, 0])
                  or bool(with_lm['finished'][n, 0]) != bool(without['finished'][n, 0]) for n in rows)
    assert changed > 0
