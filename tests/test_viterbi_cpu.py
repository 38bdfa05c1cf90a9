"""The yardstick of tests/test_gpu_viterbi.py, checked without a GPU: tests/viterbi_ref.py against brute-force enumeration, its
properties at every fixture, the fixtures' gap condition, and the tie rules."""
import itertools
import math

import numpy as np
import pytest
import torch

import viterbi_ref as R


def _log_probs(seed, *shape):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * 2).log_softmax(-1).double().numpy()


@pytest.mark.parametrize('target', [[], [1], [1, 2], [1, 1]], ids=['empty', 'one', 'two', 'repeated'])
def test_ctc_reference_is_the_best_of_all_labellings(target):
    T, C = 6, 3
    lp = _log_probs(len(target) * 7 + sum(target), T, C)
    best, arg = -math.inf, None
    for labelling in itertools.product(range(C), repeat=T):                      # all 3^6 frame labellings
        if R.collapse(labelling) == target:
            score = sum(lp[t][c] for t, c in enumerate(labelling))
            if score > best:
                best, arg = score, list(labelling)
    ref = R.ctc_align_row(lp, target, T)
    assert arg is not None
    assert abs(ref['score'] - best) <= 1e-12
    assert ref['alignment'] == arg


def test_transducer_reference_is_the_best_of_all_monotone_paths():
    T, U, K = 4, 3, 5
    joint = _log_probs(3, T, U + 1, K)
    target = [2, 4, 1]
    best, arg, paths = -math.inf, None, 0
    for where in itertools.combinations(range(T + U), U):                        # all C(7, 3) orders of 4 blanks and 3 labels ...
        if T + U - 1 in where:                                                   # ... of which a path ends in its last blank
            continue
        paths += 1
        t = u = 0
        score, frames = 0.0, []
        for move in range(T + U):
            if move in where:
                score += joint[t][u][target[u]]
                frames.append(t)
                u += 1
            else:
                score += joint[t][u][0]
                t += 1
        if score > best:
            best, arg = score, frames
    assert paths == math.comb(T + U - 1, U)
    ref = R.transducer_align_row(joint, target, T)
    assert abs(ref['score'] - best) <= 1e-12
    assert ref['frames'] == arg


@pytest.mark.parametrize('name', sorted(R.CTC_FIXTURES))
def test_ctc_fixture_properties_and_gaps(name):
    lp, targets, il, tl, rows = R.ctc_fixture(name)
    N = lp.shape[1]
    lp64 = lp.double().numpy()
    left_out = R.LEFT_OUT.get(('ctc', name), ())
    assert len(left_out) * 4 <= N
    for n, r in enumerate(rows):
        target = [int(y) for y in targets[n, :int(tl[n])]]
        kind = R.SPECIAL.get(n) if name == 'small_vocab' else None
        if kind == 'infeasible':
            assert r['score'] == -math.inf and r['alignment'] is None
            assert R.ctc_log_sum_row(lp64[:, n], target, int(il[n])) == -math.inf
            assert n not in left_out
            continue
        assert r['score'] > -math.inf
        assert len(r['alignment']) == int(il[n])
        assert R.collapse(r['alignment']) == target
        assert abs(r['score'] - sum(lp64[t, n, c] for t, c in enumerate(r['alignment']))) <= 1e-9
        assert r['score'] <= R.ctc_log_sum_row(lp64[:, n], target, int(il[n])) + 1e-9
        for u in range(len(target)):
            span = [t for t, s in enumerate(r['states']) if s == 2 * u + 1]
            assert (r['starts'][u], r['ends'][u]) == (span[0], span[-1]) and span == list(range(span[0], span[-1] + 1))
        if kind is not None:
            assert n not in left_out
        if kind in ('forced', 'empty_target', 'one_frame'):
            assert r['gap'] == math.inf                                          # one path only
        if n in left_out:
            assert r['gap'] < R.GAP                                              # the table names nothing it need not
        else:
            assert r['gap'] >= R.GAP, (name, n, r['gap'])
    if name == 'small_vocab':
        kinds = {k: n for n, k in R.SPECIAL.items()}
        assert int(tl[kinds['empty_target']]) == 0 and rows[kinds['empty_target']]['alignment'] == [0] * int(il[kinds['empty_target']])
        n = kinds['forced']
        assert int(il[n]) == int(tl[n]) + R.repeats([int(y) for y in targets[n, :int(tl[n])]])
        n = kinds['infeasible']                                                  # one frame short of what its target needs
        assert int(il[n]) == int(tl[n]) + R.repeats([int(y) for y in targets[n, :int(tl[n])]]) - 1
        n = kinds['one_frame']
        assert (int(il[n]), int(tl[n])) == (1, 1) and rows[n]['alignment'] == [int(targets[n, 0])]
        assert any(R.repeats([int(y) for y in targets[m, :int(tl[m])]]) for m in range(N))     # skips are disabled somewhere
    assert (targets[torch.arange(targets.shape[1])[None, :] >= tl[:, None]] == R.GARBAGE).all()


@pytest.mark.parametrize('name', sorted(R.TRANSDUCER_FIXTURES))
def test_transducer_fixture_properties_and_gaps(name):
    f, g, joint, targets, tn, un, rows = R.transducer_fixture(name)
    N = joint.shape[0]
    j64 = joint.double().numpy()
    left_out = R.LEFT_OUT.get(('transducer', name), ())
    assert len(left_out) * 4 <= N
    for n, r in enumerate(rows):
        Tn, Un = int(tn[n]), int(un[n])
        target = [int(y) for y in targets[n, :Un]]
        kind = R.TRANSDUCER_SPECIAL.get(n) if name == 'edges' else None
        if kind is not None:
            assert n not in left_out
        if kind == 'empty_row':
            assert Tn == 0 and r['score'] == -math.inf and r['frames'] is None
            continue
        path = r['path']
        assert path[0] == (0, 0) and path[-1] == (Tn - 1, Un) and len(path) == Tn + Un
        total, frames = j64[n, Tn - 1, Un, 0], []
        for (t0, u0), (t1, u1) in zip(path, path[1:]):
            assert (t1 - t0, u1 - u0) in ((1, 0), (0, 1))
            if u1 > u0:
                total += j64[n, t0, u0, target[u0]]
                frames.append(t0)
            else:
                total += j64[n, t0, u0, 0]
        assert frames == r['frames'] and len(frames) == Un                       # the path emits the whole target, in order
        assert abs(r['score'] - total) <= 1e-9
        assert r['score'] <= R.transducer_log_sum_row(j64[n], target, Tn) + 1e-9
        if kind == 'one_frame':
            assert Tn == 1 and r['frames'] == [0] * Un and r['gap'] == math.inf
        if kind == 'empty_target':
            assert Un == 0 and r['frames'] == [] and r['gap'] == math.inf
        if n in left_out:
            assert r['gap'] < R.GAP
        else:
            assert r['gap'] >= R.GAP, (name, n, r['gap'])


@pytest.mark.parametrize('name', sorted(R.CTC_EXACT))
def test_ctc_wide_fixtures_sum_without_rounding(name):
    lp, targets, il, tl, rows = R.ctc_exact_fixture(name)
    T = lp.shape[0]
    assert (lp * 64 == torch.round(lp * 64)).all() and float(lp.min()) >= -8 and float(lp.max()) <= 0
    assert T * 8 < 2 ** 17 and 2 ** 17 * 64 <= 2 ** 24                            # every partial sum fits fp32's 24 bits
    lp64 = lp.double().numpy()
    for n, r in enumerate(rows):
        target = [int(y) for y in targets[n, :int(tl[n])]]
        assert len(r['alignment']) == int(il[n]) and R.collapse(r['alignment']) == target
        assert r['score'] == sum(lp64[t, n, c] for t, c in enumerate(r['alignment']))
        assert np.float32(r['score']) == r['score']
    assert 2 * targets.shape[1] + 1 == {'per4': 601, 'per8': 1041, 'per16': 2061, 'per30': 7679}[name]


@pytest.mark.parametrize('name', sorted(R.TRANSDUCER_EXACT))
def test_transducer_wide_fixtures_sum_without_rounding(name):
    joint, targets, tn, un, rows = R.transducer_exact_fixture(name)
    assert (joint * 64 == torch.round(joint * 64)).all() and float(joint.min()) >= -8 and float(joint.max()) <= 0
    assert (joint.shape[1] + joint.shape[2]) * 8 < 2 ** 17
    for n, r in enumerate(rows):
        assert len(r['path']) == int(tn[n]) + int(un[n]) and len(r['frames']) == int(un[n])
        assert r['frames'] == sorted(r['frames']) and np.float32(r['score']) == r['score']


def test_tie_rules_of_the_reference():
    c = R.TIE_CTC
    r = R.ctc_align_row(np.full((c['T'], c['C']), -2.0), c['target'], c['T'])
    assert r['score'] == c['score']
    assert r['alignment'] == c['alignment'] == [1, 0, 1, 2, 0, 0, 0]             # every move as early as it is legal
    assert (r['starts'], r['ends']) == (c['starts'], c['ends'])
    assert r['gap'] == 0.0                                                       # every path ties: only the rule decides
    c = R.TIE_TRANSDUCER
    r = R.transducer_align_row(np.full((c['T'], c['U'] + 1, c['K']), -2.0), c['target'], c['T'])
    assert r['score'] == c['score']
    assert r['frames'] == c['frames'] == [0, 0]                                  # blank predecessors first, read backwards: labels at frame 0
    assert r['gap'] == 0.0


def test_empty_inputs_of_the_reference():
    lp = _log_probs(1, 4, 3)
    assert R.ctc_align_row(lp, [], 0)['score'] == 0.0
    assert R.ctc_align_row(lp, [1], 0)['score'] == -math.inf
    assert R.ctc_align_row(lp, [1, 1], 2)['score'] == -math.inf                  # a repeated pair needs three frames
    assert R.ctc_align_row(lp, [1, 1], 3)['alignment'] == [1, 0, 1]
