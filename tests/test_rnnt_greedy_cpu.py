"""The float64 restatement of greedy transducer search (tests/rnnt_greedy_ref.py) against itself, and the conditions on its fixtures
that tests/test_gpu_rnnt_decode.py relies on.  CPU only.

    teacher-forced check: nn.LSTM run teacher-forced on [0 | hyp] gives the full log_softmax joint [T, U + 1, V]; walking the returned
        frames, every free move of the path is the argmax of its node and the moves sum to the returned score (1e-9)
    lattice bound: for rows not truncated the score is the log-probability of ONE complete alignment path, so it cannot exceed the
        lattice total: -transducer_forward_score(joint, hyp) >= score - 1e-9
    fixture conditions: the smallest free-argmax gap is >= 1e-3 -- ten times the project's fp32-grade tolerance on features (SURVEY.md
        8d), so the GPU's split-bf16 arithmetic cannot flip a token; the fixtures hold an empty hypothesis, two emissions at one frame,
        a forced blank, a truncated row and a row ended by its length; at most a third of the property fixture's rows are truncated
"""
import pytest
import torch

import rnnt_greedy_ref as R
from oracle import star_ref

NAMES = sorted(R.FIXTURES)


def path_moves(hyp, frames):
    """The moves of the alignment path (frames of the emissions, blanks between them, forced blanks under the cap) of a row:
    -> [(t, u, k, free)] in order, and where it stands."""
    moves, t, here = [], 0, 0
    for u, (k, ft) in enumerate(zip(hyp.tolist(), frames.tolist())):
        while t < ft:
            moves.append((t, u, 0, here != R.MAX_SYMBOLS))
            t, here = t + 1, 0
        moves.append((t, u, k, True))
        here += 1
    return moves, t, here


@pytest.mark.parametrize('name', NAMES)
def test_path_is_greedy_and_sums_to_the_score(name):
    sd, features, il, capacity, ref = R.fixture(name)
    T = features.shape[1]
    for n in range(features.shape[0]):
        U, L = int(ref['lengths'][n]), min(int(il[n]), T)
        hyp, frames = ref['tokens'][n, :U], ref['frames'][n, :U]
        assert (ref['tokens'][n, U:] == -1).all() and (ref['frames'][n, U:] == -1).all()
        joint = R.teacher_forced_joint(sd, features[n], hyp)
        moves, t, here = path_moves(hyp, frames)
        if not ref['truncated'][n]:                       # ended by its length: blanks to the last frame
            while t < L:
                moves.append((t, U, 0, here != R.MAX_SYMBOLS))
                t, here = t + 1, 0
        total = 0.0
        for (t_, u_, k, free) in moves:
            assert t_ < L
            if free:
                assert int(joint[t_, u_].argmax()) == k, (name, n, t_, u_)
            total += float(joint[t_, u_, k])
        assert abs(total - float(ref['scores'][n])) <= 1e-9, (name, n)
        assert bool(ref['truncated'][n]) == (U == capacity)


@pytest.mark.parametrize('name', NAMES)
def test_score_is_below_the_lattice_total(name):
    sd, features, il, capacity, ref = R.fixture(name)
    T = features.shape[1]
    for n in range(features.shape[0]):
        U, L = int(ref['lengths'][n]), min(int(il[n]), T)
        if ref['truncated'][n] or L == 0:
            continue
        hyp = ref['tokens'][n, :U]
        joint = R.teacher_forced_joint(sd, features[n], hyp)
        loss = star_ref.transducer_forward_score(joint[None], hyp[None], torch.tensor([L], dtype=torch.int32),
                                                 torch.tensor([U], dtype=torch.int32))
        assert -float(loss[0]) >= float(ref['scores'][n]) - 1e-9, (name, n)


def test_fixture_conditions():
    kinds = dict(empty=0, two_at_one_frame=0, forced_blank=0, truncated=0, ended_by_length=0)
    for name in NAMES:
        sd, features, il, capacity, ref = R.fixture(name)
        assert ref['gap'] >= 1e-3, (name, ref['gap'])
        for n in range(features.shape[0]):
            U = int(ref['lengths'][n])
            fr = ref['frames'][n, :U]
            kinds['empty'] += U == 0
            kinds['two_at_one_frame'] += bool(U >= 2 and (fr[1:] == fr[:-1]).any())
            kinds['forced_blank'] += int(ref['forced'][n]) > 0
            kinds['truncated'] += bool(ref['truncated'][n])
            kinds['ended_by_length'] += not bool(ref['truncated'][n])
    assert all(v > 0 for v in kinds.values()), kinds
    ref = R.fixture('rows17')[4]
    assert int(ref['truncated'].sum()) * 3 <= len(ref['truncated'])
    assert int((R.fixture('rows17')[2] == 0).sum()) == 1                 # one row of length 0
    assert not R.fixture('rows17_long')[4]['truncated'].any()            # capacity 2 T: every row ends by its length
    assert R.fixture('small')[2].tolist() == [12, 9, 1]
