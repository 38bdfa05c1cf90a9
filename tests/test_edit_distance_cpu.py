"""CPU checks of the yardstick tests/edit_distance_ref.py (what tests/test_gpu_edit_distance.py and tests/test_gpu_mwer.py compare the
launches of csrc/edit_distance.hip with) and of the host side of haloop_amd.wer.  No device, no library call."""
import functools
import itertools
import random

import torch

import edit_distance_ref as R


def recursion(hyp, ref):
    """The error count by the textbook recursion on suffixes, memoised: independent of the yardstick's table walk."""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == len(hyp):
            return len(ref) - j
        if j == len(ref):
            return len(hyp) - i
        return min(d(i + 1, j + 1) + (hyp[i] != ref[j]), d(i + 1, j) + 1, d(i, j + 1) + 1)
    return d(0, 0)


def check_pair(hyp, ref):
    errors, (ins, del_, sub) = R.edit_distance(hyp, ref)
    assert errors == recursion(tuple(hyp), tuple(ref)), (hyp, ref)
    assert ins + del_ + sub == errors, (hyp, ref)
    assert len(hyp) - ins == len(ref) - del_, (hyp, ref)
    assert min(ins, del_, sub) >= 0, (hyp, ref)


def test_errors_match_the_recursion_on_every_short_pair():
    seqs = [s for n in range(5) for s in itertools.product('abc', repeat=n)]
    assert len(seqs) == 121
    for hyp in seqs:
        for ref in seqs:
            check_pair(hyp, ref)


def test_errors_match_the_recursion_on_random_pairs():
    rng = random.Random(5)
    for _ in range(300):
        hyp = [rng.randrange(4) for _ in range(rng.randrange(13))]
        ref = [rng.randrange(4) for _ in range(rng.randrange(13))]
        check_pair(hyp, ref)


def test_tie_order_on_hand_made_pairs():
    # ab against ba: two substitutions (the diagonal twice), not the insertion + deletion of equal cost
    assert R.edit_distance('ab', 'ba') == (2, (0, 0, 2))
    # a against aa: cell (1, 2) gets 1 from the diagonal (0, 1) and from the deletion (1, 1); the diagonal is kept
    assert R.edit_distance('a', 'aa') == (1, (0, 1, 0))
    assert R.edit_distance('aa', 'a') == (1, (1, 0, 0))
    assert R.edit_distance('ab', 'b') == (1, (1, 0, 0))
    assert R.edit_distance('', 'abc') == (3, (0, 3, 0))
    assert R.edit_distance('abc', '') == (3, (3, 0, 0))
    assert R.edit_distance('', '') == (0, (0, 0, 0))


def backtrace(hyp, ref):
    """The tie rule read the other way round: the plain cost table, then a walk back from (Lh, Lr) that takes, at every cell, the first of
    diagonal, deletion, insertion that explains the cell's cost."""
    lh, lr = len(hyp), len(ref)
    D = [[i + j if i == 0 or j == 0 else 0 for j in range(lr + 1)] for i in range(lh + 1)]
    for i in range(1, lh + 1):
        for j in range(1, lr + 1):
            D[i][j] = min(D[i - 1][j - 1] + (hyp[i - 1] != ref[j - 1]), D[i][j - 1] + 1, D[i - 1][j] + 1)
    i, j, ins, del_, sub = lh, lr, 0, 0, 0
    while i or j:
        if i and j and D[i - 1][j - 1] + (hyp[i - 1] != ref[j - 1]) == D[i][j]:
            sub += hyp[i - 1] != ref[j - 1]; i -= 1; j -= 1
        elif j and D[i][j - 1] + 1 == D[i][j]:
            del_ += 1; j -= 1
        else:
            ins += 1; i -= 1
    return D[lh][lr], (ins, del_, sub)


def test_forward_counts_are_those_of_the_backtraced_path():
    """Carrying the counts forward with the cost gives the counts of the path a backtrace under the same order walks (include/halo.h)."""
    seqs = [s for n in range(5) for s in itertools.product('abc', repeat=n)]
    for hyp in seqs:
        for ref in seqs:
            assert R.edit_distance(hyp, ref) == backtrace(hyp, ref), (hyp, ref)
    rng = random.Random(11)
    for _ in range(300):
        hyp = [rng.randrange(3) for _ in range(rng.randrange(13))]
        ref = [rng.randrange(3) for _ in range(rng.randrange(13))]
        assert R.edit_distance(hyp, ref) == backtrace(hyp, ref), (hyp, ref)


def test_batch_groups_and_absent_rows():
    hyp = [[1, 2, -1], [1, -1, -1], [-1, -1, -1], [3, 3, 3]]
    errors, counts = R.batch(hyp, [2, 1, -1, 3], [[1, 2], [3, 4]], [2, 1], group=2)
    assert errors == [0, 1, -1, 2]
    assert counts == [[0, 0, 0], [0, 1, 0], [0, 0, 0], [2, 0, 0]]


def risk_inputs(N, W, seed):
    g = torch.Generator().manual_seed(seed)
    losses = (20 + 5 * torch.randn(N, W, generator=g)).float()
    errors = torch.randint(0, 9, (N, W), generator=g, dtype=torch.int32)
    return losses, errors


def test_risk_gradient_matches_autograd():
    for W in (1, 3, 16):
        losses, errors = risk_inputs(5, W, W)
        if W > 1:
            errors[1, 1] = -1                               # a row with an absent entry
            errors[2, 1:] = -1                              # a row with one hypothesis
            errors[3, :] = -1                               # a row with nothing
        l = losses.double().requires_grad_(True)
        risk = R.nbest_risk(l, errors)
        weights = torch.arange(1, 6, dtype=torch.float64)
        (risk * weights).sum().backward()
        closed = R.nbest_risk_grad(losses, errors) * weights[:, None]
        assert torch.allclose(l.grad, closed, rtol=1e-12, atol=1e-14), W
        single = (errors >= 0).sum(1) == 1
        assert single.any()
        assert (risk[single] == 0).all() and (l.grad[single] == 0).all()
        if W > 1:
            assert risk[3] == 0 and (l.grad[3] == 0).all()
            assert (l.grad[errors < 0] == 0).all()


def test_risk_is_expected_error_less_the_mean():
    losses = torch.tensor([[1.0, 1.0, 50.0]])
    errors = torch.tensor([[2, 4, 9]], dtype=torch.int32)
    assert abs(float(R.nbest_risk(losses, errors)[0]) - (3.0 - 5.0)) < 1e-12


def test_wer_text_helpers():
    from haloop_amd import wer
    assert wer.clean_tokens('the ␣ cat  ␣ sat') == 'the cat sat'
    assert wer.clean_and_join_tokens('▁the ▁c at ␣ ▁s at') == ' the cat sat'
    assert wer.clean_and_join_tokens('▁the ▁c at ␣ ▁s at').split() == ['the', 'cat', 'sat']
    refs = [('u1', 'a b ␣ c'), ('u2', 'd'), ('u3', 'x')]
    hyps = [('u2', 'd e'), ('u1', 'a c'), ('u9', 'q')]
    keys, (ref_tok, ref_len), (hyp_tok, hyp_len) = wer._word_ids(refs, hyps, False)
    assert keys == ['u1', 'u2'] and ref_len == [3, 1] and hyp_len == [2, 2]
    assert ref_tok == [[0, 1, 2], [3, -1, -1]] and hyp_tok == [[0, 2], [3, 4]]
    keys, (ref_tok, ref_len), (hyp_tok, hyp_len) = wer._word_ids([('u', '▁a b ▁c')], [('u', '▁ab ▁c')], True)
    assert ref_tok == hyp_tok == [[0, 1]] and ref_len == hyp_len == [2]
    rows = [{'ins': 1, 'del': 0, 'sub': 2, 'total': 3, 'ref_length': 7, 'hyp_length': 8},
            {'ins': 0, 'del': 1, 'sub': 0, 'total': 1, 'ref_length': 5, 'hyp_length': 4}]
    assert wer.format_wer(rows) == ('%WER', 33.33, 'errors=4/12', 'ins=1', 'del=1', 'sub=2')
    assert wer.format_wer(rows, tag='CER')[0] == '%CER'


def test_wer_refuses_cpu_tensors():
    import pytest
    from haloop_amd import _lib, transducer, wer
    with pytest.raises(_lib.HaloError):
        wer.edit_distance(torch.zeros(1, 2, dtype=torch.int64), torch.tensor([2]), torch.zeros(1, 2, dtype=torch.int64), torch.tensor([2]))
    with pytest.raises(_lib.HaloError):
        transducer.nbest_risk(torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int32))
    assert 'wer' in __import__('haloop_amd').__all__
