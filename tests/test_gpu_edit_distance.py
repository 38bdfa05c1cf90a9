"""GPU checks of haloop_amd.wer.edit_distance (csrc/edit_distance.hip) against the plain-Python yardstick tests/edit_distance_ref.py
(tests/test_edit_distance_cpu.py validates the yardstick).  Integers: errors and counts are compared exactly.

The launch picks its kernel by the width of the reference tensor (one wave up to 64 columns, then 256 threads with 1, 2 or 4 columns
each), so the length grid is launched once per reference width -- widths 63 / 64 / 65 sit on the boundary of the two forms -- and once
more with every pair in one wide tensor.  A 5-symbol alphabet makes matches and ties common."""
import itertools

import pytest
import torch

import edit_distance_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LENGTHS = (0, 1, 2, 31, 63, 64, 65, 127, 129)
BOUND = 1024


def sequences(lengths, seed, symbols=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, symbols, (n,), generator=g).tolist() for n in lengths]


def padded(rows, width, pad=-1):
    return torch.tensor([r + [pad] * (width - len(r)) for r in rows], dtype=torch.int64).view(len(rows), width)


def run(hyp, hyp_len, ref, ref_len, group=1):
    from haloop_amd import wer
    errors, counts = wer.edit_distance(hyp.to(DEV), torch.tensor(hyp_len).to(DEV), ref.to(DEV), torch.tensor(ref_len).to(DEV), group)
    assert errors.dtype == torch.int32 and counts.dtype == torch.int32 and counts.shape == (errors.shape[0], 3)
    return errors.tolist(), counts.tolist()


def check(hyps, refs, hyp_width, ref_width, group=1):
    """hyps [P], refs [R] token lists -> launch at the given tensor widths and compare with the yardstick."""
    hyp_len, ref_len = [len(h) for h in hyps], [len(r) for r in refs]
    got = run(padded(hyps, hyp_width), hyp_len, padded(refs, ref_width), ref_len, group)
    want = R.batch(hyps, hyp_len, refs, ref_len, group)
    assert got[0] == want[0]
    assert got[1] == want[1]
    return got


@pytest.mark.parametrize('ref_length', LENGTHS)
def test_length_grid_at_each_reference_width(ref_length):
    hyps = sequences(LENGTHS, 100 + ref_length)
    refs = sequences([ref_length] * len(LENGTHS), 200 + ref_length)
    check(hyps, refs, max(LENGTHS), ref_length)


def test_length_grid_in_one_wide_launch():
    pairs = list(itertools.product(LENGTHS, LENGTHS))
    hyps, refs = sequences([a for a, _ in pairs], 1), sequences([b for _, b in pairs], 2)
    check(hyps, refs, max(LENGTHS), max(LENGTHS))


def test_mixed_reference_lengths_in_the_one_wave_form():
    pairs = list(itertools.product(LENGTHS, [n for n in LENGTHS if n <= 64]))
    hyps, refs = sequences([a for a, _ in pairs], 3), sequences([b for _, b in pairs], 4)
    check(hyps, refs, max(LENGTHS), 64)


@pytest.mark.parametrize('length', [BOUND, BOUND // 2])
def test_pair_at_the_bound_and_at_half_of_it(length):
    hyps, refs = sequences([length], 5 + length), sequences([length], 6 + length)
    check(hyps, refs, length, length)


def test_equal_and_all_different_sequences():
    seqs = sequences([1, 40, 64, 65, 200], 7)
    got = check(seqs, seqs, 200, 200)
    assert got[0] == [0] * 5
    other = [[t + 5 for t in s[:n]] for s, n in zip(seqs, (1, 33, 64, 70, 129))]        # no symbol in common; lengths differ too
    other[3] = other[3] + [9] * 5
    got = check(other, seqs, 200, 200)
    assert got[0] == [max(len(a), len(b)) for a, b in zip(other, seqs)]


def test_groups_and_absent_hypotheses():
    refs = sequences([12, 0, 70], 8)
    hyps = sequences([11, 12, 0, 3, 0, 0, 70, 64, 0], 9)
    hyp_len = [11, 12, -1, 3, -1, 0, 70, 64, -1]
    hyp, ref = padded(hyps, 70), padded(refs, 70)
    got = run(hyp, hyp_len, ref, [12, 0, 70], group=3)
    want = R.batch(hyps, hyp_len, refs, [12, 0, 70], group=3)
    assert got[0] == want[0] and got[1] == want[1]
    for p in (2, 4, 8):
        assert got[0][p] == -1 and got[1][p] == [0, 0, 0]
    # the [N, W, capacity] layout of the beam search is taken as N * W rows
    from haloop_amd import wer
    e3, c3 = wer.edit_distance(hyp.view(3, 3, 70).to(DEV), torch.tensor(hyp_len).view(3, 3).to(DEV), ref.to(DEV), torch.tensor([12, 0, 70]).to(DEV), 3)
    assert e3.tolist() == got[0] and c3.tolist() == got[1]


@pytest.mark.parametrize('width', [64, 129])
def test_padding_is_never_read_as_a_token(width):
    lengths = [n for n in LENGTHS if n <= width]
    hyps, refs = sequences(lengths, 10), sequences(list(reversed(lengths)), 11)
    hyp_len, ref_len = [len(h) for h in hyps], [len(r) for r in refs]
    a = run(padded(hyps, width), hyp_len, padded(refs, width), ref_len)
    b = run(padded(hyps, width, pad=3), hyp_len, padded(refs, width, pad=3), ref_len)
    assert a == b
    want = R.batch(hyps, hyp_len, refs, ref_len)
    assert a[0] == want[0] and a[1] == want[1]


def test_strided_hypotheses_give_the_same_bits():
    from haloop_amd import wer
    lengths = [5, 64, 65, 100]
    hyps, refs = sequences(lengths, 12), sequences([90, 64, 3, 100], 13)
    hyp, ref = padded(hyps, 100).to(DEV), padded(refs, 100).to(DEV)
    hl, rl = torch.tensor(lengths).to(DEV), torch.tensor([90, 64, 3, 100]).to(DEV)
    wide = torch.full((4, 260), 4, dtype=torch.int64, device=DEV)
    wide[:, 7:107] = hyp
    view = wide[:, 7:107]
    assert not view.is_contiguous()
    a, b = wer.edit_distance(hyp, hl, ref, rl), wer.edit_distance(view, hl, ref, rl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want = R.batch(hyps, lengths, refs, [90, 64, 3, 100])
    assert a[0].tolist() == want[0] and a[1].tolist() == want[1]


def test_a_length_above_the_bound_raises():
    from haloop_amd import _lib, ops, wer
    assert ops.EDIT_DISTANCE_MAX_LEN == BOUND
    one = torch.tensor([1]).to(DEV)
    short, long_ = torch.zeros(1, 4, dtype=torch.int64, device=DEV), torch.zeros(1, BOUND + 1, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.HaloError):
        wer.edit_distance(long_, one, short, one)
    with pytest.raises(_lib.HaloError):
        wer.edit_distance(short, one, long_, one)


def test_nbest_oracle_and_word_errors():
    from haloop_amd import wer
    errors = torch.tensor([[3, 1, 1, -1], [-1, -1, -1, -1], [-1, 0, 2, 0]], dtype=torch.int32, device=DEV)
    best, index = wer.nbest_oracle(errors)
    assert best.tolist() == [1, -1, 0] and index.tolist()[0] == 1 and index.tolist()[2] == 1
    refs = [('u1', 'the cat ␣ sat down'), ('u2', 'hello'), ('u3', 'unmatched')]
    hyps = [('u2', 'hello there'), ('u1', 'the bat sat')]
    rows = wer.word_errors(refs, hyps)
    assert rows == [{'key': 'u1', 'ins': 0, 'del': 1, 'sub': 1, 'total': 2, 'ref_length': 4, 'hyp_length': 3},
                    {'key': 'u2', 'ins': 1, 'del': 0, 'sub': 0, 'total': 1, 'ref_length': 1, 'hyp_length': 2}]
    assert wer.format_wer(rows) == ('%WER', 60.0, 'errors=3/5', 'ins=1', 'del=1', 'sub=1')
    rows = wer.word_errors([('u', '▁the ▁c at')], [('u', '▁the ▁ca t ▁s at')], join_bpe=True)
    assert rows[0]['total'] == 1 and rows[0]['ins'] == 1 and rows[0]['ref_length'] == 2
