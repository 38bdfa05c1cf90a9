"""GPU tests of transducer beam search with LM shallow fusion (haloop_amd.fusion.TransducerFusionDecoder,
recognizer.Transducer.set_fusion_lm, csrc/rnnt_lm_beam.hip) against the float64 restatement on the CPU (tests/rnnt_lm_beam_ref.py), in
`bf16x3` unless said otherwise.

Tokens, lengths and counts must equal the restatement exactly on every row the case does not leave out: tests/test_rnnt_lm_beam_cpu.py
asserts on the CPU that every prune and every final ranking of those rows was decided by a gap of at least 1e-3.  The three scores: rtol
1e-5 / atol 1e-4, the bound of tests/test_gpu_rnnt_beam.py and tests/test_gpu_ctc_lm_beam.py for the same cell launches in the same mode.

Which case reaches which route of the step kernel: 'wide' (V = 1031: above the workgroup, no multiple of 64; 2 W V = 6186 floats) and
every smaller V keep both tables in LDS; 'stream' (V = 4099, W = 3: 2 W V above 14336 floats) recomputes both from L2 in every round;
'rows17' at W = 8 runs a one-layer LM under the two-layer prediction network; 'tiny' prunes nothing.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

import rnnt_beam_ref as B
import rnnt_lm_beam_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SMALL, SMALL1, TINY, ROWS17, ROWS17W8, WIDE, STREAM = R.CASES


@contextlib.contextmanager
def math_mode(mode):
    from haloop_amd import _lib
    _lib.lib()
    prev = _lib.get_math_mode()
    _lib.set_math_mode(mode)
    try:
        yield
    finally:
        _lib.set_math_mode(prev)


@pytest.fixture(autouse=True)
def bf16x3():
    with math_mode('bf16x3'):
        yield


def close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4, err_msg=what)


def head_of(sd):
    from haloop_amd import recognizer
    head = recognizer.Transducer(sd['classifier.weight'].shape[1], sd['classifier.weight'].shape[0]).eval()
    head.load_state_dict(sd)
    return head.to(DEV)


def check(got, parts, ref, rows, what):
    tokens, lengths, scores, counts = (x.cpu() for x in got)
    rnnt_scores, lm_scores = (x.cpu() for x in parts)
    assert tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and counts.dtype == torch.int64
    assert scores.dtype == rnnt_scores.dtype == lm_scores.dtype == torch.float32
    assert tokens.shape == ref['tokens'].shape and lengths.shape == ref['lengths'].shape
    assert scores.shape == rnnt_scores.shape == lm_scores.shape == ref['scores'].shape
    rows = list(rows)
    present = ref['lengths'][rows] >= 0
    named = (('scores', scores), ('rnnt_scores', rnnt_scores), ('lm_scores', lm_scores))
    errs = {k: float((v[rows].double() - ref[k][rows])[present].abs().max()) for k, v in named}
    print(what, 'best lengths', lengths[:, 0].tolist(), 'counts', counts.tolist(), 'max |error|', errs)
    assert torch.equal(counts[rows], ref['counts'][rows]), what
    assert torch.equal(lengths[rows], ref['lengths'][rows]), what
    assert torch.equal(tokens[rows], ref['tokens'][rows]), what
    for k, v in named:
        close(v[rows].numpy(), ref[k][rows].numpy(), f'{what} {k}')


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def decoder_for(case, max_batch=None):
    from haloop_amd import fusion
    name, W, layers, seed, a, b = case
    sd, features, il, capacity, lm, ref = R.fixture(case)
    dec = fusion.TransducerFusionDecoder(head_of(sd), copy.deepcopy(lm).to(DEV), max_batch or features.shape[0], capacity, W, a, b)
    return dec, features.to(DEV), il.to(DEV), ref


def decode(dec, *args, **kwargs):
    out = dec.decode(*args, **kwargs)
    return out, dec.last_parts


@pytest.mark.parametrize('case', R.CASES)
def test_case_equals_the_restatement(case):
    dec, x, il, ref = decoder_for(case)
    assert dec.fused
    got, parts = decode(dec, x, il)
    check(got, parts, ref, R.compared_rows(case), str(case))
    assert 1 <= dec.iterations <= int(il.max()) + dec.capacity
    for n in range(x.shape[0]):                                         # a row of length 0 gives the empty hypothesis alone
        if int(il[n]) == 0:
            assert int(got[3][n]) == 1 and int(got[1][n, 0]) == 0 and got[1][n, 1:].eq(-1).all() and got[0][n].eq(-1).all()
            assert float(got[2][n, 0]) == 0.0 and float(parts[0][n, 0]) == 0.0 and float(parts[1][n, 0]) == 0.0
            assert got[2][n, 1:].eq(R.NEG).all()
    if case[0] == 'rows17':
        assert 0 in il.tolist()
        if case[1] == 8:
            assert dec.lm.num_layers == 1 and dec.head.lm.num_layers == 2


@pytest.mark.parametrize('case', [SMALL, ROWS17, ROWS17W8, WIDE, STREAM])
def test_zero_weights_are_the_unfused_search_on_the_device(case):
    from haloop_amd import transducer
    dec, x, il, ref = decoder_for(case)
    got = dec.decode(x, il, lm_weight=0.0, insertion_bonus=0.0)
    want = transducer.BeamDecoder(dec.head, x.shape[0], dec.capacity, case[1]).decode(x, il)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
    present = want[1] >= 0
    print(case, 'max |score difference|', float((got[2] - want[2])[present].abs().max()),
          'max |rnnt_scores difference|', float((dec.last_parts[0] - want[2])[present].abs().max()))
    close(got[2].cpu().numpy(), want[2].cpu().numpy(), str(case))
    close(dec.last_parts[0].cpu().numpy(), want[2].cpu().numpy(), str(case))


@pytest.mark.parametrize('case', [ROWS17, ROWS17W8])
def test_lm_scores_agree_with_a_teacher_forced_pass(case):
    from haloop_amd import fusion
    dec, x, il, ref = decoder_for(case)
    got, parts = decode(dec, x, il)
    want = fusion.lm_score(dec.lm, got[0], got[1])
    assert want.shape == parts[1].shape and want.dtype == torch.float32
    assert torch.equal(want == R.NEG, got[1] < 0)
    print(case, 'max |lm_scores - lm_score|', float((parts[1] - want)[got[1] >= 0].abs().max()))
    close(parts[1].cpu().numpy(), want.cpu().numpy(), str(case))
    rows = R.compared_rows(case)
    close(want.cpu().numpy()[rows], ref['lm_scores'][rows].numpy(), f'{case} lm_score against float64')


def test_without_pruning_rnnt_scores_equal_the_training_loss():
    """N = 2, T = 5, V = 4, cap = 2, W = 16: nothing is pruned, so every rnnt_score is -transducer_loss of the head's own training-path
    operators on f and the teacher-forced g of the returned tokens."""
    from haloop_amd import functional as HF, transducer
    dec, x, il, ref = decoder_for(TINY)
    (tokens, lengths, scores, counts), parts = decode(dec, x, il)
    check((tokens, lengths, scores, counts), parts, ref, R.compared_rows(TINY), str(TINY))
    assert counts.tolist() == [13, 13]
    head = dec.head
    with torch.no_grad():
        hyp = tokens[:, :13].reshape(26, -1).clamp(min=0)                 # (-1 past a hypothesis's length: never read by the lattice)
        hl = lengths[:, :13].reshape(26)
        rows = torch.arange(2, device=DEV).repeat_interleave(13)
        lm_in = torch.cat([hyp.new_zeros((26, 1)), hyp], dim=1)
        g, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(26))
        f = HF.linear(x[rows].float(), head.classifier.weight, head.classifier.bias)
        losses = transducer.transducer_loss(f, g, hyp, il[rows], hl)
    print('max |rnnt_score + loss|', float((parts[0][:, :13].reshape(26) + losses).abs().max()))
    close(parts[0][:, :13].reshape(26).cpu().numpy(), -losses.cpu().numpy(), 'tiny')


@pytest.mark.parametrize('case', [SMALL, ROWS17])
def test_padding_is_never_read(case):
    dec, x, il, ref = decoder_for(case)
    clean, parts = decode(dec, x, il)
    check(clean, parts, ref, R.compared_rows(case), str(case))
    poisoned = x.clone()
    for n, L in enumerate(il.tolist()):
        poisoned[n, L:] = float('nan')                                  # frames at or past the row's length
    got, got_parts = decode(dec, poisoned, il)
    assert same(got, clean) and same(got_parts, parts)


@pytest.mark.parametrize('case', [ROWS17W8, STREAM])
def test_two_identical_calls_are_bit_equal(case):
    dec, x, il, ref = decoder_for(case)
    first, first_parts = decode(dec, x, il)
    again, again_parts = decode(dec, x, il)
    assert same(first, again) and same(first_parts, again_parts)


def test_a_reused_decoder_repeats_itself_and_follows_the_parameters():
    """N = 17, then 3 rows at another width and capacity, then 17 again; then a parameter of each network changed in place."""
    from haloop_amd import fusion
    case = ROWS17W8
    dec, x, il, ref = decoder_for(case)
    first, first_parts = decode(dec, x, il)
    check(first, first_parts, ref, R.compared_rows(case), str(case))
    x3, il3 = x[3:6, :12].contiguous(), torch.tensor([12, 9, 1], device=DEV)
    three, three_parts = decode(dec, x3, il3, capacity=5, beam=4)
    fresh = fusion.TransducerFusionDecoder(dec.head, dec.lm, 3, 5, 4, case[4], case[5])
    want, want_parts = decode(fresh, x3, il3)
    assert same(three, want) and same(three_parts, want_parts)
    third, third_parts = decode(dec, x, il)
    assert same(first, third) and same(first_parts, third_parts)
    with torch.no_grad():                                               # the LM: a stale decode image would repeat the old result
        g = torch.Generator().manual_seed(3)
        dec.lm.out_layer.bias.add_(2.0 * torch.randn(67, generator=g).to(DEV))
        dec.lm.rnn.weight_hh_l0.mul_(0.5)
    changed, changed_parts = decode(dec, x, il)
    fresh = fusion.TransducerFusionDecoder(dec.head, dec.lm, 17, dec.capacity, 8, case[4], case[5])
    want, want_parts = decode(fresh, x, il)
    assert same(changed, want) and same(changed_parts, want_parts)
    assert not torch.equal(changed_parts[1], first_parts[1])
    with torch.no_grad():                                               # the prediction network
        dec.head.lm.rnn.weight_hh_l0.mul_(0.5)
    moved, moved_parts = decode(dec, x, il)
    fresh = fusion.TransducerFusionDecoder(dec.head, dec.lm, 17, dec.capacity, 8, case[4], case[5])
    want, want_parts = decode(fresh, x, il)
    assert same(moved, want) and same(moved_parts, want_parts)
    assert not torch.equal(moved_parts[0], changed_parts[0])


@pytest.mark.parametrize('case', [SMALL, ROWS17W8])
def test_the_general_path_agrees(case, monkeypatch):
    dec, x, il, ref = decoder_for(case)
    fused, fused_parts = decode(dec, x, il)
    monkeypatch.setenv('HALO_RNNT_FUSED', '0')
    assert not dec.fused
    general, general_parts = decode(dec, x, il)
    rows = R.compared_rows(case)
    check(general, general_parts, ref, rows, f'{case} general')
    assert all(torch.equal(a[rows], b[rows]) for a, b in zip((fused[0], fused[1], fused[3]), (general[0], general[1], general[3])))
    for a, b in zip((fused[2],) + fused_parts, (general[2],) + general_parts):
        close(a[rows].cpu().numpy(), b[rows].cpu().numpy(), str(case))


@pytest.mark.parametrize('mode,hidden', [('bf16x3', 64), ('f32', 512)])
def test_the_general_path_serves_what_the_fused_cells_refuse(mode, hidden):
    """An LM with H = 64, and `f32` mode: against the restatement on that LM (this test's own fixture condition: the rows of 'small' that
    decide by GAP or more, at least two of the three)."""
    from haloop_amd import fusion
    W, a, b = 4, 0.5, 1.5
    sd, features, il, capacity = B.inputs('small')
    lm = R.make_lm(20, 2, 1, hidden, hidden)
    ref = R.beam_search(sd, features, il, capacity, W, R.LM64(lm), a, b)
    rows = [n for n in range(3) if float(ref['gaps'][n]) >= R.GAP]
    assert len(rows) >= 2
    with math_mode(mode):
        dec = fusion.TransducerFusionDecoder(head_of(sd), copy.deepcopy(lm).to(DEV), 3, capacity, W, a, b)
        assert not dec.fused
        got, parts = decode(dec, features.to(DEV), il.to(DEV))
    check(got, parts, ref, rows, f'general path, {mode}, H = {hidden}')


def test_transducer_set_fusion_lm():
    from haloop_amd import fusion
    case = SMALL
    sd, features, il, capacity, lm, ref = R.fixture(case)
    head, lm = head_of(sd), copy.deepcopy(lm).to(DEV)
    x, ild = features.to(DEV), il.to(DEV)
    ct = torch.tensor([capacity - 1, 2, 1])                             # capacity = condtarget_lengths.max() + 1
    keys, count = list(head.state_dict()), len(list(head.parameters()))
    before_greedy, before_beam = head.decode(x, ild, ct), head.decode(x, ild, ct, beam_size=4)
    plain_nbest = head.last_nbest
    assert head.last_parts is None

    head.set_fusion_lm(lm, case[4], case[5])
    assert list(head.state_dict()) == keys and len(list(head.parameters())) == count
    out = head.decode(x, ild, ct, beam_size=4)
    assert len(out) == 5
    hypotheses, output_lengths, alignments, scores, nothing = out
    assert nothing is None and alignments == [None] * 3 and hypotheses.is_nested
    want, want_parts = decode(fusion.TransducerFusionDecoder(head, lm, 3, capacity, 4, case[4], case[5]), x, ild)
    assert same(head.last_nbest, want) and same(head.last_parts, want_parts)
    check(head.last_nbest, head.last_parts, ref, R.compared_rows(case), 'last_nbest')
    assert output_lengths.tolist() == want[1][:, 0].tolist() and torch.equal(scores, want[2][:, 0])
    for n, hyp in enumerate(hypotheses.unbind()):
        assert torch.equal(hyp, want[0][n, 0, :int(want[1][n, 0])])
    assert not same(head.last_nbest, plain_nbest)                        # the LM changed the lists
    greedy = head.decode(x, ild, ct)                                    # greedy stays the default, and does not use the LM
    assert all(torch.equal(a, b) for a, b in zip(greedy[1:4], before_greedy[1:4]))
    for a, b in zip(greedy[0].unbind(), before_greedy[0].unbind()):
        assert torch.equal(a, b)
    head.train()
    with pytest.raises(NotImplementedError):
        head.decode(x, ild, ct, beam_size=4)
    head.eval()
    lm.train()
    with pytest.raises(NotImplementedError):
        head.decode(x, ild, ct, beam_size=4)
    lm.eval()

    head.set_fusion_lm(None)
    after = head.decode(x, ild, ct, beam_size=4)
    assert same(head.last_nbest, plain_nbest) and head.last_parts is None
    assert torch.equal(after[3], before_beam[3]) and after[1].tolist() == before_beam[1].tolist()
    for a, b in zip(after[0].unbind(), before_beam[0].unbind()):
        assert torch.equal(a, b)
