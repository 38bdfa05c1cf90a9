"""GPU tests of CTC prefix beam search with LM shallow fusion (haloop_amd.fusion.CTCFusionDecoder and lm_score,
recognizer.TemporalClassifier.set_lm, csrc/ctc_lm_beam.hip) against the float64 restatement on the CPU (tests/ctc_lm_beam_ref.py), in
`bf16x3` unless said otherwise.

Tokens, lengths and counts must equal the restatement exactly on every row the case does not leave out: tests/test_ctc_lm_beam_cpu.py
asserts on the CPU that every prune and every final ranking of those rows was decided by a gap of at least 1e-3.  The three scores: rtol
1e-5 / atol 1e-4, the bound of tests/test_gpu_rnnt_beam.py for the same cell launches in the same mode.

Which case reaches which route of the step kernel: 'wide' (V = 300: above the workgroup, no multiple of 64) and every smaller V keep the
row's W V logits in LDS; 'stream' (V = 4100, W = 3: (W + 1) V above 14336 floats) recomputes them from L2 in every round; 'rows17cap'
refuses extensions at the capacity and runs a one-layer LM; 'long' runs the frame loop through both parities 35 times.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

import ctc_lm_beam_ref as R
import ctc_prefix_beam_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'


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


def check(got, parts, ref, rows, what):
    tokens, lengths, scores, counts = (x.cpu() for x in got)
    ctc_scores, lm_scores = (x.cpu() for x in parts)
    assert tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and counts.dtype == torch.int64
    assert scores.dtype == ctc_scores.dtype == lm_scores.dtype == torch.float32
    assert tokens.shape == ref['tokens'].shape and lengths.shape == ref['lengths'].shape
    assert scores.shape == ctc_scores.shape == lm_scores.shape == ref['scores'].shape
    rows = list(rows)
    present = ref['lengths'][rows] >= 0
    errs = {k: float((v[rows].double() - ref[k][rows])[present].abs().max())
            for k, v in (('scores', scores), ('ctc_scores', ctc_scores), ('lm_scores', lm_scores))}
    print(what, 'best lengths', lengths[:, 0].tolist(), 'counts', counts.tolist(), 'max |error|', errs,
          'largest |lm score|', float(ref['lm_scores'][rows][present].abs().max()))
    assert torch.equal(counts[rows], ref['counts'][rows]), what
    assert torch.equal(lengths[rows], ref['lengths'][rows]), what
    assert torch.equal(tokens[rows], ref['tokens'][rows]), what
    for k, v in (('scores', scores), ('ctc_scores', ctc_scores), ('lm_scores', lm_scores)):
        close(v[rows].numpy(), ref[k][rows].numpy(), f'{what} {k}')


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def decoder_for(case, max_batch=None):
    from haloop_amd import fusion
    name, W, layers, seed, a, b = case
    e, il, capacity, lm, ref = R.fixture(case)
    dec = fusion.CTCFusionDecoder(copy.deepcopy(lm).to(DEV), max_batch or e.shape[1], capacity, W, a, b)
    return dec, e.to(DEV), il.to(DEV), ref


def decode(dec, *args, **kwargs):
    out = dec.decode(*args, **kwargs)
    return out, dec.last_parts


@pytest.mark.parametrize('case', R.CASES)
def test_case_equals_the_restatement(case):
    dec, e, il, ref = decoder_for(case)
    assert dec.fused
    got, parts = decode(dec, e, il)
    check(got, parts, ref, R.compared_rows(case), str(case))
    assert dec.iterations == max(1, int(il.max()))
    for n in range(e.shape[1]):                                         # a row of length 0 gives the empty hypothesis alone
        if int(il[n]) == 0:
            assert int(got[3][n]) == 1 and int(got[1][n, 0]) == 0 and got[1][n, 1:].eq(-1).all() and got[0][n].eq(-1).all()
            assert float(got[2][n, 0]) == 0.0 and float(parts[0][n, 0]) == 0.0 and float(parts[1][n, 0]) == 0.0
            assert got[2][n, 1:].eq(R.NEG).all()


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[2], R.CASES[5], R.CASES[9]])
def test_zero_weights_are_the_unfused_search_on_the_device(case):
    from haloop_amd import ctc
    dec, e, il, ref = decoder_for(case)
    got = dec.decode(e, il, lm_weight=0.0, insertion_bonus=0.0)
    want = ctc.ctc_prefix_beam_search(e, il, case[1], dec.capacity)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
    print(case, 'max |score difference|', float((got[2] - want[2])[want[1] >= 0].abs().max()))
    close(got[2].cpu().numpy(), want[2].cpu().numpy(), str(case))
    close(dec.last_parts[0].cpu().numpy(), want[2].cpu().numpy(), str(case))


@pytest.mark.parametrize('case', [R.CASES[3], R.CASES[7]])
def test_lm_scores_agree_with_a_teacher_forced_pass(case):
    from haloop_amd import fusion
    dec, e, il, ref = decoder_for(case)
    got, parts = decode(dec, e, il)
    want = fusion.lm_score(dec.head.lm, got[0], got[1])
    assert want.shape == parts[1].shape and want.dtype == torch.float32
    assert torch.equal(want == R.NEG, got[1] < 0)
    print(case, 'max |lm_scores - lm_score|', float((parts[1] - want)[got[1] >= 0].abs().max()))
    close(parts[1].cpu().numpy(), want.cpu().numpy(), str(case))
    rows = R.compared_rows(case)
    close(want.cpu().numpy()[rows], ref['lm_scores'][rows].numpy(), f'{case} lm_score against float64')


def test_without_pruning_ctc_scores_equal_the_training_loss():
    """N = 2, T = 4, V = 3, cap = 3, W = 16: nothing is pruned, so every ctc_score is -functional.ctc_loss(reduction='none') of its
    hypothesis, the project's own training loss on the device."""
    from haloop_amd import functional as HF
    dec, e, il, ref = decoder_for(R.CASES[8])
    (tokens, lengths, scores, counts), parts = decode(dec, e, il)
    assert counts.tolist() == [13, 13]
    hyp = tokens[:, :13].reshape(26, -1).clamp(min=0)
    rows = torch.arange(2, device=DEV).repeat_interleave(13)
    losses = HF.ctc_loss(e[:, rows].contiguous(), hyp, il[rows], lengths[:, :13].reshape(26), reduction='none')
    print('max |ctc_score + loss|', float((parts[0][:, :13].reshape(26) + losses).abs().max()))
    close(parts[0][:, :13].reshape(26).cpu().numpy(), -losses.cpu().numpy(), 'tiny')


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[2]])
def test_padding_is_never_read(case):
    dec, e, il, ref = decoder_for(case)
    clean, parts = decode(dec, e, il)
    check(clean, parts, ref, R.compared_rows(case), str(case))
    T, N, V = e.shape
    poisoned = e.clone()
    for n, L in enumerate(il.tolist()):
        poisoned[L:, n] = float('nan')                                  # frames at or past the row's length
    got, got_parts = decode(dec, poisoned, il)
    assert same(got, clean) and same(got_parts, parts)
    big = torch.full((N + 1, T + 2, V + 3), float('nan'), device=DEV)   # the gaps of a strided view: rows, frames and classes beyond it
    big[:N, :T, :V] = poisoned.permute(1, 0, 2)
    view = big[:N, :T, :V].permute(1, 0, 2)
    assert view.stride(2) == 1 and not view.is_contiguous()
    got, got_parts = decode(dec, view, il)
    assert same(got, clean) and same(got_parts, parts)


@pytest.mark.parametrize('case', [R.CASES[7], R.CASES[9]])
def test_two_identical_calls_are_bit_equal(case):
    dec, e, il, ref = decoder_for(case)
    first, first_parts = decode(dec, e, il)
    again, again_parts = decode(dec, e, il)
    assert same(first, again) and same(first_parts, again_parts)


def test_a_reused_decoder_repeats_itself_and_follows_the_parameters():
    """N = 17, then 3 rows at another width and capacity, then 17 again; then an LM parameter changed in place."""
    from haloop_amd import fusion
    case = R.CASES[3]                                                   # rows17, W = 8
    dec, e, il, ref = decoder_for(case)
    first, first_parts = decode(dec, e, il)
    check(first, first_parts, ref, R.compared_rows(case), str(case))
    three, three_parts = decode(dec, e[:, :3], il[:3], capacity=5, beam=4)
    fresh = fusion.CTCFusionDecoder(dec.head.lm, 3, 5, 4, case[4], case[5])
    want, want_parts = decode(fresh, e[:, :3], il[:3])
    assert same(three, want) and same(three_parts, want_parts)
    third, third_parts = decode(dec, e, il)
    assert same(first, third) and same(first_parts, third_parts)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        dec.head.lm.out_layer.bias.add_(2.0 * torch.randn(8, generator=g).to(DEV))
        dec.head.lm.rnn.weight_hh_l1.mul_(0.5)
    changed, changed_parts = decode(dec, e, il)
    fresh = fusion.CTCFusionDecoder(dec.head.lm, 17, dec.capacity, 8, case[4], case[5])
    want, want_parts = decode(fresh, e, il)
    assert same(changed, want) and same(changed_parts, want_parts)
    assert not torch.equal(changed_parts[1], first_parts[1])


@pytest.mark.parametrize('case', [R.CASES[2], R.CASES[4]])
def test_the_general_path_agrees(case, monkeypatch):
    dec, e, il, ref = decoder_for(case)
    fused, fused_parts = decode(dec, e, il)
    monkeypatch.setenv('HALO_RNNT_FUSED', '0')
    assert not dec.fused
    general, general_parts = decode(dec, e, il)
    rows = R.compared_rows(case)
    check(general, general_parts, ref, rows, f'{case} general')
    assert all(torch.equal(x[rows], y[rows]) for x, y in zip((fused[0], fused[1], fused[3]), (general[0], general[1], general[3])))
    close(fused[2][rows].cpu().numpy(), general[2][rows].cpu().numpy(), str(case))


@pytest.mark.parametrize('mode,hidden', [('bf16x3', 64), ('f32', 512)])
def test_the_general_path_serves_what_the_fused_cells_refuse(mode, hidden):
    """An LM with H = 64, and `f32` mode: against the restatement on that LM (this test's own fixture condition: the rows that decide by
    GAP or more, at least two of the three)."""
    from haloop_amd import fusion
    W, a, b = 4, 0.5, 0.0
    e, il, capacity = P.inputs('small')
    lm = R.make_lm(5, 2, 1, hidden, hidden)
    ref = R.beam_search(e, il, capacity, W, R.LM64(lm), a, b)
    rows = [n for n in range(3) if float(ref['gaps'][n]) >= R.GAP]
    assert len(rows) >= 2
    with math_mode(mode):
        dec = fusion.CTCFusionDecoder(copy.deepcopy(lm).to(DEV), 3, capacity, W, a, b)
        assert not dec.fused
        got, parts = decode(dec, e.to(DEV), il.to(DEV))
    check(got, parts, ref, rows, f'general path, {mode}, H = {hidden}')


def test_temporal_classifier_set_lm():
    from haloop_amd import fusion, recognizer
    torch.manual_seed(5)
    head = recognizer.TemporalClassifier(16, 5)
    head.dropout.p, head.beam_size, head.mwer_beam = 0.0, 0, 0
    head = head.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    x, il = (3.0 * torch.randn(3, 6, 16, generator=g)).to(DEV), torch.tensor([6, 4, 0]).to(DEV)
    lm = copy.deepcopy(R.language_model(5, 2, 1)[0]).to(DEV)
    keys = list(head.state_dict())
    before_greedy, before_beam = head.decode(x, il, None), head.decode(x, il, None, beam_size=4)
    plain_nbest = head.last_nbest

    head.set_lm(lm, 0.7, 0.5)
    assert list(head.state_dict()) == keys and len(list(head.parameters())) == 2
    out = head.decode(x, il, None, beam_size=4)
    assert len(out) == 5
    hypotheses, output_lengths, alignments, scores, nothing = out
    assert nothing is None and alignments == [None] * 3 and hypotheses.is_nested
    with torch.no_grad():
        lp = head.log_probs(x)
    dec = fusion.CTCFusionDecoder(lm, 3, 6, 4, 0.7, 0.5)
    want, want_parts = decode(dec, lp.permute(1, 0, 2), il)
    assert same(head.last_nbest, want) and same(head.last_parts, want_parts)
    assert output_lengths.tolist() == want[1][:, 0].tolist() and torch.equal(scores, want[2][:, 0])
    for n, hyp in enumerate(hypotheses.unbind()):
        assert torch.equal(hyp, want[0][n, 0, :int(want[1][n, 0])])
    assert output_lengths[2] == 0 and float(scores[2]) == 0.0
    assert not same(head.last_nbest, plain_nbest)                        # the LM changed the lists
    greedy = head.decode(x, il, None)                                   # greedy stays the default, and does not use the LM
    assert torch.equal(greedy[3], before_greedy[3]) and torch.equal(greedy[2], before_greedy[2])
    head.train()
    with pytest.raises(NotImplementedError):
        head.decode(x, il, None, beam_size=4)
    head.eval()
    lm.train()
    with pytest.raises(NotImplementedError):
        head.decode(x, il, None, beam_size=4)
    lm.eval()

    head.set_lm(None)
    after = head.decode(x, il, None, beam_size=4)
    assert same(head.last_nbest, plain_nbest) and head.last_parts is None
    assert torch.equal(after[3], before_beam[3]) and after[1].tolist() == before_beam[1].tolist()
    for a, b in zip(after[0].unbind(), before_beam[0].unbind()):
        assert torch.equal(a, b)
