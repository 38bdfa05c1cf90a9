"""The float64 restatement of the attention decoder's beam search (tests/asr_beam_ref.py) against the greedy oracle, a brute-force
enumeration and teacher forcing; the conditions on the GPU cases; the argument checks of the public interface.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

import asr_beam_ref as R
from oracle import transformer_ref as tref

ETX = R.ETX


def _small(V=4, hd=16, heads=2, L=1, S=5, N=3, seed=3, sharp=1.0):
    pd = tref.make_decoder_params(V, hd, heads, L, seed, sharp=sharp)
    g = torch.Generator().manual_seed(seed + 100)
    feats = torch.randn(N, S, hd * heads, generator=g)
    flen = torch.randint(2, S + 1, (N,), generator=g)
    return pd, feats, flen


def _teacher_forced(pd, feats, flen, heads, n, toks, closed):
    """log P(toks (+ ETX when closed) | utterance n) from one teacher-forced pass in float64, caches unrounded."""
    p64 = {k: v.double() for k, v in pd.items()}
    prompt = torch.tensor([[R.STX] + list(toks)])
    lp = tref.decoder_logits(p64, feats[n:n + 1].double(), prompt, flen[n:n + 1], heads, pre='decoder.').log_softmax(-1)[0]
    out = list(toks) + ([ETX] if closed else [])
    return float(sum(lp[i, k] for i, k in enumerate(out)))


@pytest.mark.parametrize('name', list(R.CASES))
def test_gpu_cases_leave_out_no_more_rows_than_their_cap(name):
    """Conditions, not measurements: at most a quarter of a case's rows at W <= 8 and half at W = 16 may lie below GAP."""
    N = R.CASES[name][5]
    left_out = N - len(R.compared_rows(name))
    assert left_out <= R.excluded_cap(name), (name, left_out, R.case_result(name)['margin'].tolist())


def test_gpu_cases_cover_finished_open_and_long_hypotheses():
    assert int(R.case_result('w4')['finished'].sum()) > 34                       # most slots finished
    assert not bool(R.case_result('l3-w3')['finished'].any())                    # nothing finishes
    fin = R.case_result('w4-bonus')['finished']
    assert bool(fin.any()) and not bool(fin.all())
    assert R.CASES['v4100'][0] * R.CASES['v4100'][8] > 8192                      # the recompute route of the selection
    assert R.CASES['t18'][11] >= 17 and int(R.case_result('t18')['lengths'].max()) >= 17


def test_width_one_without_bonus_is_the_greedy_oracle():
    pd, feats, flen, tl = R.case_inputs('w4')
    heads, T = R.CASES['w4'][2], R.CASES['w4'][11]
    res = R.beam_search(pd, feats, flen, heads, 1, T, 0.0)
    outs, out_len, lps, _, _ = tref.decoder_decode(pd, feats, flen, tl, heads, pre='decoder.')
    for n in range(feats.shape[0]):
        ln, closed = int(res['lengths'][n, 0]), bool(res['finished'][n, 0])
        assert int(out_len[n]) == ln + closed                                     # greedy counts the steps a row was alive
        assert res['tokens'][n, 0, :int(out_len[n]) - 1].tolist() == outs[n].tolist()
    # float32 against float64 through two layers and nine steps: the decoder's own figure at this depth
    np.testing.assert_allclose(res['logprobs'][:, 0].numpy(), lps.double().numpy(), rtol=0, atol=2e-3)
    assert torch.equal(res['ranks'], res['logprobs'])


@pytest.mark.parametrize('bonus', [0.0, 0.7])
def test_exhaustive_beam_equals_brute_force(bonus):
    """V = 4, capacity 2, W = 16: the beam holds every prefix (1, then 4, then 3 * 4 + 1 = 13 <= 16), so the lists are the enumeration
    of all hypotheses sorted by rank."""
    pd, feats, flen = _small()
    heads, V, cap = 2, 4, 2
    res = R.beam_search(pd, feats, flen, heads, 16, cap, bonus, cache_dtype=torch.float64)
    labels = [k for k in range(V) if k != ETX]
    hyps = [((), True)] + [((a,), True) for a in labels] + [((a, b), False) for a in labels for b in labels]
    assert res['counts'].tolist() == [len(hyps)] * feats.shape[0]
    for n in range(feats.shape[0]):
        want = sorted(((_teacher_forced(pd, feats, flen, heads, n, t, c) + bonus * len(t), t, c) for t, c in hyps), key=lambda x: -x[0])
        for w, (rank, toks, closed) in enumerate(want):
            assert res['tokens'][n, w, :len(toks)].tolist() == list(toks) and int(res['lengths'][n, w]) == len(toks)
            assert bool(res['finished'][n, w]) == closed
            assert abs(float(res['ranks'][n, w]) - rank) < 1e-9
        assert bool((res['lengths'][n, len(hyps):] == -1).all()) and bool((res['ranks'][n, len(hyps):] == float('-inf')).all())


@pytest.mark.parametrize('W,bonus', [(1, 0.0), (3, 0.0), (4, 1.0)])
def test_logprobs_are_teacher_forced_and_lists_are_ordered_and_distinct(W, bonus):
    pd, feats, flen = _small(V=12, N=4, seed=5, sharp=2.0)
    heads, cap = 2, 5
    res = R.beam_search(pd, feats, flen, heads, W, cap, bonus, cache_dtype=torch.float64)
    for n in range(feats.shape[0]):
        seen = set()
        for w in range(int(res['counts'][n])):
            ln = int(res['lengths'][n, w])
            toks, closed = res['tokens'][n, w, :ln].tolist(), bool(res['finished'][n, w])
            assert all(k != ETX and k >= 0 for k in toks) and bool((res['tokens'][n, w, ln:] == -1).all())
            want = _teacher_forced(pd, feats, flen, heads, n, toks, closed)
            assert abs(float(res['logprobs'][n, w]) - want) < 1e-9
            assert abs(float(res['ranks'][n, w]) - (want + bonus * ln)) < 1e-9
            assert (tuple(toks), closed) not in seen
            seen.add((tuple(toks), closed))
        r = res['ranks'][n]
        assert bool((r[:-1] >= r[1:]).all())


def test_length_bonus_changes_the_lists():
    a, b = R.case_result('w4'), R.case_result('w4-bonus')
    assert not torch.equal(a['tokens'], b['tokens'])
    assert float(b['lengths'][:, 0].float().mean()) > float(a['lengths'][:, 0].float().mean())


def test_public_interface_argument_checks():
    from haloop_amd import transformer
    dec = transformer.Decoder(vocab=8, head_dim=16, heads=2, p_drop=0.0, layers=1)
    assert dec.beam_size == 0 and dec.length_bonus == 0.0
    for bad in (0, 17):
        with pytest.raises(ValueError):
            transformer.BeamDecoder(dec, 2, 4, beam=bad)
    with pytest.raises(ValueError):
        transformer.BeamDecoder(dec, 0, 4)
    with pytest.raises(ValueError):
        transformer.BeamDecoder(dec, 2, 0)


def test_beam_width_is_read_from_the_environment(monkeypatch):
    from haloop_amd import transformer
    monkeypatch.setenv('HALO_ASR_BEAM', '4')
    assert transformer.Decoder(vocab=8, head_dim=16, heads=2, p_drop=0.0, layers=1).beam_size == 4
