"""CPU checks of CTC prefix beam search with LM shallow fusion: the conditions of the fixtures that tests/test_gpu_ctc_lm_beam.py compares
exactly against (tests/ctc_lm_beam_ref.py), properties of the restatement itself (the unfused search at zero weights, the LM score against
a teacher-forced pass, the CTC score against torch's own CTC loss in float64), and the argument checks of the public interface.  No GPU."""
import pytest
import torch

import ctc_lm_beam_ref as R
import ctc_prefix_beam_ref as P


@pytest.mark.parametrize('name,W', [('small', 4), ('small', 1), ('rows17', 4), ('rows17cap', 4), ('tiny', 16), ('wide', 3)])
def test_zero_weights_are_the_unfused_search(name, W):
    emissions, il, capacity, plain = P.fixture(name, W)
    _, lm64 = R.language_model(emissions.shape[2], 2, 1)
    got = R.beam_search(emissions, il, capacity, W, lm64, 0.0, 0.0)
    assert torch.equal(got['tokens'], plain['tokens']) and torch.equal(got['lengths'], plain['lengths'])
    assert torch.equal(got['counts'], plain['counts']) and torch.equal(got['merges'], plain['merges'])
    present = plain['lengths'] >= 0
    assert float((got['scores'] - plain['scores'])[present].abs().max()) <= 1e-12
    assert float((got['ctc_scores'] - plain['scores'])[present].abs().max()) <= 1e-12
    assert torch.equal(got['scores'] == R.NEG, ~present)


@pytest.mark.parametrize('case', R.CASES)
def test_fixture_conditions(case):
    """Every compared row decides every prune and every final ranking by GAP or more; few rows are left out; the LM changes the lists."""
    name, W = case[0], case[1]
    emissions, il, capacity, lm, ref = R.fixture(case)
    N = emissions.shape[1]
    rows = R.compared_rows(case)
    print(case, 'gaps', [round(float(x), 5) for x in ref['gaps']], 'merges', ref['merges'].tolist())
    assert all(float(ref['gaps'][n]) >= R.GAP for n in rows)
    assert len(rows) >= N - (4 if N >= 17 else 0)
    assert all(n in range(N) for n in R.LEFT_OUT.get(case, ()))
    plain = P.fixture(name, W)[3]
    differ = [n for n in rows if not torch.equal(ref['tokens'][n], plain['tokens'][n])]
    print('rows whose lists differ from the unfused search', differ)
    assert differ
    assert all(int(ref['counts'][n]) == 1 and int(ref['lengths'][n, 0]) == 0 and float(ref['scores'][n, 0]) == 0.0
               and float(ref['ctc_scores'][n, 0]) == 0.0 and float(ref['lm_scores'][n, 0]) == 0.0 for n in range(N) if int(il[n]) == 0)


@pytest.mark.parametrize('case', R.CASES)
def test_scores_are_what_they_say(case):
    """lm_scores is the teacher-forced LM log-probability of the hypothesis, scores the ranking value of the parts, ctc_scores at most the
    CTC lattice total of the hypothesis over the row's frames."""
    name, W, layers, seed, a, b = case
    emissions, il, capacity, lm, ref = R.fixture(case)
    _, lm64 = R.language_model(emissions.shape[2], layers, seed)
    for n in range(emissions.shape[1]):
        count = int(ref['counts'][n])
        for w in range(count):
            y = ref['tokens'][n, w, :int(ref['lengths'][n, w])].tolist()
            assert abs(lm64.score(y) - float(ref['lm_scores'][n, w])) <= 1e-9
            want = float(ref['ctc_scores'][n, w]) + a * float(ref['lm_scores'][n, w]) + b * len(y)
            assert abs(want - float(ref['scores'][n, w])) <= 1e-9
        if int(il[n]) > 0:
            totals = P.lattice_totals(emissions, il, ref, n)
            assert bool((ref['ctc_scores'][n, :count] <= totals + 1e-9).all())
            if name == 'tiny':                                          # W = 16 holds all 13 hypotheses: nothing is pruned
                assert count == 13 and float((ref['ctc_scores'][n, :count] - totals).abs().max()) <= 1e-9


def test_the_abi_entry_is_bound():
    from haloop_amd import _lib, ops
    assert 'halo_ctc_lm_beam_step' in _lib.SIGNATURES and callable(ops.ctc_lm_beam_step)
    assert hasattr(_lib.lib(), 'halo_ctc_lm_beam_step')


def test_argument_checks():
    from haloop_amd import _lib, fusion, recognizer
    lm = R.make_lm(5, 1, 3, 32, 32)
    for kwargs in (dict(max_batch=0, capacity=4), dict(max_batch=2, capacity=0), dict(max_batch=2, capacity=4, beam=0),
                   dict(max_batch=2, capacity=4, beam=17), dict(max_batch=2, capacity=4, lm_weight=float('nan')),
                   dict(max_batch=2, capacity=4, insertion_bonus=float('inf')), dict(max_batch=2, capacity=4, start_token=5),
                   dict(max_batch=2, capacity=4, start_token=-1)):
        with pytest.raises(ValueError):
            fusion.CTCFusionDecoder(lm, **kwargs)
    dec = fusion.CTCFusionDecoder(lm, 2, 4, beam=4)
    assert (dec.lm_weight, dec.insertion_bonus, dec.start_token, dec.beam) == (0.5, 0.0, 0, 4)
    e = torch.randn(6, 2, 5).log_softmax(-1)
    for bad in (lambda: dec.decode(e[0]), lambda: dec.decode(torch.randn(6, 2, 7)), lambda: dec.decode(torch.randn(6, 3, 5)),
                lambda: dec.decode(e, capacity=5), lambda: dec.decode(e, capacity=0), lambda: dec.decode(e, beam=5),
                lambda: dec.decode(e, beam=0), lambda: dec.decode(e, torch.tensor([6, 6, 6])), lambda: dec.decode(e, lm_weight=float('nan'))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.HaloError):
        dec.decode(e, torch.tensor([6, 4]))                             # CPU tensors: no CPU path
    lm.train()
    with pytest.raises(NotImplementedError):
        dec.decode(e)
    with pytest.raises(NotImplementedError):
        fusion.lm_score(lm, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([1, 2]))
    lm.eval()
    with pytest.raises(_lib.HaloError):
        fusion.lm_score(lm, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        fusion.lm_score(lm, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([1, 2, 3]))

    head = recognizer.TemporalClassifier(16, 5)
    keys, params = list(head.state_dict()), [id(p) for p in head.parameters()]
    defaults = (head.beam_size, head.mwer_beam, head.last_nbest)
    with pytest.raises(ValueError):
        head.set_lm(R.make_lm(6, 1, 3, 32, 32))                         # an LM over other classes
    with pytest.raises(ValueError):
        head.set_lm(lm, lm_weight=float('inf'))
    assert head._fusion is None
    head.set_lm(lm, 0.7, 0.5)
    assert head._fusion['lm'] is lm and (head._fusion['lm_weight'], head._fusion['insertion_bonus']) == (0.7, 0.5)
    assert list(head.state_dict()) == keys == ['classifier.weight', 'classifier.bias']
    assert [id(p) for p in head.parameters()] == params and len(list(head.modules())) == 3
    assert (head.beam_size, head.mwer_beam, head.last_nbest) == defaults
    with pytest.raises(_lib.HaloError):
        head.eval().decode(torch.randn(2, 6, 16), torch.tensor([6, 4]), None, beam_size=4)
    head.set_lm(None)
    assert head._fusion is None and head.last_parts is None and list(head.state_dict()) == keys
