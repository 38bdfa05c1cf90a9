"""CPU checks of transducer beam search with LM shallow fusion: the conditions of the fixtures that tests/test_gpu_rnnt_lm_beam.py
compares exactly against (tests/rnnt_lm_beam_ref.py), properties of the restatement itself (the unfused search at zero weights, the LM
score against a teacher-forced pass, the transducer score against the lattice total in float64), and the argument checks of the public
interface.  No GPU."""
import pytest
import torch

import rnnt_beam_ref as B
import rnnt_lm_beam_ref as R


@pytest.mark.parametrize('case', R.CASES)
def test_fixture_conditions(case):
    """Every compared row decides every prune and every final ranking by GAP or more; LEFT_OUT lists exactly the rows below it, at most
    N // 4 of a case and none of the small fixtures; a row of no frames gives the empty hypothesis with every score 0."""
    name = case[0]
    sd, features, il, capacity, lm, ref = R.fixture(case)
    N = features.shape[0]
    print(case, 'gaps', [round(float(x), 5) for x in ref['gaps']], 'merges', ref['merges'].tolist(), 'best lengths', ref['lengths'][:, 0].tolist())
    below = tuple(n for n in range(N) if float(ref['gaps'][n]) < R.GAP)
    assert below == tuple(R.LEFT_OUT.get(case, ()))
    assert R.compared_rows(case) == [n for n in range(N) if n not in below]
    assert len(below) <= N // 4
    if name in ('small', 'tiny', 'wide', 'stream'):
        assert not below
    assert all(int(ref['counts'][n]) == 1 and int(ref['lengths'][n, 0]) == 0 and float(ref['scores'][n, 0]) == 0.0
               and float(ref['rnnt_scores'][n, 0]) == 0.0 and float(ref['lm_scores'][n, 0]) == 0.0 for n in range(N) if int(il[n]) == 0)


def test_left_out_names_cases():
    assert all(case in R.CASES for case in R.LEFT_OUT)


@pytest.mark.parametrize('name,W', [('small', 4), ('small', 1), ('tiny', 16), ('rows17', 4), ('wide', 3)])
def test_zero_weights_are_the_unfused_search(name, W):
    sd, features, il, capacity, plain = B.fixture(name, W)
    _, lm64 = R.language_model(B.FIXTURES[name]['V'], 2, 1)
    got = R.beam_search(sd, features, il, capacity, W, lm64, 0.0, 0.0)
    for k in ('tokens', 'lengths', 'counts', 'merges', 'gaps'):
        assert torch.equal(got[k], plain[k]), k
    assert torch.equal(got['scores'], plain['scores']) and torch.equal(got['rnnt_scores'], plain['scores'])


@pytest.mark.parametrize('case', R.CASES)
def test_scores_are_what_they_say(case):
    """lm_scores is the teacher-forced LM log-probability of the hypothesis, scores the rank of the parts, rnnt_scores at most the lattice
    total of the hypothesis over the row's frames, and equal to it where nothing is pruned."""
    name, W, layers, seed, a, b = case
    sd, features, il, capacity, lm, ref = R.fixture(case)
    _, lm64 = R.language_model(B.FIXTURES[name]['V'], layers, seed)
    for n in range(features.shape[0]):
        for w in range(int(ref['counts'][n])):
            y = ref['tokens'][n, w, :int(ref['lengths'][n, w])]
            assert abs(lm64.score(y.tolist()) - float(ref['lm_scores'][n, w])) <= 1e-9
            want = float(ref['rnnt_scores'][n, w]) + a * float(ref['lm_scores'][n, w]) + b * len(y)
            assert abs(want - float(ref['scores'][n, w])) <= 1e-9
            if name in ('tiny', 'small') and int(il[n]) > 0:
                total = B.lattice_total(sd, features[n], int(il[n]), y)
                assert float(ref['rnnt_scores'][n, w]) <= total + 1e-9
                if name == 'tiny':                                      # W = 16 holds all 13 sequences: nothing is pruned
                    assert int(ref['counts'][n]) == 13 and abs(float(ref['rnnt_scores'][n, w]) - total) <= 1e-9


def test_the_fixtures_are_lively():
    """rows17 at W = 4: best hypotheses of length 0, strictly between 0 and the capacity, and the capacity all occur; merges occur in at
    least half of the rows with frames; the LM changes the list of at least half of the rows against the unfused search."""
    case = R.CASES[3]
    assert case[:2] == ('rows17', 4)
    sd, features, il, capacity, lm, ref = R.fixture(case)
    plain = B.fixture('rows17', 4)[4]
    best = ref['lengths'][:, 0].tolist()
    print('best lengths', best, 'merges', ref['merges'].tolist())
    assert 0 in best and capacity in best and any(0 < x < capacity for x in best)
    nonempty = [n for n in range(17) if int(il[n]) > 0]
    assert 2 * sum(int(ref['merges'][n]) > 0 for n in nonempty) >= len(nonempty)
    changed = [n for n in range(17) if not torch.equal(ref['tokens'][n], plain['tokens'][n])]
    print('rows whose lists differ from the unfused search', changed)
    assert 2 * len(changed) >= 17
    small = R.fixture(R.CASES[0])[5]
    assert sum(not torch.equal(small['tokens'][n], B.fixture('small', 4)[4]['tokens'][n]) for n in range(3)) >= 1


def test_the_abi_entry_is_bound():
    from haloop_amd import _lib, ops
    assert 'halo_rnnt_lm_beam_step' in _lib.SIGNATURES and callable(ops.rnnt_lm_beam_step)
    assert hasattr(_lib.lib(), 'halo_rnnt_lm_beam_step')


def test_argument_checks():
    from haloop_amd import _lib, fusion, recognizer
    head = recognizer.Transducer(16, 5).eval()
    lm = R.make_lm(5, 1, 3, 32, 32)
    for kwargs in (dict(max_batch=0, capacity=4), dict(max_batch=2, capacity=0), dict(max_batch=2, capacity=4, beam=0),
                   dict(max_batch=2, capacity=4, beam=17), dict(max_batch=2, capacity=4, lm_weight=float('nan')),
                   dict(max_batch=2, capacity=4, insertion_bonus=float('inf')), dict(max_batch=2, capacity=4, start_token=5),
                   dict(max_batch=2, capacity=4, start_token=-1)):
        with pytest.raises(ValueError):
            fusion.TransducerFusionDecoder(head, lm, **kwargs)
    with pytest.raises(ValueError):
        fusion.TransducerFusionDecoder(head, R.make_lm(6, 1, 3, 32, 32), 2, 4)         # an LM over other classes
    dec = fusion.TransducerFusionDecoder(head, lm, 2, 4, beam=4)
    assert (dec.lm_weight, dec.insertion_bonus, dec.start_token, dec.beam) == (0.5, 0.0, 0, 4)
    assert dec.last_parts is None and dec.iterations == 0
    x, il = torch.randn(2, 6, 16), torch.tensor([6, 4])
    for bad in (lambda: dec.decode(x[0], il), lambda: dec.decode(torch.randn(3, 6, 16), torch.tensor([6, 4, 2])),
                lambda: dec.decode(x, torch.tensor([6, 6, 6])), lambda: dec.decode(x, il, capacity=5), lambda: dec.decode(x, il, capacity=0),
                lambda: dec.decode(x, il, beam=5), lambda: dec.decode(x, il, beam=0), lambda: dec.decode(x, il, lm_weight=float('nan')),
                lambda: dec.decode(x, il, insertion_bonus=float('-inf'))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.HaloError):
        dec.decode(x, il)                                               # CPU tensors: no CPU path
    lm.train()
    with pytest.raises(NotImplementedError):
        dec.decode(x, il)
    lm.eval()
    head.train()
    with pytest.raises(NotImplementedError):
        dec.decode(x, il)
    head.eval()

    keys, params = list(head.state_dict()), [id(p) for p in head.parameters()]
    modules = len(list(head.modules()))
    defaults = (head.beam_size, head.mwer_beam, head.last_nbest)
    assert head._fusion is None and head.last_parts is None
    with pytest.raises(ValueError):
        head.set_fusion_lm(R.make_lm(6, 1, 3, 32, 32))                  # an LM over other classes
    with pytest.raises(ValueError):
        head.set_fusion_lm(lm, lm_weight=float('inf'))
    assert head._fusion is None
    head.set_fusion_lm(lm, 0.7, 0.5)
    assert head._fusion['lm'] is lm and (head._fusion['lm_weight'], head._fusion['insertion_bonus']) == (0.7, 0.5)
    assert list(head.state_dict()) == keys and [id(p) for p in head.parameters()] == params and len(list(head.modules())) == modules
    assert (head.beam_size, head.mwer_beam, head.last_nbest) == defaults
    with pytest.raises(_lib.HaloError):
        head.decode(x, il, torch.tensor([3, 2]), beam_size=4)
    head.set_fusion_lm(None)
    assert head._fusion is None and head.last_parts is None and list(head.state_dict()) == keys
