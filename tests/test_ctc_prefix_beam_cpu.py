"""CPU checks of the CTC prefix beam search: the conditions of the fixtures that tests/test_gpu_ctc_prefix_beam.py compares exactly
against (tests/ctc_prefix_beam_ref.py), properties of the search itself against torch's own CTC loss in float64, and the argument checks
and defaults of the public interface.  No GPU."""
import pytest
import torch

import ctc_prefix_beam_ref as R


def rows_below_gap(ref):
    return [n for n in range(len(ref['gaps'])) if float(ref['gaps'][n]) < R.GAP]


@pytest.mark.parametrize('name,W', R.CASES)
def test_every_compared_row_decides_by_a_gap(name, W):
    ref = R.fixture(name, W)[3]
    print(name, W, 'gaps', ref['gaps'].tolist())
    left_out = R.LEFT_OUT.get((name, W), ())
    N = R.FIXTURES[name]['N']
    assert rows_below_gap(ref) == list(left_out)
    assert len(left_out) <= N // 4
    assert len(R.compared_rows(name, W)) == N - len(left_out)


def test_left_out_names_only_cases_that_run():
    assert set(R.LEFT_OUT) <= set(R.CASES)


def test_huge_holds_a_token_above_16_bits():
    ref = R.fixture('huge', 2)[3]
    assert int(ref['tokens'][0, 0].max()) >= 65536


@pytest.mark.parametrize('W', [4, 8])
def test_rows17_is_lively(W):
    e, il, cap, ref = R.fixture('rows17', W)
    nonempty = [n for n in range(len(il)) if int(il[n]) > 0]
    assert len(nonempty) == len(il) - 1
    print('merges', ref['merges'].tolist(), 'best lengths', ref['lengths'][:, 0].tolist())
    assert sum(int(ref['merges'][n]) > 0 for n in nonempty) * 2 >= len(nonempty)
    best = ref['lengths'][:, 0].tolist()
    assert 0 in best and any(0 < b < cap for b in best)
    for n in range(len(il)):
        if int(il[n]) == 0:                                             # a row of no frames: the empty hypothesis alone, score 0
            assert int(ref['counts'][n]) == 1 and int(ref['lengths'][n, 0]) == 0 and float(ref['scores'][n, 0]) == 0.0


def test_rows17_capped_reaches_the_capacity():
    e, il, cap, ref = R.fixture('rows17cap', 4)
    assert cap == 3
    best = ref['lengths'][:, 0].tolist()
    print('best lengths', best)
    assert cap in best and max(best) == cap and int(ref['lengths'].max()) == cap


def test_without_pruning_scores_are_lattice_totals():
    """N = 2, T = 4, V = 3, cap = 3, W = 16: the 15 sequences of at most three of two labels except 111 and 222 (three equal labels
    need five frames) all fit: 13 hypotheses a row, each with all of its alignments."""
    e, il, cap, ref = R.fixture('tiny', 16)
    assert ref['counts'].tolist() == [13, 13]
    for n in range(2):
        hyps = {tuple(ref['tokens'][n, w, :int(ref['lengths'][n, w])].tolist()) for w in range(13)}
        assert len(hyps) == 13 and (1, 1, 1) not in hyps and (2, 2, 2) not in hyps
        totals = R.lattice_totals(e, il, ref, n)
        err = (ref['scores'][n, :13] - totals).abs().max()
        print('row', n, 'max |score - lattice total|', float(err))
        assert float(err) <= 1e-9
        assert float(ref['scores'][n, :13].exp().sum()) <= 1.0


@pytest.mark.parametrize('name,W', [('small', 4), ('small', 1), ('rows17', 4), ('rows17cap', 4), ('long', 4)])
def test_with_pruning_scores_stay_below_lattice_totals(name, W):
    e, il, cap, ref = R.fixture(name, W)
    for n in range(len(il)):
        count = int(ref['counts'][n])
        assert 1 <= count <= W
        if int(il[n]) == 0:
            continue
        totals = R.lattice_totals(e, il, ref, n)
        assert bool((ref['scores'][n, :count] <= totals + 1e-9).all()), n
        s = ref['scores'][n, :count]
        assert bool((s[:-1] >= s[1:]).all())
        assert bool((ref['lengths'][n, count:] == -1).all()) and bool((ref['scores'][n, count:] == float('-inf')).all())


def test_prefix_beam_search_checks_its_arguments():
    from haloop_amd import _lib, ctc
    e = torch.zeros(5, 2, 4).log_softmax(-1)
    for beam in (0, 17, -1):
        with pytest.raises(ValueError):
            ctc.ctc_prefix_beam_search(e, beam=beam)
    for capacity in (0, 6, -2):
        with pytest.raises(ValueError):
            ctc.ctc_prefix_beam_search(e, capacity=capacity)
    with pytest.raises(ValueError):
        ctc.ctc_prefix_beam_search(e, torch.tensor([5, 5, 5]))          # emission_lengths of another batch
    with pytest.raises(ValueError):
        ctc.ctc_prefix_beam_search(e[0])                                # two dimensions
    with pytest.raises(ValueError):
        ctc.ctc_prefix_beam_search(e[:, :, :1])                         # the blank alone
    with pytest.raises(_lib.HaloError):
        ctc.ctc_prefix_beam_search(e, torch.tensor([5, 4]))             # CPU emissions: no CPU path


def test_library_answers_the_workspace_query_without_a_device():
    from haloop_amd import _lib
    handle = _lib.lib()
    size = handle.halo_ctc_prefix_beam_workspace_bytes
    assert size(64, 250, 256, 16, 250) == 0                             # 2 W cap = 8000 16-bit tokens: in LDS
    assert size(1, 400, 3, 16, 400) == 2 * 16 * 400 * 4                 # 12800 > 12288: the workspace, 32-bit tokens
    assert size(3, 10, 70000, 2, 10) == 3 * 2 * 2 * 10 * 4              # a token does not fit 16 bits
    for bad in ((0, 5, 4, 4, 5), (1, 0, 4, 4, 1), (1, 5, 1, 4, 5), (1, 5, 4, 0, 5), (1, 5, 4, 17, 5), (1, 5, 4, 4, 0), (1, 5, 4, 4, 6)):
        assert size(*bad) == 0


def cpu_head(V=5):
    from haloop_amd import recognizer
    return recognizer.TemporalClassifier(16, V).eval()


def test_temporal_classifier_beam_size(monkeypatch):
    import inspect
    from haloop_amd import _lib
    monkeypatch.delenv('HALO_CTC_BEAM', raising=False)
    monkeypatch.delenv('HALO_CTC_MWER', raising=False)
    head = cpu_head()
    assert head.beam_size == 0 and head.mwer_beam == 0 and head.last_nbest is None
    assert inspect.signature(head.decode).parameters['beam_size'].default is None
    assert list(head.state_dict()) == ['classifier.weight', 'classifier.bias']
    monkeypatch.setenv('HALO_CTC_BEAM', '4')
    monkeypatch.setenv('HALO_CTC_MWER', '3')
    other = cpu_head()
    assert other.beam_size == 4 and other.mwer_beam == 3
    x = torch.zeros(1, 6, 16)
    with pytest.raises(ValueError):
        head.decode(x, torch.tensor([6]), None, beam_size=-1)
    with pytest.raises(_lib.HaloError):                                 # CPU features reach the head's device check
        head.decode(x, torch.tensor([6]), None, beam_size=2)
    with pytest.raises(_lib.HaloError):                                 # ... by the attribute as by the keyword
        other.decode(x, torch.tensor([6]), None)
    head.train()
    with pytest.raises(NotImplementedError):                            # the search refuses a head in training mode
        head.decode(x, torch.tensor([6]), None, beam_size=2)
    with pytest.raises(_lib.HaloError):
        head.mwer_forward(x, torch.tensor([[1, 2]]), torch.tensor([6]), torch.tensor([2]))
    assert head.training
