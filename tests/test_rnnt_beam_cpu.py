"""CPU checks of the transducer beam search: the conditions of the fixtures that tests/test_gpu_rnnt_beam.py compares exactly against
(tests/rnnt_beam_ref.py), two properties of the search itself, and the argument checks of the public interface.  No GPU."""
import pytest
import torch

import rnnt_beam_ref as R


def rows_below_gap(ref):
    return [n for n in range(len(ref['gaps'])) if float(ref['gaps'][n]) < R.GAP]


@pytest.mark.parametrize('name,W', [('small', 4), ('small', 1), ('rows17', 4), ('wide', 3), ('stream', 3), ('tiny', 16)])
def test_every_row_decides_by_a_gap(name, W):
    ref = R.fixture(name, W)[4]
    print(name, W, 'gaps', ref['gaps'].tolist())
    assert rows_below_gap(ref) == []
    assert R.LEFT_OUT.get((name, W), ()) == ()


def test_rows17_width_8_lists_its_close_rows():
    ref = R.fixture('rows17', 8)[4]
    print('gaps', ref['gaps'].tolist())
    left_out = R.LEFT_OUT[('rows17', 8)]
    assert rows_below_gap(ref) == list(left_out)
    assert len(left_out) <= R.FIXTURES['rows17']['N'] // 4
    assert len(R.compared_rows('rows17', 8)) == R.FIXTURES['rows17']['N'] - len(left_out)


@pytest.mark.parametrize('W', [4, 8])
def test_rows17_is_lively(W):
    sd, x, il, cap, ref = R.fixture('rows17', W)
    nonempty = [n for n in range(len(il)) if int(il[n]) > 0]
    assert len(nonempty) == len(il) - 1
    assert sum(int(ref['merges'][n]) > 0 for n in nonempty) * 2 >= len(nonempty)
    best = ref['lengths'][:, 0].tolist()
    assert any(0 < b < cap for b in best) and cap in best and 0 in best
    empty = [n for n in range(len(il)) if int(il[n]) == 0]
    for n in empty:                                                     # a row of no frames: the empty hypothesis, score 0
        assert int(ref['counts'][n]) == 1 and int(ref['lengths'][n, 0]) == 0 and float(ref['scores'][n, 0]) == 0.0


def test_without_pruning_scores_are_lattice_totals():
    """N = 2, T = 5, V = 4, cap = 2, W = 16: the 13 sequences of at most two symbols all fit."""
    sd, x, il, cap, ref = R.fixture('tiny', 16)
    assert ref['counts'].tolist() == [13, 13]
    for n in range(2):
        seen = set()
        for w in range(13):
            hyp = ref['tokens'][n, w, :int(ref['lengths'][n, w])]
            seen.add(tuple(hyp.tolist()))
            total = R.lattice_total(sd, x[n], int(il[n]), hyp)
            assert abs(float(ref['scores'][n, w]) - total) <= 1e-9, (n, w, float(ref['scores'][n, w]), total)
        assert len(seen) == 13
        assert float(ref['scores'][n, :13].exp().sum()) <= 1.0


@pytest.mark.parametrize('name', ['small', 'rows17'])
def test_with_pruning_scores_stay_below_lattice_totals(name):
    sd, x, il, cap, ref = R.fixture(name, 4)
    for n in range(len(il)):
        if int(il[n]) == 0:
            continue
        for w in range(int(ref['counts'][n])):
            hyp = ref['tokens'][n, w, :int(ref['lengths'][n, w])]
            total = R.lattice_total(sd, x[n], int(il[n]), hyp)
            assert float(ref['scores'][n, w]) <= total + 1e-9, (n, w)
        s = ref['scores'][n, :int(ref['counts'][n])]
        assert bool((s[:-1] >= s[1:]).all())


def cpu_head(V=8):
    from haloop_amd import recognizer
    return recognizer.Transducer(V, V).eval()


def test_beam_decoder_checks_its_arguments():
    from haloop_amd import _lib, transducer
    head = cpu_head()
    for beam in (0, 17):
        with pytest.raises(ValueError):
            transducer.BeamDecoder(head, 2, 3, beam=beam)
    with pytest.raises(ValueError):
        transducer.BeamDecoder(head, 0, 3)
    with pytest.raises(ValueError):
        transducer.BeamDecoder(head, 2, 0)
    dec = transducer.BeamDecoder(head, 2, 3, beam=4)
    x = torch.zeros(3, 5, 8)
    with pytest.raises(ValueError):
        dec.decode(x, torch.tensor([5, 5, 5]))                          # batch above max_batch
    with pytest.raises(ValueError):
        dec.decode(x[:2], torch.tensor([5, 5, 5]))                      # input_lengths of another batch
    with pytest.raises(_lib.HaloError):
        dec.decode(x[:2], torch.tensor([5, 5]))                         # CPU features
    head.train()
    with pytest.raises(_lib.HaloError):                                 # (the device check comes first, as in GreedyDecoder)
        dec.decode(x[:2], torch.tensor([5, 5]))
    head.eval()


def test_transducer_beam_size(monkeypatch):
    import inspect
    from haloop_amd import _lib
    monkeypatch.delenv('HALO_RNNT_BEAM', raising=False)
    head = cpu_head()
    assert head.beam_size == 0 and head.last_nbest is None
    assert inspect.signature(head.decode).parameters['beam_size'].default is None
    monkeypatch.setenv('HALO_RNNT_BEAM', '4')
    assert cpu_head().beam_size == 4
    with pytest.raises(_lib.HaloError):                                 # CPU features reach the decoder's device check
        head.decode(torch.zeros(1, 5, 8), torch.tensor([5]), torch.tensor([2]), beam_size=2)
