"""Pins tests/stream_ref.py, the CPU restatement of streamed recognition that the GPU tests compare against: the reference's golden
alignments and hypotheses, float64 equality with the whole-utterance oracle, and the step arithmetic.  CPU only."""
import numpy as np
import pytest
import torch

import stream_ref
from conftest import load_golden
from oracle import cpu_ref


def _params(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}


@pytest.mark.parametrize('name', ['g1_tiny_l2', 'g1_tiny_l3'])
def test_streamed_goldens(name):
    """All 41 frames of every row as 5 pushes of 8 and a finish with a tail of 1, in float32 like the oracle's own golden test."""
    g = load_golden(name)
    x = torch.from_numpy(g['x'])
    B, T, _ = x.shape
    assert T == 41
    ref = stream_ref.stream_all(stream_ref.StreamRef(_params(g, 'encoder.'), _params(g, 'recognizer.'), B), x, [T] * B, 8)
    for b in range(B):
        assert ref.rows[b]['ali'] == g['ali'][b].tolist() and len(ref.rows[b]['ali']) == 11
        assert ref.rows[b]['hyp'] == g['hyps'][b][:g['hlen'][b]].tolist()
        assert len(ref.rows[b]['hyp']) == int(g['hlen'][b])


@pytest.mark.parametrize('name', ['g1_tiny_l2', 'g1_tiny_l3'])
def test_streamed_equals_whole_utterance_float64(name):
    """The same operations, only split: the streamed log-probs equal the whole-utterance forward of x[b, :T_b] to 1e-12 in float64."""
    g = load_golden(name)
    enc = {k: v.double() for k, v in _params(g, 'encoder.').items()}
    rec = {k: v.double() for k, v in _params(g, 'recognizer.').items()}
    x = torch.from_numpy(g['x']).double()
    lengths = [41, 23, 9]
    ref = stream_ref.stream_all(stream_ref.StreamRef(enc, rec, 3, torch.float64), x, lengths, 8)
    for b, T in enumerate(lengths):
        with torch.no_grad():
            feats, flen, _ = cpu_ref.encoder_forward(enc, x[b:b + 1, :T], torch.tensor([T]))
            whole = cpu_ref.classifier_log_probs(rec, feats)[0]
        got = ref.log_probs(b)
        assert got.shape == whole.shape and got.shape[0] == int(flen[0])
        assert (got - whole).abs().max().item() <= 1e-12
        assert ref.rows[b]['ali'] == whole.argmax(-1).tolist()
        assert ref.rows[b]['hyp'] == stream_ref.collapse(whole.argmax(-1).tolist())[0]


def test_step_counts_add_up():
    for chunk in (4, 8, 16):
        T = torch.arange(1, 131)
        want = cpu_ref.subsampled_lengths(T).tolist()
        for t, w in zip(T.tolist(), want):
            assert (t // chunk) * (chunk // 4) + stream_ref.finish_steps(t % chunk) == w, (t, chunk)


def test_schedule_closes_rows_while_others_go_on():
    calls = stream_ref.schedule([41, 23, 9], 8)
    assert [c[0] for c in calls] == ['push', 'finish', 'push', 'finish', 'push', 'push', 'push', 'finish']
    assert calls[1][1:] == ([False, False, True], [0, 0, 1]) and calls[3][1:] == ([False, True, False], [0, 7, 0])
    assert calls[-1][1:] == ([True, False, False], [1, 0, 0])
