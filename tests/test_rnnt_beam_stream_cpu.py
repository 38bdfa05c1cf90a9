"""CPU checks of the float64 restatement of the carried transducer beam search (tests/rnnt_beam_stream_ref.py): what makes the cases
of tests/test_gpu_rnnt_beam_stream.py meaningful.  Under every script the finals after the last call are ``rnnt_beam_ref.beam_search``'s
over the whole utterance -- the stall rule executes the whole search's steps and no others --, and the scripts reach the conditions the
device code has branches for: frames read from earlier calls, a ring that wraps, calls that end on either round parity, a row that
stalls while another steps, rows that pause and resume.
"""
import functools

import pytest
import torch

import rnnt_beam_ref as BR
import rnnt_beam_stream_ref as R

CASES = [('small', 4), ('small', 1), ('rows17', 4), ('rows17', 8)]


@functools.lru_cache(maxsize=None)
def streamed(name, W, kind):
    sd, features, il, cap, whole = BR.fixture(name, W)
    calls = R.script(kind, il.tolist(), features.shape[1])
    ref = R.BeamStreamRef(sd, features.shape[0], cap, W)
    R.run(ref, R.logits(name), calls)
    return ref, calls, whole, cap, features.shape[1], il.tolist()


@pytest.mark.parametrize('kind', R.SCHEDULES)
@pytest.mark.parametrize('name,W', CASES)
def test_finals_after_the_last_call_are_the_whole_search(name, W, kind):
    ref, calls, whole, cap, T, il = streamed(name, W, kind)
    got = ref.nbest()
    assert all(r['closed'] and not r['beam'] for r in ref.rows)
    assert torch.equal(got['counts'], whole['counts']) and torch.equal(got['lengths'], whole['lengths'])
    assert torch.equal(got['tokens'], whole['tokens'])
    assert torch.equal(got['scores'], whole['scores'])                  # the same float64 operations in the same order
    # every call stays within the rounds the device allows, and the ring of capacity + S + 1 frames holds every frame read
    S = R.max_chunk(calls)
    assert all(c['rounds'] <= max(1, max(counts)) + cap + 2 for c, (counts, _, _) in zip(ref.calls, calls))
    assert ref.reach <= cap + S + 1 and ref.spread <= cap


@pytest.mark.parametrize('name,W', CASES)
def test_the_scripts_reach_the_carried_search_s_branches(name, W):
    parities, old, wraps, uneven = set(), 0, 0, 0
    for kind in R.SCHEDULES:
        ref, calls, whole, cap, T, il = streamed(name, W, kind)
        p = 0
        for c in ref.calls:
            p = (p + c['rounds']) % 2
            parities.add(p)
            old += sum(c['old_reads'])
            ex = c['executed']
            uneven += any(c['stalled'][a] and ex[a] < max(ex) for a in range(len(ex)))
        wraps += max(il) > cap + R.max_chunk(calls) + 1
    assert parities == {0, 1}                   # calls end on both parities of the needed rounds
    assert old > 0                              # some step reads a frame that arrived in an earlier call
    assert wraps > 0                            # the ring wraps: a row is longer than capacity + S + 1
    assert uneven > 0                           # in some call a row stalls, its beam kept, while another still steps


@pytest.mark.parametrize('name', ['small', 'rows17'])
def test_rows_pause_and_resume_and_both_ways_to_become_final_occur(name):
    sd, features, il, cap = BR.inputs(name)
    calls = R.script('staggered', il.tolist(), features.shape[1])
    N = len(il)
    paused = 0
    for n in range(N):
        got = [counts[n] for counts, _, _ in calls]
        paused += any(a > 0 and b == 0 and any(c > 0 for c in got[j + 2:]) for j, (a, b) in enumerate(zip(got, got[1:])))
    assert paused > 0
    with_frames = sum(final[n] and counts[n] > 0 for counts, _, final in calls for n in range(N))
    without = sum(final[n] and counts[n] == 0 for counts, _, final in calls for n in range(N))
    assert with_frames > 0 and without > 0
    assert all(sum(final[n] for _, _, final in calls) == 1 for n in range(N))
    if name == 'rows17':                         # the row of no frames is final in the call it begins in, or in a later empty one
        assert 0 in il.tolist()


def test_the_stalled_beam_is_the_whole_search_s_beam_at_that_step():
    """An open row's beam after a call equals the beam of the whole search at the same step: the streamed search of the prefix with
    one more call that only marks the rows final gives ``beam_search`` of the prefix."""
    name, W = 'small', 4
    sd, features, il, cap, _ = BR.fixture(name, W)
    F = R.logits(name)
    cut = [7, 5, 1]
    ref = R.BeamStreamRef(sd, 3, cap, W)
    ref.advance(F[:, :4], [4, 4, 1], [True] * 3)
    ref.advance(F[:, 4:7], [3, 1, 0])
    assert all(not ref.hypotheses(n)[0] and ref.hypotheses(n)[1] for n in range(3))
    ref.advance(F[:, :1], [0, 0, 0], None, [True] * 3)
    want = BR.beam_search(sd, features, torch.tensor(cut), cap, W)
    got = ref.nbest()
    assert torch.equal(got['tokens'], want['tokens']) and torch.equal(got['scores'], want['scores'])
