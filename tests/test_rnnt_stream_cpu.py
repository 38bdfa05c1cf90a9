"""CPU tests of the float64 restatement of the carried greedy transducer search (tests/rnnt_stream_ref.py): under every
chunk schedule it equals ``rnnt_greedy_ref.greedy`` of the frames sent so far after every call, and the fixtures and schedules meet
the conditions that make tests/test_gpu_rnnt_stream.py meaningful.  No GPU."""
import pytest
import torch

import rnnt_greedy_ref as R
import rnnt_stream_ref as SR

FIXTURES = ('small', 'rows17', 'rows17_long')


def run(name, kind, after_call=None):
    """Streams fixture ``name`` by schedule ``kind`` -> (the restatement, the plan); after_call(j, stream, cursors) after every call."""
    sd, x, il, cap, _ = R.fixture(name)
    N, T = x.shape[:2]
    F = SR.logits(sd, x)
    calls = SR.plan(kind, il.tolist(), T)
    s = SR.GreedyStreamRef(sd, N, cap, R.MAX_SYMBOLS)
    cur = [0] * N
    for j, counts in enumerate(calls):
        s.advance(SR.chunk(F, cur, counts, float('nan')), counts, [j == 0] * N)       # NaN wherever the search may not read
        cur = [a + c for a, c in zip(cur, counts)]
        if after_call:
            after_call(j, s, cur)
    return s, calls


@pytest.mark.parametrize('kind', SR.SCHEDULES)
@pytest.mark.parametrize('name', FIXTURES)
def test_carried_search_equals_the_whole_search_of_the_prefix(name, kind):
    sd, x, il, cap, ref = R.fixture(name)

    def after_call(j, s, cur):
        want = R.greedy(sd, x, torch.tensor(cur), cap, R.MAX_SYMBOLS)
        got = s.result()
        for k in ('tokens', 'lengths', 'frames', 'truncated'):
            assert torch.equal(got[k], want[k]), (name, kind, j, k)
        assert float((got['scores'] - want['scores']).abs().max()) <= 1e-12, (name, kind, j)

    s, calls = run(name, kind, after_call)
    got = s.result()
    assert torch.equal(got['tokens'], ref['tokens']) and torch.equal(got['frames'], ref['frames'])      # every row is through
    assert s.gap >= 1e-3, s.gap


def test_conditions_of_the_gpu_cases():
    s, calls = run('rows17', 'fours')
    stats = s.calls
    assert [c['rounds'] for c in stats] == [7, 8, 6, 5, 7, 1]                       # both parities at a call boundary
    sitting_out = [any(c['emitted']) and any(e == 0 and not t for e, t in zip(c['emitted'], c['took_part'])) for c in stats]
    assert sum(sitting_out) == 5                                                   # a row sits out while another emits
    assert sum(sum(c['truncated_here']) for c in stats) == 4                       # rows truncate in the middle of a call
    for c, counts in zip(stats, calls):
        for n, t in enumerate(c['truncated_here']):
            if t:
                assert c['emitted'][n] >= 1 and counts[n] >= 1
    per_call = {e for c in stats for e, t in zip(c['emitted'], c['took_part']) if t}
    assert 0 in per_call and 1 in per_call and max(per_call) >= 2
    for name in FIXTURES:
        s, _ = run(name, 'fours')
        assert sum(sum(c['forced']) for c in s.calls) >= 1, name
    s, calls = run('rows17', 'ones')
    assert not any(calls[-1]) and s.calls[-1]['rounds'] == 0 and not any(s.calls[-1]['took_part'])
    s, _ = run('rows17_long', 'whole')
    from haloop_amd import transducer
    assert [c['rounds'] for c in s.calls] == [31] and 31 > transducer.SYNC_EVERY     # the host read of the live word is exercised


def test_staggered_rows_pause_over_an_odd_call_and_emit_again():
    """The case a wrong masked cell or a lost copy parity fails: a row that has emitted gets no frames in a call of an odd number of
    rounds and emits again afterwards."""
    s, calls = run('rows17', 'staggered')
    found = []
    for n in range(17):
        emitted = [c['emitted'][n] for c in s.calls]
        for j in range(1, len(calls) - 1):
            if calls[j][n] == 0 and s.calls[j]['rounds'] % 2 == 1 and any(emitted[:j]) and any(emitted[j + 1:]):
                found.append((n, j))
    assert found, 'no row pauses across an odd call between two emissions'
    paused = [n for n in range(17) if any(calls[j][n] == 0 and any(calls[k][n] for k in range(j + 1, len(calls))) for j in range(1, len(calls)))]
    assert len(paused) >= 8


def test_fast_case_has_a_decided_search():
    """tests/test_gpu_rnnt_stream.py compares StreamingTransducer's final hypotheses with the float64 search on the float64 logits of the
    chunked encoder: every free argmax of every row is decided by at least 1e-3, rows emit, truncate and run out."""
    c = SR.fast_case()
    assert c['gap'] >= 1e-3, c['gap']
    lengths, truncated = c['search']['lengths'].tolist(), c['search']['truncated'].tolist()
    assert [f.shape[0] for f in c['logits']] == [21, 21, 21, 21, 15]
    assert all(l > 0 for l in lengths) and any(truncated) and not all(truncated)
    assert sum(sum(s['forced']) for s in c['stats']) >= 1
