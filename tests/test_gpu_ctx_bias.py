"""GPU tests of contextual biasing inside the CTC prefix beam search (haloop_amd.biasing.ContextGraph,
ctc.ctc_prefix_beam_search(context=...), ctc.PrefixBeamStream(context=...), TemporalClassifier.set_context,
StreamingRecognizer(context=...); the BIASED instantiations of csrc/ctc_prefix_beam.hip), in fp32.

Against the float64 restatement (tests/ctx_bias_ref.py): tokens, lengths, counts and states equal on every row the fixture does not leave
out (none is: tests/test_ctx_bias_cpu.py asserts that every prune and final ranking is decided by a gap of at least 1e-3); scores and
boosts rtol 1e-5 / atol 1e-4, the tolerance of tests/test_gpu_ctc_prefix_beam.py.  Everything else is exact: zero gain against the
unbiased search, boosts and states against ContextGraph.boost, the carried search against the whole one.

The launcher's dispatch is BIASED times the unbiased search's four paths, in both entry points; the fixtures that reach them:
emissions and token rows in LDS (small, rows17, rows17cap, wide, long, tiny), token rows in the workspace / in the state (deep),
emissions from L2 (stream), both with 32-bit tokens (huge).  A thread keeps the columns of its first four classes in registers and reads
those of further classes from L2, at V > 1025: stream (4100) and huge (70000) reach that, wide (300) has two classes in registers.  No
table is cached in LDS, so there is no wide-graph path to reach.
"""
import numpy as np
import pytest
import torch

import ctc_prefix_beam_ref as R
import ctx_bias_ref as C
import stream_beam_ref as SB
import stream_ref
from test_gpu_ctc_prefix_beam import check, float64_log_probs, head_inputs, same, tiny_head
from test_gpu_streaming import FAST, _modules, hal  # noqa: F401  (hal is a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def plain(e, il, W, capacity):
    from haloop_amd import ctc
    return ctc.ctc_prefix_beam_search(e, il, W, capacity)


def biased(e, il, W, capacity, graph):
    from haloop_amd import ctc
    out = ctc.ctc_prefix_beam_search(e, il, W, capacity, context=graph, return_parts=True)
    assert len(out) == 6 and out[4].dtype == torch.float32 and out[5].dtype == torch.int64 and out[4].shape == out[5].shape == out[1].shape
    return out


@pytest.fixture(scope='module')
def device_runs():
    """The biased search of every case on the device, once: (name, W) -> the six outputs."""
    return {(name, W): biased(R.inputs(name)[0].to(DEV), R.inputs(name)[1].to(DEV), W, R.inputs(name)[2], C.graph(name, W))
            for name, W in C.CASES}


# -------------------------------------------------------------------------------------------- 1. zero gain is the unbiased search
@pytest.mark.parametrize('name,W', R.CASES)
def test_zero_gain_is_the_unbiased_search_bit_for_bit(name, W):
    from haloop_amd.biasing import ContextGraph
    e, il, capacity = R.inputs(name)
    ed, ild = e.to(DEV), il.to(DEV)
    want = plain(ed, ild, W, capacity)
    assert len(C.graph(name, W, 0.0).phrases) > 0
    for graph in (ContextGraph([], e.shape[2], 2.0), C.graph(name, W, 0.0)):
        got = biased(ed, ild, W, capacity, graph)
        assert same(got[:4], want), (name, W, graph.num_states)         # every row
        tokens, lengths, states = want[0].cpu(), want[1].cpu(), got[5].cpu()
        assert not bool(got[4].any())
        for n in range(tokens.shape[0]):                                # the states are still the graph's: the lookups did run
            for w in range(W):
                L = int(lengths[n, w])
                assert int(states[n, w]) == (graph.boost(tokens[n, w, :L].tolist())[0] if L >= 0 else -1)


# ------------------------------------------------------------------------------------------------- 2. against the float64 restatement
@pytest.mark.parametrize('name,W', C.CASES)
def test_fixture_equals_the_restatement(name, W, device_runs):
    ref = C.fixture(name, W)[3]
    got = device_runs[name, W]
    rows = C.compared_rows(name, W)
    check(got[:4], ref, rows, f'{name} W={W} biased')
    boosts, states = got[4].cpu(), got[5].cpu()
    assert torch.equal(states[rows], ref['states'][rows])
    np.testing.assert_allclose(boosts[rows].numpy(), ref['boosts'][rows].numpy(), rtol=1e-5, atol=1e-4)


# ---------------------------------------------------------------------------------------------------- 3. boosts and states, exactly
@pytest.mark.parametrize('name,W', C.CASES)
def test_boosts_and_states_are_the_graphs_bit_for_bit(name, W, device_runs):
    tokens, lengths, scores, counts, boosts, states = (t.cpu() for t in device_runs[name, W])
    g = C.graph(name, W)
    for n in range(tokens.shape[0]):                                    # every present hypothesis of every row
        count = int(counts[n])
        assert count >= 1
        for w in range(count):
            state, z = g.boost(tokens[n, w, :int(lengths[n, w])].tolist())
            assert int(states[n, w]) == state and float(boosts[n, w]) == z, (n, w)
        assert bool((states[n, count:] == -1).all()) and not bool(boosts[n, count:].any())
        assert bool((lengths[n, count:] == -1).all()) and bool((scores[n, count:] == float('-inf')).all())


def test_without_pruning_score_minus_boost_is_the_training_loss(device_runs):
    """tiny at W = 16: nothing is pruned, whatever the ranks, so scores - boosts is -functional.ctc_loss(reduction='none')."""
    from haloop_amd import functional as HF
    e, il, capacity = R.inputs('tiny')
    ed, ild = e.to(DEV), il.to(DEV)
    tokens, lengths, scores, counts, boosts, states = device_runs['tiny', 16]
    assert counts.tolist() == [13, 13] and bool(boosts.any())
    hyp = tokens[:, :13].reshape(26, -1).clamp(min=0)
    rows = torch.arange(2, device=DEV).repeat_interleave(13)
    losses = HF.ctc_loss(ed[:, rows].contiguous(), hyp, ild[rows], lengths[:, :13].reshape(26), reduction='none')
    mass = (scores - boosts)[:, :13].reshape(26)
    print('max |score - boost + loss|', float((mass + losses).abs().max()))
    np.testing.assert_allclose(mass.cpu().numpy(), -losses.cpu().numpy(), rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------ 4. the carried search
def new_stream(name, W, graph):
    from haloop_amd import ctc
    f = R.FIXTURES[name]
    return ctc.PrefixBeamStream(f['N'], f['V'], W, f['capacity'], device=DEV, context=graph)


def six(stream):
    return stream.nbest() + stream.parts()


def equals_whole(got, ed, ild, W, capacity, graph, frames):
    """The stream's six outputs against the whole biased search of every row's first min(L, frames) frames; the whole search takes a
    capacity of at most its T, below which nothing can have been refused, and the stream's further columns hold -1."""
    cap = min(capacity, frames)
    want = biased(ed[:frames], ild.clamp(max=frames), W, cap, graph)
    assert torch.equal(got[0][:, :, :cap], want[0]) and bool((got[0][:, :, cap:] == -1).all())
    assert all(torch.equal(a, b) for a, b in zip(got[1:], want[1:]))


CARRIED = [(name, W, spec) for (name, W) in C.CASES for spec in SB.SCHEDULES[(name, W)]] + \
          [(name, W, spec) for (name, W) in (('small', 4), ('rows17', 8)) for spec in (3, 7)] + [('rows17', 4, 1), ('long', 4, 3)]


@pytest.mark.parametrize('name,W,spec', CARRIED, ids=[f'{n}-{w}-{s}' for n, w, s in CARRIED])
def test_carried_equals_whole_after_every_call(name, W, spec):
    """Chunks of 1, 3 and 7 frames (and the schedules of tests/stream_beam_ref.py, which reach the four dispatch paths of the carried
    entry point), ragged n_frames from the fixture's lengths; then one row is restarted by begin while the others get no frames."""
    e, il, capacity = R.inputs(name)
    ed, ild = e.to(DEV), il.to(DEV)
    T, N, _ = e.shape
    graph = C.graph(name, W)
    stream = new_stream(name, W, graph)
    assert stream.counts.tolist() == [0] * N and bool((stream.states == -1).all())
    for i, (off, size) in enumerate(SB.calls(T, spec)):
        nf = (ild - off).clamp(0, size)
        views = stream.advance(ed[off:off + size], nf, torch.ones(N, dtype=torch.bool, device=DEV) if i == 0 else None)
        assert len(views) == 4
        equals_whole(six(stream), ed, ild, W, capacity, graph, off + size)
    last = six(stream)
    state = stream.state.clone()
    r, size = N - 1, min(3, T)                                          # row r again from the empty prefix; no other row takes part
    begin = torch.zeros(N, dtype=torch.bool, device=DEV)
    begin[r] = True
    nf = torch.zeros(N, dtype=torch.int64, device=DEV)
    nf[r] = size
    stream.advance(ed[:size], nf, begin)
    got = six(stream)
    others = [n for n in range(N) if n != r]
    assert all(torch.equal(a[others], b[others]) for a, b in zip(got, last)) and torch.equal(stream.state[others], state[others])
    equals_whole([t[r:r + 1] for t in got], ed[:, r:r + 1], nf[r:r + 1], W, capacity, graph, size)


# ------------------------------------------------------------------------------------------------------------------ 5. housekeeping
@pytest.mark.parametrize('name,W', [('small', 4), ('rows17', 4)])
def test_padding_is_never_read(name, W, device_runs):
    e, il, capacity = R.inputs(name)
    ed, ild = e.to(DEV), il.to(DEV)
    graph, clean = C.graph(name, W), device_runs[name, W]
    T, N, V = e.shape
    poisoned = ed.clone()
    for n, L in enumerate(il.tolist()):
        poisoned[L:, n] = float('nan')                                  # frames at or past the row's length
    assert same(biased(poisoned, ild, W, capacity, graph), clean)
    big = torch.full((N + 1, T + 2, V + 3), float('nan'), device=DEV)   # the gaps of a strided view: rows, frames and classes beyond it
    big[:N, :T, :V] = poisoned.permute(1, 0, 2)
    view = big[:N, :T, :V].permute(1, 0, 2)
    assert view.stride(2) == 1 and not view.is_contiguous()
    assert same(biased(view, ild, W, capacity, graph), clean)


@pytest.mark.parametrize('name,W', [('rows17', 8), ('long', 16), ('deep', 16)])
def test_calls_repeat_and_an_unbiased_call_between_changes_neither(name, W, device_runs):
    e, il, capacity = R.inputs(name)
    ed, ild = e.to(DEV), il.to(DEV)
    graph = C.graph(name, W)
    before = plain(ed, ild, W, capacity)
    first = biased(ed, ild, W, capacity, graph)
    between = plain(ed, ild, W, capacity)
    third = biased(ed, ild, W, capacity, graph)
    assert same(first, third) and same(first, device_runs[name, W]) and same(before, between)
    assert not same(first[:4], before)


def test_one_launch_per_call_and_nothing_read_from_the_device(monkeypatch):
    """The library calls of one biased search and of one biased advance, counted, under torch's sync debug mode (a read from the device
    raises): one entry point each, which is one kernel launch (csrc/ctc_prefix_beam.hip's launch())."""
    from haloop_amd import _lib, ctc, ops
    e, il, capacity = R.inputs('rows17')
    ed, ild = e.to(DEV), il.to(DEV)
    graph = C.graph('rows17', 4)
    stream = new_stream('rows17', 4, graph)
    nf, begin = ild.clamp(max=5), torch.ones(17, dtype=torch.bool, device=DEV)
    biased(ed, ild, 4, capacity, graph)                                 # (the tables are on the device from here on)
    calls, handle = [], _lib.lib()

    class Counting:
        def __getattr__(self, name):
            return lambda *a: (calls.append(name), getattr(handle, name)(*a))[1]

    monkeypatch.setattr(ops, 'lib', lambda: Counting())
    torch.cuda.set_sync_debug_mode('error')
    try:
        ctc.ctc_prefix_beam_search(ed, ild, 4, capacity, context=graph, return_parts=True)
        stream.advance(ed[:5], nf, begin)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [c for c in calls if not c.endswith('_bytes')] == ['halo_ctc_prefix_beam_biased', 'halo_ctc_prefix_beam_advance_biased']


def test_planted_phrase_is_recovered_on_the_device():
    from haloop_amd.biasing import ContextGraph
    f = C.PLANTED
    e, il, cap = C.planted_inputs()
    ed, ild = e.to(DEV), il.to(DEV)
    ref = C.beam_search(e, il, cap, f['W'], [f['phrase']], f['bonus'])
    lost = plain(ed, ild, f['W'], cap)
    got = biased(ed, ild, f['W'], cap, ContextGraph([f['phrase']], f['V'], f['bonus']))
    check(lost, R.beam_search(e, il, cap, f['W']), [0], 'planted, unbiased')
    check(got[:4], ref, [0], 'planted, biased')
    assert got[0][0, 0, :int(got[1][0, 0])].tolist() == list(f['phrase']) and float(got[4][0, 0]) == 2 * f['bonus']
    assert all(lost[0][0, w, :int(lost[1][0, w])].tolist() != list(f['phrase']) for w in range(int(lost[3][0])))


# ------------------------------------------------------------------------------------------------------------------- 6. the heads
def test_temporal_classifier_set_context():
    """The tiny head of tests/test_gpu_ctc_prefix_beam.py with three phrases over its four labels (ctx_bias_ref.random_phrases(4, 5, 3):
    the float64 search decides every ranking by a gap of 9e-2, asserted below)."""
    import copy
    import ctc_lm_beam_ref as LM
    from haloop_amd.biasing import ContextGraph
    head = tiny_head().to(DEV).eval()
    features, il = head_inputs()
    x, ild = features.to(DEV), il.to(DEV)
    phrases = C.random_phrases(4, 5, count=3)
    ref = C.beam_search(float64_log_probs(head, features).permute(1, 0, 2), il, 6, 4, phrases, C.BONUS)
    print('phrases', phrases, 'gaps', ref['gaps'].tolist(), 'boosts', ref['boosts'].tolist())
    assert float(ref['gaps'].min()) >= C.GAP                            # (this test's own fixture condition)
    today = head.decode(x, ild, None, beam_size=4)
    today_nbest = head.last_nbest
    assert head.last_parts is None

    head.set_context(ContextGraph(phrases, 5, C.BONUS))
    assert list(head.state_dict()) == ['classifier.weight', 'classifier.bias']
    hypotheses, output_lengths, alignments, scores, nothing = head.decode(x, ild, None, beam_size=4)
    assert nothing is None and alignments == [None] * 3
    assert output_lengths.tolist() == ref['lengths'][:, 0].tolist()
    for n, hyp in enumerate(hypotheses.unbind()):
        assert torch.equal(hyp.cpu(), ref['tokens'][n, 0, :ref['lengths'][n, 0]])
    np.testing.assert_allclose(scores.cpu().numpy(), ref['scores'][:, 0].numpy(), rtol=1e-5, atol=1e-4)
    check(head.last_nbest, ref, range(3), 'last_nbest, biased')
    ctc_scores, boosts = head.last_parts
    np.testing.assert_allclose(boosts.cpu().numpy(), ref['boosts'].numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(ctc_scores.cpu().numpy(), (ref['scores'] - ref['boosts']).numpy(), rtol=1e-5, atol=1e-4)
    assert not same(head.last_nbest, today_nbest)
    # greedy decoding ignores the context
    from haloop_amd import ops
    with torch.no_grad():
        want = ops.ctc_greedy(head.log_probs(x).contiguous())
    greedy = head.decode(x, ild, None)
    assert torch.equal(greedy[2], want[0]) and torch.equal(greedy[3], want[1])

    # an LM and a context: not built
    head.set_lm(copy.deepcopy(LM.language_model(5, 2, 1)[0]).to(DEV))
    with pytest.raises(NotImplementedError, match='fus'):
        head.decode(x, ild, None, beam_size=4)
    head.set_lm(None)

    head.set_context(None)
    again = head.decode(x, ild, None, beam_size=4)
    assert head.last_parts is None and same(head.last_nbest, today_nbest)
    assert torch.equal(again[3], today[3]) and again[1].tolist() == today[1].tolist()


def drive(sr, x, lengths, chunk, graph, verify):
    """tests/test_gpu_stream_beam.py's drive with a context: after every call ``nbest()`` and ``nbest_parts()`` of every slot must equal
    ``ctc_prefix_beam_search(context=graph)`` of the slot's streamed log-probs so far, bit for bit.
    -> [(nbest + parts, partial, the call's greedy alignments and step scores)] on the CPU, one per call."""
    B, W, capacity = x.shape[0], sr.beam, sr.capacity
    lp, record = [[] for _ in range(B)], []
    for call in stream_ref.schedule(lengths, chunk):
        if call[0] == 'push':
            _, k, active = call
            sr.push(x[:, k * chunk:(k + 1) * chunk].contiguous(), active, [a and k == 0 for a in active], want_log_probs=True)
        else:
            _, rows, tails = call
            sr.finish(stream_ref.tail_tensor(x, lengths, chunk, rows, tails), tails, rows, want_log_probs=True)
        n = sr.last[2].tolist()
        for b in range(B):
            lp[b].append(sr.last[3][b, :n[b]].clone())
        got = sr.nbest() + (sr.nbest_parts() if graph is not None else ())
        part = sr.partial()
        record.append(([t.cpu() for t in got], [t.cpu() for t in part], [sr.last[0].cpu().clone(), sr.last[1].cpu().clone()]))
        if not verify:
            continue
        for b in range(B):
            e = torch.cat(lp[b])[:, None, :]
            cap = min(capacity, e.shape[0])
            want = biased(e, None, W, cap, graph)
            assert torch.equal(got[0][b:b + 1, :, :cap], want[0]) and bool((got[0][b, :, cap:] == -1).all()), b
            assert all(torch.equal(a[b:b + 1], w) for a, w in zip(got[1:], want[1:])), b
        assert torch.equal(part[1], got[1][:, 0]) and torch.equal(part[2], got[2][:, 0])
    return record


def test_streaming_recognizer_with_a_context(hal):
    """The fast-path encoder of tests/test_gpu_streaming.py (5 streams, chunks of 16, row 4 closing early), capacity 8 below a stream's
    21 steps.  The phrases are cut from the unbiased run's own n-best lists (the first three tokens of every slot's second hypothesis),
    so they are spelled."""
    from oracle import cpu_ref
    from haloop_amd.biasing import ContextGraph
    c = FAST
    enc_p, rec_p = cpu_ref.make_params(c['F_'], c['C'], c['H'], c['L'], c['V'], seed=42)
    rec_p['classifier.weight'] = rec_p['classifier.weight'] * 100
    x = (8 * torch.randn(c['B'], c['T'], c['F_'], generator=torch.Generator().manual_seed(43))).to(DEV)
    enc, rec = _modules(hal, enc_p, rec_p)
    S = hal['streaming'].StreamingRecognizer
    with pytest.raises(ValueError):
        S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=8, beam=0, context=ContextGraph([(1,)], c['V']))
    unbiased = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=8, use_graph=False, beam=4)
    rec_u = drive(unbiased, x, c['lengths'], c['chunk'], None, verify=False)
    with pytest.raises(ValueError):
        unbiased.nbest_parts()
    tokens, lengths = rec_u[-1][0][0], rec_u[-1][0][1]
    phrases = [tuple(tokens[b, 1, :min(3, int(lengths[b, 1]))].tolist()) for b in range(c['B']) if int(lengths[b, 1]) > 0]
    assert phrases
    graph = ContextGraph(phrases, c['V'], C.BONUS)
    eager = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=8, use_graph=False, beam=4, context=graph)
    rec_e = drive(eager, x, c['lengths'], c['chunk'], graph, verify=True)
    replay = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=8, use_graph=True, beam=4, context=graph)
    rec_g = drive(replay, x, c['lengths'], c['chunk'], graph, verify=True)
    assert replay._graphs
    print('phrases', phrases, 'boosts', rec_e[-1][0][4].tolist())
    assert bool(rec_e[-1][0][4].any()) and not same(rec_e[-1][0][:4], rec_u[-1][0])
    for (got_e, part_e, greedy_e), (got_g, part_g, greedy_g), (_, _, greedy_u) in zip(rec_e, rec_g, rec_u):
        assert same(got_e, got_g) and same(part_e, part_g)
        assert same(greedy_e, greedy_u) and same(greedy_g, greedy_u)   # the greedy outputs are unchanged by the context
    assert torch.equal(eager._hyp, unbiased._hyp) and torch.equal(eager._hyp_len, unbiased._hyp_len)
