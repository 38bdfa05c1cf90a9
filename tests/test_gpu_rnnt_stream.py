"""GPU tests of the carried greedy transducer search (haloop_amd.transducer.GreedyStream, csrc/rnnt_decode.hip) and of streaming
transducer recognition (haloop_amd.streaming.StreamingTransducer, csrc/stream.hip), in `bf16x3` unless said otherwise.

The carried search is held to ``GreedyDecoder.decode`` of the frames sent so far bit for bit, scores included: both add the same fp32
terms in the same order from a bit-identical g.  Against the float64 restatement (tests/rnnt_stream_ref.py) the integers are exact and
the scores within rtol 1e-5 / atol 1e-4, tests/test_gpu_rnnt_decode.py's ``check``.  tests/test_rnnt_stream_cpu.py asserts on the CPU what
makes these cases meaningful (both round parities at a call boundary, rows that sit out, truncate, pause and resume).
"""
import numpy as np
import pytest
import torch

import rnnt_greedy_ref as R
import rnnt_stream_ref as SR
import stream_ref
from test_gpu_rnnt_decode import check, head_of, math_mode, same

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


@pytest.fixture(autouse=True)
def bf16x3():
    with math_mode('bf16x3'):
        yield


_cases = {}


def case(name):
    """The fixture on the device, its head, a whole-utterance decoder and f = the call GreedyDecoder makes; computed once, never changed."""
    if name not in _cases:
        from haloop_amd import functional as HF, transducer
        sd, x, il, cap, ref = R.fixture(name)
        head = head_of(sd)
        xd = x.to(DEV)
        with torch.no_grad():
            f = HF.linear(xd.float(), head.classifier.weight, head.classifier.bias).contiguous()
        _cases[name] = dict(sd=sd, x=xd, il=il.tolist(), cap=cap, ref=ref, head=head, f=f, N=x.shape[0], T=x.shape[1],
                            whole=transducer.GreedyDecoder(head, x.shape[0], cap, R.MAX_SYMBOLS))
    return _cases[name]


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def stream(gs, f, calls, fill=NAN, begin_at=0, after_call=None):
    """Feeds f [N, T, V] to ``gs`` by the plan ``calls`` (every row begins at call ``begin_at``) -> the cursors."""
    N = f.shape[0]
    cur = [0] * N
    for j, counts in enumerate(calls):
        out = gs.advance(SR.chunk(f, cur, counts, fill), i32(counts), [True] * N if j == begin_at else None)
        cur = [a + c for a, c in zip(cur, counts)]
        if after_call:
            after_call(j, cur, out)
    return cur


# ------------------------------------------------------------------------------------------------- 1. bit equality with the whole search
@pytest.mark.parametrize('kind', SR.SCHEDULES)
@pytest.mark.parametrize('name', ['small', 'rows17', 'rows17_long'])
def test_every_call_equals_the_whole_search_of_the_prefix(name, kind):
    from haloop_amd import transducer
    c = case(name)
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    assert gs.fused
    rounds = []

    def after_call(j, cur, out):
        want = c['whole'].decode(c['x'], i32(cur))
        got = gs.result()
        for a, b, what in zip(got, want, ('tokens', 'lengths', 'frames', 'scores', 'truncated')):
            assert torch.equal(a, b), (name, kind, j, what)
        assert same(out, got)                                            # (B == max_rows: the views are the whole buffers)
        rounds.append(gs.rounds)

    stream(gs, c['f'], SR.plan(kind, c['il'], c['T']), after_call=after_call)
    print(name, kind, 'rounds', rounds)
    check(gs.result(), c['ref'], f'{name} {kind}')


@pytest.mark.parametrize('kind', ['ones', 'staggered'])
def test_odd_number_of_steps_per_call(kind):
    """Three symbols per frame: chunks of one frame then take 3 + 1 advances and 3 steps of the prediction network, so the copy that
    holds the state changes parity at every call boundary."""
    from haloop_amd import transducer
    c = case('rows17')
    whole = transducer.GreedyDecoder(c['head'], c['N'], c['cap'], 3)
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], 3)
    parities = set()

    def after_call(j, cur, out):
        parities.add(gs._cur)
        assert same(gs.result(), whole.decode(c['x'], i32(cur))), (kind, j)

    stream(gs, c['f'], SR.plan(kind, c['il'], c['T']), after_call=after_call)
    assert parities == {0, 1}


# ------------------------------------------------------------------------------------------------------------- 2. float64 reference
@pytest.mark.parametrize('name,kind', [('small', 'mixed'), ('rows17', 'fours'), ('rows17_long', 'staggered')])
def test_against_the_float64_restatement_after_every_call(name, kind):
    from haloop_amd import transducer
    c = case(name)
    calls = SR.plan(kind, c['il'], c['T'])
    ref = SR.GreedyStreamRef(c['sd'], c['N'], c['cap'], R.MAX_SYMBOLS)
    F64 = SR.logits(c['sd'], c['x'].cpu())
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    cur = [0] * c['N']
    for j, counts in enumerate(calls):
        begin = [j == 0] * c['N']
        ref.advance(SR.chunk(F64, cur, counts), counts, begin)
        gs.advance(SR.chunk(c['f'], cur, counts, NAN), i32(counts), begin)
        cur = [a + n for a, n in zip(cur, counts)]
        check(gs.result(), ref.result(), f'{name} {kind} call {j}')


# --------------------------------------------------------------------------------------------------------------- 3. no stray reads
@pytest.mark.parametrize('name', ['small', 'rows17'])
def test_frames_past_n_frames_and_idle_rows_are_never_read(name):
    """NaN in every frame at or past a row's n_frames and in every row that does not take part, against zeros there; the chunk is a
    strided slice of a wider buffer."""
    from haloop_amd import transducer
    c = case(name)
    calls = SR.plan('staggered', c['il'], c['T'])
    results = []
    for fill in (0.0, NAN):
        gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
        per_call = []
        cur = [0] * c['N']
        for j, counts in enumerate(calls):
            ch = SR.chunk(c['f'], cur, counts, fill)
            wide = torch.full((ch.shape[0], ch.shape[1] + 2, ch.shape[2] + 3), fill, device=DEV)
            wide[:, 1:-1, :ch.shape[2]] = ch
            gs.advance(wide[:, 1:-1, :ch.shape[2]], i32(counts), [j == 0] * c['N'])
            cur = [a + n for a, n in zip(cur, counts)]
            per_call.append(gs.result())
        results.append(per_call)
    for a, b in zip(*results):
        assert same(a, b)
    check(results[1][-1], c['ref'], name)


# --------------------------------------------------------------------------------------------------------------- 4. begin and reuse
def test_a_row_begun_again_abandons_its_stream():
    """Row 4 begins again at call 2 and is sent its utterance from the start while the others go on: the extra step of the prediction
    network changes the copy parity under every waiting and running row."""
    from haloop_amd import transducer
    c = case('rows17')
    N, il = c['N'], c['il']
    gs = transducer.GreedyStream(c['head'], N, c['cap'], R.MAX_SYMBOLS)
    cur, j = [0] * N, 0
    while any(a < l for a, l in zip(cur, il)):
        begin = [j == 0] * N
        if j == 2:
            assert cur[4] > 0 and int(gs.result()[1][4]) > 0            # (an open stream that has emitted)
            begin[4], cur[4] = True, 0
        counts = [min(4, l - a) for a, l in zip(cur, il)]
        gs.advance(SR.chunk(c['f'], cur, counts, NAN), i32(counts), begin)
        cur = [a + n for a, n in zip(cur, counts)]
        j += 1
    assert same(gs.result(), c['whole'].decode(c['x'], i32(il)))


def test_rows_reused_after_an_unrelated_utterance_repeat_bit_for_bit():
    from haloop_amd import transducer
    c = case('rows17')
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    calls = SR.plan('fours', c['il'], c['T'])
    first = []
    stream(gs, c['f'], calls, after_call=lambda j, cur, out: first.append(gs.result()))
    other = 3 * torch.randn(c['N'], 7, c['f'].shape[2], generator=torch.Generator().manual_seed(5)).to(DEV)
    gs.advance(other[:, :5], None, [True] * c['N'])                      # n_frames None: all 5; an odd number of calls
    gs.advance(other[:, 5:], i32([2] * c['N']))
    gs.advance(other[:, :3], None)
    again = []
    stream(gs, c['f'], calls, after_call=lambda j, cur, out: again.append(gs.result()))
    assert len(first) == len(again) and all(same(a, b) for a, b in zip(first, again))


def test_begin_without_frames_leaves_the_empty_hypothesis():
    from haloop_amd import transducer
    c = case('small')
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    stream(gs, c['f'], SR.plan('whole', c['il'], c['T']))
    assert int(gs.result()[1].sum()) > 0
    tokens, lengths, frames, scores, truncated = gs.advance(torch.full_like(c['f'][:, :2], NAN), i32([0] * c['N']), [True] * c['N'])
    assert lengths.tolist() == [0] * c['N'] and scores.tolist() == [0.0] * c['N'] and not truncated.any()
    assert bool((tokens == -1).all()) and bool((frames == -1).all())
    stream(gs, c['f'], SR.plan('fours', c['il'], c['T']), begin_at=-1)   # the rows go on from the empty hypothesis without another begin
    check(gs.result(), c['ref'], 'small after an empty begin')


# ------------------------------------------------------------------------------------------------------------------- 5. truncation
def test_a_truncated_row_is_unchanged_by_later_calls():
    from haloop_amd import transducer
    c = case('rows17')
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    stream(gs, c['f'], SR.plan('fours', c['il'], c['T']))
    before = gs.result()
    rows = before[4].nonzero().view(-1)
    assert rows.numel() >= 4 and c['ref']['truncated'].sum() == rows.numel()
    junk = torch.randn(c['N'], 6, c['f'].shape[2], generator=torch.Generator().manual_seed(9)).to(DEV)
    for _ in range(2):
        gs.advance(junk, i32([6 if t else 0 for t in before[4].tolist()]))
    after = gs.result()
    assert same(before, after)


# ------------------------------------------------------------------------------------------------------------------ 6. general path
def test_fused_path_equals_general_path():
    from haloop_amd import transducer
    c = case('rows17')
    calls = SR.plan('staggered', c['il'], c['T'])
    fused = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    stream(fused, c['f'], calls)
    with math_mode('f32'):
        general = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
        assert not general.fused
        per_call = []
        stream(general, c['f'], calls, after_call=lambda j, cur, out: per_call.append((list(cur), general.result())))
        for cur, got in per_call[::3] + per_call[-1:]:
            check(got, R.greedy(c['sd'], c['x'].cpu(), torch.tensor(cur), c['cap'], R.MAX_SYMBOLS), f'general path at {cur}')
    a, b = fused.result(), general.result()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    np.testing.assert_allclose(a[3].cpu().numpy(), b[3].cpu().numpy(), rtol=1e-5, atol=1e-4)


# -------------------------------------------------------------------------------------------------------------------- 7. stale image
def test_a_changed_weight_reaches_the_next_stream():
    from haloop_amd import transducer
    sd, x, il, cap, ref = R.fixture('rows17')
    head = head_of(sd)                                                   # (a head of this test's own: its weights change)
    gs = transducer.GreedyStream(head, 17, cap, R.MAX_SYMBOLS)
    calls = SR.plan('fours', il.tolist(), x.shape[1])

    def f_of():
        from haloop_amd import functional as HF
        with torch.no_grad():
            return HF.linear(x.to(DEV), head.classifier.weight, head.classifier.bias).contiguous()
    stream(gs, f_of(), calls)
    check(gs.result(), ref, 'rows17')
    with torch.no_grad():
        head.lm.rnn.weight_hh_l0.mul_(0.5)
    sd2 = {k: v.detach().cpu().clone() for k, v in head.state_dict().items()}
    ref2 = R.greedy(sd2, x, il, cap, R.MAX_SYMBOLS)
    assert ref2['gap'] >= 1e-3 and not torch.equal(ref2['tokens'], ref['tokens'])
    stream(gs, f_of(), calls)
    check(gs.result(), ref2, 'rows17, weight_hh_l0 halved')


def test_interface_errors():
    from haloop_amd import _lib, transducer
    c = case('small')
    gs = transducer.GreedyStream(c['head'], c['N'], c['cap'], R.MAX_SYMBOLS)
    f = c['f']
    with pytest.raises(ValueError):
        gs.advance(f[:, :, :-1])
    with pytest.raises(ValueError):
        gs.advance(f, torch.zeros(c['N'], dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        gs.advance(f, None, torch.zeros(c['N'], dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        gs.advance(f, None, [True])
    with pytest.raises(_lib.HaloError):
        gs.advance(f.cpu())
    with pytest.raises(ValueError):
        transducer.GreedyStream(c['head'], 0, 4)
    c['head'].train()
    try:
        with pytest.raises(NotImplementedError):
            gs.advance(f)
    finally:
        c['head'].eval()


# ----------------------------------------------------------------------------------------------------------- 8. StreamingTransducer
def _encoder(enc_p):
    from haloop_amd import rnn
    f = SR.FAST
    enc = rnn.Encoder(f['F_'], f['C'], f['H'], num_layers=f['L'])
    enc.load_state_dict(enc_p)
    return enc.to(DEV).eval()


def _run_transducer(st, x, twin=None):
    """Streams SR.FAST's rows through ``st`` by stream_ref.schedule -> (per row the logits of its steps, every call's partial())."""
    f = SR.FAST
    B, chunk, lengths = f['B'], f['chunk'], f['lengths']
    logits, partials = [[] for _ in range(B)], []
    for call in stream_ref.schedule(lengths, chunk):
        if call[0] == 'push':
            _, k, active = call
            begin = [a and k == 0 for a in active]
            st.push(x[:, k * chunk:(k + 1) * chunk].contiguous(), active, begin)
            rows = active
        else:
            _, rows, tails = call
            begin = None
            st.finish(stream_ref.tail_tensor(x, lengths, chunk, rows, tails), tails, rows)
        lg, n = st.last
        n = n.tolist()
        for b in range(B):
            assert (n[b] > 0) == bool(rows[b])
            assert not lg[b, n[b]:].any()                                # zeros past a row's steps
            logits[b].append(lg[b, :n[b]].cpu())
        partials.append([t.cpu() for t in st.partial()])
        if twin is not None:
            twin.advance(lg.clone(), st.last[1].clone(), begin)
            assert same(st.search.result(), twin.result())
    return [torch.cat(r) for r in logits], partials


@pytest.mark.parametrize('mode', ['bf16x3', 'f32', 'bf16'])
def test_streaming_transducer_at_the_fast_path_shape(mode):
    """LC-2x1024 under a Transducer(1024, 32), 5 streams in chunks of 16, row 4 ends after 57 frames.  (1) the decoder's outputs equal a
    separate GreedyStream fed ``last``'s logits after every call; (2) the streamed logits are at most twice as far from the float64
    restatement of the chunked encoder as the whole-utterance path (Encoder.forward + the classifier) is in the same mode: 3.3v's rule;
    (3) the final hypotheses equal the float64 search on the float64 logits."""
    from haloop_amd import functional as HF, streaming, transducer
    f, c = SR.FAST, SR.fast_case()
    with math_mode(mode):
        enc, head = _encoder(c['enc_p']), head_of(c['sd'])
        x = c['x'].to(DEV)
        e_whole = 0.0
        with torch.no_grad():
            for rows, T in ((slice(0, 4), 80), (slice(4, 5), 57)):
                feats, _, _ = enc(x[rows, :T].contiguous(), torch.full((rows.stop - rows.start,), T, device=DEV))
                lg = HF.linear(feats, head.classifier.weight, head.classifier.bias).cpu().double()
                for i, b in enumerate(range(rows.start, rows.stop)):
                    e_whole = max(e_whole, (lg[i] - c['logits'][b]).abs().max().item())
        st = streaming.StreamingTransducer(enc, head, f['B'], chunk_frames=f['chunk'], capacity=f['capacity'],
                                           max_symbols_per_frame=R.MAX_SYMBOLS)
        twin = transducer.GreedyStream(head, f['B'], f['capacity'], R.MAX_SYMBOLS)
        logits, partials = _run_transducer(st, x, twin)
        e_stream = max((logits[b].double() - c['logits'][b]).abs().max().item() for b in range(f['B']))
        print(f'streaming transducer {mode}: e_stream {e_stream:.3e} e_whole {e_whole:.3e} gap {c["gap"]:.3e}')
        hyp, hyp_len, scores, steps, truncated = partials[-1]
        assert steps.tolist() == [21, 21, 21, 21, 15]
        assert e_stream <= 2 * e_whole, (e_stream, e_whole)
        want = c['search']
        assert torch.equal(hyp_len, want['lengths']) and torch.equal(hyp, want['tokens']) and torch.equal(truncated, want['truncated'])
        assert torch.equal(st.search.result()[2].cpu(), want['frames'])
        # a closed slot keeps its hypothesis: row 4 closes at its finish, two pushes and a finish of the others follow
        closed_at = max(j for j, call in enumerate(c['calls']) if call[0] == 'finish' and call[1][4])
        assert closed_at < len(partials) - 1
        for p in partials[closed_at + 1:]:
            assert all(torch.equal(a[4], b[4]) for a, b in zip(p, partials[closed_at]))


def test_streaming_transducer_general_encoder_side_and_neighbours(monkeypatch):
    """HALO_STREAM_FUSED=0 gives the same tokens; a StreamingRecognizer built next to a StreamingTransducer on the same encoder gives
    what it gives alone, the calls of the two interleaved."""
    from haloop_amd import recognizer, streaming
    from test_gpu_streaming import _stream as stream_ctc
    f, c = SR.FAST, SR.fast_case()
    enc, head = _encoder(c['enc_p']), head_of(c['sd'])
    x = c['x'].to(DEV)
    torch.manual_seed(3)
    ctc = recognizer.TemporalClassifier(f['H'], f['V']).to(DEV).eval()
    alone = streaming.StreamingRecognizer(enc, ctc, f['B'], chunk_frames=f['chunk'], capacity=32)
    ali_a, _, rec_a = stream_ctc(alone, x, f['lengths'], f['chunk'])
    st = streaming.StreamingTransducer(enc, head, f['B'], chunk_frames=f['chunk'], capacity=f['capacity'], max_symbols_per_frame=R.MAX_SYMBOLS)
    beside = streaming.StreamingRecognizer(enc, ctc, f['B'], chunk_frames=f['chunk'], capacity=32)
    st.push(x[:, :16].contiguous(), None, [True] * f['B'])              # a transducer stream is open while the recognizer runs
    ali_b, _, rec_b = stream_ctc(beside, x, f['lengths'], f['chunk'])
    assert ali_a == ali_b
    for (last_a, part_a), (last_b, part_b) in zip(rec_a, rec_b):
        assert all(torch.equal(a, b) for a, b in zip(last_a, last_b)) and all(torch.equal(a, b) for a, b in zip(part_a, part_b))
    _, fused = _run_transducer(st, x)                                    # (begins every slot again)
    monkeypatch.setenv('HALO_STREAM_FUSED', '0')
    general = streaming.StreamingTransducer(enc, head, f['B'], chunk_frames=f['chunk'], capacity=f['capacity'],
                                            max_symbols_per_frame=R.MAX_SYMBOLS)
    assert not general.fused and st.fused
    _, gen = _run_transducer(general, x)
    for a, b in zip(fused, gen):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    with pytest.raises(ValueError):
        st.push(x[:, :16].contiguous())                                  # every slot is closed
