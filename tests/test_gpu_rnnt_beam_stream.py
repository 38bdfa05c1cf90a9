"""GPU tests of the carried transducer beam search (haloop_amd.transducer.BeamStream, csrc/rnnt_beam.hip) and of
``streaming.StreamingTransducer(beam=W)``, in `bf16x3` unless said otherwise.

After the call that marks its rows final the carried search is held to ``BeamDecoder.decode`` of the whole utterance bit for bit,
scores included: the stall rule executes the whole search's steps and no others, on the same launches.  Against the float64
restatement (tests/rnnt_beam_stream_ref.py) after every call: a closed row's finals exactly, an open row's beam as a set of token
sequences -- tests/test_rnnt_beam_cpu.py pins every prune of the compared rows at a gap of 1e-3 or more; the order inside a beam is not
so pinned, so the best hypothesis is compared only where its float64 margin is 1e-3 or more -- and the scores within rtol 1e-5 / atol
1e-4, ``test_gpu_rnnt_beam.check``'s tolerance.  tests/test_rnnt_beam_stream_cpu.py asserts on the CPU what makes the cases meaningful.
"""
import numpy as np
import pytest
import torch

import rnnt_beam_ref as BR
import rnnt_beam_stream_ref as R
import rnnt_stream_ref as SR
import stream_ref
from test_gpu_rnnt_beam import head_of, math_mode, same

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
CASES = [('small', 4), ('small', 1), ('rows17', 4), ('rows17', 8)]
EDGES = [('wide', 3), ('stream', 3), ('tiny', 16)]       # the widths tests/test_gpu_rnnt_beam.py uses


@pytest.fixture(autouse=True)
def bf16x3():
    with math_mode('bf16x3'):
        yield


_cases = {}


def case(name, W):
    """The fixture on the device, its head, f = the call BeamDecoder makes and the whole search's result; computed once, never changed."""
    if (name, W) not in _cases:
        from haloop_amd import functional as HF, transducer
        sd, x, il, cap = BR.inputs(name)
        head = head_of(sd)
        xd = x.to(DEV)
        with torch.no_grad():
            f = HF.linear(xd.float(), head.classifier.weight, head.classifier.bias).contiguous()
        dec = transducer.BeamDecoder(head, x.shape[0], cap, W)
        assert dec.fused
        _cases[name, W] = dict(sd=sd, x=xd, il=il.tolist(), cap=cap, head=head, f=f, N=x.shape[0], T=x.shape[1], W=W, dec=dec,
                               whole=dec.decode(xd, il.to(DEV)))
    return _cases[name, W]


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def new_stream(c, calls):
    from haloop_amd import transducer
    bs = transducer.BeamStream(c['head'], c['N'], c['cap'], c['W'], max_chunk=R.max_chunk(calls))
    assert bs.fused
    return bs


def stream(bs, f, calls, fill=NAN, after_call=None):
    """Feeds f [N, T, V] to ``bs`` by the script ``calls`` -> the cursors."""
    cur = [0] * f.shape[0]
    for j, (counts, begin, final) in enumerate(calls):
        bs.advance(SR.chunk(f, cur, counts, fill), i32(counts), begin, final)
        cur = [a + c for a, c in zip(cur, counts)]
        if after_call:
            after_call(j, cur)
    return cur


# ------------------------------------------------------------------------------------------------- 1. bit equality with the whole search
@pytest.mark.parametrize('kind', R.SCHEDULES)
@pytest.mark.parametrize('name,W', CASES)
def test_the_final_nbest_equals_the_whole_search(name, W, kind):
    c = case(name, W)
    calls = R.script(kind, c['il'], c['T'])
    bs = new_stream(c, calls)
    rounds = []
    stream(bs, c['f'], calls, after_call=lambda j, cur: rounds.append(bs.rounds))
    print(name, W, kind, 'rounds', rounds)
    got = bs.nbest()
    for a, b, what in zip(got, c['whole'], ('tokens', 'lengths', 'scores', 'counts')):
        assert a.dtype == b.dtype and torch.equal(a, b), (name, W, kind, what)


@pytest.mark.parametrize('kind', ['ones', 'fours'])
@pytest.mark.parametrize('name,W', EDGES)
def test_the_final_nbest_equals_the_whole_search_at_the_kernel_s_edges(name, W, kind):
    """V = 1031 (several passes per thread), V = 4099 (W V above the LDS cache: the logits are recomputed in every round) and W = 16
    with nothing pruned."""
    c = case(name, W)
    calls = R.script(kind, c['il'], c['T'])
    bs = new_stream(c, calls)
    stream(bs, c['f'], calls)
    assert same(bs.nbest(), c['whole']), (name, W, kind)


def test_results_do_not_depend_on_when_the_live_word_is_read():
    """The live word read after every round, every 16 rounds and at the default cadence: the same bits after every call, and calls
    that end on either parity of the copies."""
    c = case('rows17', 4)
    calls = R.script('staggered', c['il'], c['T'])
    runs, parities = [], set()
    for every in (1, 16, None):
        bs = new_stream(c, calls)
        if every:
            bs.sync_every = every
        per_call = []

        def after_call(j, cur):
            per_call.append(bs.nbest())
            parities.add((every, bs._cur))
        stream(bs, c['f'], calls, after_call=after_call)
        runs.append(per_call)
    assert {(1, 0), (1, 1)} <= parities
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(same(a, b) for a, b in zip(runs[0], other))
    assert same(runs[0][-1], c['whole'])


# ------------------------------------------------------------------------------------------------------------- 2. float64 reference
def check_call(got, ref, rows, W, what):
    tokens, lengths, scores, counts = (x.cpu() for x in got)
    worst = 0.0
    for n in rows:
        closed, hyps = ref.hypotheses(n)
        mine = [(tuple(tokens[n, w, :lengths[n, w]].tolist()), float(scores[n, w])) for w in range(int(counts[n]))]
        assert bool((lengths[n, int(counts[n]):] == -1).all()) and bool((tokens[n, int(counts[n]):] == -1).all()), (what, n)
        if closed:
            hyps = hyps[:W]
            assert [y for y, _ in mine] == [y for y, _ in hyps], (what, n)
        else:
            assert len(mine) == len(hyps) and {y for y, _ in mine} == {y for y, _ in hyps}, (what, n)
            if len(hyps) > 1 and hyps[0][1] - hyps[1][1] >= BR.GAP:
                assert mine[0][0] == hyps[0][0], (what, n)
        want = dict(hyps)
        for y, s in mine:
            worst = max(worst, abs(s - want[y]))
            np.testing.assert_allclose(s, want[y], rtol=1e-5, atol=1e-4, err_msg=f'{what} row {n}')
    print(what, 'counts', counts.tolist(), 'max |score error|', worst)


@pytest.mark.parametrize('name,W,kind', [('small', 4, 'mixed'), ('small', 1, 'ones'), ('rows17', 4, 'staggered'), ('rows17', 8, 'fours')])
def test_against_the_float64_restatement_after_every_call(name, W, kind):
    c = case(name, W)
    calls = R.script(kind, c['il'], c['T'])
    ref = R.BeamStreamRef(c['sd'], c['N'], c['cap'], W)
    F64 = R.logits(name)
    bs = new_stream(c, calls)
    cur = [0] * c['N']
    for j, (counts, begin, final) in enumerate(calls):
        ref.advance(SR.chunk(F64, cur, counts), counts, begin, final)
        bs.advance(SR.chunk(c['f'], cur, counts, NAN), i32(counts), begin, final)
        cur = [a + n for a, n in zip(cur, counts)]
        check_call(bs.nbest(), ref, BR.compared_rows(name, W), W, f'{name} W={W} {kind} call {j}')


# --------------------------------------------------------------------------------------------------------------- 3. no stray reads
@pytest.mark.parametrize('name,W', [('small', 4), ('rows17', 4)])
def test_nothing_outside_a_row_s_frames_is_read(name, W):
    """NaN against zeros in every frame at or past a row's n_frames, in the rows that take no part, in the rows at or beyond B and in
    frames sent to rows that are closed; the chunk is a strided slice of a wider buffer."""
    c = case(name, W)
    N = c['N']
    calls = R.script('staggered', c['il'], c['T'])
    results = []
    for fill in (0.0, NAN):
        bs = new_stream(c, calls)
        per_call, cur, done = [], [0] * N, [False] * N
        for j, (counts, begin, final) in enumerate(calls):
            ch = SR.chunk(c['f'], cur, counts, fill)
            S, V = ch.shape[1], ch.shape[2]
            sent = [S if done[n] else counts[n] for n in range(N)]       # a closed row is sent S frames of the fill
            B = max([n + 1 for n in range(N) if counts[n] or begin[n] or final[n]] + [1])
            wide = torch.full((N, S + 2, V + 3), fill, device=DEV)
            wide[:B, 1:-1, :V] = ch[:B]
            bs.advance(wide[:B, 1:-1, :V], i32(sent[:B]), begin[:B], final[:B])
            cur = [a + n for a, n in zip(cur, counts)]
            done = [d or f for d, f in zip(done, final)]
            per_call.append(bs.nbest())
        results.append(per_call)
    for a, b in zip(*results):
        assert same(a, b)
    assert same(results[1][-1], c['whole'])


# --------------------------------------------------------------------------------------------------------------- 4. begin and reuse
def test_a_row_begun_again_abandons_its_stream():
    """A long row begins again at call 2 and is sent its utterance from the start while the others go on."""
    from haloop_amd import transducer
    c = case('rows17', 4)
    N, il = c['N'], c['il']
    again = next(n for n in range(N) if il[n] > 12)
    bs = transducer.BeamStream(c['head'], N, c['cap'], 4, max_chunk=4)
    cur, j = [0] * N, 0
    while any(a < l for a, l in zip(cur, il)):
        begin = [j == 0] * N
        if j == 2:
            assert cur[again] == 8 and not bool(bs._meta[3, again]) and int(bs.nbest()[3][again]) > 0       # an open stream
            begin[again], cur[again] = True, 0
        counts = [min(4, l - a) for a, l in zip(cur, il)]
        final = [a + n == l and (n > 0 or begin[k]) for k, (a, l, n) in enumerate(zip(cur, il, counts))]
        bs.advance(SR.chunk(c['f'], cur, counts, NAN), i32(counts), begin, final)
        cur = [a + n for a, n in zip(cur, counts)]
        j += 1
    assert same(bs.nbest(), c['whole'])


def test_rows_reused_after_an_unrelated_utterance_repeat_bit_for_bit():
    c = case('rows17', 4)
    calls = R.script('fours', c['il'], c['T'])
    from haloop_amd import transducer
    bs = transducer.BeamStream(c['head'], c['N'], c['cap'], 4, max_chunk=5)
    first, again = [], []
    stream(bs, c['f'], calls, after_call=lambda j, cur: first.append(bs.nbest()))
    other = 3 * torch.randn(c['N'], 7, c['f'].shape[2], generator=torch.Generator().manual_seed(5)).to(DEV)
    bs.advance(other[:, :5], None, [True] * c['N'])                      # n_frames None: all 5; the streams are left open
    bs.advance(other[:, 5:], i32([2] * c['N']))
    bs.advance(other[:, :3], None)
    stream(bs, c['f'], calls, after_call=lambda j, cur: again.append(bs.nbest()))
    assert len(first) == len(again) and all(same(a, b) for a, b in zip(first, again))
    assert same(again[-1], c['whole'])


def test_begin_without_frames_leaves_the_empty_hypothesis():
    c = case('small', 4)
    calls = R.script('fours', c['il'], c['T'])
    bs = new_stream(c, calls)
    stream(bs, c['f'], calls)
    N = c['N']
    bs.advance(torch.full_like(c['f'][:, :2], NAN), i32([0] * N), [True] * N)
    tokens, lengths, scores, counts = bs.nbest()
    assert counts.tolist() == [1] * N and lengths[:, 0].tolist() == [0] * N and scores[:, 0].tolist() == [0.0] * N
    assert bool((tokens == -1).all()) and bool((lengths[:, 1:] == -1).all()) and bool(torch.isinf(scores[:, 1:]).all())
    stream(bs, c['f'], [(counts_, [False] * N, final) for counts_, _, final in calls])     # they go on without another begin
    assert same(bs.nbest(), c['whole'])


def test_begin_and_final_without_frames_is_the_utterance_of_no_frames():
    c = case('small', 4)
    N = c['N']
    bs = new_stream(c, [([4] * N, None, None)])
    bs.advance(torch.full_like(c['f'][:, :2], NAN), i32([0] * N), [True] * N, [True] * N)
    want = c['dec'].decode(c['x'], i32([0] * N))
    assert want[3].tolist() == [1] * N and want[2][:, 0].tolist() == [0.0] * N
    assert same(bs.nbest(), want)
    bs.advance(c['f'][:, :4], None)                                      # closed rows: the frames change nothing
    assert same(bs.nbest(), want)
    # begun without frames, then final in a later call that brings none either
    bs.advance(c['f'][:, :1], i32([0] * N), [True] * N)
    bs.advance(c['f'][:, :1], i32([0] * N), None, [True] * N)
    assert same(bs.nbest(), want)


# ------------------------------------------------------------------------------------------------------- 5. paths and stale images
def test_fused_path_equals_general_path():
    c = case('rows17', 4)
    calls = R.script('staggered', c['il'], c['T'])
    fused = new_stream(c, calls)
    mid = []
    stream(fused, c['f'], calls, after_call=lambda j, cur: mid.append(fused.nbest()))
    from haloop_amd import transducer
    with math_mode('f32'):
        general = transducer.BeamStream(c['head'], c['N'], c['cap'], 4, max_chunk=R.max_chunk(calls))
        assert not general.fused
        gmid = []
        stream(general, c['f'], calls, after_call=lambda j, cur: gmid.append(general.nbest()))
    rows = BR.compared_rows('rows17', 4)
    for j in (3, len(calls) - 1):                  # open beams in the middle (sets: the order inside a beam is not pinned), finals at the end
        a, b = [x.cpu() for x in mid[j]], [x.cpu() for x in gmid[j]]
        assert torch.equal(a[3][rows], b[3][rows])
        for n in rows:
            ya = {tuple(a[0][n, w, :a[1][n, w]].tolist()): float(a[2][n, w]) for w in range(int(a[3][n]))}
            yb = {tuple(b[0][n, w, :b[1][n, w]].tolist()): float(b[2][n, w]) for w in range(int(b[3][n]))}
            assert set(ya) == set(yb), (j, n)
            for y in ya:
                np.testing.assert_allclose(ya[y], yb[y], rtol=1e-5, atol=1e-4)
    a, b = mid[-1], gmid[-1]
    assert torch.equal(a[0][rows], b[0][rows]) and torch.equal(a[1][rows], b[1][rows]) and torch.equal(a[3][rows], b[3][rows])
    np.testing.assert_allclose(a[2][rows].cpu().numpy(), b[2][rows].cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_a_changed_weight_reaches_the_next_stream():
    from haloop_amd import functional as HF, transducer
    sd, x, il, cap, ref = BR.fixture('rows17', 4)
    head = head_of(sd)                                                   # (a head of this test's own: its weights change)
    calls = R.script('fours', il.tolist(), x.shape[1])
    bs = transducer.BeamStream(head, 17, cap, 4, max_chunk=4)
    dec = transducer.BeamDecoder(head, 17, cap, 4)
    xd, ild = x.to(DEV), il.to(DEV)

    def f_of():
        with torch.no_grad():
            return HF.linear(xd, head.classifier.weight, head.classifier.bias).contiguous()
    stream(bs, f_of(), calls)
    first = dec.decode(xd, ild)
    assert same(bs.nbest(), first)
    with torch.no_grad():
        head.lm.rnn.weight_hh_l0.mul_(0.5)
    second = dec.decode(xd, ild)
    assert not torch.equal(first[0], second[0])
    stream(bs, f_of(), calls)
    assert same(bs.nbest(), second)


# ----------------------------------------------------------------------------------------------------------- 6. StreamingTransducer
def _encoder(enc_p):
    from haloop_amd import rnn
    f = SR.FAST
    enc = rnn.Encoder(f['F_'], f['C'], f['H'], num_layers=f['L'])
    enc.load_state_dict(enc_p)
    return enc.to(DEV).eval()


def test_streaming_transducer_with_a_beam(monkeypatch):
    """LC-2x1024 under a Transducer(1024, 32), 5 streams in chunks of 16, row 4 ends after 57 frames, beam 4: a twin BeamStream fed
    ``last``'s logits stays bit-equal after every call; after ``finish`` every row's n-best list is a BeamStream's that is fed the
    row's concatenated logits in one final call; ``partial()`` is the best hypothesis; beam=0 is the greedy object."""
    from haloop_amd import streaming, transducer
    f, c = SR.FAST, SR.fast_case()
    B, chunk, lengths = f['B'], f['chunk'], f['lengths']
    enc, head = _encoder(c['enc_p']), head_of(c['sd'])
    x = c['x'].to(DEV)
    st = streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=f['capacity'], beam=4)
    assert isinstance(st.search, transducer.BeamStream) and st.search.fused
    twin = transducer.BeamStream(head, B, f['capacity'], 4, max_chunk=chunk // 4 + 1)
    logits = [[] for _ in range(B)]
    for call in stream_ref.schedule(lengths, chunk):
        if call[0] == 'push':
            _, k, active = call
            begin, final = [a and k == 0 for a in active], None
            st.push(x[:, k * chunk:(k + 1) * chunk].contiguous(), active, begin)
        else:
            _, rows, tails = call
            begin, final = None, [bool(r) for r in rows]
            st.finish(stream_ref.tail_tensor(x, lengths, chunk, rows, tails), tails, rows)
        lg, n = st.last
        for b, k in enumerate(n.tolist()):
            logits[b].append(lg[b, :k].clone())
        twin.advance(lg.clone(), n.clone(), begin, final)
        assert same(st.nbest(), twin.nbest())
    tokens, lengths_, scores, counts = st.nbest()
    assert bool((st.search._meta[3] != 0).all()) and int(counts.min()) >= 1
    for b in range(B):
        row = torch.cat(logits[b])
        one = transducer.BeamStream(head, 1, f['capacity'], 4, max_chunk=row.shape[0])
        one.advance(row[None].contiguous(), None, [True], [True])
        assert all(torch.equal(p[b], q[0]) for p, q in zip((tokens, lengths_, scores, counts), one.nbest())), b
    hyp, hyp_len, best, steps, truncated = st.partial()
    assert torch.equal(hyp, tokens[:, 0]) and torch.equal(hyp_len, lengths_[:, 0]) and torch.equal(best, scores[:, 0])
    assert steps.tolist() == [21, 21, 21, 21, 15] and not bool(truncated.any())
    greedy = streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=f['capacity'], beam=0)
    assert type(greedy.search) is transducer.GreedyStream and greedy.beam == 0
    with pytest.raises(ValueError):
        greedy.nbest()
    assert type(streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=f['capacity']).search) is transducer.GreedyStream
    monkeypatch.setenv('HALO_STREAM_RNNT_BEAM', '2')
    env = streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=f['capacity'])
    assert isinstance(env.search, transducer.BeamStream) and env.search.beam == 2


# ---------------------------------------------------------------------------------------------------------------- 7. the interface
def test_interface_errors():
    from haloop_amd import _lib, transducer
    c = case('small', 4)
    bs = transducer.BeamStream(c['head'], c['N'], c['cap'], 4, max_chunk=4)
    f = c['f'][:, :4]
    with pytest.raises(ValueError):
        bs.advance(f[:, :, :-1])
    with pytest.raises(ValueError):
        bs.advance(c['f'][:, :5])                                        # more frames than max_chunk
    with pytest.raises(ValueError):
        bs.advance(f, torch.zeros(c['N'], dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        bs.advance(f, None, torch.zeros(c['N'], dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        bs.advance(f, None, None, torch.zeros(c['N'], dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        bs.advance(f, None, [True])
    with pytest.raises(ValueError):
        bs.advance(f, None, None, [True])
    with pytest.raises(_lib.HaloError):
        bs.advance(f.cpu())
    with pytest.raises(ValueError):
        transducer.BeamStream(c['head'], 0, 4)
    with pytest.raises(ValueError):
        transducer.BeamStream(c['head'], 2, 4, beam=17)
    c['head'].train()
    try:
        with pytest.raises(NotImplementedError):
            bs.advance(f)
    finally:
        c['head'].eval()
