"""GPU tests of the carried CTC prefix beam search (haloop_amd.ctc.PrefixBeamStream, streaming.StreamingRecognizer(beam=W),
halo_ctc_prefix_beam_advance in csrc/ctc_prefix_beam.hip).

The yardstick is the whole-utterance search on the same device: both entry points instantiate one frame body, so the n-best list after
any split of a row's frames into calls must be ``torch.equal`` to ``ctc.ctc_prefix_beam_search`` of their concatenation, on every row
(no gap condition: the arithmetic is identical).  Two chunked runs are also held against the float64 restatement under the rule of
tests/test_gpu_ctc_prefix_beam.py.  The schedules are those of tests/stream_beam_ref.py, which tests/test_stream_beam_cpu.py pins on
the CPU.
"""
import pytest
import torch

import ctc_prefix_beam_ref as R
import stream_beam_ref as SB
import stream_ref
from conftest import load_golden
from test_gpu_ctc_prefix_beam import check, same
from test_gpu_streaming import FAST, _modules, _params, hal, math_mode  # noqa: F401  (hal and math_mode are fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAIRS = [(name, W, spec) for (name, W) in R.CASES for spec in SB.SCHEDULES[(name, W)]]
IDS = [f'{n}-{w}-{s}' for n, w, s in PAIRS]


def whole(e, il, W, capacity):
    from haloop_amd import ctc
    return ctc.ctc_prefix_beam_search(e, il, W, capacity)


def new_stream(name, W, capacity=None):
    from haloop_amd import ctc
    f = R.FIXTURES[name]
    return ctc.PrefixBeamStream(f['N'], f['V'], W, f['capacity'] if capacity is None else capacity, device=DEV)


def feed(stream, ed, ild, spec, before_call=None):
    """The fixture's frames through ``stream`` under ``spec``: row n gets clamp(L_n - offset, 0, chunk) frames, begin on the first call."""
    T, N, _ = ed.shape
    for i, (off, size) in enumerate(SB.calls(T, spec)):
        nf = (ild - off).clamp(0, size)
        chunk = ed[off:off + size]
        if before_call is not None:
            chunk = before_call(i, chunk, nf)
        out = stream.advance(chunk, nf, torch.ones(N, dtype=torch.bool, device=DEV) if i == 0 else None)
    return out


def chunked(name, W, spec):
    e, il, _ = R.inputs(name)
    stream = new_stream(name, W)
    feed(stream, e.to(DEV), il.to(DEV), spec)
    return stream


# ------------------------------------------------------------------------------------------------ 1. chunked equals whole, bit for bit
@pytest.mark.parametrize('name,W,spec', PAIRS, ids=IDS)
def test_chunked_equals_whole_bit_for_bit(name, W, spec):
    e, il, capacity = R.inputs(name)
    ed, ild = e.to(DEV), il.to(DEV)
    stream = new_stream(name, W)
    views = feed(stream, ed, ild, spec)
    want = whole(ed, ild, W, capacity)
    got = stream.nbest()
    assert same(got, want), f'{name} W={W} chunks {spec}'
    assert same(views, want) and all(v.data_ptr() != g.data_ptr() for v, g in zip(views, got))      # views of the buffers, copies


# ----------------------------------------------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize('name,W', [('rows17', 4), ('long', 4)])
def test_chunked_against_float64(name, W):
    ref = R.fixture(name, W)[3]
    (spec,) = SB.SCHEDULES[(name, W)]
    check(chunked(name, W, spec).nbest(), ref, R.compared_rows(name, W), f'{name} W={W} chunks {spec}')


# ------------------------------------------------------------------------------------------------------ 3. untouched rows and padding
@pytest.mark.parametrize('name,W,spec', [('small', 4, 2), ('rows17', 4, 5)])
def test_rows_without_frames_are_bit_identical_and_padding_is_never_read(name, W, spec):
    e, il, capacity = R.inputs(name)
    ed, ild = e.to(DEV), il.to(DEV)
    T, N, V = e.shape
    clean = chunked(name, W, spec).nbest()
    stream = new_stream(name, W)
    seen = []

    def poison(i, chunk, nf):
        """Frames at or past a row's n_frames, and the gaps of a strided view around the chunk, hold NaN.  Before the call: the rows
        that will get no frames (and do not begin) are remembered, to be compared after it."""
        if seen:
            idle, state, outs = seen.pop()
            assert torch.equal(stream.state[idle], state) and all(torch.equal(a[idle], b) for a, b in zip(stream.nbest(), outs))
        size = chunk.shape[0]
        big = torch.full((N + 1, size + 2, V + 3), float('nan'), device=DEV)
        big[:N, :size, :V] = chunk.permute(1, 0, 2)
        view = big[:N, :size, :V].permute(1, 0, 2)
        assert view.stride(2) == 1 and not view.is_contiguous()
        view.masked_fill_((torch.arange(size, device=DEV)[:, None] >= nf[None, :])[:, :, None], float('nan'))
        idle = torch.nonzero(nf == 0)[:, 0] if i > 0 else nf.new_zeros(0)
        seen.append((idle, stream.state[idle].clone(), [t[idle] for t in stream.nbest()]))
        poison.idle_rows += idle.numel()
        return view

    poison.idle_rows = 0
    feed(stream, ed, ild, spec, poison)
    idle, state, outs = seen.pop()
    assert torch.equal(stream.state[idle], state) and all(torch.equal(a[idle], b) for a, b in zip(stream.nbest(), outs))
    assert poison.idle_rows >= 2                                        # (the schedule does leave rows without frames)
    assert same(stream.nbest(), clean)
    assert same(clean, whole(ed, ild, W, capacity))


# ---------------------------------------------------------------------------------------------------------------------- 4. reuse
def test_rows_are_reused_and_calls_repeat_bit_for_bit():
    e, il, capacity = R.inputs('rows17')
    ed, ild = e.to(DEV), il.to(DEV)
    stream = new_stream('rows17', 8)
    feed(stream, ed, ild, 5)
    first = stream.nbest()
    other = torch.randn(9, 17, 8, generator=torch.Generator().manual_seed(11)).log_softmax(-1).to(DEV)
    feed(stream, other, torch.full((17,), 9, device=DEV), 4)            # an unrelated utterance in the same rows, of other lengths
    assert not same(stream.nbest(), first)
    feed(stream, ed, ild, 5)
    assert same(stream.nbest(), first)
    again = new_stream('rows17', 8)
    feed(again, ed, ild, 5)
    assert same(again.nbest(), first) and torch.equal(again.state[:, :512], stream.state[:, :512])      # the records, bit for bit
    assert same(first, whole(ed, ild, 8, capacity))


# ------------------------------------------------------------------------------------------------------------------- 5. capacity
def test_capacity_is_independent_of_the_chunk():
    e, il, capacity = R.inputs('rows17cap')                             # capacity 3, one frame per call
    ed, ild = e.to(DEV), il.to(DEV)
    stream = new_stream('rows17cap', 4)
    feed(stream, ed, ild, 1)
    want = whole(ed, ild, 4, capacity)
    assert capacity == 3 and same(stream.nbest(), want)
    assert bool((want[1] == capacity).any())                            # (hypotheses did reach the capacity)
    # a capacity above every call's T and above the whole utterance's: the columns past T hold -1, the rest is the whole search's
    e, il, capacity = R.inputs('small')
    ed, ild = e.to(DEV), il.to(DEV)
    stream = new_stream('small', 4, capacity=100)
    feed(stream, ed, ild, 2)
    tokens, lengths, scores, counts = stream.nbest()
    want = whole(ed, ild, 4, capacity)
    assert tokens.shape == (3, 4, 100) and torch.equal(tokens[:, :, :capacity], want[0]) and bool((tokens[:, :, capacity:] == -1).all())
    assert same((lengths, scores, counts), want[1:])


# ---------------------------------------------------------------------------------------------------- 6. StreamingRecognizer(beam=W)
@pytest.fixture(scope='module')
def fast_params():
    """Parameters and inputs of test_gpu_streaming.py's fast-path case (without its float64 oracle): computed once, never changed."""
    from oracle import cpu_ref
    c = FAST
    enc_p, rec_p = cpu_ref.make_params(c['F_'], c['C'], c['H'], c['L'], c['V'], seed=42)
    rec_p['classifier.weight'] = rec_p['classifier.weight'] * 100
    x = 8 * torch.randn(c['B'], c['T'], c['F_'], generator=torch.Generator().manual_seed(43))
    return enc_p, rec_p, x


def drive(sr, x, lengths, chunk, verify=True):
    """Stream x[b, :lengths[b]] through slot b by stream_ref.schedule.  After every call, ``nbest()`` of every slot must equal the whole
    search of the slot's streamed log-probs so far (collected through want_log_probs), and ``partial()`` must describe its best
    hypothesis.  The whole search takes capacity <= T, and no hypothesis of T frames is longer than T, so it runs at min(capacity, T):
    below the stream's capacity nothing can have been refused, and the stream's further columns must hold -1.
    -> [(nbest, partial)] on the CPU, one per call."""
    from haloop_amd import ctc
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
        tokens, lengths_, scores, counts = nbest = sr.nbest()
        hyp, hyp_len, best, steps, truncated = part = sr.partial()
        record.append(([t.cpu() for t in nbest], [t.cpu() for t in part]))
        if not verify:
            continue
        assert tokens.shape == (B, W, capacity)
        for b in range(B):
            e = torch.cat(lp[b])[:, None, :]
            T = e.shape[0]
            assert T == steps[b].item() > 0
            cap = min(capacity, T)
            want = ctc.ctc_prefix_beam_search(e, None, W, cap)
            assert torch.equal(tokens[b:b + 1, :, :cap], want[0]) and bool((tokens[b, :, cap:] == -1).all()), (b, T)
            assert torch.equal(lengths_[b:b + 1], want[1]) and torch.equal(scores[b:b + 1], want[2]) and torch.equal(counts[b:b + 1], want[3])
        assert torch.equal(hyp_len, lengths_[:, 0]) and torch.equal(best, scores[:, 0])
        assert torch.equal(hyp, tokens[:, 0].clamp(min=0))              # (-1 past the length -> 0)
        assert torch.equal(truncated, (lengths_ >= capacity).any(1))
    return record


def records_equal(a, b, only=None):
    assert len(a) == len(b)
    for (nbest_a, part_a), (nbest_b, part_b) in zip(a, b):
        if only is None:
            assert same(nbest_a, nbest_b) and same(part_a, part_b)
        else:
            assert all(torch.equal(nbest_a[i], nbest_b[i]) for i in only)


@pytest.mark.parametrize('math_mode', ['bf16x3', 'f32', 'bf16'], indirect=True)
def test_recognizer_nbest_equals_the_whole_search_after_every_call(hal, fast_params, math_mode):
    """5 streams, chunks of 16, row 4 closing after 57 frames while the others go on (its beam stays readable and unchanged); capacity
    8 is below the 21 steps of a stream, so extensions are refused at it across calls."""
    enc_p, rec_p, x = fast_params
    c = FAST
    enc, rec = _modules(hal, enc_p, rec_p)
    sr = hal['streaming'].StreamingRecognizer(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=8, beam=4)
    record = drive(sr, x.to(DEV), c['lengths'], c['chunk'])
    print(math_mode, 'best lengths', record[-1][0][1][:, 0].tolist(), 'truncated', record[-1][1][4].tolist())
    closed = [r[0] for r in record[-2:]]                                # row 4 closed before the last two calls
    assert all(torch.equal(a[4], b[4]) for a, b in zip(*closed))


def test_recognizer_replay_reuse_and_general_path(hal, fast_params, monkeypatch):
    enc_p, rec_p, x = fast_params
    c = FAST
    enc, rec = _modules(hal, enc_p, rec_p)
    xd = x.to(DEV)
    S = hal['streaming'].StreamingRecognizer
    eager = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32, use_graph=False, beam=4)
    rec_e = drive(eager, xd, c['lengths'], c['chunk'])
    graph = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32, use_graph=True, beam=4)
    rec_g = drive(graph, xd, c['lengths'], c['chunk'], verify=False)
    assert graph._graphs
    records_equal(rec_e, rec_g)
    other = 3 * torch.randn(c['B'], 48, c['F_'], generator=torch.Generator().manual_seed(5)).to(DEV)
    for sr in (eager, graph):
        drive(sr, other, [48, 32, 48, 16, 48], c['chunk'], verify=False)         # an unrelated utterance in every slot
        records_equal(rec_e, drive(sr, xd, c['lengths'], c['chunk'], verify=False))
    monkeypatch.setenv('HALO_STREAM_FUSED', '0')
    general = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32, beam=4)
    assert not general.fused and eager.fused
    records_equal(rec_e, drive(general, xd, c['lengths'], c['chunk']), only=(0, 1))                 # tokens and lengths


@pytest.mark.parametrize('W', [4, 1])
def test_recognizer_on_the_tiny_golden(hal, W):
    """H = 32: the general head (the log-probs come from gemm + log_softmax) and the step-launch LSTM; chunks of 8, capacity 16."""
    g = load_golden('g1_tiny_l2')
    enc, rec = _modules(hal, _params(g, 'encoder.'), _params(g, 'recognizer.'))
    x = torch.from_numpy(g['x']).to(DEV)
    assert x.shape[0] == 3
    sr = hal['streaming'].StreamingRecognizer(enc, rec, 3, chunk_frames=8, capacity=16, beam=W)
    drive(sr, x, [41, 23, 9], 8)
    assert sr.partial()[3].tolist() == [11, 7, 3]


def test_beam_zero_is_the_greedy_object(hal, monkeypatch):
    from oracle import cpu_ref
    ops = hal['ops']
    enc_p, rec_p = cpu_ref.make_params(12, 16, 32, 2, 9, seed=3)
    enc, rec = _modules(hal, enc_p, rec_p)
    S = hal['streaming'].StreamingRecognizer
    launches = []
    real = ops.ctc_prefix_beam_advance
    monkeypatch.setattr(ops, 'ctc_prefix_beam_advance', lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    fr = torch.randn(2, 8, 12, generator=torch.Generator().manual_seed(1)).to(DEV)
    monkeypatch.delenv('HALO_STREAM_BEAM', raising=False)
    outs = []
    for kwargs in (dict(), dict(beam=0)):
        sr = S(enc, rec, 2, chunk_frames=8, capacity=4, **kwargs)
        assert sr.beam == 0 and sr._beam is None
        sr.push(fr, begin=[True, True])
        sr.finish()
        outs.append(sr.partial())
        with pytest.raises(ValueError):
            sr.nbest()
    assert not launches and same(outs[0], outs[1])
    monkeypatch.setenv('HALO_STREAM_BEAM', '4')
    sr = S(enc, rec, 2, chunk_frames=8, capacity=4)
    assert sr.beam == 4 and sr.nbest()[3].tolist() == [0, 0]            # never begun: no hypothesis
    sr.push(fr, begin=[True, True])
    sr.finish()
    assert len(launches) == 2 and sr.nbest()[0].shape == (2, 4, 4)
    assert torch.equal(sr._hyp, outs[0][0]) and torch.equal(sr._hyp_len, outs[0][1])      # the greedy state is as without a beam
    monkeypatch.setenv('HALO_STREAM_BEAM', '17')
    with pytest.raises(ValueError):
        S(enc, rec, 2, chunk_frames=8, capacity=4)


# ------------------------------------------------------------------------------------------------------------ 7. interface errors
def test_interface_errors(hal):
    from oracle import cpu_ref
    from haloop_amd import ctc
    enc_p, rec_p = cpu_ref.make_params(12, 16, 32, 2, 9, seed=3)
    enc, rec = _modules(hal, enc_p, rec_p)
    S = hal['streaming'].StreamingRecognizer
    for beam in (-1, 17):
        with pytest.raises(ValueError):
            S(enc, rec, 2, chunk_frames=8, beam=beam)
    with pytest.raises(ValueError):
        S(enc, rec, 2, chunk_frames=8, capacity=8193, beam=4)
    for kwargs in (dict(beam=0), dict(beam=17), dict(capacity=0), dict(capacity=8193)):
        with pytest.raises(ValueError):
            ctc.PrefixBeamStream(3, 5, device=DEV, **kwargs)
    stream = ctc.PrefixBeamStream(3, 5, beam=2, capacity=4, device=DEV)
    e = torch.randn(2, 3, 5).log_softmax(-1).to(DEV)
    i64 = lambda v: torch.tensor(v, device=DEV)
    for bad in (e[0], e[:, :2], e[:, :, :4], e[:0]):
        with pytest.raises(ValueError):
            stream.advance(bad)
    for kwargs in (dict(n_frames=i64([2, 2])), dict(n_frames=i64([2.0, 2.0, 2.0])), dict(begin=i64([1, 1, 1])),
                   dict(begin=torch.ones(2, dtype=torch.bool, device=DEV)), dict(n_frames=[2, 2, 2])):
        with pytest.raises(ValueError):
            stream.advance(e, **kwargs)
    with pytest.raises(hal['lib'].HaloError):
        stream.advance(e.cpu())
    with pytest.raises(hal['lib'].HaloError):
        stream.advance(e, n_frames=torch.tensor([2, 2, 2]))
    assert stream.nbest()[3].tolist() == [0, 0, 0]                      # nothing ran
    stream.advance(e, i64([2, 1, 0]).to(torch.int32), torch.tensor([1, 1, 0], dtype=torch.int32, device=DEV))
    assert stream.nbest()[3].tolist()[2] == 0 and stream.nbest()[3].tolist()[0] >= 1
