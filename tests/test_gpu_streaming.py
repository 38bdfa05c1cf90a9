"""Streaming LSTM-CTC recognition (haloop_amd/streaming.py, csrc/stream.hip) on the device: the two kernels alone against float64 and a
Python collapse, whole streams against the reference's goldens, against ``infer.LstmCtcRecognizer`` and against the float64 oracle.

Measured on an MI355X (test_streams_at_the_fast_path_shape; the bound is e_stream <= 2 * e_whole):
    bf16x3  e_stream 5.07e-5   e_whole 3.69e-5
    f32     e_stream 3.20e-6   e_whole 3.89e-6
    bf16    e_stream 2.083e-2  e_whole 2.082e-2
"""
import numpy as np
import pytest
import torch

import stream_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24


@pytest.fixture(scope='module')
def hal():
    import haloop_amd
    from haloop_amd import _lib, infer, ops, recognizer, rnn, streaming
    _lib.lib()
    _lib.lend_scratch()
    return dict(ops=ops, rnn=rnn, recognizer=recognizer, streaming=streaming, infer=infer, lib=_lib)


@pytest.fixture
def math_mode(request, hal):
    prev = hal['lib'].get_math_mode()
    hal['lib'].set_math_mode(request.param)
    yield request.param
    hal['lib'].set_math_mode(prev)


def _modules(hal, enc_p, rec_p):
    F_, C = enc_p['subsample.weight'].shape[1], enc_p['subsample.weight'].shape[0]
    H, V = rec_p['classifier.weight'].shape[1], rec_p['classifier.weight'].shape[0]
    L = sum(1 for k in enc_p if k.startswith('lstm.weight_hh_l'))
    enc, rec = hal['rnn'].Encoder(F_, C, H, num_layers=L), hal['recognizer'].TemporalClassifier(H, V)
    enc.load_state_dict(enc_p); rec.load_state_dict(rec_p)
    return enc.to(DEV).eval(), rec.to(DEV).eval()


def _params(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}


def _stream(sr, x, lengths, chunk, want_lp=False):
    """Stream x[b, :lengths[b]] (x on the device) through slot b by stream_ref.schedule -> per row (alignments, log-probs or None) and
    a copy of every call's ``last`` and ``partial()``."""
    B = x.shape[0]
    ali, lp, record = [[] for _ in range(B)], [[] for _ in range(B)], []
    for call in stream_ref.schedule(lengths, chunk):
        if call[0] == 'push':
            _, k, active = call
            sr.push(x[:, k * chunk:(k + 1) * chunk].contiguous(), active, [a and k == 0 for a in active], want_log_probs=want_lp)
            rows = active
        else:
            _, rows, tails = call
            sr.finish(stream_ref.tail_tensor(x, lengths, chunk, rows, tails), tails, rows, want_log_probs=want_lp)
        last = [t.cpu().clone() for t in sr.last]
        record.append((last, [t.cpu() for t in sr.partial()]))
        n = last[2].tolist()
        for b in range(B):
            assert (n[b] > 0) == bool(rows[b])
            ali[b] += last[0][b, :n[b]].tolist()
            assert not last[0][b, n[b]:].any() and not last[1][b, n[b]:].any()
            if want_lp:
                lp[b].append(last[3][b, :n[b]])
    return ali, [torch.cat(r) if r else None for r in lp], record


def _hyps(sr):
    hyp, hlen, score, steps, trunc = (t.cpu() for t in sr.partial())
    return [hyp[b, :hlen[b]].tolist() for b in range(hyp.shape[0])], score, steps, trunc


# ------------------------------------------------------------------------------------------------------------- 1. the front kernel
def test_front_kernel_alone(hal):
    """B = 3, F = 12, C = 16, chunks of 8: three pushes, a finish with tails 0 / 1 / 7 (1 / 1 / 3 steps), row 2 inactive in the first
    push, row 0 begun again afterwards.  fp32 bound per output, derived: the kernel sums K = 5 F products in sequence, each rounded
    once (fma), so |error| <= K u sum|w||x| to first order; 4 K u sum|w||x| + u |bias| leaves room for the bias add and second order."""
    ops = hal['ops']
    B, F_, C, Tc, L, H = 3, 12, 16, 8, 2, 8
    g = torch.Generator().manual_seed(7)
    w, bias = torch.randn(C, F_, 5, generator=g) / 4, torch.randn(C, generator=g)
    sig = [torch.randn(24, F_, generator=g), torch.randn(25, F_, generator=g), torch.randn(23, F_, generator=g), torch.randn(8, F_, generator=g)]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    carry = torch.full((B, 3, F_), 5.0, device=DEV)           # junk: a beginning stream must not read it
    h, c = torch.ones(L, B, H, device=DEV), torch.ones(L, B, H, device=DEV)
    hyp_len, steps = torch.full((B,), 9, dtype=torch.int64, device=DEV), torch.full((B,), 9, dtype=torch.int64, device=DEV)
    score, last_label = torch.ones(B, device=DEV), torch.full((B,), 3, dtype=torch.int32, device=DEV)
    hyp = torch.full((B, 5), 7, dtype=torch.int64, device=DEV)
    trunc, n_steps = torch.ones(B, dtype=torch.bool, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    wd, bd = w.to(DEV), bias.to(DEV)
    A, BG, FN = ops.STREAM_ACTIVE, ops.STREAM_BEGIN, ops.STREAM_FINAL
    out = [[], [], [], []]

    def call(frames, lengths, flags, S, dest):
        y = torch.full((S, B, C), -1.0, device=DEV)
        before = carry.clone()
        ops.stream_front(frames.to(DEV), carry, i32(lengths), i32(flags), wd, bd, y, n_steps, h, c, hyp, hyp_len, steps, score, last_label,
                         trunc)
        n = n_steps.tolist()
        for b in range(B):
            assert torch.equal(y[n[b]:, b], torch.zeros(S - n[b], C, device=DEV))          # exactly zero past n_steps
            if not flags[b] & A:
                assert n[b] == 0 and torch.equal(carry[b], before[b])                      # an inactive row: bit-identical carry
            if flags[b] & FN:
                assert torch.equal(carry[b], before[b])
            if dest[b] is not None:
                out[dest[b]].append(y[:n[b], b].cpu())
        return n

    def chunk(offsets):
        fr = torch.zeros(B, Tc, F_)
        for b, (s, o) in enumerate(offsets):
            if s is not None:
                fr[b] = sig[s][o:o + Tc]
        return fr

    assert call(chunk([(0, 0), (1, 0), (None, 0)]), [8, 8, 0], [A | BG, A | BG, 0], 2, [0, 1, None]) == [2, 2, 0]
    assert h[:, :2].abs().max() == 0 and c[:, :2].abs().max() == 0 and torch.equal(h[:, 2], torch.ones(L, H, device=DEV))
    assert hyp_len.tolist() == [0, 0, 9] and steps.tolist() == [0, 0, 9] and last_label.tolist() == [-1, -1, 3]
    assert score.tolist() == [0.0, 0.0, 1.0] and trunc.tolist() == [False, False, True]
    assert hyp.tolist() == [[0] * 5, [0] * 5, [7] * 5]
    h.fill_(1.0)
    assert call(chunk([(0, 8), (1, 8), (2, 0)]), [8, 8, 8], [A, A, A | BG], 2, [0, 1, 2]) == [2, 2, 2]
    assert torch.equal(h[:, :2], torch.ones(L, 2, H, device=DEV)) and h[:, 2].abs().max() == 0
    assert call(chunk([(0, 16), (1, 16), (2, 8)]), [8, 8, 8], [A, A, A], 2, [0, 1, 2]) == [2, 2, 2]
    tail = torch.zeros(B, 7, F_)
    tail[1, :1], tail[2, :7] = sig[1][24:25], sig[2][16:23]
    tail[0] = 3.0                                               # beyond the row's length: must read as zeros
    assert call(tail, [0, 1, 7], [A | FN] * 3, 3, [0, 1, 2]) == [1, 1, 3]
    assert call(chunk([(3, 0), (None, 0), (None, 0)]), [8, 0, 0], [A | BG, 0, 0], 2, [3, None, None]) == [2, 0, 0]      # the slot again
    assert call(torch.zeros(B, 7, F_), [0, 0, 0], [A | FN, 0, 0], 3, [3, None, None]) == [1, 0, 0]
    for s, parts in zip(sig, out):
        got = torch.cat(parts).double()
        x64, w64 = s.double().t()[None], w.double()
        want = torch.nn.functional.conv1d(x64, w64, bias.double(), stride=4, padding=3)[0].t().relu()
        mag = torch.nn.functional.conv1d(x64.abs(), w64.abs(), None, stride=4, padding=3)[0].t()
        assert got.shape == want.shape == ((s.shape[0] + 1) // 4 + 1, C)
        bound = 4 * 5 * F_ * U * mag + U * bias.double().abs()[None, :]
        assert ((got - want).abs() <= bound).all(), ((got - want).abs() / bound).max().item()


# --------------------------------------------------------------------------------------------------------- 2. the collapse alone
@pytest.mark.parametrize('capacity', [8, 2])
@pytest.mark.parametrize('V', [9, 40])
def test_collapse_only_mode(hal, V, capacity):
    """Planted log-probs, two steps per call: labels [1,1 | 1,0 | 0,2 | 2,2 | 0,0 | 2,3] -> tokens 1, 2, 2, 3 (a repeat merged across a
    boundary, a blank at a boundary between two equal labels, a label emitted again after blanks).  Row 1 never takes part."""
    ops = hal['ops']
    B, S, L, H = 2, 2, 2, 8
    labels = [[1, 1], [1, 0], [0, 2], [2, 2], [0, 0], [2, 3]]
    g = torch.Generator().manual_seed(V)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    h, c = torch.randn(L, B, H, generator=g).to(DEV), torch.randn(L, B, H, generator=g).to(DEV)
    hyp = torch.full((B, capacity), 7, dtype=torch.int64, device=DEV)
    hyp_len, steps = torch.tensor([0, 1], dtype=torch.int64, device=DEV), torch.tensor([0, 5], dtype=torch.int64, device=DEV)
    score, last_label = torch.tensor([0.0, -2.5], device=DEV), i32([-1, 4])
    trunc = torch.zeros(B, dtype=torch.bool, device=DEV)
    idle = [t[1].clone() for t in (hyp, hyp_len, steps, score, last_label, trunc)] + [h[:, 1].clone(), c[:, 1].clone()]
    want_tokens, last, total, terms = [], -1, 0.0, []
    for k, labs in enumerate(labels):
        lp = torch.randn(B, S, V, generator=g)
        for s, lab in enumerate(labs):
            lp[0, s, lab] += 10.0                                # one clearly best class per step
        lp = lp.log_softmax(-1)
        best = lp[0].max(-1)
        assert best.indices.tolist() == labs
        final = k == len(labels) - 1
        hn, cn = torch.randn(L, B, H, generator=g).to(DEV), torch.randn(L, B, H, generator=g).to(DEV)
        h_before, c_before = h.clone(), c.clone()
        ali, sc = torch.full((B, S), -1, dtype=torch.int64, device=DEV), torch.full((B, S), -1.0, device=DEV)
        ops.stream_collapse(lp.to(DEV), i32([S, 0]), i32([ops.STREAM_ACTIVE | (ops.STREAM_FINAL if final else 0), 0]), hn, cn, h, c,
                            ali, sc, hyp, hyp_len, steps, score, last_label, trunc)
        tokens, last = stream_ref.collapse(labs, last)
        want_tokens += tokens
        terms += best.values.double().tolist()
        assert ali[0].tolist() == labs and ali[1].tolist() == [0, 0]
        assert torch.equal(sc[0].cpu(), best.values) and sc[1].abs().max() == 0
        assert last_label[0].item() == last and steps[0].item() == S * (k + 1)
        assert hyp_len[0].item() == min(len(want_tokens), capacity)
        assert hyp[0, :hyp_len[0]].tolist() == want_tokens[:capacity]
        assert trunc[0].item() == (len(want_tokens) > capacity)
        # the state commit: the row that goes on takes hn / cn; a final row and an inactive row keep theirs
        assert torch.equal(h[:, 0], h_before[:, 0] if final else hn[:, 0]) and torch.equal(c[:, 0], c_before[:, 0] if final else cn[:, 0])
        total = sum(terms)
        assert abs(score[0].item() - total) <= len(terms) * U * sum(abs(t) for t in terms)
        now = [t[1] for t in (hyp, hyp_len, steps, score, last_label, trunc)] + [h[:, 1], c[:, 1]]
        assert all(torch.equal(a, b) for a, b in zip(idle, now))
    assert want_tokens == [1, 2, 2, 3]
    if capacity == 2:
        assert hyp_len[0].item() == 2 and trunc[0].item() and hyp[0].tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------- 3. end to end, the tiny goldens
@pytest.mark.parametrize('math_mode', ['f32', 'bf16x3'], indirect=True)
@pytest.mark.parametrize('name', ['g1_tiny_l2', 'g1_tiny_l3'])
def test_streams_match_the_reference_goldens(hal, name, math_mode):
    """H = 32: the general head and the step-launch LSTM.  5 pushes of 8 and a finish with a tail of 1 per row against the reference's
    alignments and hypotheses; ragged lengths (41, 23, 9) against infer.LstmCtcRecognizer on each row's own frames."""
    g = load_golden(name)
    enc, rec = _modules(hal, _params(g, 'encoder.'), _params(g, 'recognizer.'))
    x = torch.from_numpy(g['x']).to(DEV)
    B = x.shape[0]
    sr = hal['streaming'].StreamingRecognizer(enc, rec, B, chunk_frames=8, capacity=16)
    ali, _, _ = _stream(sr, x, [41] * B, 8)
    hyps, _, steps, trunc = _hyps(sr)
    assert ali == g['ali'].tolist() and steps.tolist() == [11] * B and not trunc.any()
    assert hyps == [g['hyps'][b][:g['hlen'][b]].tolist() for b in range(B)]
    lengths = [41, 23, 9]
    ali, _, _ = _stream(sr, x, lengths, 8)                      # the same slots, begun again
    hyps, score, steps, _ = _hyps(sr)
    whole = hal['infer'].LstmCtcRecognizer(enc, rec, use_graph=False)
    for b, T in enumerate(lengths):
        w_ali, w_scores, w_hyp, w_len = whole.recognize(x[b:b + 1, :T].contiguous())
        assert ali[b] == w_ali[0].tolist() and steps[b].item() == w_ali.shape[1]
        assert hyps[b] == w_hyp[0, :w_len[0]].tolist()
        assert abs(score[b].item() - w_scores.double().sum().item()) <= 1e-4 * max(1.0, abs(w_scores.double().sum().item()))


# --------------------------------------------------------------------------------------------- 4. end to end, the fast path's shape
FAST = dict(F_=80, C=128, H=1024, L=2, V=32, B=5, T=80, chunk=16, lengths=[80, 80, 80, 80, 57])


@pytest.fixture(scope='module')
def fast_case():
    """Parameters, inputs and the float64 oracle's log-probs of every row's own frames: computed once, shared, never changed."""
    from oracle import cpu_ref
    c = FAST
    enc_p, rec_p = cpu_ref.make_params(c['F_'], c['C'], c['H'], c['L'], c['V'], seed=42)
    rec_p['classifier.weight'] = rec_p['classifier.weight'] * 100
    x = 8 * torch.randn(c['B'], c['T'], c['F_'], generator=torch.Generator().manual_seed(43))
    enc64, rec64 = {k: v.double() for k, v in enc_p.items()}, {k: v.double() for k, v in rec_p.items()}
    oracle = []
    with torch.no_grad():
        for b, T in enumerate(c['lengths']):
            feats, _, _ = cpu_ref.encoder_forward(enc64, x[b:b + 1, :T].double(), torch.tensor([T]))
            oracle.append(cpu_ref.classifier_log_probs(rec64, feats)[0])
    return enc_p, rec_p, x, oracle


@pytest.mark.parametrize('math_mode', ['bf16x3', 'f32', 'bf16'], indirect=True)
def test_streams_at_the_fast_path_shape(hal, fast_case, math_mode):
    """LC-2x1024, 5 streams, chunks of 16; row 4 ends after 57 frames (3 pushes and a tail of 9) while the others go on.  The streamed
    log-probs may be at most twice as far from the float64 oracle as the whole-utterance path (Encoder + TemporalClassifier.log_probs)
    is in the same arithmetic mode; in the fp32-grade modes the labels equal the oracle's on every frame it decides by more than
    10 * e_whole, which must be at least 95 % of the frames."""
    enc_p, rec_p, x, oracle = fast_case
    c = FAST
    enc, rec = _modules(hal, enc_p, rec_p)
    xd = x.to(DEV)
    e_whole = 0.0
    with torch.no_grad():
        for rows, T in ((slice(0, 4), 80), (slice(4, 5), 57)):
            feats, _, _ = enc(xd[rows, :T].contiguous(), torch.full((rows.stop - rows.start,), T, device=DEV))
            lp = rec.log_probs(feats).cpu().double()
            for i, b in enumerate(range(rows.start, rows.stop)):
                e_whole = max(e_whole, (lp[i] - oracle[b]).abs().max().item())
    sr = hal['streaming'].StreamingRecognizer(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32)
    ali, lp, _ = _stream(sr, xd, c['lengths'], c['chunk'], want_lp=True)
    e_stream = max((lp[b].double() - oracle[b]).abs().max().item() for b in range(c['B']))
    print(f'streaming {math_mode}: e_stream {e_stream:.3e} e_whole {e_whole:.3e}')
    hyps, _, steps, _ = _hyps(sr)
    assert steps.tolist() == [o.shape[0] for o in oracle] == [21, 21, 21, 21, 15]
    assert e_stream <= 2 * e_whole, (e_stream, e_whole)
    if math_mode != 'bf16':
        total = left_out = 0
        for b in range(c['B']):
            top2 = oracle[b].topk(2, dim=-1).values
            decided = (top2[:, 0] - top2[:, 1]) > 10 * e_whole
            total += decided.numel(); left_out += int((~decided).sum())
            want = oracle[b].argmax(-1)
            assert torch.equal(torch.tensor(ali[b])[decided], want[decided])
            if bool(decided.all()):
                assert hyps[b] == stream_ref.collapse(want.tolist())[0]
        assert left_out <= 0.05 * total, (left_out, total)


# ------------------------------------------------------------------------------------------------------ 5. determinism and reuse
def _same(rec_a, rec_b):
    for (last_a, part_a), (last_b, part_b) in zip(rec_a, rec_b):
        assert all(torch.equal(a, b) for a, b in zip(last_a, last_b)) and all(torch.equal(a, b) for a, b in zip(part_a, part_b))
    assert len(rec_a) == len(rec_b)


def test_replay_reuse_and_general_path_agree(hal, fast_case, monkeypatch):
    """At the fast path's shape: graph replay and eager launches are bit-identical in ``partial()`` and ``last`` after every call; so is
    the same audio streamed again through re-begun slots after an unrelated utterance used them; HALO_STREAM_FUSED=0 gives the same
    tokens, alignments and step counts."""
    enc_p, rec_p, x, _ = fast_case
    c = FAST
    enc, rec = _modules(hal, enc_p, rec_p)
    xd = x.to(DEV)
    S = hal['streaming'].StreamingRecognizer
    eager = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32, use_graph=False)
    ali_e, _, rec_e = _stream(eager, xd, c['lengths'], c['chunk'])
    graph = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32, use_graph=True)
    ali_g, _, rec_g = _stream(graph, xd, c['lengths'], c['chunk'])
    assert graph._graphs and ali_g == ali_e
    _same(rec_e, rec_g)
    other = 3 * torch.randn(c['B'], 48, c['F_'], generator=torch.Generator().manual_seed(5)).to(DEV)
    for sr in (eager, graph):
        _stream(sr, other, [48, 32, 48, 16, 48], c['chunk'])       # an unrelated utterance in every slot
        ali_2, _, rec_2 = _stream(sr, xd, c['lengths'], c['chunk'])
        assert ali_2 == ali_e
        _same(rec_e, rec_2)
    monkeypatch.setenv('HALO_STREAM_FUSED', '0')
    general = S(enc, rec, c['B'], chunk_frames=c['chunk'], capacity=32)
    assert not general.fused and eager.fused
    ali_p, _, rec_p2 = _stream(general, xd, c['lengths'], c['chunk'])
    assert ali_p == ali_e
    for (last_e, part_e), (last_p, part_p) in zip(rec_e, rec_p2):
        assert torch.equal(last_e[2], last_p[2])                                   # n_steps
        assert torch.equal(part_e[0], part_p[0]) and torch.equal(part_e[1], part_p[1]) and torch.equal(part_e[3], part_p[3])


# ------------------------------------------------------------------------------------------------------------ 6. interface errors
def test_interface_errors(hal):
    from oracle import cpu_ref
    enc_p, rec_p = cpu_ref.make_params(12, 16, 32, 2, 9, seed=3)
    enc, rec = _modules(hal, enc_p, rec_p)
    S = hal['streaming'].StreamingRecognizer
    with pytest.raises(ValueError):
        S(enc, rec, 2, chunk_frames=10)
    with pytest.raises(ValueError):
        S(enc, rec, 2, chunk_frames=128)
    enc.train()
    with pytest.raises(ValueError):
        S(enc, rec, 2, chunk_frames=8)
    enc.eval()
    odd = hal['rnn'].Encoder(12, 16, 32, num_layers=2)
    odd.subsample = torch.nn.Conv1d(12, 16, kernel_size=3, stride=2, padding=1)
    with pytest.raises(NotImplementedError):
        S(odd.to(DEV).eval(), rec, 2, chunk_frames=8)
    sr = S(enc, rec, 2, chunk_frames=8, capacity=4)
    fr = torch.zeros(2, 8, 12, device=DEV)
    with pytest.raises(ValueError):
        sr.push(fr)                                              # closed slots without begin
    with pytest.raises(ValueError):
        sr.finish(rows=[True, False])                            # never begun
    with pytest.raises(ValueError):
        sr.push(torch.zeros(2, 4, 12, device=DEV), begin=[True, True])
    with pytest.raises(ValueError):
        sr.push(fr.double(), begin=[True, True])
    with pytest.raises(ValueError):
        sr.push(fr, active=[True], begin=[True])
    sr.push(fr, active=[True, False], begin=[True, False])
    with pytest.raises(ValueError):
        sr.push(fr)                                              # slot 1 is still closed
    sr.push(fr, active=[True, False], begin=[True, False])       # begin on an open slot abandons the stream: allowed
    with pytest.raises(ValueError):
        sr.finish(torch.zeros(2, 8, 12, device=DEV), [8, 0])      # a tail is shorter than a chunk
    with pytest.raises(ValueError):
        sr.finish(torch.zeros(2, 3, 12, device=DEV), [4, 0])
    sr.finish(torch.zeros(2, 3, 12, device=DEV), [3, 0])          # closes slot 0 (the default rows: every open slot)
    assert sr.partial()[3].tolist() == [2 + 2, 0]
    with pytest.raises(ValueError):
        sr.push(fr, active=[True, False])                        # closed again
    with pytest.raises(ValueError):
        sr.finish(rows=[0])
    enc.train()
    with pytest.raises(ValueError):
        sr.push(fr, begin=[True, True])
    enc.eval()
