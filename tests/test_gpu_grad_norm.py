"""GPU tests of the per-utterance gradient norms: csrc/ghost_norm.hip alone against the float64 direct form, and
haloop_amd.grad_norm.gradient_norms end to end against the reference's fixture (g15) and the CPU oracle (tests/grad_norm_ref.py).

Bounds (none is tuned to what the kernels give):
  kernel alone   |kernel - direct64| <= bound * sum_{t,t'} |G_a| |n_bias + G_b|, bound = max(4 x the worst such error of the float32 Gram
                 restatement on the CPU over the cases, 4 float32 ulps): the MFMA adds the same products in another order, not more of them.
  end to end     relative error of a norm <= max(4 x the float32 oracle's own worst error against the float64 oracle on the same inputs,
                 1e-6) in the 'f32' and 'bf16x3' modes; 2e-2 in 'bf16' mode (the signals themselves carry bf16 rounding).
                 Losses likewise from the oracle's loss error; squared norms per parameter from the oracle's own per-parameter error
                 (floor 2e-6: a square doubles a relative error).
Measured worst errors are printed before each assertion (pytest -s) and recorded in DESIGN.md 3.3k.
"""
import numpy as np
import pytest
import torch

import ghost_norm_ref
import grad_norm_ref
from conftest import load_golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ULP = 2.0 ** -23


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops, grad_norm, rnn, recognizer
    _lib.lib()
    _lib.lend_scratch()
    return dict(lib=_lib, ops=ops, gn=grad_norm, rnn=rnn, recognizer=recognizer)


@pytest.fixture
def math_mode(request, hal):
    prev = hal['lib'].get_math_mode()
    hal['lib'].set_math_mode(request.param)
    yield request.param
    hal['lib'].set_math_mode(prev)


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
N = 5
KS = [1, 7, 32, 100]
COMBOS = [(nb, nbias) for nb in (0, 1, 2) for nbias in (0, 1, 2)]


def _operand(g, T, K, time_major, pad=0):
    """A random [N, T, K] operand (batch-first values) and how it is laid out on the device: time-major or batch-first, rows ``pad`` floats
    apart from dense."""
    v = torch.randn(N, T, K, generator=g)
    return v, time_major, pad


def _place(v, time_major, pad):
    """-> device tensor shaped [N, T, K] / [T, N, K] whose rows are K + pad floats apart (a view into a larger buffer, unit stride along K)."""
    src = v.transpose(0, 1) if time_major else v
    buf = torch.full(src.shape[:2] + (v.shape[2] + pad,), 7.5, device=DEV)          # the padding holds a value a stray read would show
    buf[:, :, :v.shape[2]] = src.to(DEV)
    return buf[:, :, :v.shape[2]]


def build_cases():
    """name -> (T, [(a, [b...], n_bias, time_major)]) with operands as (values, time_major, pad)."""
    from haloop_amd import ops
    TT = ops.ghost_tile()
    g = torch.Generator().manual_seed(1234)
    cases = {}
    for T in (1, TT - 1, TT, TT + 1, 2 * TT + 3):
        terms = []
        for i, (nb, nbias) in enumerate(COMBOS):        # every count of operands and biases, sizes and layouts cycling
            tm = (i + T) % 2 == 1
            ka = KS[(i + T) % 4]
            bs = [_operand(g, T, KS[(i + j + 1) % 4], tm, pad=(0, 3, 4)[(i + j) % 3]) for j in range(nb)]
            terms.append((_operand(g, T, ka, tm, pad=(0, 1, 4)[i % 3]), bs, nbias, tm))
        cases[f'T{T}'] = (T, terms)
    for T in (1, TT - 1):                               # the long K with the smaller T only
        terms = [(_operand(g, T, 4096, True), [_operand(g, T, 4096, True), _operand(g, T, 7, True)], 2, True),
                 (_operand(g, T, 100, False), [_operand(g, T, 4096, False)], 1, False),
                 (_operand(g, T, 4096, False, pad=4), [], 1, False)]
        cases[f'T{T}_k4096'] = (T, terms)
    # more terms than one launch's table holds
    T = TT + 1
    cases['many_terms'] = (T, [(_operand(g, T, KS[i % 4], i % 2 == 0), [_operand(g, T, KS[(i + 1) % 4], i % 2 == 0)], i % 3, i % 2 == 0)
                               for i in range(19)])
    # cancellation: a_t = (-1)^t u, b constant + 1e-3 noise: the per-frame outer products cancel pairwise
    T = 33
    u = torch.randn(N, 1, 100, generator=g)
    sign = torch.tensor([(-1.0) ** t for t in range(T)]).view(1, T, 1)
    b = torch.randn(N, 1, 100, generator=g) + 1e-3 * torch.randn(N, T, 100, generator=g)
    cases['cancel'] = (T, [((sign * u, True, 0), [(b, True, 0)], 0, True), ((sign * u, False, 0), [(b, False, 0)], 0, False)])
    return cases


@pytest.fixture(scope='module')
def kernel_cases():
    """Cases, their float64 direct form, scale and float32-Gram error, computed once."""
    cases = build_cases()
    ref = {}
    worst32 = 0.0
    for name, (T, terms) in cases.items():
        rows = []
        for a, bs, nbias, _ in terms:
            direct = ghost_norm_ref.direct_sqnorm64(a[0], [b[0] for b in bs], nbias)
            scale = ghost_norm_ref.gram_scale64(a[0], [b[0] for b in bs], nbias)
            g32 = ghost_norm_ref.gram_sqnorm(a[0], [b[0] for b in bs], nbias, torch.float32).double()
            live = scale > 0
            if live.any():
                worst32 = max(worst32, float(((g32 - direct).abs()[live] / scale[live]).max()))
            rows.append((direct, scale))
        ref[name] = rows
    return cases, ref, worst32


def run_kernel(hal, T, terms, canary=-777.25):
    ops = hal['ops']
    recs = [ops.ghost_term(_place(*a), [_place(*b) for b in bs], nbias, time_major=tm) for a, bs, nbias, tm in terms]
    n_ws = ops.ghost_sqnorm_workspace(len(recs), N, T)
    n_sq = len(recs) * N
    G = 8                                               # guard words around every buffer
    flat = torch.full((G + n_ws + G + n_sq + G + N + G,), canary, device=DEV)
    ws = flat[G:G + n_ws]
    sq = flat[2 * G + n_ws:2 * G + n_ws + n_sq]
    norm = flat[3 * G + n_ws + n_sq:3 * G + n_ws + n_sq + N]
    ops.ghost_sqnorm(recs, N, T, workspace=ws, out=sq.view(len(recs), N), norm_out=norm)
    torch.cuda.synchronize()
    host = flat.cpu()
    guards = torch.cat([host[:G], host[G + n_ws:2 * G + n_ws], host[2 * G + n_ws + n_sq:3 * G + n_ws + n_sq], host[-G:]])
    assert torch.equal(guards, torch.full_like(guards, canary)), 'a guard word around the workspace / outputs was written'
    assert not (host[G:G + n_ws] == canary).any(), 'a workspace partial was never written'
    return sq.view(len(recs), N).cpu(), norm.cpu()


def test_kernel_against_float64_direct_form(hal, kernel_cases):
    cases, ref, worst32 = kernel_cases
    bound = max(4 * worst32, 4 * ULP)
    worst = 0.0
    for name, (T, terms) in cases.items():
        sq, norm = run_kernel(hal, T, terms)
        for i, (direct, scale) in enumerate(ref[name]):
            nb, nbias = len(terms[i][1]), terms[i][2]
            if nb == 0 and nbias == 0:
                assert torch.equal(sq[i], torch.zeros(N)), (name, i)        # no parameters: exactly 0
                continue
            err = (sq[i].double() - direct).abs() / scale
            worst = max(worst, float(err.max()))
            assert float(err.max()) <= bound, (name, i, float(err.max()), bound)
        # norm = sqrt(sum over terms): its square carries the terms' errors and the rounding of the sum and the root
        total, scale_all = sum(d for d, _ in ref[name]), sum(s for _, s in ref[name])
        assert float(((norm.double().square() - total).abs() / scale_all).max()) <= bound + 4 * ULP, name
    print(f'ghost kernel: worst error {worst:.3e} of sum|G_a||n_bias + G_b| (float32 Gram restatement on the CPU {worst32:.3e}, bound {bound:.3e})')


def test_kernel_cancellation_case(hal, kernel_cases):
    cases, ref, worst32 = kernel_cases
    T, terms = cases['cancel']
    sq, _ = run_kernel(hal, T, terms)
    bound = max(4 * worst32, 4 * ULP)
    for i, (direct, scale) in enumerate(ref['cancel']):
        err = (sq[i].double() - direct).abs() / scale
        print(f'cancellation case {i}: error {float(err.max()):.3e} of the scale, result / scale {float((direct / scale).max()):.3e}')
        assert float((direct / scale).max()) < 2e-3                          # the case does cancel: the result is a small part of the scale
        assert float(err.max()) <= bound
    assert torch.equal(sq[0], sq[1])                                         # the layout does not change a bit


def test_kernel_zero_signal_is_exactly_zero(hal):
    g = torch.Generator().manual_seed(5)
    T = hal['ops'].ghost_tile() + 1
    zero = (torch.zeros(N, T, 100), True, 0)
    terms = [(zero, [_operand(g, T, 32, True), _operand(g, T, 7, True)], 2, True), (zero, [], 1, True)]
    sq, norm = run_kernel(hal, T, terms)
    assert torch.equal(sq, torch.zeros(2, N)) and torch.equal(norm, torch.zeros(N))


def test_kernel_two_runs_are_bit_identical(hal, kernel_cases):
    cases, _, _ = kernel_cases
    for name in ('T67', 'T31_k4096'):
        T, terms = cases[name]
        first, second = run_kernel(hal, T, terms), run_kernel(hal, T, terms)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_kernel_refuses_bad_terms(hal):
    ops, lib = hal['ops'], hal['lib']
    a = torch.zeros(N, 3, 4, device=DEV)
    tm = ops.ghost_term(a, [a], 1)
    tm.n_b = 3
    with pytest.raises(lib.HaloError):
        ops.ghost_sqnorm([tm], N, 3)
    with pytest.raises(ValueError):
        ops.ghost_term(a, [a, a, a])
    with pytest.raises(ValueError):
        ops.ghost_term(a, [torch.zeros(N, 4, 4, device=DEV)])


# ----------------------------------------------------------------------------------------------------------------------- end to end
def fixture_case(L):
    g = load_golden('g15_grad_norms')
    pre = f'l{L}.'
    enc_p = {k[len(pre + 'param.encoder.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre + 'param.encoder.')}
    rec_p = {k[len(pre + 'param.recognizer.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre + 'param.recognizer.')}
    t = lambda k: torch.from_numpy(g[pre + k])
    want = dict(norms=torch.from_numpy(g[pre + 'norms']).double(), losses=torch.from_numpy(g[pre + 'losses']).double(),
                sq={k[len(pre + 'sq.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre + 'sq.')})
    return enc_p, rec_p, t('x'), t('il'), t('tg'), t('tl'), want


def build_system(hal, enc_p, rec_p, p_drop, seed=None, offset=0):
    C, F_ = enc_p['subsample.weight'].shape[:2]
    H, V = rec_p['classifier.weight'].shape[1], rec_p['classifier.weight'].shape[0]
    enc = hal['rnn'].Encoder(F_, C, H, num_layers=cpu_ref.num_lstm_layers(enc_p))
    rec = hal['recognizer'].TemporalClassifier(H, V)
    enc.load_state_dict(enc_p); rec.load_state_dict(rec_p)
    enc.dropout.p = p_drop; enc.lstm.dropout = p_drop; rec.dropout.p = p_drop
    if seed is not None:
        for m in (enc, rec):
            m.dropout_stream.seed, m.dropout_stream.offset = seed, offset
    return hal['gn'].MiniSystem(enc, rec).to(DEV)


def oracle_pair(enc_p, rec_p, x, il, tg, tl, masks):
    """The float64 oracle and the float32 oracle's own worst relative errors against it (norms, losses, per-parameter squared norms)."""
    r64 = grad_norm_ref.per_utterance(enc_p, rec_p, x, il, tg, tl, masks, torch.float64)
    r32 = grad_norm_ref.per_utterance(enc_p, rec_p, x, il, tg, tl, masks, torch.float32)
    rel = lambda a, b: float(((a.double() - b).abs() / b.abs()).max())
    e = dict(norms=rel(r32['norms'], r64['norms']), losses=rel(r32['losses'], r64['losses']),
             sq=max(rel(r32['sq'][k], r64['sq'][k]) for k in r64['sq']))
    return r64, e


def check_against(tag, got, want, e32, bf16=False):
    norms, losses, per = got
    rel = lambda a, b: float(((a.cpu().double() - b).abs() / b.abs()).max())
    b_norm = 2e-2 if bf16 else max(4 * e32['norms'], 1e-6)
    b_loss = 2e-2 if bf16 else max(4 * e32['losses'], 1e-6)
    b_sq = 4e-2 if bf16 else max(4 * e32['sq'], 2e-6)
    e_norm, e_loss = rel(norms, want['norms']), rel(losses, want['losses'])
    e_sq = {k: rel(per[k], want['sq'][k]) for k in want['sq']}
    worst = max(e_sq, key=e_sq.get)
    print(f'{tag}: norm error {e_norm:.3e} (bound {b_norm:.3e}, float32 oracle {e32["norms"]:.3e}), loss error {e_loss:.3e} (bound {b_loss:.3e}), '
          f'worst squared norm {worst} {e_sq[worst]:.3e} (bound {b_sq:.3e}, float32 oracle {e32["sq"]:.3e})')
    assert sorted(per) == sorted(want['sq'])
    assert e_loss <= b_loss, (tag, 'loss', e_loss, b_loss)
    bad = {k: v for k, v in e_sq.items() if not v <= b_sq}
    assert not bad, (tag, 'squared norms per parameter', bad, b_sq)
    assert e_norm <= b_norm, (tag, 'norm', e_norm, b_norm)


@pytest.fixture(scope='module')
def fixture_refs():
    out = {}
    for L in (2, 3):
        enc_p, rec_p, x, il, tg, tl, want = fixture_case(L)
        _, e32 = oracle_pair(enc_p, rec_p, x, il, tg, tl, None)
        out[L] = (enc_p, rec_p, x, il, tg, tl, want, e32)
    return out


@pytest.mark.parametrize('math_mode', ['f32'], indirect=True)
@pytest.mark.parametrize('L', [2, 3])
def test_fixture_norms_without_dropout(hal, math_mode, fixture_refs, L):
    enc_p, rec_p, x, il, tg, tl, want, e32 = fixture_refs[L]
    system = build_system(hal, enc_p, rec_p, 0.0)
    got = hal['gn'].gradient_norms(system, x.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV), per_parameter=True)
    assert system.training
    check_against(f'g15 L={L} f32', got, want, e32)
    norms2, losses2 = hal['gn'].gradient_norms(system, x.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV))
    assert torch.equal(norms2, got[0]) and torch.equal(losses2, got[1])          # same inputs, same bits


@pytest.mark.parametrize('math_mode', ['f32'], indirect=True)
@pytest.mark.parametrize('L', [2, 3])
def test_norms_with_dropout(hal, math_mode, L):
    enc_p, rec_p, x, il, tg, tl, _ = fixture_case(L)
    seed, offset = 4321, 7
    C, H = enc_p['subsample.weight'].shape[0], rec_p['classifier.weight'].shape[1]
    Tp = int(cpu_ref.subsampled_lengths(torch.tensor([x.shape[1]]))[0])
    masks = cpu_ref.philox_masks(x.shape[0], Tp, C, H, L, 0.2, 0.2, seed, offset)
    r64, e32 = oracle_pair(enc_p, rec_p, x, il, tg, tl, masks)
    system = build_system(hal, enc_p, rec_p, 0.2, seed, offset)
    got = hal['gn'].gradient_norms(system, x.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV), per_parameter=True)
    assert system.encoder.dropout_stream.offset == offset + 1 and system.recognizer.dropout_stream.offset == offset + 1
    check_against(f'dropout 0.2 L={L} f32', got, r64, e32)


@pytest.fixture(scope='module')
def persistent_case():
    F_, C, H, L, V, B, T, S = 80, 128, 256, 2, 32, 32, 80, 10
    enc_p, rec_p = cpu_ref.make_params(F_, C, H, L, V, 31)
    x, il, tg, tl = cpu_ref.synthetic_batch(B, T, F_, V, S, 32)
    il = torch.tensor([T - 2 * (i % 8) for i in range(B)], dtype=torch.int64)
    r64, e32 = oracle_pair(enc_p, rec_p, x, il, tg, tl, None)
    return enc_p, rec_p, x, il, tg, tl, r64, e32


@pytest.mark.parametrize('math_mode,persistent,kernel', [('bf16x3', True, 'lstm_persist_bwd_kernel'), ('bf16', True, 'lstm_persist2_bwd_kernel'),
                                                         ('bf16x3', False, 'lstm_step_bwd_kernel')], indirect=['math_mode'])
def test_persistent_paths(hal, math_mode, persistent, kernel, persistent_case):
    enc_p, rec_p, x, il, tg, tl, r64, e32 = persistent_case
    system = build_system(hal, enc_p, rec_p, 0.0)
    hal['lib'].set_lstm_persistent(persistent)
    try:
        got = hal['gn'].gradient_norms(system, x.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV), per_parameter=True)
        torch.cuda.synchronize()
        assert hal['lib'].lstm_chain_info('bwd')['kernel'] == kernel            # the path this case is here for
    finally:
        hal['lib'].set_lstm_persistent(True)
    check_against(f'H=256 L=2 B=32 {math_mode} persistent={persistent}', got, r64, e32, bf16=math_mode == 'bf16')


# ------------------------------------------------------------------------------------------------------------------- nothing leaks
def _train_step(system, x, il, tg, tl, seed, offset):
    for m in (system.encoder, system.recognizer):
        m.dropout_stream.seed, m.dropout_stream.offset = seed, offset
    system.zero_grad(set_to_none=True)
    loss = system(x, tg, il, tl)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in system.named_parameters()}


def test_training_step_is_untouched_by_a_call(hal, monkeypatch):
    enc_p, rec_p, x, il, tg, tl, _ = fixture_case(2)
    system = build_system(hal, enc_p, rec_p, 0.2, 99, 3)
    system.train()
    x, il, tg, tl = x.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)
    loss0, grads0 = _train_step(system, x, il, tg, tl, 99, 3)
    system.zero_grad(set_to_none=True)
    assert not hal['lib'].get_lstm_keep_gate_gradients()
    norms, losses = hal['gn'].gradient_norms(system, x, tg, il, tl)
    assert all(p.grad is None for p in system.parameters())
    assert not hal['lib'].get_lstm_keep_gate_gradients()
    loss1, grads1 = _train_step(system, x, il, tg, tl, 99, 3)
    assert torch.equal(loss0, loss1)
    for k in grads0:
        assert torch.equal(grads0[k], grads1[k]), k
    # a call that raises half way restores the flag too

    def boom(*args, **kwargs):
        raise RuntimeError('boom')

    monkeypatch.setattr(hal['ops'], 'lstm_ghost_terms', boom)
    with pytest.raises(RuntimeError, match='boom'):
        hal['gn'].gradient_norms(system, x, tg, il, tl)
    assert not hal['lib'].get_lstm_keep_gate_gradients()
    assert all(p.grad is None or torch.equal(p.grad, grads1[k]) for k, p in system.named_parameters())


def test_ghost_terms_need_a_kept_backward(hal):
    """Without the keep flag the backward may not leave dG in the reserve: the terms are refused, not wrong."""
    ops, lib = hal['ops'], hal['lib']
    g = torch.Generator().manual_seed(2)
    T, B, C, H, L = 5, 4, 16, 32, 2
    x = torch.randn(T, B, C, generator=g).to(DEV)
    w_ih = [torch.randn(4 * H, C if l == 0 else H, generator=g).to(DEV) * 0.1 for l in range(L)]
    w_hh = [torch.randn(4 * H, H, generator=g).to(DEV) * 0.1 for l in range(L)]
    b = [torch.zeros(4 * H, device=DEV) for l in range(L)]
    y, _, _, reserve = ops.lstm_fwd(x, w_ih, w_hh, b, b)
    with pytest.raises(lib.HaloError):
        ops.lstm_ghost_terms(x, reserve, H, L)                                   # no backward yet
    dy = torch.randn(T, B, H, generator=g).to(DEV)
    ops.lstm_bwd(x, w_ih, w_hh, dy, (B * H, H), False, reserve, want_dx=True)
    with pytest.raises(lib.HaloError):
        ops.lstm_ghost_terms(x, reserve, H, L)                                   # a backward without the flag
    y, _, _, reserve = ops.lstm_fwd(x, w_ih, w_hh, b, b, reserve=reserve)
    lib.set_lstm_keep_gate_gradients(True)
    try:
        ops.lstm_bwd(x, w_ih, w_hh, dy, (B * H, H), False, reserve, want_dx=True)
    finally:
        lib.set_lstm_keep_gate_gradients(False)
    assert len(ops.lstm_ghost_terms(x, reserve, H, L)) == L
    ops.lstm_fwd(x, w_ih, w_hh, b, b, reserve=reserve)
    with pytest.raises(lib.HaloError):
        ops.lstm_ghost_terms(x, reserve, H, L)                                   # the next forward has overwritten the gates
    torch.cuda.synchronize()


def test_unsupported_pairs_raise(hal):
    from haloop_amd import attention, attention_audio
    gn, rnn, recognizer = hal['gn'], hal['rnn'], hal['recognizer']
    x, tg = torch.zeros(2, 20, 12, device=DEV), torch.ones(2, 3, dtype=torch.int64, device=DEV)
    il, tl = torch.tensor([20, 20], device=DEV), torch.tensor([3, 2], device=DEV)
    enc, rec = rnn.Encoder(12, 16, 32, num_layers=1), recognizer.TemporalClassifier(32, 9)
    with pytest.raises(NotImplementedError, match='Transducer'):
        gn.gradient_norms(gn.MiniSystem(enc, recognizer.Transducer(32, 9)), x, tg, il, tl)
    cfg = attention.GPTConfig(block_size=64, vocab_size=11, n_layer=1, n_head=2, n_embd=64, bias=True, causal=False, d_input=12, rotary_emb_dim=0)
    with pytest.raises(NotImplementedError, match='AudioEncoder'):
        gn.gradient_norms(gn.MiniSystem(attention_audio.AudioEncoder(cfg), recognizer.TemporalClassifier(64, 9)), x, tg, il, tl)
    with pytest.raises(NotImplementedError, match='star'):
        gn.gradient_norms(gn.MiniSystem(enc, rec), x, tg, il, tl, star_penalty=1.0)
    assert not hal['lib'].get_lstm_keep_gate_gradients()
