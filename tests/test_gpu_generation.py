"""GPU tests of haloop_amd.generation (the batched sampler on the fused decode launches of csrc/gpt_decode.hip) against the CPU oracle
(oracle/gpt_ref.py), the reference's own greedy chains (tests/golden/g13_gpt_generate.npz, written by make_golden_generate.py) and a
float64 restatement of the draw on oracle/philox.py.

Logit gates (max-abs error against oracle.gpt_ref.gpt_forward on the CPU, fp32).  Measured on the MI355X over the 2 x 384 teacher-forced
positions of the 2-layer fixture model and the 128 positions of the GPT-2 small case:
    bf16x3: 7.93e-5 and 7.29e-5 (2-layer, seeds 0 and 1), 7.44e-5 (GPT-2 small)      bf16: 3.96e-2 and 4.39e-2 (2-layer), 3.95e-2 (GPT-2 small)
The gate is twice the larger figure of a mode and may not exceed 5e-3 (bf16x3) / 5e-2 (bf16), half the top-2 margins below which a
position is left out of the token comparison (1e-2 / 0.1).  bf16x3: 2 x 7.93e-5 = 1.6e-4.  bf16: 2 x 4.39e-2 = 8.8e-2 is ABOVE the cap,
so the gate is the cap, 5e-2, only 1.14 times the measured error: a finding, not a loosened gate.  The error is that of the mode (both
operands of every product rounded to bf16; GPT.forward on the general operators in the same mode sits 2.6e-2 from the fused step), and
every position with a reference margin >= 0.1 still agreed with the reference's token.
"""
import contextlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LOGIT_GATE = {'bf16x3': 1.6e-4, 'bf16': 5e-2}        # twice the measured error (docstring), capped at half the margin thresholds
MARGIN = {'bf16x3': 1e-2, 'bf16': 0.1}
# keys / values of the cache: one LayerNorm + product per layer on values of order 1.  bf16x3 carries ~2^-16 per operand (the existing
# cache test of test_gpu_parity.py gates the same products at 1e-4); bf16 rounds both operands to 2^-9 relative, a K = 768 dot product of
# order 1 then carries ~2^-8 / sqrt(3) rms and its maximum over ~10^6 elements five times that, doubled for the second layer's input
CACHE_ATOL = {'bf16x3': 2e-4, 'bf16': 3e-2}
MODES = pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
GPT_ENTRIES = ('halo_gpt_decode_linear', 'halo_gpt_decode_attention', 'halo_gpt_sample')


@pytest.fixture(scope='module', autouse=True)
def halo():
    from haloop_amd import _lib
    _lib.lib()
    _lib.lend_scratch()
    return _lib


@contextlib.contextmanager
def math_mode(mode):
    from haloop_amd import _lib
    prev = _lib.get_math_mode()
    _lib.set_math_mode(mode)
    try:
        yield
    finally:
        _lib.set_math_mode(prev)


@contextlib.contextmanager
def counted(names):
    """Counts the calls of libhalo entry points (the ctypes functions are attributes of the CDLL instance)."""
    from haloop_amd import _lib
    L = _lib.lib()
    orig = {n: getattr(L, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def wrap(n, fn):
        def f(*a):
            calls[n] += 1
            return fn(*a)
        return f
    for n, fn in orig.items():
        setattr(L, n, wrap(n, fn))
    try:
        yield calls
    finally:
        for n, fn in orig.items():
            setattr(L, n, fn)


def all_entries():
    from haloop_amd import _lib
    return tuple(n for n in _lib.SIGNATURES if not n.endswith(('_bytes', '_supported')) and n not in ('halo_get_math_mode', 'halo_set_math_mode'))


def build_model(vocab, block, n_layer, n_head, n_embd, seed):
    from haloop_amd import attention
    from oracle import gpt_ref
    params = gpt_ref.make_gpt_params(vocab, block, n_layer, n_head, n_embd, False, seed)
    model = attention.GPT(attention.GPTConfig(block_size=block, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=False))
    model.load_state_dict(params, strict=True)
    return params, model.to(DEV).eval()


def fixture_case(seed):
    g = load_golden('g13_gpt_generate')
    vocab, block, n_layer, n_head, n_embd, rows, prompt, new, stride = (int(v) for v in g['cfg'])
    prompts = torch.randint(1, vocab, (rows, prompt), generator=torch.Generator().manual_seed(seed + 1))
    assert np.array_equal(prompts.numpy(), g[f'prompts{seed}'])
    params, model = build_model(vocab, block, n_layer, n_head, n_embd, seed)
    return dict(params=params, model=model, prompts=prompts, tokens=torch.from_numpy(g[f'tokens{seed}']), top2=g[f'top2_{seed}'],
                strided=g[f'strided{seed}'], n_layer=n_layer, n_head=n_head, stride=stride, new=new)


def oracle_chain(params, n_layer, n_head, prompts, tokens):
    """Teacher-forced CPU oracle: logits [B, N, V] where logits[:, 0] follow the prompt and logits[:, i] the input tokens[:, i - 1]."""
    from oracle import gpt_ref
    torch.set_num_threads(16)
    out = []
    with torch.no_grad():
        lg, past = gpt_ref.gpt_forward(params, n_layer, n_head, prompts)
        out.append(lg[:, 0])
        for i in range(tokens.shape[1] - 1):
            lg, past = gpt_ref.gpt_forward(params, n_layer, n_head, tokens[:, i:i + 1], past=past)
            out.append(lg[:, 0])
    return torch.stack(out, 1), past


def teacher_forced(model, prompts, tokens, n_layer, max_len=None):
    """The Sampler's logits [B, N, V] on the same inputs, with the fused launches asserted taken and counted."""
    from haloop_amd import generation
    B, N = tokens.shape
    sampler = generation.Sampler(model, B, max_len=max_len, use_graph=False)
    assert sampler.fused
    out = []
    with torch.no_grad():
        out.append(sampler.prefill(prompts.to(DEV)).clone())
        dev_tokens = tokens.to(DEV)
        with counted(all_entries()) as calls:
            for i in range(N - 1):
                out.append(sampler.step(dev_tokens[:, i]).clone())
    steps = N - 1
    assert calls['halo_gpt_decode_linear'] == (4 * n_layer + 1) * steps and calls['halo_gpt_decode_attention'] == n_layer * steps, calls
    others = {n: c for n, c in calls.items() if c and n not in GPT_ENTRIES and n != 'halo_embed_fwd'}
    assert not others, others                     # no general operator ran inside a fused step
    return torch.stack(out, 1).cpu(), sampler


def check_chain(name, mode, got, oracle, ref_tokens, top2, max_left_out, strided=None, stride=None):
    err = float((got - oracle).abs().max())
    print(f'[{name} {mode}] max |logits - oracle| = {err:.3e}')
    if strided is not None:
        err_ref = float(np.abs(got.numpy()[..., ::stride] - strided).max())
        print(f'[{name} {mode}] max |logits - reference| at stride {stride} = {err_ref:.3e}')
    margin = top2[..., 0] - top2[..., 1]
    compare = margin >= MARGIN[mode]
    left_out = int((~compare).sum())
    agree = got.argmax(-1).numpy() == ref_tokens.numpy()
    print(f'[{name} {mode}] left out {left_out} of {compare.size}, disagreements among the compared {int((~agree & compare).sum())}')
    assert err <= LOGIT_GATE[mode], err
    if strided is not None:
        assert err_ref <= LOGIT_GATE[mode], err_ref
    assert left_out <= max_left_out, left_out
    assert bool(agree[compare].all())


# ---- 1. teacher-forced parity on the fixture model ---------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize('seed', [0, 1])
def test_teacher_forced_logits_match_oracle_and_reference(seed, mode):
    c = fixture_case(seed)
    with math_mode(mode):
        got, _ = teacher_forced(c['model'], c['prompts'], c['tokens'], c['n_layer'])
    oracle, _ = oracle_chain(c['params'], c['n_layer'], c['n_head'], c['prompts'], c['tokens'])
    # the oracle restates the reference: its own distance from the stored reference logits is fp32 rounding
    assert float(np.abs(oracle.numpy()[..., ::c['stride']] - c['strided']).max()) < 1e-4
    check_chain(f'fixture seed {seed}', mode, got, oracle, c['tokens'], c['top2'], {'bf16x3': 4, 'bf16': 10}[mode], c['strided'], c['stride'])


# ---- 2. GPT-2 small depth and vocabulary -------------------------------------------------------------------------------------------
@MODES
def test_gpt2_small_teacher_forced(mode):
    from oracle import gpt_ref
    n_layer, n_head, B, P, N = 12, 12, 4, 16, 32
    params, model = build_model(50304, 1024, n_layer, n_head, 768, 0)
    prompts = torch.randint(1, 50304, (B, P), generator=torch.Generator().manual_seed(1))
    # the oracle's own greedy chain, and its logits along it
    torch.set_num_threads(16)
    logits, toks = [], []
    with torch.no_grad():
        lg, past = gpt_ref.gpt_forward(params, n_layer, n_head, prompts)
        for i in range(N):
            logits.append(lg[:, 0])
            toks.append(lg[:, 0].argmax(-1))
            if i + 1 < N:
                lg, past = gpt_ref.gpt_forward(params, n_layer, n_head, toks[-1][:, None], past=past)
    oracle, tokens = torch.stack(logits, 1), torch.stack(toks, 1)
    top2 = torch.topk(oracle, 2, dim=-1).values.numpy()
    with math_mode(mode):
        got, _ = teacher_forced(model, prompts, tokens, n_layer, max_len=64)
    check_chain('gpt2 small', mode, got, oracle, tokens, top2, {'bf16x3': 3, 'bf16': 10}[mode])


# ---- 3. free-running greedy ----------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize('seed', [0, 1])
def test_free_running_greedy(seed, mode):
    from haloop_amd import generation
    c = fixture_case(seed)
    prompts, N, L = c['prompts'].to(DEV), c['new'], c['n_layer']
    with math_mode(mode), torch.no_grad():
        sampler = generation.Sampler(c['model'], 8, use_graph=False)
        with counted(GPT_ENTRIES) as calls:
            tokens, lengths = sampler.sample(prompts, N, top_k=1, stop_token=-1)
        assert sampler.fused
        # 5 n_layer + 2 launches per step: the first token needs the draw alone
        assert calls == {'halo_gpt_decode_linear': (4 * L + 1) * (N - 1), 'halo_gpt_decode_attention': L * (N - 1), 'halo_gpt_sample': N}, calls
        assert lengths.tolist() == [N] * 8
        # self-consistency, bit-equal: the arg-max chain of the Sampler's own step logits
        chain = [sampler.prefill(prompts).argmax(-1)]
        for i in range(N - 1):
            chain.append(sampler.step(chain[-1]).argmax(-1))
        assert torch.equal(torch.stack(chain, 1), tokens)
    tokens = tokens.cpu().numpy()
    margin = c['top2'][..., 0] - c['top2'][..., 1]
    compared = 0
    for r in range(8):
        under = np.nonzero(margin[r] < MARGIN[mode])[0]
        n = int(under[0]) if len(under) else N
        assert np.array_equal(tokens[r, :n], c['tokens'][r, :n].numpy()), (r, n)
        compared += n
    print(f'[free-running seed {seed} {mode}] compared {compared} of {8 * N}')
    assert compared >= 200


# ---- 4. the cache ----------------------------------------------------------------------------------------------------------------------
@MODES
def test_cache_matches_oracle_and_feeds_forward(mode):
    from haloop_amd import generation
    c = fixture_case(0)
    k = 9
    toks = c['tokens'][:, :k + 1]
    oracle, present = oracle_chain(c['params'], c['n_layer'], c['n_head'], c['prompts'], toks)
    with math_mode(mode), torch.no_grad():
        sampler = generation.Sampler(c['model'], 8, use_graph=False)
        sampler.prefill(c['prompts'].to(DEV))
        for i in range(k):
            sampler.step(toks[:, i].to(DEV))
        past = sampler.past()
        assert past.shape == present.shape == (c['n_layer'], 2, 8, c['n_head'], 16 + k, 64)
        err = float((past.cpu() - present).abs().max())
        print(f'[cache {mode}] max |past - oracle present| = {err:.3e}')
        assert err <= CACHE_ATOL[mode]
        nxt = toks[:, k:k + 1].to(DEV)
        via_forward, _ = c['model'](nxt, past=past)
        via_step = sampler.step(nxt[:, 0])
        # two paths of the same mode, each within the gate of the oracle
        diff = float((via_forward[:, 0] - via_step).abs().max())
        print(f'[cache {mode}] max |GPT.forward(past) - Sampler.step| = {diff:.3e}')
        assert diff <= 2 * LOGIT_GATE[mode]


# ---- 5. the draw -----------------------------------------------------------------------------------------------------------------------
def restated_u(rows, steps, seed):
    """u[row, step] of include/halo.h: philox4x32_10(ctr = (row, 0, stream, step), key = seed)[0] >> 8, times 2^-24."""
    from haloop_amd import _lib
    from oracle import philox
    r, s = np.meshgrid(np.arange(rows, dtype=np.uint32), np.arange(steps, dtype=np.uint32), indexing='ij')
    z = np.zeros_like(r)
    x = philox.philox4x32_10(r, z, np.full_like(r, _lib.HALO_GPT_SAMPLE_STREAM), s, seed & 0xFFFFFFFF, seed >> 32)[0]
    return (x >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def restated_cdf(logits, temperature, top_k):
    """float64: kept set (every logit >= the k-th largest: ties stay) and the CDF of the kept mass in vocabulary order."""
    l = logits.astype(np.float64)
    keep = np.ones_like(l, dtype=bool)
    if top_k is not None:
        kth = np.sort(l, axis=1)[:, -min(top_k, l.shape[1])]
        keep = l >= kth[:, None]
    s = l / temperature
    e = np.where(keep, np.exp(s - s.max(1, keepdims=True)), 0.0)
    return keep, np.cumsum(e, axis=1)


def accepted(tokens, u, keep, cdf, delta=1e-5):
    """tokens [rows, steps]: c[t - 1] - delta * total <= u * total < c[t] + delta * total, and t is a kept index."""
    rows = np.arange(tokens.shape[0])[:, None]
    total = cdf[:, -1:]
    hi = cdf[rows, tokens]
    lo = np.where(tokens > 0, cdf[rows, np.maximum(tokens - 1, 0)], 0.0)
    target = u * total
    return keep[rows, tokens] & (lo - delta * total <= target) & (target < hi + delta * total)


def run_draws(logits, steps, temperature, top_k, seed):
    from haloop_amd import ops
    rows, V = logits.shape
    cfg = ops.gpt_sample_cfg(temperature, top_k, -1, seed, DEV)
    state = torch.zeros(4, rows, device=DEV, dtype=torch.int32)
    state[3].fill_(1)
    tokens = torch.full((rows, steps), -7, device=DEV, dtype=torch.int64)
    nxt = torch.zeros(rows, device=DEV, dtype=torch.int64)
    for _ in range(steps):
        ops.gpt_sample(logits, cfg, state, tokens, nxt)
    torch.cuda.synchronize()
    assert state[1].tolist() == [steps] * rows and state[2].tolist() == [steps] * rows and state[0].tolist() == [steps] * rows
    return tokens.cpu().numpy()


@pytest.mark.parametrize('V', [2048, 50304])
@pytest.mark.parametrize('top_k', [None, 1, 40])
@pytest.mark.parametrize('temperature', [0.7, 1.0])
def test_draw_matches_float64_restatement(V, top_k, temperature):
    rows, steps, seed = 8, 512, 0x1234567887654321                          # 4096 draws
    logits = (torch.randn(rows, V, generator=torch.Generator().manual_seed(V + 7)) * 2.0).to(DEV)
    tokens = run_draws(logits, steps, temperature, top_k, seed)
    assert tokens.min() >= 0 and tokens.max() < V
    host = logits.cpu().numpy()
    if top_k == 1:
        assert np.array_equal(tokens, np.repeat(host.argmax(1)[:, None], steps, 1))
    keep, cdf = restated_cdf(host, temperature, top_k)
    assert bool(keep[np.arange(rows)[:, None], tokens].all())              # a token below the top-k threshold never appears
    ok = accepted(tokens, restated_u(rows, steps, seed), keep, cdf)
    assert bool(ok.all()), f'{int((~ok).sum())} of {ok.size} draws outside the restated CDF interval'
    if top_k != 1:
        # teeth: the same check against the uniforms of the NEXT step rejects
        wrong = accepted(tokens, restated_u(rows, steps + 1, seed)[:, 1:], keep, cdf)
        assert int((~wrong).sum()) > ok.size // 2
        assert np.array_equal(tokens, run_draws(logits, steps, temperature, top_k, seed))
        assert not np.array_equal(tokens, run_draws(logits, steps, temperature, top_k, seed + 1))


# ---- 6. the captured step ----------------------------------------------------------------------------------------------------------------
@MODES
def test_graph_replay_equals_eager(mode):
    from haloop_amd import generation
    c = fixture_case(1)
    prompts = c['prompts'].to(DEV)
    with math_mode(mode), torch.no_grad():
        eager = generation.Sampler(c['model'], 8, use_graph=False)
        replay = generation.Sampler(c['model'], 8, use_graph=True)
        captured = []
        for kw in (dict(top_k=40, temperature=0.8, seed=11), dict(top_k=None, temperature=1.0, seed=12), dict(top_k=1, seed=0)):
            te, le = eager.sample(prompts, 48, stop_token=-1, **kw)
            tr, lr = replay.sample(prompts, 48, stop_token=-1, **kw)
            assert torch.equal(te, tr) and torch.equal(le, lr), kw
            captured.append(replay._graphs[8][1])
        # one captured step served every position 16 .. 63 of all three runs
        assert len(replay._graphs) == 1 and not eager._graphs
        assert captured[0] is captured[1] is captured[2]          # captured once, not once per call
        assert torch.equal(replay.past(), eager.past())


# ---- 7. stop handling, the reference's generator signature, the general path ------------------------------------------------------------
@MODES
def test_stop_token_ends_a_row_and_leaves_the_others(mode):
    from haloop_amd import generation
    c = fixture_case(0)
    prompts, N = c['prompts'].to(DEV), 48
    with math_mode(mode), torch.no_grad():
        sampler = generation.Sampler(c['model'], 8)
        chain, _ = sampler.sample(prompts, N, top_k=1, stop_token=-1)
        chain = chain.cpu().numpy()
        stop = int(chain[3, 5])
        tokens, lengths = sampler.sample(prompts, N, top_k=1, stop_token=stop)
    tokens, lengths = tokens.cpu().numpy(), lengths.cpu().numpy()
    stopped = 0
    for r in range(8):
        hits = np.nonzero(chain[r] == stop)[0]
        first = int(hits[0]) if len(hits) else N
        stopped += first < N
        assert lengths[r] == first, (r, lengths[r], first)
        assert np.array_equal(tokens[r, :first], chain[r, :first]) and (tokens[r, first:] == stop).all(), r
    assert 1 <= stopped and lengths[3] <= 5


@pytest.mark.parametrize('name', ['g5_gpt_tiny_nobias', 'g5_gpt_tiny_bias'])
def test_generate_matches_attention_generate_on_the_general_path(name):
    from haloop_amd import attention, generation
    g = load_golden(name)
    vocab, block, n_layer, n_head, n_embd, bias, B, T, seed = (int(v) for v in g['cfg'])
    params = {k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')}
    model = attention.GPT(attention.GPTConfig(block_size=block, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bool(bias)))
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    seq = torch.from_numpy(g['inputs'])[:1, :5].to(DEV)
    new = min(8, block - 5)
    want = [int(t) for t in attention.generate(model, seq, new, top_k=1, stop_token=-1)]
    out = list(generation.generate(model, seq, new, top_k=1, stop_token=-1))
    assert all(t.shape == (1, 1) and t.dtype == torch.int64 for t in out)
    assert [int(t) for t in out] == want
    assert not model._generation_sampler.fused                # C = 64: the general step on the preallocated cache
    with torch.no_grad():
        sampler = generation.Sampler(model, 2)
        assert not sampler.fused
        both = torch.cat([seq, seq], 0)
        tokens, lengths = sampler.sample(both, new, top_k=1, stop_token=-1)
    assert tokens.tolist() == [want, want] and lengths.tolist() == [new, new]


def test_errors_are_raised_before_any_launch():
    from haloop_amd import _lib, generation
    _, model = build_model(2048, 64, 1, 12, 768, 3)
    sampler = generation.Sampler(model, 2, max_len=32)
    ids = torch.ones(2, 8, dtype=torch.long, device=DEV)
    with counted(all_entries()) as calls:
        with torch.no_grad():
            with pytest.raises(ValueError):
                sampler.sample(torch.ones(3, 8, dtype=torch.long, device=DEV), 4)
            with pytest.raises(ValueError):
                sampler.sample(ids, 25)
            with pytest.raises(_lib.HaloError):
                sampler.sample(ids.cpu(), 4)
        with pytest.raises(NotImplementedError):
            sampler.sample(ids, 4)                               # grad enabled, trainable parameters
    assert not any(calls.values()), calls
