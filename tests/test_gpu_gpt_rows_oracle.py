"""The GPT `bf16` path at the shapes where its row tiles switch on (B = 8, T = 1024: M = 8192 token rows) against the fp32 CPU oracle
(oracle/gpt_ref.py), which tests/test_oracle_golden.py pins to the reference.  The fixtures of tests/test_gpu_parity.py hold M = 1024, where
rowmajor_train_ok / rows_ok are false and the 128-tile launches run; here the same model runs on

    halo_gemm_rows (every Linear, 256-row tiles), halo_attention_fwd_b16 / _bwd_b16 (head_dim 64) or attention_fwd_bf16 / _bwd_bf16
    (head_dim 32), halo_gemm_rows_ce (lm_head + cross-entropy, the logits kept as bf16), the in-place bf16 CE gradient, and
    halo_gemm_tn_rows_group (the lm_head's weight gradient on 256-row tiles with K-sliced tail tiles)

with the training step (loss and every gradient, the tied wte / lm_head included) and scoring (per-token NLL, _trunk_rows +
halo_gemm_rows_ce) compared with ONE oracle result per config, also under forced tile shapes.  Every test asserts that it reached the
launches it claims (entry points of libhalo counted through the ctypes handle).

Gates, per config (CONFIGS):
    mean NLL within 2e-2 abs (BASELINE's bf16 gate); per-token NLL max abs error; per 256-token block (one gemm_rows / CE row tile)
    the mean error and the mean abs error, under tighter bounds;
    every gradient: norm within 5 %, cosine >= 0.995, relative error (Frobenius) of every 256-row block of its output rows (one
    gemm_tn_rows tile row) bounded, and for c_attn of every head's q / k / v rows.
The bounds (BOUNDS) are about twice the worst of the 128-tile path (HALO_GPT_ROWS=0, what the M = 1024 fixtures pin) and the row path
(the forced tile shapes included) against the oracle, measured on an MI355X -- 128-tile | row path:
              loss           nll max        block mean     block abs      grad block rel   c_attn head rel  norm           cosine
    gpt2w     1.0e-5|1.2e-4  3.1e-2|3.7e-2  1.2e-3|1.3e-3  7.4e-3|7.6e-3  1.42e-2|1.46e-2  9.3e-3|9.5e-3    7.6e-4|8.4e-4  >= 0.99996
    hd32      2.2e-4|1.4e-4  2.4e-2|2.6e-2  1.2e-3|1.7e-3  5.8e-3|5.9e-3  8.8e-3|8.9e-3    8.3e-3|8.5e-3    9.5e-4|8.4e-4  >= 0.99997
    v1000     1.3e-4|1.6e-4  2.4e-2|2.5e-2  8.7e-4|1.1e-3  5.5e-3|6.0e-3  8.6e-3|9.0e-3    8.1e-3|8.4e-3    9.5e-4|7.6e-4  >= 0.99997
test_the_gates_have_teeth applies the same comparison to perturbed copies of the GPU result (one 256-row block of the lm_head gradient
halved, as a lost K-slice would leave it; one 256-token block of the NLL shifted by twice its bound) and requires it to fail.

Cost: the oracle runs once per config on at most 16 threads (about 4 s for gpt2w, under 1 s for the others), each GPU pass takes
milliseconds.  The gpt2w oracle (V = 50304) holds the fp32 logits, their log-softmax and their gradient while it runs: about 5-7 GB of
host memory (8 GB peak resident for the process).
"""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, T, TILE = 8, 1024, 256
M = B * T

# id: (C, heads, layers, vocab)
CONFIGS = {
    'gpt2w': (768, 12, 2, 50304),       # attn_b16 forward / backward, the 288 / 192 / 96-column CE tiles, tn_rows with K-slices
    'hd32': (512, 16, 1, 2048),         # C // H = 32: the rows branch with attention_fwd_bf16 / attention_bwd_bf16
    'v1000': (512, 8, 1, 1000),         # V % 32 != 0: training falls back to gemm_split_ce; scoring: a ragged last CE column strip
}
# about twice the measured worst of the two paths (module docstring); the loss, norm and cosine gates are fixed
BOUNDS = {
    'gpt2w': dict(nll_max=8e-2, nll_block=3e-3, nll_block_abs=1.5e-2, block_rel=3e-2, head_rel=2e-2),
    'hd32': dict(nll_max=6e-2, nll_block=3.5e-3, nll_block_abs=1.2e-2, block_rel=2e-2, head_rel=1.8e-2),
    'v1000': dict(nll_max=6e-2, nll_block=3.5e-3, nll_block_abs=1.2e-2, block_rel=2e-2, head_rel=1.8e-2),
}
LOSS_ABS, NORM_REL, COS_MIN = 2e-2, 0.05, 0.995
# forced tile shapes, compared with the same oracle result: (environment, train?)
VARIANTS = {
    'gpt2w': [({'HALO_GEMM_ROWS_TN': '3'}, False), ({'HALO_GEMM_ROWS_TN': '6'}, False), ({'HALO_GEMM_ROWS_TN': '9'}, False),
              ({'HALO_GEMM_ROWS_TN': '3'}, True), ({'HALO_GEMM_ROWS_TN': '6'}, True), ({'HALO_GEMM_ROWS_TN': '9'}, True),
              ({'HALO_GEMM_TN_ROWS_TN': '4'}, True), ({'HALO_GEMM_TN_ROWS_TN': '8'}, True), ({'HALO_GEMM_TN_ROWS_TAIL': '0'}, True),
              ({'HALO_ATTN_B16_QB': '2'}, True), ({'HALO_ATTN_B16_QB': '2'}, False), ({'HALO_GEMM_TN_ROWS': '1'}, True)],
    'hd32': [({'HALO_GEMM_TN_ROWS': '1'}, True)],
    'v1000': [({'HALO_GEMM_TN_ROWS': '1'}, True)],
}
ENTRIES = ('halo_gemm_rows', 'halo_gemm_rows_ce', 'halo_gemm_split_ce', 'halo_gemm_tn_rows_group', 'halo_gemm_tn_bf16_group',
           'halo_attention_fwd_b16', 'halo_attention_bwd_b16', 'halo_attention_fwd_bf16', 'halo_attention_bwd_bf16')


# ---- the comparisons (also applied to perturbed copies by test_the_gates_have_teeth) -------------------------------------------------
def nll_failures(got, want, bounds):
    """Per-token NLL [M] against the oracle's: the max abs error; per 256-token block the mean error (a shifted tile) and the mean abs
    error (a noisier tile)."""
    err = got.double() - want.double()
    fails = []
    if float(err.abs().max()) > bounds['nll_max']:
        fails.append(f'nll max abs error {float(err.abs().max()):.3e} > {bounds["nll_max"]:.1e}')
    for what, blocks, bound in (('mean error', err.view(-1, TILE).mean(1).abs(), bounds['nll_block']),
                                ('mean abs error', err.abs().view(-1, TILE).mean(1), bounds['nll_block_abs'])):
        for i in torch.nonzero(blocks > bound).flatten().tolist():
            fails.append(f'nll block {i} (tokens {i * TILE}..{(i + 1) * TILE - 1}): {what} {float(blocks[i]):.3e} > {bound:.1e}')
    return fails


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def grad_stats(name, got, want, head_dim):
    """norm deviation, cosine, the relative error of every 256-row block of the output rows and (c_attn) of every head's q / k / v rows."""
    g, w = got.double(), want.double()
    g, w = (g.view(-1, 1), w.view(-1, 1)) if g.dim() == 1 else (g.reshape(g.shape[0], -1), w.reshape(w.shape[0], -1))
    ng, nw = float(g.norm()), float(w.norm())
    st = dict(norm=abs(ng - nw) / nw, cos=float((g * w).sum()) / (ng * nw),
              blocks=[_rel(g[r:r + TILE], w[r:r + TILE]) for r in range(0, g.shape[0], TILE)], heads=[])
    if name.endswith('attn.c_attn.weight'):
        C = g.shape[1]
        for h in range(C // head_dim):
            rows = torch.cat([torch.arange(j * C + h * head_dim, j * C + (h + 1) * head_dim) for j in range(3)])
            st['heads'].append(_rel(g[rows], w[rows]))
    return st


def grad_failures(grads, want, bounds, head_dim):
    fails = []
    for name, w in want.items():
        st = grad_stats(name, grads[name], w, head_dim)
        if st['norm'] > NORM_REL:
            fails.append(f'{name}: norm off by {st["norm"]:.3e}')
        if st['cos'] < COS_MIN:
            fails.append(f'{name}: cosine {st["cos"]:.5f}')
        for i, r in enumerate(st['blocks']):
            if r > bounds['block_rel']:
                fails.append(f'{name}: rows {i * TILE}.. relative error {r:.3e} > {bounds["block_rel"]:.1e}')
        for h, r in enumerate(st['heads']):
            if r > bounds['head_rel']:
                fails.append(f'{name}: head {h} relative error {r:.3e} > {bounds["head_rel"]:.1e}')
    return fails


# ---- oracle and GPU passes -----------------------------------------------------------------------------------------------------------
def oracle_result(cid):
    """fp32 CPU oracle: per-token NLL, the mean over the counted tokens, and every parameter's gradient of that mean (the tied wte /
    lm_head as one leaf)."""
    from oracle import gpt_ref
    C, H, L, V = CONFIGS[cid]
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        params = gpt_ref.make_gpt_params(V, T, L, H, C, bias=False, seed=17)
        ids, tg = gpt_ref.synthetic_tokens(B, T, V, seed=18)
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items() if k != 'lm_head.weight'}
        p = dict(leaves, **{'lm_head.weight': leaves['transformer.wte.weight']})
        nll = gpt_ref.gpt_forward_all(p, L, H, ids, tg, reduction='none')
        loss = nll.sum() / (tg != 0).sum()
        loss.backward()
        grads = {k: v.grad for k, v in leaves.items()}
        del p, leaves
        return dict(params=params, ids=ids, tg=tg, nll=nll.detach(), loss=float(loss.detach()), grads=grads)
    finally:
        torch.set_num_threads(threads)


@contextlib.contextmanager
def environment(pairs):
    old = {k: os.environ.get(k) for k in pairs}
    os.environ.update(pairs)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def counted(names=ENTRIES):
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


def gpu_pass(case, train, env=None):
    """One pass of the GPU model: training -> loss, gradients, the saved logits' dtype; scoring -> per-token NLL.  With the libhalo
    calls it made and whether the row-major / row-tile gates were open."""
    from haloop_amd import attention
    model, cfg = case['model'], case['model'].config
    C = cfg.n_embd
    out = {}
    with environment(env or {}), counted() as calls:
        out['rowmajor'] = attention.rowmajor_train_ok(cfg, model.transformer.h, M, train)
        out['rows'] = attention.rows_ok(M, C)
        if train:
            fwd = model._forward_train

            def keep_dtype(ids, tg):
                loss, saved = fwd(ids, tg)
                out['logits'] = saved.logits.dtype
                return loss, saved
            model._forward_train = keep_dtype
            try:
                model.train()
                for p in model.parameters():
                    p.grad = None
                loss = model.forward_all(case['ids'], case['tg'], reduction='mean')
                loss.backward()
                torch.cuda.synchronize()
            finally:
                del model._forward_train
            out['loss'] = float(loss.detach())
            out['grads'] = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
        else:
            model.eval()
            with torch.inference_mode():
                out['nll'] = model.forward_all(case['ids'], case['tg'], reduction='none').cpu()
    out['calls'] = dict(calls)
    return out


def assert_reached(cid, res, train):
    """The launches this config is meant to exercise did run."""
    calls = res['calls']
    assert res['rowmajor'] and res['rows'], (cid, res['rowmajor'], res['rows'])
    assert calls['halo_gemm_rows'] > 0, calls
    C, H, _, V = CONFIGS[cid]
    if C // H == 64:
        assert calls['halo_attention_fwd_b16'] > 0 and calls['halo_attention_fwd_bf16'] == 0, calls
    else:
        assert calls['halo_attention_fwd_bf16'] > 0 and calls['halo_attention_fwd_b16'] == 0, calls
    if not train:
        assert calls['halo_gemm_rows_ce'] == 1 and calls['halo_gemm_split_ce'] == 0, calls
        return
    if C // H == 64:
        assert calls['halo_attention_bwd_b16'] > 0, calls
    else:
        assert calls['halo_attention_bwd_bf16'] > 0 and calls['halo_attention_bwd_b16'] == 0, calls
    if V % 32 == 0:                     # logits kept as bf16 by the CE epilogue; their gradient made in place
        assert res['logits'] == torch.bfloat16 and calls['halo_gemm_rows_ce'] == 1 and calls['halo_gemm_split_ce'] == 0, (res['logits'], calls)
    else:                               # the lm_head's backward on halo_gemm_rows needs K = V % 32 == 0: the fp32-logits path
        assert res['logits'] == torch.float32 and calls['halo_gemm_rows_ce'] == 0 and calls['halo_gemm_split_ce'] == 1, (res['logits'], calls)


@pytest.fixture(scope='module')
def bf16_lib():
    from haloop_amd import _lib
    _lib.lib()
    _lib.lend_scratch(256 << 20)
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16')
    yield _lib
    _lib.set_math_mode(prev)


@pytest.fixture(scope='module', params=list(CONFIGS))
def case(request, bf16_lib):
    from haloop_amd import attention
    cid = request.param
    C, H, L, V = CONFIGS[cid]
    ref = oracle_result(cid)
    model = attention.GPT(attention.GPTConfig(block_size=T, vocab_size=V, n_layer=L, n_head=H, n_embd=C, bias=False))
    model.load_state_dict(ref['params'], strict=True)
    assert model.transformer.wte.weight is model.lm_head.weight
    case = dict(cid=cid, model=model.to(DEV), ids=ref['ids'].to(DEV), tg=ref['tg'].to(DEV), ref=ref, bounds=BOUNDS[cid], head_dim=C // H,
                done={})
    yield case
    case.clear()
    torch.cuda.empty_cache()


def default_pass(case, train):
    """The pass without forced tiles, run once per config and shared by the tests below."""
    if train not in case['done']:
        case['done'][train] = gpu_pass(case, train)
    return case['done'][train]


def check_train(case, res, what):
    ref = case['ref']
    assert abs(res['loss'] - ref['loss']) <= LOSS_ABS, (what, res['loss'], ref['loss'])
    fails = grad_failures(res['grads'], ref['grads'], case['bounds'], case['head_dim'])
    assert not fails, (what, fails[:20])


def check_score(case, res, what):
    ref = case['ref']
    valid = ref['tg'].reshape(-1) != 0
    mean = float(res['nll'][valid].double().mean())
    assert abs(mean - ref['loss']) <= LOSS_ABS, (what, mean, ref['loss'])
    fails = nll_failures(res['nll'], ref['nll'], case['bounds'])
    assert not fails, (what, fails[:20])


def test_training_step_against_the_oracle(case):
    res = default_pass(case, True)
    assert_reached(case['cid'], res, True)
    if case['cid'] == 'gpt2w':          # the lm_head's weight gradient (the preferred group) on the 256-row tiles
        assert res['calls']['halo_gemm_tn_rows_group'] > 0, res['calls']
    check_train(case, res, 'default')


def test_scoring_against_the_oracle(case):
    res = default_pass(case, False)
    assert_reached(case['cid'], res, False)
    check_score(case, res, 'default')


def test_forced_tiles_against_the_oracle(case):
    for env, train in VARIANTS[case['cid']]:
        res = gpu_pass(case, train, env)
        what = f'{env} {"training" if train else "scoring"}'
        assert_reached(case['cid'], res, train)
        if env.get('HALO_GEMM_TN_ROWS') == '1':
            assert res['calls']['halo_gemm_tn_rows_group'] > 0 and res['calls']['halo_gemm_tn_bf16_group'] == 0, (what, res['calls'])
        (check_train if train else check_score)(case, res, what)


def test_the_gates_have_teeth(case):
    """The comparisons above reject one wrong tile: one 256-row block of the lm_head gradient halved (a lost K-slice of
    halo_gemm_tn_rows_group), one 256-token block of the NLL shifted by twice the per-block bound (a wrong CE row tile)."""
    bounds = case['bounds']
    tr, sc = default_pass(case, True), default_pass(case, False)
    assert_reached(case['cid'], tr, True)
    assert_reached(case['cid'], sc, False)
    grads = dict(tr['grads'])
    assert not grad_failures(grads, case['ref']['grads'], bounds, case['head_dim'])
    head = grads['transformer.wte.weight'].clone()
    head[TILE:2 * TILE] *= 0.5
    grads['transformer.wte.weight'] = head
    fails = grad_failures(grads, case['ref']['grads'], bounds, case['head_dim'])
    assert any('transformer.wte.weight: rows 256..' in f for f in fails), fails
    assert all(f.startswith('transformer.wte.weight:') and (': rows' not in f or ': rows 256..' in f) for f in fails), fails
    nll = sc['nll'].clone()
    assert not nll_failures(nll, case['ref']['nll'], bounds)
    nll[2 * TILE:3 * TILE] += 2 * bounds['nll_block']
    fails = nll_failures(nll, case['ref']['nll'], bounds)
    assert any(f.startswith('nll block 2 ') for f in fails), fails
    assert not [f for f in fails if f.startswith('nll block') and not f.startswith('nll block 2 ')], fails
