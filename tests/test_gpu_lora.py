"""LoRA on the GPT path (haloop_amd/lora.py, csrc/lora.hip) on the MI355X: the fixtures written by the reference (ha.attention.GPT + ha.lora)
in the `f32` / `bf16x3` modes -- the general path composed from the dense operators -- and the row-major `bf16` path at B = 8, T = 1024
(M = 8192 rows), where the halo_lora_* kernels run, against the fp32 CPU oracle.  With dropout off the oracle is the base model fed
c_attn.weight = W + s B A (tests/test_lora_cpu.py pins that to the reference); under dropout this file restates the adapted forward on
stock torch ops (adapted_forward) with the Philox masks of oracle/philox.py.  Every test counts the libhalo entry points it claims to run.

Gates of the fast path (FAST): loss within 2e-2 abs, every adapter gradient's norm within 5 % and cosine >= 0.995 (BASELINE's bf16 gates,
as tests/test_gpu_gpt_rows_oracle.py applies them), and its relative error (Frobenius) under REL_BOUND = 2e-2 -- about twice the worst
measured on an MI355X (worst layer of each model; the last row with lora_dropout = 0.1 on the (768, 12, 2, 2048) model):
                       lora_A.weight   lora_B.weight   norm off by   cosine
    gpt2w r = 4        1.01e-2         9.6e-3          <= 2.2e-3     >= 0.99994
    gpt2w r = 16       1.04e-2         9.9e-3          <= 1.3e-3     >= 0.99994
    hd32  r = 4        8.9e-3          8.3e-3          <= 1.1e-3     >= 0.99996
    hd32  r = 16       8.8e-3          8.7e-3          <= 1.0e-3     >= 0.99996
    dropout r = 4      1.05e-2         9.6e-3          <= 6e-4       >= 0.99994
(the error is that of the bf16 base model -- the c_attn gradient blocks of test_gpu_gpt_rows_oracle.py sit at 1.4e-2 -- not of the rank-16
products.)  Against the dropout-free oracle the dropout run is off by 6e-2 .. 3e-1: the masks are seen.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_gpt_rows_oracle import counted
from test_lora_cpu import FIXTURES, build_model, load_fixture, merged_params, oracle_eval_nll, oracle_train

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, T = 8, 1024
M = B * T
ALPHA = 32
FAST = {'gpt2w': (768, 12, 2, 50304), 'hd32': (512, 16, 1, 2048)}       # (C, heads, layers, vocab)
DROP_CFG = (768, 12, 2, 2048)
LOSS_ABS, NORM_REL, COS_MIN = 2e-2, 0.05, 0.995
REL_BOUND = {'lora_A.weight': 2e-2, 'lora_B.weight': 2e-2}
SEED = 0xFEEDFACE12345
LORA = ('halo_lora_pack', 'halo_lora_down', 'halo_lora_up', 'halo_lora_tn')
ENTRIES = LORA + ('halo_gemm_f32', 'halo_gemm_rows', 'halo_gemm_rows_ce', 'halo_gemm_tn_rows_group', 'halo_gemm_tn_bf16_group', 'halo_gemm_split',
                  'halo_dropout_fwd', 'halo_adamw_multi', 'halo_embed_bwd', 'halo_layernorm_bwd', 'halo_layernorm_bwd_bf16', 'halo_layernorm_bwd_b16')
MODE_TOL = {'f32': dict(rtol=5e-4, atol=5e-7), 'bf16x3': dict(rtol=2e-3, atol=4e-6)}


@pytest.fixture(scope='module')
def halo():
    from haloop_amd import _lib
    _lib.lib()
    _lib.lend_scratch(256 << 20)
    return _lib


@pytest.fixture
def bf16(halo):
    prev = halo.get_math_mode()
    halo.set_math_mode('bf16')
    yield
    halo.set_math_mode(prev)


@pytest.fixture
def math_mode(request, halo):
    prev = halo.get_math_mode()
    halo.set_math_mode(request.param)
    yield request.param
    halo.set_math_mode(prev)


MODES2 = pytest.mark.parametrize('math_mode', ['f32', 'bf16x3'], indirect=True)
MODES3 = pytest.mark.parametrize('math_mode', ['f32', 'bf16x3', 'bf16'], indirect=True)


def with_threads(fn, *a, **kw):
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        return fn(*a, **kw)
    finally:
        torch.set_num_threads(threads)


def adapted_forward(params, n_layer, n_head, inputs, targets, scaling, lmasks, masks=None, reduction='mean'):
    """oracle.gpt_ref.gpt_forward_all's block loop with the adapter term written out: qkv += s * lora_B(lora_A(lmask * h)).  lmasks[i]: the
    [B, T, C] inverted-dropout multipliers of block i's adapter input; masks: those of the existing sites, as gpt_ref takes them."""
    from oracle import gpt_ref
    p = params
    Bn, Tn = inputs.shape
    C = p['transformer.wte.weight'].shape[1]
    x = F.embedding(inputs, p['transformer.wte.weight']) + p['transformer.wpe.weight'][:Tn][None]
    if masks:
        x = x * masks['emb']
    for i in range(n_layer):
        pre = f'transformer.h.{i}.'
        h = F.layer_norm(x, (C,), p[pre + 'ln_1.weight'], p.get(pre + 'ln_1.bias'), 1e-5)
        qkv = F.linear(h, p[pre + 'attn.c_attn.weight'], p.get(pre + 'attn.c_attn.bias'))
        u = F.linear(h * lmasks[i], p[pre + 'attn.c_attn.lora_A.weight'], p.get(pre + 'attn.c_attn.lora_A.bias'))
        qkv = qkv + scaling * F.linear(u, p[pre + 'attn.c_attn.lora_B.weight'], p.get(pre + 'attn.c_attn.lora_B.bias'))
        q, k, v = (t.view(Bn, Tn, n_head, C // n_head).transpose(1, 2) for t in qkv.split(C, dim=2))
        if masks:
            sc = (q @ k.transpose(-2, -1)) / math.sqrt(k.shape[-1])
            sc = sc.masked_fill(~torch.ones(Tn, Tn, dtype=torch.bool).tril(), float('-inf'))
            y = (sc.softmax(-1) * masks['att'][i]) @ v
        else:
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        r = F.linear(y.transpose(1, 2).contiguous().view(Bn, Tn, C), p[pre + 'attn.c_proj.weight'], p.get(pre + 'attn.c_proj.bias'))
        x = x + (r * masks['res'][i] if masks else r)
        h = F.layer_norm(x, (C,), p[pre + 'ln_2.weight'], p.get(pre + 'ln_2.bias'), 1e-5)
        m = F.linear(gpt_ref.new_gelu(F.linear(h, p[pre + 'mlp.c_fc.weight'], p.get(pre + 'mlp.c_fc.bias'))), p[pre + 'mlp.c_proj.weight'],
                     p.get(pre + 'mlp.c_proj.bias'))
        x = x + (m * masks['mlp'][i] if masks else m)
    x = F.layer_norm(x, (C,), p['transformer.ln_f.weight'], p.get('transformer.ln_f.bias'), 1e-5)
    logits = F.linear(x, p['transformer.wte.weight'])
    return F.cross_entropy(logits.view(-1, logits.size(-1)), targets.reshape(-1), ignore_index=0, reduction=reduction)


def adapted_train(params, n_layer, n_head, inputs, targets, scaling, lmasks, masks=None):
    leaves = {k: (v.clone().requires_grad_(True) if 'lora_' in k else v) for k, v in params.items()}
    loss = adapted_forward(leaves, n_layer, n_head, inputs, targets, scaling, lmasks, masks)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in leaves.items() if 'lora_' in k}


def lora_masks(n_layer, Bn, Tn, C, p, seed, offset=0):
    from oracle import philox
    return [torch.from_numpy(philox.dropout_mask(Bn * Tn * C, p, seed, 4096 + i, offset)).view(Bn, Tn, C) for i in range(n_layer)]


def train_pass(model, ids, tg):
    """One training forward + backward -> (loss, adapter gradients, the calls it made); every frozen parameter must end without a gradient."""
    model.train()
    for p in model.parameters():
        p.grad = None
    with counted(ENTRIES) as calls:
        loss = model.forward_all(ids, tg)
        loss.backward()
        torch.cuda.synchronize()
    grads = {}
    for n, p in model.named_parameters():
        if p.requires_grad:
            grads[n] = p.grad.detach().cpu()
        else:
            assert p.grad is None, n
    return float(loss.detach()), grads, dict(calls)


def fixture_model(fx, **kw):
    return build_model(fx, **kw).to(DEV)


# ---- 1. the fixtures, general path ---------------------------------------------------------------------------------------------------
@MODES2
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_training_step_matches_the_reference(halo, name, math_mode):
    fx = load_fixture(name)
    g = fx['g']
    model = fixture_model(fx)
    loss, grads, calls = train_pass(model, fx['inputs'].to(DEV), fx['targets'].to(DEV))
    assert calls['halo_gemm_f32'] > 0 and all(calls[n] == 0 for n in LORA), calls            # composed from the dense operators
    np.testing.assert_allclose(loss, float(g['loss']), rtol=2e-5)
    assert sorted(grads) == sorted(str(k) for k in g['trainable'])
    for k, v in grads.items():
        np.testing.assert_allclose(v.numpy(), g['grad.' + k], err_msg=k, **MODE_TOL[math_mode])


# ---- 2. eval merge, and the merge after optimizer steps ------------------------------------------------------------------------------
@MODES2
@pytest.mark.parametrize('name', FIXTURES)
def test_eval_merge_scores_like_the_reference_also_after_adamw_steps(halo, name, math_mode):
    from haloop_amd import ops
    fx = load_fixture(name)
    g = fx['g']
    model = fixture_model(fx).eval()
    ids, tg = fx['inputs'].to(DEV), fx['targets'].to(DEV)
    with torch.no_grad(), counted(ENTRIES) as calls:
        nll = model.forward_all(ids, tg, reduction='none')
    assert all(calls[n] == 0 for n in LORA) and all(blk.attn.c_attn.merged for blk in model.transformer.h), calls
    np.testing.assert_allclose(nll.cpu().numpy(), g['per_token'], rtol=2e-5, atol=2e-5)
    model.train()
    adapters = [p for p in model.parameters() if p.requires_grad]
    opt = ops.AdamWMulti(adapters, [0.0] * len(adapters), lr=1e-2, betas=(0.9, 0.95))
    with counted(ENTRIES) as calls:
        for _ in range(3):
            for p in adapters:
                p.grad = None
            model.forward_all(ids, tg).backward()
            opt.step()
    assert calls['halo_adamw_multi'] == 3, calls
    model.eval()
    with torch.no_grad():
        nll = model.forward_all(ids, tg, reduction='none')
    now = dict(fx['params'], **{n: p.detach().cpu() for n, p in model.named_parameters() if p.requires_grad})
    assert not torch.equal(now['transformer.h.0.attn.c_attn.lora_A.weight'], fx['params']['transformer.h.0.attn.c_attn.lora_A.weight'])
    want = oracle_eval_nll(now, fx['n_layer'], fx['n_head'], fx['inputs'], fx['targets'], fx['scaling'])
    np.testing.assert_allclose(nll.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)             # a stale operand image fails this


# ---- 3. unmerged inference through the KV cache --------------------------------------------------------------------------------------
@MODES2
def test_unmerged_generation_matches_the_merged_model(halo, math_mode):
    """train() mode under no_grad: the adapter is added at the c_attn site of _trunk.  The unmerged logits of a prompt + 3 cached steps
    against the merged eval() model's, and both against the fp32 CPU oracle fed c_attn.weight = W + s B A (oracle.gpt_ref.gpt_forward),
    all at the mode's generation tolerance (tests/test_gpu_parity.py, test_gpt_kv_cache_generation_matches_reference)."""
    from oracle import gpt_ref
    fx = load_fixture('g12_gpt_lora_nobias')
    model = fixture_model(fx)
    ids = fx['inputs'].to(DEV)
    split = fx['T'] // 2
    spans = ((0, split), (split, split + 1), (split + 1, split + 2), (split + 2, split + 3))

    def run():
        with torch.no_grad():
            out, past = [], None
            for lo, hi in spans:
                logits, past = model(ids[:, lo:hi], past=past)
                out.append(logits.cpu())
        return out
    model.train()
    with counted(ENTRIES) as calls:
        unmerged = run()
    assert calls['halo_gemm_f32'] > 0 and not model.transformer.h[0].attn.c_attn.merged, calls
    model.eval()
    assert model.transformer.h[0].attn.c_attn.merged
    merged = run()
    p = merged_params(fx['params'], fx['n_layer'], fx['scaling'], merged_eval=True)
    want, past = [], None
    with torch.no_grad():
        for lo, hi in spans:
            logits, past = gpt_ref.gpt_forward(p, fx['n_layer'], fx['n_head'], fx['inputs'][:, lo:hi], past)
            want.append(logits)
    tol = dict(rtol=2e-5, atol=1e-5 if math_mode == 'f32' else 1e-4)
    for a, b, w in zip(unmerged, merged, want):
        print(f'{math_mode}: max abs unmerged - merged {float((a - b).abs().max()):.3e}, unmerged - oracle {float((a - w).abs().max()):.3e}, '
              f'merged - oracle {float((b - w).abs().max()):.3e}')
        np.testing.assert_allclose(a.numpy(), b.numpy(), **tol)
        np.testing.assert_allclose(a.numpy(), w.numpy(), **tol)
        np.testing.assert_allclose(b.numpy(), w.numpy(), **tol)


# ---- 4. B = 0 is a no-op -------------------------------------------------------------------------------------------------------------
def _fresh_attach_is_a_noop(model, ids, tg):
    from haloop_amd import lora
    for p in model.parameters():
        p.requires_grad_(True)
    model.eval()
    with torch.no_grad():
        nll0 = model.forward_all(ids, tg, reduction='none').cpu()
    model.train()
    loss0 = model.forward_all(ids, tg).detach().cpu()
    lora.attach_to_c_attn(model, r=4, lora_alpha=ALPHA, lora_dropout=0.0)
    lora.mark_only_lora_as_trainable_(model)
    loss1, grads, calls = train_pass(model, ids, tg)
    assert loss1 == float(loss0), (loss1, float(loss0))
    with torch.no_grad():                                       # unmerged, train() mode: the adapter site runs and adds exact zeros
        nll_unmerged = model.forward_all(ids, tg, reduction='none').cpu()
    model.eval()
    with torch.no_grad():
        nll_merged = model.forward_all(ids, tg, reduction='none').cpu()
    assert torch.equal(nll_unmerged, nll0) and torch.equal(nll_merged, nll0)
    for n, gr in grads.items():
        if n.endswith('lora_B.weight'):
            assert float(gr.abs().max()) > 0, n
        else:
            assert not gr.any(), n                                # d lora_A = (s dqkv B)^T h with B = 0
    return calls


@MODES3
def test_fresh_adapters_change_no_bit_fixture(halo, math_mode):
    from haloop_amd import attention
    fx = load_fixture('g12_gpt_lora_nobias')
    model = attention.GPT(attention.GPTConfig(block_size=fx['block'], vocab_size=fx['vocab'], n_layer=fx['n_layer'], n_head=fx['n_head'],
                                              n_embd=fx['n_embd'], bias=False))
    model.load_state_dict({k: v for k, v in fx['params'].items() if 'lora_' not in k}, strict=True)
    calls = _fresh_attach_is_a_noop(model.to(DEV), fx['inputs'].to(DEV), fx['targets'].to(DEV))
    assert calls['halo_gemm_f32'] > 0, calls


def test_fresh_adapters_change_no_bit_fast_path(halo):
    from haloop_amd import attention
    from oracle import gpt_ref
    C, H, L, V = DROP_CFG
    prev = halo.get_math_mode()
    halo.set_math_mode('bf16')
    try:
        model = attention.GPT(attention.GPTConfig(block_size=T, vocab_size=V, n_layer=L, n_head=H, n_embd=C, bias=False))
        model.load_state_dict(gpt_ref.make_gpt_params(V, T, L, H, C, False, seed=17), strict=True)
        ids, tg = gpt_ref.synthetic_tokens(B, T, V, seed=18)
        calls = _fresh_attach_is_a_noop(model.to(DEV), ids.to(DEV), tg.to(DEV))
        assert all(calls[n] > 0 for n in LORA), calls
    finally:
        halo.set_math_mode(prev)


# ---- 5. - 8. the fast path against the oracle ----------------------------------------------------------------------------------------
def big_params(C, H, L, V, r, seed=17):
    from oracle import gpt_ref
    params = gpt_ref.make_gpt_params(V, T, L, H, C, False, seed=seed)
    g = torch.Generator().manual_seed(seed + 2)
    for i in range(L):
        pre = f'transformer.h.{i}.attn.c_attn.'
        params[pre + 'lora_A.weight'] = (torch.rand(r, C, generator=g) * 2 - 1) / math.sqrt(C)        # nn.Linear's own init range
        params[pre + 'lora_B.weight'] = torch.randn(3 * C, r, generator=g) * 0.02                      # non-zero: A's gradient exists
    ids, tg = gpt_ref.synthetic_tokens(B, T, V, seed=seed + 1)
    return params, ids, tg


def big_model(params, C, H, L, V, r, lora_dropout=0.0):
    from haloop_amd import attention, lora
    model = attention.GPT(attention.GPTConfig(block_size=T, vocab_size=V, n_layer=L, n_head=H, n_embd=C, bias=False))
    lora.attach_to_c_attn(model, r=r, lora_alpha=ALPHA, lora_dropout=lora_dropout)
    lora.mark_only_lora_as_trainable_(model)
    model.load_state_dict(params, strict=True)
    return model.to(DEV)


def grad_stats(got, want):
    g, w = got.double().flatten(), want.double().flatten()
    ng, nw = float(g.norm()), float(w.norm())
    return dict(norm=abs(ng - nw) / nw, cos=float((g * w).sum()) / (ng * nw), rel=float((g - w).norm()) / nw)


def failures(loss, grads, ref_loss, ref_grads):
    fails = []
    if abs(loss - ref_loss) > LOSS_ABS:
        fails.append(f'loss {loss} against {ref_loss}')
    for name, w in ref_grads.items():
        st = grad_stats(grads[name], w)
        kind = name.split('c_attn.')[1]
        print(f'{name}: norm {st["norm"]:.3e} cos {st["cos"]:.6f} rel {st["rel"]:.3e}')
        if st['norm'] > NORM_REL:
            fails.append(f'{name}: norm off by {st["norm"]:.3e}')
        if st['cos'] < COS_MIN:
            fails.append(f'{name}: cosine {st["cos"]:.5f}')
        if st['rel'] > REL_BOUND[kind]:
            fails.append(f'{name}: relative error {st["rel"]:.3e} > {REL_BOUND[kind]:.1e}')
    return fails


def assert_fast_launches(model, calls):
    from haloop_amd import attention
    cfg = model.config
    assert attention.rowmajor_train_ok(cfg, model.transformer.h, M, True) and attention.rows_ok(M, cfg.n_embd)
    assert all(calls[n] > 0 for n in LORA[1:]), calls                                                  # (halo_lora_pack: only when A / B changed)
    assert calls['halo_gemm_tn_rows_group'] == 0 and calls['halo_gemm_tn_bf16_group'] == 0, calls      # no base weight gradient
    assert calls['halo_gemm_rows_ce'] == 1 and calls['halo_embed_bwd'] == 0, calls
    L = cfg.n_layer                                             # the lowest block stops at its adapters: no layernorm_bwd of its ln_1
    n_ln = calls['halo_layernorm_bwd'] + calls['halo_layernorm_bwd_bf16'] + calls['halo_layernorm_bwd_b16']
    assert n_ln == 2 * L, calls                                 # ln_f + ln_2 of every block + ln_1 of all but the lowest


@pytest.fixture(scope='module', params=[(cid, r) for cid in FAST for r in (4, 16)], ids=lambda p: f'{p[0]}-r{p[1]}')
def fast_case(request, halo):
    cid, r = request.param
    C, H, L, V = FAST[cid]
    prev = halo.get_math_mode()
    halo.set_math_mode('bf16')
    params, ids, tg = big_params(C, H, L, V, r)
    ref_loss, ref_grads = with_threads(oracle_train, params, L, H, ids, tg, ALPHA / r)
    model = big_model(params, C, H, L, V, r)
    try:
        loss, grads, calls = train_pass(model, ids.to(DEV), tg.to(DEV))
    finally:
        halo.set_math_mode(prev)                                # (the tests below take the mode from the `bf16` fixture)
    yield dict(cid=cid, r=r, model=model, ids=ids.to(DEV), tg=tg.to(DEV), ref_loss=ref_loss, ref_grads=ref_grads, loss=loss, grads=grads,
               calls=calls)
    del model
    torch.cuda.empty_cache()


def test_fast_path_training_step_against_the_oracle(fast_case, bf16):
    c = fast_case
    assert_fast_launches(c['model'], c['calls'])
    fails = failures(c['loss'], c['grads'], c['ref_loss'], c['ref_grads'])
    assert not fails, fails


def test_fast_path_is_deterministic(fast_case, bf16):
    c = fast_case
    loss, grads, calls = train_pass(c['model'], c['ids'], c['tg'])
    assert_fast_launches(c['model'], calls)
    assert calls['halo_lora_pack'] == 0, calls                  # A and B did not change: the packed operands were cached
    assert loss == c['loss']
    for n, g in grads.items():
        assert torch.equal(g, c['grads'][n]), n


def test_fast_path_scores_unmerged_like_merged(fast_case, bf16):
    """Scoring in train() mode (no dropout configured): _trunk_rows adds the adapter with halo_lora_down / _up; against the merged eval()
    model, both GPU results in single-pass bf16 arithmetic: the mean NLL within the loss gate."""
    c = fast_case
    model = c['model']
    model.train()
    with torch.no_grad(), counted(ENTRIES) as calls:
        un = model.forward_all(c['ids'], c['tg'], reduction='none')
    assert calls['halo_lora_down'] > 0 and calls['halo_lora_up'] > 0 and calls['halo_lora_tn'] == 0 and calls['halo_gemm_rows_ce'] == 1, calls
    model.eval()
    with torch.no_grad():
        me = model.forward_all(c['ids'], c['tg'], reduction='none')
    model.train()
    valid = c['tg'].reshape(-1) != 0
    assert abs(float(un[valid].double().mean()) - float(me[valid].double().mean())) <= LOSS_ABS
    assert abs(float(un[valid].double().mean()) - c['ref_loss']) <= LOSS_ABS


def test_the_gates_have_teeth(fast_case, bf16):
    c = fast_case
    assert not failures(c['loss'], c['grads'], c['ref_loss'], c['ref_grads'])
    scaling = ALPHA / c['r']
    nameB = 'transformer.h.0.attn.c_attn.lora_B.weight'
    bad = dict(c['grads'])
    bad[nameB] = bad[nameB] / scaling                           # a lost scaling factor
    fails = failures(c['loss'], bad, c['ref_loss'], c['ref_grads'])
    assert fails and all(f.startswith(nameB) for f in fails), fails
    if c['model'].config.n_layer > 1:                           # one adapter's gradient swapped for the other layer's
        other = 'transformer.h.1.attn.c_attn.lora_A.weight'
        nameA = 'transformer.h.0.attn.c_attn.lora_A.weight'
        bad = dict(c['grads'])
        bad[nameA], bad[other] = bad[other], bad[nameA]
        fails = failures(c['loss'], bad, c['ref_loss'], c['ref_grads'])
        assert any(f.startswith(nameA) for f in fails) and any(f.startswith(other) for f in fails), fails


# ---- 6. dropout, same masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_restated_forward_equals_the_merged_oracle_without_masks(name):
    fx = load_fixture(name)
    ones = [torch.ones(fx['B'], fx['T'], fx['n_embd'])] * fx['n_layer']
    loss, grads = adapted_train(fx['params'], fx['n_layer'], fx['n_head'], fx['inputs'], fx['targets'], fx['scaling'], ones)
    want, want_grads = oracle_train(fx['params'], fx['n_layer'], fx['n_head'], fx['inputs'], fx['targets'], fx['scaling'])
    np.testing.assert_allclose(loss, want, rtol=2e-5)
    for k, v in want_grads.items():
        assert float((grads[k] - v).norm() / v.norm()) <= 2e-5, k


@MODES2
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_lora_dropout_matches_restated_forward_with_same_masks(halo, name, math_mode):
    fx = load_fixture(name)
    P = 0.1
    model = fixture_model(fx, lora_dropout=P)
    model.dropout_stream.seed = SEED
    loss, grads, calls = train_pass(model, fx['inputs'].to(DEV), fx['targets'].to(DEV))
    assert calls['halo_dropout_fwd'] > 0 and model.dropout_stream.offset == 1, calls
    lm = lora_masks(fx['n_layer'], fx['B'], fx['T'], fx['n_embd'], P, SEED)
    want, want_grads = adapted_train(fx['params'], fx['n_layer'], fx['n_head'], fx['inputs'], fx['targets'], fx['scaling'], lm)
    np.testing.assert_allclose(loss, want, rtol=2e-5)
    for k, v in want_grads.items():
        np.testing.assert_allclose(grads[k].numpy(), v.numpy(), err_msg=k, **MODE_TOL[math_mode])


@MODES2
def test_existing_dropout_sites_keep_their_ids_next_to_the_adapter_sites(halo, math_mode):
    """config.dropout = 0.1 and lora_dropout = 0.1: the existing sites still draw ids 64.. at offset 0, the adapters 4096 + layer."""
    from oracle import philox
    fx = load_fixture('g12_gpt_lora_nobias')
    P = 0.1
    model = fixture_model(fx, lora_dropout=P, dropout=P)
    model.dropout_stream.seed = SEED
    loss, grads, calls = train_pass(model, fx['inputs'].to(DEV), fx['targets'].to(DEV))
    assert model.dropout_stream.offset == 1
    Bn, Tn, C, H, L = fx['B'], fx['T'], fx['n_embd'], fx['n_head'], fx['n_layer']
    rows = lambda sid: torch.from_numpy(philox.dropout_mask(Bn * Tn * C, P, SEED, sid, 0)).view(Bn, Tn, C)
    masks = {'emb': rows(64), 'att': [], 'res': [], 'mlp': []}
    for i in range(L):
        masks['att'].append(torch.from_numpy(philox.attention_dropout_mask(Bn, H, Tn, Tn, P, SEED, 65 + 3 * i, 0).copy()))
        masks['res'].append(rows(66 + 3 * i))
        masks['mlp'].append(rows(67 + 3 * i))
    lm = lora_masks(L, Bn, Tn, C, P, SEED)
    want, want_grads = adapted_train(fx['params'], L, H, fx['inputs'], fx['targets'], fx['scaling'], lm, masks)
    np.testing.assert_allclose(loss, want, rtol=2e-5)
    for k, v in want_grads.items():
        np.testing.assert_allclose(grads[k].numpy(), v.numpy(), err_msg=k, **MODE_TOL[math_mode])


def test_fast_path_lora_dropout_matches_restated_forward_with_same_masks(halo):
    C, H, L, V = DROP_CFG
    P, r = 0.1, 4
    prev = halo.get_math_mode()
    halo.set_math_mode('bf16')
    try:
        params, ids, tg = big_params(C, H, L, V, r)
        model = big_model(params, C, H, L, V, r, lora_dropout=P)
        model.dropout_stream.seed = SEED
        loss, grads, calls = train_pass(model, ids.to(DEV), tg.to(DEV))
        assert_fast_launches(model, calls)
        assert calls['halo_dropout_fwd'] == 0 and model.dropout_stream.offset == 1, calls          # the masks are drawn inside halo_lora_*
        lm = lora_masks(L, B, T, C, P, SEED)
        want, want_grads = with_threads(adapted_train, params, L, H, ids, tg, ALPHA / r, lm)
        fails = failures(loss, grads, want, want_grads)
        assert not fails, fails
        # ... and the masks matter: the dropout-free oracle is not what the GPU computed
        _, nodrop = with_threads(oracle_train, params, L, H, ids, tg, ALPHA / r)
        assert failures(loss, grads, want, nodrop)
    finally:
        halo.set_math_mode(prev)


def test_rank_above_16_takes_the_general_path(halo):
    """r = 32 in bf16 mode at M = 8192: rowmajor_train_ok closes and the adapter is composed from the dense operators."""
    from haloop_amd import attention
    C, H, L, V = 256, 4, 1, 512
    prev = halo.get_math_mode()
    halo.set_math_mode('bf16')
    try:
        params, ids, tg = big_params(C, H, L, V, 32)
        model = big_model(params, C, H, L, V, 32)
        assert not attention.rowmajor_train_ok(model.config, model.transformer.h, M, True)
        loss, grads, calls = train_pass(model, ids.to(DEV), tg.to(DEV))
        assert calls['halo_gemm_f32'] > 0 and all(calls[n] == 0 for n in LORA), calls
        want, want_grads = with_threads(oracle_train, params, L, H, ids, tg, ALPHA / 32)
        assert abs(loss - want) <= LOSS_ABS
        for k, v in want_grads.items():
            st = grad_stats(grads[k], v)
            assert st['norm'] <= NORM_REL and st['cos'] >= COS_MIN, (k, st)
    finally:
        halo.set_math_mode(prev)


# ---- the module on its own, and the audio encoder's blocks ---------------------------------------------------------------------------
@pytest.mark.parametrize('bias', [False, True])
def test_linear_module_forward_on_its_own(halo, bias):
    from haloop_amd import lora
    torch.manual_seed(5)
    lin = lora.Linear(64, 192, r=4, lora_alpha=32, lora_dropout=0.1, bias=bias)
    with torch.no_grad():
        lin.lora_B.weight.normal_(0, 0.05)
    x = torch.randn(3, 7, 64)
    want = F.linear(x, lin.weight, lin.bias) + lin.scaling * lin.lora_B(lin.lora_A(x))
    lin = lin.to(DEV)
    with pytest.raises(NotImplementedError):
        lin(x.to(DEV))                                          # under autograd: training goes through GPT.forward_all
    with torch.no_grad(), counted(ENTRIES) as calls:
        got = lin(x.to(DEV))
    assert calls['halo_gemm_f32'] == 3, calls
    np.testing.assert_allclose(got.cpu().numpy(), want.detach().numpy(), rtol=2e-5, atol=2e-6)
    lin.eval()                                                  # merged: one product
    with torch.no_grad(), counted(ENTRIES) as calls:
        got = lin(x.to(DEV))
    assert calls['halo_gemm_f32'] == 1, calls
    if not bias:                                                # (with bias=True the merge drops the adapter Linears' own biases, as the reference)
        np.testing.assert_allclose(got.cpu().numpy(), want.detach().numpy(), rtol=2e-5, atol=2e-6)


@MODES2
def test_audio_encoder_blocks_take_the_adapters(halo, math_mode):
    """Same Block as the GPT: unmerged (train() mode) features equal the merged (eval()) ones at the mode's tolerance of the GPT generation
    test above (LayerNorm'd features of order 1, like logits); the autograd path returns the same features and leaves gradients on the
    adapters only."""
    from haloop_amd import attention, attention_audio, lora
    torch.manual_seed(7)
    cfg = attention.GPTConfig(block_size=64, vocab_size=11, n_layer=2, n_head=2, n_embd=64, bias=True, causal=False, d_input=20, rotary_emb_dim=0)
    enc = attention_audio.AudioEncoder(cfg)
    lora.attach_to_c_attn(enc, lora_dropout=0.0)
    lora.mark_only_lora_as_trainable_(enc)
    with torch.no_grad():
        for blk in enc.transformer.h:
            blk.attn.c_attn.lora_B.weight.normal_(0, 0.05)
            blk.attn.c_attn.lora_A.bias.zero_(); blk.attn.c_attn.lora_B.bias.zero_()       # (the merge ignores them)
    enc = enc.to(DEV).train()
    x, il = torch.randn(3, 41, 20).to(DEV), torch.tensor([41, 30, 17]).to(DEV)
    with torch.no_grad():
        unmerged, _, _ = enc(x, il)
    feats, _, _ = enc(x, il)
    feats.square().mean().backward()
    torch.cuda.synchronize()
    # (the two paths differ only in which launch applies GELU and the residual add: fp32 rounding)
    np.testing.assert_allclose(feats.detach().cpu().numpy(), unmerged.cpu().numpy(), rtol=1e-5, atol=1e-5)
    for n, p in enc.named_parameters():
        assert (p.grad is not None and bool(p.grad.any())) == ('lora_' in n), n
    enc.eval()
    with torch.no_grad():
        merged, _, _ = enc(x, il)
    np.testing.assert_allclose(unmerged.cpu().numpy(), merged.cpu().numpy(), rtol=2e-5, atol=1e-5 if math_mode == 'f32' else 1e-4)
