"""The lm_head and the cross-entropy on the target rows only (GPT.set_target_capacity; csrc/sparse_head.hip): the compaction, gather and
scatter kernels bit-exact against torch.nonzero / index_select / index_copy_, and the compact path of GPT.forward_all against the dense
path of the same model and against the fp32 CPU oracle (oracle/gpt_ref.py), on batches masked by the restatement of tests/test_gpu_mlm.py.

Tiny model (f32 and bf16x3; L = 2, C = 64, H = 2, V = 97, biases, bidirectional; B = 4, T = 32, 21 targets, capacity 32, which the model
runs as 96 compact rows so that the head stays on the products the dense head runs at 128 rows): compact against
dense within rtol 1e-4, atol 1e-6 x max|ref| -- the rows' dot products are the same, only the order of the fp32 sums over rows differs
(<= 128 terms at eps 6e-8) -- and against the oracle under the tolerances tests/test_gpu_parity.py applies to the g5 tiny fixtures in
the same mode.  Capacity 16 overflows: every loss is NaN, nothing raises, and the next call within capacity is clean.

Row-tile path (`bf16` mode; L = 1, C = 512, H = 8, V = 2048, no bias, bidirectional; B = 64, T = 128: M = 8192, where rowmajor_train_ok and
rows_ok hold; the masked batch at step 3 has 1230 targets; capacity 1536): halo_gemm_rows_ce runs once at 1536 rows with bf16 logits
[1536, V].  Dense (the control) and compact, training and scoring, each against ONE oracle result under the fixed gates of
tests/test_gpu_gpt_rows_oracle.py (mean NLL within 2e-2, every gradient's norm within 5 %, cosine >= 0.995) and under per-token /
per-block bounds of about twice the worse of the two paths, measured on an MI355X -- dense | compact:
    NLL on the target rows, max abs error                          2.172e-2 | 2.172e-2       bound 4.5e-2
    every gradient, relative error of every 256-row block, worst   9.077e-3 | 9.081e-3       bound 1.8e-2
    every gradient, relative error (Frobenius), worst              8.120e-3 | 8.118e-3       bound 1.6e-2
Each run prints its worst figures.
test_the_gates_have_teeth halves one 256-row block of the compact run's wte gradient and requires the comparison to fail.
"""
import os

import numpy as np
import pytest
import torch

from test_gpu_gpt_rows_oracle import COS_MIN, LOSS_ABS, NORM_REL, counted, grad_stats
from test_gpu_mlm import SEED, masked_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEW_ENTRIES = ('halo_mask_tokens', 'halo_mlm_batch_u16', 'halo_target_rows', 'halo_gather_rows', 'halo_scatter_rows')


@pytest.fixture(scope='module')
def lib():
    from haloop_amd import _lib
    _lib.lib()
    _lib.lend_scratch(256 << 20)
    prev = _lib.get_math_mode()
    yield _lib
    _lib.set_math_mode(prev)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def _targets_with(M, count, seed):
    g = torch.Generator().manual_seed(seed)
    tg = torch.zeros(M, dtype=torch.int64)
    tg[torch.randperm(M, generator=g)[:count]] = torch.randint(1, 5000, (count,), generator=g)
    return tg


@pytest.mark.parametrize('count', [0, 1, 96, 97, 1000])
def test_compaction_gather_scatter_bit_exact(lib, count):
    """M = 1000 rows, capacity 96: no target, one, exactly the capacity, one too many, every row."""
    from haloop_amd import ops
    M, K = 1000, 96
    tg = _targets_with(M, count, 100 + count)
    rec = ops.target_rows(tg.to(DEV), K)
    assert rec.capacity == K and rec.rows.dtype == torch.int32 and rec.slot.dtype == torch.int32 and rec.targets.dtype == torch.int64
    assert int(rec.count) == count
    kept = torch.nonzero(tg).flatten()[:K]                                        # ascending row order, the first K
    n = kept.numel()
    rows, slot, tc = rec.rows.cpu().long(), rec.slot.cpu().long(), rec.targets.cpu()
    assert torch.equal(rows[:n], kept) and (rows[n:] == -1).all()
    assert torch.equal(tc[:n], tg[kept]) and (tc[n:] == 0).all()
    want_slot = torch.full((M,), -1, dtype=torch.long)
    want_slot[kept] = torch.arange(n)
    assert torch.equal(slot, want_slot)
    assert torch.equal(slot[rows[:n]], torch.arange(n)) and torch.equal(rows[slot[slot >= 0]], torch.nonzero(slot >= 0).flatten())
    g = torch.Generator().manual_seed(7)
    for C in (64, 768, 1):
        src = torch.randn(M, C, generator=g) if C > 1 else torch.randn(M, generator=g)       # C = 1: the per-token loss / gradient form
        got = ops.gather_rows(src.to(DEV), rec.rows).cpu()
        want = torch.zeros((K,) + tuple(src.shape[1:]))
        want[:n] = src.index_select(0, kept)
        assert got.shape == want.shape and torch.equal(got, want), C
        comp = torch.randn((K,) + tuple(src.shape[1:]), generator=g)
        want = torch.zeros_like(src).index_copy_(0, kept, comp[:n])
        got = ops.scatter_rows(comp.to(DEV), rec, M, nan_on_overflow=False).cpu()
        assert torch.equal(got, want), C
        got, gotb = ops.scatter_rows(comp.to(DEV), rec, M, want_bf16=True)                   # with the count: the overflow is loud
        if count > K:
            assert got.isnan().all() and gotb.isnan().all(), C
        else:
            assert torch.equal(got.cpu(), want) and torch.equal(gotb.cpu(), want.bfloat16()), C


def test_scatter_writes_every_row_of_a_nan_filled_destination(lib):
    """halo_scatter_rows into a destination pre-filled with NaN: none left (called on the C ABI, which takes the destination)."""
    from haloop_amd import ops
    from haloop_amd._lib import check, ptr
    M, K = 1000, 96
    rec = ops.target_rows(_targets_with(M, 50, 3).to(DEV), K)
    for C in (1, 64, 768):
        comp = torch.randn(K, C, device=DEV)
        dst = torch.full((M, C), float('nan'), device=DEV)
        dstb = torch.full((M, C), float('nan'), device=DEV, dtype=torch.bfloat16)
        check(lib.lib().halo_scatter_rows(ptr(comp), ptr(rec.slot), ptr(rec.count), K, K, M, C, ptr(dst), ptr(dstb), ops._stream()), 'halo_scatter_rows')
        assert not dst.isnan().any() and not dstb.isnan().any()
        assert int((dst.abs().sum(1) != 0).sum()) == 50


def test_no_host_synchronisation(lib, tmp_path):
    from haloop_amd import ops, symbol_tape
    data = torch.randint(0, 30000, (5000,), dtype=torch.int16, device=DEV)
    offsets = torch.tensor([0, 100, 4990], device=DEV)
    src = torch.randn(192, 64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        x, y = symbol_tape.get_batch(data, offsets, 64, 'denoise', seed=SEED, step=2)
        rec = ops.target_rows(y, 64)
        comp = ops.gather_rows(src, rec.rows)
        back, backb = ops.scatter_rows(comp, rec, 192, want_bf16=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    n = int((y != 0).sum())
    assert int(rec.count) == n and 0 < n <= 64           # 192 positions at p = 0.15: 29 expected, standard deviation 5
    assert torch.equal(back[y.reshape(-1) != 0], src[y.reshape(-1) != 0]) and (back[y.reshape(-1) == 0] == 0).all()


# ---- the tiny model ------------------------------------------------------------------------------------------------------------------
TINY = dict(L=2, C=64, H=2, V=97, B=4, T=32)
# tests/test_gpu_parity.py on the g5 tiny fixtures: per-token NLL, mean, gradients
ORACLE_TOL = {'f32': dict(nll=dict(rtol=2e-5, atol=2e-5), mean=1e-5, grad=dict(rtol=2e-4, atol=2e-7)),
              'bf16x3': dict(nll=dict(rtol=2e-5, atol=2e-5), mean=1e-5, grad=dict(rtol=1e-3, atol=2e-6))}


@pytest.fixture(scope='module')
def tiny_ref():
    """The oracle's result, computed once: per-token NLL, their mean over the targets and its gradients."""
    from oracle import gpt_ref
    c = TINY
    _, ids, tg, masks = masked_batch(c['B'], c['T'], c['V'], 0)
    assert int(masks['selected'].sum()) == 21
    params = gpt_ref.make_gpt_params(c['V'], c['T'], c['L'], c['H'], c['C'], bias=True, seed=17)
    weights = torch.rand(c['B'] * c['T'], generator=torch.Generator().manual_seed(5)) + 0.5
    out = dict(params=params, ids=ids, tg=tg, weights=weights)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items() if k != 'lm_head.weight'}
    p = dict(leaves, **{'lm_head.weight': leaves['transformer.wte.weight']})
    nll = gpt_ref.gpt_forward_all(p, c['L'], c['H'], ids, tg, reduction='none', causal=False)
    loss = nll.sum() / (tg != 0).sum()
    loss.backward()
    out['mean'] = dict(nll=nll.detach(), loss=float(loss.detach()), grads={k: v.grad for k, v in leaves.items()})
    return out


def _tiny_model(ref):
    from haloop_amd import attention
    c = TINY
    model = attention.GPT(attention.GPTConfig(block_size=c['T'], vocab_size=c['V'], n_layer=c['L'], n_head=c['H'], n_embd=c['C'], bias=True, causal=False))
    model.load_state_dict(ref['params'], strict=True)
    return model.to(DEV).train()


def _step(model, ids, tg, reduction='mean', weights=None):
    """forward_all + backward -> (loss or weighted sum as float, per-token losses if 'none', gradients by name)."""
    for p in model.parameters():
        p.grad = None
    out = model.forward_all(ids, tg, reduction=reduction)
    loss = out if weights is None else (out * weights).sum()
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), out.detach().cpu(), {n: p.grad.detach().cpu() for n, p in model.named_parameters()}


def _close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize('mode', ['f32', 'bf16x3'])
def test_tiny_model_compact_against_dense_and_oracle(lib, tiny_ref, mode):
    lib.set_math_mode(mode)
    ref, tol = tiny_ref, ORACLE_TOL[mode]
    model = _tiny_model(ref)
    ids, tg, weights = ref['ids'].to(DEV), ref['tg'].to(DEV), ref['weights'].to(DEV)
    off = (ref['tg'].reshape(-1) == 0)
    dense = {'mean': _step(model, ids, tg), 'sum': _step(model, ids, tg, 'sum'), 'weighted': _step(model, ids, tg, 'none', weights)}
    with torch.no_grad():
        dense['score'] = model.forward_all(ids, tg, reduction='none').cpu()
    model.set_target_capacity(32)
    with counted(NEW_ENTRIES) as calls:
        comp = {'mean': _step(model, ids, tg), 'sum': _step(model, ids, tg, 'sum'), 'weighted': _step(model, ids, tg, 'none', weights)}
        assert calls['halo_target_rows'] == 3 and calls['halo_gather_rows'] == 6 and calls['halo_scatter_rows'] == 6, calls
        with torch.no_grad():
            comp['score'] = model.forward_all(ids, tg, reduction='none').cpu()
            comp['score_mean'] = float(model.forward_all(ids, tg, reduction='mean'))
        assert calls['halo_target_rows'] == 5 and calls['halo_gather_rows'] == 8 and calls['halo_scatter_rows'] == 8, calls
    # compact against dense on the same model
    for what in ('mean', 'sum', 'weighted'):
        (ld, nd, gd), (lc, nc, gc) = dense[what], comp[what]
        assert abs(lc - ld) <= 1e-4 * abs(ld) + 1e-6, (what, lc, ld)
        if what == 'weighted':
            _close(nc, nd, 1e-4, 1e-6 * float(nd.abs().max()), 'per-token losses (training)')
            assert (nc[off] == 0).all() and (nc[~off] > 0).all()                     # exactly 0 off the targets
        for name, g in gd.items():
            _close(gc[name], g, 1e-4, 1e-6 * float(g.abs().max()), f'{what}: {name}')
    _close(comp['score'], dense['score'], 1e-4, 1e-6 * float(dense['score'].abs().max()), 'per-token losses (scoring)')
    assert (comp['score'][off] == 0).all() and (comp['score'][~off] > 0).all()
    # compact (and dense, the control) against the oracle
    for res, who in ((dense, 'dense'), (comp, 'compact')):
        _close(res['score'], ref['mean']['nll'], what=f'{who} scoring', **tol['nll'])
        _close(res['weighted'][1], ref['mean']['nll'], what=f'{who} training', **tol['nll'])
        assert abs(res['mean'][0] - ref['mean']['loss']) <= tol['mean'] * abs(ref['mean']['loss']), who
        for name, g in ref['mean']['grads'].items():
            _close(res['mean'][2][name], g, what=f'{who} mean: {name}', **tol['grad'])
    assert abs(comp['score_mean'] - ref['mean']['loss']) <= tol['mean'] * abs(ref['mean']['loss'])


def test_overflow_is_loud_and_leaves_nothing_behind(lib, tiny_ref):
    lib.set_math_mode('f32')
    ref = tiny_ref
    model = _tiny_model(ref)
    ids, tg = ref['ids'].to(DEV), ref['tg'].to(DEV)
    model.set_target_capacity(32)
    clean = _step(model, ids, tg)
    with torch.no_grad():
        clean_score = model.forward_all(ids, tg, reduction='none').cpu()
    model.set_target_capacity(16)                                                    # < 21 targets
    for reduction in ('mean', 'sum', 'none'):
        loss, out, grads = _step(model, ids, tg, reduction, None if reduction != 'none' else torch.ones(ids.numel(), device=DEV))
        assert out.isnan().all() and out.numel() == (ids.numel() if reduction == 'none' else 1), reduction
        assert not any(g.isfinite().all() for n, g in grads.items() if 'h.0.ln_1' in n), reduction     # no finite, partial gradient below
        with torch.no_grad():
            assert model.forward_all(ids, tg, reduction=reduction).isnan().all(), reduction
    model.set_target_capacity(32)
    again = _step(model, ids, tg)
    assert again[0] == clean[0]
    for n, g in clean[2].items():
        if n == 'transformer.wte.weight':       # halo_embed_bwd adds the repeated tokens' rows with float atomics: equal up to their order
            _close(again[2][n], g, 0, 1e-6 * float(g.abs().max()), n)
        else:
            assert torch.equal(again[2][n], g), n
    with torch.no_grad():
        assert torch.equal(model.forward_all(ids, tg, reduction='none').cpu(), clean_score)


def test_default_runs_none_of_the_new_launches(lib, tiny_ref):
    lib.set_math_mode('bf16x3')
    ref = tiny_ref
    model = _tiny_model(ref)
    ids, tg = ref['ids'].to(DEV), ref['tg'].to(DEV)
    assert model._target_capacity is None
    with counted(NEW_ENTRIES) as calls:
        _step(model, ids, tg)
        with torch.no_grad():
            model.forward_all(ids, tg, reduction='none')
        assert not any(calls.values()), calls
        model.set_target_capacity(32)
        _step(model, ids, tg)
        assert calls['halo_target_rows'] == 1 and calls['halo_gather_rows'] == 2 and calls['halo_scatter_rows'] == 2, calls
        model.set_target_capacity(None)
        before = dict(calls)
        _step(model, ids, tg)
        assert calls == before


# ---- the row-tile path ---------------------------------------------------------------------------------------------------------------
ROWS = dict(L=1, C=512, H=8, V=2048, B=64, T=128, capacity=1536, step=3)
# about twice the worse of the dense and the compact path against the oracle (module docstring)
ROW_BOUNDS = dict(nll_max=4.5e-2, block_rel=1.8e-2, rel=1.6e-2)


@pytest.fixture(scope='module')
def rows_case(lib):
    """One oracle result and the four GPU passes (dense | compact) x (training | scoring) it is compared with."""
    from haloop_amd import attention
    from oracle import gpt_ref
    c = ROWS
    M = c['B'] * c['T']
    _, ids, tg, masks = masked_batch(c['B'], c['T'], c['V'], c['step'])
    assert int(masks['selected'].sum()) == 1230
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        params = gpt_ref.make_gpt_params(c['V'], c['T'], c['L'], c['H'], c['C'], bias=False, seed=17)
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items() if k != 'lm_head.weight'}
        p = dict(leaves, **{'lm_head.weight': leaves['transformer.wte.weight']})
        nll = gpt_ref.gpt_forward_all(p, c['L'], c['H'], ids, tg, reduction='none', causal=False)
        loss = nll.sum() / (tg != 0).sum()
        loss.backward()
        ref = dict(nll=nll.detach(), loss=float(loss.detach()), grads={k: v.grad for k, v in leaves.items()})
    finally:
        torch.set_num_threads(threads)
    prev = lib.get_math_mode()
    lib.set_math_mode('bf16')
    cfg = attention.GPTConfig(block_size=c['T'], vocab_size=c['V'], n_layer=c['L'], n_head=c['H'], n_embd=c['C'], bias=False, causal=False)
    model = attention.GPT(cfg)
    model.load_state_dict(params, strict=True)
    model = model.to(DEV)
    assert attention.rowmajor_train_ok(cfg, model.transformer.h, M, True) and attention.rows_ok(M, c['C'])
    ids_d, tg_d = ids.to(DEV), tg.to(DEV)
    L_ = lib.lib()
    ce_rows, saved_logits = [], []
    orig_ce, fwd = L_.halo_gemm_rows_ce, model._forward_train

    def ce(*a):
        ce_rows.append(a[4])
        return orig_ce(*a)

    def keep(i, t):
        loss, saved = fwd(i, t)
        saved_logits.append((saved.logits.dtype, tuple(saved.logits.shape), saved.rec is not None))
        return loss, saved
    L_.halo_gemm_rows_ce, model._forward_train = ce, keep
    res = {}
    try:
        for who, cap in (('dense', None), ('compact', c['capacity'])):
            model.set_target_capacity(cap)
            model.train()
            loss, _, grads = _step(model, ids_d, tg_d)
            model.eval()
            with torch.inference_mode():
                score = model.forward_all(ids_d, tg_d, reduction='none').cpu()
            res[who] = dict(loss=loss, grads=grads, nll=score, ce_rows=list(ce_rows), logits=saved_logits[-1])
            ce_rows.clear()
    finally:
        L_.halo_gemm_rows_ce = orig_ce
        del model._forward_train
        lib.set_math_mode(prev)
    yield dict(ref=ref, res=res, tg=tg.reshape(-1), M=M)
    torch.cuda.empty_cache()


def row_failures(res, ref, tg, bounds, report=None):
    """The fixed gates of tests/test_gpu_gpt_rows_oracle.py and the measured bounds, for one path's training and scoring results."""
    fails = []
    valid = tg != 0
    err = (res['nll'].double() - ref['nll'].double()).abs()
    mean = float(res['nll'][valid].double().mean())
    worst = dict(nll_max=float(err[valid].max()), block_rel=0.0, rel=0.0)
    if abs(res['loss'] - ref['loss']) > LOSS_ABS or abs(mean - ref['loss']) > LOSS_ABS:
        fails.append(f'mean NLL {res["loss"]:.5f} (training) / {mean:.5f} (scoring) against {ref["loss"]:.5f}')
    if not (res['nll'][~valid] == 0).all():
        fails.append('scoring: non-zero loss on a row without a target')
    if worst['nll_max'] > bounds['nll_max']:
        fails.append(f'nll max abs error on target rows {worst["nll_max"]:.3e} > {bounds["nll_max"]:.1e}')
    for name, w in ref['grads'].items():
        g = res['grads'][name]
        st = grad_stats(name, g, w, 64)
        rel = float((g.double() - w.double()).norm() / w.double().norm())
        worst['block_rel'], worst['rel'] = max(worst['block_rel'], *st['blocks']), max(worst['rel'], rel)
        if st['norm'] > NORM_REL:
            fails.append(f'{name}: norm off by {st["norm"]:.3e}')
        if st['cos'] < COS_MIN:
            fails.append(f'{name}: cosine {st["cos"]:.5f}')
        if rel > bounds['rel']:
            fails.append(f'{name}: relative error {rel:.3e} > {bounds["rel"]:.1e}')
        for i, r in enumerate(st['blocks']):
            if r > bounds['block_rel']:
                fails.append(f'{name}: rows {i * 256}.. relative error {r:.3e} > {bounds["block_rel"]:.1e}')
    if report is not None:
        report.update(worst)
    return fails


def test_row_tile_head_runs_on_the_capacity(rows_case):
    c, res = ROWS, rows_case['res']
    # training then scoring, one halo_gemm_rows_ce each: dense at M rows, compact at the capacity
    assert res['dense']['ce_rows'] == [rows_case['M']] * 2 and res['compact']['ce_rows'] == [c['capacity']] * 2, (res['dense']['ce_rows'], res['compact']['ce_rows'])
    assert res['dense']['logits'] == (torch.bfloat16, (rows_case['M'], c['V']), False)               # the dense record carries no compaction
    assert res['compact']['logits'] == (torch.bfloat16, (c['capacity'], c['V']), True)


@pytest.mark.parametrize('who', ['dense', 'compact'])
def test_row_tile_paths_against_the_oracle(rows_case, who):
    report = {}
    fails = row_failures(rows_case['res'][who], rows_case['ref'], rows_case['tg'], ROW_BOUNDS, report)
    print(f'{who}: ' + ', '.join(f'{k} {v:.3e}' for k, v in report.items()))
    assert not fails, (who, fails[:20])


def test_the_gates_have_teeth(rows_case):
    """One 256-row block of the compact run's wte gradient halved (a lost slice of the K' = 1536 contraction would leave it so)."""
    res = dict(rows_case['res']['compact'])
    assert not row_failures(res, rows_case['ref'], rows_case['tg'], ROW_BOUNDS)
    grads = dict(res['grads'])
    head = grads['transformer.wte.weight'].clone()
    head[256:512] *= 0.5
    grads['transformer.wte.weight'] = head
    res['grads'] = grads
    fails = row_failures(res, rows_case['ref'], rows_case['tg'], ROW_BOUNDS)
    assert any('transformer.wte.weight: rows 256..' in f for f in fails), fails
    assert all(f.startswith('transformer.wte.weight:') and (': rows' not in f or ': rows 256..' in f) for f in fails), fails
