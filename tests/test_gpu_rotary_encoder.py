"""GPU parity of the rotary GPT-block audio encoders (haloop_amd.attention_audio.StridingAudioEncoder, AudioEncoder with a rotary config)
and of the rotary block in the row-major bf16 forms.

* `f32` / `bf16x3`: the reference-generated fixtures g14_* (tests/golden/make_golden_rotary.py), inference and autograd path, with the
  rotation on halo_rope_rows and (HALO_ROPE_ROWS=0) on the scalar operator, at the tolerances of tests/test_gpu_audio_encoder.py; and
  training-mode dropout against tests/rotary_ref.py fed the restated Philox masks.
* `bf16`: the fp32 restatement is the reference, and the yardstick is the NON-rotary block in the same form, at the same shape and weights
  (code that does not run the rotation): max-abs error over the RMS of the reference, for the output and every gradient.  The rotary
  block must stay within 2x of it: the rotation preserves norms and adds one bf16 rounding to q and k, on top of the one the c_attn
  product's output already has.  Each test prints both figures."""
import functools

import numpy as np
import pytest
import torch

import rotary_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture
def math_mode(request):
    from haloop_amd import _lib
    _lib.lib(); _lib.lend_scratch()
    prev = _lib.get_math_mode()
    _lib.set_math_mode(request.param)
    yield request.param
    _lib.set_math_mode(prev)


BOTH_MODES = pytest.mark.parametrize('math_mode', ['f32', 'bf16x3'], indirect=True)
BF16 = pytest.mark.parametrize('math_mode', ['bf16'], indirect=True)


def _head(name):
    from haloop_amd import recognizer
    C, vocab = rotary_ref.CASES[name][3], rotary_ref.CASES[name][8]
    rec_p, x, il, tg, tl = rotary_ref.make_head_and_batch(name)
    rec = recognizer.TemporalClassifier(C, vocab)
    rec.load_state_dict(rec_p)
    return rec.to(DEV), (x, il, tg, tl)


@BOTH_MODES
@pytest.mark.parametrize('rope_rows', ['1', '0'])
@pytest.mark.parametrize('name', rotary_ref.FIXTURES)
def test_rotary_encoder_matches_reference(name, rope_rows, math_mode, monkeypatch):
    monkeypatch.setenv('HALO_ROPE_ROWS', rope_rows)
    g = load_golden(name)
    enc = rotary_ref.build(name).to(DEV).eval()
    rec, (x, il, tg, tl) = _head(name)
    rec.eval()
    with torch.no_grad():                                                     # inference path
        f0, l0, stats = enc(x.to(DEV), il.to(DEV), measure_entropy=True)
    assert stats == {} and l0.dtype == torch.int32 and np.array_equal(l0.cpu().numpy(), g['flen'])
    np.testing.assert_allclose(f0.cpu().numpy(), g['feats'], atol=1e-4)
    feats, flen, _ = enc(x.to(DEV), il.to(DEV))                               # autograd path
    feats.retain_grad()
    np.testing.assert_allclose(feats.detach().cpu().numpy(), g['feats'], atol=1e-4)
    loss, _ = rec(feats, tg.to(DEV), flen, tl.to(DEV))
    np.testing.assert_allclose(loss.item(), float(g['loss']), rtol=1e-5)
    loss.backward()
    np.testing.assert_allclose(feats.grad.cpu().numpy(), g['dfeats'], rtol=1e-3, atol=1e-6)
    named = [('grad.' + k, p) for k, p in enc.named_parameters()] + [('recgrad.' + k, p) for k, p in rec.named_parameters()]
    for key, p in named:
        got = p.grad.cpu().numpy()
        if key in g:
            np.testing.assert_allclose(got, g[key], rtol=2e-3, atol=2e-6 + 1e-4 * np.abs(g[key]).max(), err_msg=key)
        else:
            np.testing.assert_allclose(float(np.sqrt((got.astype(np.float64) ** 2).sum())), float(g['norm.' + key]), rtol=2e-4, err_msg=key)
            ref = g['slice.' + key]
            np.testing.assert_allclose(got.reshape(-1)[::97], ref, rtol=2e-3, atol=2e-6 + 1e-4 * np.abs(ref).max(), err_msg=key)


P_DROP, SEED = 0.1, 0xFEEDFACE54321


@functools.lru_cache(maxsize=None)
def _dropout_reference(with_res):
    """The CPU step of g14_striding_tiny under the restated Philox masks; ``with_res``: the c_proj site (66 + 3i) applied too, which a rotary
    block does NOT do."""
    name = 'g14_striding_tiny'
    B, Tp = rotary_ref.CASES[name][9], int(load_golden(name)['feats'].shape[1])
    masks, res = rotary_ref.philox_masks(name, B, Tp, P_DROP, SEED)
    return rotary_ref.loss_and_grads(name, masks, res if with_res else None)


@BOTH_MODES
def test_training_mode_dropout_matches_restatement_with_same_masks(math_mode):
    """config.dropout = 0.1, .train(): sites 64 (front dropout), 65 + 3i (attention probabilities), 67 + 3i (MLP output); 66 + 3i is drawn
    and not applied (flash MHA has no dropout behind out_proj)."""
    name = 'g14_striding_tiny'
    enc = rotary_ref.build(name, dropout=P_DROP).to(DEV).train()
    rec, (x, il, tg, tl) = _head(name)
    rec.eval()
    enc.dropout_stream.seed = SEED
    feats, flen, _ = enc(x.to(DEV), il.to(DEV))
    loss, _ = rec(feats, tg.to(DEV), flen, tl.to(DEV))
    loss.backward()
    f_ref, _, loss_ref, _, grads_ref, _ = _dropout_reference(False)
    got = feats.detach().cpu().numpy()
    np.testing.assert_allclose(got, f_ref.numpy(), atol=1e-4)
    np.testing.assert_allclose(loss.item(), float(loss_ref), rtol=1e-5)
    for k, p in enc.named_parameters():
        ref = grads_ref[k].numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-6 + 1e-4 * np.abs(ref).max(), err_msg=k)
    # the test can see the site layout: with the c_proj mask applied the restatement is another function
    f_res = _dropout_reference(True)[0].numpy()
    assert not np.allclose(got, f_res, atol=1e-2)


# ---- `bf16`: the row-major forms, against the non-rotary block in the same form --------------------------------------------------------
def _q(got, ref):
    """max-abs error over the RMS of the reference"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).abs().max() / ref.pow(2).mean().sqrt())


def _within_twice(what, rot, plain):
    print(f'{what}: rotary / non-rotary (max-abs error over RMS of the reference)')
    bad = []
    for k in rot:
        print(f'    {k:40s} {rot[k]:.3e}  {plain[k]:.3e}  ratio {rot[k] / plain[k]:.2f}')
        if not rot[k] <= 2 * plain[k]:
            bad.append(k)
    assert not bad, f'{what}: beyond twice the non-rotary block\'s error: {bad}'


BLOCK_C, BLOCK_H, BLOCK_B = 128, 2, 3
BLOCK_KEYS = ('ln_1.weight', 'attn.Wqkv.weight', 'attn.out_proj.weight', 'ln_2.weight', 'mlp.c_fc.weight', 'mlp.c_proj.weight')


@functools.lru_cache(maxsize=None)
def _block_case(T, rotary):
    """Parameters (the first block of g14_striding_tiny: C = 128, 2 heads), input, output gradient and the fp32 CPU result of one block."""
    p = {k[len('transformer.h.0.'):]: v for k, v in rotary_ref.make_params('g14_striding_tiny').items() if k.startswith('transformer.h.0.')}
    g = torch.Generator().manual_seed(150 + T)
    x, dout = torch.randn(BLOCK_B, T, BLOCK_C, generator=g), torch.randn(BLOCK_B, T, BLOCK_C, generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    y = rotary_ref.block(leaves, '', xr, BLOCK_H, rotary)
    (y * dout).sum().backward()
    return p, x, dout, dict({k: v.grad for k, v in leaves.items()}, out=y.detach(), dx=xr.grad)


def _run_block(T, rotary):
    """rows_block_forward(train=True) + block_backward_rm on one block -> the error figures against the restatement."""
    from haloop_amd import _lib, attention, ops
    from haloop_amd._linear import WeightImages, training_images
    p, x, dout, ref = _block_case(T, rotary)
    hd = BLOCK_C // BLOCK_H
    cfg = attention.GPTConfig(block_size=T, n_layer=1, n_head=BLOCK_H, n_embd=BLOCK_C, bias=False, causal=False, rotary_emb_dim=hd if rotary else 0)
    blk = attention.Block(cfg)
    blk.load_state_dict({(k if rotary else k.replace('Wqkv', 'c_attn').replace('out_proj', 'c_proj')): v for k, v in p.items()}, strict=True)
    blk.to(DEV)
    M = BLOCK_B * T
    assert attention.rows_ok(M, BLOCK_C)
    _lib.lend_scratch(128 << 20, device=torch.device(DEV))
    images, grads = WeightImages(), {}

    def put(prm, g):
        if prm is not None and g is not None:
            grads[id(prm)] = g
    with torch.no_grad(), training_images():
        xd, dd = x.view(M, BLOCK_C).to(DEV), dout.view(M, BLOCK_C).to(DEV).contiguous()
        y, sv = attention.rows_block_forward(images, blk, xd, BLOCK_B, T, cfg, train=True)
        assert sv.form == attention.ROWS and sv.qkv_b16
        dx, _ = attention.block_backward_rm(images, blk, sv, dd, ops.cast_bf16(dd), BLOCK_B, T, cfg, put)
    torch.cuda.synchronize()
    named = dict(blk.named_parameters())
    out = {'out': _q(y, ref['out']), 'dx': _q(dx, ref['dx'])}
    for k in BLOCK_KEYS:
        out[k] = _q(grads[id(named[k if rotary else k.replace('Wqkv', 'c_attn').replace('out_proj', 'c_proj')])], ref[k])
    return out


# B * T must be a multiple of 32 (the weight-gradient products' contraction step); the bf16-rows attention takes any T on 64-row tiles:
# 32 is the smallest the form accepts (half a tile), 64 one whole tile, 96 a tile and a half
@BF16
@pytest.mark.parametrize('T', [32, 64, 96])
def test_bf16_rows_block_stays_within_twice_the_non_rotary_block(T, math_mode):
    _within_twice(f'block, B = {BLOCK_B}, T = {T}', _run_block(T, True), _run_block(T, False))


@functools.lru_cache(maxsize=None)
def _threshold_reference(rotary):
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    try:
        return rotary_ref.loss_and_grads('rows_threshold', rotary=rotary)
    finally:
        torch.set_num_threads(threads)


def _run_threshold(rotary):
    """The striding encoder at B * T' = 25600 rows, C = 128 (rows_threshold) in `bf16`: inference features, then the no-dropout training loss
    and gradients -> the error figures against the restatement.  ``rotary`` False: the same encoder with the rotation taken out of its
    blocks (the non-rotary block in the same row-major form)."""
    from haloop_amd import attention
    name = 'rows_threshold'
    enc = rotary_ref.build(name).to(DEV).eval()
    for blk in enc.transformer.h:
        blk.rotary = rotary
    rec, (x, il, tg, tl) = _head(name)
    rec.eval()
    f_ref, _, loss_ref, dfeats_ref, grads_ref, _ = _threshold_reference(rotary)
    with torch.no_grad():
        f0, _, _ = enc(x.to(DEV), il.to(DEV))
    assert enc.last_form == attention.ROWS                                   # rows_block_forward, scoring form
    out = {'features (inference)': _q(f0, f_ref)}
    feats, flen, _ = enc(x.to(DEV), il.to(DEV))
    assert enc.last_form == attention.ROWS                                   # block_forward_train_rm on halo_gemm_rows / block_backward_rm
    feats.retain_grad()
    loss, _ = rec(feats, tg.to(DEV), flen, tl.to(DEV))
    loss.backward()
    out['features (training)'] = _q(feats, f_ref)
    out['loss'] = abs(loss.item() - float(loss_ref)) / abs(float(loss_ref))
    out['dfeats'] = _q(feats.grad, dfeats_ref)
    for k, p in enc.named_parameters():
        out[k] = _q(p.grad, grads_ref[k])
    return out


@BF16
def test_bf16_encoder_at_the_row_major_threshold(math_mode):
    B, T = rotary_ref.CASES['rows_threshold'][9:11]
    assert B * T == 25600
    _within_twice('encoder, 25600 rows', _run_threshold(True), _run_threshold(False))
