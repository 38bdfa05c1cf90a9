"""haloop_amd.lora without a GPU: the fixtures written by the reference (tests/golden/make_golden_lora.py: ha.attention.GPT + ha.lora, only the
adapters trainable) against the CPU oracle, and the module surgery / merge bookkeeping of haloop_amd.lora on CPU tensors.

The oracle needs no LoRA code: with dropout off the adapted model IS the base model with c_attn.weight = W + s B A (and, unmerged with
bias=True, c_attn.bias = b + s (B a + b_B) for the adapter Linears' own biases a, b_B; the merged eval model ignores them, as the
reference does), so oracle.gpt_ref.gpt_forward_all fed that sum with A and B as autograd leaves gives the loss and the adapter gradients.
tests/test_gpu_lora.py uses the helpers below for its references.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

FIXTURES = ['g12_gpt_lora_nobias', 'g12_gpt_lora_bias']


def load_fixture(name):
    g = load_golden(name)
    vocab, block, n_layer, n_head, n_embd, bias, B, T, seed = (int(v) for v in g['cfg'])
    params = {k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')}
    return dict(g=g, vocab=vocab, block=block, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bool(bias), B=B, T=T, r=int(g['r']),
                alpha=int(g['alpha']), scaling=int(g['alpha']) / int(g['r']), params=params, inputs=torch.from_numpy(g['inputs']),
                targets=torch.from_numpy(g['targets']))


def merged_params(params, n_layer, scaling, merged_eval=False):
    """The base-model parameter dict of the adapted model: c_attn.weight = W + s B A; the adapter biases enter c_attn.bias unless
    ``merged_eval`` (the reference's merge leaves them out).  Differentiable in whatever lora_* entries are autograd leaves."""
    p = {k: v for k, v in params.items() if 'lora_' not in k}
    for i in range(n_layer):
        pre = f'transformer.h.{i}.attn.c_attn.'
        A, Bm = params[pre + 'lora_A.weight'], params[pre + 'lora_B.weight']
        p[pre + 'weight'] = params[pre + 'weight'] + scaling * (Bm @ A)
        if pre + 'lora_A.bias' in params and not merged_eval:
            p[pre + 'bias'] = params[pre + 'bias'] + scaling * (Bm @ params[pre + 'lora_A.bias'] + params[pre + 'lora_B.bias'])
    p['lm_head.weight'] = p['transformer.wte.weight']
    return p


def oracle_train(params, n_layer, n_head, inputs, targets, scaling):
    """-> (mean loss, {adapter parameter name: gradient}) of the unmerged model with dropout off."""
    from oracle import gpt_ref
    leaves = {k: (v.clone().requires_grad_(True) if 'lora_' in k else v) for k, v in params.items()}
    loss = gpt_ref.gpt_forward_all(merged_params(leaves, n_layer, scaling), n_layer, n_head, inputs, targets)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in leaves.items() if 'lora_' in k}


def oracle_eval_nll(params, n_layer, n_head, inputs, targets, scaling):
    from oracle import gpt_ref
    with torch.no_grad():
        return gpt_ref.gpt_forward_all(merged_params(params, n_layer, scaling, merged_eval=True), n_layer, n_head, inputs, targets, reduction='none')


def build_model(fx, lora_dropout=0.0, dropout=0.0):
    """haloop_amd.attention.GPT with adapters attached as `hala --lora` does, the fixture's parameters loaded (on the CPU)."""
    from haloop_amd import attention, lora
    model = attention.GPT(attention.GPTConfig(block_size=fx['block'], vocab_size=fx['vocab'], n_layer=fx['n_layer'], n_head=fx['n_head'],
                                              n_embd=fx['n_embd'], bias=fx['bias'], dropout=dropout))
    lora.attach_to_c_attn(model, r=fx['r'], lora_alpha=fx['alpha'], lora_dropout=lora_dropout)
    lora.mark_only_lora_as_trainable_(model)
    model.load_state_dict(fx['params'], strict=True)
    return model


@pytest.mark.parametrize('name', FIXTURES)
def test_merged_weight_oracle_reproduces_the_reference(name):
    fx = load_fixture(name)
    g = fx['g']
    loss, grads = oracle_train(fx['params'], fx['n_layer'], fx['n_head'], fx['inputs'], fx['targets'], fx['scaling'])
    np.testing.assert_allclose(loss, float(g['loss']), rtol=2e-5)
    assert sorted(grads) == sorted(str(k) for k in g['trainable'])
    for k, v in grads.items():
        want = g['grad.' + k]
        assert float(np.linalg.norm(want)) > 0, k
        assert float((v - torch.from_numpy(want)).norm() / np.linalg.norm(want)) <= 2e-5, k
    nll = oracle_eval_nll(fx['params'], fx['n_layer'], fx['n_head'], fx['inputs'], fx['targets'], fx['scaling'])
    np.testing.assert_allclose(nll.numpy(), g['per_token'], rtol=2e-5)
    pre = 'transformer.h.0.attn.c_attn.'
    np.testing.assert_allclose(merged_params(fx['params'], fx['n_layer'], fx['scaling'])[pre + 'weight'].numpy(), g['merged.' + pre + 'weight'],
                               rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize('name', FIXTURES)
def test_attach_gives_the_reference_state_dict_and_trainable_set(name):
    from haloop_amd import attention, lora
    fx = load_fixture(name)
    g = fx['g']
    model = attention.GPT(attention.GPTConfig(block_size=fx['block'], vocab_size=fx['vocab'], n_layer=fx['n_layer'], n_head=fx['n_head'],
                                              n_embd=fx['n_embd'], bias=fx['bias']))
    before = [(blk.attn.c_attn.weight, blk.attn.c_attn.bias) for blk in model.transformer.h]
    lora.attach_to_c_attn(model, r=fx['r'], lora_alpha=fx['alpha'])
    for (w, b), blk in zip(before, model.transformer.h):
        lin = blk.attn.c_attn
        assert isinstance(lin, lora.Linear) and lin.weight is w and lin.bias is b              # shared, not copied
        assert lin.r == fx['r'] and lin.scaling == fx['scaling'] and lin.lora_dropout_p == 0.1 and not lin.merged
        assert not lin.lora_B.weight.any() and lin.lora_A.weight.any()
        assert (lin.lora_A.bias is not None) == fx['bias'] and (lin.lora_B.bias is not None) == fx['bias']
    lora.mark_only_lora_as_trainable_(model)
    assert sorted(model.state_dict()) == [str(k) for k in g['keys']]
    assert [n for n, p in model.named_parameters() if p.requires_grad] == [str(k) for k in g['trainable']]
    model.load_state_dict(fx['params'], strict=True)
    assert model.transformer.wte.weight is model.lm_head.weight


def test_attach_works_on_the_audio_encoder():
    from haloop_amd import attention, attention_audio, lora
    cfg = attention.GPTConfig(block_size=64, vocab_size=11, n_layer=2, n_head=2, n_embd=64, bias=True, causal=False, d_input=20, rotary_emb_dim=0)
    enc = attention_audio.AudioEncoder(cfg)
    lora.attach_to_c_attn(enc)
    lora.mark_only_lora_as_trainable_(enc)
    assert all(isinstance(blk.attn.c_attn, lora.Linear) for blk in enc.transformer.h)
    assert all(('lora_' in n) == p.requires_grad for n, p in enc.named_parameters())


@pytest.mark.parametrize('name', FIXTURES)
def test_eval_train_eval_merges_through_the_version_counter(name):
    fx = load_fixture(name)
    model = build_model(fx)
    lin = model.transformer.h[0].attn.c_attn
    W = lin.weight.detach().clone()
    want = torch.from_numpy(fx['g']['merged.transformer.h.0.attn.c_attn.weight'])
    versions = [lin.weight._version]
    for mode in (False, True, False):
        model.train(mode)
        versions.append(lin.weight._version)
        assert lin.merged == (not mode)
        np.testing.assert_allclose(lin.weight.detach().numpy(), (W if mode else want).numpy(), rtol=0, atol=2e-6)
    assert versions == sorted(set(versions)), versions                      # strictly growing: cached operand images are rebuilt
    model.eval()                                                            # merging twice must not add twice
    np.testing.assert_allclose(lin.weight.detach().numpy(), want.numpy(), rtol=0, atol=2e-6)
    if fx['bias']:
        assert torch.equal(lin.bias, fx['params']['transformer.h.0.attn.c_attn.bias'])      # the merge leaves the biases alone


def test_linear_refuses_cpu_tensors():
    from haloop_amd import _lib, lora
    lin = lora.Linear(64, 192, r=4, lora_alpha=32, bias=False)
    with pytest.raises(_lib.HaloError):
        lin(torch.randn(3, 64))
