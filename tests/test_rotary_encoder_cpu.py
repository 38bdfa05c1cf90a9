"""CPU-side checks of the rotary GPT-block audio encoders (haloop_amd.attention_audio.StridingAudioEncoder, AudioEncoder with a rotary
config): construction, the reference's state-dict names, lengths, what is still refused -- and tests/rotary_ref.py, the CPU restatement
the GPU tests compare against, pinned to the reference-generated fixtures g14_* (tests/golden/make_golden_rotary.py)."""
import numpy as np
import pytest
import torch

import rotary_ref
from conftest import load_golden

NAMES = list(rotary_ref.FIXTURES)


build = rotary_ref.build


@pytest.mark.parametrize('name', NAMES)
def test_rotary_encoders_construct_with_the_reference_names(name):
    g = load_golden(name)
    enc = build(name)
    assert sorted(enc.state_dict()) == list(g['keys'])
    assert not any('wpe' in k or 'inv_freq' in k for k in enc.state_dict())
    want = rotary_ref.make_params(name)
    assert all(tuple(enc.state_dict()[k].shape) == tuple(want[k].shape) for k in want)
    _, _, il, _, _ = rotary_ref.make_head_and_batch(name)
    flen = enc.subsampled_lengths(il)
    assert flen.dtype == torch.int32 and np.array_equal(flen.numpy(), g['flen'])
    # flash_attn's MHA carries a non-persistent rotary_emb.inv_freq: present as a buffer, ignored in a checkpoint that has it
    blk = enc.transformer.h[0]
    assert blk.attn.rotary_emb.inv_freq.shape == (enc.config.n_embd // enc.config.n_head // 2,)
    sd = dict(enc.state_dict())
    sd['transformer.h.1.attn.rotary_emb.inv_freq'] = torch.zeros(3)
    enc.load_state_dict(sd, strict=True)
    # the block forms read the two Linears under the non-rotary names: the same modules, registered once
    assert blk.attn.c_attn is blk.attn.Wqkv and blk.attn.c_proj is blk.attn.out_proj
    assert len(list(blk.attn.parameters())) == (4 if enc.config.bias else 2)


def test_what_is_still_refused():
    from haloop_amd import attention, attention_audio, lora
    with pytest.raises(NotImplementedError):                                  # a partial rotation
        attention.Block(attention.GPTConfig(n_layer=1, n_head=2, n_embd=128, rotary_emb_dim=32))
    with pytest.raises(NotImplementedError):
        attention_audio.AudioEncoder(attention.GPTConfig(block_size=64, n_layer=1, n_head=2, n_embd=64, causal=False, d_input=20, rotary_emb_dim=64))
    with pytest.raises(NotImplementedError):
        attention_audio.StridingAudioEncoder(attention.StridingAudioEncoderConfig(n_layer=1, n_head=2, n_embd=64, d_input=20, rotary_emb_dim=64))
    with pytest.raises(AssertionError):                                       # as the reference: StridingAudioEncoder asserts a rotary config
        attention_audio.StridingAudioEncoder(attention.StridingAudioEncoderConfig(n_layer=1, n_head=2, n_embd=64, rotary_emb_dim=0))
    for rot in (32, 64):                                                      # GPT with any rotary_emb_dim (64 is its head dimension here)
        with pytest.raises(NotImplementedError):
            attention.GPT(attention.GPTConfig(block_size=16, vocab_size=32, n_layer=1, n_head=2, n_embd=128, rotary_emb_dim=rot))
    enc = build('g14_audio_rotary_bias')
    with pytest.raises(NotImplementedError):                                  # LoRA on a rotary block
        lora.attach_to_c_attn(enc)
    # a rotary block with a KV cache: refused before any launch
    cfg = enc.config
    with pytest.raises(NotImplementedError):
        attention.block_forward(None, enc.transformer.h[0], None, 1, 4, cfg, kv=(None, None, 0))
    with pytest.raises(Exception):
        enc(torch.zeros(1, 16, 20), torch.tensor([16]))                       # CPU tensors: no CPU path


@pytest.mark.parametrize('name', NAMES)
def test_restatement_matches_reference(name):
    """tests/rotary_ref.py == the reference (its encoders around the stand-in MHA) on features, lengths, loss and every gradient, at the
    tolerances tests/test_oracle_golden.py holds the g7_* restatement to."""
    g = load_golden(name)
    feats, flen, loss, dfeats, grads, rec_grads = rotary_ref.loss_and_grads(name)
    assert flen.dtype == torch.int32 and np.array_equal(flen.numpy(), g['flen'])
    np.testing.assert_allclose(feats.numpy(), g['feats'], atol=1e-5)
    np.testing.assert_allclose(float(loss), float(g['loss']), rtol=1e-5)
    np.testing.assert_allclose(dfeats.numpy(), g['dfeats'], rtol=1e-4, atol=1e-6)
    named = [('grad.' + k, v) for k, v in grads.items()] + [('recgrad.' + k, v) for k, v in rec_grads.items()]
    assert len(named) == sum(1 for k in g if k.startswith(('grad.', 'recgrad.', 'norm.')))
    for key, v in named:
        if key in g:
            np.testing.assert_allclose(v.numpy(), g[key], rtol=1e-3, atol=1e-6, err_msg=key)
        else:
            np.testing.assert_allclose(float(v.double().norm()), float(g['norm.' + key]), rtol=1e-4, err_msg=key)
            np.testing.assert_allclose(v.reshape(-1)[::97].numpy(), g['slice.' + key], rtol=1e-3, atol=1e-6, err_msg=key)
