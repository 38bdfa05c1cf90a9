#!/usr/bin/env python3
"""Generate the g14_* fixtures under tests/golden/ by running the REFERENCE's rotary audio encoders on the CPU.

Run where the reference is checked out (REFERENCE_ROOT, default /root/reference); it does not exist on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_rotary.py

The reference builds its rotary blocks from flash_attn.modules.mha.MHA (ha/attention.py:155-167), which needs a GPU build of flash_attn.
Before ha.attention is imported, a stand-in module of that name is registered: Wqkv and out_proj Linears around
out_proj(SDPA(rotate_interleaved(q), rotate_interleaved(k), v, dropout_p, is_causal)), with the reference's OWN
ha.transformer.rotate_interleaved -- what the reference's tests/test_flash_compat.py pins the flash_attn module to.  Everything else
(StridingAudioEncoder / AudioEncoder, Block, MLP, LayerNorm, the convolutions, TemporalClassifier) is the reference itself, in eval().
Only data (config, expected outputs, key lists) is written; parameters and inputs are regenerated from the seed by tests/rotary_ref.py.
"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.environ.get('REFERENCE_ROOT', '/root/reference'))
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class MHA(nn.Module):
    """Stand-in for flash_attn.modules.mha.MHA as ha/attention.py constructs it (self-attention, interleaved rotary over the whole head)."""

    def __init__(self, embed_dim, num_heads, cross_attn=False, qkv_proj_bias=True, out_proj_bias=True, dropout=0.0, causal=False,
                 rotary_emb_dim=0, rotary_emb_interleaved=False, use_flash_attn=False):
        super().__init__()
        assert not cross_attn and rotary_emb_interleaved and rotary_emb_dim == embed_dim // num_heads
        self.num_heads, self.dropout, self.causal = num_heads, dropout, causal
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim, bias=qkv_proj_bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=out_proj_bias)

    def forward(self, x):
        from ha.transformer import rotate_interleaved
        B, T, C = x.shape
        q, k, v = (t.view(B, T, self.num_heads, C // self.num_heads).transpose(1, 2) for t in self.Wqkv(x).split(C, dim=2))
        y = F.scaled_dot_product_attention(rotate_interleaved(q), rotate_interleaved(k), v,
                                           dropout_p=self.dropout if self.training else 0.0, is_causal=self.causal)
        return self.out_proj(y.transpose(1, 2).reshape(B, T, C))


for name in ('flash_attn', 'flash_attn.modules', 'flash_attn.modules.mha'):
    sys.modules[name] = types.ModuleType(name)
sys.modules['flash_attn.modules.mha'].MHA = MHA

import ha.attention, ha.attention_audio, ha.init, ha.recognizer   # the reference

import rotary_ref

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def case(name):
    kind, d_input, d_conv, n_embd, n_head, n_layer, bias, strides, vocab, B, T, S, seed = rotary_ref.CASES[name]
    if kind == 'striding':
        cfg = ha.init.StridingAudioEncoderConfig(block_size=-1, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bias,
                                                 d_input=d_input, d_conv=d_conv, conv_strides=strides, rotary_emb_dim=n_embd // n_head)
        enc = ha.attention_audio.StridingAudioEncoder(cfg).eval()
    else:
        cfg = ha.init.AudioEncoderConfig(block_size=-1, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bias,
                                         d_input=d_input, rotary_emb_dim=n_embd // n_head)
        enc = ha.attention_audio.AudioEncoder(cfg).eval()
    enc.load_state_dict(rotary_ref.make_params(name), strict=True)
    rec = ha.recognizer.TemporalClassifier(feat_dim=n_embd, vocab_size=vocab).eval()
    rec_p, x, il, tg, tl = rotary_ref.make_head_and_batch(name)
    rec.load_state_dict(rec_p)
    feats, flen, stats = enc(x, il)
    feats.retain_grad()
    loss, _ = rec(feats, tg, flen, tl)
    loss.backward()
    d = {'cfg': np.array([d_input, d_conv, n_embd, n_head, n_layer, int(bias), vocab, B, T, S, seed] + list(strides)),
         'keys': np.array(sorted(enc.state_dict())), 'feats': feats.detach().numpy(), 'flen': flen.numpy(), 'loss': loss.detach().numpy(),
         'dfeats': feats.grad.numpy()}
    grads = {('grad.' + k): v.grad for k, v in enc.named_parameters()}
    grads.update({('recgrad.' + k): v.grad for k, v in rec.named_parameters()})
    for k, v in grads.items():
        if v.numel() <= 4096:
            d[k] = v.numpy()
        else:
            d['norm.' + k] = np.array(float(v.double().norm()))
            d['slice.' + k] = v.reshape(-1)[::97].numpy().copy()
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **d)
    print(name, 'loss', float(loss), 'flen', flen.tolist(), 'T\'', feats.shape[1])


if __name__ == '__main__':
    for name in rotary_ref.FIXTURES:
        case(name)
