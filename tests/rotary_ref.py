"""CPU restatement of the reference's rotary GPT-block audio encoders (ha/attention_audio.py: StridingAudioEncoder, and AudioEncoder with
rotary_emb_dim = head_dim) on stock torch ops.  TEST INFRASTRUCTURE ONLY.

    striding: x [B, T, F] -> gelu(conv) per (separable) layer of ConvEncoder -> dropout -> blocks -> ln_f
    audio:    x [B, T, F] -> gelu(conv_pre) -> gelu(conv_subsample, stride 2)  -> dropout -> blocks -> ln_f      (no positions added)
    block (ha/attention.py:171-180 with the flash_attn MHA as the reference's tests/test_flash_compat.py pins it):
        x += out_proj(SDPA(rotate_interleaved(q), rotate_interleaved(k), v))       q | k | v = Wqkv(ln_1(x)); NO dropout behind out_proj
        x += dropout(mlp(ln_2(x)))                                                  new_gelu
Functional form over a parameter dict keyed by the reference's state-dict names.  Pinned against the imported reference (with a stand-in
flash_attn MHA) by tests/golden/g14_*.npz, see tests/golden/make_golden_rotary.py.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import audio_encoder_ref, cpu_ref
from oracle.transformer_ref import conv_encoder, rotate_interleaved, subsampled_lengths


def new_gelu(x):
    """The tanh form with the cube as a pow, as ha/attention.py:12-17 evaluates it (x * x * x rounds differently in the last bit)."""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


# name -> (kind, d_input, d_conv, n_embd, n_head, n_layer, bias, strides, vocab, B, T, S, seed)
CASES = {
    'g14_striding_tiny': ('striding', 20, 32, 128, 2, 2, False, (2, 2, 1), 11, 3, 50, 4, 141),
    'g14_audio_rotary_bias': ('audio', 20, 0, 64, 2, 2, True, (), 11, 3, 37, 4, 142),
    # no fixture: B * T' = 25600 rows, the smallest count at which the row-major block forms take C = 128 (tests/test_gpu_rotary_encoder.py)
    'rows_threshold': ('striding', 20, 32, 128, 2, 1, False, (1, 1), 11, 64, 400, 4, 143),
}
FIXTURES = ('g14_audio_rotary_bias', 'g14_striding_tiny')


def make_params(name):
    """The encoder's parameters of a case, regenerated from its seed."""
    kind, d_input, d_conv, C, n_head, n_layer, bias, strides, vocab, B, T, S, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)

    def n(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    p = OrderedDict()
    if kind == 'striding':
        p['conv.0.weight'] = n((d_conv, d_input, 3), 1.0 / math.sqrt(3 * d_input))
        p['conv.0.bias'] = n((d_conv,), 0.05)
        for i in range(1, len(strides)):
            out = C if i == len(strides) - 1 else d_conv
            p[f'conv.{i}.depthwise.weight'] = n((d_conv, 1, 3), 1.0 / math.sqrt(3))
            p[f'conv.{i}.depthwise.bias'] = n((d_conv,), 0.05)
            p[f'conv.{i}.pointwise.weight'] = n((out, d_conv, 1), 1.0 / math.sqrt(d_conv))
            p[f'conv.{i}.pointwise.bias'] = n((out,), 0.05)
    else:
        p['conv_pre.weight'] = n((C, d_input, 3), 1.0 / math.sqrt(3 * d_input))
        p['conv_pre.bias'] = n((C,), 0.05)
        p['conv_subsample.weight'] = n((C, C, 3), 1.0 / math.sqrt(3 * C))
        p['conv_subsample.bias'] = n((C,), 0.05)
    for i in range(n_layer):
        pre = f'transformer.h.{i}.'
        p[pre + 'ln_1.weight'] = 1.0 + n((C,), 0.1)
        if bias: p[pre + 'ln_1.bias'] = n((C,), 0.05)
        p[pre + 'attn.Wqkv.weight'] = n((3 * C, C), 1.0 / math.sqrt(C))
        if bias: p[pre + 'attn.Wqkv.bias'] = n((3 * C,), 0.05)
        p[pre + 'attn.out_proj.weight'] = n((C, C), 0.5 / math.sqrt(C))
        if bias: p[pre + 'attn.out_proj.bias'] = n((C,), 0.05)
        p[pre + 'ln_2.weight'] = 1.0 + n((C,), 0.1)
        if bias: p[pre + 'ln_2.bias'] = n((C,), 0.05)
        p[pre + 'mlp.c_fc.weight'] = n((4 * C, C), 1.0 / math.sqrt(C))
        if bias: p[pre + 'mlp.c_fc.bias'] = n((4 * C,), 0.05)
        p[pre + 'mlp.c_proj.weight'] = n((C, 4 * C), 0.5 / math.sqrt(4 * C))
        if bias: p[pre + 'mlp.c_proj.bias'] = n((C,), 0.05)
    p['transformer.ln_f.weight'] = 1.0 + n((C,), 0.1)
    if bias: p['transformer.ln_f.bias'] = n((C,), 0.05)
    return p


def make_head_and_batch(name):
    """The CTC head's parameters and the seeded batch (ragged lengths T, T - 5, T - 10, ...) of a case."""
    kind, d_input, d_conv, C, n_head, n_layer, bias, strides, vocab, B, T, S, seed = CASES[name]
    return audio_encoder_ref.make_head_and_batch(C, vocab, d_input, B, T, S, seed)


def lengths(name, input_lengths):
    kind, strides = CASES[name][0], CASES[name][7]
    return subsampled_lengths(input_lengths, strides) if kind == 'striding' else audio_encoder_ref.subsampled_lengths(input_lengths)


def block(p, pre, y, n_head, rotary=True, att_mask=None, res_mask=None, mlp_mask=None):
    """One block on y [B, T, C] (ha/attention.py:171-180); ``rotary`` False: the non-rotary block under the same parameter names."""
    B, T, C = y.shape
    h = F.layer_norm(y, (C,), p[pre + 'ln_1.weight'], p.get(pre + 'ln_1.bias'), 1e-5)
    qkv = F.linear(h, p[pre + 'attn.Wqkv.weight'], p.get(pre + 'attn.Wqkv.bias'))
    q, k, v = (t.view(B, T, n_head, C // n_head).transpose(1, 2) for t in qkv.split(C, dim=2))
    if rotary:
        q, k = rotate_interleaved(q), rotate_interleaved(k)
    if att_mask is not None:
        sc = (q @ k.transpose(-2, -1)) / math.sqrt(k.shape[-1])
        a = (sc.softmax(-1) * att_mask) @ v
    else:
        a = F.scaled_dot_product_attention(q, k, v, is_causal=False)
    a = a.transpose(1, 2).contiguous().view(B, T, C)
    r = F.linear(a, p[pre + 'attn.out_proj.weight'], p.get(pre + 'attn.out_proj.bias'))
    y = y + (r * res_mask if res_mask is not None else r)
    h = F.layer_norm(y, (C,), p[pre + 'ln_2.weight'], p.get(pre + 'ln_2.bias'), 1e-5)
    h = new_gelu(F.linear(h, p[pre + 'mlp.c_fc.weight'], p.get(pre + 'mlp.c_fc.bias')))
    m = F.linear(h, p[pre + 'mlp.c_proj.weight'], p.get(pre + 'mlp.c_proj.bias'))
    return y + (m * mlp_mask if mlp_mask is not None else m)


def forward(name, p, x, input_lengths, masks=None, res_masks=None, rotary=True):
    """-> (features [B, T', C], lengths int32).  masks (training-mode parity): {'emb': [B,T',C], 'att': [per layer [B,H,T',T']], 'mlp': [...]}
    inverted-dropout multipliers.  ``res_masks`` (per layer [B,T',C]) multiplies the out_proj output, which the reference does NOT do:
    only for showing that a test can tell.  ``rotary`` False: the same encoder around non-rotary blocks."""
    kind, d_input, d_conv, C, n_head, n_layer, bias, strides, *_ = CASES[name]
    if kind == 'striding':
        y = conv_encoder(p, '', x.mT, strides).mT
    else:
        y = F.gelu(F.conv1d(x.mT, p['conv_pre.weight'], p['conv_pre.bias'], stride=1, padding=1))
        y = F.gelu(F.conv1d(y, p['conv_subsample.weight'], p['conv_subsample.bias'], stride=2, padding=1)).mT
    if masks:
        y = y * masks['emb']
    for i in range(n_layer):
        y = block(p, f'transformer.h.{i}.', y, n_head, rotary, att_mask=masks['att'][i] if masks else None,
                  res_mask=res_masks[i] if res_masks else None, mlp_mask=masks['mlp'][i] if masks else None)
    y = F.layer_norm(y, (C,), p['transformer.ln_f.weight'], p.get('transformer.ln_f.bias'), 1e-5)
    return y, lengths(name, input_lengths)


def philox_masks(name, B, T, P, seed):
    """The Philox masks of one training forward at offset 0, in the encoders' site layout: 64 the front dropout; per block i 65 + 3i the
    attention probabilities, 66 + 3i the c_proj site (DRAWN, NOT APPLIED by a rotary block: returned apart, as ``res``), 67 + 3i the MLP."""
    from oracle import philox
    kind, d_input, d_conv, C, n_head, n_layer, *_ = CASES[name]
    rows = lambda sid: torch.from_numpy(philox.dropout_mask(B * T * C, P, seed, sid, 0)).view(B, T, C)
    masks, res = {'emb': rows(64), 'att': [], 'mlp': []}, []
    for i in range(n_layer):
        masks['att'].append(torch.from_numpy(philox.attention_dropout_mask(B, n_head, T, T, P, seed, 65 + 3 * i, 0).copy()))
        res.append(rows(66 + 3 * i))
        masks['mlp'].append(rows(67 + 3 * i))
    return masks, res


def loss_and_grads(name, masks=None, res_masks=None, rotary=True):
    """The whole CPU step of a case: -> (features, lengths, loss, dfeats, {encoder name: grad}, {head name: grad})."""
    p = {k: v.clone().requires_grad_(True) for k, v in make_params(name).items()}
    rec_p, x, il, tg, tl = make_head_and_batch(name)
    rec_p = {k: v.clone().requires_grad_(True) for k, v in rec_p.items()}
    feats, flen = forward(name, p, x, il, masks, res_masks, rotary)
    feats.retain_grad()
    loss, _ = cpu_ref.classifier_loss(rec_p, feats, tg, flen, tl)
    loss.backward()
    return feats.detach(), flen, loss.detach(), feats.grad, {k: v.grad for k, v in p.items()}, {k: v.grad for k, v in rec_p.items()}


def build(name, dropout=0.0):
    """The haloop_amd encoder of a fixture's config, its parameters loaded (strict)."""
    from haloop_amd import attention, attention_audio
    kind, d_input, d_conv, n_embd, n_head, n_layer, bias, strides, vocab, B, T, S, seed = CASES[name]
    if kind == 'striding':
        cfg = attention.StridingAudioEncoderConfig(block_size=-1, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bias,
                                                   d_input=d_input, d_conv=d_conv, conv_strides=strides, rotary_emb_dim=n_embd // n_head,
                                                   dropout=dropout)
        enc = attention_audio.StridingAudioEncoder(cfg)
    else:
        cfg = attention.AudioEncoderConfig(block_size=-1, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bias,
                                           d_input=d_input, rotary_emb_dim=n_embd // n_head, dropout=dropout)
        enc = attention_audio.AudioEncoder(cfg)
    enc.load_state_dict(make_params(name), strict=True)
    return enc
