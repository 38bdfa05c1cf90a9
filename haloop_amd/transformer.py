"""Drop-in for the inference/scoring side of ha/transformer.py (encoder-decoder attention ASR, `hala`):
AudioEncoder, Block, MultiHeadAttention, Decoder (teacher-forced loss and batched greedy decode with fp16
KV caches), CTCAttentionDecoder, rotate_interleaved, attend, attend_chunked -- on the HIP
operators of csrc/attn.hip, csrc/conv.hip, csrc/gpt.hip and the GEMMs.

Same constructor arguments, attribute and state-dict names as the reference (``h.{i}.ln_time``,
``h.{i}.mix_time.{q,k,v,proj}``, ``h.{i}.mix_memory.*``, ``h.{i}.ln_chan``, ``h.{i}.mix_chan.{0,2}``, ``ln_f``,
``wte``, ``lm_head``, ``recognizer.classifier``), so reference checkpoints load unchanged.

Arithmetic: fp32 state; Linear layers on the split-bf16 (bf16x3) or exact-f32 MFMA GEMMs per
``halo_set_math_mode``; attention, LayerNorm, softmax, rotary and losses in fp32.  The greedy decoder keeps
the reference's float16 cache layout ``[L, 2, N, heads, S|T, head_dim]`` (ha/transformer.py:150-153) -- the
reference itself only decodes under fp16 autocast -- and computes everything around the caches in fp32.

Training: with grad enabled ``AudioEncoder.forward`` and ``Decoder.forward`` (hence CTCAttentionDecoder.forward:
decoder CE + 0.3 CTC) return tensors with a grad_fn whose backward is hand-written end to end (conv front-end,
blocks with shared-x_norm cross/self attention, inverse rotary, exact-GELU MLP, LayerNorm, embedding, CE), so
``loss.backward()`` fills ``.grad`` of every parameter like the reference's autograd does.

Training-mode dropout (p_drop > 0): every site of the reference (encoder input, attention probabilities, both
proj outputs, MLP output) draws from a Philox stream keyed by torch.initial_seed() -- statistically the reference's
dropout, not torch's bit stream; the output dropouts are GEMM epilogues, the probability dropout lives inside the
attention kernels (forward and both backward sweeps recompute the same mask).

Beam search (the reference decodes greedily only): ``BeamDecoder`` on the fused decode launches over N * W rows,
``Decoder.decode(..., beam_size=W)`` / HALO_ASR_BEAM, and ``CTCAttentionDecoder.decode(..., ctc_weight=c)`` re-ranking the lists with
the CTC head.

Not built (raises): prompts under beam search, autograd through a bare Block / MultiHeadAttention call, ``kv_cache_parts`` on the public Block / MultiHeadAttention.forward (Decoder.decode drives the caches
itself), arbitrary attention masks (only the key-padding masks Block builds, transformer.py:476).
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib, _slots, ops
from ._capture import GraphCache
from ._linear import (NO_SITES, DropSites, WeightImages, training_images, drop_rows, forward_images, grad_images, linear, linear_dw, linear_dx, ln_linear,
                      normed_image, rowmajor_ok, use_split)
from .attention import LayerNorm
from .conv import ConvEncoder
from .recognizer import TemporalClassifier
from .rnn import DropoutStream

BlockKVCache = namedtuple('BlockKVCache', ['memory', 'time'])
Stats = namedtuple('Stats', ['meme_entropy', 'self_entropy'])

STX, ETX = 2, 3


def _wants_grad(module):
    return torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())


def _check_device_and_dropout(module, x):
    if not x.is_cuda:
        raise _lib.HaloError(f'haloop_amd.transformer.{type(module).__name__} runs on the HIP device only (no CPU path)')
    if module.training and not _wants_grad(module) and _p_drop(module) > 0:
        raise NotImplementedError('training-mode dropout is built into the autograd path only: enable grad, or call .eval()')


def _p_drop(module):
    """The model's dropout probability (the reference builds every site from one p_drop)."""
    ps = {float(m.p) for m in module.modules() if isinstance(m, nn.Dropout)}
    ps |= {float(m.p_drop) for m in module.modules() if hasattr(m, 'p_drop')}
    if len(ps) > 1:
        raise NotImplementedError(f'one dropout probability per model is built, found {sorted(ps)}')
    return ps.pop() if ps else 0.0


def _require_inference(module, x):
    """Module-level calls (Block, MultiHeadAttention, attend) have no autograd of their own: gradients flow through
    AudioEncoder.forward / Decoder.forward, whose backward is hand-written end to end."""
    if not x.is_cuda:
        raise _lib.HaloError(f'haloop_amd.transformer.{type(module).__name__} runs on the HIP device only (no CPU path)')
    if module.training and _p_drop(module) > 0:
        raise NotImplementedError('training-mode dropout is built into the AudioEncoder / Decoder autograd path only: call .eval()')
    if _wants_grad(module):
        raise NotImplementedError('haloop_amd.transformer.' + type(module).__name__ + ' has no autograd of its own: train through '
                                  'AudioEncoder / Decoder / CTCAttentionDecoder, or call it under torch.no_grad()')


class _GradSink:
    """Collects parameter gradients of one hand-written backward (summing when a parameter is hit twice)."""

    def __init__(self):
        self.g = {}

    def __call__(self, p, grad):
        if p is None or grad is None or not p.requires_grad:
            return
        k = id(p)
        self.g[k] = grad if k not in self.g else self.g[k] + grad


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        with training_images():
            out, saved = model._forward_train(x)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        return out

    @staticmethod
    def backward(ctx, dout):
        sink = _GradSink()
        ctx.model._backward_train(ctx.saved, dout.contiguous().float(), sink)
        ctx.saved = None
        return (None, None) + tuple(sink.g.get(id(p)) for p in ctx.params)


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, features, prompt, tg, mlen, *params):
        with training_images():
            loss, saved = model._forward_train(features, prompt, tg, mlen)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        return loss

    @staticmethod
    def backward(ctx, grad_rows):
        sink = _GradSink()
        dfeat = ctx.model._backward_train(ctx.saved, grad_rows.contiguous().float(), sink)
        ctx.saved = None
        return (None, dfeat if ctx.needs_input_grad[1] else None, None, None, None) + tuple(sink.g.get(id(p)) for p in ctx.params)


def _rope_table(cache, T, head_dim, device):
    hit = cache.get((head_dim, str(device)))
    if hit is None or hit.T < T:
        hit = ops.RopeTable(max(T, 256), head_dim, device)
        cache[(head_dim, str(device))] = hit
    return hit


_ROPE_TABLES = {}


def rotate_interleaved(x, *, t0=0, base=10000):
    "rotate query or key embedding as in https://arxiv.org/abs/2104.09864 GPT-J style (ha/transformer.py:16-31)"
    *lead, T, C = x.shape
    if not x.is_cuda:
        raise _lib.HaloError('haloop_amd.transformer.rotate_interleaved runs on the HIP device only')
    table = ops.RopeTable(t0 + T, C, x.device, base) if base != 10000 else _rope_table(_ROPE_TABLES, t0 + T, C, x.device)
    y = x.float().contiguous().clone().view(-1, C)
    ops.rope_(y, T, 1, C, table, t0=t0)
    return y.view(*lead, T, C)


def attend(q, k, v, mask):
    """(N, heads, T, hd) x (N, heads, S, hd) -> (N, heads, T, hd), entropy (ha/transformer.py:413-430).
    ``mask`` None, a key-padding mask (N, 1, 1, S) whose True entries form a suffix (the models' case: the tiled kernel), or any
    boolean mask broadcastable to (N, heads, T, S) -- and any head dimension -- through the general one-wave-per-row kernel."""
    N, H, T, hd = q.shape
    S = k.shape[-2]
    lens = None
    if hd not in (16, 32, 64) or (mask is not None and not _is_suffix_padding_mask(mask, N, S)):
        y, ent = ops.attention_masked(q, k, v, mask)
        return y.to(q.dtype), ent.mean()
    if mask is not None:
        lens = _suffix_mask_lengths(mask, N, S)
    q2, k2, v2 = (t.transpose(1, 2).reshape(N * t.shape[2], H * hd).float().contiguous() for t in (q, k, v))
    y, _, ent = ops.attention_fwd(q2, k2, v2, N, H, hd, T, S, key_lengths=lens, want_entropy=True)
    return y.view(N, T, H, hd).transpose(1, 2), ent.mean()


def attend_chunked(q, k, v, mask, chunk_size=32):
    "same result as attend without the monitor (ha/transformer.py:374-410); the kernel is already tiled"
    x, _ = attend(q, k, v, mask)
    return x, torch.tensor(float('-inf'))


def _is_suffix_padding_mask(mask, N, S):
    if mask.numel() != N * S or mask.shape[0] != N or mask.shape[-1] != S:
        return False
    m = mask.reshape(N, S)
    lens = (~m).sum(-1)
    return bool((m == (torch.arange(S, device=m.device)[None, :] >= lens[:, None])).all())


def _suffix_mask_lengths(mask, N, S):
    m = mask.reshape(N, -1, S)
    if m.shape[1] != 1:
        raise NotImplementedError('only key-padding masks of shape (N, 1, 1, S) are built')
    m = m[:, 0]
    lens = (~m).sum(-1).to(torch.int32)
    if not bool((m == (torch.arange(S, device=m.device)[None, :] >= lens[:, None])).all()):
        raise NotImplementedError('only key-padding masks whose masked keys form a suffix are built')
    return lens


class MultiHeadAttention(nn.Module):
    def __init__(self, head_dim: int = 64, heads: int = 12, p_drop: float = 0.1):
        super().__init__()
        self.head_dim = head_dim
        self.heads = heads
        self.q = nn.Linear(head_dim * heads, head_dim * heads, bias=False)
        self.k = nn.Linear(head_dim * heads, head_dim * heads, bias=False)
        self.v = nn.Linear(head_dim * heads, head_dim * heads, bias=False)
        self.proj = nn.Linear(head_dim * heads, head_dim * heads, bias=False)
        self.p_drop = p_drop
        self.dropout = nn.Dropout(p_drop)
        self._images = WeightImages()
        self._tables = {}

    def init_from_flash_mha_(self, mha):
        step = self.head_dim * self.heads
        assert mha.Wqkv.weight.shape[0] == step * 3
        self.q.weight.data = mha.Wqkv.weight.data[0*step:1*step, :]
        self.k.weight.data = mha.Wqkv.weight.data[1*step:2*step, :]
        self.v.weight.data = mha.Wqkv.weight.data[2*step:3*step, :]
        self.proj.weight.data = mha.out_proj.weight.data
        return self

    def read_memory(self, memory):
        N, S, C = memory.shape
        kv = linear(self._images, memory.reshape(N * S, C).float().contiguous(), (self.k.weight, self.v.weight))
        k, v = kv[:, :C], kv[:, C:]
        return (k.reshape(N, S, self.heads, self.head_dim).transpose(-3, -2),
                v.reshape(N, S, self.heads, self.head_dim).transpose(-3, -2))

    # x2d [N*T, C] (already normalised), mem2d [N*S, C] or None for self-attention -> attention output [N*T, C] (before proj)
    def _attend2d(self, x2d, mem2d, N, T, S, key_lengths=None, causal=False, rope=False, t0=0, measure_entropy=False, x_img=None):
        C = self.heads * self.head_dim
        if mem2d is None:
            qkv = linear(self._images, x2d, (self.q.weight, self.k.weight, self.v.weight), a_image=x_img)   # one GEMM, [N*T, 3C]
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        else:
            q = linear(self._images, x2d, self.q.weight, a_image=x_img)
            kv = linear(self._images, mem2d, (self.k.weight, self.v.weight))
            k, v = kv[:, :C], kv[:, C:]
        if rope:
            table = _rope_table(self._tables, max(t0 + T, S), self.head_dim, x2d.device)
            ops.rope_(q, T, self.heads, self.head_dim, table, t0=t0)
            ops.rope_(k, S, self.heads, self.head_dim, table)
        y, _, ent = ops.attention_fwd(q, k, v, N, self.heads, self.head_dim, T, S, causal=causal, key_lengths=key_lengths,
                                      want_entropy=measure_entropy)
        return y, (ent.mean() if measure_entropy else torch.tensor(float('-inf')))

    # training twins of _attend2d: keep q/k/v (after the rotary), the output and the log-sum-exp
    def _attend2d_train(self, x2d, mem2d, N, T, S, key_lengths=None, causal=False, rope=False, site=(ops.NO_DROPOUT, 0), x_img=None):
        C = self.heads * self.head_dim
        if mem2d is None:
            qkv = linear(self._images, x2d, (self.q.weight, self.k.weight, self.v.weight), a_image=x_img)
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        else:
            q = linear(self._images, x2d, self.q.weight, a_image=x_img)
            kv = linear(self._images, mem2d, (self.k.weight, self.v.weight))
            k, v = kv[:, :C], kv[:, C:]
        table = None
        if rope:
            table = _rope_table(self._tables, max(T, S), self.head_dim, x2d.device)
            ops.rope_(q, T, self.heads, self.head_dim, table)
            ops.rope_(k, S, self.heads, self.head_dim, table)
        y, lse, _ = ops.attention_fwd(q, k, v, N, self.heads, self.head_dim, T, S, causal=causal, key_lengths=key_lengths, want_lse=True,
                                      drop=site[0], stream_id=site[1])
        return y, (x2d, mem2d, q, k, v, y, lse, key_lengths, causal, table, N, T, S, site)

    def _attend2d_bwd(self, saved, dy, put, dx_out=None, dmem_out=None):
        """dy: gradient of the attention output (before proj).  Accumulates the input gradient into dx_out (allocates it
        when None) and, for cross-attention, the memory gradient into dmem_out.  -> dx"""
        x2d, mem2d, q, k, v, y, lse, key_lengths, causal, table, N, T, S, site = saved
        C = self.heads * self.head_dim
        dev = x2d.device
        if mem2d is None:
            dqkv = torch.empty(N * T, 3 * C, device=dev, dtype=torch.float32)
            dq, dk, dv = dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]
        else:
            dq = torch.empty(N * T, C, device=dev, dtype=torch.float32)
            dkv = torch.empty(N * S, 2 * C, device=dev, dtype=torch.float32)
            dk, dv = dkv[:, :C], dkv[:, C:]
        ops.attention_bwd(q, k, v, y, dy, lse, dq, dk, dv, N, self.heads, self.head_dim, T, S, causal=causal, key_lengths=key_lengths,
                          drop=site[0], stream_id=site[1])
        if table is not None:                                   # the rotation is orthogonal: its transpose rotates back
            ops.rope_(dq, T, self.heads, self.head_dim, table, inverse=True)
            ops.rope_(dk, S, self.heads, self.head_dim, table, inverse=True)
        ws = (self.q.weight, self.k.weight, self.v.weight)
        # each projection gradient feeds a weight-gradient and an input-gradient GEMM: both operand images from one read
        if mem2d is None:
            im, im_t = grad_images(dqkv, C)
            dw = linear_dw(dqkv, x2d, dy_image_t=im_t)          # [3C, C]
            for i, w in enumerate(ws):
                put(w, dw[i * C:(i + 1) * C])
            return linear_dx(self._images, dqkv, ws, out=dx_out, accumulate=dx_out is not None, dy_image=im)
        im, im_t = grad_images(dq, C)
        put(self.q.weight, linear_dw(dq, x2d, dy_image_t=im_t))
        km, km_t = grad_images(dkv, C) if dmem_out is not None else (None, None)
        dwkv = linear_dw(dkv, mem2d, dy_image_t=km_t)
        put(self.k.weight, dwkv[:C]); put(self.v.weight, dwkv[C:])
        if dmem_out is not None:
            linear_dx(self._images, dkv, ws[1:], out=dmem_out, accumulate=True, dy_image=km)
        return linear_dx(self._images, dq, self.q.weight, out=dx_out, accumulate=dx_out is not None, dy_image=im)

    def forward(self, x, memory, *, mask=None, causal=False, measure_entropy=False, kv_cache_parts=None, t0=0, rope=False,
                _key_lengths=None):
        _require_inference(self, x)
        if kv_cache_parts is not None:
            raise NotImplementedError('kv_cache_parts: the fp16 caches are driven by haloop_amd.transformer.Decoder.decode')
        N, T, C = x.shape
        S = memory.shape[1]
        if mask is not None and _key_lengths is None:
            _key_lengths = _suffix_mask_lengths(mask, N, S)
        x2d = x.reshape(N * T, C).float().contiguous()
        mem2d = None if memory is x else memory.reshape(N * S, C).float().contiguous()
        y, ent = self._attend2d(x2d, mem2d, N, T, S, _key_lengths, causal and _key_lengths is None, rope, t0, measure_entropy)
        return linear(self._images, y, self.proj.weight).view(N, T, C), ent


class Block(nn.Module):
    def __init__(self, head_dim: int, heads: int, p_drop: float, memory=False):
        super().__init__()
        self.heads = heads
        self.head_dim = head_dim
        self.ln_time = LayerNorm(head_dim * heads, bias=False)
        self.mix_time = MultiHeadAttention(head_dim=head_dim, heads=heads, p_drop=p_drop)
        self.mix_memory = MultiHeadAttention(head_dim=head_dim, heads=heads, p_drop=p_drop) if memory else None
        self.ln_chan = LayerNorm(head_dim * heads, bias=False)
        self.mix_chan = nn.Sequential(
            nn.Linear(head_dim * heads, head_dim * heads * 4, bias=False),
            nn.GELU(),
            nn.Linear(head_dim * heads * 4, head_dim * heads, bias=False),
            nn.Dropout(p_drop),
        )
        self._images = WeightImages()

    # x2d [N*T, C] is updated IN PLACE (the caller owns it); memory rows [N*S, C]
    def _forward2d(self, x2d, N, T, causal=False, mem2d=None, S=0, memory_lengths=None, measure_entropy=False, time_lengths=None):
        # ln_time(x) feeds up to two GEMMs (cross query, self q|k|v): one LayerNorm pass writes their shared operand image
        x_norm, x_img = normed_image(x2d, self.ln_time.weight, n_out=x2d.shape[1])
        m_ent = torch.tensor(float('-inf'))
        if self.mix_memory is not None:
            mm = self.mix_memory
            m, m_ent = mm._attend2d(x_norm, mem2d, N, T, S, key_lengths=memory_lengths, measure_entropy=measure_entropy, x_img=x_img)
            linear(mm._images, m, mm.proj.weight, out=x2d, accumulate=True)                      # x += cross(ln(x), memory)
        mt = self.mix_time
        t, t_ent = mt._attend2d(x_norm, None, N, T, T, key_lengths=time_lengths, causal=causal and time_lengths is None, rope=True,
                                measure_entropy=measure_entropy, x_img=x_img)                    # the SAME x_norm (:476-494)
        linear(mt._images, t, mt.proj.weight, out=x2d, accumulate=True)
        M, C = x2d.shape
        if rowmajor_ok(M, 4 * C, C) and C % 32 == 0:        # the MLP's activations go on as row-major bf16 (halo_gemm_split_io)
            h, _ = ln_linear(self._images, x2d, self.ln_chan.weight, None, self.mix_chan[0].weight, gelu='erf', out_rowmajor=True)
            linear(self._images, None, self.mix_chan[2].weight, out=x2d, accumulate=True, a_rowmajor=h, shape=(M, 4 * C))
            return m_ent, t_ent
        h, _ = ln_linear(self._images, x2d, self.ln_chan.weight, None, self.mix_chan[0].weight, gelu='erf')
        linear(self._images, h, self.mix_chan[2].weight, out=x2d, accumulate=True)
        return m_ent, t_ent

    def _forward2d_train(self, x0, N, T, causal=False, mem2d=None, S=0, memory_lengths=None, sites=NO_SITES):
        """Dropout sites in forward order: [cross-attention probabilities, cross proj output,] self-attention probabilities,
        self proj output, MLP output (ha/transformer.py:356,371,457); each output dropout is the GEMM's epilogue."""
        x_norm, x_img = normed_image(x0, self.ln_time.weight, n_out=x0.shape[1])
        xa, sv_m, s_mo = x0, None, None
        if self.mix_memory is not None:
            mm = self.mix_memory
            ym, sv_m = mm._attend2d_train(x_norm, mem2d, N, T, S, key_lengths=memory_lengths, site=sites.next(), x_img=x_img)
            s_mo = sites.next()
            xa = linear(mm._images, ym, mm.proj.weight, out=x0.clone(), accumulate=True, drop=s_mo[0], stream_id=s_mo[1])
        mt = self.mix_time
        yt, sv_t = mt._attend2d_train(x_norm, None, N, T, T, causal=causal, rope=True, site=sites.next(), x_img=x_img)
        s_to = sites.next()
        xb = linear(mt._images, yt, mt.proj.weight, out=xa.clone(), accumulate=True, drop=s_to[0], stream_id=s_to[1])
        a, hn = ln_linear(self._images, xb, self.ln_chan.weight, None, self.mix_chan[0].weight, want_normed=True)
        # gelu(a) is only ever a GEMM operand (mix_chan[2] now, its weight gradient later): write its two images, not the matrix
        g_img, g_img_t = forward_images(a, x0.shape[1], ops.PAIR_GELU_ERF)
        g = ops.gelu_fwd(a, exact=True) if g_img is None else None
        s_co = sites.next()
        xc = linear(self._images, g, self.mix_chan[2].weight, out=xb.clone(), accumulate=True, drop=s_co[0], stream_id=s_co[1],
                    a_image=g_img, shape=a.shape)
        return xc, (x0, sv_m, sv_t, xb, hn, a, g, g_img_t, s_mo, s_to, s_co)

    def _backward2d(self, saved, dxc, put, dmem_out=None):
        x0, sv_m, sv_t, xb, hn, a, g, g_img_t, s_mo, s_to, s_co = saved
        w0, w2 = self.mix_chan[0].weight, self.mix_chan[2].weight
        C, M = x0.shape[1], x0.shape[0]
        dmlp = drop_rows(dxc, s_co)                                             # gradient at the MLP output, before its dropout
        dm_img, dm_img_t = grad_images(dmlp, a.shape[1])
        put(w2, linear_dw(dmlp, g, dy_image_t=dm_img_t, x_image_t=g_img_t, shapes=(dmlp.shape, a.shape)))
        dg = linear_dx(self._images, dmlp, w2, dy_image=dm_img)
        if use_split(M, C, a.shape[1]) and use_split(a.shape[1], C, M):
            da_img, da_img_t = ops.image_pair(dg, ops.PAIR_GELU_ERF_BWD, a)    # da = dg * gelu'(a), as its two operand images only
            put(w0, linear_dw(None, hn, dy_image_t=da_img_t, shapes=(a.shape, hn.shape)))
            d_ln = linear_dx(self._images, None, w0, dy_image=da_img, shape=a.shape)
        else:
            da = ops.gelu_bwd(dg, a, exact=True)
            put(w0, linear_dw(da, hn))
            d_ln = linear_dx(self._images, da, w0)
        dxb, dw, _ = ops.layernorm_bwd(d_ln, xb, self.ln_chan.weight, dxc)
        put(self.ln_chan.weight, dw)
        mt = self.mix_time
        dto = drop_rows(dxb, s_to)
        im, im_t = grad_images(dto, C)
        put(mt.proj.weight, linear_dw(dto, sv_t[5], dy_image_t=im_t))
        dxn = mt._attend2d_bwd(sv_t, linear_dx(mt._images, dto, mt.proj.weight, dy_image=im), put)
        if sv_m is not None:
            mm = self.mix_memory
            dmo = drop_rows(dxb, s_mo)
            im, im_t = grad_images(dmo, C)
            put(mm.proj.weight, linear_dw(dmo, sv_m[5], dy_image_t=im_t))
            mm._attend2d_bwd(sv_m, linear_dx(mm._images, dmo, mm.proj.weight, dy_image=im), put, dx_out=dxn, dmem_out=dmem_out)
        dx0, dw, _ = ops.layernorm_bwd(dxn, x0, self.ln_time.weight, dxb)      # both attentions read the same ln_time(x)
        put(self.ln_time.weight, dw)
        return dx0

    def forward(self, x, time_mask=None, causal=False, memory=None, memory_lengths=None, measure_entropy=False,
                kv_cache_parts=BlockKVCache(memory=None, time=None), t0=0):
        _require_inference(self, x)
        if kv_cache_parts.memory is not None or kv_cache_parts.time is not None:
            raise NotImplementedError('kv_cache_parts: the fp16 caches are driven by haloop_amd.transformer.Decoder.decode')
        if t0 != 0:
            raise NotImplementedError('t0 != 0 only occurs with kv caches')
        N, T, C = x.shape
        x2d = x.reshape(N * T, C).float().clone()
        mem2d, S, mlen = None, 0, None
        if self.mix_memory is not None:
            S = memory.shape[1]
            mem2d = memory.reshape(N * S, C).float().contiguous()
            mlen = memory_lengths.to(device=x.device, dtype=torch.int32)
        tlen = _suffix_mask_lengths(time_mask, N, T) if time_mask is not None else None
        ents = self._forward2d(x2d, N, T, causal, mem2d, S, mlen, measure_entropy, tlen)
        return x2d.view(N, T, C), ents


class Decoder(nn.Module):
    def __init__(self, *, vocab: int, head_dim: int, heads: int, p_drop: float, layers: int):
        super().__init__()
        self.wte = nn.Embedding(vocab, head_dim * heads)
        self.h = nn.ModuleList([Block(head_dim=head_dim, heads=heads, p_drop=p_drop, memory=True) for _ in range(layers)])
        self.ln_f = LayerNorm(head_dim * heads, bias=False)
        self.lm_head = nn.Linear(head_dim * heads, vocab, bias=False)
        self._images = WeightImages()
        self._graphs = GraphCache()                                       # captured greedy decodes, see _decode_graph
        self.dropout_stream = DropoutStream()                             # Philox (seed, offset) per training forward
        self.beam_size = int(os.environ.get('HALO_ASR_BEAM', '0'))        # decode(): 0 greedy, W >= 1 BeamDecoder's search
        self.length_bonus = 0.0                                           # of that search
        self._beams = {}                                                  # its BeamDecoder, built at the first beam decode
        self.last_parts = None                                            # (attention, lm_scores) of a beam decode after set_fusion_lm

    def forward(self, features, targets, input_lengths=None, target_lengths=None, star_penalty=None, measure_entropy=False,
                drop_labels=None, reduction='mean'):
        _check_device_and_dropout(self, features)
        dev = features.device
        targets = targets.to(dev)
        N, T = targets.shape
        # prompt: STX a b c / target: a b c ETX PAD (ha/transformer.py:84-98)
        prompt = nn.functional.pad(targets, (1, 0), value=STX)
        tg = nn.functional.pad(targets, (0, 1), value=0)
        tg.scatter_(1, target_lengths.to(device=dev, dtype=torch.long).view(N, 1), ETX)       # tg[n, target_lengths[n]] = ETX, capture-safe
        T = T + 1
        if (drop_labels is None and self.training) or drop_labels:
            # label dropout (ha/transformer.py:100-103): integer data preparation, drawn from torch's generator like the reference
            keep = torch.empty_like(prompt).bernoulli_(0.9).bool()
            prompt = torch.where(keep, prompt, torch.ones_like(prompt))
        S, C = features.shape[1], features.shape[2]
        mlen = input_lengths.to(device=dev, dtype=torch.int32)
        if _wants_grad(self) or (torch.is_grad_enabled() and features.requires_grad):
            if measure_entropy or reduction == 'sumeach':
                raise NotImplementedError("measure_entropy / reduction='sumeach' are inference-only here: call under torch.no_grad()")
            params = [p for p in self.parameters() if p.requires_grad]
            per_tok = _DecoderFn.apply(self, features, prompt, tg, mlen, *params)
            if reduction == 'none':
                loss = per_tok
            elif reduction == 'sum':
                loss = per_tok.sum()
            elif reduction == 'mean':
                loss = per_tok.sum() / (tg != 0).sum()
            else:
                raise ValueError(f'{reduction} is not a valid value for reduction')
            ninf = [torch.tensor(float('-inf'))] * len(self.h)
            return loss, Stats(meme_entropy=list(ninf), self_entropy=list(ninf))._asdict()
        mem2d = features.reshape(N * S, C).float().contiguous()
        stats = Stats(meme_entropy=[], self_entropy=[])
        y = ops.embed_fwd(prompt, self.wte.weight, None)
        for block in self.h:
            m_ent, t_ent = block._forward2d(y, N, T, True, mem2d, S, mlen, measure_entropy)
            stats.meme_entropy.append(m_ent)
            stats.self_entropy.append(t_ent)
        logits = linear(self._images, ops.layernorm_fwd(y, self.ln_f.weight), self.lm_head.weight)   # [N*T, V]
        if reduction == 'sumeach':
            loss = ops.logprob_max(logits)[0].view(N, T).sum(dim=-1)
        else:
            per_tok = ops.cross_entropy_fwd(logits, tg.reshape(-1), ignore_index=0)
            if reduction == 'none':
                loss = per_tok
            elif reduction == 'sum':
                loss = per_tok.sum()
            elif reduction == 'mean':
                loss = per_tok.sum() / (tg != 0).sum()
            else:
                raise ValueError(f'{reduction} is not a valid value for reduction')
        return loss, stats._asdict()

    @torch.no_grad()
    def _forward_train(self, features, prompt, tg, mlen):
        N, T = prompt.shape
        S, C = features.shape[1], features.shape[2]
        mem2d = features.detach().reshape(N * S, C).float().contiguous()
        y = ops.embed_fwd(prompt, self.wte.weight, None)
        sites = DropSites(self.dropout_stream.next(_p_drop(self), self.training))
        blocks = []
        for block in self.h:
            y, sv = block._forward2d_train(y, N, T, True, mem2d, S, mlen, sites)
            blocks.append(sv)
        xf = ops.layernorm_fwd(y, self.ln_f.weight)
        logits = linear(self._images, xf, self.lm_head.weight)
        loss, row_lse = ops.cross_entropy_fwd_lse(logits, tg.reshape(-1), ignore_index=0)
        return loss, (prompt, tg.reshape(-1), blocks, y, xf, logits, row_lse, (N, S, C))

    @torch.no_grad()
    def _backward_train(self, saved, grad_rows, put):
        prompt, tg, blocks, y_last, xf, logits, row_lse, (N, S, C) = saved
        dlogits = ops.cross_entropy_bwd_(logits, tg, row_lse, grad_rows, ignore_index=0)
        put(self.lm_head.weight, linear_dw(dlogits, xf))
        dy, dw, _ = ops.layernorm_bwd(linear_dx(self._images, dlogits, self.lm_head.weight), y_last, self.ln_f.weight)
        put(self.ln_f.weight, dw)
        dmem = torch.zeros(N * S, C, device=xf.device, dtype=torch.float32)
        for block, sv in zip(reversed(self.h), reversed(blocks)):
            dy = block._backward2d(sv, dy, put, dmem_out=dmem)
        dwte = torch.zeros_like(self.wte.weight)
        ops.embed_bwd(prompt, dy, dwte, None)
        put(self.wte.weight, dwte)
        return dmem.view(N, S, C)

    def _memory_caches_general(self, mem2d, rows, S):
        """The cross-attention caches of the operator-per-launch path [L, 2, rows, heads, S, head_dim], warmed once per decode (:324-334)."""
        C = mem2d.shape[1]
        heads, head_dim = self.h[0].heads, self.h[0].head_dim
        mem_cache = torch.zeros((len(self.h), 2, rows, heads, S, head_dim), dtype=torch.float16, device=mem2d.device)
        for l, block in enumerate(self.h):
            mm = block.mix_memory
            kv = linear(mm._images, mem2d, (mm.k.weight, mm.v.weight))
            ops.kv_cache_store(kv, C, mem_cache[l, 0], mem_cache[l, 1], rows, S, heads, head_dim, 0)
        return mem_cache

    def _step_general(self, y, mem_cache, mlen, time_cache, n_keys, table):
        """One step on the operator-per-launch path: the rows' embeddings y [rows, C] (updated in place) -> logits [rows, V], over the
        memory caches (key lengths mlen) and the self-attention caches, which receive position n_keys - 1."""
        C, S = y.shape[1], mem_cache.shape[4]
        for l, block in enumerate(self.h):
            mm, mt = block.mix_memory, block.mix_time
            xn = ops.layernorm_fwd(y, block.ln_time.weight)
            # both attentions read the same ln_time(x) (:476-494): one GEMM gives the cross query and the self q | k | v
            a = linear(mt._images, xn, (mm.q.weight, mt.q.weight, mt.k.weight, mt.v.weight))      # [rows, 4C]
            m = ops.attention_decode(a, mem_cache[l, 0], mem_cache[l, 1], S, key_lengths=mlen)
            linear(mm._images, m, mm.proj.weight, out=y, accumulate=True)
            # cache store (fp16) + rotary + attention over the n_keys cached positions in one launch
            s = ops.attention_decode_step(a[:, C:2 * C], a[:, 2 * C:3 * C], a[:, 3 * C:], time_cache[l, 0], time_cache[l, 1], n_keys,
                                          table=table)
            linear(mt._images, s, mt.proj.weight, out=y, accumulate=True)
            h = linear(block._images, ops.layernorm_fwd(y, block.ln_chan.weight), block.mix_chan[0].weight, gelu='erf')
            linear(block._images, h, block.mix_chan[2].weight, out=y, accumulate=True)
        return linear(self._images, ops.layernorm_fwd(y, self.ln_f.weight), self.lm_head.weight)

    @torch.no_grad()
    def _decode_core(self, mem2d, mlen, tokens_init, plen, N, S, T):
        """All launches of one batched greedy decode, host-sync free (capturable in a HIP graph).
        mem2d [N*S, C] fp32 features, mlen [N] int32, tokens_init [N, W] int64 (STX, optional prompt, ETX fill)."""
        dev = mem2d.device
        L = len(self.h)
        heads, head_dim = self.h[0].heads, self.h[0].head_dim
        tokens = tokens_init.clone()
        mem_cache = self._memory_caches_general(mem2d, N, S)
        time_cache = torch.zeros((L, 2, N, heads, T, head_dim), dtype=torch.float16, device=dev)
        table = ops.RopeTable(T, head_dim, dev)
        alive = torch.ones(N, dtype=torch.uint8, device=dev)
        out_len = torch.zeros(N, dtype=torch.int32, device=dev)
        log_probs = torch.zeros(N, dtype=torch.float32, device=dev)
        sum_entropies = torch.zeros(N, dtype=torch.float32, device=dev)
        # every step computes all N rows; rows that are no longer alive are ignored by the update (the reference
        # compacts to the alive rows instead, which changes no alive row's result) and nothing syncs with the host
        for t in range(T):
            y = ops.embed_fwd(tokens[:, t:t + 1], self.wte.weight, None)         # [N, C]
            logits = self._step_general(y, mem_cache, mlen, time_cache, t + 1, table)
            val, idx, negent = ops.logprob_max(logits, want_entropy=True)
            ops.greedy_update(val, idx, negent, tokens, t, plen, ETX, alive, out_len, log_probs, sum_entropies)
        return tokens, out_len, log_probs, sum_entropies

    def _fused_decode_ok(self, C):
        """The fused decode launches (csrc/decode.hip): split-bf16 arithmetic, so not in exact-f32 mode; HALO_DECODE_FUSED=0 keeps
        the operator-per-launch path (same results up to the products' rounding)."""
        return (os.environ.get('HALO_DECODE_FUSED', '1') != '0' and _lib.get_math_mode() != 'f32'
                and ops.decode_linear_supported(C, True) and ops.decode_linear_supported(2 * C, False)
                and ops.decode_linear_supported(4 * C, False) and self.h[0].head_dim in (16, 32, 64, 128))

    @torch.no_grad()
    def _decode_images(self):
        """Decode images of every product of a step, rebuilt when a parameter changes: per layer the merged projection
        [mm.q; mt.q; mt.k; mt.v], the merged output projection [mm.proj | mt.proj] (K = 2C: cross | self attention outputs), the two
        MLP weights; and lm_head."""
        stamp = tuple((p._version, p.data_ptr()) for p in self.parameters())
        if getattr(self, '_dec_images', None) is None or self._dec_images[0] != stamp:
            layers = []
            for block in self.h:
                mm, mt = block.mix_memory, block.mix_time
                layers.append((ops.decode_image(torch.cat([mm.q.weight, mt.q.weight, mt.k.weight, mt.v.weight], 0).float().contiguous()),
                               ops.decode_image(torch.cat([mm.proj.weight, mt.proj.weight], 1).float().contiguous()),
                               ops.decode_image(block.mix_chan[0].weight.detach().float().contiguous()),
                               ops.decode_image(block.mix_chan[2].weight.detach().float().contiguous())))
            head = ops.decode_image(self.lm_head.weight.detach().float().contiguous())
            self._dec_images = (stamp, layers, head)
        return self._dec_images[1], self._dec_images[2]

    def _memory_caches_fused(self, mem2d, N, S):
        """The cross-attention caches of the fused path [L, 2, N, heads, S, head_dim], warmed once per decode (:324-334): the memory
        keys / values of all layers are ONE product and one store."""
        heads, head_dim = self.h[0].heads, self.h[0].head_dim
        mem_cache = torch.empty((len(self.h), 2, N, heads, S, head_dim), dtype=torch.float16, device=mem2d.device)
        kv_weights = tuple(w for block in self.h for w in (block.mix_memory.k.weight, block.mix_memory.v.weight))
        ops.decode_memory_caches(linear(self._images, mem2d, kv_weights), mem_cache)
        return mem_cache

    @staticmethod
    def _decode_ksplit(C):
        """The two accumulating products of a layer (K = 2C, 4C into C features: 128 workgroups at N = 64, each streaming its weights and
        its rows over the whole K) run as two K-slices on twice the workgroups (HALO_DECODE_KSPLIT=0: one slice, the round-4 launches):
        _step_fused then needs the two side buffers."""
        return os.environ.get('HALO_DECODE_KSPLIT', '1') != '0' and (2 * C) % 512 == 0

    def _step_fused(self, images, y, a, att, hid, logits, sa, sb, attention):
        """The launches of one step on the fused path, 5 per layer and the ln_f + lm_head product: the rows' embeddings y [rows, C]
        -> logits [rows, V].  a, hid [rows, 4C]: cross query | self q | k | v and the MLP hidden rows; att [rows, 2C]: cross | self
        attention outputs, written from a by ``attention(l)``, the step's attention launch of layer l.  With side buffers sa, sb
        [rows, C] (K-sliced products) the residual stream is the pair (y, side): slice 0 writes y = (y + side) + its half, slice 1 its
        half to the OTHER side buffer; the LayerNorm launches read y + side.  Every sum in a fixed order."""
        layers, head_img = images
        C, V = y.shape[1], logits.shape[1]
        side = None                                                          # (y alone: the embedding of the step's token)
        for l, block in enumerate(self.h):
            w_qkv, w_proj, w_fc, w_fc2 = layers[l]
            ops.decode_linear(y, w_qkv, 4 * C, a, ln_weight=block.ln_time.weight, x_side=side)      # both attentions read ln_time(x) (:476-494)
            attention(l)
            ops.decode_linear(att, w_proj, C, y, accumulate=True, side_in=side, side_out=sa)         # x += cross proj + self proj
            ops.decode_linear(y, w_fc, 4 * C, hid, ln_weight=block.ln_chan.weight, gelu=True, x_side=sa)
            ops.decode_linear(hid, w_fc2, C, y, accumulate=True, side_in=sa, side_out=sb)
            side = sb
        ops.decode_linear(y, head_img, V, logits, ln_weight=self.ln_f.weight, x_side=side)

    @torch.no_grad()
    def _decode_core_fused(self, mem2d, mlen, tokens_init, plen, N, S, T):
        """_decode_core on the fused launches: 5 per layer and step, 2 per step for the head (+ the cache warm-up)."""
        dev = mem2d.device
        C = mem2d.shape[1]
        L = len(self.h)
        heads, head_dim = self.h[0].heads, self.h[0].head_dim
        V = self.lm_head.weight.shape[0]
        images = self._decode_images()
        tokens = tokens_init.clone()
        mem_cache = self._memory_caches_fused(mem2d, N, S)
        time_cache = torch.zeros((L, 2, N, heads, T, head_dim), dtype=torch.float16, device=dev)
        table = ops.RopeTable(T, head_dim, dev)
        alive = torch.ones(2, N, dtype=torch.uint8, device=dev)             # double-buffered by step parity (halo_decode_token)
        out_len = torch.zeros(N, dtype=torch.int32, device=dev)
        log_probs = torch.zeros(N, dtype=torch.float32, device=dev)
        sum_entropies = torch.zeros(N, dtype=torch.float32, device=dev)
        a = torch.empty(N, 4 * C, device=dev, dtype=torch.float32)           # cross query | self q | k | v, then the MLP hidden rows
        att = torch.empty(N, 2 * C, device=dev, dtype=torch.float32)         # cross | self attention outputs
        hid = torch.empty(N, 4 * C, device=dev, dtype=torch.float32)
        logits = torch.empty(N, V, device=dev, dtype=torch.float32)
        wte = self.wte.weight.detach()
        y = ops.embed_fwd(tokens[:, 0:1], wte, None)                         # [N, C]; later steps: written by decode_token
        sa, sb = (torch.empty(N, C, device=dev, dtype=torch.float32) for _ in range(2)) if self._decode_ksplit(C) else (None, None)
        for t in range(T):
            self._step_fused(images, y, a, att, hid, logits, sa, sb, lambda l: ops.decode_attention_pair(
                a, mem_cache[l, 0], mem_cache[l, 1], mlen, time_cache[l, 0], time_cache[l, 1], t + 1, table, att))
            ops.decode_token(logits, tokens, t, plen, ETX, alive, out_len, log_probs, sum_entropies, wte, y if t + 1 < T else None)
        return tokens, out_len, log_probs, sum_entropies

    def _decode_graph(self, key, mem2d, mlen, tokens, plen, N, S, T):
        """One HIP graph per (shape, parameter version): ~13 launches x layers x steps become one replay."""
        core = self._decode_core_fused if self._fused_decode_ok(mem2d.shape[1]) else self._decode_core
        entry = self._graphs.entry(self, key, lambda: (mem2d.clone(), mlen.clone(), tokens.clone()),
                                   lambda static: core(*static, plen, N, S, T))
        for dst, src in zip(entry['static'], (mem2d, mlen, tokens)):
            dst.copy_(src)
        entry['graph'].replay()
        return tuple(o.clone() for o in entry['outs'])

    def set_fusion_lm(self, lm, lm_weight=0.5, start_token=0, lm_eos=None):
        """Shallow fusion for ``decode(..., beam_size=W)``: ``lm``, an ``rnn.Decoder`` over this decoder's classes, scores every candidate
        inside the search (``fusion.AttentionFusionDecoder``), and ``last_parts`` = (attention, lm_scores) is kept with
        ``last_nbest``.  The LM is not a submodule: the state dict and the parameters are unchanged.  ``set_fusion_lm(None)``: the plain
        search again.  Greedy decoding does not use it."""
        self._beams.pop('fusion', None)
        if lm is None:
            self._beams.pop('lm', None)
            return
        from .fusion import _fusion_settings
        a, start, eos, _ = _fusion_settings('Decoder.set_fusion_lm', lm, self.lm_head.weight.shape[0], lm_weight, start_token, lm_eos)
        self._beams['lm'] = dict(lm=lm, lm_weight=a, start_token=start, lm_eos=eos)        # (in the dict: not registered as a submodule)

    @torch.no_grad()
    def _decode_beam(self, features, input_lengths, T, W, ctc_log_probs=None, ctc_weight=0.0, fusion=True):
        """Beam search at width W with room for T steps (the greedy decode's step count): each row's best hypothesis in the greedy
        decode's five-value form, the lists in ``last_nbest``.  With ``ctc_log_probs`` and a weight: the joint search.  With an LM set
        by ``set_fusion_lm`` (and ``fusion``): the search with the LM, ``last_parts`` kept."""
        N = features.shape[0]
        which = 'fusion' if fusion and 'lm' in self._beams else 'decoder'
        bd = self._beams.get(which)
        if bd is None or bd.max_batch < N or bd.capacity < T or bd.beam < W or bd._device != self.wte.weight.device \
                or bd.length_bonus != float(self.length_bonus):
            sizes = (max(N, bd.max_batch if bd else 0), max(T, bd.capacity if bd else 0), max(W, bd.beam if bd else 0))
            if which == 'fusion':
                from .fusion import AttentionFusionDecoder
                f = self._beams['lm']
                bd = AttentionFusionDecoder(self, f['lm'], *sizes, f['lm_weight'], self.length_bonus, f['start_token'], f['lm_eos'])
            else:
                bd = BeamDecoder(self, *sizes, self.length_bonus)
            self._beams[which] = bd
        self._beams['used'] = which
        self.last_nbest = bd.decode(features, input_lengths, capacity=T, beam=W, ctc_log_probs=ctc_log_probs, ctc_weight=ctc_weight)
        self.last_parts = bd.last_parts if which == 'fusion' else None
        tokens, lengths, _, _ = self.last_nbest
        # greedy's output_lengths count the steps a row was alive: its tokens and, where it closed, the ETX; greedy's outputs are
        # tokens[1:output_lengths] (sic: a row that never closed loses its last token, ha/transformer.py:197) -- kept, so W = 1 is greedy
        out_len = lengths[:, 0].clamp(min=0) + bd.last_finished[:, 0].long()
        lens = out_len.tolist()
        outputs = torch.nested.nested_tensor([tokens[i, 0, :max(n - 1, 0)] for i, n in enumerate(lens)])
        nan = torch.full((N,), float('nan'), device=features.device)     # summed over all alive rows (sic) in greedy: no beam analogue
        return outputs, out_len.to(input_lengths.dtype), [None] * N, bd.last_logprobs[:, 0].clone(), nan

    @torch.no_grad()
    def decode(self, features, input_lengths, target_lengths, prompt=None, beam_size=None, fusion=True):
        """Perform batched greedy decoding (ha/transformer.py:124-199).  ``beam_size`` W >= 1 (default: the attribute ``beam_size``, read
        from HALO_ASR_BEAM when the module is built; 0: greedy): ``BeamDecoder``'s search at width W with the attribute ``length_bonus``
        and the greedy decode's step count; returns each row's best hypothesis (its plain log-probability, NaN for the entropy sum) and
        keeps the lists as ``last_nbest``.  After ``set_fusion_lm`` the search ranks with the LM (``fusion=False``: without it)."""
        _require_inference(self, features)
        width = self.beam_size if beam_size is None else int(beam_size)
        if width < 0:
            raise ValueError(f'Decoder.decode: beam_size {width} is negative')
        if width:
            if prompt is not None:
                raise NotImplementedError('Decoder.decode(beam_size >= 1): prompts are not built')
            return self._decode_beam(features, input_lengths, int(target_lengths.max().item()) + 1, width, fusion=fusion)
        dev = features.device
        N, S, C = features.shape
        T = int(target_lengths.max().item()) + 1
        if prompt is None:
            tokens = torch.full((N, T + 1), ETX, dtype=torch.long, device=dev)
            tokens[:, 0] = STX
            plen = 0
        else:
            P = prompt.shape[-1]
            tokens = torch.full((N, T + 1 + P), ETX, dtype=torch.long, device=dev)
            tokens[:, 0] = STX
            tokens[:, 1:1 + P] = prompt.to(dev)
            plen = 1
        mlen = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
        mem2d = features.reshape(N * S, C).float().contiguous()
        if os.environ.get('HALO_DECODE_GRAPH', '1') != '0':
            key = (N, S, T, tokens.shape[1], plen, str(dev), _lib.get_math_mode(), self._fused_decode_ok(C))
            tokens, out_len, log_probs, sum_entropies = self._decode_graph(key, mem2d, mlen, tokens, plen, N, S, T)
        else:
            core = self._decode_core_fused if self._fused_decode_ok(C) else self._decode_core
            tokens, out_len, log_probs, sum_entropies = core(mem2d, mlen, tokens, plen, N, S, T)
        output_lengths = out_len.to(input_lengths.dtype)
        lens = output_lengths.tolist()
        outputs = torch.nested.nested_tensor([p[1:l] for p, l in zip(tokens, lens)])
        alignments = [None] * N
        return outputs, output_lengths, alignments, log_probs, sum_entropies


BEAM_MAX = 16            # csrc/decode_beam.hip keeps an utterance's records in LDS arrays of this many entries
PREFIX_MAX_FRAMES = 4096  # csrc/ctc_prefix_score.hip keeps two rows of S floats of a slot's state in 32 KiB of LDS


class BeamDecoder:
    """Beam search for a ``Decoder`` (the reference decodes greedily only, so the definition is this library's own, fixed
    in include/halo.h), with preallocated buffers for ``max_batch`` utterances, ``beam`` hypotheses each and ``capacity`` steps.  Per
    utterance, with W = beam:

        B = [slot 0: tokens [STX], log-probability 0, length 0]                    # the other slots are empty
        for t in 0 .. capacity - 1:                                                # nothing ends early: no host read
            lp_j = log_softmax(logits of live slot j)
            candidates: (j, k) for every live j and k < V with score_j + lp_j[k] and length len_j + (k != ETX); (j, ETX) for every
                        finished j, unchanged
            B = the W best by (rank = fmaf(length_bonus, length, score) descending, position j V + k ascending), rank > -inf

    W = 1 with length_bonus 0 is ``Decoder.decode``'s greedy search token for token.  The fused path costs ``5 * layers + 2`` launches per
    step for the whole batch (csrc/decode.hip's products and its attention through a per-slot ancestor table on N * W rows,
    csrc/decode_beam.hip's selection), replayed from a captured graph unless HALO_DECODE_GRAPH=0; the general path (f32 mode, widths the fused
    products refuse, HALO_DECODE_FUSED=0) runs the same search on ``Decoder._decode_core``'s operators over N * W rows, the caches
    gathered physically and the candidates pruned by a stable sort.

    Joint CTC/attention decoding (the definition: include/halo.h): ``decode(..., ctc_log_probs, ctc_weight=c)`` with c > 0
    ranks every candidate by ``(1 - c) * rank + c * psi``, psi the CTC prefix score of the extended token sequence (for ETX and for a
    finished slot: the full CTC log-probability of the hypothesis).  Three more launches a step (csrc/ctc_prefix_score.hip's scores, the
    joint selection, the state advance): ``5 * layers + 4``; the general path takes scores and advance from the same launches.

    LM shallow fusion: ``fusion.AttentionFusionDecoder`` runs these cores with an LM side, which puts
    ``halo_decode_beam_select_lm`` in the place of the selection and the LM's cell launches behind it."""

    def __init__(self, decoder, max_batch, capacity, beam=4, length_bonus=0.0):
        self.decoder = decoder
        self.max_batch, self.capacity, self.beam, self.length_bonus = int(max_batch), int(capacity), int(beam), float(length_bonus)
        _slots.check_sizes('BeamDecoder', self, BEAM_MAX)
        wte = decoder.wte.weight
        dev, C, V, L = wte.device, wte.shape[1], decoder.lm_head.weight.shape[0], len(decoder.h)
        R, cap = self.max_batch * self.beam, self.capacity
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            # flat buffers, viewed per call at that call's N * W slots.  The beam's records exist twice (step parity): log-probabilities,
            # lengths, finished flags, tokens, ancestor rows
            self._rec = [(torch.zeros(R, **f32), torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros(R * cap, **i32),
                          torch.zeros(R * cap, **i32)) for _ in range(2)]
            self._rank = torch.zeros(R, **f32)
            self._time = torch.zeros(L * 2 * R * C * cap, device=dev, dtype=torch.float16)
            self._a, self._hid = torch.zeros(R * 4 * C, **f32), torch.zeros(R * 4 * C, **f32)
            self._att, self._logits = torch.zeros(R * 2 * C, **f32), torch.zeros(R * V, **f32)
            self._y, self._sa, self._sb = (torch.zeros(R * C, **f32) for _ in range(3))
        self._device = dev      # of the buffers: a decoder moved since needs a new BeamDecoder
        self._graphs = GraphCache()
        self.last_logprobs = self.last_finished = self.last_ctc = self._last_lm = None
        self._joint = None      # the joint search's buffers, allocated at its first use and again when S grows
        self._joint_S = 0

    def _joint_buffers(self, S):
        """The prefix states (two copies by step parity), psi of the candidates and of the slots, parents and last tokens: allocated
        once, for the largest S seen (graphs captured over the earlier buffers are dropped)."""
        if self._joint is None or S > self._joint_S:
            V = self.decoder.lm_head.weight.shape[0]
            R = self.max_batch * self.beam
            i32, f32 = dict(device=self._device, dtype=torch.int32), dict(device=self._device, dtype=torch.float32)
            with torch.inference_mode(False):
                self._joint = dict(state=[torch.zeros(R * S * 2, **f32) for _ in range(2)], cand=torch.zeros(R * V, **f32),
                                   psi=[torch.zeros(R, **f32) for _ in range(2)], par=torch.zeros(R, **i32),
                                   last=[torch.zeros(R, **i32) for _ in range(2)])
            self._joint_S = S
            self._graphs.entries = {k: v for k, v in self._graphs.entries.items() if 'joint' not in k}
        return self._joint

    @property
    def fused(self):
        return self.decoder._fused_decode_ok(self.decoder.wte.weight.shape[1])

    @torch.no_grad()
    def decode(self, features, input_lengths, capacity=None, beam=None, ctc_log_probs=None, ctc_weight=0.0):
        """features [N, S, C], input_lengths [N] -> (tokens [N, W, capacity] int64 without STX and ETX, -1 past a hypothesis's length
        and in absent hypotheses; lengths [N, W] int64, -1: absent; scores [N, W] float32 = the rank, best first, -inf: absent; counts
        [N] int64).  ``last_logprobs`` [N, W]: the plain log-probabilities; ``last_finished`` [N, W]: the hypothesis closed with ETX.
        ``capacity`` / ``beam``: search with less room than the buffers hold (default: all of it).
        ``ctc_log_probs`` [N, S, V] float32 (the CTC head's, V the decoder's) with ``ctc_weight`` in (0, 1]: the joint search; scores
        hold the joint rank, ``last_ctc`` [N, W] each hypothesis's psi (-inf: absent).  Without them the attention-only launches run."""
        return self._search(features, input_lengths, capacity, beam, ctc_log_probs, ctc_weight)

    @torch.no_grad()
    def _search(self, features, input_lengths, capacity, beam, ctc_log_probs, ctc_weight, side=None):
        """``decode``; ``side``: the LM side of ``fusion.AttentionFusionDecoder``, whose scores are kept as ``_last_lm``."""
        dec = self.decoder
        _require_inference(dec, features)
        if dec.wte.weight.device != self._device or features.device != self._device:
            raise ValueError('BeamDecoder: the decoder or the features are not on the device of the buffers')
        cap, W = _slots.room('BeamDecoder', self, capacity, beam)
        N, S, C = features.shape
        if N < 1 or N > self.max_batch:
            raise ValueError(f'BeamDecoder: {N} utterances outside 1 .. {self.max_batch}')
        c = float(ctc_weight)
        if not 0.0 <= c <= 1.0:
            raise ValueError(f'BeamDecoder: ctc_weight {c} outside 0 .. 1')
        x = None
        if ctc_log_probs is not None and c > 0.0:
            V = dec.lm_head.weight.shape[0]
            if ctc_log_probs.shape != (N, S, V) or ctc_log_probs.dtype != torch.float32 or ctc_log_probs.device != features.device:
                raise ValueError(f'BeamDecoder: ctc_log_probs must be float32 [{N}, {S}, {V}] on the device of the features')
            if S > PREFIX_MAX_FRAMES:
                raise ValueError(f'BeamDecoder: the joint search holds {PREFIX_MAX_FRAMES} frames at most, got {S}')
            x = ctc_log_probs.detach().contiguous()
            self._joint_buffers(S)
        with torch.no_grad():
            dev = features.device
            mlen = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
            mem2d = features.reshape(N * S, C).float().contiguous()
            if not (self.fused and (side is None or side.fused)):
                outs = self._core_general(mem2d, mlen, N, S, W, cap, x, c, side)
            elif os.environ.get('HALO_DECODE_GRAPH', '1') != '0':
                outs = self._graph(mem2d, mlen, N, S, W, cap, x, c, side)
            else:
                outs = tuple(t.clone() for t in self._core_fused(mem2d, mlen, N, S, W, cap, x, c, side))
            scores, lengths, fin, tokens, ranks = outs[:5]
            self.last_ctc = outs[5] if x is not None else None
            absent = ~(scores > float('-inf'))
            self._last_lm = torch.where(absent, torch.full_like(scores, float('-inf')), outs[-1]) if side is not None else None
            lengths = torch.where(absent, torch.full_like(lengths, -1), lengths).long()
            self.last_logprobs = scores
            self.last_finished = (fin != 0) & ~absent
            return _slots.mask_tokens(tokens[:, :, :cap], lengths), lengths, ranks, (~absent).sum(1)

    # ---- the fused path: 5 * layers + 2 launches per step --------------------------------------------------------------------------
    def _core_fused(self, mem2d, mlen, N, S, W, cap, x=None, c=0.0, side=None):
        """All launches of one search, host-sync free (capturable); returns views of the final beam's records (the joint search, x
        given: and of the slots' psi; with the LM ``side``: and of the slots' lm).  The LM side adds its selection in the place of the
        other two and, behind it, the LM's cell and out_layer launches for the next step: one linear chain on the one stream."""
        dec = self.decoder
        dev, C = mem2d.device, mem2d.shape[1]
        L, heads, head_dim = len(dec.h), dec.h[0].heads, dec.h[0].head_dim
        V = dec.lm_head.weight.shape[0]
        images = dec._decode_images()
        R, ld = N * W, self.capacity
        mem_cache = dec._memory_caches_fused(mem2d, N, S)                    # one per utterance, not per slot
        table = ops.RopeTable(cap, head_dim, dev)
        rec = [(s[:R].view(N, W), n[:R].view(N, W), f[:R].view(N, W), t[:R * ld].view(N, W, ld), a[:R * ld].view(R, ld))
               for s, n, f, t, a in self._rec]
        ranks = self._rank[:R].view(N, W)
        time_cache = self._time[:L * 2 * R * C * cap].view(L, 2, R, heads, cap, head_dim)
        a, hid = self._a[:R * 4 * C].view(R, 4 * C), self._hid[:R * 4 * C].view(R, 4 * C)
        att, logits = self._att[:R * 2 * C].view(R, 2 * C), self._logits[:R * V].view(R, V)
        y = self._y[:R * C].view(R, C)
        wte = dec.wte.weight.detach()
        y.copy_(wte[STX].expand(R, C))                                       # later steps: written by decode_beam_select
        sa, sb = (self._sa[:R * C].view(R, C), self._sb[:R * C].view(R, C)) if dec._decode_ksplit(C) else (None, None)
        if x is not None:
            jb = self._joint
            state = [b[:R * S * 2].view(R, S, 2) for b in jb['state']]
            psi_cand, par = jb['cand'][:R * V].view(R, V), jb['par'][:R].view(N, W)
            psi, last = [b[:R].view(N, W) for b in jb['psi']], [b[:R].view(N, W) for b in jb['last']]
            ops.ctc_prefix_advance(x, mlen, ETX, state[0])                   # the empty prefix's state into slot 0 of every utterance
        if side is not None:
            side.start(N, W)                                                 # the LM after its start token, in every slot
        for t in range(cap):
            q = t & 1
            y_next = y if t + 1 < cap else None
            dec._step_fused(images, y, a, att, hid, logits, sa, sb, lambda l: ops.decode_beam_attention(
                a, mem_cache[l, 0], mem_cache[l, 1], mlen, time_cache[l, 0], time_cache[l, 1], t + 1, rec[q][4], table, att))
            if x is None:
                if side is None:
                    ops.decode_beam_select(logits, t, cap, ETX, self.length_bonus, rec[q], rec[1 - q], ranks, wte, y_next)
                else:
                    side.select(logits, t, cap, self.length_bonus, rec[q], rec[1 - q], ranks, wte, y_next)
                    side.step(t, cap)
                continue
            s_in, n_in, f_in = rec[q][:3]
            ops.ctc_prefix_scores(x, mlen, state[q], t, ETX, psi_cand, last[q], n_in, s_in, f_in)
            if side is None:
                ops.decode_beam_select_joint(logits, t, cap, ETX, self.length_bonus, c, psi_cand, psi[q], psi[1 - q], rec[q], rec[1 - q],
                                             ranks, par, last[1 - q], wte, y_next)
            else:
                side.select(logits, t, cap, self.length_bonus, rec[q], rec[1 - q], ranks, wte, y_next, par, last[1 - q], c, psi_cand, psi[q],
                            psi[1 - q])
            if t + 1 < cap:                                                  # (the last beam's states are read by nobody)
                ops.ctc_prefix_advance(x, mlen, ETX, state[1 - q], state[q], par, last[1 - q], rec[1 - q][1], last[q])
            if side is not None:
                side.step(t, cap)
        s, n, f, tok, _ = rec[cap & 1]
        outs = (s, n, f, tok, ranks) if x is None else (s, n, f, tok, ranks, psi[cap & 1])
        return outs if side is None else outs + (side.scores(cap),)

    def _graph(self, mem2d, mlen, N, S, W, cap, x=None, c=0.0, side=None):
        """One HIP graph per (shape, width, parameter version), the sibling of ``Decoder._decode_graph``; the joint search has graphs of
        its own, with the log-probabilities copied into a static buffer, and so has the search with an LM side (keyed by the LM's
        parameter stamp, its weight, start token and end class; its decode images are built before the capture)."""
        key = (N, S, W, cap, self.length_bonus, str(mem2d.device), _lib.get_math_mode())
        if x is not None:
            key += ('joint', c)
        if side is not None:
            key += ('lm', side.key())
        entry = self._graphs.entry(self.decoder, key, lambda: (mem2d.clone(), mlen.clone()) + ((x.clone(),) if x is not None else ()),
                                   lambda static: self._core_fused(*static[:2], N, S, W, cap, static[2] if x is not None else None, c, side))
        for dst, src in zip(entry['static'], (mem2d, mlen, x)):
            dst.copy_(src)
        entry['graph'].replay()
        return tuple(o.clone() for o in entry['outs'])

    # ---- the general path: the same search on Decoder._decode_core's operators over N * W rows ---------------------------------------
    def _core_general(self, mem2d, mlen, N, S, W, cap, x=None, c=0.0, side=None):
        dec = self.decoder
        dev, C = mem2d.device, mem2d.shape[1]
        L, heads, head_dim = len(dec.h), dec.h[0].heads, dec.h[0].head_dim
        V = dec.lm_head.weight.shape[0]
        R = N * W
        utt = torch.arange(N, device=dev).repeat_interleave(W)
        mem_r = mem2d.view(N, S, C)[utt].reshape(R * S, C)
        mlen_r = mlen[utt].contiguous()
        mem_cache = dec._memory_caches_general(mem_r, R, S)
        time_cache = torch.zeros((L, 2, R, heads, cap, head_dim), dtype=torch.float16, device=dev)
        table = ops.RopeTable(cap, head_dim, dev)
        ninf = float('-inf')
        score = torch.full((N, W), ninf, device=dev)
        score[:, 0] = 0.0
        length = torch.zeros(N, W, dtype=torch.long, device=dev)
        fin = torch.zeros(N, W, dtype=torch.bool, device=dev)
        tokens = torch.zeros(N, W, cap, dtype=torch.long, device=dev)
        rank = torch.full((N, W), ninf, device=dev)
        cur = torch.full((R, 1), STX, dtype=torch.long, device=dev)
        is_label = (torch.arange(V, device=dev) != ETX)
        own = torch.arange(W, device=dev)[None, :].expand(N, W)
        if x is not None:      # the joint search: scores and advance from the launches of the fused path (fp32 in every mode)
            state = [torch.empty(R, S, 2, device=dev) for _ in range(2)]
            psi_cand, psi = torch.empty(R, V, device=dev), torch.full((N, W), ninf, device=dev)
            last = torch.zeros(N, W, dtype=torch.int32, device=dev)
            ops.ctc_prefix_advance(x, mlen, ETX, state[0])
        if side is not None:   # the LM side: rnn.Decoder.forward at T = 1 over the R rows, the states gathered by index_select
            lm, lm_w, lm_eos = side.lm, side.weight, side.eos
            lg, lstate = lm.forward(torch.full((1, R), side.start_token, dtype=torch.long, device=dev), lm.init_hidden(R))
            lms = torch.zeros(N, W, device=dev)                                               # (finite in absent slots: they rank -inf anyway)
        for t in range(cap):
            y = ops.embed_fwd(cur, dec.wte.weight, None)
            logits = dec._step_general(y, mem_cache, mlen_r, time_cache, t + 1, table)
            lp = torch.log_softmax(logits.float(), -1).view(N, W, V)
            present = score > ninf
            live, done = present & ~fin, present & fin
            cand = torch.where(live[:, :, None], score[:, :, None] + lp, torch.full_like(lp, ninf))
            cand[:, :, ETX] = torch.where(done, score, cand[:, :, ETX])                       # a finished slot: the one candidate (j, ETX)
            newlen = length[:, :, None] + (is_label[None, None, :] & live[:, :, None]).long()
            rk = cand + self.length_bonus * newlen.float()
            if x is not None:
                ops.ctc_prefix_scores(x, mlen, state[t & 1], t, ETX, psi_cand, last, length.int(), score.contiguous(), fin.int())
                pc = psi_cand.view(N, W, V).clone()
                pc[:, :, ETX] = torch.where(done, psi, pc[:, :, ETX])                         # a finished slot carries its psi
                rk = (1.0 - c) * rk + c * pc
            if side is not None:
                llp = torch.log_softmax(lg.float(), -1).view(N, W, V)
                lmc = lms[:, :, None] + llp
                lmc[:, :, ETX] = lms + llp[:, :, lm_eos] if lm_eos is not None else lms       # closing: the LM's end class, or nothing
                lmc[:, :, ETX] = torch.where(done, lms, lmc[:, :, ETX])
                rk = rk + lm_w * lmc
            rk = torch.where(rk.isnan(), torch.full_like(rk, ninf), rk)
            top, idx = rk.view(N, W * V).sort(dim=1, descending=True, stable=True)             # equal ranks: position ascending
            top, idx = top[:, :W], idx[:, :W]
            taken = top > ninf
            par, k = torch.where(taken, idx // V, own), idx % V
            pfin, plen = done.gather(1, par), length.gather(1, par)
            grow = taken & ~pfin & (k != ETX)
            tokens = tokens.gather(1, par[:, :, None].expand(N, W, cap))
            at = plen.clamp(max=cap - 1)[:, :, None]
            tokens.scatter_(2, at, torch.where(grow[:, :, None], k[:, :, None], tokens.gather(2, at)))
            score = torch.where(taken, cand.view(N, W * V).gather(1, idx), torch.full_like(top, ninf))
            rank = torch.where(taken, top, torch.full_like(top, ninf))
            length = torch.where(taken, plen + grow.long(), torch.zeros_like(plen))
            fin = taken & (pfin | (k == ETX))
            src = (torch.arange(N, device=dev)[:, None] * W + par).view(-1)
            time_cache = time_cache.index_select(2, src)                                      # the parent's history, physically
            cur = torch.where(taken, k, torch.full_like(k, ETX)).view(R, 1)
            if x is not None:
                psi = torch.where(taken, pc.view(N, W * V).gather(1, idx), torch.full_like(top, ninf))
                new_last = cur.view(N, W).int()
                if t + 1 < cap:
                    ops.ctc_prefix_advance(x, mlen, ETX, state[1 - (t & 1)], state[t & 1], torch.where(taken, par, -1).int(), new_last,
                                           length.int(), last)
                last = new_last
            if side is not None:
                lms = torch.where(taken, lmc.view(N, W * V).gather(1, idx), torch.zeros_like(top))
                if t + 1 < cap:                                                               # a slot that took a label: from its parent's state
                    step = grow.view(-1)
                    lg, lstate = _slots.step_general(lm, lg, lstate, src, torch.where(step, k.view(-1), torch.zeros_like(src)), step)
        outs = (score, length.int(), fin.int(), tokens.int(), rank) + ((psi,) if x is not None else ())
        return outs if side is None else outs + (lms,)


class CTCAttentionDecoder(nn.Module):
    "CTC loss on the encoder, CE loss on the decoder (ha/transformer.py:34-57)"
    def __init__(self, *, vocab: int, head_dim: int, heads: int, p_drop: float, layers: int):
        super().__init__()
        self.decoder = Decoder(vocab=vocab, head_dim=head_dim, heads=heads, p_drop=p_drop, layers=layers)
        self.recognizer = TemporalClassifier(feat_dim=head_dim * heads, vocab_size=vocab)
        self.joint = os.environ.get('HALO_ASR_JOINT', '0') == '1'         # decode(beam_size, ctc_weight): one-pass joint search

    def forward(self, features, condtargets, input_lengths=None, condtarget_lengths=None, star_penalty=None,
                measure_entropy=False, drop_labels=False):
        # remove prompts for CTC. we assume there is only one prompt token
        targets = condtargets[:, 1:]
        target_lengths = condtarget_lengths - 1 if condtarget_lengths is not None else None
        decoder_loss, decoder_stats = self.decoder(features, condtargets, input_lengths, condtarget_lengths, star_penalty,
                                                   measure_entropy, drop_labels)
        recognizer_loss, recognizer_stats = self.recognizer(features, targets, input_lengths, target_lengths, star_penalty)
        return decoder_loss + 0.3 * recognizer_loss, {**decoder_stats, **recognizer_stats}

    def decode(self, features, input_lengths, target_lengths, prompt=None, beam_size=None, ctc_weight=0.0, joint=None):
        """``Decoder.decode``.  With a beam (``beam_size`` or the decoder's attribute >= 1) and ``ctc_weight`` c > 0 the jointly trained
        CTC head rescores the final lists: they are re-ranked by (1 - c) * rank + c * (-ctc_loss(hypothesis)), ties in the old order,
        a hypothesis the lattice cannot spell (infinite loss) last; the search itself is unchanged.  ``last_nbest``: the re-ranked lists
        (scores = the joint score), ``last_parts`` = (attention ranks, CTC log-probabilities) [N, W] in the new order; the returned
        log-probability stays the decoder's own.
        ``joint=True`` (default: the attribute ``joint``, read from HALO_ASR_JOINT=1 when the module is built; off): the one-pass joint
        search instead (``BeamDecoder.decode`` with the head's log-probabilities) -- every candidate extension is ranked
        by (1 - c) * rank + c * its CTC prefix score while the search runs; ``last_nbest`` / ``last_parts`` as above, in the search's
        order.  It needs a beam and c > 0 (``joint=True`` without them: ValueError).  An LM set by ``decoder.set_fusion_lm`` takes part
        in the joint search alone (``last_parts`` = (attention, ctc, lm) then); greedy decoding and the re-ranking route do not use it."""
        width = self.decoder.beam_size if beam_size is None else int(beam_size)
        c = float(ctc_weight)
        if joint and (width < 1 or not c > 0.0):
            raise ValueError('CTCAttentionDecoder.decode(joint=True) needs beam_size >= 1 and ctc_weight > 0')
        if (self.joint if joint is None else bool(joint)) and width >= 1 and c > 0.0:
            if prompt is not None:
                raise NotImplementedError('CTCAttentionDecoder.decode(joint=True): prompts are not built')
            with torch.no_grad():
                _require_inference(self.decoder, features)
                lp =self.recognizer.log_probs(features).float()                             # [N, S, V]
                out = self.decoder._decode_beam(features, input_lengths, int(target_lengths.max().item()) + 1, width,
                                                ctc_log_probs=lp, ctc_weight=c)
                bd = self.decoder._beams[self.decoder._beams['used']]
                self.last_nbest = self.decoder.last_nbest
                lengths = self.last_nbest[1]
                if self.decoder.last_parts is not None:                                     # set_fusion_lm: (attention, ctc, lm)
                    self.last_parts = (self.decoder.last_parts[0], bd.last_ctc, self.decoder.last_parts[1])
                else:
                    self.last_parts = (bd.last_logprobs + float(self.decoder.length_bonus) * lengths.clamp(min=0).float(), bd.last_ctc)
            return out
        out = self.decoder.decode(features, input_lengths, target_lengths, prompt=prompt, beam_size=beam_size, fusion=False)
        if not width:
            return out
        self.last_nbest = self.decoder.last_nbest
        if not c > 0.0:
            return out
        from . import functional as HF
        tokens, lengths, ranks, counts = self.last_nbest
        bd = self.decoder._beams['decoder']
        N, W, cap = tokens.shape
        dev = features.device
        with torch.no_grad():
            lp = self.recognizer.log_probs(features)                                         # [N, S, V]
            S, V = lp.shape[1], lp.shape[2]
            rows = lp[:, None].expand(N, W, S, V).reshape(N * W, S, V)                       # one call over N * W rows, as mwer_forward does
            il = input_lengths.to(dev)[:, None].expand(N, W).reshape(-1)
            ctc = -HF.ctc_loss(rows.permute(1, 0, 2), tokens.clamp(min=0).view(N * W, cap), il, lengths.clamp(min=0).view(-1),
                               reduction='none').view(N, W)
            absent = lengths < 0
            joint = (1.0 - c) * ranks + c * ctc
            joint = torch.where(absent | joint.isnan(), torch.full_like(joint, float('-inf')), joint)
            # absent hypotheses stay behind the present ones, also behind those the lattice cannot spell: two stable sorts
            order = (-joint).argsort(dim=1, stable=True)
            order = order.gather(1, absent.gather(1, order).long().argsort(dim=1, stable=True))
            pick = lambda t: t.gather(1, order)
            tokens = tokens.gather(1, order[:, :, None].expand(N, W, cap))
            lengths, fin, logp = pick(lengths), pick(bd.last_finished), pick(bd.last_logprobs)
            self.last_nbest = (tokens, lengths, pick(joint), counts)
            self.last_parts = (pick(ranks), pick(ctc))
            out_len = lengths[:, 0].clamp(min=0) + fin[:, 0].long()
            lens = out_len.tolist()
            outputs = torch.nested.nested_tensor([tokens[i, 0, :max(n - 1, 0)] for i, n in enumerate(lens)])
            return outputs, out_len.to(input_lengths.dtype), [None] * N, logp[:, 0].clone(), out[4]


class AudioEncoder(nn.Module):
    def __init__(self, *, head_dim: int = 64, heads: int = 12, p_drop: float = 0.2, layers: int = 12, input_dim: int = 80,
                 conv_dim: int = 256, conv_strides: tuple = (2, 2, 2)):
        super().__init__()
        self.head_dim = head_dim
        self.heads = heads
        self.conv = ConvEncoder(input_dim=input_dim, hidden_dim=conv_dim, output_dim=head_dim * heads, strides=conv_strides)
        self.drop = nn.Dropout(p_drop)
        self.h = nn.ModuleList([Block(head_dim=head_dim, heads=heads, p_drop=p_drop) for _ in range(layers)])
        self.ln_f = LayerNorm(head_dim * heads, bias=False)
        self.dropout_stream = DropoutStream()
        self._graphs = GraphCache()                                       # captured inference forwards, see _forward_graph

    def subsampled_lengths(self, input_lengths):
        return self.conv.subsampled_lengths(input_lengths)

    def forward(self, x, input_lengths, measure_entropy=False):
        """x [N, T, F] -> (features [N, T', C], lengths int32, stats); no time mask, like the reference (:245-247)."""
        _check_device_and_dropout(self, x)
        if _wants_grad(self):
            if measure_entropy:
                raise NotImplementedError('measure_entropy is inference-only here: call under torch.no_grad()')
            out = _EncoderFn.apply(self, x, *[p for p in self.parameters() if p.requires_grad])
            ninf = [torch.tensor(float('-inf'))] * len(self.h)
            return out, self.conv.subsampled_lengths(input_lengths), Stats(meme_entropy=list(ninf), self_entropy=list(ninf))._asdict()
        out_lengths = self.conv.subsampled_lengths(input_lengths)
        if not measure_entropy and os.environ.get('HALO_ENCODER_GRAPH', '1') != '0':
            out = self._forward_graph(x.float().contiguous())
            ninf = [torch.tensor(float('-inf'))] * len(self.h)
            return out, out_lengths, Stats(meme_entropy=list(ninf), self_entropy=list(ninf))._asdict()
        out, stats = self._forward_core(x, measure_entropy)
        return out, out_lengths, stats._asdict()

    @torch.no_grad()
    def _forward_core(self, x, measure_entropy=False):
        y = self.conv.forward_cl(x)                                              # channels-last: no .mT round trip
        N, T, C = y.shape
        y2d = y.view(N * T, C)
        stats = Stats(meme_entropy=[], self_entropy=[])
        for block in self.h:
            m_ent, t_ent = block._forward2d(y2d, N, T, measure_entropy=measure_entropy)
            stats.meme_entropy.append(m_ent)
            stats.self_entropy.append(t_ent)
        return ops.layernorm_fwd(y2d, self.ln_f.weight).view(N, T, C), stats

    def _forward_graph(self, x):
        """Inference forward replayed from one HIP graph per (input shape, arithmetic mode, parameter version): the ~17 small
        launches per block are host-launch bound when issued eagerly."""
        key = (tuple(x.shape), str(x.device), _lib.get_math_mode())
        entry = self._graphs.entry(self, key, x.clone, lambda static: self._forward_core(static)[0])
        entry['static'].copy_(x)
        entry['graph'].replay()
        return entry['outs'].clone()

    @torch.no_grad()
    def _forward_train(self, x):
        y, conv_saved = self.conv._forward_cl_train(x)
        N, T, C = y.shape
        sites = DropSites(self.dropout_stream.next(_p_drop(self), self.training))
        s_in = sites.next()
        y2d = drop_rows(y.view(N * T, C), s_in)                                    # self.drop(x), ha/transformer.py:239
        blocks = []
        for block in self.h:
            y2d, sv = block._forward2d_train(y2d, N, T, sites=sites)
            blocks.append(sv)
        out = ops.layernorm_fwd(y2d, self.ln_f.weight)
        return out.view(N, T, C), (conv_saved, blocks, y2d, (N, T, C), s_in)

    @torch.no_grad()
    def _backward_train(self, saved, dout, put):
        conv_saved, blocks, y_last, (N, T, C), s_in = saved
        dy, dw, _ = ops.layernorm_bwd(dout.reshape(N * T, C), y_last, self.ln_f.weight)
        put(self.ln_f.weight, dw)
        for block, sv in zip(reversed(self.h), reversed(blocks)):
            dy = block._backward2d(sv, dy, put)
        self.conv._backward_cl(conv_saved, drop_rows(dy, s_in).view(N, T, C), put)
