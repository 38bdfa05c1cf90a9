"""Drop-in for the scoring path of ha/attention.py: GPT.forward_all (attention.py:205-232) and the
modules under it, forward only, on the HIP operators of csrc/gpt.hip and the GEMMs.

Same constructor (a config object with the GPTConfig fields of ha/init.py:25-36), same attribute
and state-dict names (``transformer.{wte,wpe}.weight``, ``transformer.h.{i}.{ln_1,attn.c_attn,
attn.c_proj,ln_2,mlp.c_fc,mlp.c_proj}``, ``transformer.ln_f``, tied ``lm_head.weight``), so
checkpoints load unchanged and ``hap`` (ha/score.py:72-73) can call ``forward_all(...,
reduction='none')`` as is.  Arithmetic is fp32 state with split-bf16 (bf16x3) or exact-f32 MFMA
GEMMs per ``halo_set_math_mode``; attention, LayerNorm, softmax and the loss are fp32.

Training: with grad enabled ``forward_all`` returns a loss with a ``grad_fn`` (one autograd.Function whose
backward is the hand-written HIP backward: cross-entropy, lm_head, LayerNorm, GELU, attention and embedding
gradients), so ``loss.backward()``, ``clip_grad_norm_`` and the optimizers of ha/attention_loop.py work unchanged.

Generation: ``forward(input_ids, past)`` / ``forward_context`` / ``generate`` keep the reference's fp32 KV cache
layout ``[L, 2, B, nh, T, hs]`` (attend_cached, ha/attention.py:64-93); attention reads the cache in place.

Training-mode dropout (config.dropout > 0): Philox masks at the reference's four kinds of site (embeddings, attention
probabilities inside the attention kernels, c_proj and MLP outputs as GEMM epilogues), see haloop_amd/transformer.py.

``stable_embedding`` (ha/attention.py:30-61: each embedding followed by its own LayerNorm) is built, forward and backward.

LoRA (haloop_amd/lora.py, ``hala --lora``): a ``c_attn`` that is a lora.Linear with an unmerged adapter adds its low-rank term at every
c_attn site below, and the backward computes a weight gradient only for parameters that require one (a frozen base pays for no
weight-gradient product).

Rotary blocks (``config.rotary_emb_dim`` equal to the head dimension: the reference's flash_attn ``MHA(rotary_emb_interleaved=True)``,
ha/attention.py:155-167, which its tests/test_flash_compat.py pins to ``rotate_interleaved`` on q and k, softmax scale 1/sqrt(head_dim),
``out_proj``): the attention module carries flash_attn's parameter names (``attn.Wqkv``, ``attn.out_proj``; ``attn.c_attn`` / ``attn.c_proj``
read the same two Linears, so the block forms below are stated once), the rotation is ONE ``ops.rope_rows_`` launch on the packed q | k | v
rows between the c_attn product and the attention launch of every form, and one inverse launch on dq | dk | dv in the backward (fp32
rows: ``HALO_ROPE_ROWS`` chooses between that launch and the scalar operator, one launch per tensor; DESIGN.md 3.3i has the default).  flash MHA
has no dropout behind ``out_proj``: a rotary block draws the c_proj site (the stream ids of every other site keep their numbering) and does
not apply it.  They are what haloop_amd.attention_audio's rotary encoders are built from.

Not built (raises NotImplementedError): a ``rotary_emb_dim`` other than the head dimension (no arch rotates part of a head), a rotary block
with a KV cache, ``GPT`` with rotary blocks (no arch builds one), LoRA on a rotary block.

The pre-LN block (ha/attention.py:147-180) is stated once per form, as a launch sequence:

- ``block_forward``: inference on the 128-tile products, the residual stream updated in place; with ``kv`` the new keys / values go into
  a cache and attention reads the cache.  GPT._trunk (scoring at few rows or in f32 / bf16x3, generation) and AudioEncoder.
- ``block_forward_train`` / ``block_backward`` (form IMAGES): training in any mode and shape, operand images of the activations.
- ``block_forward_train_rm`` / ``block_backward_rm``: training in `bf16` with row-major bf16 activations where ``rowmajor_train_ok``
  holds -- on ``halo_gemm_rows`` (form ROWS: ``rows_block_forward``, which is also GPT._trunk_rows' scoring block) where ``rows_ok``
  holds, else on the 128-tile products (form RM128).

Each training forward records its form in the BlockSaved it returns, and the backward reads the record.  The ``HALO_GPT_*`` switches and
``HALO_ROPE_ROWS`` are read by the predicates right below the imports and nowhere else.
"""
import math
import os
from collections import namedtuple
from dataclasses import dataclass, asdict

import torch
import torch.nn as nn

from . import _lib, lora, ops
from ._linear import (SMALL_M, DropSites, training_images, WeightImages, drop_rows, forward_images, grad_images, linear, linear_dw, linear_dx, rowmajor_ok,
                      ln_linear, use_split)
from .rnn import DropoutStream


# ---- the HALO_GPT_* switches of the block paths (README): read here and nowhere else, at call time; '0' is off ----------------------
def _switch(name, default):
    return os.environ.get(name, default) != '0'


def rowmajor_on(): return _switch('HALO_GPT_ROWMAJOR', '1')             # row-major bf16 activations in `bf16` training and scoring
def rows_on(): return _switch('HALO_GPT_ROWS', '1')                     # ... on the 256-row tiles of halo_gemm_rows
def attn_b16_on(): return _switch('HALO_GPT_ATTN_B16', '1')             # q | k | v kept as bf16 rows at head_dim 64
def dw_group_on(): return _switch('HALO_GPT_DW_GROUP', '1')             # a block's four weight gradients in one grouped launch
# built, measured, off: the epilogue's arithmetic is not covered at one workgroup per CU (13.57 against 13.45 ms per step on one box,
# DESIGN.md section 8); the bf16 gradient rows gain nothing (12.40 against 12.40 ms)
def gelu_epilogue_on(): return _switch('HALO_GPT_GELU_EPILOGUE', '0')   # new_gelu in the c_fc product's epilogue
def dln_b16_on(): return _switch('HALO_GPT_DLN_B16', '0')               # input gradients that only a LayerNorm backward reads as bf16 rows
# rotary blocks: q and k of fp32 rows rotated by ONE halo_rope_rows launch; '0': by the scalar operator, one launch each (bf16 rows have
# the one kernel).  Built, not yet measured against the two scalar launches on an MI355X: off until it is
def rope_rows_on(): return _switch('HALO_ROPE_ROWS', '0')


@dataclass
class GPTConfig:
    """ha/init.py:25-36."""
    block_size: int = 1024
    vocab_size: int = 50304
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    dropout: float = 0.0
    bias: bool = False
    stable_embedding: bool = False
    causal: bool = True
    d_input: int = 1
    rotary_emb_dim: int = 0

    def state_dict(self):
        return asdict(self)


@dataclass
class AudioEncoderConfig(GPTConfig):
    """ha/init.py:42-48."""
    block_size: int = 2048
    vocab_size: int = 128
    causal: bool = False
    d_input: int = 80
    rotary_emb_dim: int = 64


@dataclass
class StridingAudioEncoderConfig(GPTConfig):
    """ha/init.py:51-59."""
    block_size: int = 2048
    vocab_size: int = 16384
    causal: bool = False
    d_input: int = 80
    rotary_emb_dim: int = 64
    d_conv: int = 256
    conv_strides: tuple = (2, 2, 2)


def new_gelu(x):
    """Kept for surface parity (ha/attention.py:12-17); the fused path applies it in the GEMM epilogue."""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


class LayerNorm(nn.Module):
    def __init__(self, ndim, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(ndim))
        self.bias = nn.Parameter(torch.zeros(ndim)) if bias else None

    def forward(self, input):
        shp = input.shape
        return ops.layernorm_fwd(input.reshape(-1, shp[-1]).contiguous(), self.weight, self.bias, 1e-5).view(shp)


class StableEmbedding(nn.Embedding):
    """nn.Embedding followed by its own LayerNorm (ha/attention.py:30-61); GPT runs the gather and the norm on the HIP ops."""

    def __init__(self, num_embeddings, embedding_dim, **kw):
        super().__init__(num_embeddings, embedding_dim, **kw)
        self.norm = nn.LayerNorm(embedding_dim)

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        self._fill_padding_idx_with_zero()


class MonitoredSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        assert config.n_embd % config.n_head == 0
        self.c_attn = nn.Linear(config.n_embd, 3 * config.n_embd, bias=config.bias)
        self.c_proj = nn.Linear(config.n_embd, config.n_embd, bias=config.bias)
        self.resid_dropout = nn.Dropout(config.dropout)
        self.n_head, self.n_embd, self.dropout, self.causal = config.n_head, config.n_embd, config.dropout, config.causal


def check_rotary(config):
    """What a rotary config must satisfy to be built: the whole head is rotated."""
    if config.rotary_emb_dim and config.rotary_emb_dim != config.n_embd // config.n_head:
        raise NotImplementedError(f'rotary_emb_dim {config.rotary_emb_dim} is not the head dimension {config.n_embd // config.n_head}: partial '
                                  'rotations are not built (no arch of ha/init.py uses one; flash_attn asserts rotary_dim <= headdim)')
    if config.rotary_emb_dim % 8:
        raise NotImplementedError('rotary blocks need a head dimension that is a multiple of 8 (halo_rope_rows)')


class RotaryEmbedding(nn.Module):
    """The ``rotary_emb`` submodule of flash_attn's MHA as far as a state dict sees it: the non-persistent buffer ``inv_freq``.  Nothing
    here computes with it (the angles are ops.RopeTable's, rotate_interleaved's arithmetic); checkpoints written when the buffer was
    persistent still load with strict=True."""

    def __init__(self, dim, base=10000.0):
        super().__init__()
        self.register_buffer('inv_freq', 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim)), persistent=False)

    def _load_from_state_dict(self, state_dict, prefix, *args):
        state_dict.pop(prefix + 'inv_freq', None)
        super()._load_from_state_dict(state_dict, prefix, *args)


class RotarySelfAttention(nn.Module):
    """flash_attn.modules.mha.MHA(rotary_emb_dim=head_dim, rotary_emb_interleaved=True) as ha/attention.py:155-167 builds it: its parameter
    names, and the two Linears under the names the block forms read."""

    def __init__(self, config):
        super().__init__()
        assert config.n_embd % config.n_head == 0
        self.Wqkv = nn.Linear(config.n_embd, 3 * config.n_embd, bias=config.bias)
        self.out_proj = nn.Linear(config.n_embd, config.n_embd, bias=config.bias)
        self.rotary_emb = RotaryEmbedding(config.rotary_emb_dim)
        self.n_head, self.n_embd, self.dropout, self.causal = config.n_head, config.n_embd, config.dropout, config.causal

    c_attn = property(lambda self: self.Wqkv)
    c_proj = property(lambda self: self.out_proj)


class MLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.c_fc = nn.Linear(config.n_embd, 4 * config.n_embd, bias=config.bias)
        self.c_proj = nn.Linear(4 * config.n_embd, config.n_embd, bias=config.bias)
        self.dropout = nn.Dropout(config.dropout)


class Block(nn.Module):
    def __init__(self, config):
        super().__init__()
        check_rotary(config)
        self.rotary = bool(config.rotary_emb_dim)
        self.ln_1 = LayerNorm(config.n_embd, bias=config.bias)
        self.attn = RotarySelfAttention(config) if self.rotary else MonitoredSelfAttention(config)
        self.ln_2 = LayerNorm(config.n_embd, bias=config.bias)
        self.mlp = MLP(config)


# What a block's training forward keeps for its backward: which form ran, whether q | k | v were kept as bf16 rows (form ROWS only), that
# form's tensors (ImagesCore, or RowMajorCore for ROWS and RM128, which keep the same things) and the adapter's record (u, dropout site)
# when an unmerged LoRA adapter sat on c_attn, else None.
IMAGES, RM128, ROWS = 'images', 'rm128', 'rows'
BlockSaved = namedtuple('BlockSaved', 'form qkv_b16 core lora')
ImagesCore = namedtuple('ImagesCore', 'x0 h1 qkv y y_img_t lse x1 h2 a g g_img_t s_att s_res s_mlp')
RowMajorCore = namedtuple('RowMajorCore', 'x0 h1b qkv y yb lse x1 h2b a gb s_att')
# The head's record (GPT._head_train): which of its forms ran -- ROWS (halo_gemm_rows_ce, bf16 logits), SPLIT_CE (halo_gemm_split_ce) or DENSE
# -- the residual rows x it read, ln_f's rows, the logits and the rows' lse.  The whole step's holds the head's fields in line, in the
# order the step's tuple always had (positional readers keep working), then ``rec`` -- None on the dense path, the compaction record
# with a target capacity (x, xf, logits are then the compacted rows') -- and the head's form.
SPLIT_CE, DENSE = 'split_ce', 'dense'
HeadSaved = namedtuple('HeadSaved', 'x xf logits row_lse form')
StepSaved = namedtuple('StepSaved', 'input_ids targets blocks x xf logits row_lse s_emb emb rec head_form')


def adapter_dropout(blocks):
    """The largest lora_dropout of the unmerged adapters on ``blocks`` (0.0: none would draw a mask in a training forward)."""
    return max([blk.attn.c_attn.lora_dropout_p for blk in blocks if lora.is_active(blk.attn.c_attn)], default=0.0)


def train_sites(stream, p, training, blocks):
    """DropSites of one training forward over ``blocks``: the module's stream hands out one (seed, offset) per forward, shared by the
    existing sites (probability p) and the adapter sites (each adapter's own lora_dropout); the offset advances once per forward if
    either probability is positive."""
    p_lora = adapter_dropout(blocks) if training else 0.0
    if p_lora > 0.0 and stream.counter is not None:
        raise NotImplementedError('adapter dropout under a device-side step counter (captured graph steps) is not built')
    state = (stream.seed, stream.offset, stream.counter)
    drop = stream.next(p, training)
    if p_lora <= 0.0:
        return DropSites(drop)
    if drop is ops.NO_DROPOUT:
        stream.offset += 1
    return DropSites(drop, state)


# ---- the rotation of a rotary block's q and k -----------------------------------------------------------------------------------
_ROPE_TABLES = {}


def _rope_table(T, head_dim, device):
    """The cos / sin tables per (head_dim, device), grown on demand (as transformer._rope_table)."""
    hit = _ROPE_TABLES.get((head_dim, str(device)))
    if hit is None or hit.T < T:
        hit = ops.RopeTable(max(T, 256), head_dim, device)
        _ROPE_TABLES[(head_dim, str(device))] = hit
    return hit


def rope_qk_(blk, rows, T, cfg, inverse=False):
    """A rotary block: rotate_interleaved on the q and k column blocks of the packed rows [B*T, 3C] (fp32 or bf16), in place, row r at
    position r % T; ``inverse``: the backward, on dq | dk | dv.  Any other block: nothing."""
    if not blk.rotary:
        return
    if lora.is_active(blk.attn.c_attn):
        raise NotImplementedError('LoRA adapters on a rotary block are not built')
    C, H = cfg.n_embd, cfg.n_head
    table = _rope_table(T, C // H, rows.device)
    if rows.dtype == torch.float32 and not rope_rows_on():
        ops.rope_(rows[:, :C], T, H, C // H, table, inverse=inverse)
        ops.rope_(rows[:, C:2 * C], T, H, C // H, table, inverse=inverse)
    else:
        ops.rope_rows_(rows, T, H, C // H, table, inverse=inverse)


def res_site(blk, site):
    """The c_proj dropout site as the block applies it: flash MHA has no dropout behind out_proj, so a rotary block draws the site (the
    stream ids keep their numbering) and runs without it."""
    return (ops.NO_DROPOUT, site[1]) if blk.rotary else site


# ---- one pre-LN GPT block (ha/attention.py:147-180), shared by GPT and haloop_amd.attention_audio's encoders -------------------
def block_forward(images, blk, x, B, T, cfg, kv=None):
    """Inference: the residual stream x [B*T, C] is updated in place.  ``kv`` = (cache_k, cache_v, t0), one layer's fp32 cache
    [B, nh, Tc, hs] that holds positions [0, t0): the T new keys / values are stored behind them and attention runs over t0 + T keys."""
    C, H = cfg.n_embd, cfg.n_head
    if blk.rotary and kv is not None:
        raise NotImplementedError('a rotary block with a KV cache is not built (the cached keys would have to be kept rotated)')
    lo = lora.is_active(blk.attn.c_attn)
    qkv, h1 = ln_linear(images, x, blk.ln_1.weight, blk.ln_1.bias, blk.attn.c_attn.weight, bias=blk.attn.c_attn.bias, want_normed=lo)
    if lo:
        lora.lora_forward(blk.attn.c_attn, h1, qkv)
    rope_qk_(blk, qkv, T, cfg)
    if kv is not None:
        cache_k, cache_v, t0 = kv
        ops.kv_cache_store(qkv[:, C:], C, cache_k, cache_v, B, T, H, C // H, t0)
        y = ops.attention_cached_fwd(qkv, cache_k, cache_v, T, t0 + T, causal=cfg.causal)
    else:
        y, _, _ = ops.attention_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, H, C // H, T, T, causal=cfg.causal)
    linear(images, y, blk.attn.c_proj.weight, bias=blk.attn.c_proj.bias, out=x, accumulate=True)           # x += c_proj(y)
    # where it can, gelu(c_fc(ln_2(x))) leaves its GEMM as row-major bf16 (hi, lo) and the c_proj GEMM stages it from there: neither the
    # fp32 activations nor an operand image of them are written
    rm = rowmajor_ok(B * T, 4 * C, C) and C % 32 == 0
    h, _ = ln_linear(images, x, blk.ln_2.weight, blk.ln_2.bias, blk.mlp.c_fc.weight, bias=blk.mlp.c_fc.bias, gelu=True, out_rowmajor=rm)
    if rm:
        linear(images, None, blk.mlp.c_proj.weight, bias=blk.mlp.c_proj.bias, out=x, accumulate=True, a_rowmajor=h, shape=(B * T, 4 * C))
    else:
        linear(images, h, blk.mlp.c_proj.weight, bias=blk.mlp.c_proj.bias, out=x, accumulate=True)
    return x                                                                                              # x += mlp(x)


def prefetch_block_weights(images, blocks, M):
    """The weight images of every block's four Linears (forward image + the transposed one its backward reads) in a few multi-matrix
    launches at the head of a training forward, instead of one small launch per Linear on first use: they all went stale together
    at the optimizer step.  Only where linear() will take the split GEMM."""
    if _lib.get_math_mode() == 'f32' or M <= SMALL_M:
        return
    sets = [(w,) for blk in blocks for w in (blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight)
            if w.shape[0] >= 64 and w.shape[1] >= 64]
    images.prefetch_pairs(sets)


def block_forward_train(images, blk, x0, B, T, cfg, sites):
    """Training forward: returns (x_out, saved).  Dropout sites in forward order (ha/attention.py:90,127,141): attention
    probabilities, c_proj output, MLP output; the output dropouts are GEMM epilogues."""
    C, H = cfg.n_embd, cfg.n_head
    qkv, h1 = ln_linear(images, x0, blk.ln_1.weight, blk.ln_1.bias, blk.attn.c_attn.weight, bias=blk.attn.c_attn.bias, want_normed=True)
    s_att, s_res, s_mlp = sites.next(), res_site(blk, sites.next()), sites.next()
    lo = lora.is_active(blk.attn.c_attn)
    s_lo = sites.next_lora(blk.attn.c_attn.lora_dropout_p if lo else 0.0)
    lo_saved = (lora.lora_forward(blk.attn.c_attn, h1, qkv, s_lo), s_lo) if lo else None
    rope_qk_(blk, qkv, T, cfg)                               # (the saved qkv is the rotated one: what the attention backward needs)
    y, lse, _ = ops.attention_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, H, C // H, T, T, causal=cfg.causal, want_lse=True,
                                  drop=s_att[0], stream_id=s_att[1])
    # y and gelu(a) each feed one Linear now and its weight gradient later: both operand images come out of one read, and
    # gelu(a) is never written in fp32
    y_img, y_img_t = forward_images(y, C)
    x1 = linear(images, y, blk.attn.c_proj.weight, bias=blk.attn.c_proj.bias, residual=x0, drop=s_res[0],
                stream_id=s_res[1], a_image=y_img)
    a, h2 = ln_linear(images, x1, blk.ln_2.weight, blk.ln_2.bias, blk.mlp.c_fc.weight, bias=blk.mlp.c_fc.bias, want_normed=True)
    g_img, g_img_t = forward_images(a, C, ops.PAIR_GELU)
    g = ops.gelu_fwd(a) if g_img is None else None
    x = linear(images, g, blk.mlp.c_proj.weight, bias=blk.mlp.c_proj.bias, residual=x1, drop=s_mlp[0],
               stream_id=s_mlp[1], a_image=g_img, shape=a.shape)
    return x, BlockSaved(IMAGES, False, ImagesCore(x0, h1, qkv, y, y_img_t, lse, x1, h2, a, g, g_img_t, s_att, s_res, s_mlp), lo_saved)


def block_backward(images, blk, saved, dx, B, T, cfg, put, need_dx=True):
    """dx: gradient w.r.t. the block's output [B*T, C]; returns the gradient w.r.t. its input; parameter gradients go to put(p, g).
    A weight-gradient product runs only for a parameter that requires a gradient; ``need_dx`` False (nothing trainable below the block's
    c_attn): the block stops after c_attn's own gradients and returns None."""
    C, H = cfg.n_embd, cfg.n_head
    M = B * T
    img = images
    k = saved.core                                           # ImagesCore
    want = lambda p: p is not None and p.requires_grad
    # x = x1 + drop(c_proj(gelu(c_fc(ln_2(x1)))))
    dm = drop_rows(dx, k.s_mlp)
    dm_img, dm_img_t = grad_images(dm, 4 * C, want_dw=want(blk.mlp.c_proj.weight))
    if want(blk.mlp.c_proj.weight): put(blk.mlp.c_proj.weight, linear_dw(dm, k.g, dy_image_t=dm_img_t, x_image_t=k.g_img_t, shapes=(dm.shape, k.a.shape)))
    if want(blk.mlp.c_proj.bias): put(blk.mlp.c_proj.bias, ops.colsum(dm))
    dg = linear_dx(img, dm, blk.mlp.c_proj.weight, dy_image=dm_img)
    if blk.mlp.c_fc.bias is None and use_split(M, C, 4 * C) and use_split(4 * C, C, M):
        # da = dg * gelu'(a) is only ever a GEMM operand: write its two images, not the fp32 matrix
        da_img, da_img_t = ops.image_pair(dg, ops.PAIR_GELU_BWD, k.a, cols_image=want(blk.mlp.c_fc.weight))
        if want(blk.mlp.c_fc.weight): put(blk.mlp.c_fc.weight, linear_dw(None, k.h2, dy_image_t=da_img_t, shapes=(k.a.shape, k.h2.shape)))
        d_ln2 = linear_dx(img, None, blk.mlp.c_fc.weight, dy_image=da_img, shape=k.a.shape)
        del da_img, da_img_t
    else:
        da = ops.gelu_bwd(dg, k.a)
        if want(blk.mlp.c_fc.weight): put(blk.mlp.c_fc.weight, linear_dw(da, k.h2))
        if want(blk.mlp.c_fc.bias): put(blk.mlp.c_fc.bias, ops.colsum(da))
        d_ln2 = linear_dx(img, da, blk.mlp.c_fc.weight)
    dx1, dw, db = ops.layernorm_bwd(d_ln2, k.x1, blk.ln_2.weight, dx, blk.ln_2.bias is not None)
    put(blk.ln_2.weight, dw); put(blk.ln_2.bias, db)
    # x1 = x0 + drop(c_proj(attention(c_attn(ln_1(x0)))))
    dr = drop_rows(dx1, k.s_res)
    dr_img, dr_img_t = grad_images(dr, C, want_dw=want(blk.attn.c_proj.weight))
    if want(blk.attn.c_proj.weight): put(blk.attn.c_proj.weight, linear_dw(dr, k.y, dy_image_t=dr_img_t, x_image_t=k.y_img_t))
    if want(blk.attn.c_proj.bias): put(blk.attn.c_proj.bias, ops.colsum(dr))
    dy = linear_dx(img, dr, blk.attn.c_proj.weight, dy_image=dr_img)
    qkv = k.qkv
    dqkv = torch.empty_like(qkv)
    ops.attention_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], k.y, dy, k.lse, dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:],
                      B, H, C // H, T, T, causal=cfg.causal, drop=k.s_att[0], stream_id=k.s_att[1])
    rope_qk_(blk, dqkv, T, cfg, inverse=True)
    dq_img, dq_img_t = grad_images(dqkv, C, want_dx=need_dx, want_dw=want(blk.attn.c_attn.weight))
    if want(blk.attn.c_attn.weight): put(blk.attn.c_attn.weight, linear_dw(dqkv, k.h1, dy_image_t=dq_img_t))
    if want(blk.attn.c_attn.bias): put(blk.attn.c_attn.bias, ops.colsum(dqkv))
    d_ln1 = linear_dx(img, dqkv, blk.attn.c_attn.weight, dy_image=dq_img) if need_dx else None
    if saved.lora is not None:                               # the adapter: its gradients, and its share of d ln_1(x0)
        u, s_lo = saved.lora
        lora.lora_backward(blk.attn.c_attn, k.h1, u, dqkv, d_ln1, put, s_lo)
    if not need_dx:
        return None
    dx0, dw, db = ops.layernorm_bwd(d_ln1, k.x0, blk.ln_1.weight, dx1, blk.ln_1.bias is not None)
    put(blk.ln_1.weight, dw); put(blk.ln_1.bias, db)
    return dx0


# ---- the same block in `bf16` arithmetic with ROW-MAJOR bf16 activations between the launches (round 3) ---------------------------
# Every Linear's input and output gradient exist once, as row-major bf16 written by the launch that produced them (the LayerNorm
# kernels, the two GELU passes); the forward and input-gradient products stage
# their A operand from those rows (halo_gemm_split_io), the weight-gradient products read both operands from them and transpose on the way
# from LDS into the MFMA (halo_gemm_tn_bf16).  Gone against block_forward_train / block_backward: the four operand-image launches of the
# activations per block and direction (gelu pair, gelu-backward pair, dy pairs, transposed LayerNorm outputs) and the fp32 round trips of
# gelu(a)'s gradient and of the normalised rows.  Same bf16 operand values, same fp32 accumulation.
def rowmajor_train_ok(cfg, blocks, M, training):
    """bf16 arithmetic, no biases, no output dropout, enough rows that the products without split-K fill the chip."""
    if not rowmajor_on() or _lib.get_math_mode() != 'bf16':
        return False
    C = cfg.n_embd
    if cfg.bias or (training and cfg.dropout > 0.0) or M % 32 != 0 or C % 32 != 0 or not rowmajor_ok(M, 4 * C, C) or not rowmajor_ok(M, C, C):
        return False
    if C // cfg.n_head not in (32, 64):               # the matrix-core attention kernels write the bf16 outputs
        return False
    # (an unmerged adapter on c_attn rides along on the halo_lora_* kernels up to rank 16; a larger one takes the model to the general path)
    return all(blk.attn.c_attn.bias is None and blk.mlp.c_fc.bias is None
               and (not lora.is_active(blk.attn.c_attn) or lora.fast_ok(blk.attn.c_attn, M)) for blk in blocks)


def rows_ok(M, C):
    """The 256-row-tile products (halo_gemm_rows: single-pass bf16 arithmetic) take every Linear of a block of width C at M rows."""
    return rows_on() and ops.gemm_rows_supported(M, C, C) and C % 32 == 0


def rows_block_forward(images, blk, x, B, T, cfg, train=False, s_att=(ops.NO_DROPOUT, 0), s_lo=(ops.NO_DROPOUT, 0)):
    """The block with every activation-by-weight product on halo_gemm_rows (round 5: 256-row tiles cut to whole rounds of the CUs, A staged
    from the row-major bf16 rows the producing launch left); c_fc's result and the MLP's hidden activations stay bf16 (what the reference's
    autocast path holds there, ha/attention_loop.py:164) -- no fp32 [M, 4C] round trip between c_fc and new_gelu.
    Scoring (``train`` False): the fp32 residual stream x is updated in place by the products' residual epilogues -> (x, None).
    Training: x is left as it is, the attention launch also writes the rows' lse and takes the dropout site ``s_att``, the adapter its
    site ``s_lo`` -> (the block's output, BlockSaved)."""
    C, H, M = cfg.n_embd, cfg.n_head, B * T
    w = lambda lin: images.split((lin.weight,))
    h1b = ops.layernorm_bf16(x, blk.ln_1.weight, blk.ln_1.bias)
    # q | k | v stay bf16 between the c_attn product and the attention launches (forward and backward stage the rows as they are, two
    # tiles in flight: csrc/attn_b16.hip); the attention output is kept as bf16 only
    b16 = C // H == 64 and attn_b16_on()
    qkv = ops.gemm_rows(h1b, w(blk.attn.c_attn), M, 3 * C, C, out_bf16=b16)
    u = lora.lora_rows_forward(images, blk.attn.c_attn, h1b, qkv, s_lo) if lora.is_active(blk.attn.c_attn) else None
    rope_qk_(blk, qkv, T, cfg)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    if b16:
        y, lse, yb = ops.attention_fwd_b16(q, k, v, B, H, C // H, T, T, causal=cfg.causal, want_lse=train)
    else:
        y, lse, yb = ops.attention_fwd_bf16(q, k, v, B, H, C // H, T, T, causal=cfg.causal, drop=s_att[0], stream_id=s_att[1])
    x1 = ops.gemm_rows(yb, w(blk.attn.c_proj), M, C, C, out=None if train else x, residual=x)               # x + c_proj(y)
    h2b = ops.layernorm_bf16(x1, blk.ln_2.weight, blk.ln_2.bias)
    if gelu_epilogue_on():                                                    # new_gelu in the c_fc product's epilogue
        gb = ops.gemm_rows_gelu(h2b, w(blk.mlp.c_fc), M, 4 * C, C, keep_pre=train)
        gb, a = gb if train else (gb, None)                                   # (training keeps the pre-activation for gelu's backward)
    else:
        a = ops.gemm_rows(h2b, w(blk.mlp.c_fc), M, 4 * C, C, out_bf16=True)
        gb = ops.gelu_b16(a)
    x2 = ops.gemm_rows(gb, w(blk.mlp.c_proj), M, C, 4 * C, out=None if train else x1, residual=x1)          # x1 + mlp(x1)
    if not train:
        return x2, None
    return x2, BlockSaved(ROWS, b16, RowMajorCore(x, h1b, qkv, y, yb, lse, x1, h2b, a, gb, s_att), None if u is None else (u, s_lo))


def block_forward_train_rm(images, blk, x0, B, T, cfg, sites):
    """Training forward with row-major bf16 activations: rows_block_forward where rows_ok holds, else the 128-tile products below."""
    C, H, M = cfg.n_embd, cfg.n_head, B * T
    w = lambda lin: images.split((lin.weight,))
    rows = rows_ok(M, C)
    s_att, _, _ = sites.next(), sites.next(), sites.next()         # (the two output dropouts keep their ids: this path runs without them)
    lo = lora.is_active(blk.attn.c_attn)
    s_lo = sites.next_lora(blk.attn.c_attn.lora_dropout_p if lo else 0.0)
    if rows:
        _lib.lend_scratch(128 << 20, device=x0.device)      # K-slice slabs of the lm_head's input gradient and of the weight gradients' tails
        return rows_block_forward(images, blk, x0, B, T, cfg, True, s_att, s_lo)
    # (the normalised rows twice from one launch: the tiled image for the forward product, which stages an image 10-15 % faster than
    # rows from cold caches, and the row-major rows for the weight-gradient product)
    h1b, h1i = ops.layernorm_bf16(x0, blk.ln_1.weight, blk.ln_1.bias, want_image=True)
    qkv = ops.gemm_split(h1i, w(blk.attn.c_attn), M, 3 * C, C)
    del h1i
    lo_saved = (lora.lora_rows_forward(images, blk.attn.c_attn, h1b, qkv, s_lo), s_lo) if lo else None
    rope_qk_(blk, qkv, T, cfg)
    y, lse, yb = ops.attention_fwd_bf16(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, H, C // H, T, T, causal=cfg.causal,
                                        drop=s_att[0], stream_id=s_att[1])
    x1 = ops.gemm_split_io((yb, None), w(blk.attn.c_proj), M, C, C, residual=x0)
    h2b, h2i = ops.layernorm_bf16(x1, blk.ln_2.weight, blk.ln_2.bias, want_image=True)
    a = ops.gemm_split(h2i, w(blk.mlp.c_fc), M, 4 * C, C)
    del h2i
    gb = ops.gelu_bf16(a)
    x = ops.gemm_split_io((gb, None), w(blk.mlp.c_proj), M, C, 4 * C, residual=x1)
    return x, BlockSaved(RM128, False, RowMajorCore(x0, h1b, qkv, y, yb, lse, x1, h2b, a, gb, s_att), lo_saved)


def block_backward_rm(images, blk, saved, dx, dxb, B, T, cfg, put, need_dx=True):
    """dx / dxb: the gradient w.r.t. the block's output as fp32 and as row-major bf16 -> the same pair for its input ((None, None) with
    ``need_dx`` False: nothing trainable below the block's c_attn).  Weight-gradient products only for parameters that require one."""
    C, H, M = cfg.n_embd, cfg.n_head, B * T
    k = saved.core                                       # RowMajorCore
    rows = saved.form == ROWS                            # the forward ran on halo_gemm_rows
    # the four weight gradients contract over the same M token rows: collected here, ONE grouped launch at the end of the block
    # (whole-K tiles, no K-slices or reduce launches); HALO_GPT_DW_GROUP=0: one launch each, as round 4
    grouped = dw_group_on() and M % 32 == 0
    # the two input gradients that only a LayerNorm backward reads leave their products as bf16 rows (that launch adds the fp32 residual
    # gradient to them in fp32)
    b16_ln = rows and C % 4 == 0 and C <= 2048 and dln_b16_on()
    todo = []

    def dweight(p, dy_b, x_b):
        if not p.requires_grad:
            return
        if grouped:
            todo.append((p, dy_b, x_b))
        else:
            put(p, ops.gemm_tn(dy_b, x_b))

    def dinput(dy_b, lin, N, K, out_bf16=False):
        """dy_b [M, K] (bf16 rows) times lin's weight [K, N]: the input gradient [M, N], on the tiles the forward ran on; ``out_bf16``
        (form ROWS only): as bf16 rows."""
        if rows:
            return ops.gemm_rows(dy_b, images.split_t((lin.weight,)), M, N, K, out_bf16=out_bf16)
        return ops.gemm_split_io((dy_b, None), images.split_t((lin.weight,)), M, N, K)
    # x = x1 + c_proj(gelu(c_fc(ln_2(x1))))
    dweight(blk.mlp.c_proj.weight, dxb, k.gb)
    # d a = (dx W) gelu'(a); form ROWS: bf16 throughout
    dab = (ops.gelu_bwd_b16 if rows else ops.gelu_bwd_bf16)(dinput(dxb, blk.mlp.c_proj, 4 * C, C, out_bf16=True), k.a)
    dweight(blk.mlp.c_fc.weight, dab, k.h2b)
    d_ln2 = dinput(dab, blk.mlp.c_fc, C, 4 * C, out_bf16=b16_ln)
    dx1, dw, db, dx1b = ops.layernorm_bwd(d_ln2, k.x1, blk.ln_2.weight, dx, blk.ln_2.bias is not None, want_bf16=True)
    put(blk.ln_2.weight, dw); put(blk.ln_2.bias, db)
    # x1 = x0 + c_proj(attention(c_attn(ln_1(x0))))
    dweight(blk.attn.c_proj.weight, dx1b, k.yb)
    qkv = k.qkv
    dqkvb = torch.empty(M, 3 * C, device=dx.device, dtype=torch.bfloat16)
    dy = dinput(dx1b, blk.attn.c_proj, C, C, out_bf16=saved.qkv_b16)
    if saved.qkv_b16:                                    # the forward kept q | k | v as bf16 rows: the output gradient arrives as bf16 rows too
        ops.attention_bwd_b16(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], k.yb, dy, k.lse, dqkvb[:, :C], dqkvb[:, C:2 * C], dqkvb[:, 2 * C:],
                              B, H, C // H, T, T, causal=cfg.causal)
    else:
        ops.attention_bwd_bf16(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], k.y, dy, k.lse, dqkvb[:, :C], dqkvb[:, C:2 * C], dqkvb[:, 2 * C:],
                               B, H, C // H, T, T, causal=cfg.causal, drop=k.s_att[0], stream_id=k.s_att[1])
    rope_qk_(blk, dqkvb, T, cfg, inverse=True)
    dweight(blk.attn.c_attn.weight, dqkvb, k.h1b)
    d_ln1 = dinput(dqkvb, blk.attn.c_attn, C, 3 * C, out_bf16=b16_ln) if need_dx else None
    if saved.lora is not None:                           # the adapter: its gradients, and its share of d ln_1(x0)
        u, s_lo = saved.lora
        lora.lora_rows_backward(images, blk.attn.c_attn, k.h1b, u, dqkvb, d_ln1, put, s_lo)
    dx0 = dx0b = None
    if need_dx:
        dx0, dw, db, dx0b = ops.layernorm_bwd(d_ln1, k.x0, blk.ln_1.weight, dx1, blk.ln_1.bias is not None, want_bf16=True)
        put(blk.ln_1.weight, dw); put(blk.ln_1.bias, db)
    if todo:
        for (p, _, _), g in zip(todo, ops.gemm_tn_group([(d, x_) for _, d, x_ in todo])):
            put(p, g)
    return dx0, dx0b


class _GPTLoss(torch.autograd.Function):
    """Per-token NLL of GPT.forward_all with its hand-written backward (the autograd graph the reference gets from
    torch for ha/attention.py:205-232).  The parameters ride along as inputs so that loss.backward() fills their
    .grad exactly like the reference's, and clip_grad_norm_ / the optimizer of ha/attention_loop.py:203-215 work as is."""

    @staticmethod
    def forward(ctx, model, input_ids, target_ids, *params):
        with training_images():
            per_tok, saved = model._forward_train(input_ids, target_ids)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        return per_tok

    @staticmethod
    def backward(ctx, grad_per_tok):
        grads = ctx.model._backward_train(ctx.saved, grad_per_tok.contiguous().float())
        ctx.saved = None
        return (None, None, None) + tuple(grads.get(id(p)) for p in ctx.params)


class GPT(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        if config.rotary_emb_dim:
            raise NotImplementedError('a GPT of rotary blocks is not built (no arch of ha/init.py builds one): positions come from wpe')
        self.transformer = nn.ModuleDict(dict(
            wte=(StableEmbedding if config.stable_embedding else nn.Embedding)(config.vocab_size, config.n_embd),
            wpe=(StableEmbedding if config.stable_embedding else nn.Embedding)(config.block_size, config.n_embd),
            drop=nn.Dropout(config.dropout),
            h=nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
            ln_f=LayerNorm(config.n_embd, bias=config.bias),
        ))
        with torch.no_grad():
            self.transformer.wpe.weight.mul_(0)
            self.transformer.wte.weight.mul_(0.02)
        self.lm_head = nn.Linear(config.n_embd, config.vocab_size, bias=False)
        self.transformer.wte.weight = self.lm_head.weight       # weight tying
        self._images = WeightImages()
        self.dropout_stream = DropoutStream()                   # Philox (seed, offset) per training forward
        self._target_capacity = None                            # set_target_capacity: not part of the state dict

    def set_target_capacity(self, rows):
        """``rows``: forward_all compacts the first ``rows`` token rows whose target is non-zero, in ascending order, and runs ln_f, the
        lm_head, the cross-entropy and their backward on those rows only -- the masked objectives ("denoise":
        symbol_tape.target_capacity(B, T); "cond": B), where F.cross_entropy(ignore_index=0) ignores every other row.  Every shape is set
        by the capacity, none by the count, and nothing returns to the host.  More targets than ``rows``: every per-token loss of that
        call is NaN.  None (the default): the dense path.  Ignored with ``past``."""
        if rows is not None and (int(rows) != rows or rows <= 0):
            raise ValueError(f'target capacity must be a positive number of rows or None, got {rows!r}')
        self._target_capacity = None if rows is None else int(rows)

    def _compact_rows(self, M):
        """(compact rows K, targets allowed for) of a call with M token rows under the set capacity.  K is the capacity rounded up to a
        multiple of 32 (the weight-gradient products' contraction step) and, where the dense head runs above the small-M gate, to the
        first such count above it too: at or below SMALL_M rows the head's products would fall to the exact-f32 kernel and a contraction
        shorter than 64 rows takes its weight gradient there as well, so a small capacity would change the head's arithmetic against
        the dense path's in the bf16x3 / bf16 modes.  The padding rows cost nothing that matters at that size."""
        limit = self._target_capacity
        K = (limit + 31) // 32 * 32
        if M > SMALL_M:
            K = max(K, (SMALL_M + 1 + 31) // 32 * 32)
        return K, limit

    # ---- one Linear: y = x W^T + b, with the epilogue fused ------------------------------------
    def _linear(self, x2d, lin, out=None, gelu=False, accumulate=False, site=(ops.NO_DROPOUT, 0), a_image=None, shape=None):
        return linear(self._images, x2d, lin.weight, bias=lin.bias, out=out, gelu=gelu, accumulate=accumulate, drop=site[0],
                      stream_id=site[1], a_image=a_image, shape=shape)

    def _embed(self, input_ids, t0=0, keep=False):
        """tok_emb + pos_emb [B*T, C]; with stable_embedding each goes through its own LayerNorm first.  keep: also return
        what the backward needs (raw token rows, raw position rows)."""
        tr = self.transformer
        if not self.config.stable_embedding:
            return ops.embed_fwd(input_ids, tr.wte.weight, tr.wpe.weight, t0), None
        T = input_ids.shape[1]
        et = ops.embed_fwd(input_ids, tr.wte.weight, None)
        ep = tr.wpe.weight.detach()[t0:t0 + T].contiguous()
        x = ops.layernorm_fwd(et, tr.wte.norm.weight, tr.wte.norm.bias)
        ops.add_rows_bcast_(x, ops.layernorm_fwd(ep, tr.wpe.norm.weight, tr.wpe.norm.bias), T)
        return x, ((et, ep) if keep else None)

    @torch.no_grad()
    def _trunk(self, input_ids, past=None, want_present=False, cache=None, t0=0, want_residual=False):
        """Embedding + blocks + ln_f.  With ``past`` [L, 2, B, nh, T0, hs] (or want_present) keys/values go through a
        fp32 cache in the reference's layout (attend_cached, ha/attention.py:64-93) and ``present`` is returned.
        ``cache`` [L, 2, B, nh, Tc, hs] (haloop_amd.generation): a preallocated cache that already holds positions [0, t0); the T new
        positions are stored behind them in place, nothing is allocated or copied, and ``cache`` itself is returned as ``present``.
        ``want_residual``: the residual stream before ln_f in place of ln_f's output."""
        cfg = self.config
        B, T = input_ids.shape
        if cache is None:
            t0 = 0 if past is None else past.size(-2)
        assert t0 + T <= cfg.block_size, f'Cannot forward sequence of length {t0 + T}, block size is only {cfg.block_size}'
        C, H = cfg.n_embd, cfg.n_head
        tr = self.transformer
        x, _ = self._embed(input_ids, t0)                                                # [B*T, C], the residual stream
        present = cache
        if cache is None and (past is not None or want_present):
            present = torch.empty(cfg.n_layer, 2, B, H, t0 + T, C // H, device=x.device, dtype=torch.float32)
            if t0:
                present[..., :t0, :] = past
        for i, blk in enumerate(tr.h):
            block_forward(self._images, blk, x, B, T, cfg, None if present is None else (present[i, 0], present[i, 1], t0))
        if want_residual:
            return x, present
        return ops.layernorm_fwd(x, tr.ln_f.weight, tr.ln_f.bias), present

    @torch.no_grad()
    def _trunk_rows(self, input_ids):
        """Embedding + blocks in single-pass bf16 arithmetic on halo_gemm_rows (scoring without a KV cache): the residual stream fp32,
        updated in place by the products' residual epilogues; every Linear input row-major bf16.  -> the residual stream before ln_f."""
        cfg = self.config
        B, T = input_ids.shape
        assert T <= cfg.block_size, f'Cannot forward sequence of length {T}, block size is only {cfg.block_size}'
        x, _ = self._embed(input_ids, 0)
        for blk in self.transformer.h:
            rows_block_forward(self._images, blk, x, B, T, cfg)
        return x

    def forward_all(self, input_ids, target_ids, past=None, reduction='mean'):
        if not input_ids.is_cuda:
            raise _lib.HaloError('haloop_amd.attention.GPT runs on the HIP device only (no CPU path)')
        B, T = input_ids.shape
        V = self.config.vocab_size
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if past is not None:
                raise NotImplementedError('training through a KV-cache continuation is not built: call under torch.no_grad()')
            params = [p for p in self.parameters() if p.requires_grad]
            loss = _GPTLoss.apply(self, input_ids, target_ids, *params)          # per-token NLL with a grad_fn
            return self._reduce(loss, target_ids.reshape(-1), reduction)
        if self.training and (self.config.dropout > 0 or adapter_dropout(self.transformer.h) > 0):
            raise NotImplementedError('training-mode dropout is built into the autograd path only: enable grad, or call .eval()')
        targets = target_ids.reshape(-1)
        C, M = self.config.n_embd, B * T
        rows = past is None and M > SMALL_M and V % 8 == 0 and rows_ok(M, C) and rowmajor_train_ok(self.config, self.transformer.h, M, False)
        x = self._trunk_rows(input_ids) if rows else self._trunk(input_ids, past, want_residual=True)[0]
        if past is None and self._target_capacity is not None:
            # the masked objectives: ln_f, the lm_head and the loss on the K compacted target rows (_compact_rows), the head's product path
            # chosen from K by the predicates the dense path applies to M; the per-token losses go back to their rows
            K, limit = self._compact_rows(M)
            rec = ops.target_rows(targets, K, ignore_index=0, limit=limit)
            x_c = ops.gather_rows(x, rec.rows)
            loss = ops.scatter_rows(self._score_head(x_c, rec.targets, rows and K > SMALL_M and rows_ok(K, C)), rec, M)
        else:
            loss = self._score_head(x, targets, rows)
        return self._reduce(loss, targets, reduction)

    def _split_head(self, R):
        """The lm_head product of R rows runs on the split GEMM with the cross-entropy statistics in its epilogue."""
        return use_split(R, self.config.vocab_size, self.config.n_embd) and R > SMALL_M

    def _score_head(self, x, targets, rows):
        """Per-row NLL of lm_head(ln_f(x)) for the residual rows x [R, C] (no grad); the [R, V] logits are never written where the loss
        comes out of a GEMM's epilogue.  ``rows``: ln_f's rows as row-major bf16 into halo_gemm_rows_ce."""
        tr = self.transformer
        R, C = x.shape
        V = self.config.vocab_size
        if rows:
            loss, _, _ = ops.gemm_rows_ce(ops.layernorm_bf16(x, tr.ln_f.weight, tr.ln_f.bias), self._images.split((self.lm_head.weight,)), R, V, C,
                                          targets, ignore_index=0)
            return loss
        xf = ops.layernorm_fwd(x, tr.ln_f.weight, tr.ln_f.bias)
        if self._split_head(R):
            loss, _, _ = ops.gemm_split_ce(ops.split_image(xf), self._images.split((self.lm_head.weight,)), R, V, C, targets, ignore_index=0)
            return loss
        # otherwise in row chunks so the logits stay bounded (206 MB per 1024 rows at V=50304)
        loss = torch.empty(R, device=xf.device, dtype=torch.float32)
        chunk = max(64, min(R, (1 << 28) // (4 * V)))
        for r0 in range(0, R, chunk):
            r1 = min(R, r0 + chunk)
            logits = self._linear(xf[r0:r1], self.lm_head)
            loss[r0:r1] = ops.cross_entropy_fwd(logits, targets[r0:r1], ignore_index=0)
        return loss

    @staticmethod
    def _reduce(loss, targets, reduction):
        if reduction == 'none':
            return loss
        if reduction == 'sum':
            return loss.sum()
        if reduction == 'mean':
            return loss.sum() / (targets != 0).sum()
        raise ValueError(f'unknown reduction {reduction!r}')

    # ---- training: forward that keeps what the backward needs, and the backward itself -------------------------
    @torch.no_grad()
    def _forward_train(self, input_ids, target_ids):
        cfg = self.config
        B, T = input_ids.shape
        assert T <= cfg.block_size, f'Cannot forward sequence of length {T}, block size is only {cfg.block_size}'
        tr = self.transformer
        # dropout sites in forward order (ha/attention.py:224,90,127,141): embeddings, then per block the attention
        # probabilities, the c_proj output and the MLP output; output dropouts are GEMM epilogues
        sites = train_sites(self.dropout_stream, cfg.dropout, self.training, tr.h)
        s_emb = sites.next()
        x, emb_saved = self._embed(input_ids, 0, keep=True)
        x = drop_rows(x, s_emb)
        blocks = []
        prefetch_block_weights(self._images, tr.h, B * T)
        fwd = block_forward_train_rm if rowmajor_train_ok(cfg, tr.h, B * T, self.training) else block_forward_train
        for blk in tr.h:
            x, sv = fwd(self._images, blk, x, B, T, cfg, sites)
            blocks.append(sv)
        targets, rec = target_ids.reshape(-1), None
        if self._target_capacity is not None:
            # the masked objectives: ln_f, the lm_head and the loss on the compacted target rows; the per-token losses go back to their rows
            K, limit = self._compact_rows(B * T)
            rec = ops.target_rows(targets, K, ignore_index=0, limit=limit)
            x, targets = ops.gather_rows(x, rec.rows), rec.targets
        loss, head = self._head_train(x, targets, fwd is block_forward_train_rm)
        if rec is not None:
            loss = ops.scatter_rows(loss, rec, B * T)
        return loss, StepSaved(input_ids, targets, blocks, head.x, head.xf, head.logits, head.row_lse, s_emb, emb_saved, rec, head.form)

    def _head_train(self, x, targets, rm):
        """ln_f, the lm_head and the per-row cross-entropy on the residual rows x [R, C] -> (loss [R], HeadSaved for _head_backward).
        ``rm``: the blocks ran block_forward_train_rm."""
        cfg, tr = self.config, self.transformer
        R, C = x.shape
        V = cfg.vocab_size
        if rm and rows_ok(R, C) and ops.gemm_rows_supported(R, V, C) and ops.gemm_rows_supported(R, C, V):
            # round 5: ln_f's rows as row-major bf16, the lm_head product on halo_gemm_rows with the cross-entropy statistics in its
            # epilogue (from the fp32 accumulators) and the logits KEPT AS bf16 (1.65 GB of fp32 at B = 8, T = 1024 no longer written).
            # Only when the backward's input-gradient product (K = V) runs on halo_gemm_rows too: V % 32 == 0.
            _lib.lend_scratch(128 << 20, device=x.device)       # (the blocks lent it already unless only the compacted rows take this path)
            xf = ops.layernorm_bf16(x, tr.ln_f.weight, tr.ln_f.bias)
            loss, row_lse, logits = ops.gemm_rows_ce(xf, self._images.split((self.lm_head.weight,)), R, V, C, targets,
                                                     ignore_index=0, want_logits=True, want_lse=True)
            return loss, HeadSaved(x, xf, logits, row_lse, ROWS)
        xf = ops.layernorm_fwd(x, tr.ln_f.weight, tr.ln_f.bias)
        if self._split_head(R):                         # statistics in the GEMM epilogue; the logits are kept for the backward
            loss, row_lse, logits = ops.gemm_split_ce(ops.split_image(xf), self._images.split((self.lm_head.weight,)), R, V, C,
                                                      targets, ignore_index=0, want_logits=True, want_lse=True)
            return loss, HeadSaved(x, xf, logits, row_lse, SPLIT_CE)
        logits = self._linear(xf, self.lm_head)
        loss, row_lse = ops.cross_entropy_fwd_lse(logits, targets, ignore_index=0)
        return loss, HeadSaved(x, xf, logits, row_lse, DENSE)

    def _head_backward(self, saved, targets, grad_rows, head, want_bf16, put):
        """The backward of _head_train (``saved``: its HeadSaved) on its R rows: -> (d x [R, C], [the same as row-major bf16] with
        ``want_bf16``, the lm_head's weight gradient [V, C] or None with ``head`` False); ln_f's gradients go to put."""
        tr, img = self.transformer, self._images
        xf, logits, row_lse = saved.xf, saved.logits, saved.row_lse
        M, V = logits.shape
        C = self.config.n_embd
        if saved.form == ROWS:
            # the stored bf16 logits become d loss / d logits IN PLACE: the row-major bf16 operand of both gradient products
            dl = ops.cross_entropy_bwd_bf16_(logits, targets, row_lse, grad_rows, ignore_index=0)
            dw_head = ops.gemm_tn_group([(dl, xf)])[0] if head else None                     # [V, C]; the tied wte gradient lands here too
            dxf = ops.gemm_rows(dl, img.split_t((self.lm_head.weight,)), M, C, V)
            del dl, logits
        elif use_split(M, C, V) and use_split(V, C, M):
            # d loss / d logits goes straight into the two operand images of the lm_head's backward products
            dl_img, dl_img_t = ops.cross_entropy_bwd_images(logits, targets, row_lse, grad_rows, ignore_index=0)
            dw_head = linear_dw(None, xf, dy_image_t=dl_img_t, shapes=((M, V), xf.shape)) if head else None    # [V, C]; the tied wte gradient lands here too
            dxf = linear_dx(img, None, self.lm_head.weight, dy_image=dl_img, shape=(M, V))
            del dl_img, dl_img_t
        else:
            dlogits = ops.cross_entropy_bwd_(logits, targets, row_lse, grad_rows, ignore_index=0)
            dw_head = linear_dw(dlogits, xf) if head else None
            dxf = linear_dx(img, dlogits, self.lm_head.weight)
        dx, dw, db, *dxb = ops.layernorm_bwd(dxf, saved.x, tr.ln_f.weight, None, tr.ln_f.bias is not None, want_bf16=want_bf16)
        put(tr.ln_f.weight, dw); put(tr.ln_f.bias, db)
        return dx, dxb, dw_head

    @torch.no_grad()
    def _backward_train(self, saved, grad_per_tok):
        cfg = self.config
        input_ids, blocks, rec = saved.input_ids, saved.blocks, saved.rec
        B, T = input_ids.shape
        tr = self.transformer
        img = self._images
        grads = {}

        def put(p, g):
            if p is not None and p.requires_grad:
                grads[id(p)] = g if id(p) not in grads else grads[id(p)] + g

        # what is trainable at and below each point of the backward: a frozen parameter gets no weight-gradient product, and the sweep
        # stops at the lowest block whose c_attn adapters are the last trainable thing
        live = lambda mod: any(p.requires_grad for p in mod.parameters())
        head, emb = self.lm_head.weight.requires_grad, live(tr.wte) or live(tr.wpe)
        below = [emb]
        for blk in tr.h:
            below.append(below[-1] or live(blk))
        rm = len(blocks) > 0 and blocks[0].form != IMAGES       # block_forward_train_rm's records
        head_saved = HeadSaved(saved.x, saved.xf, saved.logits, saved.row_lse, saved.head_form)
        if rec is not None:
            # the head ran on the compacted target rows: their share of grad_per_tok in, their d x back to its rows (zero elsewhere)
            dx_c, _, dw_head = self._head_backward(head_saved, saved.targets, ops.gather_rows(grad_per_tok, rec.rows), head, False, put)
            dx, *dxb = ops.scatter_rows(dx_c, rec, B * T, want_bf16=True) if rm else (ops.scatter_rows(dx_c, rec, B * T),)
        else:
            dx, dxb, dw_head = self._head_backward(head_saved, saved.targets, grad_per_tok, head, rm, put)
        for i in reversed(range(len(blocks))):
            blk, sv = tr.h[i], blocks[i]
            need_dx = below[i] or live(blk.ln_1)
            if not (need_dx or live(blk)):
                break
            if rm:
                dx, dxb[0] = block_backward_rm(img, blk, sv, dx, dxb[0], B, T, cfg, put, need_dx)
            else:
                dx = block_backward(img, blk, sv, dx, B, T, cfg, put, need_dx)
            if not need_dx:
                break
        if not emb:
            return grads
        # (a frozen lm_head / wte or wpe takes no scatter: dw_head is None then, and the embedding kernels skip a NULL target)
        dwpe = torch.zeros_like(tr.wpe.weight) if tr.wpe.weight.requires_grad else None
        dx = drop_rows(dx, saved.s_emb)
        if saved.emb is not None:                                                # StableEmbedding: through the two LayerNorms first
            et, ep = saved.emb
            dpos = torch.empty_like(ep)
            ops.embed_bwd(input_ids, dx, None, dpos, 0)                          # dpos[t] = sum_b dx[b, t]
            dx, dw, db = ops.layernorm_bwd(dx, et, tr.wte.norm.weight, None, True)
            put(tr.wte.norm.weight, dw); put(tr.wte.norm.bias, db)
            dep, dw, db = ops.layernorm_bwd(dpos, ep, tr.wpe.norm.weight, None, True)
            put(tr.wpe.norm.weight, dw); put(tr.wpe.norm.bias, db)
            if dwpe is not None:
                dwpe[:T] = dep
            if dw_head is not None:
                ops.embed_bwd(input_ids, dx, dw_head, None, 0)                   # tied: token rows add into the lm_head gradient
        elif dw_head is not None or dwpe is not None:
            ops.embed_bwd(input_ids, dx, dw_head, dwpe, 0)
        if dw_head is not None: put(self.lm_head.weight, dw_head)
        if dwpe is not None: put(tr.wpe.weight, dwpe)
        return grads

    def forward_context(self, input_ids):
        """(ln_f(x) [B, T, C], present [L, 2, B, nh, T, hs]) -- ha/attention.py:234-251"""
        self._check_inference(input_ids)
        x, present = self._trunk(input_ids, None, want_present=True)
        return x.view(*input_ids.shape, -1), present

    def forward(self, input_ids, past=None):
        """(logits of the last position [B, 1, V], present) -- ha/attention.py:253-279"""
        self._check_inference(input_ids)
        B, T = input_ids.shape
        x, present = self._trunk(input_ids, past, want_present=True)
        last = x.view(B, T, -1)[:, -1, :].contiguous()
        return self._linear(last, self.lm_head).view(B, 1, -1), present

    def _check_inference(self, input_ids):
        if not input_ids.is_cuda:
            raise _lib.HaloError('haloop_amd.attention.GPT runs on the HIP device only (no CPU path)')
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('GPT.forward / forward_context (generation) are inference paths: call under torch.no_grad() / '
                                      'inference_mode; training goes through forward_all')


@torch.inference_mode()
def generate(self, input_ids, max_new_tokens, temperature=1.0, top_k=None, stop_token=50256):
    """Sampling loop of ha/attention.py:282-321 (same control flow and KV-cache use; the draw itself is torch.multinomial
    on the device, as in the reference)."""
    past = None
    for _ in range(max_new_tokens):
        if input_ids.size(1) >= self.config.block_size:
            past = None
            logits, _ = self(input_ids[:, -self.config.block_size:], past=None)
        elif past is None:
            logits, past = self(input_ids, past=None)
        else:
            logits, past = self(input_ids[:, [-1]], past=past)
        logits = logits[:, -1, :] / temperature
        if top_k is not None:
            v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
            logits[logits < v[:, [-1]]] = -float('Inf')
        probs = torch.softmax(logits, dim=-1)
        input_ids_next = torch.multinomial(probs, num_samples=1)
        if input_ids_next == stop_token:
            break
        input_ids = torch.cat((input_ids, input_ids_next), dim=1)
        yield input_ids_next
