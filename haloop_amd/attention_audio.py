"""Drop-in for ha/attention_audio.py: the GPT-block audio encoders that `hac` builds for the `audio-encoder*`, `striding-e8`,
`audio-transformer*` and `e*ctc-d*` archs (ha/init.py:132-250) and BASELINE config 5 names.

``AudioEncoder(config)``: Whisper-style front-end ``gelu(conv_pre) -> gelu(conv_subsample, stride 2)`` (ha/attention_audio.py:69-71,100-103),
then with ``config.rotary_emb_dim == 0`` (the `audio-encoder` arch) frozen sinusoid positions (:10-16,87-88), dropout, ``n_layer``
bidirectional pre-LN GPT blocks (ha/attention.py:147-180 with ``config.causal = False``) and ``ln_f``; with a rotary config
(`audio-encoder-rotary*`) no ``wpe`` module or key and no positional add: the blocks are haloop_amd.attention's rotary blocks.  The two
dense convolutions are channels-last unfold + GEMM (bias and exact GELU in the epilogue at inference), and conv_subsample back-propagates
to its input through GEMM + fold (``halo_col2im_cl``).

``StridingAudioEncoder(config)`` (ha/attention_audio.py:19-61): the strided front-end of haloop_amd.conv.ConvEncoder (it IS one: same
``conv.0.*``, ``conv.{i}.depthwise.*``, ``conv.{i}.pointwise.*`` keys, its training forward and backward), dropout, rotary blocks, ``ln_f``.
It asserts a rotary config, as the reference does.

Both: forward AND backward on the HIP operators -- with grad enabled ``forward`` returns features whose ``grad_fn`` is the hand-written
backward -- same constructor, attribute and state-dict names as the reference (``transformer.{wpe,h.{i}.*,ln_f}``; rotary blocks carry
flash_attn's ``attn.Wqkv`` / ``attn.out_proj``), same return triple ``(features [B, T', C], lengths int32, {})``.  The rotary encoders do
not bound T' by ``block_size`` (the reference does not; its own test builds ``block_size = -1``).

Launch sequences: the general block forms (``block_forward``; ``block_forward_train`` / ``block_backward``) everywhere, except that the
ROTARY encoders in `bf16` mode, at shapes where ``rows_ok`` and ``rowmajor_train_ok`` hold, run the row-major forms: ``rows_block_forward``
at inference, ``block_forward_train_rm`` / ``block_backward_rm`` in training without dropout.  ``last_form`` names what the last forward ran.

Not built (raises NotImplementedError, like haloop_amd.attention.Block): a ``rotary_emb_dim`` other than the head dimension, LoRA on
rotary blocks.
"""
import math

import torch
import torch.nn as nn

from . import _lib, ops
from ._linear import DropSites, WeightImages, drop_rows, linear, linear_dw, linear_dx, training_images
from .attention import (IMAGES, ROWS, Block, LayerNorm, adapter_dropout, block_backward, block_backward_rm, block_forward, block_forward_train,
                        block_forward_train_rm, check_rotary, prefetch_block_weights, rowmajor_train_ok, rows_block_forward, rows_ok, train_sites)
from .conv import ConvEncoder
from .rnn import DropoutStream


def sinusoids(length, channels, max_timescale=10000):
    """Returns sinusoids for positional embedding (ha/attention_audio.py:10-16; a constant table built once at construction)."""
    assert channels % 2 == 0
    scales = torch.arange(channels // 2) / (channels // 2 - 1)
    inv_timescales = torch.exp(-math.log(max_timescale) * scales)
    scaled_time = torch.arange(length)[:, None] * inv_timescales[None, :]
    return torch.cat([torch.sin(scaled_time), torch.cos(scaled_time)], dim=1)


# ---- what both encoders run behind their front-ends: dropout, the blocks, ln_f (ha/attention_audio.py:55-59,109-116) --------------------
def _rowmajor(enc, M, training):
    """The rotary encoders in `bf16` mode take the row-major block forms where the products of M rows fill the chip; the non-rotary
    AudioEncoder keeps the general forms in every mode."""
    cfg, blocks = enc.config, enc.transformer.h
    return bool(cfg.rotary_emb_dim) and rows_ok(M, cfg.n_embd) and rowmajor_train_ok(cfg, blocks, M, training)


def _blocks_infer(enc, y, B, T):
    """y [B*T, C], the front-end's output (positions added) -> ln_f(blocks(y)) [B, T, C]; y is updated in place."""
    cfg, tr = enc.config, enc.transformer
    rm = _rowmajor(enc, B * T, False)
    enc.last_form = ROWS if rm else 'inference'
    for blk in tr.h:
        if rm:
            rows_block_forward(enc._images, blk, y, B, T, cfg)
        else:
            block_forward(enc._images, blk, y, B, T, cfg)
    return ops.layernorm_fwd(y, tr.ln_f.weight, tr.ln_f.bias).view(B, T, -1)


def _blocks_train(enc, y, B, T):
    """The training forward of the same: -> (features [B, T, C], what _blocks_backward needs)."""
    cfg, tr = enc.config, enc.transformer
    # dropout sites in forward order: the front dropout (ha/attention_audio.py:55,109-112), then three per block
    sites = train_sites(enc.dropout_stream, cfg.dropout, enc.training, tr.h)
    s_emb = sites.next()
    y = drop_rows(y, s_emb)
    prefetch_block_weights(enc._images, tr.h, B * T)
    fwd = block_forward_train_rm if _rowmajor(enc, B * T, enc.training) else block_forward_train
    blocks = []
    for blk in tr.h:
        y, sv = fwd(enc._images, blk, y, B, T, cfg, sites)
        blocks.append(sv)
    enc.last_form = blocks[0].form if blocks else IMAGES
    out = ops.layernorm_fwd(y, tr.ln_f.weight, tr.ln_f.bias)
    return out.view(B, T, -1), (blocks, y, s_emb)


def _blocks_backward(enc, saved, dout, B, T, put):
    """dout [B, T, C] -> the gradient w.r.t. the front-end's output [B*T, C]; parameter gradients go to put."""
    cfg, tr = enc.config, enc.transformer
    blocks, y_last, s_emb = saved
    rm = len(blocks) > 0 and blocks[0].form != IMAGES
    dy, dw, db, *dyb = ops.layernorm_bwd(dout.reshape(B * T, cfg.n_embd), y_last, tr.ln_f.weight, None, tr.ln_f.bias is not None, want_bf16=rm)
    put(tr.ln_f.weight, dw); put(tr.ln_f.bias, db)
    for blk, sv in zip(reversed(tr.h), reversed(blocks)):
        if rm:
            dy, dyb[0] = block_backward_rm(enc._images, blk, sv, dy, dyb[0], B, T, cfg, put)
        else:
            dy = block_backward(enc._images, blk, sv, dy, B, T, cfg, put)
    return drop_rows(dy, s_emb)


def _encoder_forward(enc, x, input_lengths):
    """forward() of both encoders: the autograd path with grad enabled, else inference."""
    if not x.is_cuda:
        raise _lib.HaloError(f'haloop_amd.attention_audio.{type(enc).__name__} runs on the HIP device only (no CPU path)')
    if torch.is_grad_enabled() and any(p.requires_grad for p in enc.parameters()):
        out = _EncoderFn.apply(enc, x, *[p for p in enc.parameters() if p.requires_grad])
        return out, enc.subsampled_lengths(input_lengths), {}
    if enc.training and (enc.config.dropout > 0 or adapter_dropout(enc.transformer.h) > 0):
        raise NotImplementedError('training-mode dropout is built into the autograd path only: enable grad, or call .eval()')
    return enc._forward_infer(x), enc.subsampled_lengths(input_lengths), {}


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        with training_images():
            out, saved = model._forward_train(x)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        return out

    @staticmethod
    def backward(ctx, dout):
        grads = {}

        def put(p, g):
            if p is not None and g is not None and p.requires_grad:
                grads[id(p)] = g if id(p) not in grads else grads[id(p)] + g

        ctx.model._backward_train(ctx.saved, dout.contiguous().float(), put)
        ctx.saved = None
        return (None, None) + tuple(grads.get(id(p)) for p in ctx.params)


class StridingAudioEncoder(ConvEncoder):
    def __init__(self, config):
        assert config.rotary_emb_dim
        check_rotary(config)
        super().__init__(input_dim=config.d_input, hidden_dim=config.d_conv, output_dim=config.n_embd, strides=config.conv_strides)
        self.config = config
        self.transformer = nn.ModuleDict(dict(
            drop=nn.Dropout(config.dropout),
            h=nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
            ln_f=LayerNorm(config.n_embd, bias=config.bias),
        ))
        self.dropout_stream = DropoutStream()
        self.last_form = None

    def forward(self, x, input_lengths, measure_entropy=False):
        """x [B, T, F] -> (features [B, T', C], lengths int32, {}); ``measure_entropy`` is accepted and, as in the reference
        (ha/attention_audio.py:57-61), does not change what is returned."""
        return _encoder_forward(self, x, input_lengths)

    @torch.no_grad()
    def _forward_infer(self, x):
        y = self.forward_cl(x)                                                      # gelu(conv(x)) per layer, channels-last
        B, T, C = y.shape
        return _blocks_infer(self, y.view(B * T, C), B, T)

    @torch.no_grad()
    def _forward_train(self, x):
        y, conv_saved = self._forward_cl_train(x)
        B, T, C = y.shape
        out, saved = _blocks_train(self, y.view(B * T, C), B, T)
        return out, (conv_saved, saved, (B, T))

    @torch.no_grad()
    def _backward_train(self, saved, dout, put):
        conv_saved, blocks_saved, (B, T) = saved
        dy = _blocks_backward(self, blocks_saved, dout, B, T, put)
        self._backward_cl(conv_saved, dy.view(B, T, -1), put)


class AudioEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        check_rotary(config)
        # whisper style convolutions
        self.conv_pre = nn.Conv1d(config.d_input, config.n_embd, kernel_size=3, stride=1, padding=1)
        self.conv_subsample = nn.Conv1d(config.n_embd, config.n_embd, kernel_size=3, stride=2, padding=1)
        if config.rotary_emb_dim:
            self.transformer = nn.ModuleDict(dict(
                drop=nn.Dropout(config.dropout),
                h=nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
                ln_f=LayerNorm(config.n_embd, bias=config.bias),
            ))
        else:
            self.transformer = nn.ModuleDict(dict(
                wpe=nn.Embedding(config.block_size, config.n_embd),
                drop=nn.Dropout(config.dropout),
                h=nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
                ln_f=LayerNorm(config.n_embd, bias=config.bias),
            ))
            self.transformer.wpe.weight.data = sinusoids(config.block_size, config.n_embd)
            self.transformer.wpe.requires_grad_(False)
        self._images = WeightImages()
        self.dropout_stream = DropoutStream()
        self.last_form = None

    def subsampled_lengths(self, input_lengths):
        # https://github.com/vdumoulin/conv_arithmetic (ha/attention_audio.py:92-97): float floor, int32 result
        p, k, s = self.conv_subsample.padding[0], self.conv_subsample.kernel_size[0], self.conv_subsample.stride[0]
        o = input_lengths + 2 * p - k
        o = torch.floor(o / s + 1)
        return o.int()

    def forward(self, x, input_lengths, measure_entropy=False):
        """x [B, T, F] -> (features [B, T', C], lengths int32, {}); ``measure_entropy`` is accepted and, as in the reference
        (ha/attention_audio.py:113-117), does not change what is returned."""
        return _encoder_forward(self, x, input_lengths)

    def _conv(self, conv, x3d, gelu):
        col, To = ops.im2col_cl(x3d, conv.kernel_size[0], conv.stride[0], conv.padding[0])
        y = linear(self._images, col, conv.weight, bias=conv.bias.detach(), gelu='erf' if gelu else False)
        return y, col, To

    def _add_positions(self, y, T):
        """x + wpe(pos) (ha/attention_audio.py:111-112); a rotary config has no positions to add and no bound on T."""
        cfg = self.config
        if cfg.rotary_emb_dim:
            return
        assert T <= cfg.block_size, f'Cannot forward sequence of length {T}, block size is only {cfg.block_size}'
        ops.add_rows_bcast_(y, self.transformer.wpe.weight.detach()[:T].contiguous(), T)

    @torch.no_grad()
    def _forward_infer(self, x):
        x = x.float().contiguous()
        B = x.shape[0]
        y, _, T1 = self._conv(self.conv_pre, x, True)                               # F.gelu(conv_pre(x)), channels-last
        y, _, T = self._conv(self.conv_subsample, y.view(B, T1, -1), True)
        self._add_positions(y, T)
        return _blocks_infer(self, y, B, T)

    # ---- training: forward keeping what the backward needs, and the backward -----------------------------------------
    @torch.no_grad()
    def _forward_train(self, x):
        x = x.float().contiguous()
        B, T0, _ = x.shape
        a1, col1, T1 = self._conv(self.conv_pre, x, False)                          # pre-activations kept for the GELU backward
        y1 = ops.gelu_fwd(a1, exact=True)
        a2, col2, T = self._conv(self.conv_subsample, y1.view(B, T1, -1), False)
        y = ops.gelu_fwd(a2, exact=True)
        self._add_positions(y, T)
        out, saved = _blocks_train(self, y, B, T)
        return out, (col1, a1, col2, a2, saved, (B, T0, T1, T))

    @torch.no_grad()
    def _backward_train(self, saved, dout, put):
        cfg = self.config
        col1, a1, col2, a2, blocks_saved, (B, T0, T1, T) = saved
        C = cfg.n_embd
        dy = _blocks_backward(self, blocks_saved, dout, B, T, put)                  # wpe is frozen: nothing to collect for it
        # conv_subsample: y = gelu(col2 W2^T + b2)
        da2 = ops.gelu_bwd(dy, a2, exact=True)
        c2 = self.conv_subsample
        put(c2.weight, linear_dw(da2, col2).view_as(c2.weight))
        put(c2.bias, ops.colsum(da2))
        dcol2 = linear_dx(self._images, da2, c2.weight)                             # [B*T, C*3]
        dy1 = ops.col2im_cl(dcol2, B, T1, C, c2.kernel_size[0], c2.stride[0], c2.padding[0])
        # conv_pre: y1 = gelu(col1 W1^T + b1); its input is data (mel frames)
        da1 = ops.gelu_bwd(dy1.view(B * T1, C), a1, exact=True)
        c1 = self.conv_pre
        put(c1.weight, linear_dw(da1, col1).view_as(c1.weight))
        put(c1.bias, ops.colsum(da1))
