"""Drop-in for ha/lora.py as the GPT trainer uses it (ha/attention_loop.py:137-139, ha/init.py:76-79): low-rank adapters on every
``c_attn`` Linear, the base frozen.

Same call surface and state-dict names (``...attn.c_attn.lora_A.weight`` [r, in], ``...lora_B.weight`` [out, r], plus their biases when
the base Linear has one), so a checkpoint written by ``hala --lora`` loads after ``attach_to_c_attn(model)``:

    y = x W^T + b + scaling * lora_B(lora_A(dropout(x))),    scaling = lora_alpha / r

``Linear.train(False)`` with ``merge_weights`` folds ``scaling * B A`` into the base weight (the adapter Linears' own biases are NOT
folded: the reference's quirk, kept), ``train(True)`` takes it out again.  The GPT blocks do not call the module: they read ``.weight``
and, while the adapter is unmerged, add the low-rank term at every c_attn site (haloop_amd/attention.py: ``lora_forward`` /
``lora_backward`` here on the general path, ``lora_rows_forward`` / ``lora_rows_backward`` -- the ``halo_lora_*`` kernels of csrc/lora.hip
-- on the row-major bf16 path for r <= 16; a larger rank runs on the general path).  Dropout of the adapter's input is a Philox site of the model's dropout stream (id 4096 + layer) in
training forwards (``forward_all`` with grad enabled).  Without grad, in train() mode: ``GPT.forward_all`` and the audio encoder raise when
an unmerged adapter has lora_dropout > 0, exactly as they do for config.dropout > 0 (scoring wants eval()); ``GPT.forward`` /
``forward_context`` / ``generate`` and ``Linear.forward`` apply the adapter unmerged and draw no dropout of any kind, as they never did
for config.dropout.

Not built: ``MergedLinear`` (the reference never instantiates it), adapters on other Linears, adapters on rotary blocks (``attn.Wqkv``).
"""
import math

import torch
import torch.nn as nn

from . import _lib, ops

FAST_MAX_RANK = ops.LORA_RANK_PAD


class Linear(nn.Linear):
    def __init__(self, in_features, out_features, r=0, lora_alpha=1, lora_dropout=0.0, merge_weights=True, **kwargs):
        super().__init__(in_features, out_features, **kwargs)
        self.r, self.lora_alpha, self.merge_weights, self.merged = r, lora_alpha, merge_weights, False
        self.lora_dropout_p = float(lora_dropout)
        self.lora_dropout = nn.Dropout(p=lora_dropout) if lora_dropout > 0.0 else (lambda x: x)
        if r > 0:
            has_bias = bool(kwargs.get('bias', False))          # as the reference: only an explicit bias= gives the adapters one
            self.lora_A = nn.Linear(in_features, r, bias=has_bias)
            self.lora_B = nn.Linear(r, out_features, bias=has_bias)
            self.scaling = lora_alpha / r
            self.weight.requires_grad = False
            nn.init.kaiming_uniform_(self.lora_A.weight, a=math.sqrt(5))
            nn.init.zeros_(self.lora_B.weight)

    @property
    def active(self):
        """The adapter term is added separately (it exists and is not folded into the weight)."""
        return self.r > 0 and not self.merged

    def delta(self):
        return (self.lora_B.weight @ self.lora_A.weight) * self.scaling

    def train(self, mode=True):
        super().train(mode)
        if self.merge_weights and self.r > 0 and self.merged == bool(mode):
            # in place THROUGH the parameter, so that its version counter moves and the cached operand images are rebuilt
            with torch.no_grad():
                if mode:
                    self.weight.sub_(self.delta())
                else:
                    self.weight.add_(self.delta())
        if self.merge_weights:
            self.merged = not mode
        return self

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.HaloError('haloop_amd.lora.Linear runs on the HIP device only (no CPU path)')
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('lora.Linear on its own is an inference path: call under torch.no_grad(); training goes through '
                                      'GPT.forward_all / AudioEncoder')
        shp = x.shape
        x2d = x.reshape(-1, shp[-1]).contiguous().float()
        M, K = x2d.shape
        with torch.no_grad():
            y = ops.gemm(x2d, self.weight.detach(), True, True, M, self.out_features, K, bias1=self.bias)
            if self.active:
                lora_forward(self, x2d, y)
        return y.view(*shp[:-1], self.out_features)


def is_active(lin):
    return isinstance(lin, Linear) and lin.active


def fast_ok(lin, M):
    """The halo_lora_* kernels take this adapter at M rows (the callers also need the row-major bf16 path: bf16 mode, no biases)."""
    return lin.r <= FAST_MAX_RANK and lin.bias is None and lin.lora_A.bias is None and ops.lora_supported(M, lin.in_features, lin.out_features, lin.r)


def packed(images, lin):
    """(A16, At16, B16, Bt16): the rank-padded bf16 operands, rebuilt when A or B change."""
    ws = (lin.lora_A.weight, lin.lora_B.weight)
    return images._lookup('lora', ws, lambda: ops.lora_pack(ws[0].detach(), ws[1].detach()))


# ---- the general path: composed from the dense fp32 operators, any mode, any shape, adapter biases included ---------------------------
def lora_forward(lin, h, qkv, site=(ops.NO_DROPOUT, 0)):
    """qkv [M, out] (fp32, contiguous) += scaling * lora_B(lora_A(mask * h)); -> u = lora_A(mask * h) [M, r] for the backward."""
    M, K = h.shape
    drop, sid = site
    hd = ops.dropout_fwd(h, drop, sid) if drop.p > 0 else h
    A, Bm = lin.lora_A, lin.lora_B
    u = ops.gemm(hd, A.weight.detach(), True, True, M, lin.r, K, bias1=A.bias)
    t = ops.gemm(u, Bm.weight.detach(), True, True, M, lin.out_features, lin.r, bias1=Bm.bias)
    ops.scale_add_(qkv, t, 1.0, lin.scaling)
    return u


def lora_backward(lin, h, u, dqkv, d_h, put, site=(ops.NO_DROPOUT, 0)):
    """Adapter gradients to put(); d_h [M, in] (fp32, or None when nobody reads it) += mask * (du A) with du = scaling * dqkv B."""
    M, K = h.shape
    N, r, s = lin.out_features, lin.r, lin.scaling
    drop, sid = site
    A, Bm = lin.lora_A, lin.lora_B
    du = ops.gemm(dqkv, Bm.weight.detach(), True, False, M, r, N)                     # dqkv [M, N] B [N, r]
    ops.scale_add_(du, du, 0.0, s)
    if Bm.weight.requires_grad:
        us = ops.scale_add_(torch.empty_like(u), u, 0.0, s)
        put(Bm.weight, ops.gemm(dqkv, us, False, False, N, r, M))                     # s dqkv^T u
    if Bm.bias is not None and Bm.bias.requires_grad:
        db = ops.colsum(dqkv)
        put(Bm.bias, ops.scale_add_(db, db, 0.0, s))
    if A.weight.requires_grad:
        hd = ops.dropout_fwd(h, drop, sid) if drop.p > 0 else h
        put(A.weight, ops.gemm(du, hd, False, False, r, K, M))                        # du^T (mask * h)
    if A.bias is not None and A.bias.requires_grad:
        put(A.bias, ops.colsum(du))
    if d_h is not None:
        t = ops.gemm(du, A.weight.detach(), True, False, M, K, r)                     # du [M, r] A [r, in]
        if drop.p > 0:
            t = ops.dropout_fwd(t, drop, sid)
        ops.scale_add_(d_h, t, 1.0, 1.0)


# ---- the row-major bf16 path (rank <= 16, fast_ok): the halo_lora_* kernels of csrc/lora.hip on bf16 rows -----------------------------
def lora_rows_forward(images, lin, h, qkv, site=(ops.NO_DROPOUT, 0)):
    """qkv [M, out] (bf16 or fp32 rows) += scaling * ((mask * h) A^T) B^T for the bf16 rows h [M, in]; -> u [M, 16] bf16 for the backward."""
    A16, _, B16, _ = packed(images, lin)
    u = ops.lora_down(h, A16, 1.0, site[0], site[1])
    ops.lora_up_(qkv, u, B16, lin.scaling)
    return u


def lora_rows_backward(images, lin, h, u, dqkv, d_h, put, site=(ops.NO_DROPOUT, 0)):
    """Adapter gradients to put(): du = s dqkv B, dB = s dqkv^T u, dA = du^T (mask * h); d_h [M, in] (or None when nobody reads it)
    += mask * (du A).  h, u, dqkv: bf16 rows."""
    _, At16, _, Bt16 = packed(images, lin)
    du = ops.lora_down(dqkv, Bt16, lin.scaling)
    if lin.lora_B.weight.requires_grad:
        put(lin.lora_B.weight, ops.lora_tn(u, dqkv, lin.r, lin.scaling, transpose_out=True))
    if lin.lora_A.weight.requires_grad:
        put(lin.lora_A.weight, ops.lora_tn(du, h, lin.r, 1.0, drop=site[0], stream_id=site[1]))
    if d_h is not None:
        ops.lora_up_(d_h, du, At16, 1.0, site[0], site[1])


# ---- the reference's module surgery -----------------------------------------------------------------------------------------------
def attach_to_c_attn(model, r=4, lora_alpha=32, lora_dropout=0.1):
    """Replace every module whose name ends in ``c_attn`` by a lora.Linear that SHARES its weight / bias tensors."""
    for key in [k for k, _ in model.named_modules()]:
        if key.endswith('attn.Wqkv'):
            raise NotImplementedError('LoRA adapters on rotary blocks (attn.Wqkv) are not built')
        if not key.endswith('c_attn'):
            continue
        parent_name, _, child = key.rpartition('.')
        parent, old = model.get_submodule(parent_name), model.get_submodule(key)
        new = Linear(old.in_features, old.out_features, bias=old.bias is not None, r=r, lora_alpha=lora_alpha, lora_dropout=lora_dropout)
        new.weight = old.weight
        if old.bias is not None:
            new.bias = old.bias
        new.to(old.weight.device)
        setattr(parent, child, new)


def mark_only_lora_as_trainable_(model):
    for n, p in model.named_parameters():
        if 'lora_' not in n:
            p.requires_grad = False
