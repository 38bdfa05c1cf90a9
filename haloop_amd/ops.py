"""Tensor-level wrappers over the C ABI (no autograd here).  Every function enqueues on torch's
current HIP stream and allocates its outputs/workspaces with torch (device memory plumbing only).
"""
import ctypes as C
import math
from collections import namedtuple

import torch

from . import _lib
from ._lib import check, lib, ptr, ptr_array


def _stream():
    # the raw hipStream_t of torch's current stream: torch.cuda.current_stream() builds a Stream object per call (~4 us of
    # host time, half of what a small launch costs end to end); this is the accessor torch's own kernels launchers use
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f'{name}: expected a contiguous float32 HIP tensor, got {t.dtype} {t.device} '
                         f'contiguous={t.is_contiguous()}')
    return t


class Dropout:
    """Value bundle (p, seed, offset, device step counter) for one forward/backward pair."""
    __slots__ = ('p', 'seed', 'offset', 'counter')

    def __init__(self, p=0.0, seed=0, offset=0, counter=None):
        self.p, self.seed, self.offset, self.counter = float(p), int(seed), int(offset), counter

    @property
    def counter_ptr(self):
        return ptr(self.counter)


NO_DROPOUT = Dropout()


def subsampled_length(T, ks=5, stride=4, pad=3):
    return (T + 2 * pad - ks) // stride + 1


def _gemm_flags(relu, gelu, accumulate):
    """gelu: False, True / 'tanh' (new_gelu) or 'erf' (nn.GELU())."""
    g = 0 if not gelu else (_lib.HALO_GEMM_GELU_ERF if gelu == 'erf' else _lib.HALO_GEMM_GELU)
    return (_lib.HALO_GEMM_RELU if relu else 0) | g | (_lib.HALO_GEMM_ACCUM if accumulate else 0)


def gemm(a, b, a_kcontig, b_kcontig, M, N, K, out=None, bias1=None, bias2=None, relu=False,
         drop=NO_DROPOUT, stream_id=0, gelu=False, accumulate=False):
    lda = a.stride(0) if a.dim() == 2 else a.shape[-1]          # row-strided views (column slices of packed buffers) are fine
    ldb = b.stride(0) if b.dim() == 2 else b.shape[-1]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    check(lib().halo_gemm_f32(int(a_kcontig), int(b_kcontig), M, N, K, ptr(a), lda, ptr(b), ldb, ptr(out), N,
                              ptr(bias1), ptr(bias2), _gemm_flags(relu, gelu, accumulate), drop.p, drop.seed,
                              stream_id, drop.offset, drop.counter_ptr, _stream()), 'halo_gemm_f32')
    return out


def split_image(x2d, transposed=False):
    """bf16 hi/lo tiled image of logical X[rows][k]; x2d is [rows,k], or [k,rows] when ``transposed``."""
    if x2d.dtype != torch.float32 or not x2d.is_cuda or x2d.dim() != 2 or x2d.stride(1) != 1:
        raise ValueError('split_image: expected a 2-D float32 HIP tensor with a unit column stride')
    rows, k = (x2d.shape[1], x2d.shape[0]) if transposed else x2d.shape
    img = torch.empty(lib().halo_split_image_bytes(rows, k), device=x2d.device, dtype=torch.uint8)
    check(lib().halo_split_image(ptr(x2d), rows, k, x2d.stride(0), int(transposed), ptr(img), _stream()), 'halo_split_image')
    return img


PAIR_COPY, PAIR_GELU, PAIR_GELU_ERF, PAIR_GELU_BWD, PAIR_GELU_ERF_BWD = range(5)


def image_pair(x2d, op=PAIR_COPY, x2=None, rows_image=True, cols_image=True):
    """One read of x2d [rows, cols] (through ``op``) -> (split image of value [rows][cols], split image of value^T [cols][rows]):
    the two operand images a Linear's backward wants of the same matrix (dx = dy W and dW = dy^T x); either can be skipped (None).
    ops: PAIR_COPY value = x2d; PAIR_GELU(_ERF) value = gelu(x2d); PAIR_GELU(_ERF)_BWD value = x2d * gelu'(x2) (x2d = dy)."""
    for t in (x2d, x2):
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1):
            raise ValueError('image_pair: expected 2-D float32 HIP tensors with a unit column stride')
    if op in (PAIR_GELU_BWD, PAIR_GELU_ERF_BWD) and (x2 is None or x2.shape != x2d.shape):
        raise ValueError('image_pair: the GELU backward needs the pre-activation, shaped like dy')
    rows, cols = x2d.shape
    rm = torch.empty(lib().halo_split_image_bytes(rows, cols), device=x2d.device, dtype=torch.uint8) if rows_image else None
    tr = torch.empty(lib().halo_split_image_bytes(cols, rows), device=x2d.device, dtype=torch.uint8) if cols_image else None
    check(lib().halo_image_pair(ptr(x2d), ptr(x2), rows, cols, x2d.stride(0), x2.stride(0) if x2 is not None else 0, op, ptr(rm), ptr(tr),
                                _stream()), 'halo_image_pair')
    return rm, tr


def image_pairs(mats):
    """image_pair(PAIR_COPY) of several 2-D fp32 matrices in ceil(n / 6) launches -> [(image, image of the transpose), ...]."""
    import ctypes as C
    mats = list(mats)
    if not mats:
        return []
    for t in mats:
        if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError('image_pairs: expected 2-D float32 HIP tensors with a unit column stride')
    n = len(mats)
    dev = mats[0].device
    rm = [torch.empty(lib().halo_split_image_bytes(t.shape[0], t.shape[1]), device=dev, dtype=torch.uint8) for t in mats]
    tr = [torch.empty(lib().halo_split_image_bytes(t.shape[1], t.shape[0]), device=dev, dtype=torch.uint8) for t in mats]
    vp = lambda xs: (C.c_void_p * n)(*[ptr(x) for x in xs])
    check(lib().halo_image_pairs(n, vp(mats), (C.c_int * n)(*[t.shape[0] for t in mats]), (C.c_int * n)(*[t.shape[1] for t in mats]),
                                 (C.c_long * n)(*[t.stride(0) for t in mats]), vp(rm), vp(tr), _stream()), 'halo_image_pairs')
    return list(zip(rm, tr))


def layernorm_image(x2d, weight, bias=None, eps=1e-5, want_y=False):
    """LayerNorm of the rows written directly as the split operand image of the Linear that follows (C % 32 == 0).
    -> (image, y fp32 or None)"""
    _f32c(x2d, 'x')
    rows, Cn = x2d.shape
    img = torch.empty(lib().halo_split_image_bytes(rows, Cn), device=x2d.device, dtype=torch.uint8)
    y = torch.empty_like(x2d) if want_y else None
    check(lib().halo_layernorm_image(ptr(x2d), ptr(weight), ptr(bias), ptr(y), ptr(img), rows, Cn, eps, _stream()), 'halo_layernorm_image')
    return img, y


def layernorm_bf16(x2d, weight, bias=None, eps=1e-5, want_image=False):
    """LayerNorm of the rows as row-major bf16 [rows, C]: the operand form gemm_split_io (a = (hi, None)) and gemm_tn read.
    ``want_image``: -> (rows, tiled operand image of the same values) from the one launch."""
    _f32c(x2d, 'x')
    rows, Cn = x2d.shape
    y = torch.empty(rows, Cn, device=x2d.device, dtype=torch.bfloat16)
    img = torch.empty(lib().halo_split_image_bytes(rows, Cn), device=x2d.device, dtype=torch.uint8) if want_image else None
    check(lib().halo_layernorm_bf16(ptr(x2d), ptr(weight), ptr(bias), None, ptr(y), ptr(img), rows, Cn, eps, _stream()), 'halo_layernorm_bf16')
    return (y, img) if want_image else y


def gelu_bf16(a, exact=False):
    """gelu(a) as bf16 (same shape)."""
    _f32c(a, 'a')
    y = torch.empty(a.shape, device=a.device, dtype=torch.bfloat16)
    check(lib().halo_gelu_bf16(ptr(a), ptr(y), a.numel(), int(exact), _stream()), 'halo_gelu_bf16')
    return y


def gelu_bwd_bf16(dy, a, exact=False):
    """dy * gelu'(a) as bf16."""
    _f32c(dy, 'dy'); _f32c(a, 'a')
    y = torch.empty(a.shape, device=a.device, dtype=torch.bfloat16)
    check(lib().halo_gelu_bwd_bf16(ptr(dy), ptr(a), ptr(y), a.numel(), int(exact), _stream()), 'halo_gelu_bwd_bf16')
    return y


def cast_bf16(x):
    _f32c(x, 'x')
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(lib().halo_cast_bf16(ptr(x), ptr(y), x.numel(), _stream()), 'halo_cast_bf16')
    return y


def gemm_split(a_img, b_img, M, N, K, out=None, bias1=None, bias2=None, relu=False, drop=NO_DROPOUT, stream_id=0,
               gelu=False, accumulate=False, residual=None):
    """C[M,N] = A[M,K] B[N,K]^T from split images (three bf16 MFMAs per product, fp32 accumulate).  ``residual`` [M, N]: the
    result is added to it and written to ``out`` (a fresh tensor by default); ``accumulate`` adds into ``out`` in place."""
    if out is None:
        out = torch.empty(M, N, device=a_img.device, dtype=torch.float32)
    if residual is not None:
        if accumulate:
            raise ValueError('gemm_split: residual= and accumulate= are alternatives')
        _f32c(residual, 'residual')
        if residual.shape != (M, N):
            raise ValueError('gemm_split: residual must be [M, N]')
        check(lib().halo_gemm_split_residual(ptr(a_img), ptr(b_img), M, N, K, ptr(out), N, ptr(residual), N, ptr(bias1), ptr(bias2),
                                             _gemm_flags(relu, gelu, False), drop.p, drop.seed, stream_id, drop.offset,
                                             drop.counter_ptr, _stream()), 'halo_gemm_split_residual')
        return out
    check(lib().halo_gemm_split(ptr(a_img), ptr(b_img), M, N, K, ptr(out), N, ptr(bias1), ptr(bias2),
                                _gemm_flags(relu, gelu, accumulate), drop.p, drop.seed, stream_id, drop.offset,
                                drop.counter_ptr, _stream()), 'halo_gemm_split')
    return out


def gemm_split_io(a, b_img, M, N, K, out=None, out_rowmajor=False, bias1=None, bias2=None, relu=False, gelu=False, accumulate=False,
                  residual=None):
    """gemm_split with row-major bf16 activations on either side (halo_gemm_split_io).  ``a``: an operand image (uint8 tensor) or a
    (hi, lo) pair of row-major bf16 [M, K] tensors (lo None in bf16 mode).  ``out_rowmajor``: return the result as a (hi, lo) pair of
    bf16 [M, N] tensors (lo None in bf16 mode) and write no fp32 unless ``out`` is given.  -> out, or (hi, lo)."""
    x3 = lib().halo_get_math_mode() != _lib.HALO_MATH_BF16
    a_img = a_hi = a_lo = None
    lda = 0
    if isinstance(a, (tuple, list)):
        a_hi, a_lo = a
        if a_hi.dtype != torch.bfloat16 or a_hi.shape != (M, K) or a_hi.stride(1) != 1 or (x3 and (a_lo is None or a_lo.shape != (M, K) or a_lo.stride() != a_hi.stride())):
            raise ValueError('gemm_split_io: a = (hi, lo) row-major bf16 [M, K] tensors with equal strides')
        lda = a_hi.stride(0)
    else:
        a_img = a
    dev = b_img.device
    o_hi = o_lo = None
    if out_rowmajor:
        o_hi = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        o_lo = torch.empty(M, N, device=dev, dtype=torch.bfloat16) if x3 else None
    elif out is None:
        out = torch.empty(M, N, device=dev, dtype=torch.float32)
    if residual is not None:
        _f32c(residual, 'residual')
    flags = _gemm_flags(relu, gelu, accumulate or residual is not None)
    check(lib().halo_gemm_split_io(ptr(a_img), ptr(a_hi), ptr(a_lo), lda, ptr(b_img), M, N, K, ptr(out), N if out is not None else 0,
                                   ptr(o_hi), ptr(o_lo), N, ptr(residual), N if residual is not None else 0, ptr(bias1), ptr(bias2),
                                   flags, _stream()), 'halo_gemm_split_io')
    return (o_hi, o_lo) if out_rowmajor else out


def gemm_tn(a, b, out=None, accumulate=False):
    """a [K, M]^T b [K, N] -> fp32 [M, N] for row-major bf16 a, b (the contraction index is their row): halo_gemm_tn_bf16, the weight
    gradient of a Linear from row-major bf16 activations / output gradients without a transposed operand image."""
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise ValueError('gemm_tn: a [K, M], b [K, N] bf16')
    if a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError('gemm_tn: row-major operands')
    K, M = a.shape
    N = b.shape[1]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
        accumulate = False
    check(lib().halo_gemm_tn_bf16(ptr(a), a.stride(0), ptr(b), b.stride(0), M, N, K, ptr(out), out.stride(0),
                                  _lib.HALO_GEMM_ACCUM if accumulate else 0, _stream()), 'halo_gemm_tn_bf16')
    return out


def gemm_tn_group(pairs):
    """[a_i [K, M_i]^T b_i [K, N_i] for (a_i, b_i) in pairs] -> list of fp32 [M_i, N_i], row-major bf16 operands with ONE contraction length
    K: up to four products per launch on whole-K tiles -- a GPT block's four weight gradients, the lm_head's.  In single-pass bf16
    arithmetic a group of at least two rounds of 256 x 256 tiles (the lm_head) runs on halo_gemm_tn_rows_group's 256-row tiles
    (csrc/gemm_tn_rows.hip), everything else on the 128 x 128 tiles of halo_gemm_tn_bf16_group; HALO_GEMM_TN_ROWS=1 / 0 force one."""
    import ctypes as C
    import os
    outs = []
    for i0 in range(0, len(pairs), 4):
        grp = pairs[i0:i0 + 4]
        n = len(grp)
        K = grp[0][0].shape[0]
        for a, b in grp:
            if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.dim() != 2 or b.dim() != 2 or a.shape[0] != K or b.shape[0] != K \
                    or a.stride(1) != 1 or b.stride(1) != 1:
                raise ValueError('gemm_tn_group: row-major bf16 a [K, M], b [K, N] with one K')
        cs = [torch.empty(a.shape[1], b.shape[1], device=a.device, dtype=torch.float32) for a, b in grp]
        vp = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        Ms, Ns = (C.c_int * n)(*[a.shape[1] for a, _ in grp]), (C.c_int * n)(*[b.shape[1] for _, b in grp])
        force = os.environ.get('HALO_GEMM_TN_ROWS', '')
        if force != '0' and (lib().halo_gemm_tn_rows_supported if force == '1' else lib().halo_gemm_tn_rows_preferred)(n, Ms, Ns, K) \
                and all(a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 for a, b in grp):
            check(lib().halo_gemm_tn_rows_group(n, vp([a for a, _ in grp]), (C.c_long * n)(*[a.stride(0) for a, _ in grp]),
                                                vp([b for _, b in grp]), (C.c_long * n)(*[b.stride(0) for _, b in grp]), Ms, Ns, K,
                                                vp(cs), (C.c_long * n)(*[c.stride(0) for c in cs]), _stream()), 'halo_gemm_tn_rows_group')
            outs += cs
            continue
        check(lib().halo_gemm_tn_bf16_group(n, vp([a for a, _ in grp]), (C.c_long * n)(*[a.stride(0) for a, _ in grp]),
                                            vp([b for _, b in grp]), (C.c_long * n)(*[b.stride(0) for _, b in grp]),
                                            (C.c_int * n)(*[a.shape[1] for a, _ in grp]), (C.c_int * n)(*[b.shape[1] for _, b in grp]), K,
                                            vp(cs), (C.c_int * n)(*[c.stride(0) for c in cs]), 0, _stream()), 'halo_gemm_tn_bf16_group')
        outs += cs
    return outs


def gemm_split_ce(a_img, b_img, M, N, K, targets, ignore_index=0, bias=None, want_logits=False, want_lse=False):
    """Per-row cross-entropy of logits = A B^T (+ bias) straight from the split GEMM's epilogue: -> (loss [M], lse [M] or None,
    logits [M, N] or None).  Without want_logits nothing of size M x N is written."""
    tg = _i64c(targets.reshape(-1), 'targets')
    dev = a_img.device
    ws = torch.empty(lib().halo_gemm_split_ce_workspace_bytes(M, N), device=dev, dtype=torch.uint8)
    loss = torch.empty(M, device=dev, dtype=torch.float32)
    lse = torch.empty(M, device=dev, dtype=torch.float32) if want_lse else None
    logits = torch.empty(M, N, device=dev, dtype=torch.float32) if want_logits else None
    check(lib().halo_gemm_split_ce(ptr(a_img), ptr(b_img), M, N, K, ptr(logits), N, ptr(bias), ptr(tg), ignore_index, ptr(ws), ptr(loss),
                                   ptr(lse), _stream()), 'halo_gemm_split_ce')
    return loss, lse, logits


def gemm_rows_supported(M, N, K):
    """halo_gemm_rows takes this shape in the current arithmetic mode (single-pass bf16 only)."""
    return bool(lib().halo_gemm_rows_supported(M, N, K))


def gemm_rows(a, b_img, M, N, K, out=None, residual=None, out_bf16=False):
    """C [M, N] = A [M, K] B [N, K]^T on the 256-row tiles of halo_gemm_rows (single-pass bf16).  ``a``: row-major bf16 [M, K] or an operand
    image (uint8).  Result: fp32 ``out`` (fresh by default), ``residual`` [M, N] fp32 added when given; or, with ``out_bf16``, row-major
    bf16 [M, N]."""
    a_img = a_rm = None
    lda = 0
    if a.dtype == torch.bfloat16:
        if a.dim() != 2 or a.shape != (M, K) or a.stride(1) != 1:
            raise ValueError('gemm_rows: a = row-major bf16 [M, K]')
        a_rm, lda = a, a.stride(0)
    else:
        a_img = a
    dev = b_img.device
    ob = None
    if out_bf16:
        if residual is not None or out is not None:
            raise ValueError('gemm_rows: a bf16 result takes neither out= nor residual=')
        ob = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    elif out is None:
        out = torch.empty(M, N, device=dev, dtype=torch.float32)
    if residual is not None:
        _f32c(residual, 'residual')
        if residual.shape != (M, N):
            raise ValueError('gemm_rows: residual must be [M, N]')
    check(lib().halo_gemm_rows(ptr(a_img), ptr(a_rm), lda, ptr(b_img), M, N, K, ptr(out), N if out is not None else 0, ptr(residual),
                               N if residual is not None else 0, ptr(ob), N if ob is not None else 0, _stream()), 'halo_gemm_rows')
    return ob if out_bf16 else out


def gemm_rows_gelu(a, b_img, M, N, K, exact=False, keep_pre=False):
    """gelu(A B^T) as row-major bf16 [M, N] from halo_gemm_rows' epilogue; ``keep_pre``: -> (gelu, pre-activation), both bf16 -- the same
    bits as gemm_rows(out_bf16=True) followed by gelu_b16."""
    a_img = a_rm = None
    lda = 0
    if a.dtype == torch.bfloat16:
        a_rm, lda = a, a.stride(0)
    else:
        a_img = a
    g = torch.empty(M, N, device=b_img.device, dtype=torch.bfloat16)
    pre = torch.empty(M, N, device=b_img.device, dtype=torch.bfloat16) if keep_pre else None
    check(lib().halo_gemm_rows_gelu(ptr(a_img), ptr(a_rm), lda, ptr(b_img), M, N, K, ptr(g), ptr(pre), N, int(exact), _stream()), 'halo_gemm_rows_gelu')
    return (g, pre) if keep_pre else g


def gemm_rows_ce(a, b_img, M, N, K, targets, ignore_index=0, want_logits=False, want_lse=False):
    """Per-row cross-entropy of logits = A B^T from halo_gemm_rows_ce's epilogue: -> (loss [M], lse [M] or None, logits [M, N] as
    row-major bf16 or None).  ``a``: row-major bf16 [M, K] or an operand image."""
    tg = _i64c(targets.reshape(-1), 'targets')
    a_img = a_rm = None
    lda = 0
    if a.dtype == torch.bfloat16:
        a_rm, lda = a, a.stride(0)
    else:
        a_img = a
    dev = b_img.device
    ws = torch.empty(lib().halo_gemm_rows_ce_workspace_bytes(M, N), device=dev, dtype=torch.uint8)
    loss = torch.empty(M, device=dev, dtype=torch.float32)
    lse = torch.empty(M, device=dev, dtype=torch.float32) if want_lse else None
    logits = torch.empty(M, N, device=dev, dtype=torch.bfloat16) if want_logits else None
    check(lib().halo_gemm_rows_ce(ptr(a_img), ptr(a_rm), lda, ptr(b_img), M, N, K, ptr(tg), ignore_index, ptr(ws), ptr(loss), ptr(lse),
                                  ptr(logits), N if logits is not None else 0, _stream()), 'halo_gemm_rows_ce')
    return loss, lse, logits


def cross_entropy_bwd_bf16_(logits_bf16, targets, lse, grad_rows, ignore_index=0):
    """In place: bf16 logits [rows, V] -> (softmax - onehot) * grad_rows[row] as row-major bf16 (0 on ignored rows)."""
    if logits_bf16.dtype != torch.bfloat16 or logits_bf16.dim() != 2 or logits_bf16.stride(1) != 1:
        raise ValueError('cross_entropy_bwd_bf16_: row-major bf16 logits')
    tg = _i64c(targets.reshape(-1), 'targets')
    rows, V = logits_bf16.shape
    g = grad_rows.reshape(-1)
    _f32c(g, 'grad_rows'); _f32c(lse, 'lse')
    stride = 0 if g.numel() == 1 else 1
    check(lib().halo_cross_entropy_bwd_bf16(ptr(logits_bf16), ptr(tg), ptr(lse), ptr(g), stride, rows, V, logits_bf16.stride(0), ignore_index,
                                            _stream()), 'halo_cross_entropy_bwd_bf16')
    return logits_bf16


def gelu_b16(a, exact=False):
    """gelu(a), bf16 -> bf16."""
    y = torch.empty_like(a)
    check(lib().halo_gelu_b16(ptr(a), ptr(y), a.numel(), int(exact), _stream()), 'halo_gelu_b16')
    return y


def gelu_bwd_b16(dy, a, exact=False):
    """dy * gelu'(a), bf16 x bf16 -> bf16."""
    y = torch.empty_like(a)
    check(lib().halo_gelu_bwd_b16(ptr(dy), ptr(a), ptr(y), a.numel(), int(exact), _stream()), 'halo_gelu_bwd_b16')
    return y


# ---- LoRA adapters on row-major bf16 rows (csrc/lora.hip) -------------------------------------------------------------------------
LORA_RANK_PAD = 16


def lora_supported(M, n_in, n_out, r):
    """The halo_lora_* kernels take an adapter of rank r on a Linear [n_in -> n_out] at M rows."""
    return bool(lib().halo_lora_supported(M, n_in, n_out, r))


def lora_pack(A, B):
    """A [r, n_in], B [n_out, r] fp32 -> (A16 [16, n_in], At16 [n_in, 16], B16 [n_out, 16], Bt16 [16, n_out]): the rank-padded bf16
    operands of the three kernels, views of one buffer written by one launch."""
    _f32c(A, 'A'); _f32c(B, 'B')
    r, n_in = A.shape
    n_out = B.shape[0]
    if B.shape[1] != r:
        raise ValueError('lora_pack: A [r, n_in] and B [n_out, r]')
    R = LORA_RANK_PAD
    buf = torch.empty(lib().halo_lora_pack_bytes(n_in, n_out) // 2, device=A.device, dtype=torch.bfloat16)
    check(lib().halo_lora_pack(ptr(A), ptr(B), r, n_in, n_out, ptr(buf), _stream()), 'halo_lora_pack')
    na, nb = R * n_in, R * n_out
    return (buf[:na].view(R, n_in), buf[na:2 * na].view(n_in, R), buf[2 * na:2 * na + nb].view(n_out, R), buf[2 * na + nb:].view(R, n_out))


def _bf16_rows(t, name, cols=None):
    if t.dtype != torch.bfloat16 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f'{name}: expected row-major bf16 rows on the HIP device')
    return t


def lora_down(x, p16, scale=1.0, drop=NO_DROPOUT, stream_id=0):
    """U [M, 16] = scale * (mask * x [M, K]) p16 [16, K]^T as bf16; the mask of ``drop`` at the flat index row * K + col."""
    _bf16_rows(x, 'x'); _bf16_rows(p16, 'p16')
    M, K = x.shape
    if p16.shape != (LORA_RANK_PAD, K) or not p16.is_contiguous():
        raise ValueError('lora_down: p16 [16, K]')
    u = torch.empty(M, LORA_RANK_PAD, device=x.device, dtype=torch.bfloat16)
    check(lib().halo_lora_down(ptr(x), x.stride(0), ptr(p16), M, K, float(scale), ptr(u), drop.p, drop.seed, stream_id, drop.offset,
                               drop.counter_ptr, _stream()), 'halo_lora_down')
    return u


def lora_up_(y, u, p16, scale=1.0, drop=NO_DROPOUT, stream_id=0):
    """y [M, N] += scale * mask * (u [M, 16] p16 [N, 16]^T) in place; y row-major bf16 or fp32; the mask at the flat index row * N + col."""
    _bf16_rows(u, 'u', LORA_RANK_PAD); _bf16_rows(p16, 'p16', LORA_RANK_PAD)
    M, N = y.shape
    if y.dtype not in (torch.bfloat16, torch.float32) or y.stride(1) != 1 or u.shape[0] != M or p16.shape[0] != N \
            or not u.is_contiguous() or not p16.is_contiguous():
        raise ValueError('lora_up_: y [M, N] bf16 / fp32 rows, u [M, 16], p16 [N, 16]')
    b16 = y.dtype == torch.bfloat16
    check(lib().halo_lora_up(ptr(u), ptr(p16), M, N, float(scale), ptr(y) if b16 else None, None if b16 else ptr(y), y.stride(0), drop.p,
                             drop.seed, stream_id, drop.offset, drop.counter_ptr, _stream()), 'halo_lora_up')
    return y


def lora_tn(u, x, r, scale=1.0, transpose_out=False, drop=NO_DROPOUT, stream_id=0):
    """scale * u [M, 16]^T (mask * x [M, K]), rows 0 .. r-1: fp32 [r, K], or [K, r] with ``transpose_out``.  Slabs of M summed in a fixed
    order: bitwise reproducible."""
    _bf16_rows(u, 'u', LORA_RANK_PAD); _bf16_rows(x, 'x')
    M, K = x.shape
    if u.shape[0] != M or not u.is_contiguous():
        raise ValueError('lora_tn: u [M, 16] contiguous')
    g = torch.empty((K, r) if transpose_out else (r, K), device=x.device, dtype=torch.float32)
    ws = torch.empty(lib().halo_lora_tn_workspace_bytes(M, K), device=x.device, dtype=torch.uint8)
    check(lib().halo_lora_tn(ptr(u), ptr(x), x.stride(0), M, K, r, float(scale), int(transpose_out), ptr(g), ptr(ws), drop.p, drop.seed,
                             stream_id, drop.offset, drop.counter_ptr, _stream()), 'halo_lora_tn')
    return g


def dropout_fwd(x, drop, stream_id):
    _f32c(x, 'x')
    y = torch.empty_like(x)
    check(lib().halo_dropout_fwd(ptr(x), ptr(y), x.numel(), drop.p, drop.seed, stream_id, drop.offset,
                                 drop.counter_ptr, _stream()), 'halo_dropout_fwd')
    return y


def subsample_fwd(x, w, bias, drop, ks=5, stride=4, pad=3):
    """x [B,T,F] -> y [T',B,C] time-major, col (saved im2col image)."""
    _f32c(x, 'inputs'); _f32c(w, 'subsample.weight'); _f32c(bias, 'subsample.bias')
    B, T, F = x.shape
    Cc = w.shape[0]
    Tp = subsampled_length(T, ks, stride, pad)
    y = torch.empty(Tp, B, Cc, device=x.device, dtype=torch.float32)
    col = torch.empty(Tp * B, F * ks, device=x.device, dtype=torch.float32)
    check(lib().halo_subsample_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), ptr(col), B, T, F, Cc, ks, stride, pad,
                                   drop.p, drop.seed, drop.offset, drop.counter_ptr, _stream()), 'halo_subsample_fwd')
    return y, col


def subsample_bwd(dy, y, col, B, T, F, Cc, p_drop, dw=None, dbias=None, ks=5, stride=4, pad=3, slabs=1):
    """``slabs`` > 1: ``dy`` is [slabs, T', B, C], the gradient left as that many K-slices by ``lstm_bwd(..., dx_slabs=)``; they are added
    while they are read."""
    _f32c(dy, 'dy')
    if slabs > 1 and dy.numel() < slabs * y.numel():
        raise ValueError('haloop_amd.ops.subsample_bwd: dy holds fewer than `slabs` matrices')
    dpre = torch.empty_like(y)
    if dw is None:
        dw = torch.empty(Cc, F, ks, device=y.device, dtype=torch.float32)
    if dbias is None:
        dbias = torch.empty(Cc, device=y.device, dtype=torch.float32)
    check(lib().halo_subsample_bwd_slabs(ptr(dy), int(slabs), ptr(y), ptr(col), ptr(dpre), ptr(dw), ptr(dbias), B, T, F, Cc, ks, stride,
                                         pad, p_drop, _stream()), 'halo_subsample_bwd_slabs')
    return dw, dbias


def lstm_fwd(x_tm, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None, y=None, y_strides=None, y_relu=False,
             want_state=False, drop=NO_DROPOUT, expect_backward=True, reserve=None, weights_stamp=0):
    """x_tm [T,B,in] time-major.  Returns (y, hn, cn, reserve).
    expect_backward=False (inference): the two-layer launch packs only the forward's weight images (include/halo.h); with a
    caller-owned ``reserve`` (ops.lstm_reserve) and a non-zero ``weights_stamp`` that changes whenever the weights do, it keeps the
    images the previous call left there (halo_set_lstm_weights_stamp).

    y defaults to a time-major [T,B,H] tensor; pass a preallocated ``y`` with ``y_strides`` =
    (stride_t, stride_b) in elements to have the last layer write e.g. batch-first."""
    _f32c(x_tm, 'x')
    T, B, in0 = x_tm.shape
    L = len(w_hh)
    H = w_hh[0].shape[1]
    for t in list(w_ih) + list(w_hh) + list(b_ih) + list(b_hh):
        _f32c(t, 'lstm parameter')
    dev = x_tm.device
    if y is None:
        y = torch.empty(T, B, H, device=dev, dtype=torch.float32)
        y_strides = (B * H, H)
    need = (lib().halo_lstm_reserve_bytes(T, B, in0, H, L) + 3) // 4
    if reserve is None:
        reserve = torch.empty(need, device=dev, dtype=torch.float32)
    elif reserve.dtype != torch.float32 or reserve.numel() < need or not reserve.is_contiguous():
        raise ValueError('lstm_fwd: the reserve is too small for this shape (ops.lstm_reserve)')
    hn = torch.empty(L, B, H, device=dev, dtype=torch.float32) if want_state else None
    cn = torch.empty(L, B, H, device=dev, dtype=torch.float32) if want_state else None
    if h0 is not None:
        _f32c(h0, 'h0'); _f32c(c0, 'c0')
    a_ih, a_hh, a_bi, a_bh = ptr_array(w_ih), ptr_array(w_hh), ptr_array(b_ih), ptr_array(b_hh)
    if not expect_backward:
        lib().halo_set_lstm_expect_backward(0)
        lib().halo_set_lstm_weights_stamp(int(weights_stamp))
    try:
        check(lib().halo_lstm_fwd(ptr(x_tm), a_ih, a_hh, a_bi, a_bh, ptr(h0), ptr(c0), ptr(y), y_strides[0], y_strides[1],
                                  int(y_relu), ptr(hn), ptr(cn), ptr(reserve), T, B, in0, H, L, drop.p, drop.seed,
                                  drop.offset, drop.counter_ptr, _stream()), 'halo_lstm_fwd')
    finally:
        if not expect_backward:
            lib().halo_set_lstm_expect_backward(1)
            lib().halo_set_lstm_weights_stamp(0)
    return y, hn, cn, reserve


def lstm_reserve(T, B, in0, H, L, device):
    """A reserve buffer the caller owns (lstm_fwd(reserve=...))."""
    return torch.empty((lib().halo_lstm_reserve_bytes(T, B, in0, H, L) + 3) // 4, device=device, dtype=torch.float32)


def lstm_bwd_workspace(x_tm, w_hh):
    T, B, in0 = x_tm.shape
    return torch.empty((lib().halo_lstm_bwd_workspace_bytes(T, B, in0, w_hh[0].shape[1], len(w_hh)) + 3) // 4,
                       device=x_tm.device, dtype=torch.float32)


def lstm_bwd(x_tm, w_ih, w_hh, dy, y_strides, y_relu, reserve, dhn=None, dcn=None, want_dx=False,
             grads=None, drop=NO_DROPOUT, layers=None, workspace=None, dx=None, dx_slabs=1):
    """Returns (dx or None, grads dict of lists dw_ih/dw_hh/db_ih/db_hh).  ``grads`` may carry
    preallocated outputs.  ``layers=(lo, hi)`` runs only that range (top down); a split backward
    passes the same ``workspace`` (ops.lstm_bwd_workspace) to both calls.
    ``dx_slabs`` > 1: ``dx`` has room for that many [T, B, in] matrices and the call may leave the input gradient there as unreduced
    K-slices; ``lstm_dx_slabs_left()`` right after the call says how many (1: dx[0] is the gradient), for ``subsample_bwd(slabs=)``."""
    T, B, in0 = x_tm.shape
    L = len(w_hh)
    H = w_hh[0].shape[1]
    dev = x_tm.device
    if grads is None:
        grads = {
            'dw_ih': [torch.empty_like(w) for w in w_ih],
            'dw_hh': [torch.empty_like(w) for w in w_hh],
            'db_ih': [torch.empty(4 * H, device=dev, dtype=torch.float32) for _ in range(L)],
            'db_hh': [torch.empty(4 * H, device=dev, dtype=torch.float32) for _ in range(L)],
        }
    ws = workspace if workspace is not None else lstm_bwd_workspace(x_tm, w_hh)
    lo, hi = layers if layers is not None else (0, L)
    if dx is None and want_dx and lo == 0:
        dx = torch.empty(T, B, in0, device=dev, dtype=torch.float32)
    a_ih, a_hh = ptr_array(w_ih), ptr_array(w_hh)
    g_ih, g_hh = ptr_array(grads['dw_ih']), ptr_array(grads['dw_hh'])
    g_bi, g_bh = ptr_array(grads['db_ih']), ptr_array(grads['db_hh'])
    if dx_slabs > 1:
        if dx is None or dx.numel() < dx_slabs * T * B * in0:
            raise ValueError('haloop_amd.ops.lstm_bwd: dx_slabs needs a dx buffer of that many [T, B, in] matrices')
        check(lib().halo_set_lstm_dx_slabs(int(dx_slabs)), 'halo_set_lstm_dx_slabs')
    try:
        check(lib().halo_lstm_bwd(ptr(x_tm), a_ih, a_hh, ptr(dy), y_strides[0], y_strides[1], int(y_relu), ptr(dhn),
                                  ptr(dcn), ptr(reserve), ptr(ws), ptr(dx), g_ih, g_hh, g_bi, g_bh, T, B, in0, H, L, lo, hi,
                                  drop.p, drop.seed, drop.offset, drop.counter_ptr, _stream()), 'halo_lstm_bwd')
    finally:
        if dx_slabs > 1:
            lib().halo_set_lstm_dx_slabs(1)
    return dx, grads


def relu_dropout_bwd(dy, y, p_drop):
    """dpre = dy * (y > 0 ? 1 / (1 - p) : 0): the gradient at the pre-activation of relu + inverted dropout, the mask read off y."""
    _f32c(dy, 'dy'); _f32c(y, 'y')
    if dy.numel() != y.numel():
        raise ValueError('haloop_amd.ops.relu_dropout_bwd: dy and y differ in size')
    dpre = torch.empty_like(y)
    check(lib().halo_relu_dropout_bwd(ptr(dy), ptr(y), ptr(dpre), y.numel(), float(p_drop), _stream()), 'halo_relu_dropout_bwd')
    return dpre


def _ghost_operand(t, time_major, N, T, name):
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise ValueError(f'{name}: expected a 3-d float32 HIP tensor with unit stride along K')
    n_dim, t_dim = (1, 0) if time_major else (0, 1)
    if t.shape[n_dim] != N or t.shape[t_dim] != T:
        raise ValueError(f'{name}: shape {tuple(t.shape)} does not hold N = {N} utterances of T = {T} frames')
    return _lib.GhostOperand(t.data_ptr(), t.stride(n_dim), t.stride(t_dim), t.shape[2])


def ghost_term(a, bs=(), n_bias=0, time_major=False):
    """One term of ``ghost_sqnorm``: ``a`` and up to two ``bs``, each [N, T, K] (or [T, N, K] when ``time_major``) with any batch / frame
    strides, read in place; ``n_bias`` bias vectors with gradient sum_t a_t.  The record keeps its tensors alive."""
    bs = tuple(bs)
    if len(bs) > 2 or not 0 <= int(n_bias) <= 2:
        raise ValueError('haloop_amd.ops.ghost_term: at most two b operands and two bias vectors')
    N, T = (a.shape[1], a.shape[0]) if time_major else (a.shape[0], a.shape[1])
    tm = _lib.GhostTerm()
    tm.a = _ghost_operand(a, time_major, N, T, 'a')
    for j, b in enumerate(bs):
        tm.b[j] = _ghost_operand(b, time_major, N, T, f'b{j}')
    tm.n_b, tm.n_bias = len(bs), int(n_bias)
    tm.tensors = (a,) + bs
    return tm


def lstm_ghost_terms(x_tm, reserve, H, L, p_drop=0.0):
    """The LSTM's terms (one per layer: dG against the layer's input and h_{t-1}, two biases), read off the ``reserve`` that ``lstm_fwd`` and a
    whole ``lstm_bwd`` under ``_lib.set_lstm_keep_gate_gradients(True)`` have gone through (include/halo.h: halo_lstm_ghost_terms)."""
    _f32c(x_tm, 'x')
    T, B, in0 = x_tm.shape
    arr = (_lib.GhostTerm * L)()
    check(lib().halo_lstm_ghost_terms(ptr(x_tm), ptr(reserve), T, B, in0, H, L, float(p_drop), arr), 'halo_lstm_ghost_terms')
    terms = []
    for l in range(L):
        tm = _lib.GhostTerm.from_buffer_copy(arr[l])
        tm.tensors = (x_tm, reserve)
        terms.append(tm)
    return terms


def ghost_sqnorm(terms, N, T, want_norm=False, workspace=None, out=None, norm_out=None):
    """sq [n_terms, N]: per term and utterance, sum_{t,t'} <a_t, a_t'> (n_bias + sum_j <b^j_t, b^j_t'>) = the squared Frobenius norm of the
    utterance's own gradient of the term's parameters (csrc/ghost_norm.hip: exact-f32 MFMA, one launch for all terms plus a fixed-order
    sum).  ``want_norm``: also norm [N] = sqrt(sum over terms), from the same second launch.  ``workspace`` (ghost_sqnorm_workspace floats),
    ``out`` and ``norm_out`` may be the caller's."""
    terms = list(terms)
    if not terms:
        raise ValueError('haloop_amd.ops.ghost_sqnorm: no terms')
    dev = terms[0].tensors[0].device
    arr = (_lib.GhostTerm * len(terms))(*terms)
    need = ghost_sqnorm_workspace(len(terms), N, T)
    ws = workspace if workspace is not None else torch.empty(need, device=dev, dtype=torch.float32)
    if ws.dtype != torch.float32 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError('haloop_amd.ops.ghost_sqnorm: the workspace is too small (ops.ghost_sqnorm_workspace)')
    sq = out if out is not None else torch.empty(len(terms), N, device=dev, dtype=torch.float32)
    _f32c(sq, 'out')
    if sq.numel() != len(terms) * N:
        raise ValueError('haloop_amd.ops.ghost_sqnorm: out must hold [n_terms, N] floats')
    norm = norm_out if norm_out is not None else (torch.empty(N, device=dev, dtype=torch.float32) if want_norm else None)
    if norm is not None and (_f32c(norm, 'norm_out').numel() != N):
        raise ValueError('haloop_amd.ops.ghost_sqnorm: norm_out must hold N floats')
    check(lib().halo_ghost_sqnorm(arr, len(terms), N, T, ptr(ws), ptr(sq), ptr(norm), _stream()), 'halo_ghost_sqnorm')
    return (sq, norm) if norm is not None else sq


def ghost_sqnorm_workspace(n_terms, N, T):
    """Floats of workspace ``ghost_sqnorm`` needs (one partial per term, utterance and pair of frame tiles)."""
    return max(1, lib().halo_ghost_sqnorm_workspace_bytes(n_terms, N, T) // 4)


def ghost_tile():
    """Frames per tile of the ghost-norm kernel."""
    return int(lib().halo_ghost_tile())


class defer_small_jobs:
    """``with ops.defer_small_jobs():`` -- the small fixed-order reductions at the end of a backward pass (the CTC head's partial sums, the
    two-layer LSTM launch's bias-gradient partials) are queued on the context instead of launched, and ride in the tail blocks of the conv
    backward's reduce launch (``subsample_bwd``); whatever is still queued at the end of the block runs in one launch of its own.  The
    buffers those reductions read must live until then (``ctc_head_bwd(workspace=)``, the LSTM backward's workspace)."""

    def __enter__(self):
        self.begin()
        return self

    def __exit__(self, *exc):
        self.end()
        return False

    @staticmethod
    def begin():
        check(lib().halo_set_defer_small_jobs(1), 'halo_set_defer_small_jobs')

    @staticmethod
    def end():
        try:
            check(lib().halo_flush_small_jobs(_stream()), 'halo_flush_small_jobs')
        finally:
            lib().halo_set_defer_small_jobs(0)


def lstm_dx_slabs_left():
    """How many K-slices the last ``lstm_bwd`` of this thread's context left in its dx buffer (1: the gradient itself)."""
    return int(lib().halo_lstm_dx_slabs_left())


def log_softmax_fwd(x2d):
    _f32c(x2d, 'logits')
    y = torch.empty_like(x2d)
    check(lib().halo_log_softmax_fwd(ptr(x2d), ptr(y), x2d.shape[0], x2d.shape[1], _stream()), 'halo_log_softmax_fwd')
    return y


def log_softmax_bwd(dy2d, y2d):
    _f32c(dy2d, 'dy'); _f32c(y2d, 'y')
    dx = torch.empty_like(y2d)
    check(lib().halo_log_softmax_bwd(ptr(dy2d), ptr(y2d), ptr(dx), y2d.shape[0], y2d.shape[1], _stream()),
          'halo_log_softmax_bwd')
    return dx


def colsum(x2d, out=None):
    _f32c(x2d, 'x')
    if out is None:
        out = torch.empty(x2d.shape[1], device=x2d.device, dtype=torch.float32)
    check(lib().halo_colsum(ptr(x2d), x2d.shape[0], x2d.shape[1], x2d.shape[1], ptr(out), _stream()), 'halo_colsum')
    return out


def _i64c(t, name):
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    if not t.is_cuda:
        raise ValueError(f'{name}: expected a HIP tensor')
    return t.contiguous()


def ctc_fwd(lp, time_major, targets, input_lengths, target_lengths, flags=0):
    """lp: [T,N,C] (time_major) or [N,T,C]; any strides with a unit class stride.  -> (nll [N], alpha)."""
    if lp.dtype != torch.float32 or lp.stride(-1) != 1:
        raise ValueError('log-probs must be float32 with unit class stride')
    if time_major:
        T, N, Cn = lp.shape
        st, sn = lp.stride(0), lp.stride(1)
    else:
        N, T, Cn = lp.shape
        sn, st = lp.stride(0), lp.stride(1)
    targets = _i64c(targets, 'targets')
    if targets.dim() != 2:
        raise ValueError('targets must be [N,S] (padded); concatenated targets are not supported')
    S = targets.shape[1]
    tl = _i64c(target_lengths, 'target_lengths')
    il = None if input_lengths is None else _i64c(input_lengths, 'input_lengths')
    alpha = torch.empty(N, T, 2 * S + 1, device=lp.device, dtype=torch.float32)
    nll = torch.empty(N, device=lp.device, dtype=torch.float32)
    check(lib().halo_ctc_fwd(ptr(lp), st, sn, T, N, Cn, ptr(targets), targets.stride(0), S, ptr(il), ptr(tl), flags,
                             ptr(alpha), ptr(nll), _stream()), 'halo_ctc_fwd')
    return nll, alpha, (targets, il, tl)


def ctc_bwd(lp, time_major, saved, alpha, nll, grad_out):
    targets, il, tl = saved
    if time_major:
        T, N, Cn = lp.shape
        st, sn = lp.stride(0), lp.stride(1)
    else:
        N, T, Cn = lp.shape
        sn, st = lp.stride(0), lp.stride(1)
    S = targets.shape[1]
    grad = torch.empty(lp.shape, device=lp.device, dtype=torch.float32)
    gst, gsn = (grad.stride(0), grad.stride(1)) if time_major else (grad.stride(1), grad.stride(0))
    beta = torch.empty_like(alpha)
    grad_out = grad_out.to(torch.float32).contiguous()
    check(lib().halo_ctc_bwd(ptr(lp), st, sn, T, N, Cn, ptr(targets), targets.stride(0), S, ptr(il), ptr(tl),
                             ptr(alpha), ptr(nll), ptr(grad_out), ptr(beta), ptr(grad), gst, gsn, _stream()),
          'halo_ctc_bwd')
    return grad


def ctc_prepare(input_lengths, target_lengths, ks=5, stride=4, pad=3):
    """-> (feature_lengths int64 [N], grad_out f32 [N]) in one launch."""
    il, tl = _i64c(input_lengths, 'input_lengths'), _i64c(target_lengths, 'target_lengths')
    n = il.numel()
    flen = torch.empty(n, device=il.device, dtype=torch.int64)
    gout = torch.empty(n, device=il.device, dtype=torch.float32)
    check(lib().halo_ctc_prepare(ptr(il), ptr(tl), n, ks, stride, pad, ptr(flen), ptr(gout), _stream()), 'halo_ctc_prepare')
    return flen, gout


def ctc_mean_loss(nll, target_lengths, out):
    tl = _i64c(target_lengths, 'target_lengths')
    check(lib().halo_ctc_mean_loss(ptr(nll), ptr(tl), nll.numel(), ptr(out), _stream()), 'halo_ctc_mean_loss')
    return out


def ctc_head_supported(T, H, V, S):
    return bool(lib().halo_ctc_head_supported(T, H, V, S))


def ctc_head_fwd(feats, weight, bias, drop, stream_id, input_lengths, targets, target_lengths, loss, ticket, ks=5, stride=4, pad=3):
    """The CTC head's forward in one launch (include/halo.h): feats [B,T,H] -> (lp, alpha, nll, feature_lengths, grad_out); the mean
    loss goes to ``loss`` (device scalar); ``ticket``: a zero-initialised device int32 the caller keeps."""
    _f32c(feats, 'features')
    B, T, H = feats.shape
    V = weight.shape[0]
    tg = _i64c(targets, 'targets')
    il, tl = _i64c(input_lengths, 'input_lengths'), _i64c(target_lengths, 'target_lengths')
    S = tg.shape[1]
    dev = feats.device
    lp = torch.empty(B, T, V, device=dev, dtype=torch.float32)
    alpha = torch.empty(B, T, 2 * S + 1, device=dev, dtype=torch.float32)
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    flen = torch.empty(B, device=dev, dtype=torch.int64)
    grad_out = torch.empty(B, device=dev, dtype=torch.float32)
    check(lib().halo_ctc_head_fwd(ptr(feats), ptr(weight), ptr(bias), drop.p, drop.seed, stream_id, drop.offset, drop.counter_ptr,
                                  ptr(il), ks, stride, pad, ptr(tg), tg.stride(0), S, ptr(tl), ptr(lp), ptr(alpha), ptr(nll), ptr(flen),
                                  ptr(grad_out), ptr(loss), ptr(ticket), B, T, H, V, _stream()), 'halo_ctc_head_fwd')
    return lp, alpha, nll, flen, grad_out, (tg, tl)


def ctc_head_train_workspace(B, H, V, device):
    return torch.empty(lib().halo_ctc_head_train_workspace_bytes(B, H, V), device=device, dtype=torch.uint8)


def ctc_head_train_ticket(B, H, device):
    """The zero-initialised words ``ctc_head_train`` keeps between calls (loss ticket, launch count, the slices' tagged partial logits)."""
    return torch.zeros(lib().halo_ctc_head_train_ticket_words(B, H), device=device, dtype=torch.int32)


def ctc_head_train(feats, weight, bias, drop, stream_id, input_lengths, targets, target_lengths, loss, ticket, dweight, dbias,
                   workspace=None, want_lp=False, ks=5, stride=4, pad=3):
    """The CTC head of a training step, forward and backward, in ONE launch (include/halo.h: halo_ctc_head_train; not in the exact-f32
    mode).  feats [B,T,H] -> (d features [B,T,H], nll [B], feature_lengths [B], lp or None); the mean loss goes to ``loss``, the classifier's
    gradients to dweight / dbias (deferred like ``ctc_head_bwd``'s).  ``ticket``: ``ctc_head_train_ticket(B, H, device)``, the caller's to keep between calls."""
    _f32c(feats, 'features')
    B, T, H = feats.shape
    V = weight.shape[0]
    tg = _i64c(targets, 'targets')
    il, tl = _i64c(input_lengths, 'input_lengths'), _i64c(target_lengths, 'target_lengths')
    need = lib().halo_ctc_head_train_ticket_words(B, H)
    if ticket.numel() < need:
        raise ValueError(f'ctc_head_train: ticket must hold {need} words (ctc_head_train_ticket), has {ticket.numel()}')
    dev = feats.device
    lp = torch.empty(B, T, V, device=dev, dtype=torch.float32) if want_lp else None
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    flen = torch.empty(B, device=dev, dtype=torch.int64)
    dfeats = torch.empty_like(feats)
    ws = workspace if workspace is not None else ctc_head_train_workspace(B, H, V, dev)
    check(lib().halo_ctc_head_train(ptr(feats), ptr(weight), ptr(bias), drop.p, drop.seed, stream_id, drop.offset, drop.counter_ptr,
                                    ptr(il), ks, stride, pad, ptr(tg), tg.stride(0), tg.shape[1], ptr(tl), ptr(lp) if want_lp else None,
                                    ptr(nll), ptr(flen), ptr(loss), ptr(ticket), ptr(dfeats), ptr(dweight), ptr(dbias), ptr(ws),
                                    B, T, H, V, _stream()), 'halo_ctc_head_train')
    return dfeats, nll, flen, lp


def ctc_head_workspace(B, H, V, device):
    return torch.empty(lib().halo_ctc_head_workspace_bytes(B, H, V), device=device, dtype=torch.uint8)


def ctc_head_bwd(feats, weight, drop, stream_id, flen, tg, tl, lp, alpha, nll, grad_out, dweight, dbias, workspace=None):
    """The CTC head's backward (two launches): returns d features [B,T,H]; the classifier's gradients go to dweight / dbias.
    Inside ``defer_small_jobs()`` the second launch (the fixed-order sum of the per-utterance partials) is queued instead and dweight /
    dbias are complete after the block's flush; the caller then passes a ``workspace`` (``ctc_head_workspace``) that lives that long."""
    B, T, H = feats.shape
    V = weight.shape[0]
    dfeats = torch.empty_like(feats)
    ws = workspace if workspace is not None else ctc_head_workspace(B, H, V, feats.device)
    check(lib().halo_ctc_head_bwd(ptr(feats), ptr(weight), drop.p, drop.seed, stream_id, drop.offset, drop.counter_ptr, ptr(flen), ptr(tg),
                                  tg.stride(0), tg.shape[1], ptr(tl), ptr(lp), ptr(alpha), ptr(nll), ptr(grad_out), ptr(dfeats),
                                  ptr(dweight), ptr(dbias), ptr(ws), B, T, H, V, _stream()), 'halo_ctc_head_bwd')
    return dfeats


def ctc_greedy(lp):
    _f32c(lp, 'log-probs')
    N, T, Cn = lp.shape
    dev = lp.device
    ali = torch.empty(N, T, device=dev, dtype=torch.int64)
    scores = torch.empty(N, T, device=dev, dtype=torch.float32)
    hyp = torch.zeros(N, T, device=dev, dtype=torch.int64)
    hyp_len = torch.empty(N, device=dev, dtype=torch.int64)
    check(lib().halo_ctc_greedy(ptr(lp), N, T, Cn, ptr(ali), ptr(scores), ptr(hyp), ptr(hyp_len), _stream()),
          'halo_ctc_greedy')
    return ali, scores, hyp, hyp_len


def ctc_head_greedy(feats, weight, bias, want_lp=False):
    """feats [B,T,H] -> (alignments, scores, hyp (zero padded), hyp_len[, log-probs]): classifier + log_softmax + greedy collapse in one launch."""
    _f32c(feats, 'features')
    B, T, H = feats.shape
    V = weight.shape[0]
    dev = feats.device
    ali = torch.empty(B, T, device=dev, dtype=torch.int64)
    scores = torch.empty(B, T, device=dev, dtype=torch.float32)
    hyp = torch.empty(B, T, device=dev, dtype=torch.int64)
    hyp_len = torch.empty(B, device=dev, dtype=torch.int64)
    lp = torch.empty(B, T, V, device=dev, dtype=torch.float32) if want_lp else None
    check(lib().halo_ctc_head_greedy(ptr(feats), ptr(weight), ptr(bias), ptr(lp), ptr(ali), ptr(scores), ptr(hyp), ptr(hyp_len), B, T, H, V,
                                     _stream()), 'halo_ctc_head_greedy')
    return (ali, scores, hyp, hyp_len, lp) if want_lp else (ali, scores, hyp, hyp_len)


STREAM_ACTIVE, STREAM_BEGIN, STREAM_FINAL = 1, 2, 4        # per-stream flag bits of stream_front / stream_head (include/halo.h)


def stream_front(frames, carry, length, flags, w, bias, y, n_steps, h, c, hyp, hyp_len, steps, score, last_label, truncated):
    """The convolution of one streamed chunk (include/halo.h: halo_stream_front).  frames [B,Tc,F], carry [B,3,F] (updated in place),
    length / flags [B] int32 on the device -> y [S,B,C] (S from ``y``) and n_steps [B] int32; beginning streams have their rows of the
    state h / c [L,B,H], of hyp [B,capacity] int64 and of the hypothesis bookkeeping reset.  Every tensor is the caller's: nothing is
    allocated."""
    _f32c(frames, 'frames'); _f32c(carry, 'carry'); _f32c(w, 'subsample.weight'); _f32c(bias, 'subsample.bias'); _f32c(y, 'y')
    _f32c(h, 'h'); _f32c(c, 'c')
    B, Tc, F = frames.shape
    S, Cc = y.shape[0], y.shape[2]
    L, H = h.shape[0], h.shape[2]
    if carry.shape != (B, 3, F) or y.shape[1] != B or w.shape != (Cc, F, 5) or h.shape[1] != B or c.shape != h.shape:
        raise ValueError('stream_front: carry [B,3,F], y [S,B,C], weight [C,F,5] and h / c [L,B,H] do not fit frames [B,Tc,F]')
    for t, dt, name in ((length, torch.int32, 'length'), (flags, torch.int32, 'flags'), (n_steps, torch.int32, 'n_steps'),
                        (hyp_len, torch.int64, 'hyp_len'), (steps, torch.int64, 'steps'), (score, torch.float32, 'score'),
                        (last_label, torch.int32, 'last_label'), (truncated, torch.bool, 'truncated')):
        if t.dtype != dt or t.numel() != B or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'stream_front: {name} must be a contiguous {dt} HIP tensor of {B} elements')
    if hyp.dtype != torch.int64 or hyp.dim() != 2 or hyp.shape[0] != B or not hyp.is_cuda or not hyp.is_contiguous():
        raise ValueError(f'stream_front: hyp must be a contiguous int64 HIP tensor [{B}, capacity]')
    check(lib().halo_stream_front(ptr(frames), ptr(carry), ptr(length), ptr(flags), ptr(w), ptr(bias), ptr(y), ptr(n_steps), ptr(h), ptr(c),
                                  ptr(hyp), ptr(hyp_len), ptr(steps), ptr(score), ptr(last_label), ptr(truncated), B, Tc, F, Cc, S, L, H,
                                  hyp.shape[1], _stream()), 'halo_stream_front')
    return y, n_steps


def stream_head_fused(S, H, V):
    """Whether ``stream_head`` runs the classifier product itself at this shape (else the caller hands it log-probs)."""
    return ctc_head_supported(S, H, V, 0) and _lib.get_math_mode() != 'f32'


def stream_head(feats, weight, bias, n_steps, flags, hn, cn, h, c, ali, step_scores, hyp, hyp_len, steps, score, last_label, truncated,
                lp_out=None):
    """The CTC head of one streamed chunk (include/halo.h: halo_stream_head): feats [B,S,H] -> classifier, log-softmax, best class per
    step, the collapse continued across calls, and the commit of hn / cn into h / c for the streams that go on.  Where the fused product
    does not apply (``stream_head_fused``) the log-probs come from ``gemm`` + ``log_softmax_fwd`` and the kernel runs collapse-only.
    ``lp_out`` [B,S,V]: receives the log-probs."""
    _f32c(feats, 'features')
    B, S, H = feats.shape
    V = weight.shape[0]
    if not stream_head_fused(S, H, V):
        logits = gemm(feats.view(B * S, H), weight, True, True, B * S, V, H, bias1=bias)
        lp = log_softmax_fwd(logits).view(B, S, V)
        if lp_out is not None:
            lp_out.copy_(lp)
        stream_collapse(lp, n_steps, flags, hn, cn, h, c, ali, step_scores, hyp, hyp_len, steps, score, last_label, truncated)
        return
    check(lib().halo_stream_head(ptr(feats), ptr(weight), ptr(bias), None, ptr(lp_out), ptr(n_steps), ptr(flags), ptr(hn), ptr(cn),
                                 ptr(h), ptr(c), ptr(ali), ptr(step_scores), ptr(hyp), ptr(hyp_len), ptr(steps), ptr(score),
                                 ptr(last_label), ptr(truncated), B, S, H, V, h.shape[0], hyp.shape[1], _stream()), 'halo_stream_head')


def stream_collapse(lp, n_steps, flags, hn, cn, h, c, ali, step_scores, hyp, hyp_len, steps, score, last_label, truncated):
    """``stream_head``'s collapse-only mode on log-probs [B,S,V] the caller holds (any V)."""
    _f32c(lp, 'log-probs')
    B, S, V = lp.shape
    check(lib().halo_stream_head(None, None, None, ptr(lp), None, ptr(n_steps), ptr(flags), ptr(hn), ptr(cn), ptr(h), ptr(c), ptr(ali),
                                 ptr(step_scores), ptr(hyp), ptr(hyp_len), ptr(steps), ptr(score), ptr(last_label), ptr(truncated),
                                 B, S, h.shape[2], V, h.shape[0], hyp.shape[1], _stream()), 'halo_stream_head')


def stream_logits(feats, weight, bias, f, n_steps, flags, hn, cn, h, c, steps):
    """The transducer head of one streamed chunk (include/halo.h: halo_stream_logits): f [B,S,V] <- classifier(feats [B,S,H]) for each
    stream's n_steps, zeros past them, no softmax; steps [B] int64 += n_steps; hn / cn committed into h / c for the streams that go on.
    Where the fused product does not apply (``stream_head_fused``) the product comes from ``gemm`` and the launch runs commit-only."""
    _f32c(feats, 'features'); _f32c(f, 'logits')
    B, S, H = feats.shape
    V = weight.shape[0]
    if f.shape != (B, S, V) or steps.dtype != torch.int64 or steps.numel() != B:
        raise ValueError(f'stream_logits: f must be [{B}, {S}, {V}] and steps int64 [{B}]')
    fused = stream_head_fused(S, H, V)
    if not fused:
        gemm(feats.view(B * S, H), weight, True, True, B * S, V, H, out=f.view(B * S, V), bias1=bias)
    check(lib().halo_stream_logits(ptr(feats) if fused else None, ptr(weight), ptr(bias), ptr(f), ptr(n_steps), ptr(flags), ptr(hn), ptr(cn),
                                   ptr(h), ptr(c), ptr(steps), B, S, H, V, h.shape[0], _stream()), 'halo_stream_logits')


def ctc_beam(em, beam, log_domain=True):
    """em [N,T,V] -> (seqs [N,beam,T] int64, lens [N,beam] int32, scores [N,beam])."""
    _f32c(em, 'emissions')
    N, T, V = em.shape
    dev = em.device
    seqs = torch.empty(N, beam, T, device=dev, dtype=torch.int64)
    lens = torch.empty(N, beam, device=dev, dtype=torch.int32)
    scores = torch.empty(N, beam, device=dev, dtype=torch.float32)
    ws = torch.empty(lib().halo_ctc_beam_workspace_bytes(N, T, V, beam), device=dev, dtype=torch.uint8)
    check(lib().halo_ctc_beam(ptr(em), N, T, V, beam, int(log_domain), ptr(seqs), ptr(lens), ptr(scores), ptr(ws),
                              _stream()), 'halo_ctc_beam')
    return seqs, lens, scores


def logaddexp_aten(a, b):
    """torch.logaddexp(a, b) with ATen's CPU arithmetic bit for bit (1-D contiguous float32; see halo_set_beam_vector_chunk)."""
    _f32c(a, 'a'); _f32c(b, 'b')
    out = torch.empty_like(a)
    check(lib().halo_logaddexp_aten(ptr(a), ptr(b), ptr(out), a.numel(), _stream()), 'halo_logaddexp_aten')
    return out


def topk(values2d, k):
    """Row-wise top-k in torch.topk's CPU order (ties included). -> (values [rows,k], indices [rows,k] int64)"""
    _f32c(values2d, 'values')
    rows, n = values2d.shape
    dev = values2d.device
    vals = torch.empty(rows, k, device=dev, dtype=torch.float32)
    idx = torch.empty(rows, k, device=dev, dtype=torch.int64)
    ws = torch.empty(rows * n * 8, device=dev, dtype=torch.uint8)
    check(lib().halo_topk_f32(ptr(values2d), rows, n, k, ptr(vals), ptr(idx), ptr(ws), _stream()), 'halo_topk_f32')
    return vals, idx


def sumsq_partials(flat, partials=None):
    if partials is None:
        partials = torch.empty(_lib.HALO_SUMSQ_PARTS, device=flat.device, dtype=torch.float32)
    check(lib().halo_sumsq(ptr(flat), flat.numel(), ptr(partials), _stream()), 'halo_sumsq')
    return partials


def _range_arrays(ranges):
    n = len(ranges)
    return n, (C.c_size_t * n)(*[int(r[0]) for r in ranges]), (C.c_size_t * n)(*[int(r[1]) for r in ranges])


def sumsq_ranges(flat, ranges, partials):
    """partials[0:HALO_SUMSQ_PARTS] <- squared-norm partials of the concatenation of flat[lo:hi] for (lo, hi) in ranges (<= 8, multiples of 4)."""
    n, b, e = _range_arrays(ranges)
    check(lib().halo_sumsq_ranges(ptr(flat), n, b, e, ptr(partials), _stream()), 'halo_sumsq_ranges')
    return partials


def pack_ranges_bf16(flat, ranges, dst):
    """dst (bfloat16, contiguous) <- the concatenation of flat[lo:hi] for (lo, hi) in ranges, rounded to nearest-even."""
    n, b, e = _range_arrays(ranges)
    check(lib().halo_pack_ranges_bf16(ptr(flat), n, b, e, ptr(dst), _stream()), 'halo_pack_ranges_bf16')
    return dst


def expand_ranges_bf16(stage, spans, chunks, world, skip_rank, flat):
    """flat[span k] <- the gathered bf16 records of every rank but skip_rank (include/halo.h halo_expand_ranges_bf16)."""
    n = len(spans)
    b = (C.c_size_t * n)(*[int(s) for s in spans])
    c = (C.c_size_t * n)(*[int(x) for x in chunks])
    check(lib().halo_expand_ranges_bf16(ptr(stage), n, b, c, int(world), int(skip_rank), ptr(flat), _stream()), 'halo_expand_ranges_bf16')
    return flat


GRAD_SUMSQ_ALL = 31        # halo_grad_sumsq_state: both layers' matrices and biases and the conv front end have contributed


def collect_grad_sumsq(partials):
    """The backward launches that follow write the squared-norm partials of the clipped gradients they store into ``partials`` (float32;
    None: off) -- see ``grad_sumsq_state``."""
    check(lib().halo_set_grad_sumsq(ptr(partials), 0 if partials is None else partials.numel()), 'halo_set_grad_sumsq')


def grad_sumsq_state():
    """(slots written, producer bits) since ``collect_grad_sumsq``: the partials are the whole clipped norm when bits == GRAD_SUMSQ_ALL
    and the clipped parameters are the conv front end + a 2-layer LSTM."""
    n, bits = C.c_int(0), C.c_uint(0)
    check(lib().halo_grad_sumsq_state(C.byref(n), C.byref(bits)), 'halo_grad_sumsq_state')
    return int(n.value), int(bits.value)


def clip_coef(partials, count, max_norm, coef, norm, applied_steps=None):
    """applied_steps: optional device 32-bit counter advanced when the norm is finite (the Adam step count of applied updates)."""
    check(lib().halo_clip_coef_step(ptr(partials), count, float(max_norm), ptr(coef), ptr(norm), ptr(applied_steps), _stream()),
          'halo_clip_coef_step')


def adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=None):
    """In-place AdamW on flat views.  Pass views that share the parameter's version counter (``param.detach().view(-1)``,
    not ``param.data``): the update bumps it so that cached operand images of the weight (haloop_amd/_linear.py) are rebuilt."""
    _lib.bump_weights_epoch()
    check(lib().halo_adamw(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step,
                           ptr(grad_scale), _stream()), 'halo_adamw')
    torch.autograd.graph.increment_version(p)


def adamw_ranges(p, g, m, v, ranges, lr, beta1, beta2, eps, step, counter=None):
    """One-launch AdamW over ``ranges`` = [(begin, end, weight_decay, grad_scale tensor or None), ...] of flat buffers.
    ``step``: the 1-based update count as a python int, or a device int32 tensor holding it (no host scalar: graph-capturable).
    ``lr``: a python float, or (with a device ``step``) a one-element float32 device tensor the launch reads it from."""
    _lib.bump_weights_epoch()
    n = len(ranges)
    begin = (C.c_size_t * n)(*[r[0] for r in ranges])
    end = (C.c_size_t * n)(*[r[1] for r in ranges])
    wd = (C.c_float * n)(*[float(r[2]) for r in ranges])
    gs = (C.c_void_p * n)(*[ptr(r[3]) for r in ranges])
    if torch.is_tensor(step):
        lr_dev = lr if torch.is_tensor(lr) else None
        check(lib().halo_adamw_ranges_dev(ptr(p), ptr(g), ptr(m), ptr(v), n, begin, end, wd, gs, 0.0 if lr_dev is not None else lr,
                                          ptr(lr_dev), beta1, beta2, eps, ptr(step), ptr(counter), _stream()), 'halo_adamw_ranges_dev')
    else:
        check(lib().halo_adamw_ranges(ptr(p), ptr(g), ptr(m), ptr(v), n, begin, end, wd, gs, lr, beta1, beta2, eps, step, ptr(counter),
                                      _stream()), 'halo_adamw_ranges')
    torch.autograd.graph.increment_version(p)


class AdamWMulti:
    """torch.optim.AdamW arithmetic over a whole parameter list in ONE launch per 256 tensors (the reference's fused AdamW,
    ha/attention_loop.py:141-147).  ``params``: the nn.Parameters (contiguous fp32 on the HIP device); ``weight_decays``: one value
    per parameter.  The optimizer state lives here; ``step()`` reads each parameter's current ``.grad``."""

    def __init__(self, params, weight_decays, lr, betas=(0.9, 0.999), eps=1e-8):
        import numpy as np
        self.params = list(params)
        self.wds = [float(w) for w in weight_decays]
        self.param_groups = [{'lr': float(lr), 'params': self.params}]
        self.betas, self.eps = betas, float(eps)
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.is_cuda:
                raise ValueError('AdamWMulti: parameters must be contiguous float32 tensors on the HIP device')
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0
        dev = self.params[0].device
        chunk, group = lib().halo_adamw_multi_chunk(), lib().halo_adamw_multi_max_tensors()
        assert lib().halo_adamw_multi_tensor_bytes() == 40
        rec = np.dtype([('p', '<u8'), ('m', '<u8'), ('v', '<u8'), ('n', '<u8'), ('decay', '<f4'), ('pad', '<i4')])
        self.groups = []                                        # (first parameter, count, device tensor table, device chunk table, chunks)
        for first in range(0, len(self.params), group):
            idx = range(first, min(first + group, len(self.params)))
            table = np.zeros(len(idx), dtype=rec)
            for k, i in enumerate(idx):
                p = self.params[i]
                table[k] = (p.data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), p.numel(), self.wds[i], 0)
            pairs = [(k, c) for k, i in enumerate(idx) for c in range((self.params[i].numel() + chunk - 1) // chunk)]
            self.groups.append((first, len(idx), torch.from_numpy(table.view(np.uint8)).to(dev),
                                torch.tensor(pairs, dtype=torch.int32).view(-1).to(dev), len(pairs)))

    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = float(value)

    def step(self, grad_scale=None):
        _lib.bump_weights_epoch()
        self.t += 1
        for first, count, table, chunks, n_chunks in self.groups:
            ptrs = (C.c_void_p * count)()
            for k in range(count):
                p = self.params[first + k]
                g = p.grad
                if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.shape != p.shape:
                    raise ValueError('AdamWMulti.step: every parameter needs a contiguous float32 .grad of its shape on its device')
                ptrs[k] = g.data_ptr()
            check(lib().halo_adamw_multi(ptr(table), ptr(chunks), n_chunks, ptrs, count, self.lr, self.betas[0], self.betas[1], self.eps,
                                         self.t, ptr(grad_scale), _stream()), 'halo_adamw_multi')
        for p in self.params:
            torch.autograd.graph.increment_version(p)          # cached operand images of the weights are rebuilt


def scale_add_(y, x, alpha, beta, guard=None):
    """y <- alpha*y + beta*x in place (flat fp32 buffers); alpha == 0 never reads y.  guard: optional device scalar; when it is not
    finite, x contributes nothing (a micro-batch with a NaN/Inf loss is dropped, ha/loop.py:167-174)."""
    check(lib().halo_scale_add_guarded(ptr(y), ptr(x), float(alpha), float(beta), y.numel(), ptr(guard), _stream()),
          'halo_scale_add_guarded')
    return y


def cast_f32_to_bf16_(dst_bf16, src_f32):
    check(lib().halo_cast_f32_bf16(ptr(src_f32), ptr(dst_bf16), src_f32.numel(), _stream()), 'halo_cast_f32_bf16')
    return dst_bf16


def cast_bf16_to_f32_(dst_f32, src_bf16, scale=1.0):
    check(lib().halo_cast_bf16_f32(ptr(src_bf16), ptr(dst_f32), float(scale), dst_f32.numel(), _stream()), 'halo_cast_bf16_f32')
    return dst_f32


def counter_inc(counter):
    check(lib().halo_counter_inc(ptr(counter), _stream()), 'halo_counter_inc')


# ---- GPT forward operators ------------------------------------------------------------------------
def embed_fwd(ids, wte, wpe, pos0=0):
    ids = _i64c(ids, 'input_ids')
    Bn, T = ids.shape
    C = wte.shape[1]
    x = torch.empty(Bn * T, C, device=wte.device, dtype=torch.float32)
    check(lib().halo_embed_fwd(ptr(ids), ptr(wte), ptr(wpe), ptr(x), Bn * T, T, C, pos0, wte.shape[0], _stream()), 'halo_embed_fwd')
    return x


def layernorm_fwd(x2d, weight, bias=None, eps=1e-5):
    _f32c(x2d, 'x')
    y = torch.empty_like(x2d)
    check(lib().halo_layernorm_fwd(ptr(x2d), ptr(weight), ptr(bias), ptr(y), x2d.shape[0], x2d.shape[1], eps, _stream()),
          'halo_layernorm_fwd')
    return y


def attention_causal_fwd(qkv2d, B, T, n_head):
    _f32c(qkv2d, 'qkv')
    C = qkv2d.shape[1] // 3
    y = torch.empty(B * T, C, device=qkv2d.device, dtype=torch.float32)
    check(lib().halo_attention_causal_fwd(ptr(qkv2d), ptr(y), B, T, n_head, C, _stream()), 'halo_attention_causal_fwd')
    return y


def cross_entropy_fwd(logits2d, targets, ignore_index=0):
    _f32c(logits2d, 'logits')
    tg = _i64c(targets.reshape(-1), 'targets')
    loss = torch.empty(logits2d.shape[0], device=logits2d.device, dtype=torch.float32)
    check(lib().halo_cross_entropy_fwd(ptr(logits2d), ptr(tg), ptr(loss), logits2d.shape[0], logits2d.shape[1],
                                       logits2d.shape[1], ignore_index, _stream()), 'halo_cross_entropy_fwd')
    return loss


# ---- attention / rotary / KV-cache operators (GPT and the enc-dec ASR path) ------------------------------
def attention_fwd(q, k, v, N, heads, head_dim, Tq, Tk, causal=False, key_lengths=None, want_lse=False, want_entropy=False,
                  drop=NO_DROPOUT, stream_id=0):
    """q: rows [N*Tq, >=C] (a column slice of a packed GEMM output is fine), k/v: rows [N*Tk, ...] sharing one row stride.
    -> y [N*Tq, C] (+ lse / entropy [N, heads, Tq] when asked).  ``drop``: dropout on the attention probabilities."""
    C = heads * head_dim
    for t in (q, k, v):
        if t.dtype != torch.float32 or not t.is_cuda or t.stride(-1) != 1:
            raise ValueError('attention operands must be float32 HIP tensors with a unit column stride')
    if k.stride(0) != v.stride(0):
        raise ValueError('k and v must share a row stride')
    dev = q.device
    y = torch.empty(N * Tq, C, device=dev, dtype=torch.float32)
    lse = torch.empty(N, heads, Tq, device=dev, dtype=torch.float32) if want_lse else None
    ent = torch.empty(N, heads, Tq, device=dev, dtype=torch.float32) if want_entropy else None
    if key_lengths is not None:
        key_lengths = key_lengths.to(device=dev, dtype=torch.int32).contiguous()
    check(lib().halo_attention_fwd_strided(ptr(q), q.stride(0), q.stride(0) * Tq, head_dim, ptr(k), ptr(v), k.stride(0),
                                           k.stride(0) * Tk, head_dim, ptr(y), C, C * Tq, ptr(lse), ptr(ent), N, heads, head_dim, Tq, Tk,
                                           int(causal), ptr(key_lengths), drop.p, drop.seed, stream_id, drop.offset, drop.counter_ptr,
                                           _stream()), 'halo_attention_fwd')
    return y, lse, ent


class RopeTable:
    """cos/sin tables of rotate_interleaved (ha/transformer.py:16-31) for positions [0, T)."""

    def __init__(self, T, head_dim, device, base=10000.0):
        self.T, self.head_dim = T, head_dim
        self.cos = torch.empty(T, head_dim // 2, device=device, dtype=torch.float32)
        self.sin = torch.empty(T, head_dim // 2, device=device, dtype=torch.float32)
        check(lib().halo_rope_table(ptr(self.cos), ptr(self.sin), T, head_dim, float(base), _stream()), 'halo_rope_table')


def rope_(x2d, T, heads, head_dim, table, t0=0, inverse=False):
    """Rotate in place the heads*head_dim leading columns of the rows of x2d (row r is at position t0 + r % T)."""
    if x2d.dtype != torch.float32 or not x2d.is_cuda or x2d.stride(-1) != 1:
        raise ValueError('rope: expected a float32 HIP tensor with a unit column stride')
    check(lib().halo_rope_interleaved(ptr(x2d), x2d.stride(0), x2d.shape[0], T, heads, head_dim, t0, ptr(table.cos), ptr(table.sin),
                                      table.T, int(inverse), _stream()), 'halo_rope_interleaved')
    return x2d


def rope_rows_(rows, T, heads, head_dim, table, t0=0, inverse=False):
    """Rotate in place, in ONE launch, the q and the k column blocks of packed q | k | v rows [M, >= 2 * heads * head_dim] (fp32 or bf16;
    a column slice of a wider buffer is fine): row r is at position t0 + r % T, v is never touched; ``inverse`` applies the transpose
    (the backward, on dq | dk).  16-byte accesses only: head_dim % 8 == 0, aligned rows and row stride, else the library's argument error."""
    if rows.dtype not in (torch.float32, torch.bfloat16) or not rows.is_cuda or rows.dim() != 2 or rows.stride(-1) != 1:
        raise ValueError('rope_rows: expected float32 or bfloat16 HIP rows with a unit column stride')
    if rows.shape[1] < 2 * heads * head_dim:
        raise ValueError('rope_rows: the rows are narrower than the q and k column blocks')
    check(lib().halo_rope_rows(ptr(rows), int(rows.dtype == torch.bfloat16), rows.stride(0), rows.shape[0], T, heads, head_dim, t0,
                               ptr(table.cos), ptr(table.sin), table.T, int(inverse), _stream()), 'halo_rope_rows')
    return rows


def attention_cached_fwd(q, cache_k, cache_v, Tq, n_keys, causal=True):
    """q: rows [N*Tq, C] (a column slice is fine); cache_{k,v}: [N, heads, Tc, head_dim] fp32 holding n_keys valid keys.
    -> y [N*Tq, C]: attend_cached of ha/attention.py:64-93 (queries are the LAST Tq of the n_keys positions)."""
    N, heads, Tc, hd = cache_k.shape
    C = heads * hd
    y = torch.empty(N * Tq, C, device=q.device, dtype=torch.float32)
    check(lib().halo_attention_fwd_strided(ptr(q), q.stride(0), q.stride(0) * Tq, hd, ptr(cache_k), ptr(cache_v), hd, heads * Tc * hd,
                                           Tc * hd, ptr(y), C, C * Tq, None, None, N, heads, hd, Tq, n_keys, int(causal), None,
                                           0.0, 0, 0, 0, None, _stream()), 'halo_attention_fwd_strided')
    return y


def kv_cache_store(src2d, v_offset, cache_k, cache_v, N, S, heads, head_dim, t0):
    """cache_{k,v} [N, heads, Tc, head_dim] float16 (or float32) <- rows [N*S] of src2d (k at column 0, v at column v_offset)."""
    if cache_k.dtype == torch.float32:
        check(lib().halo_kv_cache_store_f32(ptr(src2d), src2d.stride(0), v_offset, ptr(cache_k), ptr(cache_v), N, S, heads, head_dim,
                                            cache_k.shape[2], t0, _stream()), 'halo_kv_cache_store_f32')
        return
    check(lib().halo_kv_cache_store(ptr(src2d), src2d.stride(0), v_offset, ptr(cache_k), ptr(cache_v), N, S, heads, head_dim,
                                    cache_k.shape[2], t0, _stream()), 'halo_kv_cache_store')


def attention_decode(q2d, cache_k, cache_v, n_keys, key_lengths=None, table=None, out=None):
    N, heads, Tc, hd = cache_k.shape
    if out is None:
        out = torch.empty(N, heads * hd, device=q2d.device, dtype=torch.float32)
    check(lib().halo_attention_decode(ptr(q2d), q2d.stride(0), ptr(cache_k), ptr(cache_v), ptr(out), out.stride(0), N, heads, hd, Tc,
                                      n_keys, ptr(key_lengths), ptr(table.cos) if table else None, ptr(table.sin) if table else None,
                                      _stream()), 'halo_attention_decode')
    return out


def attention_decode_step(q2d, k2d, v2d, cache_k, cache_v, n_keys, table=None):
    """Self-attention of one decode step in one launch: stores k2d / v2d (fp16) at cache position n_keys - 1, rotates q and the
    cached keys (table), attends over n_keys positions.  q2d / k2d / v2d: column slices of one packed row buffer."""
    N, heads, Tc, hd = cache_k.shape
    if not (q2d.stride(0) == k2d.stride(0) == v2d.stride(0)):
        raise ValueError('q, k, v must share a row stride')
    out = torch.empty(N, heads * hd, device=q2d.device, dtype=torch.float32)
    check(lib().halo_attention_decode_step(ptr(q2d), ptr(k2d), ptr(v2d), q2d.stride(0), ptr(cache_k), ptr(cache_v), ptr(out),
                                           out.stride(0), N, heads, hd, Tc, n_keys, ptr(table.cos) if table else None,
                                           ptr(table.sin) if table else None, _stream()), 'halo_attention_decode_step')
    return out


def logprob_max(logits2d, want_entropy=False):
    _f32c(logits2d, 'logits')
    rows, V = logits2d.shape
    dev = logits2d.device
    val = torch.empty(rows, device=dev, dtype=torch.float32)
    idx = torch.empty(rows, device=dev, dtype=torch.int64)
    ne = torch.empty(rows, device=dev, dtype=torch.float32) if want_entropy else None
    check(lib().halo_logprob_max(ptr(logits2d), V, rows, V, ptr(val), ptr(idx), ptr(ne), _stream()), 'halo_logprob_max')
    return val, idx, ne


def greedy_update(val, idx, negent, tokens, t, plen, etx, alive, out_len, log_probs, sum_ent):
    check(lib().halo_greedy_update(ptr(val), ptr(idx), ptr(negent), ptr(tokens), tokens.stride(0), t, plen, etx, ptr(alive),
                                   ptr(out_len), ptr(log_probs), ptr(sum_ent), tokens.shape[0], _stream()), 'halo_greedy_update')


# ---- star-CTC and transducer lattices (csrc/lattice.hip) -------------------------------------------------------
def _check_lengths(name, lengths, hi):
    if lengths.numel() and (int(lengths.min()) < 0 or int(lengths.max()) > hi):
        raise ValueError(f'{name} out of range [0, {hi}]')


def star_ctc_fwd(em, targets, emission_lengths, target_lengths, star_penalty, keep=False):
    """em [T, N, C] fp32 log-probabilities (unit column stride) -> (losses [N], workspace or None)."""
    T, N, C = em.shape
    S = targets.shape[1]
    if targets.shape[0] != N or S < 1 or C < 2:
        raise ValueError('star_ctc: targets must be [N, S >= 1] and C >= 2')
    if targets.numel() and (int(targets.min()) < 0 or int(targets.max()) >= C):
        raise ValueError('star_ctc: target label out of range')
    if emission_lengths.numel() and int(emission_lengths.min()) < 1:
        raise ValueError('star_ctc: emission_lengths must be >= 1')
    _check_lengths('star_ctc: emission_lengths', emission_lengths, T)
    _check_lengths('star_ctc: target_lengths', target_lengths, S)
    losses = torch.empty(N, device=em.device, dtype=torch.float32)
    ws = torch.empty(lib().halo_star_ctc_workspace_bytes(T, N, S), device=em.device, dtype=torch.uint8) if keep else None
    check(lib().halo_star_ctc_fwd(ptr(em), em.stride(0), em.stride(1), T, N, C, ptr(targets), S, ptr(emission_lengths), ptr(target_lengths),
                                  star_penalty, ptr(ws), ptr(losses), _stream()), 'halo_star_ctc_fwd')
    return losses, ws


def star_ctc_bwd(em, targets, emission_lengths, target_lengths, star_penalty, workspace, losses, grad_losses):
    T, N, C = em.shape
    if workspace is None:
        raise ValueError('star_ctc backward: the forward did not keep its lattice')
    grad = torch.empty_like(em)
    check(lib().halo_star_ctc_bwd(ptr(em), em.stride(0), em.stride(1), T, N, C, ptr(targets), targets.shape[1], ptr(emission_lengths),
                                  ptr(target_lengths), star_penalty, ptr(workspace), ptr(losses), ptr(grad_losses), ptr(grad), _stream()),
          'halo_star_ctc_bwd')
    return grad


def _check_transducer(name, K, T, U1, targets, joint_lengths, target_lengths, min_length=1):
    if targets.numel() and (int(targets.min()) < 0 or int(targets.max()) >= K):
        raise ValueError(f'{name}: target label out of range')
    if joint_lengths.numel() and int(joint_lengths.min()) < min_length:
        raise ValueError(f'{name}: joint_lengths must be >= {min_length}')
    _check_lengths(f'{name}: joint_lengths', joint_lengths, T)
    _check_lengths(f'{name}: target_lengths', target_lengths, U1 - 1)


def transducer_fwd(joint, targets, joint_lengths, target_lengths, keep=False, checked=False):
    """joint [N, T, U+1, K] fp32 contiguous log-probabilities -> (losses [N], workspace or None).  ``checked``: the caller has validated
    the labels and lengths already (rnnt_joint_fwd's caller: the same lengths, targets of ones)."""
    N, T, U1, K = joint.shape
    if not checked:
        _check_transducer('transducer', K, T, U1, targets, joint_lengths, target_lengths)
    losses = torch.empty(N, device=joint.device, dtype=torch.float32)
    ws = torch.empty(lib().halo_transducer_workspace_bytes(N, T, U1), device=joint.device, dtype=torch.uint8) if keep else None
    check(lib().halo_transducer_fwd(ptr(joint), N, T, U1, K, ptr(targets), ptr(joint_lengths), ptr(target_lengths), ptr(ws), ptr(losses),
                                    _stream()), 'halo_transducer_fwd')
    return losses, ws


def transducer_bwd(joint, targets, joint_lengths, target_lengths, workspace, losses, grad_losses):
    N, T, U1, K = joint.shape
    if workspace is None:
        raise ValueError('transducer backward: the forward did not keep its lattice')
    grad = torch.empty_like(joint)
    check(lib().halo_transducer_bwd(ptr(joint), N, T, U1, K, ptr(targets), ptr(joint_lengths), ptr(target_lengths), ptr(workspace),
                                    ptr(losses), ptr(grad_losses), ptr(grad), _stream()), 'halo_transducer_bwd')
    return grad


# ---- the transducer loss over the additive joint f[:, :, None] + g[:, None] (csrc/rnnt_loss.hip): nothing of N T (U+1) V elements ----
def _check_rnnt_joint(f, g, targets):
    if f.dim() != 3 or g.dim() != 3 or f.shape[0] != g.shape[0] or f.shape[2] != g.shape[2]:
        raise ValueError(f'rnnt_joint: f must be [N, T, V] and g [N, U+1, V], got {tuple(f.shape)} and {tuple(g.shape)}')
    N, T, V = f.shape
    U1 = g.shape[1]
    if tuple(targets.shape) != (N, U1 - 1):
        raise ValueError(f'rnnt_joint: targets must be [N, U] = [{N}, {U1 - 1}], got {tuple(targets.shape)}')
    if f.dtype != torch.float32 or g.dtype != torch.float32 or (V > 1 and (f.stride(2) != 1 or g.stride(2) != 1)):
        raise ValueError('rnnt_joint: f and g must be fp32 with unit stride along V')
    return N, T, U1, V


def rnnt_joint_fwd(f, g, targets, f_lengths, target_lengths, min_length=1):
    """f [N, T, V], g [N, U+1, V] fp32 logits (row strides; unit stride along V), targets [N, U] int64, lengths [N] int32 ->
    (lse [N, T, U+1], lp2 [N, T, U+1, 2]): the log-sum-exp of every cell of the additive joint and its blank / label log-probabilities.
    ``min_length``: the smallest f_lengths entry accepted (the loss needs a frame; the aligner takes empty rows)."""
    N, T, U1, V = _check_rnnt_joint(f, g, targets)
    _check_transducer('rnnt_joint', V, T, U1, targets, f_lengths, target_lengths, min_length)
    lse = torch.empty(N, T, U1, device=f.device, dtype=torch.float32)
    lp2 = torch.empty(N, T, U1, 2, device=f.device, dtype=torch.float32)
    check(lib().halo_rnnt_joint_fwd(ptr(f), f.stride(0), f.stride(1), ptr(g), g.stride(0), g.stride(1), N, T, U1, V, ptr(targets),
                                    ptr(f_lengths), ptr(target_lengths), ptr(lse), ptr(lp2), _stream()), 'halo_rnnt_joint_fwd')
    return lse, lp2


def rnnt_joint_bwd(f, g, targets, f_lengths, target_lengths, lse, grad_lp2):
    """grad_lp2 [N, T, U+1, 2] (transducer_bwd on lp2) -> (df [N, T, V] contiguous, dg [N, U+1, V] in g's layout where that is dense)."""
    N, T, U1, V = _check_rnnt_joint(f, g, targets)
    if tuple(lse.shape) != (N, T, U1) or tuple(grad_lp2.shape) != (N, T, U1, 2) or not lse.is_contiguous() or not grad_lp2.is_contiguous():
        raise ValueError('rnnt_joint backward: lse must be [N, T, U+1] and grad_lp2 [N, T, U+1, 2], contiguous')
    df = torch.empty(N, T, V, device=f.device, dtype=torch.float32)
    dg = torch.empty_like(g)                      # keeps the strides of a dense g (a transposed view of time-major rows), else contiguous
    if V > 1 and dg.stride(2) != 1:
        dg = torch.empty(N, U1, V, device=f.device, dtype=torch.float32)
    check(lib().halo_rnnt_joint_bwd(ptr(f), f.stride(0), f.stride(1), ptr(g), g.stride(0), g.stride(1), N, T, U1, V, ptr(targets),
                                    ptr(f_lengths), ptr(target_lengths), ptr(lse), ptr(grad_lp2), ptr(df), df.stride(0), df.stride(1),
                                    ptr(dg), dg.stride(0), dg.stride(1), _stream()), 'halo_rnnt_joint_bwd')
    return df, dg


# ---- forced alignment: best paths of the two lattices and their backtraces (csrc/viterbi.hip) ---------------------------------------
def ctc_viterbi(lp, time_major, targets, input_lengths, target_lengths):
    """lp: [T,N,C] (time_major) or [N,T,C] fp32 log-probabilities, any strides with a unit class stride; targets [N,S] (S >= 1) ->
    (scores [N] f32, alignments [N,T] int64, starts [N,S] int32, ends [N,S] int32) of F.ctc_loss's lattice (include/halo.h)."""
    if lp.dtype != torch.float32 or lp.dim() != 3 or lp.stride(-1) != 1 or not lp.is_cuda:
        raise ValueError('ctc_viterbi: log-probs must be a float32 HIP tensor of three dimensions with unit class stride')
    if time_major:
        T, N, Cn = lp.shape
        st, sn = lp.stride(0), lp.stride(1)
    else:
        N, T, Cn = lp.shape
        sn, st = lp.stride(0), lp.stride(1)
    targets = _i64c(targets, 'targets')
    if targets.dim() != 2 or targets.shape[0] != N or targets.shape[1] < 1:
        raise ValueError(f'ctc_viterbi: targets must be [N, S >= 1] (padded) with N = {N}, got {tuple(targets.shape)}')
    S = targets.shape[1]
    tl = _i64c(target_lengths, 'target_lengths')
    il = None if input_lengths is None else _i64c(input_lengths, 'input_lengths')
    if tl.shape != (N,) or (il is not None and il.shape != (N,)):
        raise ValueError(f'ctc_viterbi: lengths must be [{N}]')
    dev = lp.device
    ws = torch.empty(lib().halo_ctc_viterbi_workspace_bytes(T, N, S), device=dev, dtype=torch.uint8)
    scores = torch.empty(N, device=dev, dtype=torch.float32)
    ali = torch.empty(N, T, device=dev, dtype=torch.int64)
    starts = torch.empty(N, S, device=dev, dtype=torch.int32)
    ends = torch.empty(N, S, device=dev, dtype=torch.int32)
    check(lib().halo_ctc_viterbi(ptr(lp), st, sn, T, N, Cn, ptr(targets), targets.stride(0), S, ptr(il), ptr(tl), ptr(ws), ptr(scores),
                                 ptr(ali), ptr(starts), ptr(ends), _stream()), 'halo_ctc_viterbi')
    return scores, ali, starts, ends


def transducer_viterbi(joint, targets, joint_lengths, target_lengths, checked=False):
    """joint [N, T, U+1, K] fp32 contiguous log-probabilities, targets [N, U] int64, lengths [N] int32 (a joint length of 0 is an empty
    row) -> (scores [N] f32, frames [N, U] int32).  ``checked``: as ``transducer_fwd``."""
    _f32c(joint, 'joint')
    N, T, U1, K = joint.shape
    if not checked:
        _check_transducer('transducer_viterbi', K, T, U1, targets, joint_lengths, target_lengths, 0)
    ws = torch.empty(lib().halo_transducer_viterbi_workspace_bytes(N, T, U1), device=joint.device, dtype=torch.uint8)
    scores = torch.empty(N, device=joint.device, dtype=torch.float32)
    frames = torch.empty(N, U1 - 1, device=joint.device, dtype=torch.int32)
    check(lib().halo_transducer_viterbi(ptr(joint), N, T, U1, K, ptr(targets), ptr(joint_lengths), ptr(target_lengths), ptr(ws), ptr(scores),
                                        ptr(frames), _stream()), 'halo_transducer_viterbi')
    return scores, frames


# ---- CTC prefix beam search: n-best lists from CTC emissions in one launch (csrc/ctc_prefix_beam.hip) ---------------------------------
BEAM_MAX = 16                    # widths the beam searches take (csrc/beam_common.h BEAM_MAX)


def ctc_prefix_beam(emissions, emission_lengths, beam, capacity):
    """emissions [T, N, V] fp32 log-probabilities, any time and batch strides with a unit class stride; emission_lengths [N] int64 or
    None (T) -> (tokens [N, beam, capacity] int64, lengths [N, beam] int64, scores [N, beam] f32, counts [N] int64) (include/halo.h)."""
    if emissions.dtype != torch.float32 or emissions.dim() != 3 or emissions.stride(-1) != 1 or not emissions.is_cuda:
        raise ValueError('ctc_prefix_beam: emissions must be a float32 HIP tensor of three dimensions with unit class stride')
    T, N, V = emissions.shape
    il = None if emission_lengths is None else _i64c(emission_lengths, 'emission_lengths')
    if il is not None and il.shape != (N,):
        raise ValueError(f'ctc_prefix_beam: emission_lengths must be [{N}]')
    dev = emissions.device
    tokens = torch.empty(N, beam, capacity, device=dev, dtype=torch.int64)
    lengths = torch.empty(N, beam, device=dev, dtype=torch.int64)
    scores = torch.empty(N, beam, device=dev, dtype=torch.float32)
    counts = torch.empty(N, device=dev, dtype=torch.int64)
    nbytes = lib().halo_ctc_prefix_beam_workspace_bytes(N, T, V, beam, capacity)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib().halo_ctc_prefix_beam(ptr(emissions), emissions.stride(0), emissions.stride(1), T, N, V, ptr(il), beam, capacity, ptr(ws),
                                     ptr(tokens), ptr(lengths), ptr(scores), ptr(counts), _stream()), 'halo_ctc_prefix_beam')
    return tokens, lengths, scores, counts


PREFIX_BEAM_MAX_CAPACITY = 8192  # HALO_CTC_PREFIX_BEAM_MAX_CAPACITY (include/halo.h)


def ctc_prefix_beam_state_bytes(V, beam, capacity):
    """Bytes of one row of the carried search's state; 0 for a shape the search does not take (include/halo.h)."""
    return int(lib().halo_ctc_prefix_beam_state_bytes(V, beam, capacity))


def ctc_prefix_beam_advance(emissions, n_frames, flags, beam, capacity, state, tokens, lengths, scores, counts):
    """The carried CTC prefix beam search over one more chunk (include/halo.h: halo_ctc_prefix_beam_advance).  emissions [T, N, V] fp32
    log-probabilities, any time and batch strides with a unit class stride; n_frames [N] int32 or None (T); flags [N] int32 (the
    streaming flag bits, only STREAM_BEGIN is read) or None; state [N, ctc_prefix_beam_state_bytes(V, beam, capacity)] uint8.  The rows
    that take part have their rows of state, tokens [N, beam, capacity] int64, lengths [N, beam] int64, scores [N, beam] f32 and counts
    [N] int64 written in place.  Every tensor is the caller's: nothing is allocated."""
    if emissions.dtype != torch.float32 or emissions.dim() != 3 or emissions.stride(-1) != 1 or not emissions.is_cuda:
        raise ValueError('ctc_prefix_beam_advance: emissions must be a float32 HIP tensor of three dimensions with unit class stride')
    T, N, V = emissions.shape
    nbytes = ctc_prefix_beam_state_bytes(V, beam, capacity)
    if nbytes == 0:
        raise ValueError(f'ctc_prefix_beam_advance: V {V}, beam {beam}, capacity {capacity} outside what the search takes')
    for t, dt, name in ((n_frames, torch.int32, 'n_frames'), (flags, torch.int32, 'flags')):
        if t is not None and (t.dtype != dt or t.shape != (N,) or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f'ctc_prefix_beam_advance: {name} must be a contiguous {dt} HIP tensor [{N}]')
    for t, dt, shape, name in ((state, torch.uint8, (N, nbytes), 'state'), (tokens, torch.int64, (N, beam, capacity), 'tokens'),
                               (lengths, torch.int64, (N, beam), 'lengths'), (scores, torch.float32, (N, beam), 'scores'),
                               (counts, torch.int64, (N,), 'counts')):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'ctc_prefix_beam_advance: {name} must be a contiguous {dt} HIP tensor {list(shape)}')
    check(lib().halo_ctc_prefix_beam_advance(ptr(emissions), emissions.stride(0), emissions.stride(1), T, N, V, ptr(n_frames), ptr(flags),
                                             beam, capacity, ptr(state), ptr(tokens), ptr(lengths), ptr(scores), ptr(counts), _stream()),
          'halo_ctc_prefix_beam_advance')


def _context_tables(context, V, name):
    """(columns [V] int32, next [S, A + 1] int32, gain [S, A + 1] f32) of a phrase automaton on the device (include/halo.h)."""
    columns, nxt, gain = context
    for t, dt, what in ((columns, torch.int32, 'columns'), (nxt, torch.int32, 'next'), (gain, torch.float32, 'gain')):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'{name}: the context\'s {what} must be a contiguous {dt} HIP tensor')
    if columns.shape != (V,) or nxt.dim() != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1 or gain.shape != nxt.shape:
        raise ValueError(f'{name}: the context\'s tables must be columns [{V}] and next, gain [states, columns + 1]')
    return columns, nxt, gain


def ctc_prefix_beam_biased(emissions, emission_lengths, beam, capacity, context):
    """``ctc_prefix_beam`` with a phrase automaton inside the launch (include/halo.h: halo_ctc_prefix_beam_biased): context = (columns,
    next, gain) on the device -> (tokens, lengths, scores = CTC mass + boost, counts, boosts [N, beam] f32, states [N, beam] int64)."""
    if emissions.dtype != torch.float32 or emissions.dim() != 3 or emissions.stride(-1) != 1 or not emissions.is_cuda:
        raise ValueError('ctc_prefix_beam_biased: emissions must be a float32 HIP tensor of three dimensions with unit class stride')
    T, N, V = emissions.shape
    il = None if emission_lengths is None else _i64c(emission_lengths, 'emission_lengths')
    if il is not None and il.shape != (N,):
        raise ValueError(f'ctc_prefix_beam_biased: emission_lengths must be [{N}]')
    columns, nxt, gain = _context_tables(context, V, 'ctc_prefix_beam_biased')
    dev = emissions.device
    tokens = torch.empty(N, beam, capacity, device=dev, dtype=torch.int64)
    lengths = torch.empty(N, beam, device=dev, dtype=torch.int64)
    scores = torch.empty(N, beam, device=dev, dtype=torch.float32)
    counts = torch.empty(N, device=dev, dtype=torch.int64)
    boosts = torch.empty(N, beam, device=dev, dtype=torch.float32)
    states = torch.empty(N, beam, device=dev, dtype=torch.int64)
    nbytes = lib().halo_ctc_prefix_beam_workspace_bytes(N, T, V, beam, capacity)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib().halo_ctc_prefix_beam_biased(ptr(emissions), emissions.stride(0), emissions.stride(1), T, N, V, ptr(il), beam, capacity,
                                            ptr(ws), ptr(tokens), ptr(lengths), ptr(scores), ptr(counts), ptr(columns), ptr(nxt), ptr(gain),
                                            nxt.shape[0], nxt.shape[1], ptr(boosts), ptr(states), _stream()), 'halo_ctc_prefix_beam_biased')
    return tokens, lengths, scores, counts, boosts, states


def ctc_prefix_beam_biased_state_bytes(V, beam, capacity):
    """Bytes of one row of the biased carried search's state; 0 for a shape the search does not take (include/halo.h)."""
    return int(lib().halo_ctc_prefix_beam_biased_state_bytes(V, beam, capacity))


def ctc_prefix_beam_advance_biased(emissions, n_frames, flags, beam, capacity, state, tokens, lengths, scores, counts, context, boosts,
                                   states):
    """``ctc_prefix_beam_advance`` with a phrase automaton inside the launch (include/halo.h: halo_ctc_prefix_beam_advance_biased):
    state [N, ctc_prefix_beam_biased_state_bytes(V, beam, capacity)] uint8, context = (columns, next, gain) on the device, boosts
    [N, beam] f32 and states [N, beam] int64 written in place with the other four.  Nothing is allocated."""
    if emissions.dtype != torch.float32 or emissions.dim() != 3 or emissions.stride(-1) != 1 or not emissions.is_cuda:
        raise ValueError('ctc_prefix_beam_advance_biased: emissions must be a float32 HIP tensor of three dimensions with unit class stride')
    T, N, V = emissions.shape
    nbytes = ctc_prefix_beam_biased_state_bytes(V, beam, capacity)
    if nbytes == 0:
        raise ValueError(f'ctc_prefix_beam_advance_biased: V {V}, beam {beam}, capacity {capacity} outside what the search takes')
    columns, nxt, gain = _context_tables(context, V, 'ctc_prefix_beam_advance_biased')
    for t, dt, name in ((n_frames, torch.int32, 'n_frames'), (flags, torch.int32, 'flags')):
        if t is not None and (t.dtype != dt or t.shape != (N,) or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f'ctc_prefix_beam_advance_biased: {name} must be a contiguous {dt} HIP tensor [{N}]')
    for t, dt, shape, name in ((state, torch.uint8, (N, nbytes), 'state'), (tokens, torch.int64, (N, beam, capacity), 'tokens'),
                               (lengths, torch.int64, (N, beam), 'lengths'), (scores, torch.float32, (N, beam), 'scores'),
                               (counts, torch.int64, (N,), 'counts'), (boosts, torch.float32, (N, beam), 'boosts'),
                               (states, torch.int64, (N, beam), 'states')):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'ctc_prefix_beam_advance_biased: {name} must be a contiguous {dt} HIP tensor {list(shape)}')
    check(lib().halo_ctc_prefix_beam_advance_biased(ptr(emissions), emissions.stride(0), emissions.stride(1), T, N, V, ptr(n_frames),
                                                    ptr(flags), beam, capacity, ptr(state), ptr(tokens), ptr(lengths), ptr(scores),
                                                    ptr(counts), ptr(columns), ptr(nxt), ptr(gain), nxt.shape[0], nxt.shape[1], ptr(boosts),
                                                    ptr(states), _stream()), 'halo_ctc_prefix_beam_advance_biased')


# ---- edit distance and the risk of an n-best list (csrc/edit_distance.hip) -----------------------------------------------------------
EDIT_DISTANCE_MAX_LEN = 1024     # HALO_EDIT_DISTANCE_MAX_LEN (include/halo.h)


def edit_distance(hyp, hyp_lengths, ref, ref_lengths, group):
    """hyp [P, Lh] int64 (any row stride, unit token stride), hyp_lengths [P] int32, ref [R, Lr] int64, ref_lengths [R] int32 contiguous,
    P = R * group -> (errors [P] int32, counts [P, 3] int32 = ins, del, sub) under the tie rule of include/halo.h."""
    for t, name in ((hyp, 'hyp'), (ref, 'ref')):
        if t.dtype != torch.int64 or t.dim() != 2 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f'edit_distance: {name} must be a two-dimensional int64 HIP tensor with unit stride along the tokens')
    P, R = hyp.shape[0], ref.shape[0]
    for t, name, n in ((hyp_lengths, 'hyp_lengths', P), (ref_lengths, 'ref_lengths', R)):
        if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'edit_distance: {name} must be a contiguous int32 HIP tensor of [{n}]')
    if group < 1 or R * group != P or P < 1:
        raise ValueError(f'edit_distance: {P} hypotheses are not {R} references x group {group}')
    errors = torch.empty(P, device=hyp.device, dtype=torch.int32)
    counts = torch.empty(P, 3, device=hyp.device, dtype=torch.int32)
    check(lib().halo_edit_distance(ptr(hyp), max(hyp.stride(0), hyp.shape[1]), ptr(hyp_lengths), P, hyp.shape[1], ptr(ref),
                                   max(ref.stride(0), ref.shape[1]), ptr(ref_lengths), R, ref.shape[1], group, ptr(errors), ptr(counts),
                                   _stream()), 'halo_edit_distance')
    return errors, counts


def _check_nbest(losses, errors):
    if losses.dim() != 2 or errors.dtype != torch.int32 or errors.shape != losses.shape or not errors.is_cuda or not errors.is_contiguous():
        raise ValueError('nbest_risk: losses must be [N, W] float32 and errors [N, W] int32, contiguous HIP tensors')
    return _f32c(losses, 'losses').shape


def nbest_risk_fwd(losses, errors):
    """losses [N, W] f32, errors [N, W] int32 (< 0: absent) -> risk [N] f32 (include/halo.h)."""
    N, W = _check_nbest(losses, errors)
    risk = torch.empty(N, device=losses.device, dtype=torch.float32)
    check(lib().halo_nbest_risk_fwd(ptr(losses), ptr(errors), N, W, ptr(risk), _stream()), 'halo_nbest_risk_fwd')
    return risk


def nbest_risk_bwd(losses, errors, grad_risk):
    """grad_risk [N] f32 -> dlosses [N, W] f32."""
    N, W = _check_nbest(losses, errors)
    if tuple(_f32c(grad_risk, 'grad_risk').shape) != (N,):
        raise ValueError(f'nbest_risk: grad_risk must be [{N}]')
    dlosses = torch.empty(N, W, device=losses.device, dtype=torch.float32)
    check(lib().halo_nbest_risk_bwd(ptr(losses), ptr(errors), N, W, ptr(grad_risk), ptr(dlosses), _stream()), 'halo_nbest_risk_bwd')
    return dlosses


# ---- fused launches of a greedy decode step (csrc/decode.hip) -------------------------------------------------
def decode_linear_supported(k, layernorm):
    return bool(lib().halo_decode_linear_supported(k, int(layernorm)))


def decode_image(weight):
    """Decode image (split-bf16 fragments in MFMA operand order) of an nn.Linear weight [n_out, k]."""
    _f32c(weight, 'weight')
    n_out, k = weight.shape
    img = torch.empty(lib().halo_decode_image_bytes(n_out, k), device=weight.device, dtype=torch.uint8)
    check(lib().halo_decode_image(ptr(weight), n_out, k, k, ptr(img), _stream()), 'halo_decode_image')
    return img


def decode_linear(x, image, n_out, out, ln_weight=None, eps=1e-5, accumulate=False, gelu=False, x_side=None, side_in=None, side_out=None):
    """out (+)= act(layer_norm?(x) W^T) with W given by its decode image; x [rows, k] and out [rows, >= n_out] fp32 (row strides kept).
    The residual stream as a pair (halo_decode_linear_pair): ``x_side`` (LayerNorm variants) is added to the input rows; ``side_out``
    (accumulating, no LayerNorm, k % 512 == 0) runs the product as two K-slices: out = (out + side_in) + the first half, side_out = the
    second -- the next launch reads out + side_out."""
    rows, k = x.shape
    flags = (_lib.HALO_GEMM_ACCUM if accumulate else 0) | (_lib.HALO_GEMM_GELU_ERF if gelu else 0)
    if x_side is None and side_out is None and side_in is None:
        check(lib().halo_decode_linear(ptr(x), x.stride(0), rows, k, ptr(ln_weight), eps, ptr(image), n_out, ptr(out), out.stride(0), flags,
                                       _stream()), 'halo_decode_linear')
        return out
    for t in (x_side,):
        if t is not None and (t.shape != x.shape or t.stride(0) != x.stride(0)):
            raise ValueError('decode_linear: x_side must have the shape and row stride of x')
    for t in (side_in, side_out):
        if t is not None and (t.shape != out.shape or t.stride(0) != out.stride(0)):
            raise ValueError('decode_linear: side_in / side_out must have the shape and row stride of out')
    check(lib().halo_decode_linear_pair(ptr(x), ptr(x_side), x.stride(0), rows, k, ptr(ln_weight), eps, ptr(image), n_out, ptr(out), ptr(side_in),
                                        ptr(side_out), out.stride(0), flags, _stream()), 'halo_decode_linear_pair')
    return out


def decode_attention_pair(a, mem_k, mem_v, memory_lengths, time_k, time_v, n_keys, table, out):
    """a [N, 4C] = cross query | self q | k | v -> out [N, 2C] = cross-attention output | self-attention output (one launch)."""
    N, heads, S, hd = mem_k.shape
    check(lib().halo_decode_attention_pair(ptr(a), a.stride(0), N, heads, hd, ptr(mem_k), ptr(mem_v), S, ptr(memory_lengths), ptr(time_k),
                                           ptr(time_v), time_k.shape[2], n_keys, ptr(table.cos) if table else None,
                                           ptr(table.sin) if table else None, ptr(out), out.stride(0), _stream()),
          'halo_decode_attention_pair')
    return out


def decode_memory_caches(kv, caches):
    """caches [L, 2, N, heads, S, head_dim] float16 <- kv rows [N*S, L*2C] (layer l: keys at columns l*2C, values at l*2C + C)."""
    L, _, N, heads, S, hd = caches.shape
    check(lib().halo_decode_memory_caches(ptr(kv), kv.stride(0), L, ptr(caches), N, S, heads, hd, _stream()), 'halo_decode_memory_caches')


def decode_token(logits, tokens, t, plen, etx, alive, out_len, log_probs, sum_ent, wte=None, y_next=None):
    """alive: uint8 [2, N], double-buffered -- step t reads plane t & 1 and writes plane (t + 1) & 1."""
    N, V = logits.shape
    if alive.shape != (2, N) or not alive.is_contiguous():
        raise ValueError('decode_token: alive must be a contiguous [2, N] uint8 tensor')
    check(lib().halo_decode_token(ptr(logits), logits.stride(0), N, V, ptr(tokens), tokens.stride(0), t, plen, etx, ptr(alive),
                                  ptr(out_len), ptr(log_probs), ptr(sum_ent), ptr(wte), wte.shape[0] if wte is not None else 0,
                                  wte.shape[1] if wte is not None else 0, ptr(y_next), _stream()), 'halo_decode_token')


# ---- the two launches of the attention decoder's beam search (csrc/decode.hip, decode_beam.hip); neither allocates ------------------
def decode_beam_attention(a, mem_k, mem_v, memory_lengths, time_k, time_v, n_keys, ancestors, table, out):
    """decode_attention_pair over slots = N * W rows a [slots, 4C]: mem_k / mem_v [N, heads, S, hd] per utterance, time_k / time_v
    [slots, heads, Tc, hd]; position j < n_keys - 1 is read from cache row ancestors[slot, j] (int32 [slots, >= n_keys - 1])."""
    N, heads, S, hd = mem_k.shape
    slots = time_k.shape[0]
    if slots % N or a.shape[0] != slots or out.shape[0] != slots or ancestors.shape[0] != slots or ancestors.dtype != torch.int32 \
            or ancestors.stride(1) != 1:
        raise ValueError('decode_beam_attention: a, out, ancestors (int32) and the time caches must have N * W rows')
    check(lib().halo_decode_beam_attention(ptr(a), a.stride(0), slots, slots // N, heads, hd, ptr(mem_k), ptr(mem_v), S, ptr(memory_lengths),
                                           ptr(time_k), ptr(time_v), time_k.shape[2], n_keys, ptr(ancestors), ancestors.stride(0),
                                           ptr(table.cos) if table else None, ptr(table.sin) if table else None, ptr(out), out.stride(0),
                                           _stream()), 'halo_decode_beam_attention')
    return out


def _check_beam_select(name, logits, beam_in, beam_out, ranks_out, wte, y_next):
    N, W = ranks_out.shape
    V = logits.shape[1]
    tensors = (*beam_in, *beam_out, ranks_out)
    if not all(x.is_contiguous() for x in tensors) or logits.shape[0] != N * W or logits.stride(1) != 1:
        raise ValueError(f'{name}: logits must be [N * W, V] with unit class stride and every record contiguous')
    for rec in (beam_in, beam_out):
        if any(x.shape != (N, W) for x in rec[:3]) or rec[3].shape[:2] != (N, W) or rec[4].shape[0] != N * W \
                or rec[0].dtype != torch.float32 or any(x.dtype != torch.int32 for x in rec[1:]):
            raise ValueError(f'{name}: records are (scores f32, lengths, finished [N, W], tokens [N, W, ld], ancestors [N * W, ld] int32)')
    if beam_in[3].shape != beam_out[3].shape or beam_in[4].shape != beam_out[4].shape:
        raise ValueError(f'{name}: the two copies of the beam must have one shape')
    if y_next is not None and (not y_next.is_contiguous() or not wte.is_contiguous() or y_next.shape != (N * W, wte.shape[1])):
        raise ValueError(f'{name}: y_next must be a contiguous [N * W, C] and wte contiguous')
    return N, W, V


def decode_beam_select(logits, t, capacity, etx, length_bonus, beam_in, beam_out, ranks_out, wte=None, y_next=None):
    """One step of the beam (include/halo.h) on logits [N * W, V]: beam_in / beam_out = (scores [N, W] fp32, lengths [N, W] int32,
    finished [N, W] int32, tokens [N, W, >= capacity] int32, ancestors [N * W, > t] int32), two distinct copies; ranks_out [N, W] fp32;
    y_next [N * W, C] <- wte[token]."""
    N, W, V = _check_beam_select('decode_beam_select', logits, beam_in, beam_out, ranks_out, wte, y_next)
    check(lib().halo_decode_beam_select(ptr(logits), logits.stride(0), N, W, V, int(t), int(capacity), int(etx), float(length_bonus),
                                        *(ptr(x) for x in beam_in), ptr(beam_out[0]), ptr(ranks_out), *(ptr(x) for x in beam_out[1:]),
                                        beam_in[3].shape[2], beam_in[4].shape[1], ptr(wte), wte.shape[0] if wte is not None else 0,
                                        wte.shape[1] if wte is not None else 0, ptr(y_next), _stream()), 'halo_decode_beam_select')


# ---- the three launches the joint CTC/attention search adds to a step (csrc/ctc_prefix_score.hip, decode_beam.hip); none allocates ------
def _prefix_shapes(name, log_probs, input_lengths, states, W):
    if log_probs.dim() != 3 or log_probs.dtype != torch.float32 or log_probs.stride(2) != 1:
        raise ValueError(f'{name}: log_probs must be float32 [N, S, V] with unit class stride')
    N, S, V = log_probs.shape
    if input_lengths.shape != (N,) or input_lengths.dtype != torch.int32 or not input_lengths.is_contiguous():
        raise ValueError(f'{name}: input_lengths must be a contiguous int32 [N]')
    for st in states:
        if st is not None and (st.shape != (N * W, S, 2) or st.dtype != torch.float32 or not st.is_contiguous()):
            raise ValueError(f'{name}: states must be contiguous float32 [N * W, S, 2]')
    return N, S, V


def _prefix_records(name, N, W, ints, floats=()):
    if any(x.shape != (N, W) or x.dtype != torch.int32 or not x.is_contiguous() for x in ints) \
            or any(x.shape != (N, W) or x.dtype != torch.float32 or not x.is_contiguous() for x in floats):
        raise ValueError(f'{name}: the records must be contiguous [N, W] tensors, int32 (float32: scores)')


def ctc_prefix_scores(log_probs, input_lengths, states, t, etx, psi_cand, last_tokens=None, lengths=None, scores=None, finished=None):
    """psi_cand [N * W, V] <- the CTC prefix score of every candidate of every live slot (include/halo.h), -inf in the rows of empty and
    finished slots; log_probs [N, S, V], states [N * W, S, 2], the records [N, W] as decode_beam_select reads them (none at t == 0)."""
    if psi_cand.dim() != 2 or psi_cand.dtype != torch.float32 or psi_cand.stride(1) != 1 or psi_cand.shape[0] % log_probs.shape[0]:
        raise ValueError('ctc_prefix_scores: psi_cand must be float32 [N * W, V] with unit class stride')
    W = psi_cand.shape[0] // log_probs.shape[0]
    N, S, V = _prefix_shapes('ctc_prefix_scores', log_probs, input_lengths, (states,), W)
    if psi_cand.shape[1] != V:
        raise ValueError('ctc_prefix_scores: psi_cand and log_probs differ in the class count')
    if int(t) > 0:
        if any(x is None for x in (last_tokens, lengths, scores, finished)):
            raise ValueError('ctc_prefix_scores: the records are needed after step 0')
        _prefix_records('ctc_prefix_scores', N, W, (last_tokens, lengths, finished), (scores,))
    check(lib().halo_ctc_prefix_scores(ptr(log_probs), log_probs.stride(0), log_probs.stride(1), N, W, S, V, ptr(input_lengths), ptr(states),
                                       ptr(last_tokens), ptr(lengths), ptr(scores), ptr(finished), int(t), int(etx), ptr(psi_cand),
                                       psi_cand.stride(0), _stream()), 'halo_ctc_prefix_scores')
    return psi_cand


def ctc_prefix_advance(log_probs, input_lengths, etx, states_out, states_in=None, parents=None, last_new=None, lengths_new=None,
                       last_prev=None):
    """states_out [N * W, S, 2] <- the state of every slot that took a label, from its parent's in states_in (parents, last_new,
    lengths_new: what decode_beam_select_joint wrote; last_prev: the parents' last tokens).  parents None: the empty prefix's state into
    slot 0 of every utterance."""
    if log_probs.dim() != 3 or states_out.dim() != 3 or states_out.shape[0] % log_probs.shape[0]:
        raise ValueError('ctc_prefix_advance: log_probs must be [N, S, V] and states [N * W, S, 2]')
    W = states_out.shape[0] // log_probs.shape[0]
    N, S, V = _prefix_shapes('ctc_prefix_advance', log_probs, input_lengths, (states_out, states_in), W)
    if parents is not None:
        if any(x is None for x in (states_in, last_new, lengths_new, last_prev)):
            raise ValueError('ctc_prefix_advance: parents come with states_in, last_new, lengths_new and last_prev')
        _prefix_records('ctc_prefix_advance', N, W, (parents, last_new, lengths_new, last_prev))
    check(lib().halo_ctc_prefix_advance(ptr(log_probs), log_probs.stride(0), log_probs.stride(1), N, W, S, V, ptr(input_lengths), int(etx),
                                        ptr(states_in), ptr(states_out), ptr(parents), ptr(last_new), ptr(lengths_new), ptr(last_prev),
                                        _stream()), 'halo_ctc_prefix_advance')
    return states_out


def decode_beam_select_joint(logits, t, capacity, etx, length_bonus, ctc_weight, psi_cand, psi_in, psi_out, beam_in, beam_out, ranks_out,
                             parents_out, last_out, wte=None, y_next=None):
    """decode_beam_select with rank = (1 - ctc_weight) * rank + ctc_weight * psi: psi_cand [N * W, V] from ctc_prefix_scores, psi_in /
    psi_out [N, W] float32 (two copies), parents_out / last_out [N, W] int32 <- the parent's slot index (-1: empty), the token taken."""
    N, W, V = _check_beam_select('decode_beam_select_joint', logits, beam_in, beam_out, ranks_out, wte, y_next)
    if psi_cand.shape != (N * W, V) or psi_cand.dtype != torch.float32 or psi_cand.stride(1) != 1:
        raise ValueError('decode_beam_select_joint: psi_cand must be float32 [N * W, V] with unit class stride')
    _prefix_records('decode_beam_select_joint', N, W, (parents_out, last_out), (psi_in, psi_out))
    if not 0.0 <= float(ctc_weight) <= 1.0:
        raise ValueError(f'decode_beam_select_joint: ctc_weight {ctc_weight} outside [0, 1]')
    check(lib().halo_decode_beam_select_joint(ptr(logits), logits.stride(0), N, W, V, int(t), int(capacity), int(etx), float(length_bonus),
                                              float(ctc_weight), ptr(psi_cand), psi_cand.stride(0), ptr(psi_in), ptr(psi_out),
                                              *(ptr(x) for x in beam_in), ptr(beam_out[0]), ptr(ranks_out), *(ptr(x) for x in beam_out[1:]),
                                              ptr(parents_out), ptr(last_out), beam_in[3].shape[2], beam_in[4].shape[1], ptr(wte),
                                              wte.shape[0] if wte is not None else 0, wte.shape[1] if wte is not None else 0, ptr(y_next),
                                              _stream()), 'halo_decode_beam_select_joint')


# ---- the selection with LM shallow fusion (csrc/decode_beam.hip); it does not allocate -----------------------------------
DECODE_BEAM_LM_LDS_FLOATS = 14336    # HALO_DECODE_BEAM_LM_LDS_FLOATS (include/halo.h): both tables stay in LDS while 2 W V <= this


def decode_beam_select_lm(logits, t, capacity, etx, length_bonus, lm_logits, lm_bias, lm_in, lm_out, lm_weight, lm_eos, beam_in, beam_out,
                          ranks_out, parents_out, last_out, lm_wte=None, h_in=None, c_in=None, lm_xh=None, c_out=None, wte=None, y_next=None,
                          ctc_weight=0.0, psi_cand=None, psi_in=None, psi_out=None):
    """decode_beam_select (psi_cand None) or decode_beam_select_joint with rank = fmaf(lm_weight, lmc, rank) (include/halo.h): lm_logits
    [N * W, V] the LM's logits without their bias, lm_bias [V] or None, lm_in / lm_out [N, W] float32 (two copies), lm_eos -1 .. V-1 or
    None.  With lm_xh (None: the last step) the next LM step's cell inputs are gathered: h_in, c_in, c_out [Ll, N * W, H], lm_xh
    [Ll, N * W, 2 H], lm_wte [V, H], all contiguous float32."""
    name = 'decode_beam_select_lm'
    N, W, V = _check_beam_select(name, logits, beam_in, beam_out, ranks_out, wte, y_next)
    if lm_logits.shape != (N * W, V) or lm_logits.dtype != torch.float32 or lm_logits.stride(1) != 1:
        raise ValueError(f'{name}: lm_logits must be float32 [N * W, V] with unit class stride')
    if lm_bias is not None and (lm_bias.shape != (V,) or lm_bias.dtype != torch.float32 or not lm_bias.is_contiguous()):
        raise ValueError(f'{name}: lm_bias must be a contiguous float32 [V]')
    _prefix_records(name, N, W, (parents_out, last_out), (lm_in, lm_out))
    eos = -1 if lm_eos is None else int(lm_eos)
    if not math.isfinite(float(lm_weight)) or eos < -1 or eos >= V:
        raise ValueError(f'{name}: lm_weight must be finite and lm_eos in -1 .. {V - 1}')
    if psi_cand is not None:
        if psi_cand.shape != (N * W, V) or psi_cand.dtype != torch.float32 or psi_cand.stride(1) != 1:
            raise ValueError(f'{name}: psi_cand must be float32 [N * W, V] with unit class stride')
        _prefix_records(name, N, W, (), (psi_in, psi_out))
        if not 0.0 <= float(ctc_weight) <= 1.0:
            raise ValueError(f'{name}: ctc_weight {ctc_weight} outside [0, 1]')
    elif psi_in is not None or psi_out is not None:
        raise ValueError(f'{name}: psi_in / psi_out come with psi_cand')
    H = Ll = 0
    if lm_xh is not None:
        if any(x is None for x in (lm_wte, h_in, c_in, c_out)):
            raise ValueError(f'{name}: lm_xh comes with lm_wte, h_in, c_in and c_out')
        Ll, H = _check_slot_state(name, 'LM', V, N * W, lm_wte, h_in, c_in, lm_xh, c_out)
        if lm_wte.shape[0] != V:
            raise ValueError(f'{name}: lm_wte must be [V, H]')
    else:
        lm_wte = h_in = c_in = c_out = None
    check(lib().halo_decode_beam_select_lm(ptr(logits), logits.stride(0), N, W, V, int(t), int(capacity), int(etx), float(length_bonus),
                                           float(ctc_weight), ptr(psi_cand), psi_cand.stride(0) if psi_cand is not None else 0, ptr(psi_in),
                                           ptr(psi_out), ptr(lm_logits), lm_logits.stride(0), ptr(lm_bias), ptr(lm_in), ptr(lm_out),
                                           float(lm_weight), eos, *(ptr(x) for x in beam_in), ptr(beam_out[0]), ptr(ranks_out),
                                           *(ptr(x) for x in beam_out[1:]), ptr(parents_out), ptr(last_out), beam_in[3].shape[2],
                                           beam_in[4].shape[1], ptr(wte), wte.shape[0] if wte is not None else 0,
                                           wte.shape[1] if wte is not None else 0, ptr(y_next), ptr(lm_wte), H, Ll, ptr(h_in), ptr(c_in),
                                           ptr(lm_xh), ptr(c_out), _stream()), 'halo_decode_beam_select_lm')


# ---- fused launches of a GPT sampling step (csrc/gpt_decode.hip); none of these allocates: they run inside a captured step ----------
def gpt_decode_linear_supported(k, layernorm):
    return bool(lib().halo_gpt_decode_linear_supported(k, int(layernorm)))


def gpt_decode_linear(x, image, n_out, out, ln_weight=None, eps=1e-5, accumulate=False, gelu=False):
    """out (+)= act(layer_norm?(x) W^T) with W given by its decode image, in the library's math mode (tanh-GELU)."""
    rows, k = x.shape
    flags = (_lib.HALO_GEMM_ACCUM if accumulate else 0) | (_lib.HALO_GEMM_GELU if gelu else 0)
    check(lib().halo_gpt_decode_linear(ptr(x), x.stride(0), rows, k, ptr(ln_weight), eps, ptr(image), n_out, ptr(out), out.stride(0), flags,
                                       _stream()), 'halo_gpt_decode_linear')
    return out


def gpt_decode_attention(qkv, cache_k, cache_v, pos, out):
    """qkv [B, 3C] -> out [B, C]; row b's k / v are stored at position pos[b] (device int32) of cache_{k,v} [B, heads, Tc, 64] fp32."""
    B, heads, Tc, hd = cache_k.shape
    check(lib().halo_gpt_decode_attention(ptr(qkv), qkv.stride(0), B, heads, hd, ptr(cache_k), ptr(cache_v), Tc, ptr(pos), ptr(out),
                                          out.stride(0), _stream()), 'halo_gpt_decode_attention')
    return out


def gpt_sample_cfg(temperature, top_k, stop_token, seed, device):
    """The draw's settings as the device words halo_gpt_sample reads (include/halo.h)."""
    import struct
    if not temperature > 0.0:
        raise ValueError('temperature must be positive')
    inv = struct.unpack('<i', struct.pack('<f', 1.0 / float(temperature)))[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s32 = lambda u: u - (1 << 32) if u >= (1 << 31) else u
    stop = int(stop_token)
    if not -(1 << 31) <= stop < (1 << 31):
        stop = -1
    words = [inv, int(top_k) if top_k is not None else 0, stop, s32(seed & 0xFFFFFFFF), s32(seed >> 32), 0, 0, 0]
    return torch.tensor(words, dtype=torch.int32).to(device, non_blocking=True)


def gpt_sample(logits, cfg, state, tokens, next_ids, wte=None, wpe=None, x_next=None):
    """One draw per row of logits [B, V] and the step's bookkeeping (include/halo.h): state int32 [4, >= B] = pos | step | length |
    alive; tokens int64 [B, n_slots] receives slot ``step``; next_ids int64 [B]; x_next [B, C] <- wte[token] + wpe[pos + 1]."""
    B, V = logits.shape
    check(lib().halo_gpt_sample(ptr(logits), logits.stride(0), B, V, ptr(cfg), ptr(state), state.stride(0), ptr(tokens), tokens.stride(0),
                                tokens.shape[1], ptr(next_ids), ptr(wte), ptr(wpe), wpe.shape[0] if wpe is not None else 0,
                                wte.shape[1] if wte is not None else 0, ptr(x_next), _stream()), 'halo_gpt_sample')


# ---- launches of the transducer's greedy decode (csrc/rnnt_decode.hip); none of these allocates ---------------------------------
def rnnt_advance(f, g, g_bias, input_lengths, state, scores, tokens, frames, max_symbols, wte, x_next, live):
    """One advance of every row (include/halo.h): f [N, T, V] transcription logits, g [N, V] prediction logits (bias apart), state int32
    [5, >= N] = t | u | here | done | truncated, tokens / frames int64 [N, capacity], x_next [N, >= E] <- wte[k], live: one int32 word."""
    N, T, V = f.shape
    if f.stride(2) != 1 or tokens.stride(0) != frames.stride(0) or tokens.shape != frames.shape:
        raise ValueError('rnnt_advance: f must be contiguous along V; tokens and frames must share shape and row stride')
    if wte.shape[0] < V or g.shape != (N, V):
        raise ValueError('rnnt_advance: g must be [N, V] and the embedding must have a row for every symbol')
    check(lib().halo_rnnt_advance(ptr(f), f.stride(0), f.stride(1), N, T, V, ptr(g), g.stride(0), ptr(g_bias), ptr(input_lengths), ptr(state),
                                  state.stride(0), ptr(scores), ptr(tokens), ptr(frames), tokens.stride(0), tokens.shape[1], int(max_symbols),
                                  ptr(wte), wte.shape[1], ptr(x_next), x_next.stride(0), ptr(live), _stream()), 'halo_rnnt_advance')


def rnnt_lstm_cell(xh, image, b_ih, b_hh, c, h_next, h_up, row_mask=None):
    """One LSTM layer at one step: xh [rows, 2H] = x | h_prev, image: the decode image of the gate-interleaved [W_ih | W_hh]
    (include/halo.h); c [rows, H] in place; h -> h_next and h_up (row strides kept).  ``row_mask`` int32 [rows] (halo_rnnt_lstm_cell_rows):
    a row with 0 keeps c, has its h_prev copied to h_next and writes no h_up."""
    rows, H = c.shape
    if row_mask is None:
        check(lib().halo_rnnt_lstm_cell(ptr(xh), xh.stride(0), rows, H, ptr(image), ptr(b_ih), ptr(b_hh), ptr(c), ptr(h_next),
                                        h_next.stride(0), ptr(h_up), h_up.stride(0), _stream()), 'halo_rnnt_lstm_cell')
        return
    if row_mask.dtype != torch.int32 or row_mask.numel() < rows or not row_mask.is_contiguous():
        raise ValueError(f'rnnt_lstm_cell: row_mask must be a contiguous int32 tensor of at least {rows} words')
    check(lib().halo_rnnt_lstm_cell_rows(ptr(xh), xh.stride(0), rows, H, ptr(image), ptr(b_ih), ptr(b_hh), ptr(c), ptr(h_next),
                                         h_next.stride(0), ptr(h_up), h_up.stride(0), ptr(row_mask), _stream()), 'halo_rnnt_lstm_cell_rows')


def rnnt_stream_open(n_frames, flags, state, pos, row_mask, scores, tokens, frames, xh, c, wte, live):
    """Opens a call of the carried greedy search (include/halo.h): n_frames [B] int32 and flags [>= B] int32 or None (bit STREAM_BEGIN)
    for the first B of the rows of state int32 [5, rows]; pos / row_mask int32 [rows]; tokens / frames int64 [rows, capacity]; xh
    [L, rows, 2H]: the [x | h] copy the next step reads; c [L, rows, H]; live: the call's int32 words, zeroed."""
    B, rows = n_frames.shape[0], pos.shape[0]
    L, H = c.shape[0], c.shape[2]
    for t, name in ((n_frames, 'n_frames'), (flags, 'flags'), (pos, 'pos'), (row_mask, 'row_mask'), (live, 'live')):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError(f'rnnt_stream_open: {name} must be a contiguous int32 tensor')
    if state.shape[1] != rows or row_mask.shape[0] != rows or scores.shape[0] != rows or tokens.shape[0] != rows or \
            tokens.shape != frames.shape or tokens.stride(0) != frames.stride(0) or xh.shape != (L, rows, 2 * H) or c.shape[1] != rows or \
            (flags is not None and flags.shape[0] < B) or xh.stride(2) != 1 or not c.is_contiguous():
        raise ValueError('rnnt_stream_open: the state tensors do not fit each other')
    check(lib().halo_rnnt_stream_open(ptr(n_frames), ptr(flags), B, rows, ptr(state), state.stride(0), ptr(pos), ptr(row_mask), ptr(scores),
                                      ptr(tokens), ptr(frames), tokens.stride(0), tokens.shape[1], ptr(xh), xh.stride(0), xh.stride(1),
                                      ptr(c), c.stride(0), ptr(wte), wte.shape[1], H, L, ptr(live), live.numel(), _stream()),
          'halo_rnnt_stream_open')


def rnnt_advance_stream(f, g, g_bias, n_frames, state, scores, tokens, frames, max_symbols, wte, x_next, live, pos, row_mask):
    """``rnnt_advance`` over this call's chunk f [N, S, V] from pos (include/halo.h: halo_rnnt_advance_stream): a row that runs out of
    its n_frames waits; row_mask [>= N] int32 <- whether the row emitted and goes on."""
    N, T, V = f.shape
    if f.stride(2) != 1 or tokens.stride(0) != frames.stride(0) or tokens.shape != frames.shape:
        raise ValueError('rnnt_advance_stream: f must be contiguous along V; tokens and frames must share shape and row stride')
    if wte.shape[0] < V or g.shape != (N, V) or pos.numel() < N or row_mask.numel() < N or n_frames.numel() < N:
        raise ValueError('rnnt_advance_stream: g must be [N, V], the embedding must have a row for every symbol, pos / row_mask / n_frames N words')
    check(lib().halo_rnnt_advance_stream(ptr(f), f.stride(0), f.stride(1), N, T, V, ptr(g), g.stride(0), ptr(g_bias), ptr(n_frames),
                                         ptr(state), state.stride(0), ptr(scores), ptr(tokens), ptr(frames), tokens.stride(0),
                                         tokens.shape[1], int(max_symbols), ptr(wte), wte.shape[1], ptr(x_next), x_next.stride(0),
                                         ptr(live), ptr(pos), ptr(row_mask), _stream()), 'halo_rnnt_advance_stream')


# ---- launches of the transducer's beam search (csrc/rnnt_beam.hip); none of these allocates ----------------------------------------
def _check_slot_state(name, who, V, slots, wte, h_in, c_in, xh, c_out):
    """The gather arguments of a beam step for one network (``who``): h_in / c_in / c_out [layers, slots, H], xh [layers, slots, 2 H] and
    the embedding [>= V, H], all contiguous float32 -> (layers, H)."""
    layers, H = (h_in.shape[0], h_in.shape[2]) if h_in.dim() == 3 else (0, 0)
    state = (layers, slots, H)
    if h_in.shape != state or c_in.shape != state or c_out.shape != state or xh.shape != (layers, slots, 2 * H) \
            or wte.shape != (wte.shape[0], H) or wte.shape[0] < V or not all(x.dtype == torch.float32 and x.is_contiguous()
                                                                             for x in (wte, h_in, c_in, xh, c_out)):
        raise ValueError(f'{name}: of the {who}, h_in, c_in and c_out must be contiguous float32 [layers, {slots}, H], xh [layers, {slots}, '
                         f'2 H] and the embedding [>= {V}, H]')
    return layers, H


def rnnt_beam_step(f, g, g_bias, input_lengths, step, capacity, rec_in, rec_out, parent, last, finals, wte, h_in, c_in, xh, c_out, live):
    """One alignment step of every row (include/halo.h): f [N, T, V]; g [N * W, V] (bias apart); rec_in / rec_out = (scores [N, W] fp32,
    u [N, W] int32, tokens [N, W, >= capacity] int32); parent / last [N, W] int32; finals = (scores, seq, lengths [N, W], tokens
    [N, W, >= capacity], n [N]); h_in / c_in / c_out [layers, N * W, H], xh [layers, N * W, 2 H], all contiguous; live: one int32 word."""
    N, T, V = f.shape
    W = parent.shape[1]
    layers, H = _check_slot_state('rnnt_beam_step', 'prediction network', V, N * W, wte, h_in, c_in, xh, c_out)
    if f.stride(2) != 1 or not all(t.is_contiguous() for t in (g, *rec_in, *rec_out, parent, last, *finals)):
        raise ValueError('rnnt_beam_step: f must be contiguous along V and every other tensor contiguous')
    if g.shape != (N * W, V):
        raise ValueError('rnnt_beam_step: g must be [N * W, V]')
    ld = rec_in[2].shape[2]
    if any(t.shape != (N, W) for t in (rec_in[0], rec_in[1], rec_out[0], rec_out[1], parent, last, finals[0], finals[1], finals[2])) \
            or any(t.shape != (N, W, ld) for t in (rec_in[2], rec_out[2], finals[3])) or finals[4].shape != (N,):
        raise ValueError('rnnt_beam_step: records and finals must be [N, W] with tokens [N, W, ld]')
    check(lib().halo_rnnt_beam_step(ptr(f), f.stride(0), f.stride(1), N, T, V, ptr(g), g.stride(0), ptr(g_bias), ptr(input_lengths), int(step), W,
                                    int(capacity), ptr(rec_in[0]), ptr(rec_in[1]), ptr(rec_in[2]), ptr(rec_out[0]), ptr(rec_out[1]),
                                    ptr(rec_out[2]), ld, ptr(parent), ptr(last), ptr(finals[0]), ptr(finals[1]), ptr(finals[2]),
                                    ptr(finals[3]), ptr(finals[4]), ptr(wte), H, layers, ptr(h_in), ptr(c_in), ptr(xh), ptr(c_out), ptr(live),
                                    _stream()), 'halo_rnnt_beam_step')


def rnnt_beam_keep(parent, last, h_in, c_in, g_in, h_out, c_out, g_out):
    """Blank-extended slots take their parent's h, c [layers, N * W, H] and g [N * W, V] from the step's input copy (include/halo.h)."""
    N, W = parent.shape
    layers, slots, H = h_in.shape
    tensors = (parent, last, h_in, c_in, g_in, h_out, c_out, g_out)
    if not all(t.is_contiguous() for t in tensors) or slots != N * W or g_in.shape[0] != slots or g_out.shape != g_in.shape \
            or last.shape != parent.shape or any(t.shape != h_in.shape for t in (c_in, h_out, c_out)):
        raise ValueError('rnnt_beam_keep: contiguous parent / last [N, W], state [layers, N * W, H] and g [N * W, V]')
    check(lib().halo_rnnt_beam_keep(slots, W, g_in.shape[1], H, layers, ptr(parent), ptr(last), ptr(h_in), ptr(c_in), ptr(g_in), g_in.stride(0),
                                    ptr(h_out), ptr(c_out), ptr(g_out), _stream()), 'halo_rnnt_beam_keep')


def rnnt_beam_stream_open(f, n_frames, flags, ring, stream_state, rec, finals, zero_state, h, c, g, live):
    """Opens a call of the carried beam search (include/halo.h): f [B, S, V] with unit class stride, n_frames [B] int32 and flags [>= B]
    int32 or None (bits STREAM_BEGIN, STREAM_FINAL) for the first B of the rows of ring [rows, ring_frames, V] and stream_state int32
    [4, rows]; rec = (scores, u [rows, W], ...) and h / c [layers, rows * W, H], g [rows * W, V] of the copy the next step reads;
    finals as ``rnnt_beam_step``'s; zero_state = (h0, c0 [layers, H], g0 [V]); live: the call's int32 words, zeroed."""
    B, S, V = f.shape
    rows, W = rec[0].shape
    layers, slots, H = h.shape
    tensors = (n_frames, ring, stream_state, rec[0], rec[1], *finals, *zero_state, h, c, g, live) + (() if flags is None else (flags,))
    if f.stride(2) != 1 or not all(t.is_contiguous() for t in tensors):
        raise ValueError('rnnt_beam_stream_open: f must be contiguous along V and every other tensor contiguous')
    if ring.shape[0] != rows or ring.shape[2] != V or ring.shape[1] < S or stream_state.shape != (4, rows) or slots != rows * W \
            or n_frames.shape != (B,) or B > rows or (flags is not None and flags.shape[0] < B) or c.shape != h.shape \
            or g.shape != (slots, V) or zero_state[0].shape != (layers, H) or zero_state[1].shape != (layers, H) \
            or zero_state[2].shape != (V,) or any(t.shape != (rows, W) for t in (rec[1], finals[0], finals[1], finals[2])) \
            or finals[4].shape != (rows,):
        raise ValueError('rnnt_beam_stream_open: the tensors do not fit each other')
    if any(t.dtype != torch.int32 for t in (n_frames, stream_state, live) + (() if flags is None else (flags,))):
        raise ValueError('rnnt_beam_stream_open: n_frames, flags, stream_state and live must be int32')
    check(lib().halo_rnnt_beam_stream_open(ptr(f), f.stride(0), f.stride(1), B, S, V, ptr(n_frames), ptr(flags), rows, ptr(ring),
                                           ring.shape[1], ptr(stream_state), stream_state.stride(0), W, ptr(rec[0]), ptr(rec[1]),
                                           ptr(finals[0]), ptr(finals[1]), ptr(finals[2]), ptr(finals[4]), ptr(zero_state[0]),
                                           ptr(zero_state[1]), ptr(zero_state[2]), ptr(h), ptr(c), ptr(g), g.stride(0), H, layers,
                                           ptr(live), live.numel(), _stream()), 'halo_rnnt_beam_stream_open')


def rnnt_beam_step_stream(ring, g, g_bias, stream_state, capacity, rec_in, rec_out, parent, last, finals, wte, h_in, c_in, xh, c_out, live):
    """One round of the carried beam search for every row (include/halo.h): ``rnnt_beam_step`` with the frames read from ring [rows,
    ring_frames, V] and the step, the frames received and the final / closed flags from stream_state int32 [4, rows]; a row that
    cannot execute its step does an identity round."""
    rows, ring_frames, V = ring.shape
    W = parent.shape[1]
    layers, H = _check_slot_state('rnnt_beam_step_stream', 'prediction network', V, rows * W, wte, h_in, c_in, xh, c_out)
    if not all(t.is_contiguous() for t in (ring, g, stream_state, *rec_in, *rec_out, parent, last, *finals)):
        raise ValueError('rnnt_beam_step_stream: every tensor must be contiguous')
    if g.shape != (rows * W, V) or stream_state.shape != (4, rows) or stream_state.dtype != torch.int32:
        raise ValueError('rnnt_beam_step_stream: g must be [rows * W, V] and stream_state int32 [4, rows]')
    ld = rec_in[2].shape[2]
    if any(t.shape != (rows, W) for t in (rec_in[0], rec_in[1], rec_out[0], rec_out[1], parent, last, finals[0], finals[1], finals[2])) \
            or any(t.shape != (rows, W, ld) for t in (rec_in[2], rec_out[2], finals[3])) or finals[4].shape != (rows,):
        raise ValueError('rnnt_beam_step_stream: records and finals must be [rows, W] with tokens [rows, W, ld]')
    check(lib().halo_rnnt_beam_step_stream(ptr(ring), ring_frames, rows, V, ptr(g), g.stride(0), ptr(g_bias), ptr(stream_state),
                                           stream_state.stride(0), W, int(capacity), ptr(rec_in[0]), ptr(rec_in[1]), ptr(rec_in[2]),
                                           ptr(rec_out[0]), ptr(rec_out[1]), ptr(rec_out[2]), ld, ptr(parent), ptr(last), ptr(finals[0]),
                                           ptr(finals[1]), ptr(finals[2]), ptr(finals[3]), ptr(finals[4]), ptr(wte), H, layers, ptr(h_in),
                                           ptr(c_in), ptr(xh), ptr(c_out), ptr(live), _stream()), 'halo_rnnt_beam_step_stream')


# ---- the per-frame launch of CTC prefix beam search with LM shallow fusion (csrc/ctc_lm_beam.hip); it does not allocate ---------------
def ctc_lm_beam_step(emissions, emission_lengths, frame, capacity, lm_weight, insertion_bonus, g, g_bias, rec_in, rec_out, parent, last, wte,
                     h_in, c_in, xh, c_out):
    """Frame ``frame`` of every row (include/halo.h): emissions [T, N, V] fp32 with unit class stride; emission_lengths [N] int32;
    g [N * W, V] (bias apart); rec_in / rec_out = (rec [N, W, 4] fp32, meta [N, W, 4] int32, tokens [N, W, >= capacity] int32); parent /
    last [N, W] int32; h_in / c_in / c_out [layers, N * W, H], xh [layers, N * W, 2 H], all contiguous."""
    T, N, V = emissions.shape
    W = parent.shape[1]
    layers, H = _check_slot_state('ctc_lm_beam_step', 'LM', V, N * W, wte, h_in, c_in, xh, c_out)
    tensors = (g, *rec_in, *rec_out, parent, last, emission_lengths)
    if emissions.dtype != torch.float32 or emissions.stride(2) != 1 or not all(t.is_contiguous() for t in tensors):
        raise ValueError('ctc_lm_beam_step: emissions must be fp32 with unit class stride and every other tensor contiguous')
    if g.shape != (N * W, V):
        raise ValueError('ctc_lm_beam_step: g must be [N * W, V]')
    ld = rec_in[2].shape[2]
    if any(t.shape != (N, W, 4) for t in (rec_in[0], rec_in[1], rec_out[0], rec_out[1])) or last.shape != (N, W) \
            or any(t.shape != (N, W, ld) for t in (rec_in[2], rec_out[2])) or emission_lengths.shape != (N,) \
            or emission_lengths.dtype != torch.int32:
        raise ValueError('ctc_lm_beam_step: records must be [N, W, 4] with tokens [N, W, ld], parent / last [N, W], lengths [N] int32')
    check(lib().halo_ctc_lm_beam_step(ptr(emissions), emissions.stride(0), emissions.stride(1), T, N, V, ptr(emission_lengths), int(frame), W,
                                      int(capacity), float(lm_weight), float(insertion_bonus), ptr(g), g.stride(0), ptr(g_bias),
                                      ptr(rec_in[0]), ptr(rec_in[1]), ptr(rec_in[2]), ptr(rec_out[0]), ptr(rec_out[1]), ptr(rec_out[2]), ld,
                                      ptr(parent), ptr(last), ptr(wte), H, layers, ptr(h_in), ptr(c_in), ptr(xh), ptr(c_out), _stream()),
          'halo_ctc_lm_beam_step')


# ---- the per-step launch of transducer beam search with LM shallow fusion (csrc/rnnt_lm_beam.hip); it does not allocate ----------------
def rnnt_lm_beam_step(f, g, g_bias, lg, lg_bias, input_lengths, step, capacity, lm_weight, insertion_bonus, rec_in, rec_out, parent, last,
                      finals, wte, h_in, c_in, xh, c_out, lm_wte, lm_h_in, lm_c_in, lm_xh, lm_c_out, live):
    """One alignment step of every row (include/halo.h): f [N, T, V]; g / lg [N * W, V] the prediction network's / the LM's logits (biases
    apart); rec_in / rec_out = (rec [N, W, 3] fp32 = s | lm | rank, u [N, W] int32, tokens [N, W, >= capacity] int32); parent / last
    [N, W] int32; finals = (rec [N, W, 3] = rank | s | lm, seq, lengths [N, W], tokens [N, W, >= capacity], n [N]); per network h_in /
    c_in / c_out [layers, N * W, H] and xh [layers, N * W, 2 H] with its own layers and H, all contiguous; live: one int32 word."""
    N, T, V = f.shape
    W = parent.shape[1]
    slots = N * W
    tensors = (g, lg, *rec_in, *rec_out, parent, last, *finals, input_lengths)
    if f.dtype != torch.float32 or f.stride(2) != 1 or not all(t.is_contiguous() for t in tensors):
        raise ValueError('rnnt_lm_beam_step: f must be fp32 and contiguous along V and every other tensor contiguous')
    if g.shape != (slots, V) or lg.shape != (slots, V) or input_lengths.shape != (N,) or input_lengths.dtype != torch.int32:
        raise ValueError('rnnt_lm_beam_step: g and lg must be [N * W, V], input_lengths [N] int32')
    _check_slot_state('rnnt_lm_beam_step', 'prediction network', V, slots, wte, h_in, c_in, xh, c_out)
    _check_slot_state('rnnt_lm_beam_step', 'LM', V, slots, lm_wte, lm_h_in, lm_c_in, lm_xh, lm_c_out)
    ld = rec_in[2].shape[2]
    if any(t.shape != (N, W, 3) for t in (rec_in[0], rec_out[0], finals[0])) \
            or any(t.shape != (N, W) for t in (rec_in[1], rec_out[1], parent, last, finals[1], finals[2])) \
            or any(t.shape != (N, W, ld) for t in (rec_in[2], rec_out[2], finals[3])) or finals[4].shape != (N,) or ld < capacity:
        raise ValueError('rnnt_lm_beam_step: records and finals must be [N, W, 3] / [N, W] with tokens [N, W, ld >= capacity]')
    check(lib().halo_rnnt_lm_beam_step(ptr(f), f.stride(0), f.stride(1), N, T, V, ptr(g), g.stride(0), ptr(g_bias), ptr(lg), lg.stride(0),
                                       ptr(lg_bias), ptr(input_lengths), int(step), W, int(capacity), float(lm_weight),
                                       float(insertion_bonus), ptr(rec_in[0]), ptr(rec_in[1]), ptr(rec_in[2]), ptr(rec_out[0]),
                                       ptr(rec_out[1]), ptr(rec_out[2]), ld, ptr(parent), ptr(last), ptr(finals[0]), ptr(finals[1]),
                                       ptr(finals[2]), ptr(finals[3]), ptr(finals[4]), ptr(wte), h_in.shape[2], h_in.shape[0], ptr(h_in),
                                       ptr(c_in), ptr(xh), ptr(c_out), ptr(lm_wte), lm_h_in.shape[2], lm_h_in.shape[0], ptr(lm_h_in),
                                       ptr(lm_c_in), ptr(lm_xh), ptr(lm_c_out), ptr(live), _stream()), 'halo_rnnt_lm_beam_step')


# ---- channels-last conv front-end (ha/conv.py) -------------------------------------------------------------
def conv_out_length(T, ks, stride, pad):
    return (T + 2 * pad - ks) // stride + 1


def im2col_cl(x3d, ks, stride, pad):
    _f32c(x3d, 'x')
    N, T, Cin = x3d.shape
    To = conv_out_length(T, ks, stride, pad)
    col = torch.empty(N * To, Cin * ks, device=x3d.device, dtype=torch.float32)
    check(lib().halo_im2col_cl(ptr(x3d), ptr(col), N, T, Cin, ks, stride, pad, _stream()), 'halo_im2col_cl')
    return col, To


def col2im_cl(dcol, N, T, Cin, ks, stride, pad):
    """The fold: gradient of im2col_cl. dcol [N*T', Cin*ks] -> dx [N, T, Cin]."""
    _f32c(dcol, 'dcol')
    dx = torch.empty(N, T, Cin, device=dcol.device, dtype=torch.float32)
    check(lib().halo_col2im_cl(ptr(dcol), ptr(dx), N, T, Cin, ks, stride, pad, _stream()), 'halo_col2im_cl')
    return dx


def dwconv1d_cl(x3d, weight, bias, stride, pad):
    _f32c(x3d, 'x')
    N, T, Cn = x3d.shape
    ks = weight.shape[-1]
    To = conv_out_length(T, ks, stride, pad)
    y = torch.empty(N, To, Cn, device=x3d.device, dtype=torch.float32)
    check(lib().halo_dwconv1d_cl(ptr(x3d), ptr(weight), ptr(bias), ptr(y), N, T, Cn, ks, stride, pad, _stream()), 'halo_dwconv1d_cl')
    return y


# ---- backward operators of the GPT / transformer training step ----------------------------------------------
def attention_bwd(q, k, v, y, dy, lse, dq, dk, dv, N, heads, head_dim, Tq, Tk, causal=False, key_lengths=None, drop=NO_DROPOUT,
                  stream_id=0):
    """Gradients of attention_fwd written into the caller's dq / dk / dv views (row layouts like q / k / v)."""
    C = heads * head_dim
    _f32c(y, 'y'); _f32c(dy, 'dy')
    if k.stride(0) != v.stride(0) or dk.stride(0) != dv.stride(0):
        raise ValueError('k/v (and dk/dv) must share a row stride')
    delta = torch.empty(N, heads, Tq, device=q.device, dtype=torch.float32)
    check(lib().halo_attention_bwd(ptr(q), q.stride(0), q.stride(0) * Tq, ptr(k), ptr(v), k.stride(0), k.stride(0) * Tk, ptr(y), ptr(dy),
                                   C, C * Tq, ptr(lse), ptr(delta), ptr(dq), dq.stride(0), dq.stride(0) * Tq, ptr(dk), ptr(dv),
                                   dk.stride(0), dk.stride(0) * Tk, N, heads, head_dim, Tq, Tk, int(causal), ptr(key_lengths),
                                   drop.p, drop.seed, stream_id, drop.offset, drop.counter_ptr, _stream()), 'halo_attention_bwd')


def attention_masked(q, k, v, mask):
    """ha/transformer.py:413-430 attend for any boolean mask (True = hidden; broadcastable to (N, heads, T, S)) and any head dimension:
    q (N, heads, T, hd), k / v (N, heads, S, hd) -> (y like q, entropy [N, heads, T]).  The slow general path (halo_attention_masked)."""
    N, H, T, hd = q.shape
    S = k.shape[-2]
    qc, kc, vc = (t.float().contiguous() for t in (q, k, v))
    y = torch.empty_like(qc)
    ent = torch.empty(N, H, T, device=q.device, dtype=torch.float32)
    m8, sn, sh, st = None, 0, 0, 0
    if mask is not None:
        m8 = torch.broadcast_to(mask.to(torch.uint8), (N, H, T, S))
        if m8.stride(3) not in (1, 0) or (m8.stride(3) == 0 and S > 1):
            m8 = m8.contiguous()
        sn, sh, st = m8.stride(0), m8.stride(1), m8.stride(2)
    check(lib().halo_attention_masked(ptr(qc), ptr(kc), ptr(vc), ptr(m8), sn, sh, st, ptr(y), ptr(ent), N, H, T, S, hd, _stream()),
          'halo_attention_masked')
    return y, ent


def attention_fwd_bf16(q, k, v, N, heads, head_dim, Tq, Tk, causal=False, key_lengths=None, drop=NO_DROPOUT, stream_id=0):
    """attention_fwd (training: with lse) that also returns y as row-major bf16 -> (y, lse, y_bf16)."""
    C = heads * head_dim
    dev = q.device
    y = torch.empty(N * Tq, C, device=dev, dtype=torch.float32)
    yb = torch.empty(N * Tq, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(N, heads, Tq, device=dev, dtype=torch.float32)
    if key_lengths is not None:
        key_lengths = key_lengths.to(device=dev, dtype=torch.int32).contiguous()
    check(lib().halo_attention_fwd_bf16(ptr(q), q.stride(0), q.stride(0) * Tq, ptr(k), ptr(v), k.stride(0), k.stride(0) * Tk, ptr(y), C,
                                        C * Tq, ptr(yb), C, C * Tq, ptr(lse), N, heads, head_dim, Tq, Tk, int(causal), ptr(key_lengths),
                                        drop.p, drop.seed, stream_id, drop.offset, drop.counter_ptr, _stream()), 'halo_attention_fwd_bf16')
    return y, lse, yb


def attention_fwd_b16(q, k, v, N, heads, head_dim, Tq, Tk, causal=False, want_y=False, want_lse=False):
    """Attention forward from row-major bf16 q / k / v views [N * T, heads * head_dim] (halo_attention_fwd_b16: bf16 arithmetic, head_dim 64)
    -> (y fp32 or None, lse or None, y as row-major bf16)."""
    C = heads * head_dim
    dev = q.device
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
        raise ValueError('attention_fwd_b16: bf16 q, k, v')
    y = torch.empty(N * Tq, C, device=dev, dtype=torch.float32) if want_y else None
    yb = torch.empty(N * Tq, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(N, heads, Tq, device=dev, dtype=torch.float32) if want_lse else None
    check(lib().halo_attention_fwd_b16(ptr(q), q.stride(0), q.stride(0) * Tq, ptr(k), ptr(v), k.stride(0), k.stride(0) * Tk, ptr(y), C, C * Tq,
                                       ptr(yb), C, C * Tq, ptr(lse), N, heads, head_dim, Tq, Tk, int(causal), _stream()), 'halo_attention_fwd_b16')
    return y, lse, yb


def attention_bwd_b16(q, k, v, yb, dyb, lse, dq, dk, dv, N, heads, head_dim, Tq, Tk, causal=False):
    """Backward of attention_fwd_b16: every operand row-major bf16 (q, k, v views of the c_attn rows; yb the forward's bf16 output; dyb the
    output gradient), dq / dk / dv bf16 views written in place."""
    for t in (q, k, v, yb, dyb, dq, dk, dv):
        if t.dtype != torch.bfloat16:
            raise ValueError('attention_bwd_b16: bf16 operands')
    delta = torch.empty(N * heads * Tq, device=q.device, dtype=torch.float32)
    check(lib().halo_attention_bwd_b16(ptr(q), q.stride(0), q.stride(0) * Tq, ptr(k), ptr(v), k.stride(0), k.stride(0) * Tk, ptr(yb), ptr(dyb),
                                       yb.stride(0), yb.stride(0) * Tq, ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), dq.stride(0),
                                       dq.stride(0) * Tq, N, heads, head_dim, Tq, Tk, int(causal), _stream()), 'halo_attention_bwd_b16')


def attention_bwd_bf16(q, k, v, y, dy, lse, dq, dk, dv, N, heads, head_dim, Tq, Tk, causal=False, key_lengths=None, drop=NO_DROPOUT,
                       stream_id=0):
    """attention_bwd with dq / dk / dv bf16 views of one row stride (the column blocks of a packed [rows, 3C] bf16 buffer)."""
    C = heads * head_dim
    _f32c(y, 'y'); _f32c(dy, 'dy')
    if not (dq.dtype == dk.dtype == dv.dtype == torch.bfloat16) or not (dq.stride(0) == dk.stride(0) == dv.stride(0)) or Tq != Tk:
        raise ValueError('attention_bwd_bf16: bf16 dq / dk / dv with one row stride (self-attention)')
    delta = torch.empty(N, heads, Tq, device=q.device, dtype=torch.float32)
    check(lib().halo_attention_bwd_bf16(ptr(q), q.stride(0), q.stride(0) * Tq, ptr(k), ptr(v), k.stride(0), k.stride(0) * Tk, ptr(y), ptr(dy),
                                        C, C * Tq, ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), dq.stride(0), dq.stride(0) * Tq, N, heads,
                                        head_dim, Tq, Tk, int(causal), ptr(key_lengths), drop.p, drop.seed, stream_id, drop.offset,
                                        drop.counter_ptr, _stream()), 'halo_attention_bwd_bf16')


def layernorm_bwd(dy, x2d, weight, dres=None, has_bias=False, eps=1e-5, want_bf16=False):
    """-> (dx = dres + dLN, dweight, dbias or None[, dx as row-major bf16 with ``want_bf16``]).  dy: fp32, or row-major bf16 (the
    input-gradient product's bf16 result)."""
    _f32c(x2d, 'x')
    rows, C = x2d.shape
    if dy.dtype == torch.bfloat16:
        dev = x2d.device
        dx = torch.empty_like(x2d)
        dw = torch.empty(C, device=dev, dtype=torch.float32)
        db = torch.empty(C, device=dev, dtype=torch.float32) if has_bias else None
        ws = torch.empty(lib().halo_layernorm_bwd_workspace_bytes(rows, C), device=dev, dtype=torch.uint8)
        dxb = torch.empty(rows, C, device=dev, dtype=torch.bfloat16) if want_bf16 else None
        check(lib().halo_layernorm_bwd_b16(ptr(dy), ptr(x2d), ptr(weight), ptr(dres), ptr(dx), ptr(dxb), ptr(dw), ptr(db), ptr(ws), rows, C,
                                           eps, _stream()), 'halo_layernorm_bwd_b16')
        return (dx, dw, db, dxb) if want_bf16 else (dx, dw, db)
    _f32c(dy, 'dy')
    dev = x2d.device
    dx = torch.empty_like(x2d)
    dw = torch.empty(C, device=dev, dtype=torch.float32)
    db = torch.empty(C, device=dev, dtype=torch.float32) if has_bias else None
    ws = torch.empty(lib().halo_layernorm_bwd_workspace_bytes(rows, C), device=dev, dtype=torch.uint8)
    if want_bf16:
        dxb = torch.empty(rows, C, device=dev, dtype=torch.bfloat16)
        check(lib().halo_layernorm_bwd_bf16(ptr(dy), ptr(x2d), ptr(weight), ptr(dres), ptr(dx), ptr(dxb), ptr(dw), ptr(db), ptr(ws), rows, C,
                                            eps, _stream()), 'halo_layernorm_bwd_bf16')
        return dx, dw, db, dxb
    check(lib().halo_layernorm_bwd(ptr(dy), ptr(x2d), ptr(weight), ptr(dres), ptr(dx), ptr(dw), ptr(db), ptr(ws), rows, C, eps,
                                   _stream()), 'halo_layernorm_bwd')
    return dx, dw, db


def gelu_fwd(a, exact=False):
    _f32c(a, 'a')
    y = torch.empty_like(a)
    check(lib().halo_gelu_fwd(ptr(a), ptr(y), a.numel(), int(exact), _stream()), 'halo_gelu_fwd')
    return y


def gelu_bwd(dy, a, exact=False, out=None):
    _f32c(dy, 'dy'); _f32c(a, 'a')
    da = out if out is not None else torch.empty_like(a)
    check(lib().halo_gelu_bwd(ptr(dy), ptr(a), ptr(da), a.numel(), int(exact), _stream()), 'halo_gelu_bwd')
    return da


def cross_entropy_fwd_lse(logits2d, targets, ignore_index=0):
    _f32c(logits2d, 'logits')
    tg = _i64c(targets.reshape(-1), 'targets')
    rows, V = logits2d.shape
    loss = torch.empty(rows, device=logits2d.device, dtype=torch.float32)
    lse = torch.empty(rows, device=logits2d.device, dtype=torch.float32)
    check(lib().halo_cross_entropy_fwd_lse(ptr(logits2d), ptr(tg), ptr(loss), ptr(lse), rows, V, V, ignore_index, _stream()),
          'halo_cross_entropy_fwd_lse')
    return loss, lse


def cross_entropy_bwd_(logits2d, targets, lse, grad_rows, ignore_index=0):
    """logits2d <- d loss / d logits in place; grad_rows [rows] (or a 1-element tensor broadcast to all rows)."""
    _f32c(logits2d, 'logits'); _f32c(grad_rows, 'grad')
    tg = _i64c(targets.reshape(-1), 'targets')
    rows, V = logits2d.shape
    stride = 0 if grad_rows.numel() == 1 else 1
    check(lib().halo_cross_entropy_bwd(ptr(logits2d), ptr(tg), ptr(lse), ptr(grad_rows), stride, rows, V, V, ignore_index, _stream()),
          'halo_cross_entropy_bwd')
    return logits2d


def cross_entropy_bwd_images(logits2d, targets, lse, grad_rows, ignore_index=0):
    """d loss / d logits (as cross_entropy_bwd_ computes it) written as the two split images the lm_head's backward
    products read -- (image of [rows][V], image of [V][rows]) -- without materialising it in fp32; logits2d is not modified."""
    _f32c(logits2d, 'logits'); _f32c(grad_rows, 'grad')
    tg = _i64c(targets.reshape(-1), 'targets')
    rows, V = logits2d.shape
    stride = 0 if grad_rows.numel() == 1 else 1
    rm = torch.empty(lib().halo_split_image_bytes(rows, V), device=logits2d.device, dtype=torch.uint8)
    tr = torch.empty(lib().halo_split_image_bytes(V, rows), device=logits2d.device, dtype=torch.uint8)
    check(lib().halo_cross_entropy_bwd_images(ptr(logits2d), ptr(tg), ptr(lse), ptr(grad_rows), stride, rows, V, V, ignore_index,
                                              ptr(rm), ptr(tr), _stream()), 'halo_cross_entropy_bwd_images')
    return rm, tr


def embed_bwd(ids, dx2d, dwte, dwpe, pos0=0, accumulate_wpe=False):
    ids = _i64c(ids, 'input_ids')
    Bn, T = ids.shape
    vocab = dwte.shape[0] if dwte is not None else 1
    check(lib().halo_embed_bwd(ptr(ids), ptr(dx2d), ptr(dwte), ptr(dwpe), Bn, T, dx2d.shape[1], pos0, vocab,
                               int(accumulate_wpe), _stream()), 'halo_embed_bwd')


def embed_bwd_ordered(ids, dx2d, vocab):
    """ids (any shape, n tokens), dx2d [n, C] f32 -> dwte [vocab, C]: the scatter-add of embed_bwd in token order, no atomics."""
    ids = _i64c(ids, 'input_ids')
    _f32c(dx2d, 'dx')
    dwte = torch.empty(vocab, dx2d.shape[1], device=dx2d.device, dtype=torch.float32)
    check(lib().halo_embed_bwd_ordered(ptr(ids), ptr(dx2d), ptr(dwte), ids.numel(), dx2d.shape[1], vocab, _stream()), 'halo_embed_bwd_ordered')
    return dwte


def dwconv1d_cl_bwd(dy3d, x3d, weight, stride, pad, want_dx=True, has_bias=True):
    """-> (dx or None, dweight [C, ks], dbias or None)"""
    _f32c(dy3d, 'dy'); _f32c(x3d, 'x')
    N, T, Cn = x3d.shape
    ks = weight.shape[-1]
    dev = x3d.device
    dx = torch.empty_like(x3d) if want_dx else None
    dw = torch.empty(Cn, ks, device=dev, dtype=torch.float32)
    db = torch.empty(Cn, device=dev, dtype=torch.float32) if has_bias else None
    ws = torch.empty(lib().halo_dwconv1d_cl_bwd_workspace_bytes(Cn, ks), device=dev, dtype=torch.uint8)
    check(lib().halo_dwconv1d_cl_bwd(ptr(dy3d), ptr(x3d), ptr(weight), ptr(dx), ptr(dw), ptr(db), ptr(ws), N, T, Cn, ks, stride, pad,
                                     _stream()), 'halo_dwconv1d_cl_bwd')
    return dx, dw, db


def add_rows_bcast_(x2d, p2d, T):
    """x2d[n] += p2d[n % T] in place."""
    _f32c(x2d, 'x'); _f32c(p2d, 'p')
    check(lib().halo_add_rows_bcast(ptr(x2d), ptr(p2d), x2d.shape[0], T, x2d.shape[1], _stream()), 'halo_add_rows_bcast')
    return x2d


# ---- the masked objectives: token masking, and the compaction of the rows that carry a target (csrc/sparse_head.hip) ----------------
def mask_tokens_(inputs, mlm_probability, mask_token, endoftext_token, max_token, seed, step=0):
    """inputs [..] int64, masked in place as include/halo.h defines the draws -> labels (same shape)."""
    if inputs.dtype != torch.int64 or not inputs.is_cuda or not inputs.is_contiguous():
        raise ValueError('mask_tokens_: expected a contiguous int64 HIP tensor')
    labels = torch.empty_like(inputs)
    check(lib().halo_mask_tokens(ptr(inputs), ptr(labels), inputs.numel(), mlm_probability, mask_token, endoftext_token, max_token,
                                 seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, _stream()), 'halo_mask_tokens')
    return labels


TargetRows = namedtuple('TargetRows', 'rows targets slot count capacity limit')


def target_rows(targets, capacity, ignore_index=0, limit=None):
    """targets [M] int64 -> TargetRows: ``rows`` [capacity] int32 (the first ``limit`` rows whose target is not ignore_index, ascending,
    -1 behind them), ``targets`` [capacity] int64 (theirs, ignore_index behind them), ``slot`` [M] int32 (the inverse map, -1 where
    a row has no place), ``count`` [1] int32 (every row with a target; more than ``limit``: overflow).  ``limit`` (default: capacity)
    is the number of targets allowed for, ``capacity`` >= limit the number of compact rows.  Nothing returns to the host."""
    tg = _i64c(targets.reshape(-1), 'targets')
    M, dev = tg.numel(), tg.device
    limit = capacity if limit is None else limit
    rows = torch.empty(capacity, device=dev, dtype=torch.int32)
    tc = torch.empty(capacity, device=dev, dtype=torch.int64)
    slot = torch.empty(M, device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    check(lib().halo_target_rows(ptr(tg), M, ignore_index, capacity, limit, ptr(rows), ptr(tc), ptr(slot), ptr(count), _stream()),
          'halo_target_rows')
    return TargetRows(rows, tc, slot, count, capacity, limit)


def gather_rows(src, rows):
    """src [M, C] (or [M]) fp32 -> [K, C] (or [K]): src[rows[k]], zeros where rows[k] < 0."""
    _f32c(src, 'src')
    K = rows.numel()
    dst = torch.empty((K,) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32)
    check(lib().halo_gather_rows(ptr(src), ptr(rows), src.shape[0], K, src[0].numel(), ptr(dst), _stream()), 'halo_gather_rows')
    return dst


def scatter_rows(src, tr, M, want_bf16=False, nan_on_overflow=True):
    """src [capacity, C] (or [capacity]) fp32 -> dst [M, C] (or [M]) with dst[i] = src[tr.slot[i]], zeros where a row has no slot: every
    row is written.  ``nan_on_overflow``: all NaN when tr.count > tr.limit.  ``want_bf16``: -> (dst, dst as row-major bf16)."""
    _f32c(src, 'src')
    if src.shape[0] != tr.capacity or tr.slot.numel() != M:
        raise ValueError('scatter_rows: src must hold tr.capacity rows and tr.slot M entries')
    dst = torch.empty((M,) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32)
    dstb = torch.empty_like(dst, dtype=torch.bfloat16) if want_bf16 else None
    check(lib().halo_scatter_rows(ptr(src), ptr(tr.slot), ptr(tr.count) if nan_on_overflow else None, tr.capacity, tr.limit, M, src[0].numel(),
                                  ptr(dst),
                                  ptr(dstb), _stream()), 'halo_scatter_rows')
    return (dst, dstb) if want_bf16 else dst
