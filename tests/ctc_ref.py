"""Plain-numpy yardstick for the CTC loss (csrc/ctc.hip) and the fused CTC head (csrc/head.hip): float64 by default, the same code
in float32 when ``dtype='float32'`` (that run measures what fp32 arithmetic itself loses on a case).  No torch autograd here: the
gradients are written out, so tests/test_ctc_ref_cpu.py can hold this file to float64 torch autograd as an independent statement.

ctc     alpha-beta over the extended labels (blank 0, the skip rule of F.ctc_loss), gradient in ATen's convention
head    dropout mask -> Linear -> log_softmax -> CTC -> mean(nll / max(tl, 1)) and the backward of that chain
greedy  per-frame arg max (lowest index on ties), repeats collapsed, blanks dropped
"""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------- CTC
def _lse_rows(x, axis):
    """log-sum-exp along ``axis``; an all -inf slice gives -inf."""
    m = x.max(axis=axis, keepdims=True)
    safe = np.where(np.isfinite(m), m, 0).astype(x.dtype)
    with np.errstate(divide='ignore'):
        out = np.log(np.exp(x - safe).sum(axis=axis, keepdims=True, dtype=x.dtype)) + safe
    return np.squeeze(out, axis=axis).astype(x.dtype)


def ctc(lp, targets, il, tl, dtype='float64'):
    """lp [N,T,C] log-probabilities, targets [N,S] (padded), il / tl [N] -> (nll [N], dlp [N,T,C]) in ``dtype``.

    alpha[0, 0] = lp[0, blank], alpha[0, 1] = lp[0, l1]; alpha[t, s] = lp[t, ext[s]] + log(e^alpha[t-1, s] + e^alpha[t-1, s-1] +
    [ext[s] != blank and ext[s] != ext[s-2]] e^alpha[t-1, s-2]); nll = -log(e^alpha[il-1, 2 tl] + e^alpha[il-1, 2 tl - 1]); beta the
    mirror image from frame il - 1.  The gradient is ATen's: exp(lp[t, c]) - exp(logsum_{s: ext[s] = c}(alpha + beta)[t, s] + nll - lp[t, c])
    for grad_out = 1 (the true derivative after a log_softmax; alpha and beta both hold frame t's emission, hence the - lp).  Rows at
    and beyond il are zero; il = 0 gives nll = 0 for an empty target and +inf otherwise; an infeasible row has nll = +inf and a NaN
    gradient row (nothing is promised there); where lp = -inf the occupancy is taken as 0 (the gradient is then exp(-inf) - 0 = 0)."""
    dt = np.dtype(dtype)
    lp = np.asarray(lp).astype(dt)
    targets, il, tl = (np.asarray(a).astype(np.int64) for a in (targets, il, tl))
    N, T, C = lp.shape
    nll = np.zeros(N, dtype=dt)
    dlp = np.zeros((N, T, C), dtype=dt)
    ninf = dt.type(-np.inf)
    for n in range(N):
        Tn, Sn = int(min(max(il[n], 0), T)), int(min(max(tl[n], 0), targets.shape[1]))
        if Tn == 0:
            nll[n] = 0.0 if Sn == 0 else np.inf
            continue
        ext = np.zeros(2 * Sn + 1, dtype=np.int64)
        ext[1::2] = targets[n, :Sn]
        L = ext.size
        skip = np.zeros(L, dtype=bool)
        skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
        em = lp[n, :Tn][:, ext]                                              # [Tn, L] emissions of the states
        alpha = np.full((Tn, L), ninf, dtype=dt)
        alpha[0, :2] = em[0, :2]
        for t in range(1, Tn):
            p = alpha[t - 1]
            acc = p.copy()
            acc[1:] = np.logaddexp(acc[1:], p[:-1])
            acc[2:] = np.where(skip[2:], np.logaddexp(acc[2:], p[:-2]), acc[2:])
            alpha[t] = acc + em[t]
        beta = np.full((Tn, L), ninf, dtype=dt)
        beta[Tn - 1, max(L - 2, 0):] = em[Tn - 1, max(L - 2, 0):]
        for t in range(Tn - 2, -1, -1):
            q = beta[t + 1]
            acc = q.copy()
            acc[:-1] = np.logaddexp(acc[:-1], q[1:])
            acc[:-2] = np.where(skip[2:], np.logaddexp(acc[:-2], q[2:]), acc[:-2])
            beta[t] = acc + em[t]
        ll = np.logaddexp(alpha[Tn - 1, L - 1], alpha[Tn - 1, L - 2]) if L > 1 else alpha[Tn - 1, 0]
        nll[n] = -ll
        if not np.isfinite(ll):
            nll[n] = np.inf
            dlp[n, :Tn] = np.nan
            continue
        ab = alpha + beta
        lcab = np.full((Tn, C), ninf, dtype=dt)
        for c in np.unique(ext):
            lcab[:, c] = _lse_rows(ab[:, ext == c], axis=1)
        row = lp[n, :Tn]
        with np.errstate(invalid='ignore'):
            occ = np.where(np.isfinite(row), np.exp(lcab + nll[n] - row), 0)
        dlp[n, :Tn] = np.exp(row) - occ.astype(dt)
    return nll, dlp


# --------------------------------------------------------------------------------------------------------------------- head
def feature_lengths(il, T, ks=5, stride=4, pad=3):
    """The reference's rule (ha/rnn.py:13-18; halo_ctc_prepare, feature_length() in csrc/ctc_head_dev.h): floor((il + 2 pad - ks) / stride + 1)
    in float32 arithmetic, clamped to [0, T]."""
    o = (np.asarray(il).astype(np.int64) + 2 * pad - ks).astype(np.float32)
    f = np.floor(o / np.float32(stride) + np.float32(1.0)).astype(np.int64)
    return np.clip(f, 0, T)


def bf16_round(x32):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32: what the (__bf16) casts of split8() do."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    r = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def _split(x, dt):
    """split8() of csrc/dev_util.h: the operand as fp32, hi = bf16(x), lo = bf16(x - hi) (the difference is exact in fp32)."""
    x32 = np.asarray(x).astype(np.float32)
    hi = bf16_round(x32)
    lo = bf16_round(x32 - hi)
    return hi.astype(dt), lo.astype(dt)


def _product(a, b, split, dt):
    """a [.., M, K] @ b [K, N] in ``dt`` with the operands as the math mode rounds them."""
    if split is None:
        return np.matmul(a.astype(dt), b.astype(dt))
    if split != 'bf16x3':
        raise ValueError(f'unknown operand model {split!r}')
    ah, al = _split(a, dt)
    bh, bl = _split(b, dt)
    return np.matmul(ah, bl) + np.matmul(al, bh) + np.matmul(ah, bh)


def head(feats, W, b, mask, il, targets, tl, ks=5, stride=4, pad=3, dtype='float64', split=None):
    """feats [B,T,H], W [V,H], b [V], mask [B,T,H] of 0 / 1/(1-p) multipliers or None, il [B] INPUT lengths (before the convolution),
    targets [B,S], tl [B] -> dict(flen, lp, nll, loss, dW, db, dfeats).

        x = feats * mask;  logits = x W^T + b;  lp = log_softmax(logits);  (nll, g) = ctc(lp, targets, flen, tl)
        loss = mean(nll / max(tl, 1));  g *= 1 / (max(tl, 1) B);  dlogit = g - exp(lp) sum_c g
        dfeats = (dlogit W) * mask;  dW = sum_n dlogit^T x;  db = sum_{n,t} dlogit

    ``split`` is the rounding the kernels apply to the operands of the three products (logits, dfeats, dW):

    None       exact: ctc_head_fwd_kernel / ctc_head_bwd_kernel (the 'f32' math mode) multiply fp32 operands on the exact-f32 MFMA
               (v_mfma_f32_32x32x2f32, head.hip:97, 283, 307); x = feats * mask is an fp32 product (head.hip:88, 300).
    'bf16x3'   every operand is taken as fp32 and split into hi = bf16(v), lo = bf16(v - hi); a product is hi*lo + lo*hi + hi*hi with
               the lo*lo term left out, accumulated in fp32.  ctc_head_train_kernel does this for the logits (split8 of the fp32
               product feats * mask and of W, three MFMAs: head.hip:433-441) and for both backward products (split8 of dlogit and of
               W, respectively of x = feats * scale where kept: head.hip:652-665; the dfeats tile is multiplied by the mask on the
               way out, head.hip:671), and ctc_head_greedy2_kernel does it for the logits (ctc_head_dev.h:84-96).  halo_ctc_head_train
               and halo_ctc_head_greedy branch only on 'f32' against the rest (head.hip:794, 847): the 'bf16' math mode runs the
               SAME three-term split as 'bf16x3' in these kernels, so both modes are modelled by split='bf16x3'.
    Everything else (bias, log_softmax, lattice, dlogit, the sums over utterances) is fp32 arithmetic in the kernels and ``dtype``
    arithmetic here."""
    dt = np.dtype(dtype)
    feats, W, b = (np.asarray(a).astype(dt) for a in (feats, W, b))
    B, T, H = feats.shape
    V = W.shape[0]
    tl = np.asarray(tl).astype(np.int64)
    flen = feature_lengths(il, T, ks, stride, pad)
    m = None if mask is None else np.asarray(mask).astype(dt).reshape(B, T, H)
    x = feats if m is None else feats * m
    logits = _product(x.reshape(B * T, H), W.T, split, dt) + b
    mx = logits.max(axis=1, keepdims=True)
    lp = (logits - mx - np.log(np.exp(logits - mx).sum(axis=1, keepdims=True, dtype=dt))).astype(dt).reshape(B, T, V)
    nll, g = ctc(lp, targets, flen, tl, dt)
    denom = np.maximum(tl, 1).astype(dt)
    loss = (nll / denom).mean(dtype=dt)
    g = g * (1.0 / (denom * B)).astype(dt)[:, None, None]
    dl = (g - np.exp(lp) * g.sum(axis=2, keepdims=True, dtype=dt)).astype(dt)
    dfeats = _product(dl.reshape(B * T, V), W, split, dt).reshape(B, T, H)
    if m is not None:
        dfeats = dfeats * m
    dW = _product(dl.transpose(0, 2, 1), x, split, dt).sum(axis=0, dtype=dt)
    db = dl.sum(axis=(0, 1), dtype=dt)
    return dict(flen=flen, lp=lp, nll=nll, loss=loss, dW=dW.astype(dt), db=db.astype(dt), dfeats=dfeats.astype(dt))


# ------------------------------------------------------------------------------------------------------------------- greedy
def greedy(lp):
    """lp [N,T,C] -> (alignments [N,T] int64, scores [N,T], hyp: list of N lists, hyp_len [N] int64)."""
    lp = np.asarray(lp)
    ali = lp.argmax(axis=2).astype(np.int64)                                # numpy's argmax takes the first maximum
    scores = np.take_along_axis(lp, ali[:, :, None], axis=2)[:, :, 0]
    hyp = []
    for row in ali:
        out, prev = [], -1
        for sym in row.tolist():
            if sym != prev and sym != 0:
                out.append(sym)
            prev = sym
        hyp.append(out)
    return ali, scores, hyp, np.array([len(h) for h in hyp], dtype=np.int64)


def top_two_margin(lp):
    """Per utterance the smallest gap between the best and the second-best class over its frames ([N]; inf for one class)."""
    lp = np.asarray(lp, dtype=np.float64)
    if lp.shape[2] < 2:
        return np.full(lp.shape[0], np.inf)
    part = np.sort(lp, axis=2)
    return (part[:, :, -1] - part[:, :, -2]).min(axis=1)
