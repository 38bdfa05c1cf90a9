"""Yardstick of the star-CTC and transducer lattices (haloop_amd.star / haloop_amd.transducer, csrc/lattice.hip) at sizes the
state-by-state oracle (oracle/star_ref.py) cannot reach: the same recursions, vectorised, in a chosen precision.

``dtype='float64'`` is the reference value; ``dtype='float32'`` runs the SAME statements with every intermediate in float32, so
max|ref(float32) - ref(float64)| says what fp32 arithmetic itself loses on a case (the tolerance of tests/test_gpu_lattice_f64.py).

star-CTC (ha/star.py:65-166, the header of csrc/lattice.hip): 4S+3 states  blank <star\\a> blank a ... blank <star> blank; into state i
    blank  i-1, i        star  i-1, i, i+1, plus the penalty        label  i-3, i-1, i-2, and i-4 unless both labels are equal
four virtual states before state 0 (0 at frame 0, finfo(float32).min afterwards), -7007.7007 past the last state, "log 0" =
finfo(float32).min, <star\\s> = cs + log1p(-exp(lp[s] - cs)) with cs = logsumexp(lp[1:]).  The recursion is walked per utterance over
the states of one frame at a time (numpy); it stops at frame emission_lengths[n], the only frame the read-out looks at.  The
gradient is the explicit alpha-beta one: autograd through log1p(-exp(0)) (C = 2, where every <star\\s> is log 0) gives 0 * inf.

transducer (ha/transducer.py:175-207): tests/rnnt_loss_ref.py's cell-by-cell lattice with torch autograd, handed the blank and label
log-probability of every cell as a K = 2 joint so that one cell's backward touches [T, U+1, 2] numbers and not [T, U+1, K].
CPU only."""
import numpy as np
import torch

import rnnt_loss_ref

VOID = float(np.finfo(np.float32).min)
TOOT = -7007.7007


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    safe = np.where(np.isfinite(m), m, 0).astype(x.dtype)
    return (np.log(np.exp(x - safe).sum(axis=axis, keepdims=True, dtype=x.dtype)) + safe).squeeze(axis)


def star_ctc(lp, targets, em_len, tg_len, penalty=-0.5, dtype='float64'):
    """lp [T, N, C] log-probabilities, targets [N, S], lengths [N] -> (losses [N], grad [T, N, C] = d sum(losses) / d lp), both of
    ``dtype``; grad is zero for frames >= em_len[n]."""
    dt = np.dtype(dtype)
    lp, targets, em_len, tg_len = _np(lp).astype(dt), _np(targets).astype(np.int64), _np(em_len), _np(tg_len)
    T, N, C = lp.shape
    S = targets.shape[1]
    S_ = 4 * S + 3
    pen, void, toot = dt.type(penalty), dt.type(VOID), dt.type(TOOT)
    idx = np.arange(S_)
    blank, star, label = idx % 2 == 0, idx % 4 == 1, idx % 4 == 3
    losses, grad = np.zeros(N, dt), np.zeros((T, N, C), dt)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        for n in range(N):
            Tn, s_last = int(em_len[n]), 4 * int(tg_len[n]) + 2
            tg, x = targets[n], lp[:Tn, n]                                  # x [Tn, C]
            # symbol of every state (stars: the label they exclude, 0 = the complete star) and the emissions em[t, i]
            sym = np.zeros(S_, np.int64)
            sym[3::4] = tg
            sym[1:4 * S:4] = tg
            cs = _lse(x[:, 1:], 1)                                          # [Tn]
            se = np.where(sym[None, star] == 0, cs[:, None], cs[:, None] + np.log1p(-np.exp(x[:, sym[star]] - cs[:, None])))   # [Tn, S+1]
            em = x[:, sym]
            em[:, star] = se
            same = np.zeros(S_, bool)
            same[7::4] = tg[1:] == tg[:-1]
            # alpha[t - 1]: after frame t (1-based)
            alpha = np.empty((Tn, S_), dt)
            P = np.concatenate([np.zeros(4, dt), np.full(S_, void), [toot]])   # four virtual states | the real ones | past the end
            for t in range(Tn):
                m4, m3, m2, m1, a0, p1 = P[0:S_], P[1:S_ + 1], P[2:S_ + 2], P[3:S_ + 3], P[4:S_ + 4], P[5:S_ + 5]
                near = np.logaddexp(m1, a0)
                lab = np.logaddexp(np.logaddexp(m3, m1), m2)
                tr = np.where(blank, near, np.where(star, np.logaddexp(near, p1) + pen, np.where(same, lab, np.logaddexp(lab, m4))))
                alpha[t] = tr + em[t]
                P = np.concatenate([np.full(4, void), alpha[t], [toot]])
            # read-out: states s_last-3 .. s_last; index -1 (an empty target) is the last virtual state
            z = P[4 + s_last]
            for d in (1, 2, 3):
                z = np.logaddexp(z, P[4 + s_last - d])
            losses[n] = -z
            # beta sweep; occ[t, i] = posterior of state i at frame t + 1
            beta = np.full(S_, -np.inf, dt)
            beta[max(s_last - 3, 0):s_last + 1] = 0
            occ = np.empty((Tn, S_), dt)
            into = np.where(star, pen, dt.type(0))                          # the penalty rides on every transition into a star
            ninf = np.full(S_, -np.inf, dt)
            for t in range(Tn - 1, -1, -1):
                occ[t] = np.where(beta == -np.inf, 0, np.exp(alpha[t] + beta - z))
                e = np.concatenate([em[t] + beta + into, np.full(4, -np.inf, dt), [-np.inf]])   # e[-1] = e[S_ + 4] = -inf for j - 1 = -1
                j = idx
                beta = np.logaddexp.reduce(np.stack([
                    np.where(~label, e[j], ninf),                           # j -> j        (blank, star)
                    e[j + 1],                                               # j -> j + 1
                    np.where(j % 4 == 2, e[j - 1], ninf),                   # the blank after a star -> that star
                    np.where(star, e[j + 2], ninf),                         # star -> its label
                    np.where(j % 4 == 0, e[j + 3], ninf),                   # the blank before a star -> the label
                    np.where(label & ~np.concatenate([same[4:], np.ones(4, bool)]), e[j + 4], ninf),   # label -> the next, unless equal
                ]), axis=0)
            # occupancies -> symbols: blanks and labels directly; a star spreads over the symbols it sums,
            # d <star\s> / d lp[k] = exp(lp[k] - <star\s>) for k >= 1, k != s
            g = np.zeros((Tn, C), dt)
            g[:, 0] = occ[:, blank].sum(1, dtype=dt)
            for k in range(S):
                g[:, tg[k]] += occ[:, 4 * k + 3]
            o = occ[:, star]                                                # [Tn, S+1]
            w = np.exp(x[:, None, 1:] - np.where(o != 0, se, 0)[:, :, None])                  # [Tn, S+1, C-1]
            w = np.where((o != 0)[:, :, None] & (sym[star][None, :, None] != np.arange(1, C)[None, None, :]), w, 0)
            g[:, 1:] += (o[:, :, None] * w).sum(1, dtype=dt)
            grad[:Tn, n] = -g
    return losses, grad


def _transducer_compact(lp, targets, j_len, t_len):
    """lp [N, T, U+1, K] (torch, any float dtype, may require grad) -> losses [N] through rnnt_loss_ref.lattice_losses on the K = 2
    joint (blank, the cell's label), one utterance at a time over the cells inside its lengths."""
    N, T, U1, K = lp.shape
    y = torch.cat([targets.long(), targets.new_zeros((N, 1), dtype=torch.long)], 1)             # [N, U+1]; the last row has no label
    lp2 = torch.stack([lp[..., 0], lp.gather(3, y[:, None, :, None].expand(N, T, U1, 1))[..., 0]], -1)
    ones = torch.ones(1, max(U1 - 1, 1), dtype=torch.long)
    out = []
    for n in range(N):
        Tn, Un = int(j_len[n]), int(t_len[n])
        out.append(rnnt_loss_ref.lattice_losses(lp2[n:n + 1, :Tn, :Un + 1], ones, [Tn], [Un])[0])
    return torch.stack(out)


def transducer(joint, targets, j_len, t_len, dtype='float64', weights=None):
    """joint [N, T, U+1, K] log-probabilities, targets [N, U] -> (losses [N], grad [N, T, U+1, K] = d sum(losses * weights) / d joint)
    as torch tensors of ``dtype`` (weights default to ones)."""
    dt = getattr(torch, dtype)
    lp = joint.detach().cpu().to(dt).requires_grad_(True)
    losses = _transducer_compact(lp, targets.cpu(), j_len, t_len)
    w = torch.ones_like(losses) if weights is None else weights.detach().cpu().to(dt)
    (losses * w).sum().backward()
    return losses.detach(), lp.grad


def transducer_additive(f, g, targets, f_len, t_len, dtype='float64', weights=None):
    """rnnt_loss_ref.transducer_loss_ref's quantity, (f[:, :, None] + g[:, None]).log_softmax(-1) into the lattice, in ``dtype`` and
    at lattice sizes its dense cell-by-cell backward is too slow for -> (losses [N], df [N, T, V], dg [N, U+1, V])."""
    dt = getattr(torch, dtype)
    fd, gd = f.detach().cpu().to(dt).requires_grad_(True), g.detach().cpu().to(dt).requires_grad_(True)
    lp = (fd[:, :, None, :] + gd[:, None, :, :]).log_softmax(-1)
    losses = _transducer_compact(lp, targets.cpu(), f_len, t_len)
    w = torch.ones_like(losses) if weights is None else weights.detach().cpu().to(dt)
    (losses * w).sum().backward()
    return losses.detach(), fd.grad, gd.grad
