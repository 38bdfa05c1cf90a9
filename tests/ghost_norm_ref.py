"""CPU statements of what csrc/ghost_norm.hip computes, for the tests: the direct form in float64 (the gradient itself, then its squared
norm) and the Gram form the kernel evaluates, in any dtype.  Operands are torch CPU tensors, batch-first [N, T, K]."""
import torch


def direct_sqnorm64(a, bs=(), n_bias=0):
    """sum_j ||sum_t a_t b^j_t^T||_F^2 + n_bias ||sum_t a_t||^2 per utterance, formed the obvious way in float64 -> [N]."""
    a = a.double()
    out = n_bias * a.sum(dim=1).square().sum(dim=1)
    for b in bs:
        out = out + torch.einsum('ntk,ntj->nkj', a, b.double()).square().sum(dim=(1, 2))
    return out


def grams(a, bs=(), n_bias=0, dtype=torch.float32):
    """(G_a, n_bias + sum_j G_b^j), both [N, T, T], evaluated in ``dtype``."""
    a = a.to(dtype)
    ga = a @ a.mT
    gb = torch.full_like(ga, float(n_bias))
    for b in bs:
        b = b.to(dtype)
        gb = gb + b @ b.mT
    return ga, gb


def gram_sqnorm(a, bs=(), n_bias=0, dtype=torch.float32):
    """sum_{t,t'} G_a (n_bias + sum_j G_b^j) per utterance in ``dtype`` -> [N]."""
    ga, gb = grams(a, bs, n_bias, dtype)
    return (ga * gb).sum(dim=(1, 2))


def gram_scale64(a, bs=(), n_bias=0):
    """sum_{t,t'} |G_a| |n_bias + sum_j G_b^j| in float64: what an error of the Gram form is measured against (the result itself can
    cancel to far less) -> [N]."""
    ga, gb = grams(a, bs, n_bias, torch.float64)
    return (ga.abs() * gb.abs()).sum(dim=(1, 2))
