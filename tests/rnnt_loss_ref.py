"""Float64 yardstick of the transducer loss over the additive joint (haloop_amd.transducer.transducer_loss): from the two factors
f [N, T, V] and g [N, U + 1, V] it builds the dense joint f[:, :, None] + g[:, None], its log-softmax, and the lattice score of
ha/transducer.py:175-207 cell by cell,

    alpha[0, 0] = 0;   alpha[t, 0] = alpha[t - 1, 0] + lp[t - 1, 0, 0]
    alpha[t, u] = logaddexp(alpha[t, u - 1] + lp[t, u - 1, y[u - 1]], alpha[t - 1, u] + lp[t - 1, u, 0])      (t = 0: the first term only)
    loss = -(alpha[T_n - 1, U_n] + lp[T_n - 1, U_n, 0])

all in float64 (oracle/star_ref.py transducer_forward_score is the fp32 statement; tests/test_rnnt_loss_cpu.py holds the two together),
with the gradients w.r.t. f and g from torch autograd.  Only the cells inside a row's lengths are walked: the loss reads no other.
CPU only."""
import torch


def make_case(N, T, U1, V, f_lengths=None, target_lengths=None, seed=0, repeat_label=False):
    """Seeded randn logits scaled by 3 (cells far from uniform), labels in [1, V), loss weights in [0.5, 1.5) ->
    (f, g, targets, f_lengths, target_lengths, weights).  ``repeat_label``: row 0's first two labels are equal."""
    gen = torch.Generator().manual_seed(seed)
    f = torch.randn(N, T, V, generator=gen) * 3
    g = torch.randn(N, U1, V, generator=gen) * 3
    targets = torch.randint(1, V, (N, U1 - 1), generator=gen)
    if repeat_label:
        targets[0, 1] = targets[0, 0]
    fl = torch.tensor(f_lengths if f_lengths is not None else [T] * N, dtype=torch.int32)
    tl = torch.tensor(target_lengths if target_lengths is not None else [U1 - 1] * N, dtype=torch.int32)
    return f, g, targets, fl, tl, torch.rand(N, generator=gen) + 0.5


def lattice_losses(lp, targets, f_lengths, target_lengths):
    """lp [N, T, U + 1, V] float64 log-probabilities -> losses [N], differentiable."""
    losses = []
    for n in range(lp.shape[0]):
        Tn, Un = int(f_lengths[n]), int(target_lengths[n])
        y = [int(v) for v in targets[n, :Un]]
        alpha = [[None] * (Un + 1) for _ in range(Tn)]
        for t in range(Tn):
            for u in range(Un + 1):
                if t == 0 and u == 0:
                    a = lp.new_zeros(())
                elif u == 0:
                    a = alpha[t - 1][0] + lp[n, t - 1, 0, 0]
                else:
                    a = alpha[t][u - 1] + lp[n, t, u - 1, y[u - 1]]
                    if t > 0:
                        a = torch.logaddexp(a, alpha[t - 1][u] + lp[n, t - 1, u, 0])
                alpha[t][u] = a
        losses.append(-(alpha[Tn - 1][Un] + lp[n, Tn - 1, Un, 0]))
    return torch.stack(losses)


def transducer_loss_ref(f, g, targets, f_lengths, target_lengths, weights=None):
    """-> (losses [N], df [N, T, V], dg [N, U + 1, V]) in float64; df / dg are the gradients of (losses * weights).sum() (weights
    default to ones)."""
    f64 = f.detach().cpu().double().requires_grad_(True)
    g64 = g.detach().cpu().double().requires_grad_(True)
    lp = (f64[:, :, None, :] + g64[:, None, :, :]).log_softmax(-1)
    losses = lattice_losses(lp, targets.cpu(), f_lengths.cpu(), target_lengths.cpu())
    w = torch.ones_like(losses) if weights is None else weights.detach().cpu().double()
    (losses * w).sum().backward()
    return losses.detach(), f64.grad, g64.grad
