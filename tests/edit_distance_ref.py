"""Yardstick for csrc/edit_distance.hip: the Levenshtein table with the tie rule of include/halo.h in plain Python, and the n-best risk with
its gradient in float64 torch.  Nothing here touches the device or the library."""
import torch


def edit_distance(hyp, ref):
    """hyp, ref: sequences of hashable tokens -> (errors, (ins, del, sub)).  D[i][j] scores the first i hypothesis tokens against the first
    j reference tokens; a cell keeps one predecessor among those of minimal total in the order diagonal, deletion (i, j-1), insertion
    (i-1, j), and carries that predecessor's counts: they are the counts of the path those choices lead along from (Lh, Lr)."""
    lh, lr = len(hyp), len(ref)
    prev = [(j, 0, j, 0) for j in range(lr + 1)]                 # row 0: (total, ins, del, sub)
    for i in range(1, lh + 1):
        cur = [(i, i, 0, 0)]
        h = hyp[i - 1]
        for j in range(1, lr + 1):
            d, l, u = prev[j - 1], cur[j - 1], prev[j]
            sub = 0 if h == ref[j - 1] else 1
            best = min(d[0] + sub, l[0] + 1, u[0] + 1)
            if d[0] + sub == best:
                cur.append((best, d[1], d[2], d[3] + sub))
            elif l[0] + 1 == best:
                cur.append((best, l[1], l[2] + 1, l[3]))
            else:
                cur.append((best, u[1] + 1, u[2], u[3]))
        prev = cur
    total, ins, del_, sub = prev[lr]
    return total, (ins, del_, sub)


def batch(hyp, hyp_lengths, ref, ref_lengths, group=1):
    """The launch's arguments as nested lists -> (errors [P], counts [P][3]); a negative hypothesis length is an absent hypothesis."""
    errors, counts = [], []
    for p, (row, n) in enumerate(zip(hyp, hyp_lengths)):
        if n < 0:
            errors.append(-1); counts.append([0, 0, 0])
            continue
        r = p // group
        e, c = edit_distance(list(row[:n]), list(ref[r][:ref_lengths[r]]))
        errors.append(e); counts.append(list(c))
    return errors, counts


def nbest_risk(losses, errors):
    """losses [N, W] (any float dtype; taken to float64, autograd flows through), errors [N, W] integers (< 0: absent) -> risk [N] float64:
    over a row's present hypotheses, sum_w softmax(-losses)_w err_w - mean_w err_w; 0 for a row without one."""
    l = losses.double()
    present = errors >= 0
    err = errors.clamp(min=0).double()
    logits = torch.where(present, -l, torch.full_like(l, float('-inf')))
    any_present = present.any(1, keepdim=True)
    p = torch.softmax(torch.where(any_present, logits, torch.zeros_like(l)), dim=1) * present
    expected = (p * err).sum(1)
    mean = err.sum(1) / present.sum(1).clamp(min=1)
    return torch.where(any_present[:, 0], expected - mean, torch.zeros_like(mean))


def nbest_risk_grad(losses, errors):
    """The closed form of d risk[n] / d losses[n, w] in float64: -p_w (err_w - sum_v p_v err_v), 0 for an absent hypothesis."""
    l = losses.detach().double()
    present = errors >= 0
    err = errors.clamp(min=0).double()
    grad = torch.zeros_like(l)
    for n in range(l.shape[0]):
        idx = present[n].nonzero().view(-1)
        if idx.numel():
            p = torch.softmax(-l[n, idx], 0)
            grad[n, idx] = -p * (err[n, idx] - (p * err[n, idx]).sum())
    return grad
