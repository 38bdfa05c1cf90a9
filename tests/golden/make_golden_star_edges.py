#!/usr/bin/env python3
"""Generate tests/golden/g8_star_edges.npz: star-CTC with EMPTY targets, from the REFERENCE's own ha.star on the CPU.

Run where the reference is checked out (REFERENCE_ROOT names the checkout); it does not exist on the GPU box:

    REFERENCE_ROOT=... PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_star_edges.py

With target_lengths[n] == 0 the read-out of ha/star.py:109-110,156-163 takes the padded states S_last-3 .. S_last = the last of the four
virtual states before state 0 (finfo.min after frame 0) and the real states 0, 1, 2: blank, the first star, blank.  g8_star.npz has no
such row.  Two cases, both with the key layout of g8_star.npz (tests/golden/make_golden.py star_case):

    empty_target   T 15, N 3, C 9, S 4   target_lengths 0, 4, 0; emission_lengths 15, 15, 1 (an empty target read after a single frame)
    mixed          T 12, N 4, C 7, S 3   target_lengths 0, 3, 0, 3 with ragged emission lengths, penalty -1.5, a repeated label

Only data is written: the inputs, ha.star.star_ctc_forward_score's losses and its autograd gradient of their sum, and
ha.star.intersperse_stars' targets and first-frame emissions.
"""
import os
import sys

if 'REFERENCE_ROOT' not in os.environ:
    sys.exit('set REFERENCE_ROOT to the reference checkout')
sys.path.insert(0, os.environ['REFERENCE_ROOT'])
sys.dont_write_bytecode = True

import numpy as np
import torch

import ha.star      # the reference

OUT = os.path.dirname(os.path.abspath(__file__))


def star_case(name, T, N, C, S, seed, penalty, il, tl, targets=None):
    g = torch.Generator().manual_seed(seed)
    em = torch.randn(T, N, C, generator=g).log_softmax(-1).requires_grad_(True)
    if targets is None:
        targets = torch.randint(1, C, (N, S), generator=g)
    losses = ha.star.star_ctc_forward_score(em, targets, il, tl, star_penalty=penalty)
    losses.sum().backward()
    assert torch.isfinite(losses).all() and torch.isfinite(em.grad).all()
    with torch.no_grad():
        s_em, s_tg = ha.star.intersperse_stars(em, targets)
    print(name, 'losses', losses.tolist())
    return {name + '.emissions': em.detach().numpy(), name + '.targets': targets.numpy(), name + '.il': il.numpy(), name + '.tl': tl.numpy(),
            name + '.penalty': np.float32(penalty), name + '.losses': losses.detach().numpy(), name + '.grad': em.grad.numpy(),
            name + '.star_targets': s_tg.numpy(), name + '.star_emissions_t0': s_em[0].numpy()}


def main():
    d = {}
    d.update(star_case('empty_target', 15, 3, 9, 4, 8, -0.5, il=torch.tensor([15, 15, 1]), tl=torch.tensor([0, 4, 0])))
    d.update(star_case('mixed', 12, 4, 7, 3, 9, -1.5, il=torch.tensor([12, 12, 7, 5]), tl=torch.tensor([0, 3, 0, 3]),
                       targets=torch.tensor([[2, 4, 1], [3, 3, 6], [5, 5, 5], [1, 6, 6]])))
    path = os.path.join(OUT, 'g8_star_edges.npz')
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
