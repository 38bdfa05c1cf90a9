#!/usr/bin/env python3
"""Generate tests/golden/g15_grad_norms.npz: per-utterance gradient norms of the LSTM-CTC model from the REFERENCE's own modules on the CPU.

Run where the reference is checked out (REFERENCE_ROOT names the checkout); it does not exist on the GPU box:

    REFERENCE_ROOT=... PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_grad_norms.py

The reference's own ``ha.grad_norm.gradient_norms`` cannot run this model: it differentiates under vmap, which has no batching rule for
F.ctc_loss (ha/grad_norm.py:14-16 strips the CTC loss for that reason).  What it WOULD compute is well defined all the same and is what
this script records: ``ha.rnn.Encoder`` + ``ha.recognizer.TemporalClassifier`` in train() mode with every dropout probability set to 0
(the reference's "test time dropout" draws from torch's generator, which no other implementation can replay), each utterance run as a
batch of one through forward and backward, and the gradients folded by the reference's ``ha.grad_norm.norm_batched`` exactly as its
gradient_norms folds them.  Only data is written: the state dict, the inputs, per-utterance norms and losses, per-parameter squared norms.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
if 'REFERENCE_ROOT' not in os.environ:
    sys.exit('set REFERENCE_ROOT to the reference checkout')
sys.path.insert(0, os.environ['REFERENCE_ROOT'])
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

import ha.rnn, ha.recognizer, ha.grad_norm      # the reference

from oracle import cpu_ref

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)

F_, T, C, H, V, B, S = 80, 80, 128, 32, 32, 5, 10


def feasible(tg, tl, flen):
    """CTC needs one frame per label and one more per repeated neighbour."""
    for n in range(tg.shape[0]):
        lab = tg[n, :int(tl[n])]
        if int(tl[n]) + int((lab[1:] == lab[:-1]).sum()) > int(flen[n]):
            return False
    return True


def run(L, seed):
    enc_p, rec_p = cpu_ref.make_params(F_, C, H, L, V, seed)
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(B, T, F_, generator=g)
    il = torch.randint(64, 81, (B,), generator=g, dtype=torch.int64)
    il[0], il[1] = 80, 64                                           # both ends of the range
    tg = torch.randint(1, V, (B, S), generator=g, dtype=torch.int64)
    tl = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int64)
    tl[2], tl[3] = 1, S
    enc = ha.rnn.Encoder(input_dim=F_, subsample_dim=C, hidden_dim=H)
    enc.lstm = nn.LSTM(C, H, num_layers=L, batch_first=True, dropout=0.0)
    rec = ha.recognizer.TemporalClassifier(feat_dim=H, vocab_size=V)
    enc.load_state_dict(enc_p); rec.load_state_dict(rec_p)
    enc.dropout.p = 0.0; rec.dropout.p = 0.0
    enc.train(); rec.train()
    assert feasible(tg, tl, enc.subsampled_lengths(il)), 'an utterance has fewer frames than its labels need'
    named = [('encoder.' + k, p) for k, p in enc.named_parameters()] + [('recognizer.' + k, p) for k, p in rec.named_parameters()]
    losses, grads = [], {k: [] for k, _ in named}
    for n in range(B):                                              # every utterance as a batch of one
        feats, flen, _ = enc(x[n:n + 1], il[n:n + 1])
        loss, _ = rec(feats, tg[n:n + 1], flen, tl[n:n + 1])
        assert torch.isfinite(loss)
        gs = torch.autograd.grad(loss, [p for _, p in named])
        losses.append(loss.detach())
        for (k, _), gr in zip(named, gs):
            grads[k].append(gr)
    stacked = {k: torch.stack(v) for k, v in grads.items()}
    norms = ha.grad_norm.norm_batched(torch.stack([ha.grad_norm.norm_batched(v) for v in stacked.values()]).T)
    d = {'cfg': np.array([F_, T, C, H, L, V, B, S, seed], dtype=np.int64), 'x': x.numpy(), 'il': il.numpy(), 'tg': tg.numpy(), 'tl': tl.numpy(),
         'norms': norms.numpy(), 'losses': torch.stack(losses).numpy()}
    for k, v in enc_p.items():
        d['param.encoder.' + k] = v.numpy()
    for k, v in rec_p.items():
        d['param.recognizer.' + k] = v.numpy()
    for k, v in stacked.items():
        d['sq.' + k] = v.double().reshape(B, -1).square().sum(dim=1).numpy()
    print(f'L={L}: norms', norms.tolist(), 'losses', [float(v) for v in losses])
    return d


def main():
    out = {}
    for L, seed in ((2, 15), (3, 16)):
        for k, v in run(L, seed).items():
            out[f'l{L}.{k}'] = v
    path = os.path.join(OUT, 'g15_grad_norms.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
