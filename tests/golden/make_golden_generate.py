#!/usr/bin/env python3
"""Generate the generation fixture (g13_gpt_generate.npz) by running the REFERENCE itself on CPU: ha.attention.generate, greedy
(top_k=1, stop_token=-1), one row at a time (the reference's loop is batch-1), on parameters the tests regenerate from the seed.

    HA_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_generate.py

Like make_golden_lora.py it runs where the reference is checked out and writes data only.  Per seed s in (0, 1):
    parameters  oracle.gpt_ref.make_gpt_params(2048, 256, 2, 12, 768, False, s)       (not stored)
    prompts     randint(1, 2048, (8, 16)) from Generator().manual_seed(s + 1)         (stored, and regenerated in the test)
    tokens      [8, 48] the reference's greedy chain
    top2        [8, 48, 2] the two largest logits of every step (the margin decides which positions a test may compare)
    strided     [8, 48, 128] the step's logits at vocabulary indices 0, 16, 32, ...
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
if 'HA_REFERENCE' not in os.environ:
    sys.exit('set HA_REFERENCE to a checkout of the reference (the directory that holds ha/)')
sys.path.insert(0, os.environ['HA_REFERENCE'])
sys.dont_write_bytecode = True

import numpy as np
import torch

import ha.attention, ha.init          # the reference

from oracle import gpt_ref

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)
VOCAB, BLOCK, LAYERS, HEADS, EMBD = 2048, 256, 2, 12, 768
ROWS, PROMPT, NEW, STRIDE = 8, 16, 48, 16


def chain(seed):
    cfg = ha.init.GPTConfig(block_size=BLOCK, vocab_size=VOCAB, n_layer=LAYERS, n_head=HEADS, n_embd=EMBD, bias=False)
    model = ha.attention.GPT(cfg)
    model.load_state_dict(gpt_ref.make_gpt_params(VOCAB, BLOCK, LAYERS, HEADS, EMBD, False, seed), strict=True)
    model.eval()
    prompts = torch.randint(1, VOCAB, (ROWS, PROMPT), generator=torch.Generator().manual_seed(seed + 1))
    seen = []
    hook = model.register_forward_hook(lambda mod, args, out: seen.append(out[0][:, -1, :].detach().clone()))
    tokens = np.zeros((ROWS, NEW), dtype=np.int64)
    top2 = np.zeros((ROWS, NEW, 2), dtype=np.float32)
    strided = np.zeros((ROWS, NEW, VOCAB // STRIDE), dtype=np.float32)
    for r in range(ROWS):
        del seen[:]
        out = [int(t) for t in ha.attention.generate(model, prompts[r:r + 1], NEW, top_k=1, stop_token=-1)]
        assert len(out) == NEW and len(seen) == NEW
        tokens[r] = out
        for i, lg in enumerate(seen):
            top2[r, i] = torch.topk(lg[0], 2).values.numpy()
            strided[r, i] = lg[0, ::STRIDE].numpy()
            assert int(lg[0].argmax()) == out[i]
    hook.remove()
    return prompts.numpy(), tokens, top2, strided


if __name__ == '__main__':
    d = {'cfg': np.array([VOCAB, BLOCK, LAYERS, HEADS, EMBD, ROWS, PROMPT, NEW, STRIDE])}
    for seed in (0, 1):
        p, t, m, s = chain(seed)
        d[f'prompts{seed}'], d[f'tokens{seed}'], d[f'top2_{seed}'], d[f'strided{seed}'] = p, t, m, s
        margin = m[..., 0] - m[..., 1]
        print('seed', seed, 'positions under 1e-2:', int((margin < 1e-2).sum()), 'under 0.1:', int((margin < 0.1).sum()))
    path = os.path.join(OUT, 'g13_gpt_generate.npz')
    np.savez_compressed(path, **d)
    print(os.path.getsize(path), 'bytes')
