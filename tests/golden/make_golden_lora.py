#!/usr/bin/env python3
"""Generate the LoRA fixtures (g12_gpt_lora_*.npz) by running the REFERENCE itself on CPU: ha.attention.GPT with ha.lora attached to every
c_attn and only the adapters trainable, as `hala --lora` sets it up (ha/attention_loop.py:137-139).

    HA_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_lora.py

Like make_golden.py it runs where the reference is checked out and writes data only: config,
r and alpha, every parameter (lora_B drawn NON-zero: at its zero init A's gradient is zero and a test would see nothing), inputs, targets,
the train-mode loss at lora_dropout = 0 with the gradients of the trainable parameters, the sorted state-dict keys, the trainable names,
the eval-mode (merged) per-token NLL and the merged c_attn.weight of layer 0.
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

import ha.attention, ha.init, ha.lora          # the reference

from oracle import gpt_ref

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)
R, ALPHA = 4, 32


def lora_case(name, vocab, block, n_layer, n_head, n_embd, bias, B, T, seed):
    cfg = ha.init.GPTConfig(block_size=block, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bias)
    model = ha.attention.GPT(cfg)
    model.load_state_dict(gpt_ref.make_gpt_params(vocab, block, n_layer, n_head, n_embd, bias, seed), strict=True)
    ha.lora.attach_to_c_attn(model, r=R, lora_alpha=ALPHA, lora_dropout=0.0)
    ha.lora.mark_only_lora_as_trainable_(model)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for k, v in model.named_parameters():
            if 'lora_A.weight' in k:                  # in the range of the reference's init (kaiming_uniform_, a = sqrt(5)), but seeded
                v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) / v.shape[1] ** 0.5)
            elif 'lora_' in k:                        # B and the adapter biases non-zero
                v.copy_(torch.randn(v.shape, generator=g) * 0.05)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    inputs, targets = gpt_ref.synthetic_tokens(B, T, vocab, seed + 1)
    model.train()
    model.zero_grad()
    loss = model.forward_all(inputs, targets, reduction='mean')
    loss.backward()
    d = {'cfg': np.array([vocab, block, n_layer, n_head, n_embd, int(bias), B, T, seed]), 'r': np.array(R), 'alpha': np.array(ALPHA),
         'inputs': inputs.numpy(), 'targets': targets.numpy(), 'loss': loss.detach().numpy(),
         'keys': np.array(sorted(model.state_dict())), 'trainable': np.array([k for k, v in model.named_parameters() if v.requires_grad])}
    for k, v in model.named_parameters():
        if v.requires_grad:
            d['grad.' + k] = v.grad.numpy().copy()
        else:
            assert v.grad is None
    for k, v in params.items():
        d['param.' + k] = v.numpy()
    model.eval()                                      # merges scaling * B A into every c_attn.weight
    with torch.no_grad():
        d['per_token'] = model.forward_all(inputs, targets, reduction='none').numpy()
    d['merged.transformer.h.0.attn.c_attn.weight'] = model.transformer.h[0].attn.c_attn.weight.detach().numpy().copy()
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **d)
    print(name, 'loss', float(loss), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    lora_case('g12_gpt_lora_nobias', 97, 32, 2, 2, 64, False, 3, 20, 31)
    lora_case('g12_gpt_lora_bias', 97, 32, 2, 2, 64, True, 3, 20, 32)
