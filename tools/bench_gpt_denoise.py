#!/usr/bin/env python3
"""The denoise objective (`hala --objective denoise`) on the reference's `encoder` arch at GPT-2-small width -- block 128, bidirectional,
vocabulary 50304, B = 64 (M = 8192 token rows), `bf16` arithmetic -- on one MI355X: one masked batch from symbol_tape.get_batch, then the
full training step (forward + backward + AdamW) with the dense head against the head on the target rows only
(GPT.set_target_capacity(symbol_tape.target_capacity(B, T)) = 1536 rows), measured in the SAME run in alternating windows; the head's
own launches (ln_f, lm_head, cross-entropy and their backward) timed with HIP events on both paths; the HIP-event times of the new
kernels at the step's shapes.  Prints human-readable lines and ONE JSON line (last).

    python tools/bench_gpt_denoise.py [--rounds 5] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, attention, mlm, ops, symbol_tape

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--batch', type=int, default=64)
args = ap.parse_args()

_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16')
B, T, SEED = args.batch, 128, 0x5EED0D15EA5E
cfg = attention.GPTConfig(block_size=T, causal=False)                  # ha/init.py:119-121 at n_layer 12, n_head 12, n_embd 768, vocab 50304
torch.manual_seed(0)
model = attention.GPT(cfg).cuda().train()
with torch.no_grad():                                                  # the reference's init zeroes wpe; give it content
    model.transformer.wpe.weight.normal_(0, 0.02)
M, C, V = B * T, cfg.n_embd, cfg.vocab_size
K = symbol_tape.target_capacity(B, T)
tape = torch.randint(1, 50257, (B * T + T,), generator=torch.Generator().manual_seed(3)).to(torch.int16).cuda()
offsets = (torch.arange(B) * T).cuda()
inputs_d, targets_d = symbol_tape.get_batch(tape, offsets, T, 'denoise', seed=SEED, step=0)
n_targets = int((targets_d != 0).sum())
assert n_targets <= K, (n_targets, K)
assert attention.rowmajor_train_ok(cfg, model.transformer.h, M, True) and attention.rows_ok(M, C)
params = list(model.parameters())
opt = ops.AdamWMulti(params, [0.1 if p.dim() >= 2 else 0.0 for p in params], lr=3e-4, betas=(0.9, 0.95), eps=1e-8)


def stepper(capacity):
    def step():
        model.set_target_capacity(capacity)
        for p in params: p.grad = None
        loss = model.forward_all(inputs_d, targets_d)
        loss.backward()
        opt.step()
        return loss
    return step


def window(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


def event_us(fn, reps=50):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


legs = {'dense': stepper(None), 'compact': stepper(K)}
times = {k: [] for k in legs}
for fn in legs.values():                                               # warm every shape of both legs
    window(fn, 3)
last = {}
for _ in range(args.rounds):                                           # alternating windows: both legs see the same machine state
    for k, fn in legs.items():
        t, last[k] = window(fn, args.steps)
        times[k].append(t)
ms = {k: round(1e3 * statistics.median(v), 3) for k, v in times.items()}
spread = {k: round(1e3 * (max(v) - min(v)), 3) for k, v in times.items()}
for k in legs:
    print(f'encoder-arch GPT (12 x 768, V={V}) denoise step B={B} T={T} bf16, {k} head: {ms[k]:.2f} ms (windows '
          f'{[round(1e3 * t, 2) for t in times[k]]})  loss {last[k].item():.4f}')
res = {'metric': 'ms per training step, encoder-arch GPT at GPT-2-small width, B=64 T=128 bf16, denoise objective: dense head against the head '
                 'on the target rows (forward + backward + AdamW)',
       'unit': 'ms', 'n_gpus': 1, 'value': ms['compact'],
       'config': {'batch': B, 'seq_len': T, 'math': 'bf16', 'rows': M, 'targets': n_targets, 'capacity': K, 'rounds': args.rounds,
                  'steps_per_window': args.steps},
       'dense_step_ms': ms['dense'], 'compact_step_ms': ms['compact'], 'saved_ms': round(ms['dense'] - ms['compact'], 3),
       'window_spread_ms': spread, 'windows_ms': {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()}}

# the head alone on both paths: ln_f, lm_head + cross-entropy, the CE gradient, both gradient products, ln_f's backward -- and, compact,
# the compaction, the two gathers and the two scatters around them
model.set_target_capacity(None)
x = torch.randn(M, C, device='cuda')
grad = torch.full((M,), 1.0 / n_targets, device='cuda')
tg = targets_d.reshape(-1)
put = lambda p, g: None


def head_dense():
    with torch.no_grad(), attention.training_images():
        loss, saved = model._head_train(x, tg, True)
        return model._head_backward(saved, tg, grad, True, True, put)


def head_compact():
    with torch.no_grad(), attention.training_images():
        rec = ops.target_rows(tg, K)
        x_c = ops.gather_rows(x, rec.rows)
        loss_c, saved = model._head_train(x_c, rec.targets, True)
        ops.scatter_rows(loss_c, rec, M)
        dx_c, _, dw = model._head_backward(saved, rec.targets, ops.gather_rows(grad, rec.rows), True, False, put)
        return ops.scatter_rows(dx_c, rec, M, want_bf16=True)


head = {'dense': event_us(head_dense, 20), 'compact': event_us(head_compact, 20)}
res['head_us'] = head
res['head_share'] = {k: round(head[k] / (1e3 * ms[k]), 4) for k in head}
for k in head:
    print(f'head ({k}): {head[k]:.0f} us = {100 * res["head_share"][k]:.1f} % of the {k} step')

# the new kernels at the step's shapes (HIP events over 50 back-to-back launches)
rec = ops.target_rows(tg, K)
x_c = ops.gather_rows(x, rec.rows)
loss_c = torch.randn(K, device='cuda')
ids = inputs_d.clone()
kern = {
    f'mlm_batch_u16  [{B}, {T}] gather + mask': lambda: symbol_tape.get_batch(tape, offsets, T, 'denoise', seed=SEED, step=1),
    f'mask_tokens    [{B}, {T}] in place': lambda: mlm.mask_tokens(ids, seed=SEED, step=1),
    f'target_rows    M={M} -> K={K}': lambda: ops.target_rows(tg, K),
    f'gather_rows    [{K}, {C}] fp32': lambda: ops.gather_rows(x, rec.rows),
    f'gather_rows    [{K}] per-token gradient': lambda: ops.gather_rows(grad, rec.rows),
    f'scatter_rows   [{M}, {C}] fp32 + bf16': lambda: ops.scatter_rows(x_c, rec, M, want_bf16=True),
    f'scatter_rows   [{M}] per-token loss': lambda: ops.scatter_rows(loss_c, rec, M),
}
res['kernels_us'] = {}
for name, fn in kern.items():
    res['kernels_us'][name] = event_us(fn)
    print(f'{name}: {res["kernels_us"][name]:.1f} us')
print(json.dumps(res), flush=True)
