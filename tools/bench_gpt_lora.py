#!/usr/bin/env python3
"""GPT-2 small (124 M), B = 8, T = 1024, `bf16` arithmetic on one MI355X: the full training step against the LoRA step (`hala --lora`:
adapters of rank 4 on every c_attn, lora_dropout 0.1, the base frozen; forward + backward + AdamW over the adapters only), measured in
the SAME run in alternating windows, then scoring with the adapters merged (eval) and the HIP-event times of the three halo_lora_*
kernels at the step's shapes.  Prints human-readable lines and ONE JSON line (last).

    python tools/bench_gpt_lora.py [--rounds 3] [--steps 10]
    python tools/bench_gpt_lora.py --leg full|lora --steps 10        # one leg only, for a kernel-trace run of its own
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, attention, lora, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--leg', choices=['both', 'full', 'lora'], default='both')
ap.add_argument('--rank', type=int, default=4)
ap.add_argument('--lora-dropout', type=float, default=0.1)
args = ap.parse_args()

_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16')
B, T = int(os.environ.get('B', '8')), 1024
cfg = attention.GPTConfig()
torch.manual_seed(0)
full = attention.GPT(cfg).cuda().train()
with torch.no_grad():                                     # the reference's init zeroes wpe; give it content
    full.transformer.wpe.weight.normal_(0, 0.02)
inputs, targets = synth.synthetic_tokens(B, T, cfg.vocab_size, 3, pad_tail=False)
inputs_d, targets_d = inputs.cuda(), targets.cuda()
M, C = B * T, cfg.n_embd


def stepper(model, params, decays):
    opt = ops.AdamWMulti(params, decays, lr=3e-4, betas=(0.9, 0.95), eps=1e-8)

    def step():
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


legs = {}
if args.leg in ('both', 'full'):
    ps = list(full.parameters())
    legs['full'] = stepper(full, ps, [0.1 if p.dim() >= 2 else 0.0 for p in ps])
if args.leg in ('both', 'lora'):
    adapted = copy.deepcopy(full) if args.leg == 'both' else full
    adapted._images = attention.WeightImages()
    lora.attach_to_c_attn(adapted, r=args.rank, lora_alpha=32, lora_dropout=args.lora_dropout)
    lora.mark_only_lora_as_trainable_(adapted)
    with torch.no_grad():                                 # B at its zero init makes A's gradient zero; timing does not care, the loss line does
        for blk in adapted.transformer.h:
            blk.attn.c_attn.lora_B.weight.normal_(0, 0.02)
    assert attention.rowmajor_train_ok(cfg, adapted.transformer.h, M, True) and attention.rows_ok(M, C)
    ps = [p for p in adapted.parameters() if p.requires_grad]
    legs['lora'] = stepper(adapted, ps, [0.0] * len(ps))

times = {k: [] for k in legs}
for fn in legs.values():                                  # warm every shape of both legs
    window(fn, 3)
last = {}
for _ in range(args.rounds):                              # alternating windows: both legs see the same machine state
    for k, fn in legs.items():
        t, last[k] = window(fn, args.steps)
        times[k].append(t)
ms = {k: round(1e3 * statistics.median(v), 3) for k, v in times.items()}
for k in legs:
    print(f'GPT-2 small {k} step B={B} T={T} bf16: {ms[k]:.2f} ms (windows {[round(1e3 * t, 2) for t in times[k]]})  loss {last[k].item():.4f}')
res = {'metric': 'ms per training step, GPT-2 small B=8 T=1024 bf16: full fine-tuning against LoRA on c_attn (forward + backward + AdamW)',
       'unit': 'ms', 'n_gpus': 1, 'config': {'batch': B, 'seq_len': T, 'math': 'bf16', 'rank': args.rank, 'lora_dropout': args.lora_dropout,
                                             'rounds': args.rounds, 'steps_per_window': args.steps},
       'full_step_ms': ms.get('full'), 'lora_step_ms': ms.get('lora'),
       'windows_ms': {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()}}
if args.leg != 'both':
    print(json.dumps(res), flush=True)
    sys.exit(0)
res['value'] = ms['lora']
res['saved_ms'] = round(ms['full'] - ms['lora'], 3)

# scoring with the adapters merged: eval() folds s B A into c_attn.weight, no adapter launch runs
adapted.eval()
with torch.inference_mode():
    window(lambda: adapted.forward_all(inputs_d, targets_d, reduction='none'), 2)
    t_score, _ = window(lambda: adapted.forward_all(inputs_d, targets_d, reduction='none'), 5)
full.eval()
with torch.inference_mode():
    window(lambda: full.forward_all(inputs_d, targets_d, reduction='none'), 2)
    t_score_base, _ = window(lambda: full.forward_all(inputs_d, targets_d, reduction='none'), 5)
res['merged_scoring_ms'], res['base_scoring_ms'] = round(1e3 * t_score, 3), round(1e3 * t_score_base, 3)
print(f'scoring B={B} T={T}: adapters merged {1e3 * t_score:.2f} ms, base model {1e3 * t_score_base:.2f} ms')


def event_us(fn, reps=50):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


# the three kernels at the step's shapes (HIP events over 50 back-to-back launches; algorithmic bytes = the rows each must move once)
lin = adapted.transformer.h[0].attn.c_attn
A16, At16, B16, Bt16 = lora.packed(adapted._images, lin)
drop = ops.Dropout(args.lora_dropout, 1234, 0)
h1b = torch.randn(M, C, device='cuda').bfloat16()
dqkvb = torch.randn(M, 3 * C, device='cuda').bfloat16()
qkv = torch.randn(M, 3 * C, device='cuda').bfloat16()
dln = torch.randn(M, C, device='cuda')
u = ops.lora_down(h1b, A16)
kern = {
    'lora_down fwd  X=h1b [M,768] masked': (lambda: ops.lora_down(h1b, A16, 1.0, drop, 4096), 2 * M * C),
    'lora_down bwd  X=dqkv [M,2304]': (lambda: ops.lora_down(dqkvb, Bt16, lin.scaling), 2 * M * 3 * C),
    'lora_up   fwd  qkv bf16 [M,2304] +=': (lambda: ops.lora_up_(qkv, u, B16, lin.scaling), 4 * M * 3 * C),
    'lora_up   bwd  d_ln1 fp32 [M,768] += masked': (lambda: ops.lora_up_(dln, u, At16, 1.0, drop, 4096), 8 * M * C),
    'lora_tn   dB   X=dqkv [M,2304]': (lambda: ops.lora_tn(u, dqkvb, lin.r, lin.scaling, transpose_out=True), 2 * M * 3 * C),
    'lora_tn   dA   X=h1b [M,768] masked': (lambda: ops.lora_tn(u, h1b, lin.r, 1.0, drop=drop, stream_id=4096), 2 * M * C),
}
res['kernels'] = {}
for name, (fn, nbytes) in kern.items():
    us = event_us(fn)
    res['kernels'][name] = {'us': us, 'algorithmic_bytes': nbytes, 'GB_per_s': round(nbytes / us / 1e3, 1)}
    print(f'{name}: {us:.1f} us  ({nbytes / us / 1e3:.0f} GB/s of algorithmic bytes)')
res['kernels_us_per_step_estimate'] = round(cfg.n_layer * sum(v['us'] for v in res['kernels'].values()), 1)
print(json.dumps(res), flush=True)
