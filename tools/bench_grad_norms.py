#!/usr/bin/env python3
"""Per-utterance gradient norms of the LSTM-CTC model on one MI355X, at LC-2x1024 (F = 80, conv 128, H = 1024, 2 layers, V = 32), B = 64,
T = 80 (T' = 21), training mode with the model's dropout, for each arithmetic mode:

  ghost     haloop_amd.grad_norm.gradient_norms: one forward, one backward, one Gram launch and its fixed-order sum;
  single    the only alternative without it: B single-utterance forward + backward passes through the autograd path (MiniSystem.forward
            on a batch of one, loss.backward()), the .grads folded by norm_batched as the reference folds them;
  launch    the Gram launch and its sum alone (ops.ghost_sqnorm on the terms of one backward), by device events.

`ghost` and `single` are timed in the SAME process in alternating windows of a host clock around work that ends in a device synchronise,
after a warm-up of every leg; the median, minimum and maximum of the windows are reported.  Human-readable lines, then ONE JSON line.

    python tools/bench_grad_norms.py [--rounds 5] [--reps 20] [--single-reps 1] [--modes f32,bf16x3,bf16]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, grad_norm, ops, recognizer, rnn
from oracle import cpu_ref

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='gradient_norms calls per timed window')
ap.add_argument('--single-reps', type=int, default=1, help='batches of B single-utterance passes per timed window')
ap.add_argument('--launch-reps', type=int, default=200)
ap.add_argument('--modes', default='f32,bf16x3,bf16')
ap.add_argument('--batch', type=int, default=64)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit('bench_grad_norms: no GPU; a timing needs the device (not measured)')
F_, C, H, L, V, B, T, S = 80, 128, 1024, 2, 32, args.batch, 80, 10
_lib.lib(); _lib.lend_scratch(256 << 20)
enc_p, rec_p = cpu_ref.make_params(F_, C, H, L, V, 1)
x, il, tg, tl = cpu_ref.synthetic_batch(B, T, F_, V, S, 2)
il = torch.tensor([T - 3 * (i % 8) for i in range(B)], dtype=torch.int64)
enc = rnn.Encoder(F_, C, H, num_layers=L); rec = recognizer.TemporalClassifier(H, V)
enc.load_state_dict(enc_p); rec.load_state_dict(rec_p)
system = grad_norm.MiniSystem(enc, rec).cuda().train()
x, il, tg, tl = x.cuda(), il.cuda(), tg.cuda(), tl.cuda()
names = [k for k, _ in system.named_parameters()]


def ghost():
    return grad_norm.gradient_norms(system, x, tg, il, tl)


def single():
    """B batches of one through autograd; the gradients of every utterance kept (B x 13.2 M floats) and folded as ha/grad_norm.py:101 does."""
    rows, losses = [], []
    for n in range(B):
        system.zero_grad(set_to_none=True)
        loss = system(x[n:n + 1], tg[n:n + 1], il[n:n + 1], tl[n:n + 1])
        loss.backward()
        rows.append([p.grad for p in system.parameters()])
        losses.append(loss.detach())
    per_param = [grad_norm.norm_batched(torch.stack([rows[n][i] for n in range(B)])) for i in range(len(names))]
    system.zero_grad(set_to_none=True)
    return grad_norm.norm_batched(torch.stack(per_param).T), torch.stack(losses)


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def launch_alone():
    with torch.no_grad():
        terms, _, n, tp, _ = grad_norm._backward_terms(system, x, tg, il, tl)
        ws = torch.empty(ops.ghost_sqnorm_workspace(len(terms), n, tp), device='cuda')
        sq = torch.empty(len(terms), n, device='cuda'); norm = torch.empty(n, device='cuda')
        run = lambda: ops.ghost_sqnorm(terms, n, tp, workspace=ws, out=sq, norm_out=norm)
        for _ in range(10):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(args.rounds):
            e0.record()
            for _ in range(args.launch_reps):
                run()
            e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.launch_reps)
        return times, len(terms)


results = []
for mode in args.modes.split(','):
    _lib.set_math_mode(mode)
    g_norms, g_losses = ghost(); ghost()                               # warm both legs
    s_norms, s_losses = single()
    rel = float(((g_norms - s_norms).abs() / s_norms).max())           # different dropout draws per leg: an order-of-magnitude check only
    times = {'ghost': [], 'single': []}
    for _ in range(args.rounds):                                       # alternating windows
        times['ghost'].append(window(ghost, args.reps))
        times['single'].append(window(single, args.single_reps))
    lt, n_terms = launch_alone()
    r = dict(mode=mode, ghost_ms=statistics.median(times['ghost']) * 1e3, ghost_ms_min=min(times['ghost']) * 1e3, ghost_ms_max=max(times['ghost']) * 1e3,
             single_ms=statistics.median(times['single']) * 1e3, single_ms_min=min(times['single']) * 1e3, single_ms_max=max(times['single']) * 1e3,
             launch_us=statistics.median(lt) * 1e3, launch_us_min=min(lt) * 1e3, launch_us_max=max(lt) * 1e3, terms=n_terms,
             lstm_bwd_kernel=_lib.lstm_chain_info('bwd')['kernel'], norm_rel_diff_between_legs=rel)
    r['speedup'] = r['single_ms'] / r['ghost_ms']
    results.append(r)
    print(f"{mode:7s} gradient_norms {r['ghost_ms']:8.3f} ms/batch (min {r['ghost_ms_min']:.3f} max {r['ghost_ms_max']:.3f}); "
          f"{B} single-utterance passes {r['single_ms']:9.3f} ms/batch (min {r['single_ms_min']:.3f} max {r['single_ms_max']:.3f}): {r['speedup']:.1f}x; "
          f"Gram launch + sum alone {r['launch_us']:.1f} us (min {r['launch_us_min']:.1f} max {r['launch_us_max']:.1f}), {n_terms} terms; "
          f"backward chain {r['lstm_bwd_kernel']}", flush=True)
_lib.set_math_mode('f32')
print(json.dumps(dict(bench='grad_norms', F=F_, conv=C, H=H, L=L, V=V, B=B, T=T, rounds=args.rounds, reps=args.reps, single_reps=args.single_reps,
                      launch_reps=args.launch_reps, results=results)))
