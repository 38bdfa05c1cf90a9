#!/usr/bin/env python3
"""The loss part of the rnn-transducer head's training step on one MI355X, from the two factors of the additive joint (f [N, T, V]
transcription logits, g [N, U + 1, V] prediction-network logits, both leaves) to their gradients, on its two routes:

    dense   f[:, :, None] + g[:, None] -> HF.log_softmax -> transducer_forward_score -> mean -> backward   (recognizer.Transducer today)
    fused   transducer.transducer_loss -> mean -> backward                          (csrc/rnnt_loss.hip; HALO_RNNT_LOSS_FUSED=1)

measured in the SAME process in alternating windows (the method of tools/bench_rnnt_decode.py).  Shapes (N, T, U + 1, V): the arch's
(64, 21, 11, 32) and (64, 21, 11, 256), and (16, 250, 61, 1024), an ordinary utterance batch whose dense tensors are 0.98 GB each.
Reports ms per forward + backward and the rise of torch.cuda.max_memory_allocated above what is allocated before the step.
Human-readable lines, then ONE JSON line.

    python tools/bench_rnnt_loss.py [--rounds 5] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, functional as HF, transducer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='steps per timed window (a fifth of it where a dense tensor passes 256 MB)')
ap.add_argument('--shapes', default='64x21x11x32,64x21x11x256,16x250x61x1024')
args = ap.parse_args()

_lib.lib(); _lib.lend_scratch(256 << 20)


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


results = []
for shape in args.shapes.split(','):
    N, T, U1, V = (int(v) for v in shape.split('x'))
    gen = torch.Generator().manual_seed(V)
    f = (torch.randn(N, T, V, generator=gen) * 3).cuda().requires_grad_(True)
    g = (torch.randn(N, U1, V, generator=gen) * 3).cuda().requires_grad_(True)
    tg = torch.randint(1, V, (N, U1 - 1), generator=gen).cuda()
    fl = torch.randint(max(1, T // 2), T + 1, (N,), generator=gen).cuda()
    tl = torch.randint(0, U1, (N,), generator=gen).cuda()
    fl[0], tl[0] = T, U1 - 1

    def dense():
        f.grad = g.grad = None
        joint = f[:, :, None, :] + g[:, None, :, :]
        transducer.transducer_forward_score(HF.log_softmax(joint), tg, fl, tl).mean().backward()

    def fused():
        f.grad = g.grad = None
        transducer.transducer_loss(f, g, tg, fl, tl).mean().backward()

    legs = {'dense': dense, 'fused': fused}
    grads, peak = {}, {}
    for k, fn in legs.items():                                       # warm every leg, then one step under the allocator's peak counter
        fn()
        grads[k] = (f.grad.clone(), g.grad.clone())
        f.grad = g.grad = None
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    diff = max(float((grads['dense'][i] - grads['fused'][i]).abs().max()) for i in range(2))
    del grads
    f.grad = g.grad = None
    torch.cuda.empty_cache()
    dense_bytes = N * T * U1 * V * 4
    reps = args.reps if dense_bytes < (256 << 20) else max(2, args.reps // 5)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                      # alternating windows
        for k, fn in legs.items():
            times[k].append(window(fn, reps))
    for k in legs:
        ms = statistics.median(times[k]) * 1e3
        r = dict(N=N, T=T, U1=U1, V=V, leg=k, ms_per_step=ms, ms_min=min(times[k]) * 1e3, ms_max=max(times[k]) * 1e3,
                 peak_bytes_above_baseline=peak[k], dense_tensor_bytes=dense_bytes, max_abs_grad_difference_between_legs=diff)
        results.append(r)
        print(f"{shape:>16s} {k:5s} {ms:9.3f} ms/step (min {r['ms_min']:.3f} max {r['ms_max']:.3f})  peak +{peak[k] / 1e6:9.2f} MB "
              f"(one dense tensor {dense_bytes / 1e6:.1f} MB); grads of the two legs differ by at most {diff:.2e}", flush=True)
    del f, g
    torch.cuda.empty_cache()

print(json.dumps(dict(bench='rnnt_loss', mode=_lib.get_math_mode(), rounds=args.rounds, reps=args.reps, results=results)))
