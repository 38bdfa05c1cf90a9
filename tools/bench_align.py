#!/usr/bin/env python3
"""Forced alignment on one MI355X (csrc/viterbi.hip), measured in the SAME process in alternating windows (the method of
tools/bench_rnnt_loss.py), against two comparators per point:

    torch    the same max-plus recursion and backtrace written with torch operators on the device, vectorised over the batch and the
             states (CTC) or the anti-diagonal (transducer): the general path a user would otherwise write
    alpha    the sum-semiring kernel of the same shape: halo_ctc_fwd / halo_transducer_fwd (the same dependency chain, no backtrace)

For CTC the two launches are also timed alone on buffers allocated once (viterbi_launch / alpha_launch: back to back, so the host's side
of a call -- the wrappers and five or two allocations -- is hidden behind the kernels where they are long enough).

CTC, N = 64, C = 32: T x S = 21 x 10 (the bench lattice) and 1000 x 200 (a long utterance).  Transducer, (N, T, U + 1, V) =
(64, 21, 11, 32) and (16, 250, 61, 1024): the lattice launch alone on a dense joint (viterbi / alpha / torch), and the two routes from
the factors f, g -- dense (f + g -> HF.log_softmax -> transducer_viterbi) against factors (transducer_align) -- with the rise of
torch.cuda.max_memory_allocated above what is allocated before the call.  Reads nothing outside the repository.
Human-readable lines, then ONE JSON line.

    python tools/bench_align.py [--rounds 5] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, ctc, functional as HF, ops, transducer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='calls per timed window (the torch legs: one per ~20 ms of their first call)')
ap.add_argument('--ctc', default='64x21x10x32,64x1000x200x32', help='N x T x S x C')
ap.add_argument('--transducer', default='64x21x11x32,16x250x61x1024', help='N x T x U1 x V')
args = ap.parse_args()

_lib.lib(); _lib.lend_scratch(256 << 20)
NINF = float('-inf')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(legs, reps):
    """Alternating windows -> {leg: (median ms, min ms, max ms)}; a leg slower than 20 ms a call runs fewer calls per window."""
    per = {}
    for k, fn in legs.items():
        fn()                                                              # warm
        per[k] = max(1, min(reps, int(0.4 / max(window(fn, 1), 1e-5))))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(window(fn, per[k]))
    return {k: (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for k, v in times.items()}


def peak_above_baseline(fn):
    fn()
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def torch_ctc_viterbi(lp, targets, il, tl):
    """The recursion of ctc_viterbi with torch operators: lp [T, N, C] -> (scores, alignments [N, T])."""
    T, N, _ = lp.shape
    S = targets.shape[1]
    dev = lp.device
    ext = torch.zeros(N, 2 * S + 1, dtype=torch.long, device=dev)
    ext[:, 1::2] = targets
    em = lp.gather(2, ext[None].expand(T, N, 2 * S + 1))
    skip = torch.zeros(N, 2 * S + 1, dtype=torch.bool, device=dev)
    skip[:, 2:] = (ext[:, 2:] != 0) & (ext[:, 2:] != ext[:, :-2])
    state = torch.arange(2 * S + 1, device=dev)[None]
    dead = state > 2 * tl[:, None]
    ninf = torch.full((N, 2), NINF, device=dev)
    v = torch.full((N, 2 * S + 1), NINF, device=dev)
    v[:, :2] = em[0, :, :2]
    v = v.masked_fill(dead, NINF)
    back = torch.zeros(T, N, 2 * S + 1, dtype=torch.long, device=dev)
    for t in range(1, T):
        padded = torch.cat([ninf, v], 1)
        cands = torch.stack([v, padded[:, 1:-1], padded[:, :-2].masked_fill(~skip, NINF)], 0)
        best, arg = cands.max(0)                                          # the first of equal maxima: the smallest shift
        live = (t < il)[:, None]
        v = torch.where(live, (best + em[t]).masked_fill(dead, NINF), v)
        back[t] = arg
    last = torch.stack([v.gather(1, 2 * tl[:, None]), v.gather(1, (2 * tl[:, None] - 1).clamp(min=0)).masked_fill(tl[:, None] == 0, NINF)], 0)
    scores, which = last.max(0)
    s = (2 * tl[:, None] - which)
    ali = torch.full((N, T), -1, dtype=torch.long, device=dev)
    for t in range(T - 1, -1, -1):
        live = (t < il)[:, None]
        ali[:, t:t + 1] = torch.where(live, ext.gather(1, s), ali[:, t:t + 1])
        s = torch.where(live, s - back[t].gather(1, s), s)
    return scores[:, 0], ali


def torch_transducer_viterbi(joint, targets, tn, un):
    """The recursion of transducer_viterbi with torch operators, one anti-diagonal per step: -> (scores, frames [N, U])."""
    N, T, U1, _ = joint.shape
    dev = joint.device
    blank = joint[..., 0]                                                  # [N, T, U1]
    label = torch.cat([joint[:, :, :-1].gather(3, targets[:, None, :, None].expand(N, T, U1 - 1, 1))[..., 0],
                       torch.full((N, T, 1), NINF, device=dev)], 2)      # arc (t, u) -> (t, u + 1)
    u = torch.arange(U1, device=dev)
    v = torch.full((N, T, U1), NINF, device=dev)
    v[:, 0, 0] = 0.0
    from_label = torch.zeros(N, T, U1, dtype=torch.bool, device=dev)
    for d in range(1, T + U1 - 1):
        t = d - u
        ok = (t >= 0) & (t < T)
        tt, uu = t[ok], u[ok]
        a = torch.where(tt[None] >= 1, v[:, (tt - 1).clamp(min=0), uu] + blank[:, (tt - 1).clamp(min=0), uu], torch.tensor(NINF, device=dev))
        b = torch.where(uu[None] >= 1, v[:, tt, (uu - 1).clamp(min=0)] + label[:, tt, (uu - 1).clamp(min=0)], torch.tensor(NINF, device=dev))
        v[:, tt, uu] = torch.maximum(a, b)
        from_label[:, tt, uu] = b > a
    rows = torch.arange(N, device=dev)
    t, uu = (tn - 1).clamp(min=0), un.clone()
    scores = v[rows, t, uu] + blank[rows, t, uu]
    frames = torch.full((N, U1), -1, dtype=torch.long, device=dev)
    for _ in range(T + U1 - 2):
        lab = from_label[rows, t, uu]
        frames[rows, (uu - 1).clamp(min=0)] = torch.where(lab, t, frames[rows, (uu - 1).clamp(min=0)])
        uu, t = uu - lab.long(), (t - (~lab & (t > 0)).long())
    return scores, frames[:, :U1 - 1]


results = []
for shape in args.ctc.split(','):
    N, T, S, C = (int(v) for v in shape.split('x'))
    gen = torch.Generator().manual_seed(T)
    lp = (torch.randn(T, N, C, generator=gen) * 2).log_softmax(-1).cuda()
    tg = torch.randint(1, C, (N, S), generator=gen).cuda()
    il = torch.randint(T - T // 5, T + 1, (N,), generator=gen).cuda()
    tl = torch.randint(S // 2, S + 1, (N,), generator=gen).cuda()
    il[0], tl[0] = T, S
    # the two launches alone, on buffers allocated once: back to back they hide the host's side of a call
    h, ptr, stream = _lib.lib(), ops.ptr, ops._stream()
    ws = torch.empty(h.halo_ctc_viterbi_workspace_bytes(T, N, S), dtype=torch.uint8, device='cuda')
    sc, nll = torch.empty(N, device='cuda'), torch.empty(N, device='cuda')
    al = torch.empty(N, T, dtype=torch.long, device='cuda')
    first, last = torch.empty(N, S, dtype=torch.int32, device='cuda'), torch.empty(N, S, dtype=torch.int32, device='cuda')
    alpha = torch.empty(N, T, 2 * S + 1, device='cuda')
    common = (ptr(lp), lp.stride(0), lp.stride(1), T, N, C, ptr(tg), tg.stride(0), S, ptr(il), ptr(tl))
    legs = {'viterbi': lambda: ctc.ctc_viterbi(lp, tg, il, tl), 'alpha': lambda: ops.ctc_fwd(lp, True, tg, il, tl),
            'viterbi_launch': lambda: h.halo_ctc_viterbi(*common, ptr(ws), ptr(sc), ptr(al), ptr(first), ptr(last), stream),
            'alpha_launch': lambda: h.halo_ctc_fwd(*common, 0, ptr(alpha), ptr(nll), stream),
            'torch': lambda: torch_ctc_viterbi(lp, tg, il, tl)}
    a, b = legs['viterbi'](), legs['torch']()
    feasible = a[0] > NINF
    agree = float((a[1][feasible] == b[1][feasible]).float().mean())
    for k, (ms, lo, hi) in measure(legs, args.reps).items():
        results.append(dict(lattice='ctc', N=N, T=T, S=S, C=C, leg=k, ms=ms, ms_min=lo, ms_max=hi, frames_agreeing_with_torch_leg=agree))
        print(f'ctc {shape:>18s} {k:14s} {ms:9.4f} ms (min {lo:.3f} max {hi:.3f})', flush=True)
    del lp

for shape in args.transducer.split(','):
    N, T, U1, V = (int(v) for v in shape.split('x'))
    gen = torch.Generator().manual_seed(V)
    f = (torch.randn(N, T, V, generator=gen) * 2).cuda()
    g = (torch.randn(N, U1, V, generator=gen) * 2).cuda()
    tg = torch.randint(1, V, (N, U1 - 1), generator=gen).cuda()
    fl = torch.randint(max(1, T // 2), T + 1, (N,), generator=gen).int().cuda()
    tl = torch.randint(0, U1, (N,), generator=gen).int().cuda()
    fl[0], tl[0] = T, U1 - 1
    dense_route = lambda: transducer.transducer_viterbi(HF.log_softmax(f[:, :, None, :] + g[:, None, :, :]), tg, fl, tl)
    factor_route = lambda: transducer.transducer_align(f, g, tg, fl, tl)
    peak = {'route_dense': peak_above_baseline(dense_route), 'route_factors': peak_above_baseline(factor_route)}
    joint = HF.log_softmax(f[:, :, None, :] + g[:, None, :, :])
    legs = {'route_dense': dense_route, 'route_factors': factor_route,
            'viterbi': lambda: ops.transducer_viterbi(joint, tg, fl, tl, checked=True),
            'alpha': lambda: ops.transducer_fwd(joint, tg, fl, tl, checked=True),
            'torch': lambda: torch_transducer_viterbi(joint, tg, fl.long(), tl.long())}
    a, b, c = legs['viterbi'](), legs['torch'](), factor_route()
    agree = float((a[1] == b[1]).float().mean())
    agree_routes = float((a[1] == c[1]).float().mean())
    dense_bytes = N * T * U1 * V * 4
    for k, (ms, lo, hi) in measure(legs, args.reps).items():
        results.append(dict(lattice='transducer', N=N, T=T, U1=U1, V=V, leg=k, ms=ms, ms_min=lo, ms_max=hi,
                            peak_bytes_above_baseline=peak.get(k), dense_tensor_bytes=dense_bytes,
                            frames_agreeing_with_torch_leg=agree, frames_agreeing_between_routes=agree_routes))
        extra = f'  peak +{peak[k] / 1e6:9.2f} MB (one dense tensor {dense_bytes / 1e6:.1f} MB)' if k in peak else ''
        print(f'transducer {shape:>18s} {k:14s} {ms:9.3f} ms (min {lo:.3f} max {hi:.3f}){extra}', flush=True)
    del joint, f, g
    torch.cuda.empty_cache()

print(json.dumps(dict(bench='align', mode=_lib.get_math_mode(), rounds=args.rounds, reps=args.reps, results=results)))
