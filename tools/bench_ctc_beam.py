#!/usr/bin/env python3
"""CTC prefix beam search on one MI355X: haloop_amd.ctc.ctc_prefix_beam_search (csrc/ctc_prefix_beam.hip, one launch per batch) against
    greedy  ops.ctc_greedy, the head's default decoder,
    beam    ops.ctc_beam, the reference's unmerged beam (halo_ctc_beam) at the same width,
    torch   the same prefix search written with torch operators on the device and a host loop over the frames,
measured in the SAME process in alternating windows (the method of tools/bench_rnnt_beam.py).  N = 64 rows of T x V = 21 x 32 and
250 x 256 (every row at full length, capacity T), W = 4, 8 and 16, fp32.  The emissions are log_softmax of randn logits plus 3.0 on one
drawn class per frame, as the fixtures of tests/ctc_prefix_beam_ref.py.  No ratio is required of any leg: the figures are reported.
Human-readable lines, then ONE JSON line (also written to --out).

    python tools/bench_ctc_beam.py [--rounds 5] [--reps 20] [--torch-reps 1] [--legs prefix,greedy,beam,torch] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, ctc, ops

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='decodes per timed window of the library legs')
ap.add_argument('--torch-reps', type=int, default=1, help='decodes per timed window of the torch-operator search')
ap.add_argument('--shapes', default='21x32,250x256')
ap.add_argument('--beams', default='4,8,16')
ap.add_argument('--legs', default='prefix,greedy,beam,torch', help='a kernel trace of one leg: --legs prefix --rounds 1')
ap.add_argument('--out', default=None, help='also write the JSON line to this file')
args = ap.parse_args()

N = 64
NEG = float('-inf')
_lib.lib()


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def torch_prefix_beam(e, W, cap):
    """The search of include/halo.h on e [T, N, V] with torch operators, every row at full length: one pass of batched operators per
    frame, driven from the host.  topk breaks ties its own way (the kernel's order is score, then candidate position)."""
    T, n, V = e.shape
    dev = e.device
    pb = torch.full((n, W), NEG, device=dev); pb[:, 0] = 0
    pnb = torch.full((n, W), NEG, device=dev)
    tok = torch.zeros(n, W, cap, dtype=torch.int64, device=dev)
    ln = torch.zeros(n, W, dtype=torch.int64, device=dev)
    last = torch.zeros(n, W, dtype=torch.int64, device=dev)
    x = torch.arange(cap, device=dev)
    rows = torch.arange(n, device=dev)[:, None].expand(n, W)
    for t in range(T):
        et = e[t]                                                                   # [n, V]
        tot = torch.logaddexp(pb, pnb)                                              # -inf for a slot without a member
        stay_pb = tot + et[:, :1]
        stay_pnb = torch.where(ln > 0, pnb + et.gather(1, last), torch.full_like(pnb, NEG))
        ext = et[:, None, :] + tot[:, :, None]                                      # [n, W, V]
        ext.scatter_(2, last[:, :, None], (et.gather(1, last) + pb)[:, :, None])    # k == last: only the alignments ending in blank
        ext[:, :, 0] = NEG
        ext = ext.masked_fill((ln >= cap)[:, :, None], NEG)
        # y_s = y_j + [last_s]: one token longer and equal on the first len_j tokens
        eq = ((tok[:, :, None, :] == tok[:, None, :, :]) | (x >= ln[:, None, :, None])).all(3) & (ln[:, :, None] == ln[:, None, :] + 1)
        eq &= (tot > NEG)[:, :, None] & (tot > NEG)[:, None, :]
        has, j = eq.any(2), eq.int().argmax(2)                                      # [n, s]
        moved = ext[rows, j, last]
        stay_pnb = torch.where(has, torch.logaddexp(stay_pnb, moved), stay_pnb)
        ext[rows[has], j[has], last[has]] = NEG
        score = torch.cat([torch.logaddexp(stay_pb, stay_pnb), ext.reshape(n, W * V)], 1)
        best, pos = score.topk(W, dim=1)
        is_ext = pos >= W
        par = torch.where(is_ext, (pos - W) // V, pos)
        k = torch.where(is_ext, (pos - W) % V, torch.zeros_like(pos))
        pln = ln.gather(1, par)
        tok = tok.gather(1, par[:, :, None].expand(n, W, cap))
        tok = torch.where(is_ext[:, :, None] & (x == pln[:, :, None]), k[:, :, None], tok)
        pb = torch.where(is_ext, torch.full_like(best, NEG), stay_pb.gather(1, par))
        pnb = torch.where(is_ext, best, stay_pnb.gather(1, par))
        pb, pnb = pb.masked_fill(best == NEG, NEG), pnb.masked_fill(best == NEG, NEG)
        ln = torch.where(is_ext, pln + 1, pln)
        last = torch.where(is_ext, k, last.gather(1, par))
    present = best > NEG
    lengths = torch.where(present, ln, torch.full_like(ln, -1))
    tokens = tok.masked_fill(x >= lengths[:, :, None], -1)
    return tokens, lengths, best, present.sum(1)


results = []
for shape in args.shapes.split(','):
    T, V = (int(v) for v in shape.split('x'))
    gen = torch.Generator().manual_seed(T * 1000 + V)
    logits = torch.randn(T, N, V, generator=gen)
    cls = torch.randint(0, V, (T, N), generator=gen)
    logits.scatter_add_(2, cls[:, :, None], torch.full((T, N, 1), 3.0))
    e = logits.log_softmax(-1).cuda()                                   # [T, N, V], what the search reads
    lp = e.permute(1, 0, 2).contiguous()                                # [N, T, V], what greedy and the unmerged beam read
    for W in (int(w) for w in args.beams.split(',')):
        legs = {'prefix': lambda: ctc.ctc_prefix_beam_search(e, None, W), 'greedy': lambda: ops.ctc_greedy(lp),
                'beam': lambda: ops.ctc_beam(lp, W), 'torch': lambda: torch_prefix_beam(e, W, T)}
        legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
        reps = {'prefix': args.reps, 'greedy': args.reps, 'beam': args.reps, 'torch': args.torch_reps}
        out = {k: fn() for k, fn in legs.items()}                       # warm every leg
        torch.cuda.synchronize()
        r = dict(T=T, V=V, W=W)
        if 'prefix' in legs:
            tokens, lengths, scores, counts = out['prefix']
            r['best_length_mean'] = float(lengths[:, 0].float().mean())
            r['distinct_hypotheses_mean'] = float(counts.float().mean())
            if 'torch' in legs:         # random emissions have near ties that fp32 may resolve differently: reported, not required
                r['torch_agrees_rows'] = int(((out['torch'][0] == tokens).all(2).all(1) & (out['torch'][1] == lengths).all(1)).sum())
            if 'greedy' in legs:
                g_hyp, g_len = out['greedy'][2], out['greedy'][3]
                same = (g_len == lengths[:, 0]) & ((tokens[:, 0].clamp(min=0) == g_hyp) | (tokens[:, 0] < 0)).all(1)
                r['best_differs_from_greedy_rows'] = int((~same).sum())
            if 'beam' in legs:          # the unmerged beam's W outputs of a row: how many different labellings they are
                seqs, lens = out['beam'][0].cpu(), out['beam'][1].cpu()
                r['unmerged_beam_distinct_mean'] = statistics.mean(
                    len({tuple(seqs[n, w, :int(lens[n, w])].tolist()) for w in range(W)}) for n in range(N))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                    # alternating windows
            for k, fn in legs.items():
                times[k].append(window(fn, reps[k]))
        med = {k: statistics.median(times[k]) * 1e3 for k in legs}
        for k in legs:
            r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
            r[k + '_windows_ms'] = [x * 1e3 for x in times[k]]
        if 'prefix' in legs:
            for k in legs:
                if k != 'prefix':
                    r[f'prefix_over_{k}'] = med['prefix'] / med[k]
        results.append(r)
        print(f'T={T:3d} V={V:3d} W={W:2d}: ' + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})"
                                                       for k in legs)
              + '; ' + ', '.join(f'{k} {v}' for k, v in r.items() if not k.endswith(('_ms_per_batch', '_ms_min', '_ms_max', '_windows_ms'))
                                 and k not in 'TVW'), flush=True)

line = json.dumps(dict(bench='ctc_prefix_beam', N=N, mode='fp32', rounds=args.rounds, reps=args.reps, torch_reps=args.torch_reps,
                       results=results))
print(line)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
