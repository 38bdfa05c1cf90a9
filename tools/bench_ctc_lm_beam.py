#!/usr/bin/env python3
"""CTC prefix beam search with LM shallow fusion on one MI355X: haloop_amd.fusion.CTCFusionDecoder on its fused launches
(csrc/ctc_lm_beam.hip: num_layers + 3 launches per frame) against
    general  the same decoder on its general path (HALO_RNNT_FUSED=0: rnn.Decoder.forward at T = 1, pruned on the host),
    prefix   ctc.ctc_prefix_beam_search at the same width, the unfused search in one launch,
    greedy   ops.ctc_greedy, the head's default decoder,
measured in the SAME process in alternating windows (the method of tools/bench_ctc_beam.py).  N = 64 rows of T x V = 21 x 32 and
250 x 256 (every row at full length, capacity T), W = 4 and 8, `bf16x3`; the LM is an untrained rnn.Decoder(V, 512, 512, 2), lm_weight 0.5.
The emissions are log_softmax of randn logits plus 3.0 on one drawn class per frame, as tools/bench_ctc_beam.py's.  No ratio is required
of any leg: the figures are reported.  Human-readable lines, then ONE JSON line (also written to --out).

    python tools/bench_ctc_lm_beam.py [--rounds 5] [--reps 5] [--general-reps 1] [--legs fused,general,prefix,greedy] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, ctc, fusion, ops, rnn

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=5, help='decodes per timed window of the library legs')
ap.add_argument('--general-reps', type=int, default=1, help='decodes per timed window of the general path')
ap.add_argument('--shapes', default='21x32,250x256')
ap.add_argument('--beams', default='4,8')
ap.add_argument('--legs', default='fused,general,prefix,greedy', help='a kernel trace of one leg: --legs fused --rounds 1')
ap.add_argument('--out', default=None, help='also write the JSON line to this file')
args = ap.parse_args()

N = 64
_lib.lib()
_lib.set_math_mode('bf16x3')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def general(dec, e, W):
    os.environ['HALO_RNNT_FUSED'] = '0'
    try:
        return dec.decode(e, None, beam=W)
    finally:
        os.environ.pop('HALO_RNNT_FUSED')


results = []
for shape in args.shapes.split(','):
    T, V = (int(v) for v in shape.split('x'))
    gen = torch.Generator().manual_seed(T * 1000 + V)
    logits = torch.randn(T, N, V, generator=gen)
    cls = torch.randint(0, V, (T, N), generator=gen)
    logits.scatter_add_(2, cls[:, :, None], torch.full((T, N, 1), 3.0))
    e = logits.log_softmax(-1).cuda()                                   # [T, N, V], what the searches read
    lp = e.permute(1, 0, 2).contiguous()                                # [N, T, V], what greedy reads
    torch.manual_seed(V)
    lm = rnn.Decoder(V, 512, 512, 2).cuda().eval()
    for W in (int(w) for w in args.beams.split(',')):
        dec = fusion.CTCFusionDecoder(lm, N, T, W, lm_weight=0.5)
        assert dec.fused
        legs = {'fused': lambda: dec.decode(e, None), 'general': lambda: general(dec, e, W),
                'prefix': lambda: ctc.ctc_prefix_beam_search(e, None, W), 'greedy': lambda: ops.ctc_greedy(lp)}
        legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
        reps = {'fused': args.reps, 'general': args.general_reps, 'prefix': args.reps, 'greedy': args.reps}
        out = {k: fn() for k, fn in legs.items()}                       # warm every leg
        torch.cuda.synchronize()
        r = dict(T=T, V=V, W=W)
        if 'fused' in legs:
            tokens, lengths, scores, counts = out['fused']
            r['best_length_mean'] = float(lengths[:, 0].float().mean())
            if 'prefix' in legs:
                r['best_differs_from_unfused_rows'] = int((~(tokens[:, 0] == out['prefix'][0][:, 0]).all(1)).sum())
            if 'general' in legs:       # random emissions have near ties that fp32 may resolve differently: reported, not required
                r['general_agrees_rows'] = int(((out['general'][0] == tokens).all(2).all(1)).sum())
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                    # alternating windows
            for k, fn in legs.items():
                times[k].append(window(fn, reps[k]))
        med = {k: statistics.median(times[k]) * 1e3 for k in legs}
        for k in legs:
            r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
            r[k + '_windows_ms'] = [x * 1e3 for x in times[k]]
        if 'fused' in legs:
            r['fused_us_per_frame'] = med['fused'] * 1e3 / T
            for k in legs:
                if k != 'fused':
                    r[f'fused_over_{k}'] = med['fused'] / med[k]
        results.append(r)
        print(f'T={T:3d} V={V:3d} W={W:2d}: ' + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})"
                                                       for k in legs)
              + '; ' + ', '.join(f'{k} {v}' for k, v in r.items() if not k.endswith(('_ms_per_batch', '_ms_min', '_ms_max', '_windows_ms'))
                                 and k not in 'TVW'), flush=True)

line = json.dumps(dict(bench='ctc_lm_beam', N=N, mode='bf16x3', lm='rnn.Decoder(V, 512, 512, 2)', lm_weight=0.5, rounds=args.rounds,
                       reps=args.reps, general_reps=args.general_reps, results=results))
print(line)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
