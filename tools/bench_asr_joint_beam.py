#!/usr/bin/env python3
"""Joint CTC/attention beam search on one MI355X: CTCAttentionDecoder.decode(beam_size=W, ctc_weight=0.3, joint=True) --
the fused decode launches plus csrc/ctc_prefix_score.hip's scores and advance and the joint selection every step -- against the
attention-only BeamDecoder search followed by the CTC head's re-ranking of the finished lists (joint=False), measured in the SAME process
in alternating windows (the method of tools/bench_asr_beam.py).  Two more legs time BeamDecoder.decode alone, with and without the CTC
log-probabilities: their difference over the step count is what the three new launches add to a step.  The `transformer:32` decoder (12
layers, 8 x 64, V = 32; untrained: oracle.transformer_ref.make_decoder_params) with its CTC head, features [64, S, 512], 10 steps,
`bf16x3`; rows (S, W) = (10, 4), (10, 8) and (125, 4), the last at a realistic utterance length.  Human-readable lines, then ONE JSON line.

    python tools/bench_asr_joint_beam.py [--rounds 5] [--reps 20] [--rows 10:4,10:8,125:4] [--legs joint,rerank,joint_search,plain_search]

The kernels of a step, in a run of its own (eager launches, one leg, one row):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_asr_joint_beam.py --eager --legs joint_search --rows 10:4 --rounds 1
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, transformer
from oracle import transformer_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='decodes per timed window')
ap.add_argument('--rows', default='10:4,10:8,125:4', help='S:W pairs')
ap.add_argument('--ctc-weight', type=float, default=0.3)
ap.add_argument('--legs', default='joint,rerank,joint_search,plain_search')
ap.add_argument('--eager', action='store_true', help='HALO_DECODE_GRAPH=0: every launch appears in a kernel trace under its own name')
args = ap.parse_args()

N, CAPACITY, V, HD, H, L = 64, 10, 32, 64, 8, 12
if args.eager:
    os.environ['HALO_DECODE_GRAPH'] = '0'
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


model = transformer.CTCAttentionDecoder(vocab=V, head_dim=HD, heads=H, p_drop=0.2, layers=L)
model.load_state_dict(ref.make_decoder_params(V, HD, H, L, 29))
model.cuda().eval()
dec, c = model.decoder, args.ctc_weight
tl = torch.full((N,), CAPACITY - 1).cuda()          # Decoder.decode runs target_lengths.max() + 1 steps

results = []
with torch.inference_mode():
    for S, W in ((int(a), int(b)) for a, b in (row.split(':') for row in args.rows.split(','))):
        g = torch.Generator().manual_seed(S)
        feats = torch.randn(N, S, H * HD, generator=g).cuda()
        flen = torch.full((N,), S).cuda()
        lp = model.recognizer.log_probs(feats).float()
        bd = transformer.BeamDecoder(dec, N, CAPACITY, W, 0.0)
        legs = {'joint': lambda: model.decode(feats, flen, tl, beam_size=W, ctc_weight=c, joint=True),
                'rerank': lambda: model.decode(feats, flen, tl, beam_size=W, ctc_weight=c, joint=False),
                'joint_search': lambda: bd.decode(feats, flen, ctc_log_probs=lp, ctc_weight=c),
                'plain_search': lambda: bd.decode(feats, flen)}
        legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
        for fn in legs.values():                                        # warm every leg (weight images, graphs)
            fn()
        r = dict(S=S, W=W)
        if 'joint' in legs and 'rerank' in legs:                        # how often the one-pass search finds another best hypothesis
            legs['joint'](); a = model.last_nbest[0][:, 0].clone()
            legs['rerank'](); r['best_differs'] = float((a != model.last_nbest[0][:, 0]).any(1).float().mean())
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                    # alternating windows
            for k, fn in legs.items():
                times[k].append(window(fn, args.reps))
        med = {k: statistics.median(times[k]) * 1e3 for k in legs}
        for k in legs:
            r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
        r['joint_over_rerank'] = med['joint'] / med['rerank'] if 'joint' in legs and 'rerank' in legs else None
        if 'joint_search' in legs and 'plain_search' in legs:
            r['search_ratio'] = med['joint_search'] / med['plain_search']
            r['plain_step_us'] = med['plain_search'] * 1e3 / CAPACITY
            r['prefix_us_per_step'] = (med['joint_search'] - med['plain_search']) * 1e3 / CAPACITY
        results.append(r)
        print(f"S={S} W={W}: " + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})" for k in legs)
              + f"; joint / rerank {r['joint_over_rerank']}; joint / plain search {r.get('search_ratio')}; the three launches add "
              f"{r.get('prefix_us_per_step')} us to a step of {r.get('plain_step_us')} us; best hypothesis differs in "
              f"{r.get('best_differs')} of the rows", flush=True)
        del bd

print(json.dumps(dict(bench='asr_joint_beam', N=N, capacity=CAPACITY, V=V, layers=L, heads=H, head_dim=HD, mode='bf16x3', rounds=args.rounds,
                      reps=args.reps, ctc_weight=c, eager=args.eager, results=results)))
