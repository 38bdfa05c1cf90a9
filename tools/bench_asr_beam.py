#!/usr/bin/env python3
"""Beam search of the attention decoder on one MI355X: haloop_amd.transformer.BeamDecoder on its fused launches (csrc/decode.hip's
products and attention on N * W rows, csrc/decode_beam.hip's selection, one graph replay per decode) at W = 1, 4, 8 against
Decoder.decode's greedy search on its fused launches as the yardstick and against the beam's general path (torch operators, physically
gathered caches, stable sort), measured in the SAME process in alternating windows (the method of tools/bench_rnnt_beam.py).  The
`transformer:32` decoder (12 layers, 8 x 64, V = 32; untrained: oracle.transformer_ref.make_decoder_params), features [64, 10, 512],
10 steps, `bf16x3`.  Reports ms per batch of each leg and every width as a ratio to greedy from the same run.  Human-readable lines,
then ONE JSON line.

    python tools/bench_asr_beam.py [--rounds 5] [--reps 20] [--general-reps 1] [--beams 1,4,8] [--legs fused,general,greedy]
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
ap.add_argument('--reps', type=int, default=20, help='decodes per timed window of the fused legs')
ap.add_argument('--general-reps', type=int, default=1, help='decodes per timed window of the general path')
ap.add_argument('--beams', default='1,4,8')
ap.add_argument('--length-bonus', type=float, default=0.0)
ap.add_argument('--legs', default='fused,general,greedy', help='a kernel trace of one leg: --legs fused --beams 4 --rounds 1')
args = ap.parse_args()

N, S, CAPACITY, V, HD, H, L = 64, 10, 10, 32, 64, 8, 12
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


pd = ref.make_decoder_params(V, HD, H, L, 29, with_ctc=False)
dec = transformer.Decoder(vocab=V, head_dim=HD, heads=H, p_drop=0.2, layers=L)
dec.load_state_dict(pd)
dec.cuda().eval()
g = torch.Generator().manual_seed(0)
feats = torch.randn(N, S, H * HD, generator=g).cuda()
flen = torch.full((N,), S).cuda()
tl = torch.full((N,), CAPACITY - 1).cuda()          # Decoder.decode runs target_lengths.max() + 1 steps

results = []
with torch.inference_mode():
    for W in (int(w) for w in args.beams.split(',')):
        bd = transformer.BeamDecoder(dec, N, CAPACITY, W, args.length_bonus)

        def leg(fused):
            os.environ['HALO_DECODE_FUSED'] = '1' if fused else '0'
            assert bd.fused == fused
            return bd.decode(feats, flen)

        def greedy_leg():
            os.environ['HALO_DECODE_FUSED'] = '1'
            return dec.decode(feats, flen, tl, beam_size=0)
        legs = {'fused': lambda: leg(True), 'general': lambda: leg(False), 'greedy': greedy_leg}
        legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
        reps = {'fused': args.reps, 'general': args.general_reps, 'greedy': args.reps}
        out = {k: fn() for k, fn in legs.items()}                       # warm every leg (weight images, graphs)
        # an untrained model has near ties that the two paths' arithmetic may resolve differently: reported, not required
        agree = bool(torch.equal(out['fused'][0], out['general'][0])) if 'general' in legs and 'fused' in legs else None
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                    # alternating windows
            for k, fn in legs.items():
                times[k].append(window(fn, reps[k]))
        med = {k: statistics.median(times[k]) * 1e3 for k in legs}
        r = dict(W=W, paths_agree=agree, best_length_mean=float(out['fused'][1][:, 0].float().mean()) if 'fused' in legs else None,
                 finished=float(bd.last_finished.float().mean()) if bd.last_finished is not None else None,
                 fused_over_greedy=med['fused'] / med['greedy'] if 'greedy' in legs and 'fused' in legs else None,
                 general_over_fused=med['general'] / med['fused'] if 'general' in legs and 'fused' in legs else None)
        for k in legs:
            r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
        results.append(r)
        print(f"W={W}: " + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})" for k in legs)
              + f"; fused / greedy {r['fused_over_greedy']}; general / fused {r['general_over_fused']}; best hypotheses of "
              f"{r['best_length_mean']} tokens; paths agree: {agree}", flush=True)
        del bd
os.environ.pop('HALO_DECODE_FUSED', None)

print(json.dumps(dict(bench='asr_beam', N=N, S=S, capacity=CAPACITY, V=V, layers=L, heads=H, head_dim=HD, mode='bf16x3', rounds=args.rounds,
                      reps=args.reps, general_reps=args.general_reps, length_bonus=args.length_bonus, results=results)))
