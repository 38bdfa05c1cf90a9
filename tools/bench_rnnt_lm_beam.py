#!/usr/bin/env python3
"""Transducer beam search with LM shallow fusion on one MI355X: haloop_amd.fusion.TransducerFusionDecoder on its fused launches
(csrc/rnnt_lm_beam.hip: Lp + Ll + 5 launches per alignment step) against
    general  the same decoder on its general path (HALO_RNNT_FUSED=0: rnn.Decoder.forward at T = 1 for both networks, pruned on the host),
    beam     transducer.BeamDecoder.decode at the same width, the unfused search (Lp + 3 launches per alignment step),
    rescore  BeamDecoder.decode followed by fusion.lm_score on its lists, the route the fused search replaces,
measured in the SAME process in alternating windows (the method of tools/bench_rnnt_beam.py).  Features [64, 21, 1024] with the planted
symbols of tools/bench_rnnt_beam.py, an untrained Transducer head, V = 32 and 256, capacity 11, W = 4 and 8, `bf16x3`; the LM is an
untrained rnn.Decoder(V, 512, 512, 2), lm_weight 0.5, insertion_bonus round(0.5 ln V, 1) (without a bonus an untrained LM empties the
lists).  Reports ms per batch of each leg, the fused search's cost per alignment step over the unfused search's, and the libhalo calls
of one fused decode by entry point.  No ratio is required of any leg: the figures are reported.  Human-readable lines, then ONE JSON
line (also written to --out).

    python tools/bench_rnnt_lm_beam.py [--rounds 5] [--reps 10] [--general-reps 1] [--legs fused,general,beam,rescore] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, fusion, recognizer, rnn, transducer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=10, help='decodes per timed window of the library legs')
ap.add_argument('--general-reps', type=int, default=1, help='decodes per timed window of the general path')
ap.add_argument('--vocabs', default='32,256')
ap.add_argument('--beams', default='4,8')
ap.add_argument('--legs', default='fused,general,beam,rescore', help='a kernel trace of one leg: --legs fused --rounds 1')
ap.add_argument('--out', default=None, help='also write the JSON line to this file')
args = ap.parse_args()

N, T, FEAT, CAPACITY = 64, 21, 1024, 11
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def count_calls(fn):
    """libhalo calls of one fn(), by entry point."""
    lib = _lib.lib()
    names = [n for n in _lib.SIGNATURES if not n.endswith(('_bytes', '_supported')) and 'math_mode' not in n]
    orig = {n: getattr(lib, n) for n in names}
    seen = {}

    def wrap(n, f):
        def g(*a):
            seen[n] = seen.get(n, 0) + 1
            return f(*a)
        return g
    for n, f in orig.items():
        setattr(lib, n, wrap(n, f))
    try:
        fn()
    finally:
        for n, f in orig.items():
            setattr(lib, n, f)
    return seen


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def planted(gen, V):
    x = torch.randn(N, T, FEAT, generator=gen)
    lab = torch.randint(1, V, (N, T), generator=gen)
    is_lab = torch.rand(N, T, generator=gen) < 0.25
    ch = torch.where(is_lab, lab, torch.zeros_like(lab))
    x.scatter_add_(2, ch[:, :, None], torch.full((N, T, 1), 7.0))
    x[:, :, 0] += 4.5
    return x


results = []
for V in (int(v) for v in args.vocabs.split(',')):
    torch.manual_seed(V)
    head = recognizer.Transducer(FEAT, V).cuda().eval()
    with torch.no_grad():
        head.classifier.weight.copy_(torch.eye(V, FEAT))
        head.classifier.bias.zero_()
    lm = rnn.Decoder(V, 512, 512, 2).cuda().eval()
    features = planted(torch.Generator().manual_seed(V + 1), V).cuda()
    il = torch.full((N,), T, dtype=torch.int64).cuda()
    a, b = 0.5, round(0.5 * math.log(V), 1)
    for W in (int(w) for w in args.beams.split(',')):
        dec = fusion.TransducerFusionDecoder(head, lm, N, CAPACITY, W, a, b)
        plain = transducer.BeamDecoder(head, N, CAPACITY, W)

        def leg(fused):
            os.environ['HALO_RNNT_FUSED'] = '1' if fused else '0'
            assert dec.fused == fused
            return dec.decode(features, il)

        def beam_leg():
            os.environ['HALO_RNNT_FUSED'] = '1'
            assert plain.fused
            return plain.decode(features, il)

        def rescore_leg():
            out = beam_leg()
            return out, fusion.lm_score(lm, out[0], out[1])
        legs = {'fused': lambda: leg(True), 'general': lambda: leg(False), 'beam': beam_leg, 'rescore': rescore_leg}
        legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
        reps = {'fused': args.reps, 'general': args.general_reps, 'beam': args.reps, 'rescore': args.reps}
        out = {k: fn() for k, fn in legs.items()}                       # warm every leg
        torch.cuda.synchronize()
        r = dict(V=V, W=W, lm_weight=a, insertion_bonus=b)
        if 'fused' in legs:
            tokens, lengths, scores, counts = out['fused']
            calls = count_calls(legs['fused'])
            steps = dec.iterations
            r.update(alignment_steps=steps, libhalo_calls=calls, libhalo_calls_per_alignment_step=sum(calls.values()) / steps,
                     best_length_mean=float(lengths[:, 0].float().mean()))
            if 'beam' in legs:
                r['best_differs_from_unfused_rows'] = int((~(tokens[:, 0] == out['beam'][0][:, 0]).all(1)).sum())
                r['unfused_alignment_steps'] = plain.iterations
            if 'general' in legs:       # an untrained model has near ties that the two paths may resolve differently: reported, not required
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
            r['fused_us_per_alignment_step'] = med['fused'] * 1e3 / steps
            for k in legs:
                if k != 'fused':
                    r[f'fused_over_{k}'] = med['fused'] / med[k]
            if 'beam' in legs:
                r['beam_us_per_alignment_step'] = med['beam'] * 1e3 / plain.iterations
                r['fusion_us_per_alignment_step'] = r['fused_us_per_alignment_step'] - r['beam_us_per_alignment_step']
        results.append(r)
        print(f'V={V:3d} W={W:2d}: ' + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})"
                                               for k in legs)
              + '; ' + ', '.join(f'{k} {v}' for k, v in r.items() if not k.endswith(('_ms_per_batch', '_ms_min', '_ms_max', '_windows_ms'))
                                 and k not in 'VW'), flush=True)
        del dec, plain
    del head, lm
os.environ.pop('HALO_RNNT_FUSED', None)

line = json.dumps(dict(bench='rnnt_lm_beam', N=N, T=T, feat=FEAT, capacity=CAPACITY, mode='bf16x3', lm='rnn.Decoder(V, 512, 512, 2)',
                       rounds=args.rounds, reps=args.reps, general_reps=args.general_reps, results=results))
print(line)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
