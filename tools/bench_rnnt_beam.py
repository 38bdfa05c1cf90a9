#!/usr/bin/env python3
"""Beam search of the rnn-transducer head on one MI355X: haloop_amd.transducer.BeamDecoder on its fused launches (csrc/rnnt_beam.hip)
against its general path (rnn.Decoder.forward at T = 1 over N * W rows, pruned on the host) and against transducer.GreedyDecoder on its
fused launches as the yardstick, measured in the SAME process in alternating windows (the method of tools/bench_rnnt_decode.py).  The
arch's shapes: features [64, 21, 1024], V = 32 and 256, capacity 11, W = 4 and 8, `bf16x3`.  The head is untrained; the features carry
planted symbols as the fixtures of tests/rnnt_beam_ref.py do (the classifier reads the first V channels: randn, plus 7.0 on a drawn
label channel in a quarter of the frames and on the blank channel elsewhere, plus 4.5 on the blank channel everywhere).
Reports ms per batch of each leg, the beam's cost as a multiple of greedy's, alignment steps taken and libhalo calls per alignment
step.  Human-readable lines, then ONE JSON line.

    python tools/bench_rnnt_beam.py [--rounds 5] [--reps 20] [--general-reps 1] [--legs fused,general,greedy]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, recognizer, transducer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='decodes per timed window of the fused legs')
ap.add_argument('--general-reps', type=int, default=1, help='decodes per timed window of the general path')
ap.add_argument('--vocabs', default='32,256')
ap.add_argument('--beams', default='4,8')
ap.add_argument('--legs', default='fused,general,greedy', help='a kernel trace of one leg: --legs fused --rounds 1')
args = ap.parse_args()

N, T, FEAT, CAPACITY = 64, 21, 1024, 11
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def count_calls(fn):
    lib = _lib.lib()
    names = [n for n in _lib.SIGNATURES if not n.endswith(('_bytes', '_supported')) and 'math_mode' not in n]
    orig = {n: getattr(lib, n) for n in names}
    total = [0]

    def wrap(f):
        def g(*a):
            total[0] += 1
            return f(*a)
        return g
    for n, f in orig.items():
        setattr(lib, n, wrap(f))
    try:
        fn()
    finally:
        for n, f in orig.items():
            setattr(lib, n, f)
    return total[0]


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
    features = planted(torch.Generator().manual_seed(V + 1), V).cuda()
    il = torch.full((N,), T, dtype=torch.int64).cuda()
    greedy = transducer.GreedyDecoder(head, N, CAPACITY)
    for W in (int(w) for w in args.beams.split(',')):
        dec = transducer.BeamDecoder(head, N, CAPACITY, W)

        def leg(fused):
            os.environ['HALO_RNNT_FUSED'] = '1' if fused else '0'
            assert dec.fused == fused
            return dec.decode(features, il)

        def greedy_leg():
            os.environ['HALO_RNNT_FUSED'] = '1'
            assert greedy.fused
            return greedy.decode(features, il)
        legs = {'fused': lambda: leg(True), 'general': lambda: leg(False), 'greedy': greedy_leg}
        legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
        reps = {'fused': args.reps, 'general': args.general_reps, 'greedy': args.reps}
        out = {k: fn() for k, fn in legs.items()}                       # warm every leg
        # an untrained model has near ties that the two paths' arithmetic may resolve differently: reported, not required
        agree = bool(torch.equal(out['fused'][0], out['general'][0])) if 'general' in legs else None
        differs = int((out['fused'][1][:, 0] != out['greedy'][1]).sum()
                      + ((out['fused'][1][:, 0] == out['greedy'][1])
                         & (out['fused'][0][:, 0] != out['greedy'][0]).any(1)).sum()) if 'greedy' in legs else None
        calls = count_calls(legs['fused'])
        steps = dec.iterations
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                    # alternating windows
            for k, fn in legs.items():
                times[k].append(window(fn, reps[k]))
        med = {k: statistics.median(times[k]) * 1e3 for k in legs}
        r = dict(V=V, W=W, paths_agree=agree, best_differs_from_greedy_rows=differs, alignment_steps=steps,
                 libhalo_calls_per_alignment_step=calls / steps, best_length_mean=float(out['fused'][1][:, 0].float().mean()),
                 fused_over_greedy=med['fused'] / med['greedy'] if 'greedy' in legs else None,
                 general_over_fused=med['general'] / med['fused'] if 'general' in legs else None)
        for k in legs:
            r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
        results.append(r)
        print(f"V={V:3d} W={W}: " + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})" for k in legs)
              + f"; fused / greedy {r['fused_over_greedy']}; {steps} alignment steps, {r['libhalo_calls_per_alignment_step']:.2f} libhalo "
              f"calls each; best hypotheses of {r['best_length_mean']:.1f} symbols, {differs} rows differ from greedy; paths agree: "
              f"{agree}", flush=True)
        del dec
    del greedy, head
os.environ.pop('HALO_RNNT_FUSED', None)

print(json.dumps(dict(bench='rnnt_beam', N=N, T=T, feat=FEAT, capacity=CAPACITY, mode='bf16x3', rounds=args.rounds, reps=args.reps,
                      general_reps=args.general_reps, results=results)))
