#!/usr/bin/env python3
"""Greedy decode of the rnn-transducer head on one MI355X: haloop_amd.transducer.GreedyDecoder on its fused launches
(csrc/rnnt_decode.hip) against its general path (rnn.Decoder.forward at T = 1 + torch log_softmax, one host read per lattice node),
measured in the SAME process in alternating windows (the method of tools/bench_gpt_generate.py).  The arch's shapes: features
[64, 21, 1024], V = 32 and 256, capacity 11, `bf16x3`.  The head is untrained: its blank bias is raised by 2 and the cap is two symbols
per frame (the setting of tests/rnnt_greedy_ref.py), without which an untrained model emits to capacity at frame 0 or never emits.
Reports ms per batch, us per iteration (fused: an advance and the prediction-network step behind it; general: a lattice node visited by
the batch in lockstep) and libhalo calls per iteration.  Human-readable lines, then ONE JSON line.

    python tools/bench_rnnt_decode.py [--rounds 5] [--reps 50]
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
ap.add_argument('--reps', type=int, default=50, help='decodes per timed window')
ap.add_argument('--vocabs', default='32,256')
args = ap.parse_args()

N, T, FEAT, CAPACITY, MAX_SYMBOLS = 64, 21, 1024, 11, 2
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


def window(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.reps


results = []
for V in (int(v) for v in args.vocabs.split(',')):
    torch.manual_seed(V)
    head = recognizer.Transducer(FEAT, V).cuda().eval()
    with torch.no_grad():
        head.classifier.bias[0] += 2.0
    features = torch.randn(N, T, FEAT, generator=torch.Generator().manual_seed(V + 1)).cuda()
    il = torch.full((N,), T, dtype=torch.int64).cuda()
    dec = transducer.GreedyDecoder(head, N, CAPACITY, MAX_SYMBOLS)

    def leg(fused):
        os.environ['HALO_RNNT_FUSED'] = '1' if fused else '0'
        assert dec.fused == fused
        return dec.decode(features, il)
    legs = {'fused': lambda: leg(True), 'general': lambda: leg(False)}
    out = {k: fn() for k, fn in legs.items()}                       # warm every leg
    # an untrained model has near ties that the two paths' arithmetic may resolve differently: reported, not required
    agree = bool(torch.equal(out['fused'][0], out['general'][0]) and torch.equal(out['fused'][2], out['general'][2]))
    iters, calls = {}, {}
    for k, fn in legs.items():
        calls[k] = count_calls(fn)
        iters[k] = dec.iterations
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                                      # alternating windows
        for k, fn in legs.items():
            times[k].append(window(fn))
    for k in legs:
        ms = statistics.median(times[k]) * 1e3
        r = dict(V=V, leg=k, ms_per_batch=ms, ms_min=min(times[k]) * 1e3, ms_max=max(times[k]) * 1e3, iterations=iters[k],
                 us_per_iteration=ms * 1e3 / iters[k], libhalo_calls_per_iteration=calls[k] / iters[k],
                 symbols_per_row=float(out[k][1].float().mean()), truncated_rows=int(out[k][4].sum()), paths_agree=agree)
        results.append(r)
        print(f"V={V:3d} {k:7s} {ms:8.3f} ms/batch (min {r['ms_min']:.3f} max {r['ms_max']:.3f})  {iters[k]:3d} iterations, "
              f"{r['us_per_iteration']:.1f} us each, {r['libhalo_calls_per_iteration']:.1f} libhalo calls each; "
              f"{r['symbols_per_row']:.1f} symbols per row, {r['truncated_rows']} rows truncated; paths agree: {agree}", flush=True)
    del dec, head
os.environ.pop('HALO_RNNT_FUSED', None)

print(json.dumps(dict(bench='rnnt_decode', N=N, T=T, feat=FEAT, capacity=CAPACITY, max_symbols_per_frame=MAX_SYMBOLS, mode='bf16x3',
                      rounds=args.rounds, reps=args.reps, results=results)))
