#!/usr/bin/env python3
"""The waveform stage on one MI355X (haloop_amd.features.resample_batch / speed_perturb, csrc/resample.hip), measured in
the SAME process in alternating windows (the method of tools/bench_frontend.py) against the route the reference takes:

    loop     per utterance, torchaudio's own formulation on the device: pad, torch.nn.functional.conv1d with the dense [new, 1, K]
             kernel at stride orig, reshape, cut to ceil(new * len / orig); then pad_sequence.  The lengths (and, for speed, the
             factor of each utterance) are host values here, as a DataLoader would have them.
    batch    one launch on the padded batch with device lengths (speed: the factor drawn per utterance inside the launch)

Three paths -- speed_perturb with the reference's five factors, 48000 -> 16000, 22050 -> 16000 -- at N = 64 utterances of 13040 and
160000 input samples, full and ragged (lengths uniform in [0.5, 1] of the maximum); FrontEnd('mask:fbank:speed') against
FrontEnd('mask:fbank') in training mode for what the stage adds to a batch; and each launch alone on buffers allocated once.
A loop leg whose first pass takes longer than --loop-budget seconds (every new length is a new convolution shape) is left out and
reported as such.  Human-readable lines, then ONE JSON line, also written to --out.

    python tools/bench_resample.py [--rounds 5] [--reps 500] [--out profiles/resample_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pad_sequence

from haloop_amd import _lib, features, ops

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=500, help='calls per timed window (fewer for a leg slower than 0.8 ms a call)')
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', default='13040,160000')
ap.add_argument('--loop-budget', type=float, default=60.0, help='seconds a loop leg may take for its first pass')
ap.add_argument('--out', default=None)
args = ap.parse_args()

_lib.lib()
FACTORS = (0.95, 0.98, 1.0, 1.02, 1.05)
SPEED_RATIOS = [features._reduced(int(f * 16000), 16000) for f in FACTORS]
FEATURE_LAUNCH_MS = {13040: 0.025, 160000: 0.220}   # halo_features_batch alone at these shapes, printed for scale


def dense_kernel(orig, new):
    """[new, 1, K] on the device and the width, from the packed table."""
    width, stride, phases, packed = features.resample_taps(orig, new)
    dense = torch.zeros(new, 2 * width + orig)
    for p in range(new):
        lo, cnt = int(phases[0, p]), int(phases[1, p])
        dense[p, lo:lo + cnt] = packed[p, :cnt]
    return dense[:, None, :].cuda(), width


def conv_resample(x, orig, new, kernel, width):
    """One utterance [len] -> [ceil(new * len / orig)]: torchaudio's _apply_sinc_resample_kernel."""
    if orig == new:
        return x.clone()
    y = F.conv1d(F.pad(x[None, None], (width, width + orig)), kernel, stride=orig)
    return y.transpose(1, 2).reshape(-1)[:(new * x.shape[0] + orig - 1) // orig]


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(legs, reps):
    """Alternating windows -> {leg: (median ms, min ms, max ms)}."""
    per = {}
    for k, fn in legs.items():
        fn()                                                              # warm (and the tables)
        per[k] = max(1, min(reps, int(0.4 / max(window(fn, 1), 1e-5))))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(window(fn, per[k]))
    return {k: (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for k, v in times.items()}


results, skipped = [], []
N = args.batch
for samples in (int(s) for s in args.samples.split(',')):
    for ragged in (False, True):
        gen = torch.Generator().manual_seed(samples)
        wav = (0.1 * torch.randn(N, samples, generator=gen)).cuda()
        host_lengths = [samples] * N if not ragged else torch.randint(samples // 2, samples + 1, (N,), generator=gen).tolist()
        lengths = torch.tensor(host_lengths).cuda()
        host_factor = random.Random(samples).choices(range(len(FACTORS)), k=N)
        name = f'{samples}{"_ragged" if ragged else ""}'
        kernels = {r: dense_kernel(*r) for r in set(SPEED_RATIOS + [(3, 1), (441, 320)])}

        def loop_of(ratio_of):
            def loop(budget=None):
                t0, rows = time.perf_counter(), []
                for n in range(N):
                    r = ratio_of(n)
                    rows.append(conv_resample(wav[n, :host_lengths[n]], r[0], r[1], *kernels[r]))
                    if budget is not None:
                        torch.cuda.synchronize()
                        if time.perf_counter() - t0 > budget:
                            return None
                return pad_sequence(rows, batch_first=True)
            return loop

        h, ptr, stream = _lib.lib(), ops.ptr, ops._stream()
        out_len = torch.empty(N, dtype=torch.int64, device='cuda')
        idx = torch.empty(N, dtype=torch.int32, device='cuda')

        def launch_of(ratios, draw):
            desc, phases, taps = features._resample_tables(tuple(ratios), wav.device)
            L_out = max((new * samples + orig - 1) // orig for orig, new in ratios)
            out = torch.empty(N, L_out, device='cuda')
            return lambda: h.halo_resample_batch(ptr(wav), ptr(lengths), N, samples, desc, len(ratios), ptr(phases), phases.numel(), ptr(taps),
                                                 taps.numel(), None, draw, 1, 2, ptr(out), L_out, ptr(out_len), ptr(idx), stream)

        front_speed, front = features.FrontEnd('mask:fbank:speed').train(), features.FrontEnd('mask:fbank').train()
        loops = {'speed': loop_of(lambda n: SPEED_RATIOS[host_factor[n]]), 'r48000': loop_of(lambda n: (3, 1)),
                 'r22050': loop_of(lambda n: (441, 320))}
        legs = {'speed_batch': lambda: features.speed_perturb(wav, lengths, seed=1, step=2),
                'r48000_batch': lambda: features.resample_batch(wav, lengths, 48000),
                'r22050_batch': lambda: features.resample_batch(wav, lengths, 22050),
                'front_mask_fbank_speed': lambda: front_speed(wav, lengths, seed=1, step=2),
                'front_mask_fbank': lambda: front(wav, lengths, seed=1, step=2),
                'speed_launch': launch_of(SPEED_RATIOS, 1), 'r48000_launch': launch_of([(3, 1)], 0), 'r22050_launch': launch_of([(441, 320)], 0)}
        errs = {}
        for k, loop in loops.items():
            t0 = time.perf_counter()
            first = loop(budget=args.loop_budget)
            print(f'{name:>16s} {k}_loop first pass {time.perf_counter() - t0:.2f} s', flush=True)
            if first is None:
                skipped.append(dict(samples=samples, ragged=ragged, leg=f'{k}_loop', reason=f'first pass over {args.loop_budget} s'))
                continue
            legs[f'{k}_loop'] = loop
            if k != 'speed':                                 # (the loop's host factors are not the launch's draws)
                got = features.resample_batch(wav, lengths, 48000 if k == 'r48000' else 22050)[0]
                errs[k] = float((got[:, :first.shape[1]] - first).abs().max())
        m = measure(legs, args.reps)
        for k, (ms, lo, hi) in m.items():
            path = k.split('_')[0]
            ratio = m[f'{path}_loop'][0] / ms if k.endswith('_batch') and f'{path}_loop' in m else None
            results.append(dict(samples=samples, ragged=ragged, N=N, leg=k, ms=ms, ms_min=lo, ms_max=hi, loop_over_batch=ratio,
                                batch_vs_loop_max_abs=errs.get(path) if k.endswith('_batch') else None))
            note = f'  x{ratio:7.1f} of the loop' if ratio else ''
            print(f'{name:>16s} {k:24s} {ms:9.4f} ms (min {lo:.4f} max {hi:.4f}){note}', flush=True)
        print(f'{name:>16s} stage adds {m["front_mask_fbank_speed"][0] - m["front_mask_fbank"][0]:.4f} ms to a batch; batch vs loop max abs '
              f'{errs}; the feature launch it feeds: {FEATURE_LAUNCH_MS.get(samples)} ms', flush=True)
        del wav, legs, loops
        torch.cuda.empty_cache()

line = json.dumps(dict(bench='resample', rounds=args.rounds, reps=args.reps, feature_launch_ms=FEATURE_LAUNCH_MS, skipped=skipped, results=results))
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line)
