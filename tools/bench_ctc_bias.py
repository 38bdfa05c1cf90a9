#!/usr/bin/env python3
"""Contextual biasing inside the CTC prefix beam search on one MI355X: ctc.ctc_prefix_beam_search(context=graph) against the unbiased
ctc.ctc_prefix_beam_search, and the carried biased launch (ctc.PrefixBeamStream(context=graph).advance) against the carried unbiased
one at chunks of 16 frames, measured in the SAME process in alternating windows (the method of tools/bench_ctc_beam.py).  N = 64 rows of
T x V = 21 x 32 and 250 x 256 (every row at full length, capacity T), W = 4 and 8, graphs of 16 and 256 phrases of 2 to 4 tokens drawn
over the labels, bonus 1.5, fp32.  The emissions are those of tools/bench_ctc_beam.py.  No ratio is required: the figures are reported.

The structural claims are checked here, not timed: the library calls of one biased search and of one biased ``advance`` are counted
(every entry point of libhalo that returns a status is one launch sequence; the searches' are one kernel each), and both run under
``torch.cuda.set_sync_debug_mode('error')``, which raises on any read from the device.
Human-readable lines, then ONE JSON line (also written to --out).

    python tools/bench_ctc_bias.py [--rounds 5] [--reps 20] [--out FILE]
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
from haloop_amd.biasing import ContextGraph

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='decodes per timed window')
ap.add_argument('--shapes', default='21x32,250x256')
ap.add_argument('--beams', default='4,8')
ap.add_argument('--phrases', default='16,256')
ap.add_argument('--chunk', type=int, default=16)
ap.add_argument('--out', default=None, help='also write the JSON line to this file')
args = ap.parse_args()

N, BONUS = 64, 1.5
_lib.lib()


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


class CountingLib:
    """libhalo with every call counted by name (size queries too; they launch nothing and are told apart by their names)."""

    def __init__(self, handle):
        self.handle, self.calls = handle, []

    def __getattr__(self, name):
        fn = getattr(self.handle, name)

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def launches_and_reads(fn):
    """fn() with the library calls counted and any read from the device an error -> the launching calls' names."""
    counting = CountingLib(_lib.lib())
    real = ops.lib
    ops.lib = lambda: counting
    torch.cuda.set_sync_debug_mode('error')
    try:
        fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
        ops.lib = real
    return [c for c in counting.calls if not c.endswith('_bytes')]


def phrase_list(count, V, gen):
    out = set()
    while len(out) < count:
        n = int(torch.randint(2, 5, (1,), generator=gen))
        out.add(tuple(int(k) for k in torch.randint(1, V, (n,), generator=gen)))
    return sorted(out)


results = []
for shape in args.shapes.split(','):
    T, V = (int(v) for v in shape.split('x'))
    gen = torch.Generator().manual_seed(T * 1000 + V)
    logits = torch.randn(T, N, V, generator=gen)
    cls = torch.randint(0, V, (T, N), generator=gen)
    logits.scatter_add_(2, cls[:, :, None], torch.full((T, N, 1), 3.0))
    e = logits.log_softmax(-1).cuda()                                   # [T, N, V]
    chunks = [e[off:off + args.chunk] for off in range(0, T, args.chunk)]
    begin = torch.ones(N, dtype=torch.bool, device='cuda')
    for P in (int(p) for p in args.phrases.split(',')):
        graph = ContextGraph(phrase_list(P, V, gen), V, BONUS)
        graph.to(e.device)
        for W in (int(w) for w in args.beams.split(',')):
            plain_stream = ctc.PrefixBeamStream(N, V, W, T, device='cuda')
            biased_stream = ctc.PrefixBeamStream(N, V, W, T, device='cuda', context=graph)

            def carried(stream):
                for i, chunk in enumerate(chunks):
                    stream.advance(chunk, None, begin if i == 0 else None)

            legs = {'unbiased': lambda: ctc.ctc_prefix_beam_search(e, None, W),
                    'biased': lambda: ctc.ctc_prefix_beam_search(e, None, W, context=graph, return_parts=True),
                    'carried_unbiased': lambda: carried(plain_stream), 'carried_biased': lambda: carried(biased_stream)}
            out = {k: fn() for k, fn in legs.items()}                   # warm every leg
            torch.cuda.synchronize()
            whole_calls = launches_and_reads(legs['biased'])
            advance_calls = launches_and_reads(lambda: biased_stream.advance(chunks[-1]))
            assert whole_calls == ['halo_ctc_prefix_beam_biased'], whole_calls
            assert advance_calls == ['halo_ctc_prefix_beam_advance_biased'], advance_calls
            legs['carried_biased']()
            assert all(torch.equal(a, b) for a, b in zip(biased_stream.nbest() + biased_stream.parts(), out['biased']))
            tokens, lengths, scores, counts, boosts, states = out['biased']
            r = dict(T=T, V=V, W=W, phrases=P, states=graph.num_states, columns=graph.num_columns, table_bytes=8 * graph.next.numel(),
                     calls=len(chunks), launches_per_search=len(whole_calls), launches_per_advance=len(advance_calls), device_reads=0,
                     best_differs_from_unbiased_rows=int((out['unbiased'][0][:, 0] != tokens[:, 0]).any(1).sum()),
                     best_boost_mean=float(boosts[:, 0].mean()))
            times = {k: [] for k in legs}
            for _ in range(args.rounds):                                # alternating windows
                for k, fn in legs.items():
                    times[k].append(window(fn, args.reps))
            med = {k: statistics.median(times[k]) * 1e3 for k in legs}
            for k in legs:
                r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
                r[k + '_windows_ms'] = [x * 1e3 for x in times[k]]
            r['biased_over_unbiased'] = med['biased'] / med['unbiased']
            r['carried_biased_over_carried_unbiased'] = med['carried_biased'] / med['carried_unbiased']
            results.append(r)
            print(f'T={T:3d} V={V:3d} W={W:2d} phrases={P:3d} (states {graph.num_states}, columns {graph.num_columns}): '
                  + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})" for k in legs)
                  + f"; biased/unbiased {r['biased_over_unbiased']:.3f}, carried {r['carried_biased_over_carried_unbiased']:.3f}"
                  + f"; best differs in {r['best_differs_from_unbiased_rows']} rows, mean best boost {r['best_boost_mean']:.2f}", flush=True)

line = json.dumps(dict(bench='ctc_context_bias', N=N, mode='fp32', rounds=args.rounds, reps=args.reps, chunk=args.chunk, bonus=BONUS,
                       results=results))
print(line)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
