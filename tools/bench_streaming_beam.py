#!/usr/bin/env python3
"""Streaming CTC prefix beam search on one MI355X (haloop_amd/streaming.py StreamingRecognizer(beam=W), ctc.PrefixBeamStream,
csrc/ctc_prefix_beam.hip halo_ctc_prefix_beam_advance): ms per push of 64 streams on LC-2x1024 (F = 80, C = 128,
H = 1024, L = 2, V = 32) in `bf16` and `bf16x3`, at widths 4 and 8 and chunk_frames 16, 32 and 64 (S = 4, 8, 16 steps a call), measured
in the SAME process in alternating windows (the method of tools/bench_streaming.py):

    greedy           (a) the greedy push (beam=0), launched eagerly (the default)
    beam             the push with the beam's launch behind the head, launched eagerly
    greedy_graph /   the same two replayed from one HIP graph (use_graph=True)
    beam_graph
    advance          (c) halo_ctc_prefix_beam_advance alone on the push's log-probs, the beam carried from call to call
    advance_begin    (c') the same launch with every row beginning: the search of (d) plus the state's store
    oneshot          (d) halo_ctc_prefix_beam alone on the same S steps: what the search costs without a carried state
    prefix_80 /      (b) the only route before: ctc.ctc_prefix_beam_search over the accumulated log-probs, at prefixes of 80 and 1000
    prefix_1000      frames (20 and 250 steps); per width, the log-probs are fp32 in every mode

A stream is begun again every 16th call in the legs that carry a beam (and in the greedy leg, for the same host work), so the
hypotheses stay below the capacity of 256 as they do in an utterance of 16 chunks; a beam left to run into its capacity takes no
extensions and would time a cheaper frame.  (c), (c') and (d) are bare C calls on buffers allocated once, so their host cost is the
same.  No ratio is required of any leg: the figures are reported.  Human-readable lines, then ONE JSON line, also written to --out.

    python tools/bench_streaming_beam.py [--rounds 5] [--reps 200] [--out profiles/streaming_beam_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, ctc, ops, recognizer, rnn, streaming, synth

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=200, help='calls per timed window (fewer for a leg slower than 2 ms a call)')
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--chunks', default='16,32,64')
ap.add_argument('--widths', default='4,8')
ap.add_argument('--modes', default='bf16,bf16x3')
ap.add_argument('--out', default=None)
args = ap.parse_args()

lib = _lib.lib()
F_, C, H, L, V, B = 80, 128, 1024, 2, 32, args.batch
CAPACITY, UTTERANCE = 256, 16           # the longest hypothesis; calls between two begins
ptr, stream_of = ops.ptr, ops._stream


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
        fn(); fn()                                                        # warm (a graph leg captures here)
        per[k] = max(1, min(reps, int(0.4 / max(window(fn, 1), 1e-5))))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(window(fn, per[k]))
    return {k: (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for k, v in times.items()}


enc_p, rec_p = synth.make_params(F_, C, H, L, V, 42)
enc, rec = rnn.Encoder(F_, C, H, num_layers=L), recognizer.TemporalClassifier(H, V)
enc.load_state_dict(enc_p); rec.load_state_dict(rec_p)
enc.cuda().eval(); rec.cuda().eval()
audio = torch.randn(B, 1000, F_, generator=torch.Generator().manual_seed(43)).cuda()
ALL, NONE = [True] * B, [False] * B


def push_leg(chunk, W, frames, graph):
    sr = streaming.StreamingRecognizer(enc, rec, B, chunk_frames=chunk, capacity=CAPACITY, use_graph=graph, beam=W)
    calls = [0]

    def run():
        sr.push(frames, ALL, ALL if calls[0] % UTTERANCE == 0 else NONE)
        calls[0] += 1
    return run


def launch_legs(lp, W):
    """(c), (c') and (d) on the log-probs lp [B, S, V] of one push, read in place as [S, B, V]."""
    S = lp.shape[1]
    em = lp.permute(1, 0, 2)
    bs = ctc.PrefixBeamStream(B, V, W, CAPACITY, device=lp.device)
    begin = torch.full((B,), ops.STREAM_BEGIN, dtype=torch.int32, device=lp.device)
    one = [torch.empty(B, W, S, dtype=torch.int64, device=lp.device), torch.empty(B, W, dtype=torch.int64, device=lp.device),
           torch.empty(B, W, device=lp.device), torch.empty(B, dtype=torch.int64, device=lp.device)]
    adv = lambda flags: lib.halo_ctc_prefix_beam_advance(ptr(em), em.stride(0), em.stride(1), S, B, V, None, ptr(flags), W, CAPACITY,
                                                         ptr(bs.state), ptr(bs.tokens), ptr(bs.lengths), ptr(bs.scores), ptr(bs.counts),
                                                         stream_of())
    calls = [0]

    def carried():
        assert adv(begin if calls[0] % UTTERANCE == 0 else None) == 0
        calls[0] += 1

    def beginning():
        assert adv(begin) == 0

    def oneshot():
        assert lib.halo_ctc_prefix_beam(ptr(em), em.stride(0), em.stride(1), S, B, V, None, W, S, None, ptr(one[0]), ptr(one[1]), ptr(one[2]),
                                        ptr(one[3]), stream_of()) == 0
    return {'advance': carried, 'advance_begin': beginning, 'oneshot': oneshot}, (bs, begin, one, em)


results = []
widths = [int(w) for w in args.widths.split(',')]
for mode in args.modes.split(','):
    _lib.set_math_mode(mode)
    for chunk in (int(c) for c in args.chunks.split(',')):
        frames = audio[:, 100:100 + chunk].contiguous()
        probe = streaming.StreamingRecognizer(enc, rec, B, chunk_frames=chunk, capacity=CAPACITY, use_graph=False, beam=0)
        probe.push(frames, ALL, ALL, want_log_probs=True)
        lp = probe.last[3].clone()
        for W in widths:
            legs = {'greedy': push_leg(chunk, 0, frames, False), 'beam': push_leg(chunk, W, frames, False),
                    'greedy_graph': push_leg(chunk, 0, frames, True), 'beam_graph': push_leg(chunk, W, frames, True)}
            alone, keep = launch_legs(lp, W)
            legs.update(alone)
            m = measure(legs, args.reps)
            for k, (ms, lo, hi) in m.items():
                results.append(dict(mode=mode, chunk_frames=chunk, steps=chunk // 4, W=W, B=B, leg=k, ms=ms, ms_min=lo, ms_max=hi))
                print(f'{mode:>7s} chunk {chunk:3d} W {W:2d} {k:14s} {ms:8.4f} ms (min {lo:.4f} max {hi:.4f})', flush=True)
            del legs, alone, keep

# (b) the route before: the whole search over the accumulated log-probs of 80 and 1000 frames (the log-probs of one chunk, repeated)
for W in widths:
    legs = {}
    for frames_so_far in (80, 1000):
        steps = frames_so_far // 4
        e = lp.permute(1, 0, 2).repeat((steps + lp.shape[1] - 1) // lp.shape[1], 1, 1)[:steps].contiguous()
        legs[f'prefix_{frames_so_far}'] = lambda e=e, W=W, steps=steps: ctc.ctc_prefix_beam_search(e, None, W, min(CAPACITY, steps))
    m = measure(legs, args.reps)
    for k, (ms, lo, hi) in m.items():
        results.append(dict(mode='fp32', W=W, B=B, leg=k, ms=ms, ms_min=lo, ms_max=hi))
        print(f'   fp32           W {W:2d} {k:14s} {ms:8.4f} ms (min {lo:.4f} max {hi:.4f})', flush=True)

state_bytes = {W: ops.ctc_prefix_beam_state_bytes(V, W, CAPACITY) for W in widths}
line = json.dumps(dict(bench='streaming_beam', rounds=args.rounds, reps=args.reps, capacity=CAPACITY, calls_per_begin=UTTERANCE,
                       state_bytes_per_row=state_bytes, results=results))
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line)
