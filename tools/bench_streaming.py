#!/usr/bin/env python3
"""Streaming LSTM-CTC recognition on one MI355X (haloop_amd/streaming.py, csrc/stream.hip): ms per push of 64 streams
on LC-2x1024 (F = 80, C = 128, H = 1024, L = 2, V = 32) in `bf16` and `bf16x3`, measured in the SAME process in alternating windows
(the method of tools/bench_frontend.py):

    fused_graph     halo_stream_front + ops.lstm_fwd + halo_stream_head replayed from one HIP graph
    fused_eager     the same launches issued eagerly
    general         HALO_STREAM_FUSED=0: torch.cat + ops.subsample_fwd + ops.lstm_fwd + ops.gemm + ops.log_softmax_fwd + ops.ctc_greedy
                    and torch operators for the merging
    prefix_80 /     the only route without streaming: infer.LstmCtcRecognizer.recognize on the whole prefix so far, at prefixes of 80
    prefix_1000     and 1000 frames

at chunk_frames 16, 32 and 64, and the total for an 80-frame utterance streamed as 5 pushes and a finish against ONE recognize call (the
price of streaming).  The real-time factor is ms of audio (10 ms a frame) per ms of compute, times the 64 streams.  Human-readable
lines, then ONE JSON line, also written to --out.

    python tools/bench_streaming.py [--rounds 5] [--reps 200] [--out profiles/streaming_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, infer, recognizer, rnn, streaming, synth

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=200, help='calls per timed window (fewer for a leg slower than 2 ms a call)')
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--chunks', default='16,32,64')
ap.add_argument('--modes', default='bf16,bf16x3')
ap.add_argument('--out', default=None)
args = ap.parse_args()

_lib.lib()
F_, C, H, L, V, B = 80, 128, 1024, 2, 32, args.batch
FRAME_MS = 10.0


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
gen = torch.Generator().manual_seed(43)
audio = torch.randn(B, 1000, F_, generator=gen).cuda()
ALL, NONE = [True] * B, [False] * B


def recognizer_of(chunk, fused, graph):
    sr = streaming.StreamingRecognizer(enc, rec, B, chunk_frames=chunk, capacity=256, use_graph=graph)
    sr.fused = fused
    sr.push(audio[:, :chunk].contiguous(), ALL, ALL)
    return sr


results = []
for mode in args.modes.split(','):
    _lib.set_math_mode(mode)
    whole = infer.LstmCtcRecognizer(enc, rec)
    whole1000 = infer.LstmCtcRecognizer(enc, rec)
    x80, x1000 = audio[:, :80].contiguous(), audio
    for chunk in (int(c) for c in args.chunks.split(',')):
        frames = audio[:, 100:100 + chunk].contiguous()
        srs = {'fused_graph': recognizer_of(chunk, True, True), 'fused_eager': recognizer_of(chunk, True, False),
               'general': recognizer_of(chunk, False, False)}
        legs = {k: (lambda sr=sr: sr.push(frames)) for k, sr in srs.items()}
        legs['prefix_80'] = lambda: whole.recognize(x80, clone=False)
        legs['prefix_1000'] = lambda: whole1000.recognize(x1000, clone=False)
        m = measure(legs, args.reps)
        for k, (ms, lo, hi) in m.items():
            rtf = chunk * FRAME_MS / ms * B if k in srs else None
            results.append(dict(mode=mode, chunk_frames=chunk, B=B, leg=k, ms=ms, ms_min=lo, ms_max=hi, real_time_factor=rtf))
            note = f'  {rtf:9.0f} x real time over {B} streams' if rtf else ''
            print(f'{mode:>7s} chunk {chunk:3d} {k:12s} {ms:8.4f} ms (min {lo:.4f} max {hi:.4f}){note}', flush=True)
        del srs, legs

    # the price of streaming: an 80-frame utterance as 5 pushes of 16 and a finish, against one recognize call
    pieces = [audio[:, 16 * k:16 * k + 16].contiguous() for k in range(5)]

    def utterance(sr):
        def run():
            for k in range(5):
                sr.push(pieces[k], ALL, ALL if k == 0 else NONE)
            sr.finish()
        return run
    legs = {'utt_fused_graph': utterance(recognizer_of(16, True, True)), 'utt_fused_eager': utterance(recognizer_of(16, True, False)),
            'utt_general': utterance(recognizer_of(16, False, False)), 'utt_recognize': lambda: whole.recognize(x80, clone=False)}
    m = measure(legs, args.reps)
    for k, (ms, lo, hi) in m.items():
        results.append(dict(mode=mode, chunk_frames=16, B=B, leg=k, ms=ms, ms_min=lo, ms_max=hi, over_recognize=ms / m['utt_recognize'][0]))
        print(f'{mode:>7s} 80 frames  {k:16s} {ms:8.4f} ms (min {lo:.4f} max {hi:.4f})  x{ms / m["utt_recognize"][0]:.2f} of one recognize call', flush=True)
    del legs

line = json.dumps(dict(bench='streaming', rounds=args.rounds, reps=args.reps, results=results))
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line)
