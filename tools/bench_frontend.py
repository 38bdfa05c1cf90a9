#!/usr/bin/env python3
"""The batched feature front-end on one MI355X (haloop_amd.features, csrc/frontend.hip), measured in the SAME process
in alternating windows (the method of tools/bench_align.py) against the path it replaces:

    loop     a Python loop of fbank.fbank over the utterances + pad_sequence: two launches and an [m, 512] buffer per utterance,
             the parent commit's kernels (the lengths are host integers here, as a DataLoader would have them)
    batch    features.fbank_batch on the padded batch with device lengths: one launch

N = 64 utterances at 13040 samples (80 frames, the benchmark's shape), at 160000 samples (998 frames) and ragged with lengths uniform
in [0.5, 1] of each maximum; then mfcc_batch with CMVN, FrontEnd('mask:fbank') in training mode, and the three launches alone on
buffers allocated once (back to back, so the host's side of a call hides behind the kernels where they are long enough).
Human-readable lines, then ONE JSON line.

    python tools/bench_frontend.py [--rounds 5] [--reps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.nn.utils.rnn import pad_sequence

from haloop_amd import _lib, fbank, features, ops

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=50, help='calls per timed window (fewer for a leg slower than 8 ms a call)')
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', default='13040,160000')
args = ap.parse_args()

_lib.lib()
LSTM_CTC_STEP_MS = 0.41          # the flagship step, 64 utterances of 80 frames (README), printed for scale


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


results = []
N = args.batch
for samples in (int(s) for s in args.samples.split(',')):
    for ragged in (False, True):
        gen = torch.Generator().manual_seed(samples)
        wav = (0.1 * torch.randn(N, samples, generator=gen)).cuda()
        host_lengths = [samples] * N if not ragged else torch.randint(samples // 2, samples + 1, (N,), generator=gen).tolist()
        lengths = torch.tensor(host_lengths).cuda()
        M = 1 + (samples - 400) // 160
        name = f'{samples}{"_ragged" if ragged else ""}'

        def loop():
            return pad_sequence([fbank.fbank(wav[n, :host_lengths[n]][None], num_mel_bins=80) for n in range(N)], batch_first=True)

        front = features.FrontEnd('mask:fbank').train()
        # the launches alone, on buffers allocated once
        h, ptr, stream = _lib.lib(), ops.ptr, ops._stream()
        window_t, twiddle, ranges, weights, _ = features._tables(80, 400, 16000.0, 20.0, 0.0, 0, 0.0, wav.device)
        _, _, ranges23, weights23, dct = features._tables(23, 400, 16000.0, 20.0, 0.0, 13, 22.0, wav.device)
        out80, out13 = torch.empty(N, M, 80, device='cuda'), torch.empty(N, M, 13, device='cuda')
        flen = torch.empty(N, dtype=torch.int64, device='cuda')
        eps = float(torch.finfo(torch.float32).eps)
        launch_fbank = lambda: h.halo_features_batch(ptr(wav), ptr(lengths), N, samples, 0, 400, 160, 0.97, 1, ptr(window_t), ptr(twiddle), ptr(ranges),
                                                     ptr(weights), weights.numel(), 80, None, 0, eps, ptr(out80), M, ptr(flen), stream)
        launch_mfcc = lambda: h.halo_features_batch(ptr(wav), ptr(lengths), N, samples, 1, 400, 160, 0.97, 1, ptr(window_t), ptr(twiddle), ptr(ranges23),
                                                    ptr(weights23), weights23.numel(), 23, ptr(dct), 13, eps, ptr(out13), M, ptr(flen), stream)
        legs = {'loop': loop,
                'batch': lambda: features.fbank_batch(wav, lengths),
                'mfcc_cmvn': lambda: features.mfcc_batch(wav, lengths),
                'mask_fbank_train': lambda: front(wav, lengths, seed=1, step=2),
                'launch_fbank': launch_fbank, 'launch_mfcc': launch_mfcc,
                'launch_cmvn80': lambda: h.halo_cmvn_batch(ptr(out80), ptr(flen), N, M, 80, stream),
                'launch_cmvn13': lambda: h.halo_cmvn_batch(ptr(out13), ptr(flen), N, M, 13, stream),
                'launch_mask80': lambda: h.halo_spec_mask(ptr(out80), ptr(flen), N, M, 80, 13, 7, 1, 2, stream)}
        a, b = legs['batch']()[0], legs['loop']()
        err = float((a[:, :b.shape[1]] - b).abs().max())
        m = measure(legs, args.reps)
        for k, (ms, lo, hi) in m.items():
            results.append(dict(samples=samples, ragged=ragged, N=N, frames=M, leg=k, ms=ms, ms_min=lo, ms_max=hi, batch_vs_loop_max_abs=err))
            note = f'  x{m["loop"][0] / ms:7.1f} of the loop' if k in ('batch', 'mfcc_cmvn', 'mask_fbank_train') else ''
            print(f'{name:>16s} {k:18s} {ms:9.4f} ms (min {lo:.4f} max {hi:.4f}){note}', flush=True)
        print(f'{name:>16s} batch vs loop max abs {err:.2e}; the LSTM-CTC step these features feed: {LSTM_CTC_STEP_MS} ms', flush=True)
        del wav
        torch.cuda.empty_cache()

print(json.dumps(dict(bench='frontend', rounds=args.rounds, reps=args.reps, lstm_ctc_step_ms=LSTM_CTC_STEP_MS, results=results)))
