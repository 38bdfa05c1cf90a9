#!/usr/bin/env python3
"""The rotary striding encoder of the `e6ctc-d4` arch (ha/init.py: StridingAudioEncoderConfig, n_layer 6, n_head 8, n_embd 512, conv strides
(2, 2, 1), d_conv 256) at N = 64 utterances of 1000 frames x 80 mel on one MI355X: T' = 250, 16000 token rows.

Measured, in `bf16x3` and in `bf16`, each with the q | k rotation on halo_rope_rows (HALO_ROPE_ROWS=1) and on the scalar operator, one launch
per tensor (HALO_ROPE_ROWS=0), in alternating windows of the SAME run: the eval forward, and forward + backward (no dropout, so that `bf16`
takes the row-major forms).  Then the rotation launches on their own (HIP events over back-to-back launches) at the step's shapes: the
packed fp32 rows [16000, 1536] by the one launch and by the two scalar launches, and the packed bf16 rows.  Prints human-readable lines and
ONE JSON line (last).

    python tools/bench_audio_encoder.py [--rounds 3] [--steps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, attention, attention_audio, ops

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--frames', type=int, default=1000)
args = ap.parse_args()

_lib.lib(); _lib.lend_scratch(256 << 20)
cfg = attention.StridingAudioEncoderConfig(dropout=0.0, n_layer=6, n_head=8, n_embd=512, conv_strides=(2, 2, 1))
torch.manual_seed(0)
enc = attention_audio.StridingAudioEncoder(cfg).cuda().eval()
N, T0 = args.batch, args.frames
x = torch.randn(N, T0, cfg.d_input, device='cuda')
il = torch.full((N,), T0, dtype=torch.int64, device='cuda')
T = int(enc.subsampled_lengths(il)[0])
M, C, H = N * T, cfg.n_embd, cfg.n_head
dout = torch.randn(N, T, C, device='cuda')
params = list(enc.parameters())


def forward():
    with torch.no_grad():
        return enc(x, il)[0]


def forward_backward():
    for p in params: p.grad = None
    feats = enc(x, il)[0]
    feats.backward(dout)
    return feats


def window(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


res = {'metric': 'ms per pass, e6ctc-d4 encoder (6 rotary blocks, C=512, 8 heads) N=64 x 1000 frames: rotation on halo_rope_rows against the scalar operator',
       'unit': 'ms', 'n_gpus': 1, 'config': {'batch': N, 'frames': T0, 'rows': M, 'rounds': args.rounds, 'steps_per_window': args.steps},
       'passes': {}, 'forms': {}}
for mode in ('bf16x3', 'bf16'):
    _lib.set_math_mode(mode)
    for what, fn in (('forward', forward), ('forward_backward', forward_backward)):
        times = {'1': [], '0': []}
        for sw in times:                                  # warm every shape of both legs
            os.environ['HALO_ROPE_ROWS'] = sw
            window(fn, 3)
        res['forms'][f'{mode} {what}'] = enc.last_form
        for _ in range(args.rounds):                      # alternating windows: both legs see the same machine state
            for sw in times:
                os.environ['HALO_ROPE_ROWS'] = sw
                times[sw].append(window(fn, args.steps))
        ms = {sw: round(1e3 * statistics.median(v), 3) for sw, v in times.items()}
        res['passes'][f'{mode} {what}'] = {'rope_rows_ms': ms['1'], 'scalar_ms': ms['0'],
                                           'windows_ms': {sw: [round(1e3 * t, 3) for t in v] for sw, v in times.items()}}
        print(f'{mode} {what} ({enc.last_form}): halo_rope_rows {ms["1"]:.3f} ms, scalar operator {ms["0"]:.3f} ms  '
              f'(windows {[round(1e3 * t, 2) for t in times["1"]]} | {[round(1e3 * t, 2) for t in times["0"]]})')
os.environ.pop('HALO_ROPE_ROWS')
res['value'] = res['passes']['bf16x3 forward_backward']['rope_rows_ms']


def event_us(fn, reps=200):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


# the rotation launches on their own; algorithmic bytes: q and k read and written once (the tables stay in L2)
hd = C // H
table = ops.RopeTable(max(T, 256), hd, 'cuda')
rows32 = torch.randn(M, 3 * C, device='cuda')
rows16 = torch.randn(M, 3 * C, device='cuda').bfloat16()


def scalar_pair():
    ops.rope_(rows32[:, :C], T, H, hd, table)
    ops.rope_(rows32[:, C:2 * C], T, H, hd, table)


kern = {
    'halo_rope_rows fp32 [16000, 1536] q | k, one launch': (lambda: ops.rope_rows_(rows32, T, H, hd, table), 2 * 4 * M * 2 * C),
    'halo_rope_interleaved fp32, q then k, two launches': (scalar_pair, 2 * 4 * M * 2 * C),
    'halo_rope_rows bf16 [16000, 1536] q | k, one launch': (lambda: ops.rope_rows_(rows16, T, H, hd, table), 2 * 2 * M * 2 * C),
}
res['kernels'] = {}
for _ in range(2):                                        # twice, alternating: the second round is reported, the first shows the spread
    for name, (fn, nbytes) in kern.items():
        us = event_us(fn)
        res['kernels'].setdefault(name, {'algorithmic_bytes': nbytes, 'us_rounds': []})['us_rounds'].append(us)
for name, k in res['kernels'].items():
    k['us'] = k['us_rounds'][-1]
    k['GB_per_s'] = round(k['algorithmic_bytes'] / k['us'] / 1e3, 1)
    print(f'{name}: {k["us"]:.1f} us (rounds {k["us_rounds"]})  ({k["GB_per_s"]:.0f} GB/s of algorithmic bytes)')
print(json.dumps(res), flush=True)
