#!/usr/bin/env python3
"""GPT-2 small (124 M) generation on one MI355X: the operator-per-launch loop (haloop_amd.attention.generate, batch 1 only) against
haloop_amd.generation.Sampler, eager launches and one captured step replayed, measured in the SAME process in alternating windows
(the method of tools/bench_gpt_lora.py).  B in {1, 8}, prompt 16 and 512, 128 new tokens, `bf16x3` and `bf16` arithmetic, top_k = 40 at
temperature 0.8, no stop token.  Every leg is timed at 128 new tokens and at 1 (the prefill and the first draw); the decode cost per token
is the difference over 127.  Also: libhalo calls per token, the fraction of the HBM roof (the bytes a token must read -- the decode
images' fragments the mode reads plus the keys and values of the cached positions -- over 8.0 TB/s, against the decode time per token), and
halo_gpt_decode_attention alone at 1024 keys with four and with sixteen waves per (row, head), B in {1, 8, 32}.  Human-readable lines, then ONE JSON line.

    python tools/bench_gpt_generate.py [--rounds 3] [--new 128]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, attention, generation, ops

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--new', type=int, default=128)
ap.add_argument('--modes', default='bf16x3,bf16')
ap.add_argument('--prompts', default='16,512')
ap.add_argument('--batches', default='1,8')
ap.add_argument('--leg', choices=['all', 'parent', 'eager', 'replay'], default='all', help='one leg only, for a kernel-trace run of its own')
ap.add_argument('--attention-child', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()

HBM_PEAK = 8.0e12            # bytes / s, the MI355X specification
ATTN_BATCHES = (1, 8, 32)


def attention_child(rounds):
    """Windows of 200 back-to-back halo_gpt_decode_attention launches at 1024 keys (GPT-2 small heads), us per launch, per batch size."""
    H, C = 12, 768
    out = {}
    for B in ATTN_BATCHES:
        ck, cv = (torch.randn(B, H, 1024, 64, device='cuda') for _ in range(2))
        qkv, y = torch.randn(B, 3 * C, device='cuda'), torch.empty(B, C, device='cuda')
        pos = torch.full((B,), 1023, device='cuda', dtype=torch.int32)
        t = []
        for r in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                ops.gpt_decode_attention(qkv, ck, cv, pos, y)
            e1.record(); torch.cuda.synchronize()
            if r:                                                 # round 0 warms
                t.append(e0.elapsed_time(e1) / 200 * 1e3)
        out[B] = t
    print(json.dumps(out))


_lib.lib(); _lib.lend_scratch(256 << 20)
if args.attention_child:
    attention_child(args.rounds)
    sys.exit(0)
cfg = attention.GPTConfig()
torch.manual_seed(0)
model = attention.GPT(cfg).cuda().eval()
with torch.no_grad():                                     # the reference's init zeroes wpe; give it content
    model.transformer.wpe.weight.normal_(0, 0.02)
L, C, H, V = cfg.n_layer, cfg.n_embd, cfg.n_head, cfg.vocab_size
N = args.new
DRAW = dict(temperature=0.8, top_k=40, stop_token=-1)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


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


def token_bytes(mode, B, P):
    """What one decode step must read: per weight the fragments its mode reads (bf16x3: hi + lo, 4 bytes per weight; bf16: hi, 2), and the
    cached keys and values of the positions before it (fp32), averaged over the N - 1 steps."""
    weights = L * 12 * C * C + V * C
    keys = P + (N - 1) / 2.0
    return weights * (4 if mode == 'bf16x3' else 2) + L * 2 * B * C * keys * 4


results = []
with torch.inference_mode():
    for mode in args.modes.split(','):
        _lib.set_math_mode(mode)
        for P in (int(p) for p in args.prompts.split(',')):
            for B in (int(b) for b in args.batches.split(',')):
                ids = torch.randint(1, V, (B, P), generator=torch.Generator().manual_seed(P + B)).cuda()
                eager = generation.Sampler(model, B, use_graph=False)
                replay = generation.Sampler(model, B, use_graph=True)
                legs = {}
                if B == 1 and args.leg in ('all', 'parent'):
                    legs['parent'] = lambda n: [t for t in attention.generate(model, ids, n, **DRAW)]
                if args.leg in ('all', 'eager'):
                    legs['eager'] = lambda n: eager.sample(ids, n, seed=1, **DRAW)
                if args.leg in ('all', 'replay'):
                    legs['replay'] = lambda n: replay.sample(ids, n, seed=1, **DRAW)
                assert eager.fused and replay.fused
                for fn in legs.values():                              # warm every shape of every leg (and capture the step)
                    fn(N); fn(1)
                if 'eager' in legs and 'replay' in legs:
                    assert torch.equal(legs['eager'](N)[0], legs['replay'](N)[0])
                calls = {k: (count_calls(lambda: fn(N)) - count_calls(lambda: fn(1))) / (N - 1) for k, fn in legs.items() if k != 'replay'}
                times = {k: ([], []) for k in legs}
                for _ in range(args.rounds):                          # alternating windows
                    for k, fn in legs.items():
                        times[k][0].append(timed(lambda: fn(N)))
                        times[k][1].append(timed(lambda: fn(1)))
                for k in legs:
                    whole, first = times[k]
                    dec = [(a - b) / (N - 1) * 1e3 for a, b in zip(whole, first)]
                    r = dict(mode=mode, B=B, prompt=P, leg=k, ms_per_token_whole_call=statistics.median(whole) / N * 1e3,
                             decode_ms_per_token=statistics.median(dec), decode_ms_min=min(dec), decode_ms_max=max(dec),
                             prefill_ms=statistics.median(first) * 1e3, libhalo_calls_per_token=calls.get(k, calls.get('eager')),
                             hbm_roof_fraction=token_bytes(mode, B, P) / HBM_PEAK / (statistics.median(dec) * 1e-3))
                    results.append(r)
                    print(f"{mode:7s} B={B} P={P:3d} {k:7s} decode {r['decode_ms_per_token']:.3f} ms/token (min {r['decode_ms_min']:.3f} max "
                          f"{r['decode_ms_max']:.3f})  whole call {r['ms_per_token_whole_call']:.3f} ms/token  prefill+draw {r['prefill_ms']:.2f} ms  "
                          f"libhalo calls/token {r['libhalo_calls_per_token']}  HBM roof {100 * r['hbm_roof_fraction']:.1f} %", flush=True)
                del eager, replay

# ---- halo_gpt_decode_attention alone at 1024 keys: four against sixteen waves per (row, head).  The library reads the switch once per
#      process, so each setting runs in child processes of its own, in the order 4, 16, 16, 4; a child times rounds windows of 200 launches ----
attn = []
if args.leg == 'all':
    del model
    torch.cuda.empty_cache()
    runs = {4: [], 16: []}
    for waves in (4, 16, 16, 4):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--attention-child', '--rounds', str(args.rounds)], check=True,
                             capture_output=True, text=True, env=dict(os.environ, HALO_GPT_ATTN_WAVES=str(waves))).stdout
        runs[waves].append(json.loads(out.strip().splitlines()[-1]))
    for B in ATTN_BATCHES:
        t = {w: [x for run in runs[w] for x in run[str(B)]] for w in (4, 16)}
        a = dict(B=B, keys=1024, us_4_waves=statistics.median(t[4]), us_16_waves=statistics.median(t[16]),
                 us_4_waves_range=[min(t[4]), max(t[4])], us_16_waves_range=[min(t[16]), max(t[16])])
        attn.append(a)
        print(f"attention alone B={B} 1024 keys: 4 waves {a['us_4_waves']:.1f} us (min {min(t[4]):.1f} max {max(t[4]):.1f}), 16 waves "
              f"{a['us_16_waves']:.1f} us (min {min(t[16]):.1f} max {max(t[16]):.1f}) per launch, back to back")

print(json.dumps(dict(bench='gpt_generate', model='gpt2-small', new_tokens=N, rounds=args.rounds, results=results, attention=attn)))
