#!/usr/bin/env python3
"""Edit distance on the device and the MWER training step on one MI355X (csrc/edit_distance.hip), measured in the SAME
process in alternating windows (the method of tools/bench_rnnt_beam.py), `bf16x3`:

    (a) wer.edit_distance on the n-best lists of the arch's batch -- features [64, 21, 1024], V = 32, capacity 11, W = 4 and 8, the
        planted features of tools/bench_rnnt_beam.py -- against what the repository did before: the tokens copied to the host and a
        Python edit-distance loop over the N * W pairs (the loop of tools/bench_asr.py);
    (b) the same two legs on 256 pairs of 200 x 200 random tokens over 32 symbols;
    (c) an MWER step of the head (mwer_forward at W = 4, mle_weight 0.01, and its backward; V = 32 and 256) against the ordinary
        fused_loss step of the same head, with the parts of the MWER forward timed on their own: search (BeamDecoder), distance
        (wer.edit_distance), loss (the prediction network over the N * W hypotheses and transducer_loss, no backward), risk
        (nbest_risk forward and backward).

Human-readable lines, then ONE JSON line, also written to --out.

    python tools/bench_mwer.py [--rounds 5] [--reps 20] [--out profiles/mwer_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from haloop_amd import _lib, functional as HF, recognizer, transducer, wer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='calls per timed window (a leg slower than 20 ms a call runs fewer)')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mwer_bench.json'))
args = ap.parse_args()

N, T, FEAT, CAPACITY = 64, 21, 1024, 11
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(legs):
    """Alternating windows -> {leg: (median ms, min ms, max ms, calls per window)}."""
    per = {}
    for k, fn in legs.items():
        fn(); fn()                                                        # warm
        per[k] = max(1, min(args.reps, int(0.4 / max(window(fn, 1), 1e-5))))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(window(fn, per[k]))
    return {k: (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3, per[k]) for k, v in times.items()}


def host_edit_distance(a, b):
    d = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, cb in enumerate(b, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (ca != cb))
    return d[-1]


def host_leg(hyp, hyp_len, ref, ref_len, group):
    """The tokens pulled off the device, then the Python loop over the pairs: errors only (the loop keeps no counts)."""
    h, hl, r, rl = hyp.reshape(-1, hyp.shape[-1]).tolist(), hyp_len.reshape(-1).tolist(), ref.tolist(), ref_len.tolist()
    return [host_edit_distance(h[p][:hl[p]], r[p // group][:rl[p // group]]) if hl[p] >= 0 else -1 for p in range(len(h))]


def planted(gen, V):
    x = torch.randn(N, T, FEAT, generator=gen)
    lab = torch.randint(1, V, (N, T), generator=gen)
    is_lab = torch.rand(N, T, generator=gen) < 0.25
    ch = torch.where(is_lab, lab, torch.zeros_like(lab))
    x.scatter_add_(2, ch[:, :, None], torch.full((N, T, 1), 7.0))
    x[:, :, 0] += 4.5
    return x


def make_head(V):
    torch.manual_seed(V)
    head = recognizer.Transducer(FEAT, V).cuda()
    with torch.no_grad():
        head.classifier.weight.copy_(torch.eye(V, FEAT))
        head.classifier.bias.zero_()
    head.fused_loss = True
    return head


def report(results, part, shape, timing, **extra):
    for k, (ms, lo, hi, reps) in timing.items():
        results.append(dict(part=part, shape=shape, leg=k, ms=ms, ms_min=lo, ms_max=hi, calls_per_window=reps, **extra))
        print(f'{part} {shape:>28s} {k:12s} {ms:10.4f} ms (min {lo:.4f} max {hi:.4f}, {reps} calls per window)', flush=True)


results = []
gen = torch.Generator().manual_seed(7)
targets = torch.randint(1, 32, (N, CAPACITY - 1), generator=gen).cuda()
tl = torch.randint(CAPACITY // 2, CAPACITY, (N,), generator=gen).cuda()
il = torch.full((N,), T, dtype=torch.int64).cuda()

# (a) the n-best lists of the arch's batch
head = make_head(32).eval()
features = planted(torch.Generator().manual_seed(33), 32).cuda()
for W in (4, 8):
    tokens, lengths, _, _ = transducer.BeamDecoder(head, N, CAPACITY, W).decode(features, il)
    device_leg = lambda: wer.edit_distance(tokens, lengths, targets, tl, group=W)
    assert device_leg()[0].tolist() == host_leg(tokens, lengths, targets, tl, W)
    legs = {'device': device_leg, 'device_read': lambda: device_leg()[0].tolist(), 'host_loop': lambda: host_leg(tokens, lengths, targets, tl, W)}
    report(results, 'a', f'{N * W} pairs, {CAPACITY} x {CAPACITY - 1}', measure(legs), pairs=N * W, mean_hyp_length=float(lengths.clamp(min=0).float().mean()))

# (b) 256 pairs of 200 x 200 tokens
hyp, ref = torch.randint(0, 32, (256, 200), generator=gen).cuda(), torch.randint(0, 32, (256, 200), generator=gen).cuda()
full = torch.full((256,), 200, dtype=torch.int32).cuda()
device_leg = lambda: wer.edit_distance(hyp, full, ref, full)
assert device_leg()[0].tolist() == host_leg(hyp, full, ref, full, 1)
legs = {'device': device_leg, 'device_read': lambda: device_leg()[0].tolist(), 'host_loop': lambda: host_leg(hyp, full, ref, full, 1)}
report(results, 'b', '256 pairs, 200 x 200', measure(legs), pairs=256)

# (c) the MWER step against the ordinary step of the same head
W = 4
for V in (32, 256):
    head = make_head(V).train()
    features = planted(torch.Generator().manual_seed(V + 1), V).cuda()
    tg = torch.randint(1, V, (N, CAPACITY - 1), generator=gen).cuda()

    def step(mwer):
        head.zero_grad(set_to_none=True)
        head.mwer_beam = W if mwer else 0
        loss, _ = head(features, tg, il, tl)
        loss.backward()
        head.mwer_beam = 0
        return loss

    nbest = head._search_nbest(features, il, CAPACITY, W)
    tokens, lengths = nbest[0], nbest[1]
    errors = wer.edit_distance(tokens, lengths, tg, tl, group=W)[0].view(N, W)
    hyps = tokens.clamp(min=0).view(N * W, -1)
    lm_in = torch.cat([hyps.new_zeros((N * W, 1)), hyps], dim=1)

    @torch.no_grad()
    def loss_part():
        feats = HF.linear(features, head.classifier.weight, head.classifier.bias)
        g, _ = head.lm.forward_batch_first(lm_in, head.lm.init_hidden(N * W))
        rows = feats[:, None].expand(N, W, T, V).reshape(N * W, T, V)
        return transducer.transducer_loss(rows, g, hyps, il[:, None].expand(N, W).reshape(-1), lengths.clamp(min=0).view(-1)).view(N, W)

    losses = loss_part()

    def risk_part():
        l = losses.clone().requires_grad_(True)
        transducer.nbest_risk(l, errors).mean().backward()
        return l.grad

    legs = {'mwer_step': lambda: step(True), 'fused_loss_step': lambda: step(False),
            'search': lambda: head._search_nbest(features, il, CAPACITY, W),
            'distance': lambda: wer.edit_distance(tokens, lengths, tg, tl, group=W), 'loss_forward': loss_part, 'risk': risk_part}
    report(results, 'c', f'N {N}, T {T}, V {V}, W {W}', measure(legs), V=V, W=W, f_copy_bytes=N * W * T * V * 4)

line = json.dumps(dict(bench='mwer', mode=_lib.get_math_mode(), rounds=args.rounds, reps=args.reps, results=results))
print(line)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write(line + '\n')
