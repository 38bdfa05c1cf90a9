#!/usr/bin/env python3
"""LM shallow fusion inside the attention decoder's beam search on one MI355X: fusion.AttentionFusionDecoder.decode --
the fused decode launches, halo_decode_beam_select_lm and the LM's cell and out_layer launches every step -- against, in the SAME process
in alternating windows (the method of tools/bench_asr_beam.py): the BeamDecoder search without the LM (`plain`), that search followed by
fusion.lm_score's re-ranking of the final lists (`rerank`), and the general path of the fused search (`general`: HALO_DECODE_FUSED=0).
The `transformer:32` decoder (12 layers, 8 x 64, V = 32; untrained: oracle.transformer_ref.make_decoder_params), an untrained
rnn.Decoder(32, 512, 512, 2), features [64, 10, 512], 10 steps, `bf16x3`, W = 4 and 8; every leg again at ctc_weight 0.3 with the CTC
head's log-probabilities.  (fused - plain) / steps is what the LM adds to a step.  Human-readable lines, then ONE JSON line.

    python tools/bench_asr_lm_beam.py [--rounds 5] [--reps 20] [--widths 4,8] [--legs fused,plain,rerank,general] [--ctc-weights 0,0.3]

`--probe` adds the selection launch alone on drawn records of the same shape (N = 64, V = 32, H = 512, Ll = 2), 200 launches back to
back between two events: `halo_decode_beam_select`, `halo_decode_beam_select_lm` without the gather, and with it, at step 0 (one live
slot) and at a later step (every slot live or finished).

The kernels of a step, in a run of its own (eager launches, one leg, one row):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_asr_lm_beam.py --eager --legs fused --widths 4 --ctc-weights 0 --rounds 1
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, fusion, rnn, transformer
from oracle import transformer_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20, help='decodes per timed window')
ap.add_argument('--widths', default='4,8')
ap.add_argument('--ctc-weights', default='0,0.3')
ap.add_argument('--lm-weight', type=float, default=0.5)
ap.add_argument('--legs', default='fused,plain,rerank,general')
ap.add_argument('--probe', action='store_true', help='also time the selection launch alone, with and without the LM and its gather')
ap.add_argument('--eager', action='store_true', help='HALO_DECODE_GRAPH=0: every launch appears in a kernel trace under its own name')
args = ap.parse_args()

N, S, CAPACITY, V, HD, H, L, LM_H, LM_L = 64, 10, 10, 32, 64, 8, 12, 512, 2
if args.eager:
    os.environ['HALO_DECODE_GRAPH'] = '0'
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


model = transformer.CTCAttentionDecoder(vocab=V, head_dim=HD, heads=H, p_drop=0.2, layers=L)
model.load_state_dict(ref.make_decoder_params(V, HD, H, L, 29))
model.cuda().eval()
torch.manual_seed(1)
lm = rnn.Decoder(V, LM_H, LM_H, LM_L).cuda().eval()
dec, a = model.decoder, args.lm_weight
g = torch.Generator().manual_seed(S)
feats = torch.randn(N, S, H * HD, generator=g).cuda()
flen = torch.full((N,), S).cuda()


def unfused(fn):
    """The leg under HALO_DECODE_FUSED=0 (read at every decode): the general path."""
    def run():
        os.environ['HALO_DECODE_FUSED'] = '0'
        try:
            return fn()
        finally:
            del os.environ['HALO_DECODE_FUSED']
    return run


results = []
with torch.inference_mode():
    lp_all = model.recognizer.log_probs(feats).float()
    for c in (float(x) for x in args.ctc_weights.split(',')):
        for W in (int(x) for x in args.widths.split(',')):
            lp = lp_all if c > 0.0 else None
            bd = transformer.BeamDecoder(dec, N, CAPACITY, W, 0.0)
            fd = fusion.AttentionFusionDecoder(dec, lm, N, CAPACITY, W, a, 0.0, 0, transformer.ETX)
            gd = fusion.AttentionFusionDecoder(dec, lm, N, CAPACITY, W, a, 0.0, 0, transformer.ETX)
            assert fd.fused

            def rerank():
                tokens, lengths, ranks, _ = bd.decode(feats, flen, ctc_log_probs=lp, ctc_weight=c)
                return (ranks + a * fusion.lm_score(lm, tokens, lengths, 0)).argsort(dim=1, descending=True, stable=True)

            legs = {'fused': lambda: fd.decode(feats, flen, ctc_log_probs=lp, ctc_weight=c),
                    'plain': lambda: bd.decode(feats, flen, ctc_log_probs=lp, ctc_weight=c),
                    'rerank': rerank,
                    'general': unfused(lambda: gd.decode(feats, flen, ctc_log_probs=lp, ctc_weight=c))}
            legs = {k: fn for k, fn in legs.items() if k in args.legs.split(',')}
            for fn in legs.values():                                        # warm every leg (weight images, graphs)
                fn()
            r = dict(W=W, ctc_weight=c)
            if 'fused' in legs and 'plain' in legs:                         # how often the LM inside the search finds another best hypothesis
                best = legs['fused']()[0][:, 0].clone()
                r['best_differs'] = float((best != legs['plain']()[0][:, 0]).any(1).float().mean())
            times = {k: [] for k in legs}
            for _ in range(args.rounds):                                    # alternating windows
                for k, fn in legs.items():
                    times[k].append(window(fn, args.reps if k != 'general' else max(1, args.reps // 10)))
            med = {k: statistics.median(times[k]) * 1e3 for k in legs}
            for k in legs:
                r[k + '_ms_per_batch'], r[k + '_ms_min'], r[k + '_ms_max'] = med[k], min(times[k]) * 1e3, max(times[k]) * 1e3
            if 'fused' in legs and 'plain' in legs:
                r['fused_over_plain'] = med['fused'] / med['plain']
                r['plain_step_us'] = med['plain'] * 1e3 / CAPACITY
                r['lm_us_per_step'] = (med['fused'] - med['plain']) * 1e3 / CAPACITY
            if 'fused' in legs and 'rerank' in legs:
                r['fused_over_rerank'] = med['fused'] / med['rerank']
            results.append(r)
            print(f"W={W} ctc_weight={c}: " + ', '.join(f"{k} {med[k]:.3f} ms/batch (min {r[k + '_ms_min']:.3f} max {r[k + '_ms_max']:.3f})"
                                                         for k in legs)
                  + f"; fused / plain {r.get('fused_over_plain')}; fused / rerank {r.get('fused_over_rerank')}; the LM adds "
                  f"{r.get('lm_us_per_step')} us to a step of {r.get('plain_step_us')} us; best hypothesis differs in "
                  f"{r.get('best_differs')} of the rows", flush=True)
            del bd, fd, gd


def probe(W):
    """us per launch of the selection alone at width W: (step, plain, with the LM, with the LM and the gather)."""
    from haloop_amd import ops
    R, C, etx = N * W, H * HD, transformer.ETX
    gen = torch.Generator().manual_seed(W)
    logits, lg = torch.randn(R, V, generator=gen).cuda() * 3, torch.randn(R, V, generator=gen).cuda()
    rec = lambda: (-torch.rand(N, W, generator=gen).cuda(), torch.randint(0, 3, (N, W), generator=gen, dtype=torch.int32).cuda(),
                   torch.zeros(N, W, dtype=torch.int32).cuda(), torch.randint(4, V, (N, W, CAPACITY), generator=gen, dtype=torch.int32).cuda(),
                   torch.randint(0, R, (R, CAPACITY), generator=gen, dtype=torch.int32).cuda())
    a_, b_ = rec(), rec()
    ranks, lm0, lm1 = torch.zeros(N, W).cuda(), -torch.rand(N, W, generator=gen).cuda(), torch.zeros(N, W).cuda()
    par, last = (torch.zeros(N, W, dtype=torch.int32).cuda() for _ in range(2))
    wte, y = torch.randn(V, C, generator=gen).cuda(), torch.zeros(R, C).cuda()
    lm_wte, h, c_ = (torch.randn(*shape, generator=gen).cuda() for shape in ((V, LM_H), (LM_L, R, LM_H), (LM_L, R, LM_H)))
    xh, c_out = torch.zeros(LM_L, R, 2 * LM_H).cuda(), torch.zeros(LM_L, R, LM_H).cuda()

    def us(fn, reps=200):
        for _ in range(20):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); start.record()
        for _ in range(reps):
            fn()
        end.record(); torch.cuda.synchronize()
        return start.elapsed_time(end) / reps * 1e3

    rows = []
    for t in (0, 4):
        rows.append(dict(W=W, t=t,
                         select_us=us(lambda: ops.decode_beam_select(logits, t, CAPACITY, etx, 0.0, a_, b_, ranks, wte, y)),
                         select_lm_no_gather_us=us(lambda: ops.decode_beam_select_lm(logits, t, CAPACITY, etx, 0.0, lg, None, lm0, lm1, a, etx, a_,
                                                                                     b_, ranks, par, last, wte=wte, y_next=y)),
                         select_lm_us=us(lambda: ops.decode_beam_select_lm(logits, t, CAPACITY, etx, 0.0, lg, None, lm0, lm1, a, etx, a_, b_, ranks,
                                                                           par, last, lm_wte, h, c_, xh, c_out, wte, y))))
        print(f"selection alone, W={W} t={t}: " + ', '.join(f'{k} {v:.1f}' for k, v in rows[-1].items() if k.endswith('_us')), flush=True)
    return rows


selection = [row for W in (int(x) for x in args.widths.split(',')) for row in probe(W)] if args.probe else None
print(json.dumps(dict(bench='asr_lm_beam', selection_alone=selection, N=N, S=S, capacity=CAPACITY, V=V, layers=L, heads=H, head_dim=HD, lm_hidden=LM_H, lm_layers=LM_L,
                      lm_weight=a, mode='bf16x3', rounds=args.rounds, reps=args.reps, eager=args.eager, results=results)))
