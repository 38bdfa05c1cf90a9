#!/usr/bin/env python3
"""Streaming transducer recognition on one MI355X: haloop_amd.streaming.StreamingTransducer's push -- stream_front, the
persistent LSTM, stream_logits and transducer.GreedyStream's rounds -- for 64 streams over the LC-2x1024 encoder and the
`rnn-transducer` head at V = 32 and 256, in chunks of 16, 32 and 64 frames, `bf16x3`.  In the SAME process, in alternating windows
(the method of tools/bench_rnnt_decode.py):

    stream     ms per push, the mean rounds and emitted symbols per push
    general    the same pushes with the search on its general path (HALO_RNNT_FUSED=0)
    ctc        StreamingRecognizer's greedy push on the same encoder: the encoder's share
    prefix     the route before: GreedyDecoder.decode over the accumulated prefix, at 80 and at 1000 frames (20 and 250 steps)
    round      the launches of one round alone (advance, masked cells, out_layer), no row live

The head is untrained, so the logits carry planted symbols as tools/bench_rnnt_beam.py's features do (randn, plus 7.0 on a drawn label
in a quarter of the steps and on the blank elsewhere, plus 4.5 on the blank everywhere): the tool copies each push's planted logits
over the ones the encoder produced (one copy launch, inside the timed window), so the encoder runs for real and the rounds per push
resemble speech.  Human-readable lines, then ONE JSON line.

    python tools/bench_rnnt_stream.py [--rounds 5] [--reps 3] [--max-symbols 1] [--vocabs 32,256] [--chunks 16,32,64] [--legs stream,general,ctc,prefix,round]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, ops, recognizer, rnn, streaming, transducer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5, help='alternating windows per leg')
ap.add_argument('--reps', type=int, default=3, help='streams of --frames frames per timed window of the fused legs')
ap.add_argument('--frames', type=int, default=320, help='frames of one stream (a multiple of every chunk)')
ap.add_argument('--max-symbols', type=int, default=1, help='max_symbols_per_frame of every search: the untrained prediction network does '
                'not suppress a planted label once it is emitted, so a planted step emits up to this cap (1: about one symbol per four steps)')
ap.add_argument('--vocabs', default='32,256')
ap.add_argument('--chunks', default='16,32,64')
ap.add_argument('--legs', default='stream,general,ctc,prefix,round')
args = ap.parse_args()
LEGS = args.legs.split(',')

B, F_, C, H, L, CAPACITY = 64, 80, 128, 1024, 2, 256
_lib.lib(); _lib.lend_scratch(256 << 20)
_lib.set_math_mode('bf16x3')


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def planted(gen, steps, V, width):
    x = torch.zeros(B, steps, width)
    x[:, :, :V] = torch.randn(B, steps, V, generator=gen)
    lab = torch.randint(1, V, (B, steps), generator=gen)
    is_lab = torch.rand(B, steps, generator=gen) < 0.25
    ch = torch.where(is_lab, lab, torch.zeros_like(lab))
    x.scatter_add_(2, ch[:, :, None], torch.full((B, steps, 1), 7.0))
    x[:, :, 0] += 4.5
    return x


def summary(times):
    return dict(ms=statistics.median(times) * 1e3, ms_min=min(times) * 1e3, ms_max=max(times) * 1e3)


torch.manual_seed(1)
enc = rnn.Encoder(F_, C, H, num_layers=L).cuda().eval()
frames_all = torch.randn(B, args.frames, F_, generator=torch.Generator().manual_seed(2)).cuda()
results = []
for V in (int(v) for v in args.vocabs.split(',')):
    torch.manual_seed(V)
    head = recognizer.Transducer(H, V).cuda().eval()
    with torch.no_grad():
        head.classifier.weight.copy_(torch.eye(V, H))
        head.classifier.bias.zero_()
    ctc_head = recognizer.TemporalClassifier(H, V).cuda().eval()
    feats = planted(torch.Generator().manual_seed(V + 1), 250, V, H).cuda()          # classifier(feats) = the planted logits
    logits_all = feats[:, :, :V].contiguous()
    res = dict(V=V)

    if 'prefix' in LEGS:                                                             # the route before, on the same build
        whole = transducer.GreedyDecoder(head, B, CAPACITY, args.max_symbols)
        for steps in (20, 250):
            x, il = feats[:, :steps].contiguous(), torch.full((B,), steps, dtype=torch.int64).cuda()
            out = whole.decode(x, il)
            times = [window(lambda: whole.decode(x, il), args.reps) for _ in range(args.rounds)]
            res[f'prefix_{4 * steps}_frames'] = dict(summary(times), advances=whole.iterations, symbols_mean=float(out[1].float().mean()))
            print(f'V={V:3d} GreedyDecoder.decode of a prefix of {4 * steps} frames ({steps} steps): {res[f"prefix_{4 * steps}_frames"]}', flush=True)
        del whole

    for chunk in (int(c) for c in args.chunks.split(',')):
        S, n_push = chunk // 4, args.frames // chunk
        assert args.frames % chunk == 0 and n_push * S <= 250
        st = streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=CAPACITY, max_symbols_per_frame=args.max_symbols)
        ctc = streaming.StreamingRecognizer(enc, ctc_head, B, chunk_frames=chunk, capacity=CAPACITY, use_graph=False)
        search_advance = st.search._advance
        stats = dict(rounds=0, pushes=0)

        def advance_planted(f, nf, flags, any_begin, k=[0]):
            f.copy_(logits_all[:, k[0] * S:(k[0] + 1) * S])                           # this push's planted logits over the encoder's
            k[0] = (k[0] + 1) % n_push
            out = search_advance(f, nf, flags, any_begin)
            stats['rounds'] += st.search.rounds; stats['pushes'] += 1
            return out
        st.search._advance = advance_planted

        def one_stream(obj):
            for k in range(n_push):
                obj.push(frames_all[:, k * chunk:(k + 1) * chunk], None, [k == 0] * B)

        def leg(fused):
            os.environ['HALO_RNNT_FUSED'] = '1' if fused else '0'
            assert st.search.fused == fused
            one_stream(st)
        legs = {'stream': lambda: leg(True), 'general': lambda: leg(False), 'ctc': lambda: one_stream(ctc)}
        legs = {k: fn for k, fn in legs.items() if k in LEGS}
        reps = {'stream': args.reps, 'general': 1, 'ctc': args.reps}
        for fn in legs.values():
            fn()                                                                     # warm every leg
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                                 # alternating windows
            for k, fn in legs.items():
                if k == 'stream':
                    stats.update(rounds=0, pushes=0)
                times[k].append(window(fn, reps[k]) / n_push)
                if k == 'stream':
                    mean_rounds = stats['rounds'] / stats['pushes']
        os.environ['HALO_RNNT_FUSED'] = '1'
        r = dict(chunk_frames=chunk, steps_per_push=S, pushes_per_stream=n_push)
        for k in legs:
            r[k] = summary(times[k])
        if 'stream' in legs:
            leg(True)
            r['rounds_per_push_mean'] = mean_rounds
            r['symbols_per_push_mean'] = float(st.partial()[1].float().mean()) / n_push
        if 'round' in LEGS:                                                          # one round's launches alone: no row is live
            gs, lm = st.search, head.lm
            layers, head_image = gs._net.images()
            nf = torch.zeros(B, dtype=torch.int32).cuda()
            f = logits_all[:, :S].contiguous()
            gs._live.zero_()

            def one_round():
                ops.rnnt_advance_stream(f, gs._g, lm.out_layer.bias, nf, gs._state, gs._scores, gs._tokens, gs._frames, gs.max_symbols,
                                        lm.embedding.weight, gs._xh[gs._cur, 0], gs._live, gs._pos, gs._mask)
                gs._lm_step(B, gs._cur, layers, head_image, gs._mask)
                gs._cur = 1 - gs._cur
            gs._state[3].fill_(1)
            one_round()
            r['round_us'] = statistics.median(window(one_round, 200) for _ in range(args.rounds)) * 1e6
        res[f'chunk_{chunk}'] = r
        print(f'V={V:3d} chunk {chunk:2d}: ' + ', '.join(f'{k} {r[k]["ms"]:.3f} ms/push (min {r[k]["ms_min"]:.3f} max {r[k]["ms_max"]:.3f})' for k in legs)
              + f'; rounds/push {r.get("rounds_per_push_mean")}, symbols/push {r.get("symbols_per_push_mean")}, one round {r.get("round_us")} us',
              flush=True)
        del st, ctc
    results.append(res)
os.environ.pop('HALO_RNNT_FUSED', None)

print(json.dumps(dict(bench='rnnt_stream', streams=B, encoder='LC-2x1024', capacity=CAPACITY, frames=args.frames, max_symbols_per_frame=args.max_symbols, mode='bf16x3',
                      rounds=args.rounds, reps=args.reps, results=results)))
