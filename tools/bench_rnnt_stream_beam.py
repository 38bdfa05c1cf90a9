#!/usr/bin/env python3
"""Streaming transducer beam search on one MI355X: haloop_amd.streaming.StreamingTransducer(beam=W)'s push --
stream_front, the persistent LSTM, stream_logits and transducer.BeamStream's rounds -- for 64 streams over the LC-2x1024 encoder and
the `rnn-transducer` head at V = 32 and 256, in chunks of 16, 32 and 64 frames, W = 4 and 8, `bf16x3`.  In the SAME process, in
alternating windows (the method of tools/bench_rnnt_stream.py):

    beam       ms per push at every cadence of --cadences (the live word is read after S rounds, then every that many rounds)
    greedy     the greedy push (beam=0) on the same encoder and logits
    general    the beam object's general path (HALO_RNNT_FUSED=0): --general-pushes pushes of a stream per window, it is host-bound
    prefix     the route this replaces: BeamDecoder.decode over the accumulated prefix, at 80 and at 1000 frames (20 and 250 steps)

and, from one more untimed stream, the rounds per push and the share of them that ran past the last live one.  The logits carry planted
symbols exactly as in tools/bench_rnnt_stream.py.  Human-readable lines, then ONE JSON line.

    python tools/bench_rnnt_stream_beam.py [--rounds 5] [--reps 3] [--vocabs 32,256] [--chunks 16,32,64] [--beams 4,8]
                                           [--cadences 1,2,4,8] [--legs beam,greedy,general,prefix]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from haloop_amd import _lib, recognizer, rnn, streaming, transducer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5, help='alternating windows per leg')
ap.add_argument('--reps', type=int, default=3, help='streams of --frames frames per timed window of the fused legs')
ap.add_argument('--frames', type=int, default=320, help='frames of one stream (a multiple of every chunk)')
ap.add_argument('--vocabs', default='32,256')
ap.add_argument('--chunks', default='16,32,64')
ap.add_argument('--beams', default='4,8')
ap.add_argument('--cadences', default='1,2,4,8')
ap.add_argument('--general-pushes', type=int, default=2, help='pushes per window of the general leg (the first of a stream)')
ap.add_argument('--legs', default='beam,greedy,general,prefix')
args = ap.parse_args()
LEGS = args.legs.split(',')
CADENCES = [int(c) for c in args.cadences.split(',')]

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


def plant(st, logits_all, S, n_push, stats=None):
    """This push's planted logits over the encoder's (one copy launch, inside the timed window), as tools/bench_rnnt_stream.py does."""
    search_advance = st.search._advance

    def advance_planted(f, nf, flags, any_begin, k=[0]):
        if any_begin:
            k[0] = 0
        f.copy_(logits_all[:, k[0] * S:(k[0] + 1) * S])
        k[0] = (k[0] + 1) % n_push
        search_advance(f, nf, flags, any_begin)
        if stats is not None and stats['on']:
            rounds = st.search.rounds
            live = st.search._live[:rounds].tolist()
            needed = next((i for i, w in enumerate(live) if w == 0), rounds - 1) + 1
            stats['rounds'] += rounds; stats['needed'] += needed; stats['pushes'] += 1
    st.search._advance = advance_planted


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
    feats = planted(torch.Generator().manual_seed(V + 1), 250, V, H).cuda()          # classifier(feats) = the planted logits
    logits_all = feats[:, :, :V].contiguous()
    for W in (int(w) for w in args.beams.split(',')):
        res = dict(V=V, W=W)
        if 'prefix' in LEGS:                                                         # the route this replaces, on the same build
            whole = transducer.BeamDecoder(head, B, CAPACITY, W)
            for steps in (20, 250):
                x, il = feats[:, :steps].contiguous(), torch.full((B,), steps, dtype=torch.int64).cuda()
                whole.decode(x, il)
                times = [window(lambda: whole.decode(x, il), 1 if steps > 20 else args.reps) for _ in range(args.rounds)]
                res[f'prefix_{4 * steps}_frames'] = dict(summary(times), steps=whole.iterations)
                print(f'V={V:3d} W={W} BeamDecoder.decode of a prefix of {4 * steps} frames ({steps} steps): {res[f"prefix_{4 * steps}_frames"]}',
                      flush=True)
            del whole

        for chunk in (int(c) for c in args.chunks.split(',')):
            S, n_push = chunk // 4, args.frames // chunk
            assert args.frames % chunk == 0 and n_push * S <= 250
            stats = dict(on=False, rounds=0, needed=0, pushes=0)
            st = streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=CAPACITY, beam=W)
            greedy = streaming.StreamingTransducer(enc, head, B, chunk_frames=chunk, capacity=CAPACITY, max_symbols_per_frame=1, beam=0)
            plant(st, logits_all, S, n_push, stats)
            plant(greedy, logits_all, S, n_push)

            def one_stream(obj, pushes=n_push):
                for k in range(pushes):
                    obj.push(frames_all[:, k * chunk:(k + 1) * chunk], None, [k == 0] * B)

            def beam_leg(every):
                os.environ['HALO_RNNT_FUSED'] = '1'
                st.search.sync_every = every
                one_stream(st)

            def general_leg():
                os.environ['HALO_RNNT_FUSED'] = '0'
                assert not st.search.fused
                one_stream(st, args.general_pushes)
            legs, reps, pushes = {}, {}, {}
            if 'beam' in LEGS:
                for every in CADENCES:
                    legs[f'beam_every_{every}'] = lambda every=every: beam_leg(every)
            if 'greedy' in LEGS:
                legs['greedy'] = lambda: one_stream(greedy)
            if 'general' in LEGS:
                legs['general'] = general_leg
            for k in legs:
                reps[k], pushes[k] = (1, args.general_pushes) if k == 'general' else (args.reps, n_push)
            for fn in legs.values():
                fn()                                                                 # warm every leg
            times = {k: [] for k in legs}
            for _ in range(args.rounds):                                             # alternating windows
                for k, fn in legs.items():
                    times[k].append(window(fn, reps[k]) / pushes[k])
            os.environ['HALO_RNNT_FUSED'] = '1'
            r = dict(chunk_frames=chunk, steps_per_push=S, pushes_per_stream=n_push)
            for k in legs:
                r[k] = summary(times[k])
            if 'beam' in LEGS:                                                       # one more stream per cadence, untimed: the rounds
                for every in CADENCES:
                    stats.update(on=True, rounds=0, needed=0, pushes=0)
                    beam_leg(every)
                    stats['on'] = False
                    r[f'beam_every_{every}'].update(rounds_per_push=stats['rounds'] / stats['pushes'], needed_per_push=stats['needed'] / stats['pushes'],
                                                    share_past_last_live=1 - stats['needed'] / stats['rounds'])
                r['best_length_mean'] = float(st.partial()[1].float().mean())
            res[f'chunk_{chunk}'] = r
            print(f'V={V:3d} W={W} chunk {chunk:2d}: ' + ', '.join(f'{k} {r[k]["ms"]:.3f} ms/push' for k in legs), flush=True)
            for every in CADENCES if 'beam' in LEGS else ():
                e = r[f'beam_every_{every}']
                print(f'    every {every}: rounds/push {e["rounds_per_push"]:.2f}, needed {e["needed_per_push"]:.2f}, past the last live one '
                      f'{100 * e["share_past_last_live"]:.0f} %', flush=True)
            del st, greedy
        results.append(res)
os.environ.pop('HALO_RNNT_FUSED', None)

print(json.dumps(dict(bench='rnnt_stream_beam', streams=B, encoder='LC-2x1024', capacity=CAPACITY, frames=args.frames, mode='bf16x3',
                      rounds=args.rounds, reps=args.reps, general_pushes_per_window=args.general_pushes,
                      default_sync_every=transducer.STREAM_BEAM_SYNC_EVERY, results=results)))
