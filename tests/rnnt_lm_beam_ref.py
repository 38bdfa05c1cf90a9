"""Float64 restatement, on the CPU in plain torch, of transducer beam search with shallow fusion of an LSTM language model
(haloop_amd.fusion.TransducerFusionDecoder, csrc/rnnt_lm_beam.hip; the definition in include/halo.h), and the fixtures that
tests/test_rnnt_lm_beam_cpu.py and tests/test_gpu_rnnt_lm_beam.py share.  No tests in here.

The heads, features and lengths are those of tests/rnnt_beam_ref.py (``inputs(name)``); the LM is ``ctc_lm_beam_ref.language_model``: an
untrained ``rnn.Decoder(V, 512, 512, layers)`` from a fixed seed, evaluated in float64 by ``LM64``.  With F = classifier(features), L =
clamp(input_lengths[n], 0, T), width W, cap = capacity, a = lm_weight, b = insertion_bonus, a member of the beam is (y, s, lm, g, pstate,
lp, lstate): s the transducer mass of rnnt_beam_ref, lm the LM's log-probability of y, g / pstate the prediction network after the zero
prefix and then y, lp / lstate the LM after the start token and then y.

    B = [((), 0, 0, one prediction-network step on token 0, one LM step on the start token)]; finals = []
    if L == 0: finals = [((), rank 0, s 0, lm 0)]
    for i in 0 .. L + cap - 1, while B is not empty:
        t_j = i - len(y_j); q_j = log_softmax(F[n, t_j] + g_j)
        candidates and their order: rnnt_beam_ref's; a blank carries lm_j, the extension of j by k carries lm_j + lp_j[k]; equal token
            sequences merge into the earliest: masses by logaddexp, the earliest keeps its own lm'
        rank = s' + a lm' + b len(y'); a complete blank goes to the finals with its rank
        B = the W best by (rank descending, position ascending); a kept label steps BOTH networks from its parent's states
    result: finals sorted by (rank descending, order of appending), the first W of them
"""
import functools

import torch

import ctc_lm_beam_ref as C
import rnnt_beam_ref as B
import rnnt_greedy_ref as G

NEG = float('-inf')
GAP = B.GAP
LM64, language_model, make_lm = C.LM64, C.language_model, C.make_lm


@torch.no_grad()
def beam_row(mods, F_row, L, capacity, W, lm, a, b, start_token=0):
    """One row -> (finals: list of (tokens tuple, rank, s, lm) sorted, ALL of them; merges; gap: the smallest margin in rank by which a
    prune (W-th kept against best dropped) or a final adjacent ranking among the first W + 1 was decided, inf if none was)."""
    lstm, emb, ob, _, _ = mods
    V, E = emb.shape[0], G.E

    def step(k, state):
        out, state = lstm(emb[k].view(1, 1, E), state)
        return torch.nn.functional.linear(out.view(E), emb, ob), state

    zeros = (torch.zeros(G.LAYERS, 1, E, dtype=torch.float64), torch.zeros(G.LAYERS, 1, E, dtype=torch.float64))
    g0, state0 = step(0, zeros)
    lp0, h0, c0 = lm.step(torch.tensor([start_token]), *lm.zero_state(1))
    beam = [dict(y=(), s=0.0, lm=0.0, g=g0, state=state0, lp=lp0[0], h=h0, c=c0)] if L > 0 else []
    finals = [((), 0.0, 0.0, 0.0)] if L == 0 else []
    merges, gap = 0, float('inf')
    for i in range(L + capacity):
        if not beam:
            break
        qs = []
        for m in beam:
            t = i - len(m['y'])
            assert 0 <= t < L
            qs.append((F_row[t] + m['g']).log_softmax(-1))
        cands = []                                           # [tokens, s', lm', parent j, k]
        complete = [i - len(m['y']) + 1 == L for m in beam]
        for j, m in enumerate(beam):
            cands.append([m['y'], m['s'] + float(qs[j][0]), m['lm'], j, 0])
        for j, m in enumerate(beam):
            if len(m['y']) < capacity:
                q, lp = qs[j].tolist(), m['lp'].tolist()
                for k in range(1, V):
                    cands.append([m['y'] + (k,), m['s'] + q[k], m['lm'] + lp[k], j, k])
        first, merged = {}, []
        for c in cands:
            if c[4] == 0 and complete[c[3]]:                 # a complete blank is no candidate: nothing merges into it
                continue
            at = first.get(c[0])
            if at is None:
                first[c[0]] = len(merged)
                merged.append(c)
            else:
                m = merged[at]
                m[1] = float(torch.logaddexp(torch.tensor(m[1], dtype=torch.float64), torch.tensor(c[1], dtype=torch.float64)))
                merges += 1
        for j, m in enumerate(beam):
            if complete[j]:
                s = m['s'] + float(qs[j][0])
                finals.append((m['y'], s + a * m['lm'] + b * len(m['y']), s, m['lm']))
        ranks = [c[1] + a * c[2] + b * len(c[0]) for c in merged]
        order = sorted(range(len(merged)), key=lambda x: (-ranks[x], x))
        if len(merged) > W:
            gap = min(gap, ranks[order[W - 1]] - ranks[order[W]])
        new = []
        for x in order[:W]:
            y, s, lms, j, k = merged[x]
            p = beam[j]
            if k == 0:
                new.append(dict(p, s=s))
            else:
                g, state = step(k, p['state'])
                lp, h, c = lm.step(torch.tensor([k]), p['h'], p['c'])
                new.append(dict(y=y, s=s, lm=lms, g=g, state=state, lp=lp[0], h=h, c=c))
        beam = new
    assert not beam
    order = sorted(range(len(finals)), key=lambda x: (-finals[x][1], x))
    finals = [finals[x] for x in order]
    for x in range(min(W, len(finals) - 1)):
        gap = min(gap, finals[x][1] - finals[x + 1][1])
    return finals, merges, gap


@torch.no_grad()
def beam_search(sd, features, input_lengths, capacity, W, lm, a, b, start_token=0):
    """lm: an LM64 -> dict(tokens [N, W, capacity] int64 (-1 past a hypothesis's length and in absent ones), lengths [N, W] (-1: absent),
    scores / rnnt_scores / lm_scores [N, W] float64 (-inf: absent), counts [N], merges [N], gaps [N] float64 (inf: nothing compared))."""
    mods = G.modules(sd)
    N, T, _ = features.shape
    F = torch.nn.functional.linear(features.double(), mods[3], mods[4])
    tokens = torch.full((N, W, capacity), -1, dtype=torch.int64)
    lengths = torch.full((N, W), -1, dtype=torch.int64)
    scores, rnnt, lms = (torch.full((N, W), NEG, dtype=torch.float64) for _ in range(3))
    counts, merges = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    gaps = torch.full((N,), float('inf'), dtype=torch.float64)
    for n in range(N):
        L = max(0, min(int(input_lengths[n]), T))
        finals, merges[n], gaps[n] = beam_row(mods, F[n], L, capacity, W, lm, a, b, start_token)
        counts[n] = min(W, len(finals))
        for w, (y, r, s, m) in enumerate(finals[:W]):
            lengths[n, w], scores[n, w], rnnt[n, w], lms[n, w] = len(y), r, s, m
            tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
    return dict(tokens=tokens, lengths=lengths, scores=scores, rnnt_scores=rnnt, lm_scores=lms, counts=counts, merges=merges, gaps=gaps)


# ---- the cases the tests run: (fixture of rnnt_beam_ref, W, LM layers, LM seed, lm_weight, insertion_bonus).  The bonus is
#      round(lm_weight * ln V, 1): without one an untrained LM (about -ln V per token) drives nearly every best hypothesis to the empty one.
#      Checked on the CPU with this file's loop for the conditions tests/test_rnnt_lm_beam_cpu.py asserts. ----
CASES = [
    ('small', 4, 2, 1, 0.5, 1.5),
    ('small', 1, 2, 1, 0.7, 2.1),
    ('tiny', 16, 2, 1, 0.5, 0.7),
    ('rows17', 4, 2, 1, 0.5, 2.1),
    ('rows17', 8, 1, 1, 0.7, 2.9),          # a one-layer LM under the two-layer prediction network
    ('wide', 3, 2, 1, 0.5, 3.5),            # V = 1031, 2 W V = 6186 floats: both tables in LDS
    ('stream', 3, 2, 1, 0.7, 5.8),          # V = 4099, 2 W V = 24594 floats: both tables recomputed from L2
]

# rows of a case whose smallest gap is below GAP: their tokens and scores are compared by no test
LEFT_OUT = {('rows17', 8, 1, 1, 0.7, 2.9): (4, 14)}


@functools.lru_cache(maxsize=None)
def fixture(case):
    """case: a tuple of CASES -> (state dict, features, input_lengths, capacity, the rnn.Decoder on the CPU, reference dict).  Computed
    once per process; callers must not modify what they get."""
    name, W, layers, seed, a, b = case
    sd, features, il, capacity = B.inputs(name)
    lm, lm64 = language_model(B.FIXTURES[name]['V'], layers, seed)
    return sd, features, il, capacity, lm, beam_search(sd, features, il, capacity, W, lm64, a, b)


def compared_rows(case):
    N = B.FIXTURES[case[0]]['N']
    return [n for n in range(N) if n not in LEFT_OUT.get(case, ())]
