"""Float64 restatement, on the CPU in plain torch, of alignment-length synchronous beam search with exact merging ([Saon20] Saon,
Tueske, Audhkhasi: Alignment-length synchronous decoding for RNN transducer, ICASSP 2020) for haloop_amd.recognizer.Transducer, and
the fixtures that tests/test_rnnt_beam_cpu.py and tests/test_gpu_rnnt_beam.py share.  No tests in here.

The modules come from ``rnnt_greedy_ref.modules``.  With F = classifier(features), L = clamp(input_lengths[n], 0, T), beam width W and
cap = capacity, the search of row n is

    g0, state0 = lm_step(embedding[0], zeros)                              # the zero prefix of training
    B = [((), 0.0, g0, state0)]; finals = []
    if L == 0: finals = [((), 0.0)]
    for i in 0 .. L + cap - 1, while B is not empty:
        for hypothesis j of B, in order: t_j = i - len(y_j); lp_j = log_softmax(F[n, t_j] + g_j)         # t_j < L always holds
        candidates, in this order:
            for j in order: the blank extension (y_j, s_j + lp_j[0]); if t_j + 1 == L it is complete: appended to finals, no candidate
            for j in order, if len(y_j) < cap: for k = 1 .. V-1: (y_j + [k], s_j + lp_j[k])
        candidates with equal token sequences are merged into the earliest of them, scores combined by logaddexp
        B = the W best candidates by (score descending, candidate position ascending)
            a blank extension keeps its parent's g and state; a label extension gets lm_step(embedding[k], parent's state)
    result: finals sorted by (score descending, order of appending), the first W of them

All hypotheses alive at step i have consumed t frames and emitted u symbols with t + u = i, so equal token sequences sit at the same
frame and their scores add.  Without pruning every returned score is the lattice total log P(y | x) of its hypothesis.
"""
import functools

import torch

import rnnt_greedy_ref as G

E = G.E


@torch.no_grad()
def beam_row(mods, F_row, L, capacity, W):
    """One row -> (finals: list of (tokens tuple, score float) sorted, ALL of them, merges, gap)."""
    lstm, emb, ob, _, _ = mods
    V = emb.shape[0]

    def step(k, state):
        out, state = lstm(emb[k].view(1, 1, E), state)
        return torch.nn.functional.linear(out.view(E), emb, ob), state

    zeros = (torch.zeros(G.LAYERS, 1, E, dtype=torch.float64), torch.zeros(G.LAYERS, 1, E, dtype=torch.float64))
    g0, state0 = step(0, zeros)
    beam = [((), 0.0, g0, state0)] if L > 0 else []
    finals = [((), 0.0)] if L == 0 else []
    merges, gap = 0, float('inf')
    for i in range(L + capacity):
        if not beam:
            break
        lps = []
        for y, s, g, state in beam:
            t = i - len(y)
            assert 0 <= t < L
            lps.append((F_row[t] + g).log_softmax(-1))
        cands = []                                           # [tokens, score, parent j, k]
        for j, (y, s, g, state) in enumerate(beam):
            if i - len(y) + 1 == L:
                finals.append((y, s + float(lps[j][0])))
            else:
                cands.append([y, s + float(lps[j][0]), j, 0])
        for j, (y, s, g, state) in enumerate(beam):
            if len(y) < capacity:
                lp = lps[j].tolist()
                for k in range(1, V):
                    cands.append([y + (k,), s + lp[k], j, k])
        first, merged = {}, []
        for c in cands:
            at = first.get(c[0])
            if at is None:
                first[c[0]] = len(merged)
                merged.append(c)
            else:
                m = merged[at]
                m[1] = float(torch.logaddexp(torch.tensor(m[1], dtype=torch.float64), torch.tensor(c[1], dtype=torch.float64)))
                merges += 1
        order = sorted(range(len(merged)), key=lambda a: (-merged[a][1], a))
        if len(merged) > W:
            gap = min(gap, merged[order[W - 1]][1] - merged[order[W]][1])
        new = []
        for a in order[:W]:
            y, s, j, k = merged[a]
            if k == 0:
                new.append((y, s, beam[j][2], beam[j][3]))
            else:
                g, state = step(k, beam[j][3])
                new.append((y, s, g, state))
        beam = new
    assert not beam
    order = sorted(range(len(finals)), key=lambda a: (-finals[a][1], a))
    finals = [finals[a] for a in order]
    for a in range(min(W, len(finals) - 1)):
        gap = min(gap, finals[a][1] - finals[a + 1][1])
    return finals, merges, gap


@torch.no_grad()
def beam_search(sd, features, input_lengths, capacity, W):
    """-> dict(tokens [N, W, capacity] int64 (-1 past a hypothesis's length and in absent ones), lengths [N, W] (-1: absent), scores
    [N, W] float64 (-inf: absent), counts [N], merges [N], gaps [N] float64 (inf where nothing was compared))."""
    mods = G.modules(sd)
    N, T, _ = features.shape
    F = torch.nn.functional.linear(features.double(), mods[3], mods[4])
    tokens = torch.full((N, W, capacity), -1, dtype=torch.int64)
    lengths = torch.full((N, W), -1, dtype=torch.int64)
    scores = torch.full((N, W), float('-inf'), dtype=torch.float64)
    counts, merges = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    gaps = torch.full((N,), float('inf'), dtype=torch.float64)
    for n in range(N):
        L = max(0, min(int(input_lengths[n]), T))
        finals, merges[n], gaps[n] = beam_row(mods, F[n], L, capacity, W)
        counts[n] = min(W, len(finals))
        for w, (y, s) in enumerate(finals[:W]):
            lengths[n, w], scores[n, w] = len(y), s
            tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
    return dict(tokens=tokens, lengths=lengths, scores=scores, counts=counts, merges=merges, gaps=gaps)


@torch.no_grad()
def lattice_total(sd, features_row, L, hyp):
    """log P(hyp | the row's first L frames): the alpha recursion over ``rnnt_greedy_ref.teacher_forced_joint`` in float64."""
    joint = G.teacher_forced_joint(sd, features_row, hyp)                        # [T, U + 1, V]
    U = hyp.numel()
    neg = torch.tensor(float('-inf'), dtype=torch.float64)
    alpha = [[neg] * (U + 1) for _ in range(L)]
    for t in range(L):
        for u in range(U + 1):
            if t == 0 and u == 0:
                alpha[t][u] = torch.tensor(0.0, dtype=torch.float64)
                continue
            a = alpha[t - 1][u] + joint[t - 1, u, 0] if t > 0 else neg
            b = alpha[t][u - 1] + joint[t, u - 1, hyp[u - 1]] if u > 0 else neg
            alpha[t][u] = torch.logaddexp(a, b)
    return float(alpha[L - 1][U] + joint[L - 1, U, 0])


# ---- fixtures: a random-initialised Transducer(V, V) whose classifier is the identity, on features with planted symbols: randn plus 7.0
#      on a drawn label channel in a quarter of the frames and on the blank channel elsewhere, plus 4.5 on the blank channel everywhere.
#      The seeds were searched on the CPU with this file's loop for the conditions tests/test_rnnt_beam_cpu.py asserts. ----
GAP = 1e-3            # ten times the project's fp32-grade tolerance on features (as tests/test_rnnt_greedy_cpu.py)
FIXTURES = {
    # name: (seed, N, T, V, input_lengths (None: drawn from the seed, one 0 among them), capacity)
    'small': dict(seed=1, N=3, T=12, V=20, lengths=[12, 9, 1], capacity=6),
    'rows17': dict(seed=1, N=17, T=23, V=67, lengths=None, capacity=10),
    'wide': dict(seed=3, N=2, T=6, V=1031, lengths=[6, 4], capacity=4),
    'stream': dict(seed=2, N=2, T=6, V=4099, lengths=[6, 4], capacity=4),     # W V above what the step kernel keeps in LDS
    'tiny': dict(seed=1, N=2, T=5, V=4, lengths=[5, 3], capacity=2),          # W = 16 holds all 13 sequences: nothing is pruned
}


def planted(gen, N, T, V):
    x = torch.randn(N, T, V, generator=gen)
    lab = torch.randint(1, V, (N, T), generator=gen)
    is_lab = torch.rand(N, T, generator=gen) < 0.25
    ch = torch.where(is_lab, lab, torch.zeros_like(lab))
    x.scatter_add_(2, ch[:, :, None], torch.full((N, T, 1), 7.0))
    x[:, :, 0] += 4.5
    return x


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (state dict (float32, CPU), features [N, T, V] float32, input_lengths [N] int64, capacity).  Computed once per process; callers
    must not modify what they get."""
    from haloop_amd import recognizer
    f = FIXTURES[name]
    V = f['V']
    gen = torch.Generator().manual_seed(f['seed'])
    saved = torch.get_rng_state()
    torch.manual_seed(f['seed'])
    head = recognizer.Transducer(V, V).eval()
    torch.set_rng_state(saved)
    sd = {k: v.detach().clone() for k, v in head.state_dict().items()}
    sd['classifier.weight'] = torch.eye(V)
    sd['classifier.bias'] = torch.zeros(V)
    features = planted(gen, f['N'], f['T'], V)
    if f['lengths'] is None:
        il = torch.randint(1, f['T'] + 1, (f['N'],), generator=gen)
        il[int(torch.randint(0, f['N'], (1,), generator=gen))] = 0
    else:
        il = torch.tensor(f['lengths'])
    return sd, features, il, f['capacity']


@functools.lru_cache(maxsize=None)
def fixture(name, W):
    """-> (state dict, features, input_lengths, capacity, reference dict of ``beam_search`` at width W).  Computed once per process;
    callers must not modify what they get."""
    sd, features, il, capacity = inputs(name)
    return sd, features, il, capacity, beam_search(sd, features, il, capacity, W)


# rows of (fixture, W) whose smallest gap is below GAP: their tokens and scores are compared by no test
LEFT_OUT = {('rows17', 8): (7, 12, 15)}


def compared_rows(name, W):
    N = FIXTURES[name]['N']
    return [n for n in range(N) if n not in LEFT_OUT.get((name, W), ())]
