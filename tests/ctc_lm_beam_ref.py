"""Float64 restatement, on the CPU in plain torch, of CTC prefix beam search with shallow fusion of an LSTM language model
(haloop_amd.fusion.CTCFusionDecoder, csrc/ctc_lm_beam.hip; the definition in include/halo.h), and the fixtures that
tests/test_ctc_lm_beam_cpu.py and tests/test_gpu_ctc_lm_beam.py share.  No tests in here.

The emissions are those of tests/ctc_prefix_beam_ref.py (``inputs(name)``); the LM is an untrained ``rnn.Decoder(V, 512, 512, layers)``
from a fixed seed, evaluated here in float64 from its parameters.  With e[t, k] the log-probabilities of a row, L its frames, width W,
cap = capacity, a = lm_weight, b = insertion_bonus, a member of the beam is (y, pb, pnb, lm, lp, state): pb / pnb the CTC masses of
ctc_prefix_beam_ref, lm the LM's log-probability of y, lp = log_softmax(out_layer(h)) over all V classes after the LM consumed the start
token and then y, state the LSTM state behind lp.

    beam = [((), pb = 0, pnb = -inf, lm = 0, lp / state after one LM step on the start token from the zero state)]
    for t in 0 .. L-1:
        candidates and their order: ctc_prefix_beam_ref's; an extension of j by k carries lm_j + lp_j[k], a stay its member's lm; a
            merged extension contributes its CTC mass only
        beam = the W best by (logaddexp(pb', pnb') + a lm' + b len(y') descending, position ascending); CTC mass -inf is never kept
        a kept extension takes one LM step from its parent's state; a kept stay keeps lp and state
    result: the beam after frame L-1, best first: the ranking value, logaddexp(pb, pnb), lm.  L == 0: the empty hypothesis, all three 0.
"""
import functools

import torch

import ctc_prefix_beam_ref as P

NEG = float('-inf')
GAP = P.GAP
HIDDEN = 512            # the smallest hidden size the fused cells accept


def make_lm(V, layers, seed, emb=HIDDEN, hidden=HIDDEN):
    """An untrained rnn.Decoder in eval mode on the CPU, drawn from ``seed`` without touching the global generator's state."""
    from haloop_amd import rnn
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lm = rnn.Decoder(V, emb, hidden, layers)
    return lm.eval()


class LM64:
    """The LM of an rnn.Decoder in float64: embedding, LSTM layers with nn.LSTM's gate order (i, f, g, o), out_layer, log_softmax."""

    def __init__(self, lm):
        from haloop_amd.rnn import lstm_param_list
        self.wte = lm.embedding.weight.detach().double().cpu()
        self.out_w = lm.out_layer.weight.detach().double().cpu()
        self.out_b = lm.out_layer.bias.detach().double().cpu()
        p = [x.detach().double().cpu() for x in lstm_param_list(lm.rnn)]
        self.layers = [p[4 * l:4 * l + 4] for l in range(lm.num_layers)]
        self.hidden = lm.hidden_dim

    def zero_state(self, B):
        z = torch.zeros(len(self.layers), B, self.hidden, dtype=torch.float64)
        return z, z.clone()

    def step(self, tokens, h, c):
        """tokens [B] int64, h / c [layers, B, H] -> (lp [B, V], h, c)."""
        x = self.wte[tokens]
        hs, cs = [], []
        for l, (wi, wh, bi, bh) in enumerate(self.layers):
            i, f, g, o = (x @ wi.T + bi + h[l] @ wh.T + bh).chunk(4, 1)
            cn = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
            x = torch.sigmoid(o) * torch.tanh(cn)
            hs.append(x); cs.append(cn)
        return (x @ self.out_w.T + self.out_b).log_softmax(-1), torch.stack(hs), torch.stack(cs)

    def score(self, y, start_token=0):
        """The teacher-forced log-probability of the tokens y after the start token (0 for no tokens)."""
        h, c = self.zero_state(1)
        total, prev = 0.0, start_token
        for k in y:
            lp, h, c = self.step(torch.tensor([prev]), h, c)
            total += float(lp[0, k])
            prev = k
        return total


def beam_row(e_row, L, capacity, W, lm, a, b, start_token=0):
    """e_row [T, V] float64 -> (the beam after frame L-1: list of (tokens tuple, rank, ctc, lm), best first; merges; gap: the smallest
    margin by which a per-frame prune (W-th kept against best dropped) or a final adjacent ranking was decided, inf if none was)."""
    V = e_row.shape[1]
    h0, c0 = lm.zero_state(1)
    lp, h, c = lm.step(torch.tensor([start_token]), h0, c0)
    beam = [dict(y=(), pb=0.0, pnb=NEG, lm=0.0, rank=0.0, lp=lp[0], h=h[:, 0], c=c[:, 0])]
    merges, gap = 0, float('inf')
    for t in range(L):
        et = e_row[t]
        nb = len(beam)
        total = [P.lae(m['pb'], m['pnb']) for m in beam]
        spb = [total[j] + float(et[0]) for j in range(nb)]
        spnb = [m['pnb'] + float(et[m['y'][-1]]) if m['y'] else NEG for m in beam]
        ctc = torch.full((nb, V), NEG, dtype=torch.float64)           # the extensions' CTC mass; -inf: no candidate
        lmn = torch.zeros(nb, V, dtype=torch.float64)
        for j, m in enumerate(beam):
            if len(m['y']) >= capacity:
                continue
            ctc[j] = et + total[j]
            if m['y']:
                ctc[j, m['y'][-1]] = et[m['y'][-1]] + m['pb']
            lmn[j] = m['lm'] + m['lp']
        ctc[:, 0] = NEG
        where = {m['y']: j for j, m in enumerate(beam)}
        for s, m in enumerate(beam):                                    # the extension of y[:-1] by y[-1] merges into y's stay
            j = where.get(m['y'][:-1]) if m['y'] else None
            if j is not None and ctc[j, m['y'][-1]] > NEG:
                spnb[s] = P.lae(spnb[s], float(ctc[j, m['y'][-1]]))
                ctc[j, m['y'][-1]] = NEG
                merges += 1
        sctc = torch.tensor([P.lae(spb[j], spnb[j]) for j in range(nb)], dtype=torch.float64)
        slm = torch.tensor([m['lm'] for m in beam], dtype=torch.float64)
        slen = torch.tensor([float(len(m['y'])) for m in beam], dtype=torch.float64)
        stay_rank = torch.where(sctc > NEG, sctc + a * slm + b * slen, torch.full_like(sctc, NEG))
        ext_rank = torch.where(ctc > NEG, ctc + a * lmn + b * (slen[:, None] + 1), torch.full_like(ctc, NEG))
        vals = torch.cat([stay_rank, ext_rank.reshape(-1)])             # in candidate order: stay j at j, the extension at nb + j V + k
        order = torch.sort(-vals, stable=True).indices[:W + 1].tolist()
        order = [x for x in order if float(vals[x]) > NEG]
        if len(order) > W:
            gap = min(gap, float(vals[order[W - 1]] - vals[order[W]]))
        new, steps = [], []
        for x in order[:W]:
            if x < nb:
                m = beam[x]
                new.append(dict(m, pb=spb[x], pnb=spnb[x], rank=float(vals[x])))
            else:
                j, k = (x - nb) // V, (x - nb) % V
                m = beam[j]
                steps.append((len(new), j, k))
                new.append(dict(y=m['y'] + (k,), pb=NEG, pnb=float(ctc[j, k]), lm=float(lmn[j, k]), rank=float(vals[x])))
        if steps:                                                       # one LM step for the kept extensions, from their parents' state
            hs = torch.stack([beam[j]['h'] for _, j, _ in steps], 1)
            cs = torch.stack([beam[j]['c'] for _, j, _ in steps], 1)
            lp, hs, cs = lm.step(torch.tensor([k for _, _, k in steps]), hs, cs)
            for i, (r, _, _) in enumerate(steps):
                new[r].update(lp=lp[i], h=hs[:, i], c=cs[:, i])
        beam = new
    final = [(m['y'], m['rank'], P.lae(m['pb'], m['pnb']), m['lm']) for m in beam]
    for x in range(len(final) - 1):
        gap = min(gap, final[x][1] - final[x + 1][1])
    return final, merges, gap


def beam_search(emissions, emission_lengths, capacity, W, lm, a, b, start_token=0):
    """emissions [T, N, V], lm: an LM64 -> dict(tokens [N, W, capacity] int64 (-1 past a hypothesis's length and in absent ones),
    lengths [N, W] (-1: absent), scores / ctc_scores / lm_scores [N, W] float64 (-inf: absent), counts [N], merges [N], gaps [N])."""
    T, N, _ = emissions.shape
    e = emissions.double()
    tokens = torch.full((N, W, capacity), -1, dtype=torch.int64)
    lengths = torch.full((N, W), -1, dtype=torch.int64)
    scores, ctc, lms = (torch.full((N, W), NEG, dtype=torch.float64) for _ in range(3))
    counts, merges = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    gaps = torch.full((N,), float('inf'), dtype=torch.float64)
    for n in range(N):
        L = T if emission_lengths is None else max(0, min(int(emission_lengths[n]), T))
        final, merges[n], gaps[n] = beam_row(e[:, n], L, capacity, W, lm, a, b, start_token)
        counts[n] = len(final)
        for w, (y, s, cs, ls) in enumerate(final):
            lengths[n, w], scores[n, w], ctc[n, w], lms[n, w] = len(y), s, cs, ls
            tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
    return dict(tokens=tokens, lengths=lengths, scores=scores, ctc_scores=ctc, lm_scores=lms, counts=counts, merges=merges, gaps=gaps)


# ---- the cases the tests run: (emission fixture of ctc_prefix_beam_ref, W, LSTM layers, LM seed, lm_weight, insertion_bonus).  The LM
#      seeds were searched on the CPU with this file's loop for the conditions tests/test_ctc_lm_beam_cpu.py asserts. ----
CASES = [
    ('small', 4, 2, 1, 0.5, 0.0),
    ('small', 1, 2, 1, 0.7, 0.5),
    ('rows17', 4, 2, 1, 0.5, 0.0),
    ('rows17', 8, 2, 1, 0.7, 0.5),
    ('rows17cap', 4, 1, 1, 0.7, 0.5),
    ('wide', 3, 2, 1, 0.5, 0.0),
    ('long', 4, 2, 1, 0.5, 0.0),
    ('long', 16, 2, 11, 0.7, 0.5),
    ('tiny', 16, 2, 1, 0.5, 0.0),
    ('stream', 3, 2, 1, 0.7, 0.5),
]

# rows of a case whose smallest gap is below GAP: their tokens and scores are compared by no test
LEFT_OUT = {('rows17', 4, 2, 1, 0.5, 0.0): (15,), ('rows17', 8, 2, 1, 0.7, 0.5): (3,)}


@functools.lru_cache(maxsize=None)
def language_model(V, layers, seed):
    """-> (the rnn.Decoder on the CPU, its LM64).  Built once per process; callers must not modify the module (copy it to the device)."""
    lm = make_lm(V, layers, seed)
    return lm, LM64(lm)


@functools.lru_cache(maxsize=None)
def fixture(case):
    """case: a tuple of CASES -> (emissions, emission_lengths, capacity, the rnn.Decoder on the CPU, reference dict).  Computed once per
    process; callers must not modify what they get."""
    name, W, layers, seed, a, b = case
    emissions, il, capacity = P.inputs(name)
    lm, lm64 = language_model(emissions.shape[2], layers, seed)
    return emissions, il, capacity, lm, beam_search(emissions, il, capacity, W, lm64, a, b)


def compared_rows(case):
    N = P.FIXTURES[case[0]]['N']
    return [n for n in range(N) if n not in LEFT_OUT.get(case, ())]
