"""Float64 restatement, on the CPU in plain Python and torch, of CTC prefix beam search with exact merging ([Hannun14] Hannun, Maas,
Jurafsky, Ng: First-pass large vocabulary continuous speech recognition using bi-directional recurrent DNNs, 2014; Graves' prefix search)
for haloop_amd.ctc.ctc_prefix_beam_search, and the fixtures that tests/test_ctc_prefix_beam_cpu.py and
tests/test_gpu_ctc_prefix_beam.py share.  No tests in here.

With e[t, k] the given log-probabilities (class 0 the blank; not normalised here), L = clamp(emission_lengths[n], 0, T), width W and
cap = capacity, the search of row n is

    beam = [((), pb = 0, pnb = -inf)]                    # pb / pnb: log-mass of alignments of the prefix ending in blank / in its last label
    for t in 0 .. L-1:
        total_j = logaddexp(pb_j, pnb_j)
        candidates, in this order:
            for j in beam order: stay       (y_j,       pb' = total_j + e[t,0],  pnb' = pnb_j + e[t, last(y_j)]  (-inf for the empty prefix))
            for j in beam order, if len(y_j) < cap, for k = 1 .. V-1:
                                 extension  (y_j + [k], pb' = -inf,  pnb' = e[t,k] + (pb_j if k == last(y_j) else total_j))
        an extension that spells the prefix of a stay candidate s is merged into it (pnb'_s = logaddexp(pnb'_s, extension's pnb')) and dropped
        beam = the W best candidates by (logaddexp(pb', pnb') descending, candidate position ascending); candidates at -inf are never kept
    result: the beam after frame L-1, in that order; score = logaddexp(pb, pnb).  L == 0: the empty hypothesis alone, score 0.

Two different beam members can never extend to the same prefix, so merging into stay candidates is the only merge there is.  Without
pruning every score is the CTC lattice total log P(y | x); with pruning a lower bound of it.
"""
import functools
import math

import torch

NEG = float('-inf')


def lae(a, b):
    m = max(a, b)
    return m if m == NEG else m + math.log1p(math.exp(-abs(a - b)))


def beam_row(e_row, L, capacity, W):
    """e_row [T, V] float64 -> (the beam after frame L-1: list of (tokens tuple, score float), best first; merges; gap: the smallest
    margin by which a per-frame prune (W-th kept against best dropped) or a final adjacent ranking was decided, inf if none was)."""
    V = e_row.shape[1]
    beam = [((), 0.0, NEG)]
    merges, gap = 0, float('inf')
    for t in range(L):
        et = e_row[t].tolist()
        total = [lae(pb, pnb) for _, pb, pnb in beam]
        cands = [[y, total[j] + et[0], pnb + et[y[-1]] if y else NEG] for j, (y, pb, pnb) in enumerate(beam)]
        stays = {c[0]: s for s, c in enumerate(cands)}
        for j, (y, pb, pnb) in enumerate(beam):
            if len(y) >= capacity:
                continue
            for k in range(1, V):
                v = et[k] + (pb if y and k == y[-1] else total[j])
                s = stays.get(y + (k,))
                if s is None:
                    cands.append([y + (k,), NEG, v])
                else:
                    cands[s][2] = lae(cands[s][2], v)
                    merges += 1
        score = [lae(pb, pnb) for _, pb, pnb in cands]
        order = sorted((a for a in range(len(cands)) if score[a] > NEG), key=lambda a: (-score[a], a))
        if len(order) > W:
            gap = min(gap, score[order[W - 1]] - score[order[W]])
        beam = [tuple(cands[a]) for a in order[:W]]
    final = [(y, lae(pb, pnb)) for y, pb, pnb in beam]
    for a in range(len(final) - 1):
        gap = min(gap, final[a][1] - final[a + 1][1])
    return final, merges, gap


def beam_search(emissions, emission_lengths, capacity, W):
    """emissions [T, N, V] -> dict(tokens [N, W, capacity] int64 (-1 past a hypothesis's length and in absent ones), lengths [N, W] (-1:
    absent), scores [N, W] float64 (-inf: absent), counts [N], merges [N], gaps [N] float64 (inf where nothing was compared))."""
    T, N, _ = emissions.shape
    e = emissions.double()
    tokens = torch.full((N, W, capacity), -1, dtype=torch.int64)
    lengths = torch.full((N, W), -1, dtype=torch.int64)
    scores = torch.full((N, W), NEG, dtype=torch.float64)
    counts, merges = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    gaps = torch.full((N,), float('inf'), dtype=torch.float64)
    for n in range(N):
        L = T if emission_lengths is None else max(0, min(int(emission_lengths[n]), T))
        final, merges[n], gaps[n] = beam_row(e[:, n], L, capacity, W)
        counts[n] = len(final)
        for w, (y, s) in enumerate(final):
            lengths[n, w], scores[n, w] = len(y), s
            tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
    return dict(tokens=tokens, lengths=lengths, scores=scores, counts=counts, merges=merges, gaps=gaps)


def lattice_totals(emissions, emission_lengths, ref, n):
    """log P(hypothesis | the row's frames) of every present hypothesis of row n: minus torch's own CTC loss in float64 on the CPU."""
    count = int(ref['counts'][n])
    hyp = ref['tokens'][n, :count].clamp(min=0)
    lp = emissions[:, n].double()[:, None, :].expand(-1, count, -1)
    il = torch.full((count,), int(emission_lengths[n]), dtype=torch.int64)
    return -torch.nn.functional.ctc_loss(lp, hyp, il, ref['lengths'][n, :count], blank=0, reduction='none', zero_infinity=False)


# ---- fixtures: log_softmax of randn logits, optionally plus a bonus planted on one drawn class (the blank among them) per frame.  The
#      seeds were searched on the CPU with this file's loop for the conditions tests/test_ctc_prefix_beam_cpu.py asserts. ----
GAP = 1e-3            # the project's value (rnnt_beam_ref.GAP): ten times its fp32-grade tolerance
FIXTURES = {
    # name: seed, N, T, V, emission lengths, capacity, the planted bonus (0: none)
    'small': dict(seed=1, N=3, T=6, V=5, lengths=[6, 4, 0], capacity=6, bonus=0.0),
    'rows17': dict(seed=1, N=17, T=12, V=8, lengths=[0 if n == 9 else 12 - n % 5 for n in range(17)], capacity=12, bonus=2.0),
    'rows17cap': dict(seed=1, N=17, T=12, V=8, lengths=[0 if n == 9 else 12 - n % 5 for n in range(17)], capacity=3, bonus=2.0),
    'wide': dict(seed=32, N=2, T=5, V=300, lengths=[5, 3], capacity=5, bonus=0.0),      # V above the workgroup, no multiple of 64
    'long': dict(seed=73, N=2, T=70, V=6, lengths=[70, 45], capacity=70, bonus=3.0),   # the frame loop past 64, long prefixes
    'tiny': dict(seed=4, N=2, T=4, V=3, lengths=[4, 4], capacity=3, bonus=0.0),       # W = 16 holds all 13 hypotheses: no pruning
    # the paths the shapes above do not reach (csrc/ctc_prefix_beam.hip): V above 4096, the emissions read from L2 in every round;
    # 2 W capacity above 12288, the token rows in the workspace.  The second needs T = capacity >= 385 at W = 16: a bonus of 6.0 keeps
    # the 16 kept scores above about -30, so fp32 rounding over the frame sum (400 x 6e-8 x 30 = 7e-4 if every rounding went one way,
    # about its root-T share of 4e-5 in a run) stays under GAP and the score tolerance, as the 70 frames of 'long' do at scores near -50
    'stream': dict(seed=4, N=2, T=4, V=4100, lengths=[4, 3], capacity=4, bonus=0.0),
    'deep': dict(seed=14, N=1, T=400, V=3, lengths=[400], capacity=400, bonus=6.0),
    # both at once, and tokens that do not fit 16 bits (V above 65536 sends the token rows to the workspace too): a bonus of 14.0 against
    # the mass of 70000 classes; the best hypothesis holds token 67177
    'huge': dict(seed=3, N=1, T=2, V=70000, lengths=[2], capacity=2, bonus=14.0),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (emissions [T, N, V] float32 log-probabilities, emission_lengths [N] int64, capacity).  Computed once per process; callers must
    not modify what they get."""
    f = FIXTURES[name]
    gen = torch.Generator().manual_seed(f['seed'])
    x = torch.randn(f['T'], f['N'], f['V'], generator=gen)
    if f['bonus']:
        cls = torch.randint(0, f['V'], (f['T'], f['N']), generator=gen)
        x.scatter_add_(2, cls[:, :, None], torch.full((f['T'], f['N'], 1), f['bonus']))
    return x.log_softmax(-1), torch.tensor(f['lengths'], dtype=torch.int64), f['capacity']


@functools.lru_cache(maxsize=None)
def fixture(name, W):
    """-> (emissions, emission_lengths, capacity, reference dict of ``beam_search`` at width W).  Computed once per process; callers must
    not modify what they get."""
    emissions, il, capacity = inputs(name)
    return emissions, il, capacity, beam_search(emissions, il, capacity, W)


# the (fixture, W) pairs the tests run
CASES = [('small', 4), ('small', 1), ('rows17', 4), ('rows17', 8), ('rows17cap', 4), ('wide', 3), ('long', 4), ('long', 16), ('tiny', 16),
         ('stream', 3), ('deep', 16), ('huge', 2)]

# rows of (fixture, W) whose smallest gap is below GAP: their tokens and scores are compared by no test
LEFT_OUT = {('rows17', 4): (7,), ('rows17', 8): (6, 7)}


def compared_rows(name, W):
    N = FIXTURES[name]['N']
    return [n for n in range(N) if n not in LEFT_OUT.get((name, W), ())]
