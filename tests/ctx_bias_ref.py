"""Float64 restatement, on the CPU in plain Python and torch, of the contextually biased CTC prefix beam search
(haloop_amd.ctc.ctc_prefix_beam_search(context=...), include/halo.h: halo_ctc_prefix_beam_biased), a brute-force statement of the boost
that uses no failure links and no tables, and the fixtures that tests/test_ctx_bias_cpu.py and tests/test_gpu_ctx_bias.py share.  No
tests in here.

The search is tests/ctc_prefix_beam_ref.py's loop -- the same candidate order, the same merge, the same gap bookkeeping -- with ranks in
place of scores: a member is (y, pb, pnb, c, z), c the state of the phrase automaton after y and z the boost y holds; a stay candidate
ranks by logaddexp(pb', pnb') + z, the extension of j by k by its CTC mass + z_j + gain(c_j, k); a candidate whose CTC mass is -inf is
never kept; pb / pnb stay CTC masses.

The brute force (``Brute``): the state after a text is the longest suffix of the text that is a path of the phrases' trie, found by
trying the suffixes from the longest; d(s) is its length; fa(s), straight from the phrase set, is the length of the longest proper prefix
of s that is a phrase (0: none); held(s) = 0 if s is a phrase else bonus * (d(s) - fa(s)); the token that leads from s to s' gains
bonus * (d(s') - fa(s')) - held(s).  States are numbered as haloop_amd.biasing.ContextGraph numbers them: the root 0, then every new
prefix in the order the phrases spell them.
"""
import functools

import torch

import ctc_prefix_beam_ref as R

NEG, lae, GAP = R.NEG, R.lae, R.GAP


class Brute:
    def __init__(self, phrases, bonus):
        self.phrases = {tuple(p) for p in phrases}
        self.bonus = float(bonus)
        self.index = {(): 0}
        for p in phrases:
            for i in range(1, len(p) + 1):
                self.index.setdefault(tuple(p[:i]), len(self.index))
        self.longest = max((len(p) for p in self.phrases), default=0)

    def fa(self, s):
        return max((i for i in range(1, len(s)) if s[:i] in self.phrases), default=0)

    def value(self, s):
        return self.bonus * (len(s) - self.fa(s))

    def held(self, s):
        return 0.0 if s in self.phrases else self.value(s)

    def step(self, s, k):
        """(the state, a tuple of tokens; a token) -> (the next state, the gain in float64)"""
        text = s + (k,)
        for i in range(len(text) + 1):                                  # the suffixes, longest first; the empty one is the root
            if text[i:] in self.index:
                nxt = text[i:]
                break
        return nxt, self.value(nxt) - self.held(s)

    def boost(self, tokens):
        """-> (the state after the text, its boost: the gains added left to right in float64, the list of the gains)"""
        s, z, gains = (), 0.0, []
        for k in tokens:
            s, g = self.step(s, int(k))
            gains.append(g)
            z += g
        return s, z, gains


def beam_row(e_row, L, capacity, W, brute):
    """ctc_prefix_beam_ref.beam_row with ranks: -> (list of (tokens, rank, boost, state index), best first; merges; gap)."""
    V = e_row.shape[1]
    beam = [((), 0.0, NEG, (), 0.0)]
    merges, gap = 0, float('inf')
    for t in range(L):
        et = e_row[t].tolist()
        total = [lae(pb, pnb) for _, pb, pnb, _, _ in beam]
        cands = [[y, total[j] + et[0], pnb + et[y[-1]] if y else NEG, c, z] for j, (y, pb, pnb, c, z) in enumerate(beam)]
        stays = {c[0]: s for s, c in enumerate(cands)}
        steps = {}
        for j, (y, pb, pnb, c, z) in enumerate(beam):
            if len(y) >= capacity:
                continue
            for k in range(1, V):
                v = et[k] + (pb if y and k == y[-1] else total[j])
                s = stays.get(y + (k,))
                if s is None:
                    if (c, k) not in steps:
                        steps[c, k] = brute.step(c, k)
                    c2, g = steps[c, k]
                    cands.append([y + (k,), NEG, v, c2, z + g])
                else:
                    cands[s][2] = lae(cands[s][2], v)
                    merges += 1
        mass = [lae(pb, pnb) for _, pb, pnb, _, _ in cands]
        rank = [m + c[4] for m, c in zip(mass, cands)]
        order = sorted((a for a in range(len(cands)) if mass[a] > NEG), key=lambda a: (-rank[a], a))
        if len(order) > W:
            gap = min(gap, rank[order[W - 1]] - rank[order[W]])
        beam = [tuple(cands[a]) for a in order[:W]]
    final = [(y, lae(pb, pnb) + z, z, brute.index[c]) for y, pb, pnb, c, z in beam]
    for a in range(len(final) - 1):
        gap = min(gap, final[a][1] - final[a + 1][1])
    return final, merges, gap


def beam_search(emissions, emission_lengths, capacity, W, phrases, bonus):
    """emissions [T, N, V] -> ctc_prefix_beam_ref.beam_search's dict with scores = ranks, and boosts [N, W] float64 (0 where absent),
    states [N, W] int64 (-1 where absent)."""
    T, N, _ = emissions.shape
    e = emissions.double()
    brute = Brute(phrases, bonus)
    tokens = torch.full((N, W, capacity), -1, dtype=torch.int64)
    lengths = torch.full((N, W), -1, dtype=torch.int64)
    scores = torch.full((N, W), NEG, dtype=torch.float64)
    boosts = torch.zeros((N, W), dtype=torch.float64)
    states = torch.full((N, W), -1, dtype=torch.int64)
    counts, merges = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    gaps = torch.full((N,), float('inf'), dtype=torch.float64)
    for n in range(N):
        L = T if emission_lengths is None else max(0, min(int(emission_lengths[n]), T))
        final, merges[n], gaps[n] = beam_row(e[:, n], L, capacity, W, brute)
        counts[n] = len(final)
        for w, (y, s, z, c) in enumerate(final):
            lengths[n, w], scores[n, w], boosts[n, w], states[n, w] = len(y), s, z, c
            tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
    return dict(tokens=tokens, lengths=lengths, scores=scores, counts=counts, merges=merges, gaps=gaps, boosts=boosts, states=states)


# ---- fixtures: the emissions of ctc_prefix_beam_ref.FIXTURES, each with a phrase list.  'seed': six phrases of one to three tokens drawn
#      from 1 .. min(V, 64) - 1 by random_phrases(seed); 'nbest': phrases cut from the fixture's own unbiased n-best lists at that width
#      (the whole of every present non-empty hypothesis behind the best one), where a drawn list would never be spelled.  The seeds were
#      searched on the CPU with this file's loop, from 0 upwards, for the conditions tests/test_ctx_bias_cpu.py asserts. ----
BONUS = 1.5


def random_phrases(seed, V, count=6, longest=3):
    gen = torch.Generator().manual_seed(seed)
    top = min(V, 64)
    out = []
    for _ in range(count):
        n = int(torch.randint(1, longest + 1, (1,), generator=gen))
        out.append(tuple(int(k) for k in torch.randint(1, top, (n,), generator=gen)))
    return out


def nbest_phrases(name, W):
    ref = R.fixture(name, W)[3]
    out = []
    for n in range(ref['tokens'].shape[0]):
        for w in range(1, int(ref['counts'][n])):
            y = tuple(ref['tokens'][n, w, :int(ref['lengths'][n, w])].tolist())
            if y and y not in out:
                out.append(y)
    return out


# (fixture, W): the seed of its phrase list, or 'nbest'
PHRASES = {
    ('small', 4): 0, ('small', 1): 0, ('rows17', 4): 0, ('rows17', 8): 0, ('rows17cap', 4): 0, ('wide', 3): 0, ('long', 4): 0,
    ('long', 16): 1, ('tiny', 16): 0, ('stream', 3): 'nbest', ('deep', 16): 0, ('huge', 2): 'nbest',
}
CASES = list(R.CASES)

# rows of (fixture, W) whose smallest gap is below GAP: their tokens and scores are compared by no test that needs a ranking decided
LEFT_OUT = {}


def compared_rows(name, W):
    N = R.FIXTURES[name]['N']
    return [n for n in range(N) if n not in LEFT_OUT.get((name, W), ())]


@functools.lru_cache(maxsize=None)
def phrases(name, W):
    how = PHRASES[name, W]
    return tuple(nbest_phrases(name, W) if how == 'nbest' else random_phrases(how, R.FIXTURES[name]['V']))


@functools.lru_cache(maxsize=None)
def graph(name, W, bonus=BONUS):
    """The fixture's haloop_amd.biasing.ContextGraph.  Computed once per process."""
    from haloop_amd.biasing import ContextGraph
    return ContextGraph(phrases(name, W), R.FIXTURES[name]['V'], bonus)


@functools.lru_cache(maxsize=None)
def fixture(name, W):
    """-> (emissions, emission_lengths, capacity, reference dict of the biased ``beam_search`` at width W).  Computed once per process;
    callers must not modify what they get."""
    emissions, il, capacity = R.inputs(name)
    return emissions, il, capacity, beam_search(emissions, il, capacity, W, phrases(name, W), BONUS)


# ---- the planted case: one row of T = 6 frames over V = 6 classes (log_softmax of 3 randn) whose unbiased search at W = 2 no longer
#      holds PLANTED['phrase'] after the last frame (it returns (5, 2, 4) and (5, 2, 5, 4)), while the search biased towards that one
#      phrase returns it first.  Found on the CPU by find_planted(): the first seed that has one. ----
PLANTED = dict(seed=25, T=6, V=6, W=2, scale=3.0, phrase=(5, 4), bonus=1.5)


@functools.lru_cache(maxsize=None)
def planted_inputs():
    f = PLANTED
    gen = torch.Generator().manual_seed(f['seed'])
    return (f['scale'] * torch.randn(f['T'], 1, f['V'], generator=gen)).log_softmax(-1), torch.tensor([f['T']], dtype=torch.int64), f['T']


def hypotheses(ref, n):
    return [tuple(ref['tokens'][n, w, :int(ref['lengths'][n, w])].tolist()) for w in range(int(ref['counts'][n]))]


def find_planted(seeds=range(300), T=6, V=6, W=2, scale=3.0, bonus=1.5):
    """The search that found PLANTED: the first seed and two-token phrase (in the order of the unbiased width-8 list) that the unbiased
    width-W search has lost by the last frame and the biased one returns first, every ranking of both decided by GAP."""
    for seed in seeds:
        gen = torch.Generator().manual_seed(seed)
        e = (scale * torch.randn(T, 1, V, generator=gen)).log_softmax(-1)
        plain = R.beam_search(e, None, T, W)
        if float(plain['gaps'][0]) < GAP:
            continue
        for y in hypotheses(R.beam_search(e, None, T, 8), 0):
            if len(y) != 2 or y in hypotheses(plain, 0):
                continue
            ref = beam_search(e, None, T, W, [y], bonus)
            if float(ref['gaps'][0]) >= GAP and hypotheses(ref, 0)[0] == y:
                return dict(seed=seed, T=T, V=V, W=W, scale=scale, phrase=y, bonus=bonus)
    return None
