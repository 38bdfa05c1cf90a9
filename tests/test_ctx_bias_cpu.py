"""CPU checks of contextual biasing: haloop_amd.biasing.ContextGraph against the brute force of tests/ctx_bias_ref.py (no failure links,
no tables), the float64 restatement of the biased search against the unbiased one, the conditions of the fixtures that
tests/test_gpu_ctx_bias.py compares exactly against, and the argument checks of the public interface.  No GPU."""
import random

import pytest
import torch

import ctc_prefix_beam_ref as R
import ctx_bias_ref as C


def graph_of(phrases, V, bonus):
    from haloop_amd.biasing import ContextGraph
    return ContextGraph(phrases, V, bonus)


def random_set(rng, V, count, longest):
    return [tuple(rng.randrange(1, V) for _ in range(rng.randint(1, longest))) for _ in range(count)]


# phrases that are prefixes, suffixes and infixes of one another, a single-token phrase, a repeated token, a duplicate
NESTED = [(1, 2, 3, 4), (1, 2), (2, 3), (3, 4), (3,), (2, 3, 4, 1), (4, 4), (4, 4, 4), (1, 2)]
SETS = [('nested', 5, NESTED, 1.5), ('nested-negative', 5, NESTED, -0.75), ('empty', 5, [], 1.0), ('single', 8, [(7,)], 0.3)] + \
       [(f'random-{V}-{i}', V, random_set(random.Random(100 * V + i), V, count, longest), bonus)
        for V, count, longest in ((5, 7, 4), (8, 10, 5), (300, 40, 4)) for i, bonus in enumerate((1.0, 0.1, -2.5))]


@pytest.mark.parametrize('name,V,phrases,bonus', SETS, ids=[s[0] for s in SETS])
def test_context_graph_equals_the_brute_force(name, V, phrases, bonus):
    g, b = graph_of(phrases, V, bonus), C.Brute(phrases, bonus)
    assert g.num_states == len(b.index) and g.num_columns == len({k for p in phrases for k in p}) and g.width == g.num_columns + 1
    assert g.next.shape == g.gain.shape == (g.num_states, g.width) and g.columns.shape == (V,)
    assert g.next.dtype == torch.int32 and g.columns.dtype == torch.int32 and g.gain.dtype == torch.float32 and g.held.dtype == torch.float32
    path = {i: s for s, i in b.index.items()}
    # every transition of every state, tokens in no phrase (column 0) among them, exactly in float64
    for i, s in path.items():
        assert float(g.held64[i]) == b.held(s) and g.depth[i] == len(s) and g.final[i] == (s in b.phrases)
        for k in range(1, V) if V <= 8 else sorted({k for p in phrases for k in p} | {1, V - 1}):
            nxt, gain = b.step(s, k)
            col = int(g.columns[k])
            assert int(g.next[i, col]) == b.index[nxt] and float(g.gain64[i, col]) == gain, (s, k)
            assert g.step(i, k) == (b.index[nxt], float(g.gain[i, col]))
        assert int(g.next[i, 0]) == 0 and float(g.gain64[i, 0]) == -b.held(s)
    in_phrases = {k for p in phrases for k in p}
    assert all((int(g.columns[k]) != 0) == (k in in_phrases) for k in range(V)) and int(g.columns[0]) == 0
    # the float32 tables are the float64 ones, rounded once
    assert torch.equal(g.gain, g.gain64.float()) and torch.equal(g.held, g.held64.float())
    # random texts: the state and the float64 sum of the gains; boost() adds the rounded gains in float32, left to right
    rng = random.Random(7)
    alphabet = sorted(in_phrases) or [1]
    for _ in range(60):
        text = [rng.choice(alphabet) if rng.random() < 0.8 else rng.randrange(1, V) for _ in range(rng.randint(0, 12))]
        s, z, gains = b.boost(text)
        state, z32, z64 = 0, torch.zeros((), dtype=torch.float32), 0.0
        for k, want in zip(text, gains):
            col = int(g.columns[k])
            assert float(g.gain64[state, col]) == want
            z32 = z32 + g.gain[state, col]
            z64 += float(g.gain64[state, col])
            state = int(g.next[state, col])
        assert state == b.index[s] and z64 == z
        assert g.boost(text) == (state, float(z32))
        if bonus in (1.0, 1.5, -0.75, -2.5):                            # gains that float32 holds exactly: the two sums are one number
            assert float(z32) == z


def test_what_a_boost_means():
    g = graph_of([(1, 2, 3), (1, 2), (4,)], 6, 1.5)
    assert g.boost([1])[1] == 1.5 and g.boost([1, 5])[1] == 0.0          # a broken match gives back what it held
    assert g.boost([1, 2])[1] == 3.0 and g.boost([1, 2, 5])[1] == 3.0    # a completed phrase keeps what it earned
    assert g.boost([1, 2, 3])[1] == 4.5 and g.boost([1, 2, 3, 5])[1] == 4.5      # banked at its end, the longer one went on earning
    assert g.boost([1, 1])[1] == 1.5                                     # down to what the longest suffix that still matches holds
    assert g.boost([4, 4])[1] == 3.0 and g.boost([5, 4, 5])[1] == 1.5
    h = graph_of([(1, 2, 3), (2,)], 6, 1.0)                              # output links are not followed: (2,) inside 1 2 earns nothing
    assert h.boost([1, 2])[1] == 2.0 and h.boost([1, 2, 5])[1] == 0.0 and h.boost([5, 2, 5])[1] == 1.0
    assert [float(x) for x in g.held] == [0.0, 1.5, 0.0, 0.0, 0.0]


def test_context_graph_checks_its_arguments():
    from haloop_amd.biasing import ContextGraph
    for bad in ([()], [(0,)], [(5,)], [(1, -1)], [(1, 2), (3, 7)]):
        with pytest.raises(ValueError):
            ContextGraph(bad, 5)
    for bonus in (float('inf'), float('nan')):
        with pytest.raises(ValueError):
            ContextGraph([(1,)], 5, bonus)
    with pytest.raises(ValueError):
        ContextGraph([(1,)], 1)
    with pytest.raises(ValueError):                                      # above 65535 states
        ContextGraph([(1 + i // 300, 1 + i % 300, 1 + j) for i in range(22000) for j in range(3)], 400)
    with pytest.raises(ValueError):                                      # 3001 states x 3001 columns x 8 bytes: above 64 MiB
        ContextGraph([(k,) for k in range(1, 3001)], 3002)
    g = ContextGraph([(1, 2), (1, 2), [1, 2]], 5)
    assert g.phrases == ((1, 2),) and g.num_states == 3
    empty = ContextGraph([], 5, 2.0)
    assert empty.num_states == 1 and empty.width == 1 and empty.boost([1, 2, 3]) == (0, 0.0) and not bool(empty.columns.any())


@pytest.mark.parametrize('name,W', [c for c in C.CASES if c[0] not in ('huge', 'stream', 'deep')])
def test_zero_gain_restatement_is_the_unbiased_restatement(name, W):
    e, il, cap, plain = R.fixture(name, W)
    for phrases, bonus in (([], C.BONUS), (C.phrases(name, W), 0.0)):
        ref = C.beam_search(e, il, cap, W, phrases, bonus)
        for key in ('tokens', 'lengths', 'scores', 'counts', 'merges', 'gaps'):
            assert torch.equal(ref[key], plain[key]), key
        assert not bool(ref['boosts'].any())


@pytest.mark.parametrize('name,W', C.CASES)
def test_every_compared_row_decides_by_a_gap(name, W):
    ref = C.fixture(name, W)[3]
    print(name, W, 'phrases', C.phrases(name, W), 'gaps', ref['gaps'].tolist())
    left_out = C.LEFT_OUT.get((name, W), ())
    assert [n for n in range(len(ref['gaps'])) if float(ref['gaps'][n]) < C.GAP] == list(left_out)
    assert len(left_out) <= (2 if name == 'rows17' else 0)
    assert set(C.LEFT_OUT) <= set(C.CASES) and set(C.PHRASES) == set(C.CASES) == set(R.CASES)
    assert bool((ref['boosts'] != 0).any())                              # the biasing is felt
    # the restatement's own boosts and states are the graph's
    g = C.graph(name, W)
    for n in range(ref['tokens'].shape[0]):
        for w in range(int(ref['counts'][n])):
            y = ref['tokens'][n, w, :int(ref['lengths'][n, w])].tolist()
            state, z = g.boost(y)
            assert state == int(ref['states'][n, w]) and z == float(ref['boosts'][n, w])       # (multiples of 1.5: exact in fp32)


@pytest.mark.parametrize('W', [4, 8])
def test_rows17_best_hypotheses_change(W):
    plain, ref = R.fixture('rows17', W)[3], C.fixture('rows17', W)[3]
    differ = sum(C.hypotheses(plain, n)[0] != C.hypotheses(ref, n)[0] for n in range(17))
    print('rows17', W, 'rows whose best hypothesis differs', differ)
    assert differ * 2 >= 17


def test_planted_phrase_is_lost_unbiased_and_first_biased():
    f = C.PLANTED
    e, il, cap = C.planted_inputs()
    plain = R.beam_search(e, il, cap, f['W'])
    ref = C.beam_search(e, il, cap, f['W'], [f['phrase']], f['bonus'])
    print('unbiased', C.hypotheses(plain, 0), 'biased', C.hypotheses(ref, 0), 'gaps', float(plain['gaps'][0]), float(ref['gaps'][0]))
    assert f['phrase'] not in C.hypotheses(plain, 0) and C.hypotheses(ref, 0)[0] == f['phrase']
    assert float(plain['gaps'][0]) >= C.GAP and float(ref['gaps'][0]) >= C.GAP
    assert f['phrase'] in C.hypotheses(R.beam_search(e, il, cap, 8), 0)   # (a wider unbiased search still holds it)
    assert C.find_planted(range(f['seed'], f['seed'] + 1)) == f


def test_interface_checks_without_a_device():
    from haloop_amd import _lib, ctc, recognizer
    from haloop_amd.biasing import ContextGraph
    e = torch.zeros(5, 2, 4).log_softmax(-1)
    g4, g5 = ContextGraph([(1, 2)], 4), ContextGraph([(1, 2)], 5)
    with pytest.raises(ValueError):
        ctc.ctc_prefix_beam_search(e, context=g5)                       # compiled for another vocabulary
    with pytest.raises(ValueError):
        ctc.ctc_prefix_beam_search(e, context=[(1, 2)])                 # no ContextGraph
    with pytest.raises(_lib.HaloError):
        ctc.ctc_prefix_beam_search(e, context=g4)                       # CPU emissions: no CPU path
    with pytest.raises(ValueError):
        ctc.PrefixBeamStream(2, 4, context=g5, device='cpu')
    head = recognizer.TemporalClassifier(16, 5).eval()
    assert head._context is None
    with pytest.raises(ValueError):
        head.set_context(g4)
    head.set_context(g5)
    assert head._context is g5 and list(head.state_dict()) == ['classifier.weight', 'classifier.bias']
    with pytest.raises(_lib.HaloError):                                 # CPU features reach the head's device check
        head.decode(torch.zeros(1, 6, 16), torch.tensor([6]), None, beam_size=2)
    import ctc_lm_beam_ref as LM
    head.set_lm(LM.make_lm(5, 1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='not built'):         # an LM and a context at once
        head.decode(torch.zeros(1, 6, 16), torch.tensor([6]), None, beam_size=2)
    head.set_lm(None)
    head.set_context(None)
    assert head._context is None and head.last_parts is None
    handle = _lib.lib()
    plain, biased = handle.halo_ctc_prefix_beam_state_bytes, handle.halo_ctc_prefix_beam_biased_state_bytes
    for shape in ((256, 4, 32), (3, 16, 400), (70000, 2, 10)):
        assert biased(*shape) == plain(*shape) + 128
    assert biased(1, 4, 32) == 0 and biased(256, 17, 32) == 0 and biased(256, 4, 8193) == 0
