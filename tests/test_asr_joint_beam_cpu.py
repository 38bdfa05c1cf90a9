"""The float64 restatement of the joint CTC/attention beam search (tests/asr_joint_beam_ref.py) against an enumeration of all CTC paths,
a brute-force maximisation of the joint objective, the attention-only restatement and torch's ctc_loss; the conditions on the GPU cases;
the argument checks of the public interface.  No GPU."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import asr_beam_ref as A
import asr_joint_beam_ref as J
from oracle import transformer_ref as tref

ETX, NINF = J.ETX, J.NINF


def _collapse(path):
    out, prev = [], 0
    for k in path:
        if k != 0 and k != prev:
            out.append(k)
        prev = k
    return tuple(out)


def _enumerate(x, frames):
    """{collapsed sequence: [mass of the paths over frames 0 .. frames - 1 ending in a non-blank, ... in a blank]} in probability."""
    V = x.shape[1]
    prob = x.exp()
    table = {}
    for path in itertools.product(range(V), repeat=frames):
        m = 1.0
        for t, k in enumerate(path):
            m *= float(prob[t, k])
        table.setdefault(_collapse(path), [0.0, 0.0])[path[-1] == 0] += m
    return table


def test_prefix_scores_and_states_against_all_ctc_paths():
    """T = 5, V = 5: psi(g, k) is the mass of the V^T paths whose spelling starts with g.k, psi(g, ETX) the mass of those that spell
    exactly g, r[t] the two masses over frames 0 .. t; every prefix over the labels {1, 2, 4} to depth 4, repeated tokens included."""
    T, V = 5, 5
    x = torch.randn(T, V, generator=torch.Generator().manual_seed(1), dtype=torch.float64).log_softmax(-1)
    tables = [_enumerate(x, t + 1) for t in range(T)]
    full = {g: sum(m) for g, m in tables[T - 1].items()}
    labels = [k for k in range(1, V) if k != ETX]
    xb, Tb = x[None], torch.tensor([T])
    worst = 0.0

    def walk(g, r, depth):
        nonlocal worst
        last = torch.tensor([g[-1] if g else -1])
        for t in range(T):
            want = tables[t].get(g, [0.0, 0.0])
            worst = max(worst, abs(math.exp(float(r[0, t, 0])) - want[0]), abs(math.exp(float(r[0, t, 1])) - want[1]))
        psi = J.prefix_scores(xb, Tb, r, last)[0]
        assert float(psi[0]) == NINF
        worst = max(worst, abs(math.exp(float(psi[ETX])) - full.get(g, 0.0)))
        for k in labels:
            h = g + (k,)
            want = sum(m for s, m in full.items() if s[:len(h)] == h)
            worst = max(worst, abs(math.exp(float(psi[k])) - want))
            if depth < 4:
                walk(h, J.prefix_advance(xb, Tb, r, last, torch.tensor([k])), depth + 1)

    walk((), J.prefix_init(xb, Tb), 0)
    assert worst < 1e-12, worst


def test_prefix_functions_never_read_frames_past_the_length():
    S, V = 6, 5
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, S, V, generator=g, dtype=torch.float64).log_softmax(-1)
    T = torch.tensor([1, 4, 6])
    bad = x.clone()
    for n in range(3):
        bad[n, int(T[n]):] = float('nan')
    for src in (x, bad):
        r = J.prefix_init(src, T)
        q = J.prefix_advance(src, T, r, torch.tensor([-1, -1, -1]), torch.tensor([1, 2, 4]))
        psi = J.prefix_scores(src, T, q, torch.tensor([1, 2, 4]))
        assert not bool(r.isnan().any()) and not bool(q.isnan().any()) and not bool(psi.isnan().any())
        if src is x:
            want = (r, q, psi)
    assert torch.equal(want[0], r) and torch.equal(want[1], q) and torch.equal(want[2], psi)
    assert float(psi[0, 1]) == NINF and float(psi[0, ETX]) > NINF                  # one frame: the prefix (1) cannot repeat its token


def _small(V=4, hd=16, heads=2, L=1, S=5, N=3, seed=3, sharp=1.0):
    pd = tref.make_decoder_params(V, hd, heads, L, seed, sharp=sharp)
    g = torch.Generator().manual_seed(seed + 100)
    feats = torch.randn(N, S, hd * heads, generator=g)
    flen = torch.randint(2, S + 1, (N,), generator=g)
    lp = torch.randn(N, S, V, generator=g, dtype=torch.float64).log_softmax(-1)
    return pd, feats, flen, lp


def _teacher_forced(pd, feats, flen, heads, n, toks, closed):
    """log P(toks (+ ETX when closed) | utterance n) from one teacher-forced pass in float64, caches unrounded."""
    p64 = {k: v.double() for k, v in pd.items()}
    prompt = torch.tensor([[J.STX] + list(toks)])
    lp = tref.decoder_logits(p64, feats[n:n + 1].double(), prompt, flen[n:n + 1], heads, pre='decoder.').log_softmax(-1)[0]
    out = list(toks) + ([ETX] if closed else [])
    return float(sum(lp[i, k] for i, k in enumerate(out)))


@pytest.mark.parametrize('bonus,c', [(0.0, 0.3), (0.7, 0.5)])
def test_exhaustive_joint_beam_equals_brute_force(bonus, c):
    """V = 4, capacity 2, W = 16: the beam holds every hypothesis the lattice can spell ((), (a) closed, (a, b) open over the labels
    {1, 2}: 7 at most), so the lists are their enumeration sorted by the joint objective, the CTC part from all V^T paths."""
    pd, feats, flen, lp = _small()
    heads, V, cap = 2, 4, 2
    res = J.joint_beam_search(pd, feats, flen, lp, heads, 16, cap, bonus, c, cache_dtype=torch.float64)
    labels = [1, 2]
    hyps = [((), True)] + [((a,), True) for a in labels] + [((a, b), False) for a in labels for b in labels]
    for n in range(feats.shape[0]):
        full = {g: sum(m) for g, m in _enumerate(lp[n, :int(flen[n])], int(flen[n])).items()}
        want = []
        for toks, closed in hyps:
            mass = full.get(toks, 0.0) if closed else sum(m for s, m in full.items() if s[:len(toks)] == toks)
            if mass > 0:
                att = _teacher_forced(pd, feats, flen, heads, n, toks, closed) + bonus * len(toks)
                want.append(((1 - c) * att + c * math.log(mass), toks, closed, att, math.log(mass)))
        want.sort(key=lambda v: -v[0])
        assert int(res['counts'][n]) == len(want)
        for w, (rank, toks, closed, att, ctc) in enumerate(want):
            assert res['tokens'][n, w, :len(toks)].tolist() == list(toks) and int(res['lengths'][n, w]) == len(toks)
            assert bool(res['finished'][n, w]) == closed
            assert abs(float(res['ranks'][n, w]) - rank) < 1e-9 and abs(float(res['ctc'][n, w]) - ctc) < 1e-9
            assert abs(float(res['attention'][n, w]) - att) < 1e-9


@pytest.mark.parametrize('W,bonus', [(3, 0.0), (4, 1.0)])
def test_weight_zero_restates_the_attention_only_search(W, bonus):
    pd, feats, flen, lp = _small(V=12, N=4, seed=5, sharp=2.0)
    a = A.beam_search(pd, feats, flen, 2, W, 5, bonus)
    b = J.joint_beam_search(pd, feats, flen, lp, 2, W, 5, bonus, 0.0)
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('name,c', J.JOINT_CASES)
def test_gpu_cases_leave_out_no_more_rows_than_their_cap(name, c):
    N = J.CASES[name][5]
    left_out = N - len(J.compared_rows(name, c))
    print(name, c, 'rows left out:', left_out)
    assert left_out <= A.excluded_cap(name), (name, c, left_out, J.case_result(name, c)['margin'].tolist())


@pytest.mark.parametrize('name,c', J.JOINT_CASES)
def test_finished_psi_is_minus_ctc_loss_and_no_hypothesis_outruns_its_frames(name, c):
    res = J.case_result(name, c)
    _, _, flen, _ = A.case_inputs(name)
    x = J.ctc_log_probs(name)
    N, W, cap = res['tokens'].shape
    assert bool((res['lengths'] <= flen[:, None]).all())
    rows = x[:, None].expand(N, W, *x.shape[1:]).reshape(N * W, *x.shape[1:])
    loss = F.ctc_loss(rows.permute(1, 0, 2), res['tokens'].clamp(min=0).view(N * W, cap), flen[:, None].expand(N, W).reshape(-1),
                      res['lengths'].clamp(min=0).view(-1), reduction='none').view(N, W)
    fin = res['finished']
    assert int(fin.sum()) > 0
    assert float((res['ctc'][fin] + loss[fin]).abs().max()) < 1e-9
    joint = (1 - c) * res['attention'] + c * res['ctc']
    assert float((joint[fin] - res['ranks'][fin]).abs().max()) < 1e-9


def test_gpu_cases_cover_finished_open_and_ctc_pruned_hypotheses():
    fins = torch.cat([J.case_result(name, c)['finished'].view(-1) for name, c in J.JOINT_CASES])
    present = torch.cat([(J.case_result(name, c)['lengths'] >= 0).view(-1) for name, c in J.JOINT_CASES])
    assert bool(fins.any()) and bool((present & ~fins).any())
    for name, c in J.JOINT_CASES:
        joint, plain = J.case_result(name, c), A.case_result(name)
        differs = ((joint['tokens'][:, 0] != plain['tokens'][:, 0]).any(1) | (joint['finished'][:, 0] != plain['finished'][:, 0]))
        rows = [n for n in J.compared_rows(name, c) if bool(differs[n])]
        print(name, c, 'best hypothesis differs from the attention-only search in', int(differs.sum()), 'rows')
        assert rows                                     # the CTC head prunes: the attention-only search cannot pass the joint test


def test_public_interface_argument_checks():
    from haloop_amd import ops, transformer
    model = transformer.CTCAttentionDecoder(vocab=8, head_dim=16, heads=2, p_drop=0.0, layers=1).eval()
    assert model.joint is False
    feats, il, tl = torch.zeros(2, 5, 32), torch.tensor([5, 4]), torch.tensor([3, 3])
    with pytest.raises(ValueError):
        model.decode(feats, il, tl, joint=True)                                       # no beam
    with pytest.raises(ValueError):
        model.decode(feats, il, tl, beam_size=2, joint=True)                          # no weight
    with pytest.raises(ValueError):
        model.decode(feats, il, tl, beam_size=2, ctc_weight=-0.5, joint=True)
    N, W, S, V = 2, 2, 5, 8
    x, lens = torch.zeros(N, S, V), torch.tensor([5, 4], dtype=torch.int32)
    st, psi = torch.zeros(N * W, S, 2), torch.zeros(N * W, V)
    rec = lambda dt=torch.int32: torch.zeros(N, W, dtype=dt)
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x.double(), lens, st, 0, ETX, psi)
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens.long(), st, 0, ETX, psi)
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens, st[:, :4], 0, ETX, psi)
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens, st, 0, ETX, psi[:, :7])
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens, st, 1, ETX, psi)                               # records missing after step 0
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens, st, 1, ETX, psi, rec(), rec(), rec(), rec())   # scores are float32
    with pytest.raises(ValueError):
        ops.ctc_prefix_advance(x, lens, ETX, st, None, rec())                         # parents without the rest
    with pytest.raises(ValueError):
        ops.ctc_prefix_advance(x, lens, ETX, st, st.clone(), rec(torch.int64), rec(), rec(), rec())
    with pytest.raises(ValueError):
        ops.ctc_prefix_advance(x, lens, ETX, torch.zeros(N * W, S + 1, 2))


def test_joint_switch_is_read_from_the_environment(monkeypatch):
    from haloop_amd import transformer
    monkeypatch.setenv('HALO_ASR_JOINT', '1')
    assert transformer.CTCAttentionDecoder(vocab=8, head_dim=16, heads=2, p_drop=0.0, layers=1).joint is True
    monkeypatch.setenv('HALO_ASR_JOINT', '0')
    assert transformer.CTCAttentionDecoder(vocab=8, head_dim=16, heads=2, p_drop=0.0, layers=1).joint is False
