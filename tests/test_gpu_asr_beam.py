"""GPU checks of the attention decoder's beam search (haloop_amd/transformer.py BeamDecoder, csrc/decode.hip, csrc/decode_beam.hip;
DESIGN.md 3.3r):

    halo_decode_beam_attention  with W = 1 and the identity table BITWISE halo_decode_attention_pair; with W = 3 and a random ancestor
        table within 2e-6 (that launch's own bound against its predecessors) of the existing launch on physically gathered caches;
        at 1024 and 1025 keys (both key capacities of the kernel the two launches share) both comparisons bitwise, and
        both launches against a float64 restatement in torch;
    halo_decode_beam_select  against a float64 restatement in torch: integers, tokens, ancestor rows and embeddings exact, scores 1e-5;
    BeamDecoder.decode in `bf16x3` against tests/asr_beam_ref.py on the rows that file says are comparable (every decision decided by
        GAP = 4e-3 or more): tokens, lengths, finished flags and counts EXACT, ranks and log-probabilities within 2e-3 (the figure of
        tests/test_gpu_decode.py for this decoder at this depth);
    W = 1 against the greedy decode, graph replay against eager launches, stale buffers, NaN past the input lengths, parameters changed
        in place, the general path, refusals, and the CTC head's rescoring of the lists.
"""
import numpy as np
import pytest
import torch

import asr_beam_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ETX = R.ETX
NINF = float('-inf')


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops, transformer
    _lib.lib()
    _lib.lend_scratch()
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16x3')
    yield dict(ops=ops, tr=transformer, lib=_lib)
    _lib.set_math_mode(prev)


# ---- halo_decode_beam_attention ---------------------------------------------------------------------------------------------------
def _attention_inputs(ops, N, W, heads, hd, S, Tc, n_keys, seed):
    C, R_ = heads * hd, N * W
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(R_, 4 * C, generator=g).to(DEV)
    mem = torch.randn(2, N, heads, S, hd, generator=g).half().to(DEV)
    time = torch.randn(2, R_, heads, Tc, hd, generator=g).half()
    time[:, :, :, n_keys - 1:] = 0
    mlen = torch.randint(1, S + 1, (N,), generator=g, dtype=torch.int32).to(DEV)
    anc = torch.randint(0, R_, (R_, Tc), generator=g, dtype=torch.int32)
    return a, mem, time.to(DEV), mlen, anc, ops.RopeTable(Tc, hd, DEV)


@pytest.mark.parametrize('hd', [16, 64, 128])
@pytest.mark.parametrize('n_keys', [1, 9, 17])
def test_beam_attention_at_width_one_is_the_pair_launch_bitwise(hal, hd, n_keys):
    ops = hal['ops']
    N, heads, S, Tc = 3, 2, 5, 18
    a, mem, time_a, mlen, _, table = _attention_inputs(ops, N, 1, heads, hd, S, Tc, n_keys, hd + n_keys)
    time_b = time_a.clone()
    ident = torch.arange(N, dtype=torch.int32)[:, None].expand(N, Tc).contiguous().to(DEV)
    ya = torch.full((N, 2 * heads * hd), float('nan'), device=DEV)
    yb = ya.clone()
    ops.decode_attention_pair(a, mem[0], mem[1], mlen, time_a[0], time_a[1], n_keys, table, ya)
    ops.decode_beam_attention(a, mem[0], mem[1], mlen, time_b[0], time_b[1], n_keys, ident, table, yb)
    assert torch.equal(ya, yb) and torch.equal(time_a, time_b)


@pytest.mark.parametrize('hd', [16, 64, 128])
@pytest.mark.parametrize('n_keys', [1, 9, 17])
def test_beam_attention_reads_its_history_through_the_ancestor_table(hal, hd, n_keys):
    ops = hal['ops']
    N, W, heads, S, Tc = 3, 3, 2, 5, 18
    R_, t = N * W, n_keys - 1
    a, mem, time, mlen, anc, table = _attention_inputs(ops, N, W, heads, hd, S, Tc, n_keys, 7 * hd + n_keys)
    utt = torch.arange(R_, device=DEV) // W
    # the existing launch on physically gathered caches: slot s holds position j of row anc[s, j], and its utterance's memory
    gathered = time.clone()
    for j in range(t):
        gathered[:, :, :, j] = time[:, anc[:, j].long().to(DEV), :, j]
    mem_g, mlen_g = mem[:, utt].contiguous(), mlen[utt].contiguous()
    want = torch.full((R_, 2 * heads * hd), float('nan'), device=DEV)
    ops.decode_attention_pair(a, mem_g[0], mem_g[1], mlen_g, gathered[0], gathered[1], n_keys, table, want)
    got = torch.full_like(want, float('nan'))
    before = time.clone()
    ops.decode_beam_attention(a, mem[0], mem[1], mlen, time[0], time[1], n_keys, anc.to(DEV), table, got)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=2e-6)
    assert torch.equal(time[:, :, :, t], gathered[:, :, :, t])                      # position t: stored into the slot's own row
    keep = torch.ones(Tc, dtype=torch.bool)
    keep[t] = False
    assert torch.equal(time[:, :, :, keep], before[:, :, :, keep])                  # and nothing else is written


# ---- the MAXK dispatch both attention launches share: more than 1024 keys take the 8192-key instantiation, which no decode above reaches
MAXK_CASES = [(1024, 4, 2),        # (S, Tc, n_keys): the last shape of the 1024 instantiation, its score row full
              (1025, 4, 2),        # the first shape of the 8192 instantiation, taken by the cross side
              (5, 1025, 1025)]     # the 8192 instantiation, taken by the self side
# Largest |launch - float64| of the launches as they were before they shared one body, over the six cases and both launches, measured on
# an MI355X: 4.195e-07 (hd = 128, 1024 memory keys, the launch through the ancestor table; fp32 scores, softmax and sums over up to
# 1025 keys of fp16 caches).  The bound is twice that, rounded up to one significant digit; the margin is for other random draws.
MAXK_BOUND = 9e-7


def _attention_f64(a, mem_k, mem_v, mlen, time_k, time_v, n_keys, table):
    """Both attentions of a step in float64 -> ([rows, 2C], this step's k and v as the cache holds them [rows, heads, hd]).  mem_* [rows,
    heads, S, hd] and time_* [rows, heads, Tc, hd] are each row's own (gathered) caches, positions < n_keys - 1 of the latter are read."""
    rows, heads, S, hd = mem_k.shape
    C, t = heads * hd, n_keys - 1
    a = a.double().cpu()
    q_x, q_s = a[:, :C].view(rows, heads, hd), a[:, C:2 * C].view(rows, heads, hd)
    k_t = a[:, 2 * C:3 * C].half().view(rows, heads, hd)
    v_t = a[:, 3 * C:].half().view(rows, heads, hd)
    scale = 1.0 / hd ** 0.5
    # cross: key-length mask, no rotary
    sc = torch.einsum('rhd,rhsd->rhs', q_x, mem_k.double().cpu()) * scale
    past = torch.arange(S)[None, None, :] >= mlen.cpu().long()[:, None, None]
    cross = torch.einsum('rhs,rhsd->rhd', sc.masked_fill(past, NINF).softmax(-1), mem_v.double().cpu())
    # self: rotary (interleaved pairs) on q at position t and on the keys at theirs
    cos, sin = table.cos.double().cpu(), table.sin.double().cpu()

    def rot(x, pos):                                                         # x [..., hd] at positions pos (broadcast over x[..., 0])
        x0, x1 = x[..., 0::2], x[..., 1::2]
        return torch.stack((x0 * cos[pos] - x1 * sin[pos], x1 * cos[pos] + x0 * sin[pos]), -1).flatten(-2)

    keys = torch.cat([time_k.double().cpu()[:, :, :t], k_t.double()[:, :, None]], 2)               # [rows, heads, n_keys, hd]
    vals = torch.cat([time_v.double().cpu()[:, :, :t], v_t.double()[:, :, None]], 2)
    sc = torch.einsum('rhd,rhjd->rhj', rot(q_s, t), rot(keys, torch.arange(n_keys))) * scale
    own = torch.einsum('rhj,rhjd->rhd', sc.softmax(-1), vals)
    return torch.cat([cross.reshape(rows, C), own.reshape(rows, C)], 1), k_t, v_t


@pytest.fixture(scope='module')
def maxk_runs(hal):
    """Every case once: the pair launch and the W = 1 beam launch on N = 2 rows, the W = 2 beam launch with a random ancestor table on
    one utterance and the pair launch on its gathered caches, and the float64 results of the two constructions."""
    ops, runs = hal['ops'], {}

    def run(hd, case):
        if (hd, case) in runs:
            return runs[hd, case]
        S, Tc, n_keys = case
        heads, t = 1, n_keys - 1
        nan = lambda rows: torch.full((rows, 2 * heads * hd), float('nan'), device=DEV)
        r = {}
        # N = 2, W = 1
        a, mem, time, _, _, table = _attention_inputs(ops, 2, 1, heads, hd, S, Tc, n_keys, 31 * hd + S + n_keys)
        mlen = torch.tensor([S, S - 1], dtype=torch.int32, device=DEV)
        ident = torch.arange(2, dtype=torch.int32)[:, None].expand(2, Tc).contiguous().to(DEV)
        r['f64_pair'] = _attention_f64(a, mem[0], mem[1], mlen, time[0], time[1], n_keys, table)[0]
        r['time_pair'], r['time_one'] = time.clone(), time.clone()
        r['pair'] = ops.decode_attention_pair(a, mem[0], mem[1], mlen, r['time_pair'][0], r['time_pair'][1], n_keys, table, nan(2))
        r['one'] = ops.decode_beam_attention(a, mem[0], mem[1], mlen, r['time_one'][0], r['time_one'][1], n_keys, ident, table, nan(2))
        # N = 1, W = 2 through the table, and the pair launch on the physically gathered caches
        a, mem, time, _, anc, table = _attention_inputs(ops, 1, 2, heads, hd, S, Tc, n_keys, 37 * hd + S + n_keys)
        mlen = torch.tensor([S - 1], dtype=torch.int32, device=DEV)
        gathered = time.gather(1, anc.long().to(DEV)[None, :, None, :, None].expand_as(time))      # slot s: position j of row anc[s, j]
        gathered[:, :, :, t:] = time[:, :, :, t:]
        mem_g, mlen_g = mem[:, [0, 0]].contiguous(), mlen[[0, 0]].contiguous()
        r['f64_beam'] = _attention_f64(a, mem_g[0], mem_g[1], mlen_g, gathered[0], gathered[1], n_keys, table)[0]
        r['time_beam'] = time.clone()
        r['beam'] = ops.decode_beam_attention(a, mem[0], mem[1], mlen, r['time_beam'][0], r['time_beam'][1], n_keys, anc.to(DEV), table, nan(2))
        r['time_gathered'] = gathered
        r['gathered'] = ops.decode_attention_pair(a, mem_g[0], mem_g[1], mlen_g, gathered[0], gathered[1], n_keys, table, nan(2))
        r['t'] = t
        runs[hd, case] = r
        return r
    return run


@pytest.mark.parametrize('hd', [16, 128])
@pytest.mark.parametrize('case', MAXK_CASES)
def test_both_key_capacities_width_one_is_the_pair_launch_bitwise(maxk_runs, hd, case):
    r = maxk_runs(hd, case)
    assert torch.equal(r['pair'], r['one']) and torch.equal(r['time_pair'], r['time_one'])


@pytest.mark.parametrize('hd', [16, 128])
@pytest.mark.parametrize('case', MAXK_CASES)
def test_both_key_capacities_ancestor_table_is_the_gathered_cache_bitwise(maxk_runs, hd, case):
    """The two sides differ in the address of a key's plane only: the same bits."""
    r = maxk_runs(hd, case)
    assert torch.equal(r['beam'], r['gathered'])
    assert torch.equal(r['time_beam'][:, :, :, r['t']], r['time_gathered'][:, :, :, r['t']])


@pytest.mark.parametrize('hd', [16, 128])
@pytest.mark.parametrize('case', MAXK_CASES)
def test_both_key_capacities_against_float64(maxk_runs, hd, case):
    r = maxk_runs(hd, case)
    dev_pair = (r['pair'].double().cpu() - r['f64_pair']).abs().max().item()
    dev_beam = (r['beam'].double().cpu() - r['f64_beam']).abs().max().item()
    print(f'maxk hd={hd} case={case}: |pair - f64| = {dev_pair:.3e}, |beam - f64| = {dev_beam:.3e}')
    assert dev_pair <= MAXK_BOUND and dev_beam <= MAXK_BOUND       # (NaN fails both)


# ---- halo_decode_beam_select ------------------------------------------------------------------------------------------------------
def _select_ref(logits, t, bonus, rec, W):
    """One step of the definition in float64 (the vectorised form of tests/asr_beam_ref.py's step) -> the new records and the smallest
    gap between two candidates of unequal rank around the cut."""
    score, length, fin, tokens, anc = rec
    N, V = score.shape[0], logits.shape[1]
    cap = tokens.shape[2]
    if t == 0:
        score = torch.full_like(score, NINF); score[:, 0] = 0
        length, fin = torch.zeros_like(length), torch.zeros_like(fin)
    score, length, fin = score.double(), length.long(), fin.bool()
    lp = logits.double().log_softmax(-1).view(N, W, V)
    present = score > NINF
    live, done = present & ~fin, present & fin
    cand = torch.where(live[:, :, None], score[:, :, None] + lp, torch.full_like(lp, NINF))
    cand[:, :, ETX] = torch.where(done, score, cand[:, :, ETX])
    newlen = length[:, :, None] + ((torch.arange(V) != ETX)[None, None, :] & live[:, :, None]).long()
    rk = cand + bonus * newlen.double()
    srt, idx = rk.view(N, W * V).sort(dim=1, descending=True, stable=True)
    d = srt[:, :W] - srt[:, 1:W + 1]
    gap = float(d[(d > 0) & (srt[:, 1:W + 1] > NINF)].min()) if bool(((d > 0) & (srt[:, 1:W + 1] > NINF)).any()) else float('inf')
    top, idx = srt[:, :W], idx[:, :W]
    taken = top > NINF
    own = torch.arange(W)[None, :].expand(N, W)
    par, k = torch.where(taken, idx // V, own), idx % V
    pfin, plen = done.gather(1, par), length.gather(1, par)
    grow = taken & ~pfin & (k != ETX)
    ntok = tokens.long().gather(1, par[:, :, None].expand(N, W, cap))
    at = plen.clamp(max=cap - 1)[:, :, None]
    ntok.scatter_(2, at, torch.where(grow[:, :, None], k[:, :, None], ntok.gather(2, at)))
    nscore = torch.where(taken, cand.view(N, W * V).gather(1, idx), torch.full_like(top, NINF))
    nlen = torch.where(taken, plen + grow.long(), torch.zeros_like(plen))
    nfin = taken & (pfin | (k == ETX))
    rows = torch.arange(N)[:, None] * W
    nanc = anc.long().view(N, W, -1).gather(1, par[:, :, None].expand(N, W, anc.shape[1])).clone()
    nanc = torch.where(taken[:, :, None], nanc, (rows + own)[:, :, None].expand_as(nanc))
    nanc[:, :, t] = rows + par
    tok_next = torch.where(taken, k, torch.full_like(k, ETX))
    return dict(score=nscore, rank=torch.where(taken, top, torch.full_like(top, NINF)), length=nlen, fin=nfin, tokens=ntok,
                anc=nanc.view(N * W, -1), next=tok_next, gap=gap)


@pytest.mark.parametrize('V,W', [(32, 1), (32, 4), (300, 16), (4100, 3)])
@pytest.mark.parametrize('t,bonus', [(0, 0.0), (3, 0.0), (4, 0.75)])
def test_beam_select_against_the_float64_step(hal, V, W, t, bonus):
    ops = hal['ops']
    N, cap, ld, C = 5, 6, 7, 64
    g = torch.Generator().manual_seed(V + 31 * W + t)
    logits = torch.randn(N * W, V, generator=g) * 3
    score = -torch.rand(N, W, generator=g) * 6
    length = torch.randint(0, t + 1, (N, W), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 4, (N, W), generator=g)                                  # 0: empty, 1: finished, else live
    kind[:, 0] = 2
    score = torch.where(kind == 0, torch.full_like(score, NINF), score)
    fin = (kind == 1).int()
    tokens = torch.randint(4, V, (N, W, ld), generator=g, dtype=torch.int32)
    anc = torch.randint(0, N * W, (N * W, ld), generator=g, dtype=torch.int32)
    if W >= 2:        # two live slots with equal logits, scores and lengths: every pair of their candidates ties and position decides
        logits[1] = logits[0]
        score[0, 1], length[0, 1], fin[0, 1] = score[0, 0], length[0, 0], 0
        fin[0, 0] = 0
    if W >= 4:        # and a finished slot whose rank equals a live one's ETX candidate cannot be planted exactly; two equal finished ones can
        score[1, 2], length[1, 2], fin[1, 2] = -0.5, min(t, 2), 1
        score[1, 3], length[1, 3], fin[1, 3] = -0.5, min(t, 2), 1
    rec = (score, length, fin, tokens, anc)
    want = _select_ref(logits, t, bonus, rec, W)
    assert want['gap'] > 1e-4                  # the float32 launch and the float64 step order every pair of unequal candidates alike
    wte = torch.randn(V, C, generator=g).to(DEV)
    rec_in = tuple(x.to(DEV).contiguous() for x in rec)
    rec_out = (torch.full((N, W), 7.0, device=DEV), *(torch.full(x.shape, -7, dtype=torch.int32, device=DEV) for x in rec[1:]))
    ranks = torch.full((N, W), 7.0, device=DEV)
    y = torch.full((N * W, C), float('nan'), device=DEV)
    ops.decode_beam_select(logits.to(DEV), t, cap, ETX, bonus, rec_in, rec_out, ranks, wte, y)
    s, n, f, tok, a = (x.cpu() for x in rec_out)
    for x, ref in zip(rec_in, rec):
        assert torch.equal(x.cpu(), ref)                                             # the copy read is not written
    assert torch.equal(n.long(), want['length']) and torch.equal(f.bool(), want['fin'])
    assert torch.equal(torch.isinf(s), torch.isinf(want['score']))
    ok = ~torch.isinf(want['score'])
    np.testing.assert_allclose(s[ok].numpy(), want['score'][ok].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(ranks.cpu()[ok].numpy(), want['rank'][ok].numpy(), rtol=0, atol=1e-5)
    assert bool((ranks.cpu()[~ok] == NINF).all())
    for i in range(N):
        for w in range(W):
            m = int(want['length'][i, w])
            assert tok[i, w, :m].tolist() == want['tokens'][i, w, :m].tolist(), (i, w)
    assert torch.equal(a[:, :t + 1].long(), want['anc'][:, :t + 1])
    assert bool((a[:, t + 1:] == -7).all())                                          # nothing written past position t
    assert torch.equal(y.cpu(), wte.cpu()[want['next'].view(-1)])
    # without the embedding (the last step): the same records
    rec_b = (torch.zeros(N, W, device=DEV), *(torch.zeros(x.shape, dtype=torch.int32, device=DEV) for x in rec[1:]))
    ranks_b = torch.zeros(N, W, device=DEV)
    ops.decode_beam_select(logits.to(DEV), t, cap, ETX, bonus, rec_in, rec_b, ranks_b)
    assert torch.equal(rec_b[0], rec_out[0]) and torch.equal(ranks_b, ranks) and torch.equal(rec_b[1], rec_out[1])


def test_beam_select_refusals(hal):
    ops, lib = hal['ops'], hal['lib']
    N, W, V, ld = 2, 2, 32, 4
    rec = lambda: (torch.zeros(N, W, device=DEV), torch.zeros(N, W, dtype=torch.int32, device=DEV), torch.zeros(N, W, dtype=torch.int32, device=DEV),
                   torch.zeros(N, W, ld, dtype=torch.int32, device=DEV), torch.zeros(N * W, ld, dtype=torch.int32, device=DEV))
    a, b = rec(), rec()
    logits, ranks = torch.zeros(N * W, V, device=DEV), torch.zeros(N, W, device=DEV)
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select(logits, 0, ld, ETX, 0.0, a, a, ranks)                 # one copy for both
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select(logits, ld, ld, ETX, 0.0, a, b, ranks)                # a step past the capacity
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select(logits, 0, ld + 1, ETX, 0.0, a, b, ranks)             # token rows shorter than the capacity


# ---- end to end -------------------------------------------------------------------------------------------------------------------
_DECODERS = {}


def _decoder(tr, name):
    """The case's Decoder on the device, built once (its weight images and graphs are reused by the tests that do not change it)."""
    if name not in _DECODERS:
        V, hd, heads, L = R.CASES[name][:4]
        pd = R.case_inputs(name)[0]
        dec = tr.Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
        dec.load_state_dict({k[len('decoder.'):]: v for k, v in pd.items() if k.startswith('decoder.')}, strict=True)
        _DECODERS[name] = dec.to(DEV).eval()
    return _DECODERS[name]


def _run(tr, name, dec=None, feats=None, rows=None):
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = R.CASES[name]
    _, f, flen, _ = R.case_inputs(name)
    f = f if feats is None else feats
    rows = slice(None) if rows is None else rows
    dec = dec or _decoder(tr, name)
    bd = tr.BeamDecoder(dec, N, T, W, bonus)
    out = bd.decode(f[rows].to(DEV), flen[rows].to(DEV))
    return tuple(x.cpu() for x in out) + (bd.last_logprobs.cpu(), bd.last_finished.cpu())


def _assert_lists_match_the_oracle(name, got, rows=None):
    want = R.case_result(name)
    rows = R.compared_rows(name) if rows is None else rows
    assert rows
    tokens, lengths, ranks, counts, logprobs, finished = got
    assert torch.equal(tokens[rows], want['tokens'][rows]) and torch.equal(lengths[rows], want['lengths'][rows])
    assert torch.equal(finished[rows], want['finished'][rows]) and torch.equal(counts[rows], want['counts'][rows])
    for a, b in ((ranks, want['ranks']), (logprobs, want['logprobs'])):
        assert torch.equal(torch.isinf(a[rows]), torch.isinf(b[rows]))
        ok = ~torch.isinf(b[rows])
        np.testing.assert_allclose(a[rows][ok].double().numpy(), b[rows][ok].numpy(), rtol=0, atol=2e-3)


@pytest.mark.parametrize('name', list(R.CASES))
def test_fused_beam_search_matches_the_float64_search(hal, name):
    dec = _decoder(hal['tr'], name)
    assert dec._fused_decode_ok(R.CASES[name][1] * R.CASES[name][2])
    _assert_lists_match_the_oracle(name, _run(hal['tr'], name))


def test_width_one_is_the_greedy_decode(hal):
    tr = hal['tr']
    name = 'w4'
    heads, T = R.CASES[name][2], R.CASES[name][11]
    _, feats, flen, tl = R.case_inputs(name)
    dec = _decoder(tr, name)
    N = feats.shape[0]
    outs, out_len, _, lps, _ = dec.decode(feats.to(DEV), flen.to(DEV), tl.to(DEV))
    bd = tr.BeamDecoder(dec, N, T, 1, 0.0)
    tokens, lengths, ranks, counts = bd.decode(feats.to(DEV), flen.to(DEV))
    assert counts.tolist() == [1] * N
    greedy = [o.tolist() for o in outs.unbind()]
    closed = bd.last_finished[:, 0].cpu()
    assert bool(closed.any())
    for n in range(N):
        m = int(lengths[n, 0])
        assert int(out_len[n]) == m + int(closed[n])                                  # greedy counts the steps a row was alive
        assert tokens[n, 0, :int(out_len[n]) - 1].tolist() == greedy[n]               # (sic) an open row's last token is not in greedy's output
    np.testing.assert_allclose(bd.last_logprobs[:, 0].cpu().numpy(), lps.cpu().numpy(), rtol=0, atol=1e-5)
    assert torch.equal(ranks, bd.last_logprobs)
    # Decoder.decode(beam_size=1): greedy's five values
    b_outs, b_len, b_al, b_lps, b_ent = dec.decode(feats.to(DEV), flen.to(DEV), tl.to(DEV), beam_size=1)
    assert [o.tolist() for o in b_outs.unbind()] == greedy and torch.equal(b_len.cpu(), out_len.cpu()) and b_al == [None] * N
    np.testing.assert_allclose(b_lps.cpu().numpy(), lps.cpu().numpy(), rtol=0, atol=1e-5)
    assert bool(b_ent.isnan().all()) and b_ent.shape == (N,)
    assert torch.equal(dec.last_nbest[0], tokens)


def test_decoder_decode_returns_the_best_hypothesis_and_keeps_the_lists(hal, monkeypatch):
    tr = hal['tr']
    name = 'w4'
    _, feats, flen, tl = R.case_inputs(name)
    want = R.case_result(name)
    monkeypatch.setenv('HALO_ASR_BEAM', '4')
    V, hd, heads, L = R.CASES[name][:4]
    dec = tr.Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)         # the width comes from the environment
    dec.load_state_dict(_decoder(tr, name).state_dict())
    dec = dec.to(DEV).eval()
    outs, out_len, _, lps, _ = dec.decode(feats.to(DEV), flen.to(DEV), tl.to(DEV))
    rows = R.compared_rows(name)
    assert torch.equal(dec.last_nbest[0].cpu()[rows], want['tokens'][rows])
    outs = [o.tolist() for o in outs.unbind()]
    for n in rows:
        m, closed = int(want['lengths'][n, 0]), int(want['finished'][n, 0])
        assert int(out_len[n]) == m + closed and outs[n] == want['tokens'][n, 0, :m + closed - 1].tolist()
    np.testing.assert_allclose(lps.cpu()[rows].double().numpy(), want['logprobs'][rows, 0].numpy(), rtol=0, atol=2e-3)
    # beam_size=0 is the greedy decode whatever the attribute says
    g = dec.decode(feats.to(DEV), flen.to(DEV), tl.to(DEV), beam_size=0)
    assert not bool(g[4].isnan().any())


def test_graph_replay_equals_eager_launches_bitwise(hal, monkeypatch):
    monkeypatch.setenv('HALO_DECODE_GRAPH', '1')
    a = _run(hal['tr'], 'w4-bonus')
    monkeypatch.setenv('HALO_DECODE_GRAPH', '0')
    b = _run(hal['tr'], 'w4-bonus')
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_decodes_of_other_batch_sizes_leave_nothing_behind(hal):
    tr = hal['tr']
    name = 'w4-bonus'
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = R.CASES[name]
    _, feats, flen, _ = R.case_inputs(name)
    bd = tr.BeamDecoder(_decoder(tr, name), N, T, W, bonus)
    runs = []
    for rows in (slice(None), slice(0, 3), slice(None)):
        out = bd.decode(feats[rows].to(DEV), flen[rows].to(DEV))
        runs.append(tuple(x.cpu() for x in out) + (bd.last_logprobs.cpu(),))
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[2]))
    few = [n for n in R.compared_rows(name) if n < 3]
    assert few and torch.equal(runs[1][0][few], runs[0][0][few]) and torch.equal(runs[1][1][few], runs[0][1][few])


def test_memory_rows_past_the_input_lengths_are_never_read(hal):
    name = 'w4-bonus'
    _, feats, flen, _ = R.case_inputs(name)
    poisoned = feats.clone()
    for n in range(feats.shape[0]):
        poisoned[n, int(flen[n]):] = float('nan')
    assert bool(poisoned.isnan().any())
    a, b = _run(hal['tr'], name), _run(hal['tr'], name, feats=poisoned)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_parameter_changed_in_place_rebuilds_the_images(hal):
    tr = hal['tr']
    name = 'w4'
    V, hd, heads, L = R.CASES[name][:4]
    dec = tr.Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
    dec.load_state_dict(_decoder(tr, name).state_dict())
    dec = dec.to(DEV).eval()
    first = _run(tr, name, dec=dec)
    with torch.no_grad():
        dec.lm_head.weight[5] += 0.5 * dec.lm_head.weight[ETX]
        dec.h[0].mix_chan[2].weight.mul_(0.5)
    second = _run(tr, name, dec=dec)
    fresh = tr.Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
    fresh.load_state_dict(dec.state_dict())
    third = _run(tr, name, dec=fresh.to(DEV).eval())
    assert not torch.equal(first[2], second[2])
    assert all(torch.equal(x, y) for x, y in zip(second, third))


@pytest.mark.parametrize('name', ['w4', 'w4-bonus', 'l3-w3'])
@pytest.mark.parametrize('how', ['f32', 'unfused'])
def test_general_path_returns_the_same_lists(hal, monkeypatch, name, how):
    tr, lib = hal['tr'], hal['lib']
    dec = _decoder(tr, name)
    fused = _run(tr, name)
    if how == 'f32':
        lib.set_math_mode('f32')
    else:
        monkeypatch.setenv('HALO_DECODE_FUSED', '0')
    try:
        assert not dec._fused_decode_ok(R.CASES[name][1] * R.CASES[name][2])
        general = _run(tr, name)
    finally:
        lib.set_math_mode('bf16x3')
    _assert_lists_match_the_oracle(name, general)
    rows = R.compared_rows(name)
    assert torch.equal(general[0][rows], fused[0][rows]) and torch.equal(general[1][rows], fused[1][rows])


def test_prompts_and_training_mode_raise(hal):
    tr = hal['tr']
    name = 'w4'
    V, hd, heads, L = R.CASES[name][:4]
    _, feats, flen, tl = R.case_inputs(name)
    dec = _decoder(tr, name)
    with pytest.raises(NotImplementedError):
        dec.decode(feats.to(DEV), flen.to(DEV), tl.to(DEV), prompt=torch.tensor([[7, 9]] * feats.shape[0]), beam_size=2)
    hot = tr.Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L).to(DEV).train()
    with pytest.raises(NotImplementedError):
        tr.BeamDecoder(hot, feats.shape[0], 9, 2).decode(feats.to(DEV), flen.to(DEV))
    with pytest.raises(NotImplementedError):
        hot.decode(feats.to(DEV), flen.to(DEV), tl.to(DEV), beam_size=2)


# ---- the CTC head rescoring the lists -----------------------------------------------------------------------------------------------
def test_ctc_head_rescoring_is_the_reranking_in_torch(hal):
    from haloop_amd import functional as HF
    tr = hal['tr']
    name = 'w4-bonus'
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = R.CASES[name]
    pd, feats, flen, tl = R.case_inputs(name)
    model = tr.CTCAttentionDecoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
    model.load_state_dict(pd, strict=True)
    model = model.to(DEV).eval()
    model.decoder.length_bonus = bonus
    f, il = feats.to(DEV), flen.to(DEV)
    plain = model.decode(f, il, tl.to(DEV), beam_size=W)                              # ctc_weight = 0: the order is left alone
    tokens, lengths, ranks, counts = (x.clone() for x in model.decoder.last_nbest)
    assert all(torch.equal(x, y) for x, y in zip(model.last_nbest, (tokens, lengths, ranks, counts)))
    _assert_lists_match_the_oracle(name, tuple(x.cpu() for x in (tokens, lengths, ranks, counts)) +
                                   (model.decoder._beams['decoder'].last_logprobs.cpu(), model.decoder._beams['decoder'].last_finished.cpu()))
    c = 0.3
    out = model.decode(f, il, tl.to(DEV), beam_size=W, ctc_weight=c)
    with torch.no_grad():
        lp = model.recognizer.log_probs(f)
        rows = lp[:, None].expand(N, W, S, V).reshape(N * W, S, V)
        loss = HF.ctc_loss(rows.permute(1, 0, 2), tokens.clamp(min=0).view(N * W, -1), il[:, None].expand(N, W).reshape(-1),
                           lengths.clamp(min=0).view(-1), reduction='none').view(N, W)
    joint = (1 - c) * ranks + c * (-loss)
    assert bool(torch.isfinite(joint).any()) and bool(torch.isinf(loss).any())          # short utterances cannot spell nine tokens
    order = (-joint).argsort(dim=1, stable=True)                                      # -inf (unspellable) last, ties in the old order
    r_tokens, r_lengths, r_scores, r_counts = model.last_nbest
    assert torch.equal(r_tokens, tokens.gather(1, order[:, :, None].expand_as(tokens)))
    assert torch.equal(r_lengths, lengths.gather(1, order)) and torch.equal(r_counts, counts)
    assert torch.equal(r_scores, joint.gather(1, order))
    assert torch.equal(model.last_parts[0], ranks.gather(1, order)) and torch.equal(model.last_parts[1], (-loss).gather(1, order))
    assert bool((order != torch.arange(W, device=DEV)[None, :]).any())                # the CTC head does change some row's order
    best = [o.tolist() for o in out[0].unbind()]
    for n in range(N):
        m = int(r_lengths[n, 0])
        assert best[n] == r_tokens[n, 0, :max(int(out[1][n]) - 1, 0)].tolist() and int(out[1][n]) - m in (0, 1)
    assert len(plain) == 5
