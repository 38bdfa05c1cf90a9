"""GPU checks of the joint CTC/attention beam search (haloop_amd/transformer.py BeamDecoder with ctc_log_probs, csrc/ctc_prefix_score.hip,
csrc/decode_beam.hip):

    halo_ctc_prefix_scores / halo_ctc_prefix_advance  against tests/asr_joint_beam_ref.py's float64 functions on the same float32 inputs:
        rtol 1e-5 / atol 1e-4, the project's tolerance for fp32 lattice scores (tests/test_gpu_ctc_prefix_beam.py);
    halo_decode_beam_select_joint  against a float64 step: integers, tokens, ancestor rows, parents, last tokens and embeddings exact,
        scores 1e-5; with ctc_weight = 0 BITWISE halo_decode_beam_select;
    BeamDecoder.decode(ctc_log_probs, ctc_weight) in `bf16x3` against the float64 search on the rows whose every decision was decided by
        GAP = 4e-3 or more: tokens, lengths, finished flags and counts EXACT, ranks, log-probabilities and psi within 2e-3;
    graph replay, the general path, the attention-only bits, NaN past the lengths, stale buffers, ctc_loss, and CTCAttentionDecoder.decode.
"""
import numpy as np
import pytest
import torch

import asr_beam_ref as A
import asr_joint_beam_ref as J

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ETX, NINF = J.ETX, J.NINF
LATTICE = dict(rtol=1e-5, atol=1e-4)


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops, recognizer, transformer
    _lib.lib()
    _lib.lend_scratch()
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16x3')
    yield dict(ops=ops, tr=transformer, lib=_lib, rec=recognizer)
    _lib.set_math_mode(prev)


def _close(got, want, **tol):
    """got float32 against want float64: the same entries infinite, the finite ones within the tolerance."""
    got, want = got.detach().cpu().double(), want.double()
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    ok = ~torch.isinf(want)
    np.testing.assert_allclose(got[ok].numpy(), want[ok].numpy(), **tol)


# ---- the prefix scorer's two launches ---------------------------------------------------------------------------------------------------
SHAPES = [(32, 4, 10, 5), (300, 16, 37, 3), (4100, 3, 5, 2), (32, 2, 1000, 2)]       # (V, W, S, N)
_LATTICES = {}


def _lattice(V, W, S, N):
    """Ragged utterances (T_n = 1 and T_n = S among them) and, per slot, a random prefix advanced in float64 from the empty one: slot 0 of
    every utterance the empty prefix, the others up to min(T_n, 12 (3 at S > 64)) tokens -- as long as T_n where that is shorter --, some
    with a repeated last token; every third slot finished, every fifth empty.  Built once per shape (do not modify)."""
    key = (V, W, S, N)
    if key in _LATTICES:
        return _LATTICES[key]
    g = torch.Generator().manual_seed(V + 7 * W + S)
    x = (torch.randn(N, S, V, generator=g, dtype=torch.float64) * 2).log_softmax(-1).float()
    T = torch.randint(1, S + 1, (N,), generator=g)
    T[0], T[1] = 1, S
    R = N * W
    utt = torch.arange(N).repeat_interleave(W)
    xr, Tr = x[utt].double(), T[utt]
    labels = torch.tensor([k for k in range(1, V) if k != ETX])
    longest = 12 if S <= 64 else 3
    length = torch.minimum(torch.randint(1, longest + 1, (R,), generator=g), Tr)
    length[torch.arange(R) % 3 == 2] = torch.minimum(Tr, torch.tensor(longest))[torch.arange(R) % 3 == 2]        # as long as T_n
    length[::W] = 0
    state = J.prefix_init(xr, Tr)
    last = torch.full((R,), -1, dtype=torch.long)
    for i in range(int(length.max())):
        k = labels[torch.randint(0, len(labels), (R,), generator=g)]
        k = torch.where((torch.arange(R) % 4 == 1) & (last >= 0), last, k)             # a repeated token: needs a blank between
        grow = length > i
        state = torch.where(grow[:, None, None], J.prefix_advance(xr, Tr, state, last, k), state)
        last = torch.where(grow, k, last)
    state32 = state.float()                      # what the launches read; the float64 side starts from the same rounded values
    kind = torch.ones(R, dtype=torch.long)       # 1 live, 2 finished, 0 empty
    kind[torch.arange(R) % 3 == 1] = 2
    kind[torch.arange(R) % 5 == 4] = 0
    kind[::W] = 1
    out = dict(x=x, T=T, xr=xr, Tr=Tr, state=state32, last=last, length=length, kind=kind, labels=labels)
    _LATTICES[key] = out
    return out


@pytest.mark.parametrize('V,W,S,N', SHAPES)
def test_prefix_scores_against_float64(hal, V, W, S, N):
    ops = hal['ops']
    lat = _lattice(V, W, S, N)
    R, kind = N * W, lat['kind']
    t = int(lat['length'].max())
    x, lens = lat['x'].to(DEV), lat['T'].int().to(DEV)
    want = J.prefix_scores(lat['xr'], lat['Tr'], lat['state'].double(), lat['last'])
    want[kind != 1] = NINF
    score = torch.where(kind == 0, torch.tensor(NINF), -torch.rand(R, generator=torch.Generator().manual_seed(5)) * 5).view(N, W)
    psi = torch.full((R, V), float('nan'), device=DEV)
    ops.ctc_prefix_scores(x, lens, lat['state'].to(DEV), t, ETX, psi, lat['last'].int().view(N, W).to(DEV),
                          lat['length'].int().view(N, W).to(DEV), score.to(DEV), (kind == 2).int().view(N, W).to(DEV))
    assert not bool(psi.isnan().any())
    _close(psi, want, **LATTICE)
    psi = psi.cpu()
    assert bool((psi[:, 0] == NINF).all()) and bool((psi[kind != 1] == NINF).all())     # the blank column; empty and finished slots
    live = (kind == 1).nonzero().view(-1)
    both = torch.logaddexp(lat['state'][:, :, 0].double(), lat['state'][:, :, 1].double())
    _close(psi[live, ETX], both[live, lat['Tr'][live] - 1], **LATTICE)                 # the ETX column: the full-sequence mass
    assert bool(torch.isfinite(psi[live][:, 1]).any())
    # step 0: no record is read, slot 0 of every utterance holds the empty prefix
    init = J.prefix_init(lat['xr'], lat['Tr'])
    want0 = J.prefix_scores(lat['xr'], lat['Tr'], init.float().double(), torch.full((R,), -1))
    want0[torch.arange(R) % W != 0] = NINF
    psi0 = torch.full((R, V), float('nan'), device=DEV)
    ops.ctc_prefix_scores(x, lens, init.float().to(DEV), 0, ETX, psi0)
    _close(psi0, want0, **LATTICE)


@pytest.mark.parametrize('V,W,S,N', SHAPES)
def test_prefix_advance_against_float64(hal, V, W, S, N):
    ops = hal['ops']
    lat = _lattice(V, W, S, N)
    R, labels = N * W, lat['labels']
    g = torch.Generator().manual_seed(3 * V + W)
    x, lens = lat['x'].to(DEV), lat['T'].int().to(DEV)
    par = torch.randint(0, W, (N, W), generator=g)
    par[:, 1::2] = torch.arange(W)[1::2]                                             # odd slots continue themselves: a prefix with a last token
    src = (torch.arange(N)[:, None] * W + par).view(-1)
    plast, plen = lat['last'][src], lat['length'][src]
    k = labels[torch.randint(0, len(labels), (R,), generator=g)]
    k = torch.where((torch.arange(R) % W % 2 == 1) & (plast >= 0), plast, k)           # and extend with their parent's last token
    kept = torch.ones(R, dtype=torch.bool)
    kept[torch.arange(R) % 5 == 3] = False                                           # empty slots
    closed = torch.arange(R) % 7 == 5                                                # slots that took ETX
    assert bool((kept & ~closed & (k == plast)).any())
    want = J.prefix_advance(lat['xr'], lat['Tr'], lat['state'].double()[src], plast, k)
    out = torch.full((R, S, 2), 7.0, device=DEV)
    ops.ctc_prefix_advance(x, lens, ETX, out, lat['state'].to(DEV), torch.where(kept, par.view(-1), -1).int().view(N, W).to(DEV),
                           torch.where(closed, ETX, k).int().view(N, W).to(DEV), (plen + 1).int().view(N, W).to(DEV),
                           lat['last'].int().view(N, W).to(DEV))
    out = out.cpu()
    frames = torch.arange(S)[None, :] < lat['Tr'][:, None]
    wrote = (kept & ~closed)[:, None] & frames
    assert bool((out[~wrote] == 7.0).all())                                          # frames at or past T_n, finished and empty slots
    _close(out[wrote], want[wrote], **LATTICE)
    # step 0 (parents None): the empty prefix's state into slot 0 of every utterance
    out0 = torch.full((R, S, 2), 7.0, device=DEV)
    ops.ctc_prefix_advance(x, lens, ETX, out0)
    out0 = out0.cpu()
    wrote0 = (torch.arange(R) % W == 0)[:, None] & frames
    assert bool((out0[~wrote0] == 7.0).all())
    _close(out0[wrote0], J.prefix_init(lat['xr'], lat['Tr'])[wrote0], **LATTICE)


def test_prefix_launch_refusals(hal):
    ops, lib = hal['ops'], hal['lib']
    N, W, V = 1, 2, 8
    lens = torch.ones(N, dtype=torch.int32, device=DEV)

    def run(N, W, S, V):
        x, st = torch.zeros(N, S, V, device=DEV), torch.zeros(N * W, S, 2, device=DEV)
        ops.ctc_prefix_scores(x, torch.ones(N, dtype=torch.int32, device=DEV), st, 0, ETX, torch.zeros(N * W, V, device=DEV))
        ops.ctc_prefix_advance(x, torch.ones(N, dtype=torch.int32, device=DEV), ETX, st)

    run(N, W, 16, V)
    for bad in ((N, W, 4097, V), (N, 17, 16, V)):                                     # S > 4096, W > 16
        with pytest.raises(lib.HaloError):
            run(*bad)
    x, st, psi = torch.zeros(N, 16, V, device=DEV), torch.zeros(N * W, 16, 2, device=DEV), torch.zeros(N * W, V, device=DEV)
    with pytest.raises(lib.HaloError):
        ops.ctc_prefix_scores(x, lens, st, 0, V, psi)                                  # ETX outside the classes
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens, st[:, :8], 0, ETX, psi)
    with pytest.raises(ValueError):
        ops.ctc_prefix_scores(x, lens, st, 0, ETX, psi[:, :V - 1])
    rec = torch.zeros(N, W, dtype=torch.int32, device=DEV)
    with pytest.raises(lib.HaloError):
        ops.ctc_prefix_advance(x, lens, ETX, st, st, rec, rec, rec, rec)               # one copy of the states for both
    with pytest.raises(ValueError):
        ops.ctc_prefix_advance(x, lens, ETX, st, st.clone(), rec[:, :1], rec, rec, rec)


# ---- halo_decode_beam_select_joint ------------------------------------------------------------------------------------------------------
def _select_ref(logits, t, bonus, c, psi_cand, psi_in, rec, W):
    """One step of the definition in float64 -> the new records and the smallest gap between two candidates of unequal rank at the cut."""
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
    pc = torch.where(live[:, :, None], psi_cand.double().view(N, W, V), torch.full_like(lp, NINF))
    pc[:, :, ETX] = torch.where(done, psi_in.double(), pc[:, :, ETX])
    rk = (1 - c) * (cand + bonus * newlen.double()) + c * pc
    rk = torch.where(rk.isnan(), torch.full_like(rk, NINF), rk)
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
    ninf = torch.full_like(top, NINF)
    nscore = torch.where(taken, cand.view(N, W * V).gather(1, idx), ninf)
    npsi = torch.where(taken, pc.view(N, W * V).gather(1, idx), ninf)
    nlen = torch.where(taken, plen + grow.long(), torch.zeros_like(plen))
    nfin = taken & (pfin | (k == ETX))
    rows = torch.arange(N)[:, None] * W
    nanc = anc.long().view(N, W, -1).gather(1, par[:, :, None].expand(N, W, anc.shape[1])).clone()
    nanc = torch.where(taken[:, :, None], nanc, (rows + own)[:, :, None].expand_as(nanc))
    nanc[:, :, t] = rows + par
    tok_next = torch.where(taken, k, torch.full_like(k, ETX))
    return dict(score=nscore, rank=torch.where(taken, top, ninf), psi=npsi, length=nlen, fin=nfin, tokens=ntok, anc=nanc.view(N * W, -1),
                next=tok_next, parents=torch.where(taken, par, torch.full_like(par, -1)), gap=gap)


def _select_inputs(V, W, t, finite_psi=False):
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
    psi_cand = -torch.rand(N * W, V, generator=g) * 8
    psi_in = -torch.rand(N, W, generator=g) * 8
    if not finite_psi:
        psi_cand[:, 0] = NINF                                                        # the blank, and classes the lattice cannot reach
        psi_cand[torch.rand(N * W, V, generator=g) < 0.2] = NINF
    if W >= 2:        # two live slots with equal logits, scores, lengths and prefix scores: every pair of their candidates ties
        logits[1], psi_cand[1] = logits[0], psi_cand[0]
        score[0, 1], length[0, 1], fin[0, 1] = score[0, 0], length[0, 0], 0
        fin[0, 0] = 0
    if W >= 4:        # two equal finished slots
        for j in (2, 3):
            score[1, j], length[1, j], fin[1, j], psi_in[1, j] = -0.5, min(t, 2), 1, -1.25
    wte = torch.randn(V, C, generator=g)
    return N, cap, C, logits, (score, length, fin, tokens, anc), psi_cand, psi_in, wte


def _fresh(rec, N, W):
    return (torch.full((N, W), 7.0, device=DEV), *(torch.full(x.shape, -7, dtype=torch.int32, device=DEV) for x in rec[1:]))


@pytest.mark.parametrize('V,W', [(32, 4), (300, 16), (4100, 3)])
@pytest.mark.parametrize('t,bonus', [(0, 0.0), (3, 1.0), (4, 0.0)])
def test_joint_select_against_the_float64_step(hal, V, W, t, bonus):
    ops = hal['ops']
    c = 0.3
    N, cap, C, logits, rec, psi_cand, psi_in, wte = _select_inputs(V, W, t)
    want = _select_ref(logits, t, bonus, c, psi_cand, psi_in, rec, W)
    assert want['gap'] > 1e-4                  # the float32 launch and the float64 step order every pair of unequal candidates alike
    rec_in = tuple(x.to(DEV).contiguous() for x in rec)
    rec_out = _fresh(rec, N, W)
    ranks, psi_out = torch.full((N, W), 7.0, device=DEV), torch.full((N, W), 7.0, device=DEV)
    par, last = (torch.full((N, W), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    y = torch.full((N * W, C), float('nan'), device=DEV)
    ops.decode_beam_select_joint(logits.to(DEV), t, cap, ETX, bonus, c, psi_cand.to(DEV), psi_in.to(DEV), psi_out, rec_in, rec_out, ranks,
                                 par, last, wte.to(DEV), y)
    s, n, f, tok, a = (x.cpu() for x in rec_out)
    for x, ref in zip(rec_in, rec):
        assert torch.equal(x.cpu(), ref)                                             # the copy read is not written
    assert torch.equal(n.long(), want['length']) and torch.equal(f.bool(), want['fin'])
    assert torch.equal(par.cpu().long(), want['parents']) and torch.equal(last.cpu().long(), want['next'])
    _close(s, want['score'], rtol=0, atol=1e-5)
    _close(ranks, want['rank'], rtol=0, atol=1e-5)
    _close(psi_out, want['psi'], rtol=0, atol=1e-5)
    for i in range(N):
        for w in range(W):
            m = int(want['length'][i, w])
            assert tok[i, w, :m].tolist() == want['tokens'][i, w, :m].tolist(), (i, w)
    assert torch.equal(a[:, :t + 1].long(), want['anc'][:, :t + 1])
    assert bool((a[:, t + 1:] == -7).all())                                          # nothing written past position t
    assert torch.equal(y.cpu(), wte[want['next'].view(-1)])


@pytest.mark.parametrize('V,W', [(32, 4), (300, 16), (4100, 3)])
@pytest.mark.parametrize('t,bonus', [(0, 0.0), (3, 1.0)])
def test_joint_select_at_weight_zero_is_the_plain_select_bitwise(hal, V, W, t, bonus):
    ops = hal['ops']
    N, cap, C, logits, rec, psi_cand, psi_in, wte = _select_inputs(V, W, t, finite_psi=True)
    rec_in = tuple(x.to(DEV).contiguous() for x in rec)
    a, b = _fresh(rec, N, W), _fresh(rec, N, W)
    ranks_a, ranks_b = torch.full((N, W), 7.0, device=DEV), torch.full((N, W), 7.0, device=DEV)
    ya, yb = (torch.full((N * W, C), float('nan'), device=DEV) for _ in range(2))
    psi_out = torch.zeros(N, W, device=DEV)
    par, last = (torch.zeros(N, W, dtype=torch.int32, device=DEV) for _ in range(2))
    ops.decode_beam_select(logits.to(DEV), t, cap, ETX, bonus, rec_in, a, ranks_a, wte.to(DEV), ya)
    ops.decode_beam_select_joint(logits.to(DEV), t, cap, ETX, bonus, 0.0, psi_cand.to(DEV), psi_in.to(DEV), psi_out, rec_in, b, ranks_b,
                                 par, last, wte.to(DEV), yb)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(ranks_a, ranks_b) and torch.equal(ya, yb)


def test_joint_select_refusals(hal):
    ops, lib = hal['ops'], hal['lib']
    N, W, V, ld = 2, 2, 32, 4
    rec = lambda: (torch.zeros(N, W, device=DEV), torch.zeros(N, W, dtype=torch.int32, device=DEV), torch.zeros(N, W, dtype=torch.int32, device=DEV),
                   torch.zeros(N, W, ld, dtype=torch.int32, device=DEV), torch.zeros(N * W, ld, dtype=torch.int32, device=DEV))
    a, b = rec(), rec()
    logits, ranks, cand = torch.zeros(N * W, V, device=DEV), torch.zeros(N, W, device=DEV), torch.zeros(N * W, V, device=DEV)
    psi = [torch.zeros(N, W, device=DEV) for _ in range(2)]
    par, last = (torch.zeros(N, W, dtype=torch.int32, device=DEV) for _ in range(2))
    ops.decode_beam_select_joint(logits, 0, ld, ETX, 0.0, 0.3, cand, psi[0], psi[1], a, b, ranks, par, last)
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select_joint(logits, 0, ld, ETX, 0.0, 0.3, cand, psi[0], psi[0], a, b, ranks, par, last)     # one copy of psi
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select_joint(logits, 0, ld, ETX, 0.0, 0.3, cand, psi[0], psi[1], a, a, ranks, par, last)     # one copy of the beam
    with pytest.raises(ValueError):
        ops.decode_beam_select_joint(logits, 0, ld, ETX, 0.0, 1.5, cand, psi[0], psi[1], a, b, ranks, par, last)
    with pytest.raises(ValueError):
        ops.decode_beam_select_joint(logits, 0, ld, ETX, 0.0, 0.3, cand[:, :V - 1], psi[0], psi[1], a, b, ranks, par, last)
    with pytest.raises(ValueError):
        ops.decode_beam_select_joint(logits, 0, ld, ETX, 0.0, 0.3, cand, psi[0], psi[1], a, b, ranks, par.long(), last)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _models(hal, name):
    """The case's Decoder and CTC head on the device, built once."""
    if name not in _MODELS:
        V, hd, heads, L = J.CASES[name][:4]
        pd = A.case_inputs(name)[0]
        dec = hal['tr'].Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
        dec.load_state_dict({k[len('decoder.'):]: v for k, v in pd.items() if k.startswith('decoder.')}, strict=True)
        head = hal['rec'].TemporalClassifier(hd * heads, V)
        with torch.no_grad():
            head.classifier.weight.copy_(J.ctc_head_weight(name))
            head.classifier.bias.zero_()
        _MODELS[name] = (dec.to(DEV).eval(), head.to(DEV).eval())
    return _MODELS[name]


def _log_probs(hal, name, feats=None):
    with torch.no_grad():
        f = A.case_inputs(name)[1] if feats is None else feats
        return _models(hal, name)[1].log_probs(f.to(DEV))


def _run(hal, name, c, feats=None, rows=None, lp=None, bd=None):
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = J.CASES[name]
    _, f, flen, _ = A.case_inputs(name)
    f = f if feats is None else feats
    rows = slice(None) if rows is None else rows
    lp = _log_probs(hal, name, f) if lp is None else lp
    bd = bd or hal['tr'].BeamDecoder(_models(hal, name)[0], N, T, W, bonus)
    out = bd.decode(f[rows].to(DEV), flen[rows].to(DEV), ctc_log_probs=lp[rows], ctc_weight=c)
    return tuple(x.cpu() for x in out) + (bd.last_logprobs.cpu(), bd.last_finished.cpu(), bd.last_ctc.cpu())


def _assert_lists_match_the_oracle(name, c, got, rows=None):
    want = J.case_result(name, c)
    rows = J.compared_rows(name, c) if rows is None else rows
    assert rows
    tokens, lengths, ranks, counts, logprobs, finished, ctc = got
    assert torch.equal(tokens[rows], want['tokens'][rows]) and torch.equal(lengths[rows], want['lengths'][rows])
    assert torch.equal(finished[rows], want['finished'][rows]) and torch.equal(counts[rows], want['counts'][rows])
    for a, b in ((ranks, want['ranks']), (logprobs, want['logprobs']), (ctc, want['ctc'])):
        _close(a[rows], b[rows], rtol=0, atol=2e-3)


@pytest.mark.parametrize('name,c', J.JOINT_CASES)
def test_fused_joint_search_matches_the_float64_search(hal, name, c):
    dec = _models(hal, name)[0]
    assert dec._fused_decode_ok(J.CASES[name][1] * J.CASES[name][2])
    got = _run(hal, name, c)
    _assert_lists_match_the_oracle(name, c, got)
    # and not the attention-only search's lists: the CTC head prunes while the search runs
    plain = A.case_result(name)
    rows = J.compared_rows(name, c)
    assert not torch.equal(got[0][rows, 0], plain['tokens'][rows, 0])


def test_graph_replay_equals_eager_launches_bitwise(hal, monkeypatch):
    monkeypatch.setenv('HALO_DECODE_GRAPH', '1')
    a = _run(hal, 'w4-bonus', 0.3)
    monkeypatch.setenv('HALO_DECODE_GRAPH', '0')
    b = _run(hal, 'w4-bonus', 0.3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('how', ['f32', 'unfused'])
def test_general_path_returns_the_same_lists(hal, monkeypatch, how):
    lib = hal['lib']
    name, c = 'w4-bonus', 0.3
    dec = _models(hal, name)[0]
    fused = _run(hal, name, c)
    lp = _log_probs(hal, name)
    if how == 'f32':
        lib.set_math_mode('f32')
    else:
        monkeypatch.setenv('HALO_DECODE_FUSED', '0')
    try:
        assert not dec._fused_decode_ok(J.CASES[name][1] * J.CASES[name][2])
        general = _run(hal, name, c, lp=lp)
    finally:
        lib.set_math_mode('bf16x3')
    _assert_lists_match_the_oracle(name, c, general)
    rows = J.compared_rows(name, c)
    assert torch.equal(general[0][rows], fused[0][rows]) and torch.equal(general[1][rows], fused[1][rows])


def test_without_the_ctc_head_the_attention_only_bits(hal):
    name = 'w4-bonus'
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = J.CASES[name]
    _, feats, flen, _ = A.case_inputs(name)
    bd = hal['tr'].BeamDecoder(_models(hal, name)[0], N, T, W, bonus)
    f, il, lp = feats.to(DEV), flen.to(DEV), _log_probs(hal, name)
    plain = bd.decode(f, il) + (bd.last_logprobs, bd.last_finished)
    joint = bd.decode(f, il, ctc_log_probs=lp, ctc_weight=0.3)
    assert bd.last_ctc is not None and not torch.equal(joint[0], plain[0])
    for kwargs in (dict(ctc_log_probs=lp, ctc_weight=0.0), dict(ctc_log_probs=None, ctc_weight=0.3)):
        again = bd.decode(f, il, **kwargs) + (bd.last_logprobs, bd.last_finished)
        assert bd.last_ctc is None and all(torch.equal(x, y) for x, y in zip(plain, again))
    want = A.case_result(name)
    rows = A.compared_rows(name)
    assert torch.equal(plain[0].cpu()[rows], want['tokens'][rows])
    with pytest.raises(ValueError):
        bd.decode(f, il, ctc_log_probs=lp, ctc_weight=1.5)
    with pytest.raises(ValueError):
        bd.decode(f, il, ctc_log_probs=lp[:, :, :V - 1], ctc_weight=0.3)
    with pytest.raises(ValueError):
        bd.decode(f, il, ctc_log_probs=lp.double(), ctc_weight=0.3)


def test_frames_past_the_input_lengths_are_never_read(hal):
    name, c = 'w4-bonus', 0.3
    _, feats, flen, _ = A.case_inputs(name)
    lp = _log_probs(hal, name)
    poisoned, lp_bad = feats.clone(), lp.clone()
    for n in range(feats.shape[0]):
        poisoned[n, int(flen[n]):] = float('nan')
        lp_bad[n, int(flen[n]):] = float('nan')
    assert bool(poisoned.isnan().any()) and bool(lp_bad.isnan().any())
    a, b = _run(hal, name, c, lp=lp), _run(hal, name, c, feats=poisoned, lp=lp_bad)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_decodes_of_other_batch_sizes_and_lengths_leave_nothing_behind(hal):
    name, c = 'w4-bonus', 0.3
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = J.CASES[name]
    _, feats, flen, _ = A.case_inputs(name)
    bd = hal['tr'].BeamDecoder(_models(hal, name)[0], N, T, W, bonus)
    lp = _log_probs(hal, name)
    first = _run(hal, name, c, lp=lp, bd=bd)
    few = _run(hal, name, c, lp=lp, bd=bd, rows=slice(0, 3))
    # other S: the same utterances with more frames behind them (never read), then fewer utterances at a shorter S
    g = torch.Generator().manual_seed(1)
    longer = torch.cat([feats, torch.randn(N, 7, feats.shape[2], generator=g)], 1)
    lp_longer = torch.cat([lp, torch.randn(N, 7, V, generator=g).log_softmax(-1).to(DEV)], 1)
    more = _run(hal, name, c, feats=longer, lp=lp_longer, bd=bd)
    short = min(int(flen[:2].max()), S - 1)
    _run(hal, name, c, feats=feats[:, :short].contiguous(), lp=lp[:, :short].contiguous(), bd=bd, rows=slice(0, 2))
    last = _run(hal, name, c, lp=lp, bd=bd)
    assert all(torch.equal(x, y) for x, y in zip(first, last))
    every = J.compared_rows(name, c)
    assert torch.equal(more[0][every], first[0][every]) and torch.equal(more[1][every], first[1][every])
    rows = [n for n in every if n < 3]
    assert rows and torch.equal(few[0][rows], first[0][rows]) and torch.equal(few[1][rows], first[1][rows])


def test_finished_hypotheses_score_as_the_reranking_scores_them(hal):
    from haloop_amd import functional as HF
    name, c = 'w4-bonus', 0.3
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = J.CASES[name]
    _, _, flen, _ = A.case_inputs(name)
    lp = _log_probs(hal, name)
    tokens, lengths, ranks, counts, logprobs, finished, ctc = (x.to(DEV) for x in _run(hal, name, c, lp=lp))
    cap = tokens.shape[2]
    rows = lp[:, None].expand(N, W, S, V).reshape(N * W, S, V)
    il = flen.to(DEV)[:, None].expand(N, W).reshape(-1)
    want = -HF.ctc_loss(rows.permute(1, 0, 2), tokens.clamp(min=0).view(N * W, cap), il, lengths.clamp(min=0).view(-1),
                        reduction='none').view(N, W)
    assert int(finished.sum()) > N
    np.testing.assert_allclose(ctc[finished].cpu().numpy(), want[finished].cpu().numpy(), **LATTICE)
    attention = logprobs + bonus * lengths.clamp(min=0).float()
    joint = (1.0 - c) * attention + c * want
    np.testing.assert_allclose(ranks[finished].cpu().numpy(), joint[finished].cpu().numpy(), **LATTICE)
    assert bool((lengths <= flen.to(DEV)[:, None]).all())                              # no hypothesis outruns its frames


# ---- CTCAttentionDecoder.decode(joint=True) -----------------------------------------------------------------------------------------------
def _joint_model(hal, name, bonus):
    V, hd, heads, L = J.CASES[name][:4]
    model = hal['tr'].CTCAttentionDecoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
    model.load_state_dict(A.case_inputs(name)[0], strict=True)
    with torch.no_grad():
        model.recognizer.classifier.weight.copy_(J.ctc_head_weight(name))
        model.recognizer.classifier.bias.zero_()
    model = model.to(DEV).eval()
    model.decoder.length_bonus = bonus
    return model


def test_ctc_attention_decoder_joint_decode(hal, monkeypatch):
    name, c = 'w4-bonus', 0.3
    V, hd, heads, L, S, N, _, _, W, bonus, _, T = J.CASES[name]
    _, feats, flen, tl = A.case_inputs(name)
    f, il, t = feats.to(DEV), flen.to(DEV), tl.to(DEV)
    model = _joint_model(hal, name, bonus)
    assert model.joint is False
    rerank = model.decode(f, il, t, beam_size=W, ctc_weight=c)
    rerank_lists, rerank_parts = tuple(x.clone() for x in model.last_nbest), tuple(x.clone() for x in model.last_parts)
    out = model.decode(f, il, t, beam_size=W, ctc_weight=c, joint=True)
    assert len(out) == 5 and out[2] == [None] * N
    tokens, lengths, scores, counts = model.last_nbest
    bd = model.decoder._beams['decoder']
    want = J.case_result(name, c)
    rows = J.compared_rows(name, c)
    _assert_lists_match_the_oracle(name, c, tuple(x.cpu() for x in (tokens, lengths, scores, counts, bd.last_logprobs, bd.last_finished,
                                                                    model.last_parts[1])))
    _close(model.last_parts[0][rows], want['attention'][rows], rtol=0, atol=2e-3)
    best = [o.tolist() for o in out[0].unbind()]
    for n in rows:
        m, closed = int(want['lengths'][n, 0]), int(want['finished'][n, 0])
        assert int(out[1][n]) == m + closed and best[n] == want['tokens'][n, 0, :max(m + closed - 1, 0)].tolist()
    np.testing.assert_allclose(out[3].cpu()[rows].double().numpy(), want['logprobs'][rows, 0].numpy(), rtol=0, atol=2e-3)
    # joint=False: today's re-ranking, bit for bit
    again = model.decode(f, il, t, beam_size=W, ctc_weight=c, joint=False)
    assert all(torch.equal(x, y) for x, y in zip(model.last_nbest, rerank_lists))
    assert all(torch.equal(x, y) for x, y in zip(model.last_parts, rerank_parts))
    assert torch.equal(again[1], rerank[1]) and torch.equal(again[3], rerank[3])
    assert not torch.equal(rerank_lists[0], tokens)
    # HALO_ASR_JOINT=1 switches the default
    monkeypatch.setenv('HALO_ASR_JOINT', '1')
    switched = _joint_model(hal, name, bonus)
    assert switched.joint is True
    switched.decode(f, il, t, beam_size=W, ctc_weight=c)
    assert all(torch.equal(x, y) for x, y in zip(switched.last_nbest, (tokens, lengths, scores, counts)))
    switched.decode(f, il, t, beam_size=W, ctc_weight=c, joint=False)
    assert all(torch.equal(x, y) for x, y in zip(switched.last_nbest, rerank_lists))


def test_ctc_attention_decoder_joint_decode_raises(hal):
    name = 'w4'
    V, hd, heads, L = J.CASES[name][:4]
    _, feats, flen, tl = A.case_inputs(name)
    f, il, t = feats.to(DEV), flen.to(DEV), tl.to(DEV)
    model = _joint_model(hal, name, 0.0)
    with pytest.raises(ValueError):
        model.decode(f, il, t, joint=True)                                            # no beam
    with pytest.raises(ValueError):
        model.decode(f, il, t, beam_size=4, joint=True)                               # no weight
    with pytest.raises(NotImplementedError):
        model.decode(f, il, t, prompt=torch.tensor([[7, 9]] * feats.shape[0]), beam_size=2, ctc_weight=0.3, joint=True)
    hot = hal['tr'].CTCAttentionDecoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L).to(DEV).train()
    with pytest.raises(NotImplementedError):
        hot.decode(f, il, t, beam_size=2, ctc_weight=0.3, joint=True)
