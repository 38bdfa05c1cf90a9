"""GPU checks of LM shallow fusion inside the attention decoder's beam search (haloop_amd/fusion.py AttentionFusionDecoder,
csrc/decode_beam.hip halo_decode_beam_select_lm):

    halo_decode_beam_select_lm  against a float64 step in torch: integers, tokens, ancestor rows, parents, embeddings and the gathered LM
        rows exact (bitwise copies of the parent's; zeros in the slots that step nothing), scores, ranks, lm and psi within 1e-5 (the
        figure of the existing selection tests); with lm_weight = 0 every output shared with halo_decode_beam_select / _joint equal;
    AttentionFusionDecoder.decode in `bf16x3` against tests/asr_lm_beam_ref.py on the rows whose every decision was decided by GAP =
        4.5e-3 or more: tokens, lengths, finished flags and counts EXACT, log-probabilities, attention and psi within 2e-3, ranks within
        2.1e-3 (2e-3 + 0.7 x 1e-4), lm_scores rtol 1e-5 / atol 1e-4 (the fusion tests' bound for the same cell launches);
    lm_weight = 0 against BeamDecoder.decode, graph replay, reuse, parameters changed in place, NaN past the lengths, the general path,
    Decoder.set_fusion_lm, CTCAttentionDecoder.decode(joint=True), and the refusals.
"""
import copy

import numpy as np
import pytest
import torch

import asr_beam_ref as A
import asr_joint_beam_ref as J
import asr_lm_beam_ref as R
import ctc_lm_beam_ref as LMR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
STX, ETX, NINF = R.STX, R.ETX, R.NINF
LATTICE = dict(rtol=1e-5, atol=1e-4)
LDS_FLOATS = 14336                           # ops.DECODE_BEAM_LM_LDS_FLOATS, asserted below


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, fusion, ops, recognizer, transformer
    _lib.lib()
    _lib.lend_scratch()
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16x3')
    yield dict(ops=ops, tr=transformer, lib=_lib, rec=recognizer, fusion=fusion)
    _lib.set_math_mode(prev)


def _close(got, want, what='', **tol):
    """got float32 against want float64: the same entries infinite, the finite ones within the tolerance."""
    got, want = got.detach().cpu().double(), want.double()
    assert torch.equal(torch.isinf(got), torch.isinf(want)), what
    ok = ~torch.isinf(want)
    if what and bool(ok.any()):
        print(f'{what}: max abs error {float((got[ok] - want[ok]).abs().max()):.3e}')
    np.testing.assert_allclose(got[ok].numpy(), want[ok].numpy(), **tol)


# ---- halo_decode_beam_select_lm alone -----------------------------------------------------------------------------------------------------
H = 512
SELECT_SHAPES = [(3, 1, 5), (2, 3, 67), (2, 16, 300), (2, 4, LDS_FLOATS // 8), (2, 4, LDS_FLOATS // 8 + 1)]     # (N, W, V): the last two
# hold 2 W V = 14336 floats (both tables in LDS) and 14344 (both recomputed from L2)
SELECT_STEPS = [(0, None, False, 1, 0.0), (3, ETX, True, 2, 1.0), (3, None, False, 2, 1.0), (2, 0, True, 1, 0.0)]   # (t, lm_eos, joint, Ll, bonus)


def _select_inputs(N, W, V, t, Ll, tie=False):
    """Live, finished and empty slots mixed (slot 0 of every utterance live); drawn once per shape and step."""
    cap, ld, C = 6, 7, 64
    g = torch.Generator().manual_seed(1000 * V + 31 * W + 7 * t + Ll)
    R_ = N * W
    logits, lg = torch.randn(R_, V, generator=g) * 3, torch.randn(R_, V, generator=g) * 2
    lg_bias = torch.randn(V, generator=g)
    score, lm = -torch.rand(N, W, generator=g) * 6, -torch.rand(N, W, generator=g) * 9
    length = torch.randint(0, t + 1, (N, W), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 4, (N, W), generator=g)                                  # 0: empty, 1: finished, else live
    kind[:, 0] = 2
    score = torch.where(kind == 0, torch.full_like(score, NINF), score)
    fin = (kind == 1).int()
    tokens = torch.randint(min(4, V - 1), V, (N, W, ld), generator=g, dtype=torch.int32)
    anc = torch.randint(0, R_, (R_, ld), generator=g, dtype=torch.int32)
    psi_cand, psi_in = -torch.rand(R_, V, generator=g) * 8, -torch.rand(N, W, generator=g) * 8
    if tie:           # two live slots equal in everything: every pair of their candidates ties, the lower position must win
        logits[1], lg[1], psi_cand[1] = logits[0], lg[0], psi_cand[0]
        score[0, 1], length[0, 1], fin[0, 1], lm[0, 1], psi_in[0, 1] = score[0, 0], length[0, 0], 0, lm[0, 0], psi_in[0, 0]
        fin[0, 0] = 0
    wte, lm_wte = torch.randn(V, C, generator=g), torch.randn(V, H, generator=g)
    h_in, c_in = torch.randn(Ll, R_, H, generator=g), torch.randn(Ll, R_, H, generator=g)
    return dict(cap=cap, C=C, logits=logits, lg=lg, lg_bias=lg_bias, rec=(score, length, fin, tokens, anc), lm=lm, psi_cand=psi_cand,
                psi_in=psi_in, wte=wte, lm_wte=lm_wte, h_in=h_in, c_in=c_in)


def _select_ref(x, W, t, bonus, a, eos, c):
    """One step of the definition in float64 (c None: the attention-only rank) -> the new records, which slots step the LM, and the
    smallest difference between neighbours among each utterance's W + 1 best candidates (ties apart)."""
    score, length, fin, tokens, anc = x['rec']
    lm, psi_in = x['lm'], x['psi_in']
    N, V = score.shape[0], x['logits'].shape[1]
    cap = tokens.shape[2]
    if t == 0:
        score = torch.full_like(score, NINF); score[:, 0] = 0
        length, fin, lm, psi_in = torch.zeros_like(length), torch.zeros_like(fin), torch.zeros_like(lm), torch.zeros_like(psi_in)
    score, length, fin, lm = score.double(), length.long(), fin.bool(), lm.double()
    lp = x['logits'].double().log_softmax(-1).view(N, W, V)
    llp = (x['lg'].double() + x['lg_bias'].double()).log_softmax(-1).view(N, W, V)
    present = score > NINF
    live, done = present & ~fin, present & fin
    cand = torch.where(live[:, :, None], score[:, :, None] + lp, torch.full_like(lp, NINF))
    cand[:, :, ETX] = torch.where(done, score, cand[:, :, ETX])
    newlen = length[:, :, None] + ((torch.arange(V) != ETX)[None, None, :] & live[:, :, None]).long()
    rk = cand + bonus * newlen.double()
    pc = torch.where(live[:, :, None], x['psi_cand'].double().view(N, W, V), torch.full_like(lp, NINF))
    pc[:, :, ETX] = torch.where(done, psi_in.double(), pc[:, :, ETX])
    if c is not None:
        rk = (1 - c) * rk + c * pc
    lmc = lm[:, :, None] + llp
    lmc[:, :, ETX] = lm + llp[:, :, eos] if eos is not None else lm
    lmc[:, :, ETX] = torch.where(done, lm, lmc[:, :, ETX])
    rk = rk + a * lmc
    rk = torch.where(rk.isnan(), torch.full_like(rk, NINF), rk)
    srt, idx = rk.view(N, W * V).sort(dim=1, descending=True, stable=True)
    d = srt[:, :W] - srt[:, 1:W + 1]
    open_ = srt[:, 1:W + 1] > NINF
    ties = int(((d == 0) & open_).sum())
    gap = float(d[(d > 0) & open_].min()) if bool(((d > 0) & open_).any()) else float('inf')
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
    pick = lambda v: torch.where(taken, v.view(N, W * V).gather(1, idx), ninf)
    nlen = torch.where(taken, plen + grow.long(), torch.zeros_like(plen))
    rows = torch.arange(N)[:, None] * W
    nanc = anc.long().view(N, W, -1).gather(1, par[:, :, None].expand(N, W, anc.shape[1])).clone()
    nanc = torch.where(taken[:, :, None], nanc, (rows + own)[:, :, None].expand_as(nanc))
    nanc[:, :, t] = rows + par
    return dict(score=pick(cand), rank=torch.where(taken, top, ninf), psi=pick(pc), lm=pick(lmc), length=nlen, fin=taken & (pfin | (k == ETX)),
                tokens=ntok, anc=nanc.view(N * W, -1), next=torch.where(taken, k, torch.full_like(k, ETX)),
                parents=torch.where(taken, par, torch.full_like(par, -1)), steps=grow, src=rows + par, gap=gap, ties=ties)


def _fresh(rec, N, W):
    return (torch.full((N, W), 7.0, device=DEV), *(torch.full(x.shape, -7, dtype=torch.int32, device=DEV) for x in rec[1:]))


def _launch(ops, x, N, W, t, bonus, a, eos, c, Ll, bias=True, gather=True):
    """The launch on the inputs x -> every output on the CPU."""
    V = x['logits'].shape[1]
    rec_in = tuple(v.to(DEV).contiguous() for v in x['rec'])
    rec_out = _fresh(x['rec'], N, W)
    ranks, lm_out, psi_out = (torch.full((N, W), 7.0, device=DEV) for _ in range(3))
    par, last = (torch.full((N, W), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    y = torch.full((N * W, x['C']), float('nan'), device=DEV)
    xh, c_out = torch.full((Ll, N * W, 2 * H), 7.0, device=DEV), torch.full((Ll, N * W, H), 7.0, device=DEV)
    joint = dict(ctc_weight=c, psi_cand=x['psi_cand'].to(DEV), psi_in=x['psi_in'].to(DEV), psi_out=psi_out) if c is not None else {}
    state = (x['lm_wte'].to(DEV), x['h_in'].to(DEV), x['c_in'].to(DEV), xh, c_out) if gather else (None,) * 5
    ops.decode_beam_select_lm(x['logits'].to(DEV), t, x['cap'], ETX, bonus, x['lg'].to(DEV), x['lg_bias'].to(DEV) if bias else None,
                              x['lm'].to(DEV), lm_out, a, eos, rec_in, rec_out, ranks, par, last, *state, x['wte'].to(DEV), y, **joint)
    for v, ref in zip(rec_in, x['rec']):
        assert torch.equal(v.cpu(), ref)                                             # the copy read is not written
    return dict(rec=tuple(v.cpu() for v in rec_out), ranks=ranks.cpu(), lm=lm_out.cpu(), psi=psi_out.cpu(), par=par.cpu(), last=last.cpu(),
                y=y.cpu(), xh=xh.cpu(), c_out=c_out.cpu())


def _assert_step(x, got, want, N, W, t, Ll, c):
    s, n, f, tok, anc = got['rec']
    assert torch.equal(n.long(), want['length']) and torch.equal(f.bool(), want['fin'])
    assert torch.equal(got['par'].long(), want['parents']) and torch.equal(got['last'].long(), want['next'])
    _close(s, want['score'], 'scores', rtol=0, atol=1e-5)
    _close(got['ranks'], want['rank'], 'ranks', rtol=0, atol=1e-5)
    _close(got['lm'], want['lm'], 'lm', rtol=0, atol=1e-5)
    if c is not None:
        _close(got['psi'], want['psi'], 'psi', rtol=0, atol=1e-5)
    for i in range(N):
        for w in range(W):
            m = int(want['length'][i, w])
            assert tok[i, w, :m].tolist() == want['tokens'][i, w, :m].tolist(), (i, w)
    assert torch.equal(anc[:, :t + 1].long(), want['anc'][:, :t + 1])
    assert bool((anc[:, t + 1:] == -7).all())                                        # nothing written past position t
    assert torch.equal(got['y'], x['wte'][want['next'].view(-1)])
    # the next LM step's rows: bitwise copies of the parent's where a label was taken, zeros elsewhere; the x halves above layer 0 untouched
    steps, src, k = want['steps'].view(-1), want['src'].view(-1), want['next'].view(-1)
    keep = steps[None, :, None].float()
    assert torch.equal(got['xh'][:, :, H:], x['h_in'][:, src] * keep)
    assert torch.equal(got['c_out'], x['c_in'][:, src] * keep)
    assert torch.equal(got['xh'][0, :, :H], x['lm_wte'][k] * keep[0])
    assert bool((got['xh'][1:, :, :H] == 7.0).all())
    return int(steps.sum()), int((~steps).sum())


def test_the_exported_lds_budget(hal):
    assert hal['ops'].DECODE_BEAM_LM_LDS_FLOATS == LDS_FLOATS and LDS_FLOATS * 4 < 64 * 1024


@pytest.mark.parametrize('N,W,V', SELECT_SHAPES)
@pytest.mark.parametrize('t,eos,joint,Ll,bonus', SELECT_STEPS)
def test_select_lm_against_the_float64_step(hal, N, W, V, t, eos, joint, Ll, bonus):
    a, c = 0.6, 0.3 if joint else None
    x = _select_inputs(N, W, V, t, Ll)
    want = _select_ref(x, W, t, bonus, a, eos, c)
    assert want['ties'] == 0 and want['gap'] >= 1e-3           # the float32 launch and the float64 step order every pair alike
    got = _launch(hal['ops'], x, N, W, t, bonus, a, eos, c, Ll)
    stepped, idle = _assert_step(x, got, want, N, W, t, Ll, c)
    assert stepped > 0 and (idle > 0 or t == 0 or W <= 3)      # slots that close or stay finished get zeros, not their parent's rows


def test_select_lm_with_fewer_candidates_than_slots(hal):
    """Step 0 at W = 16 over V = 5 classes: five candidates, eleven empty slots (no parent: zeros for the LM, their own ancestor row)."""
    N, W, V, t, Ll = 2, 16, 5, 0, 2
    x = _select_inputs(N, W, V, t, Ll)
    want = _select_ref(x, W, t, 1.0, 0.6, ETX, None)
    assert want['ties'] == 0 and want['gap'] >= 1e-3 and int((want['parents'] < 0).sum()) == N * (W - V)
    got = _launch(hal['ops'], x, N, W, t, 1.0, 0.6, ETX, None, Ll)
    _assert_step(x, got, want, N, W, t, Ll, None)
    assert bool((got['lm'][:, V:] == NINF).all())


def test_select_lm_tie_falls_to_the_lower_position(hal):
    N, W, V, t, Ll = 2, 4, 67, 3, 1
    for c in (None, 0.3):
        x = _select_inputs(N, W, V, t, Ll, tie=True)
        want = _select_ref(x, W, t, 1.0, 0.6, ETX, c)
        assert want['ties'] > 0 and want['gap'] >= 1e-3         # slots 0 and 1 of utterance 0 tie candidate for candidate: the float64
        # step's stable sort keeps the lower position first (at c = 0.3 the cut falls between the two), and the launch must match it
        got = _launch(hal['ops'], x, N, W, t, 1.0, 0.6, ETX, c, Ll)
        _assert_step(x, got, want, N, W, t, Ll, c)


@pytest.mark.parametrize('N,W,V', SELECT_SHAPES)
@pytest.mark.parametrize('t,joint', [(0, False), (3, False), (3, True)])
def test_select_lm_at_weight_zero_equals_the_launches_without_the_lm(hal, N, W, V, t, joint):
    ops = hal['ops']
    x = _select_inputs(N, W, V, t, 1)
    c = 0.3 if joint else None
    got = _launch(ops, x, N, W, t, 1.0, 0.0, ETX, c, 1, bias=False, gather=False)
    rec_in = tuple(v.to(DEV).contiguous() for v in x['rec'])
    rec_out, ranks = _fresh(x['rec'], N, W), torch.full((N, W), 7.0, device=DEV)
    y = torch.full((N * W, x['C']), float('nan'), device=DEV)
    if joint:
        psi_out = torch.full((N, W), 7.0, device=DEV)
        par, last = (torch.full((N, W), -7, dtype=torch.int32, device=DEV) for _ in range(2))
        ops.decode_beam_select_joint(x['logits'].to(DEV), t, x['cap'], ETX, 1.0, c, x['psi_cand'].to(DEV), x['psi_in'].to(DEV), psi_out, rec_in,
                                     rec_out, ranks, par, last, x['wte'].to(DEV), y)
        assert torch.equal(got['psi'], psi_out.cpu()) and torch.equal(got['par'], par.cpu()) and torch.equal(got['last'], last.cpu())
    else:
        ops.decode_beam_select(x['logits'].to(DEV), t, x['cap'], ETX, 1.0, rec_in, rec_out, ranks, x['wte'].to(DEV), y)
    assert all(torch.equal(p, q.cpu()) for p, q in zip(got['rec'], rec_out))
    assert torch.equal(got['ranks'], ranks.cpu()) and torch.equal(got['y'], y.cpu())
    assert bool((got['xh'] == 7.0).all()) and bool((got['c_out'] == 7.0).all())      # no state given: no gather


def test_select_lm_refusals(hal):
    ops, lib = hal['ops'], hal['lib']
    N, W, V, ld = 2, 2, 32, 4
    rec = lambda: (torch.zeros(N, W, device=DEV), torch.zeros(N, W, dtype=torch.int32, device=DEV), torch.zeros(N, W, dtype=torch.int32, device=DEV),
                   torch.zeros(N, W, ld, dtype=torch.int32, device=DEV), torch.zeros(N * W, ld, dtype=torch.int32, device=DEV))
    a, b = rec(), rec()
    logits, ranks, lg = torch.zeros(N * W, V, device=DEV), torch.zeros(N, W, device=DEV), torch.zeros(N * W, V, device=DEV)
    lm = [torch.zeros(N, W, device=DEV) for _ in range(2)]
    par, last = (torch.zeros(N, W, dtype=torch.int32, device=DEV) for _ in range(2))
    state = lambda: (torch.zeros(V, H, device=DEV), torch.zeros(1, N * W, H, device=DEV), torch.zeros(1, N * W, H, device=DEV),
                     torch.zeros(1, N * W, 2 * H, device=DEV), torch.zeros(1, N * W, H, device=DEV))
    ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg, None, lm[0], lm[1], 0.5, None, a, b, ranks, par, last, *state())
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg, None, lm[0], lm[0], 0.5, None, a, b, ranks, par, last)      # one copy of lm
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg, None, lm[0], lm[1], 0.5, None, a, a, ranks, par, last)      # one copy of the beam
    wte, h, c_, xh, c_out = state()
    with pytest.raises(lib.HaloError):
        ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg, None, lm[0], lm[1], 0.5, None, a, b, ranks, par, last, wte, h, c_, xh, c_)
    for weight, eos in ((float('nan'), None), (float('inf'), None), (0.5, V), (0.5, -2)):
        with pytest.raises(ValueError):
            ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg, None, lm[0], lm[1], weight, eos, a, b, ranks, par, last)
    with pytest.raises(ValueError):
        ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg[:, :V - 1], None, lm[0], lm[1], 0.5, None, a, b, ranks, par, last)
    with pytest.raises(ValueError):
        ops.decode_beam_select_lm(logits, 0, ld, ETX, 0.0, lg, None, lm[0], lm[1], 0.5, None, a, b, ranks, par, last, wte, h, c_, xh[:, :, :H], c_out)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _id(case):
    return '-'.join(str(v) for v in case[:8])


def _models(hal, case, fresh=False):
    """The case's Decoder, CTC head and LM on the device, built once (``fresh``: copies of its own for a test that changes them)."""
    name, Ll = R.base_case(case[0]), case[3]
    if (name, Ll) not in _MODELS:
        V, hd, heads, L = A.CASES[name][:4]
        pd = A.case_inputs(name)[0]
        dec = hal['tr'].Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
        dec.load_state_dict({k[len('decoder.'):]: v for k, v in pd.items() if k.startswith('decoder.')}, strict=True)
        head = hal['rec'].TemporalClassifier(hd * heads, V)
        with torch.no_grad():
            head.classifier.weight.copy_(J.ctc_head_weight(name))
            head.classifier.bias.zero_()
        lm = copy.deepcopy(R.language_model(case)[0])
        _MODELS[(name, Ll)] = (dec.to(DEV).eval(), head.to(DEV).eval(), lm.to(DEV).eval())
    models = _MODELS[(name, Ll)]
    return tuple(copy.deepcopy(m) for m in models) if fresh else models


def _log_probs(hal, case, feats=None):
    if not case[2] > 0.0:
        return None
    with torch.no_grad():
        f = R.case_inputs(case[0])[1] if feats is None else feats
        return _models(hal, case)[1].log_probs(f.to(DEV))


def _decoder(hal, case, models=None, lm=None, **over):
    name, W, c, Ll, a, bonus, start, eos, _ = case
    N, T = A.CASES[R.base_case(name)][5], A.CASES[R.base_case(name)][11]
    dec, _, own = models or _models(hal, case)
    kw = dict(beam=W, lm_weight=a, length_bonus=bonus, start_token=start, lm_eos=eos)
    kw.update(over)
    return hal['fusion'].AttentionFusionDecoder(dec, lm or own, N, T, **kw)


def _run(hal, case, fd=None, feats=None, lp=None, rows=None, **kw):
    """-> (tokens, lengths, ranks, counts, logprobs, finished, attention, lm[, ctc]) on the CPU."""
    _, f, flen, _ = R.case_inputs(case[0])
    f = f if feats is None else feats
    rows = slice(None) if rows is None else rows
    lp = _log_probs(hal, case, f) if lp is None else lp
    fd = fd or _decoder(hal, case)
    out = fd.decode(f[rows].to(DEV), flen[rows].to(DEV), ctc_log_probs=None if lp is None else lp[rows], ctc_weight=case[2], **kw)
    ctc = (fd.last_ctc,) if lp is not None else ()
    return tuple(v.cpu() for v in out + (fd.last_logprobs, fd.last_finished) + fd.last_parts + ctc)


def _assert_lists_match(case, got, want=None, rows=None):
    want = R.case_result(case) if want is None else want
    rows = R.compared_rows(case) if rows is None else rows
    assert rows
    tokens, lengths, ranks, counts, logprobs, finished, attention, lm = got[:8]
    assert torch.equal(tokens[rows], want['tokens'][rows]) and torch.equal(lengths[rows], want['lengths'][rows])
    assert torch.equal(finished[rows], want['finished'][rows]) and torch.equal(counts[rows], want['counts'][rows])
    _close(logprobs[rows], want['logprobs'][rows], 'log-probabilities', rtol=0, atol=2e-3)
    _close(attention[rows], want['attention'][rows], 'attention', rtol=0, atol=2e-3)
    _close(ranks[rows], want['ranks'][rows], 'ranks', rtol=0, atol=2.1e-3)
    _close(lm[rows], want['lm'][rows], 'lm_scores', **LATTICE)
    if len(got) > 8:
        _close(got[8][rows], want['ctc'][rows], 'psi', rtol=0, atol=2e-3)


@pytest.mark.parametrize('case', R.CASES, ids=_id)
def test_fused_search_matches_the_float64_search(hal, case):
    fd = _decoder(hal, case)
    assert fd.fused
    got = _run(hal, case, fd)
    _assert_lists_match(case, got)
    # and not the lists of the search without the LM: it prunes while the search runs
    rows = R.compared_rows(case)
    plain = R.case_result(case, 0.0)
    assert not (torch.equal(got[0][rows, 0], plain['tokens'][rows, 0]) and torch.equal(got[5][rows, 0], plain['finished'][rows, 0]))
    if case[7] is None:                          # closing costs nothing: lm_scores are the teacher-forced scores of the tokens
        tokens, lengths = got[0].to(DEV), got[1].to(DEV)
        forced = hal['fusion'].lm_score(_models(hal, case)[2], tokens, lengths, case[6])
        _close(got[7], forced.cpu().double(), 'lm_scores against lm_score', **LATTICE)


@pytest.mark.parametrize('case', [R.CASES[1], R.CASES[3]], ids=_id)
def test_weight_zero_is_the_search_without_the_lm_bitwise(hal, case):
    name, W, c, Ll, a, bonus, start, eos, _ = case
    N, T = A.CASES[name][5], A.CASES[name][11]
    _, f, flen, _ = R.case_inputs(name)
    lp = _log_probs(hal, case)
    bd = hal['tr'].BeamDecoder(_models(hal, case)[0], N, T, W, bonus)
    want = bd.decode(f.to(DEV), flen.to(DEV), ctc_log_probs=lp, ctc_weight=c) + (bd.last_logprobs,)
    fd = _decoder(hal, case)
    got = fd.decode(f.to(DEV), flen.to(DEV), ctc_log_probs=lp, ctc_weight=c, lm_weight=0.0) + (fd.last_logprobs,)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not torch.equal(fd.decode(f.to(DEV), flen.to(DEV), ctc_log_probs=lp, ctc_weight=c)[0], want[0])    # the decoder's own weight again


@pytest.mark.parametrize('case', [R.CASES[1], R.CASES[4]], ids=_id)
def test_graph_replay_equals_eager_launches_and_repeats_bitwise(hal, monkeypatch, case):
    monkeypatch.setenv('HALO_DECODE_GRAPH', '1')
    fd = _decoder(hal, case)
    a, again = _run(hal, case, fd), _run(hal, case, fd)
    monkeypatch.setenv('HALO_DECODE_GRAPH', '0')
    b = _run(hal, case)
    assert all(torch.equal(x, y) for x, y in zip(a, again)) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_decoder_reused_at_other_sizes_repeats_itself(hal):
    case = R.CASES[3]                            # the joint search: every buffer in use
    fd = _decoder(hal, case)
    lp = _log_probs(hal, case)
    first = _run(hal, case, fd, lp=lp)
    few = _run(hal, case, fd, lp=lp, rows=slice(0, 3))
    _run(hal, case, fd, lp=lp, rows=slice(2, 7), beam=3, capacity=5)
    last = _run(hal, case, fd, lp=lp)
    assert all(torch.equal(x, y) for x, y in zip(first, last))
    rows = [n for n in R.compared_rows(case) if n < 3]
    assert rows and torch.equal(few[0][rows], first[0][rows]) and torch.equal(few[1][rows], first[1][rows])


def test_parameters_changed_in_place_are_followed(hal):
    case = R.CASES[1]
    models = _models(hal, case, fresh=True)
    fd = _decoder(hal, case, models)
    before = _run(hal, case, fd)
    with torch.no_grad():
        models[2].out_layer.bias.add_(torch.linspace(-1, 1, models[2].num_classes, device=DEV))
    after_lm = _run(hal, case, fd)
    assert all(torch.equal(x, y) for x, y in zip(after_lm, _run(hal, case, _decoder(hal, case, models))))
    assert not torch.equal(after_lm[2], before[2]) and not torch.equal(after_lm[7], before[7])
    with torch.no_grad():
        models[0].lm_head.weight.mul_(0.9)
    after_dec = _run(hal, case, fd)
    assert all(torch.equal(x, y) for x, y in zip(after_dec, _run(hal, case, _decoder(hal, case, models))))
    assert not torch.equal(after_dec[2], after_lm[2]) and not torch.equal(after_dec[4], after_lm[4])


def test_frames_past_the_input_lengths_are_never_read(hal):
    case = R.CASES[3]
    _, feats, flen, _ = R.case_inputs(case[0])
    lp = _log_probs(hal, case)
    poisoned, lp_bad = feats.clone(), lp.clone()
    for n in range(feats.shape[0]):
        poisoned[n, int(flen[n]):] = float('nan')
        lp_bad[n, int(flen[n]):] = float('nan')
    assert bool(poisoned.isnan().any()) and bool(lp_bad.isnan().any())
    a, b = _run(hal, case, lp=lp), _run(hal, case, feats=poisoned, lp=lp_bad)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('case', [R.CASES[1], R.CASES[4]], ids=_id)
def test_general_path_without_the_fused_decode_agrees(hal, monkeypatch, case):
    fused = _run(hal, case)
    lp = _log_probs(hal, case)
    monkeypatch.setenv('HALO_DECODE_FUSED', '0')
    fd = _decoder(hal, case)
    assert not fd.fused
    general = _run(hal, case, fd, lp=lp)
    _assert_lists_match(case, general)
    rows = R.compared_rows(case)
    assert all(torch.equal(general[i][rows], fused[i][rows]) for i in (0, 1, 3, 5))


def test_general_path_in_f32_mode(hal):
    case, lib = R.CASES[1], hal['lib']
    lib.set_math_mode('f32')
    try:
        fd = _decoder(hal, case)
        assert not fd.fused
        general = _run(hal, case, fd)
    finally:
        lib.set_math_mode('bf16x3')
    _assert_lists_match(case, general)


def test_general_path_with_an_lm_the_fused_cells_refuse(hal):
    """An LM of H = 64 (the fused cells need H % 512 == 0) against the restatement on that LM.  The fixture's own condition: at most a
    third of the rows may have a decision below GAP."""
    case = R.CASES[1]
    name, W, c, Ll, a, bonus, start, eos, _ = case
    N, heads, T = A.CASES[name][5], A.CASES[name][2], A.CASES[name][11]
    small = LMR.make_lm(A.CASES[name][0], Ll, R.LM_SEED, emb=64, hidden=64)
    pd, feats, flen, _ = R.case_inputs(name)
    want = R.lm_beam_search(pd, feats, flen, LMR.LM64(small), heads, W, T, bonus, a, start, eos)
    rows = (want['margin'] >= R.GAP).nonzero().view(-1).tolist()
    assert 3 * (N - len(rows)) <= N
    fd = _decoder(hal, case, lm=copy.deepcopy(small).to(DEV).eval())
    assert not fd.fused and _decoder(hal, case).fused
    _assert_lists_match(case, _run(hal, case, fd), want, rows)


# ---- Decoder.set_fusion_lm and CTCAttentionDecoder.decode(joint=True) --------------------------------------------------------------------
def _joint_model(hal, case):
    name = case[0]
    V, hd, heads, L = A.CASES[name][:4]
    model = hal['tr'].CTCAttentionDecoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L)
    model.load_state_dict(A.case_inputs(name)[0], strict=True)
    with torch.no_grad():
        model.recognizer.classifier.weight.copy_(J.ctc_head_weight(name))
        model.recognizer.classifier.bias.zero_()
    model = model.to(DEV).eval()
    model.decoder.length_bonus = case[5]
    return model


def test_set_fusion_lm_on_the_decoder(hal):
    case = R.CASES[1]
    name, W, c, Ll, a, bonus, start, eos, _ = case
    _, feats, flen, tl = R.case_inputs(name)
    f, il, t = feats.to(DEV), flen.to(DEV), tl.to(DEV)
    model = _joint_model(hal, case)
    dec, lm = model.decoder, _models(hal, case)[2]
    keys, count = list(dec.state_dict().keys()), sum(p.numel() for p in dec.parameters())
    plain = dec.decode(f, il, t, beam_size=W)
    plain_lists = tuple(x.clone() for x in dec.last_nbest)
    greedy = dec.decode(f, il, t)
    assert dec.last_parts is None
    dec.set_fusion_lm(lm, lm_weight=a, start_token=start, lm_eos=eos)
    assert list(dec.state_dict().keys()) == keys and sum(p.numel() for p in dec.parameters()) == count
    assert lm not in list(dec.modules())
    out = dec.decode(f, il, t, beam_size=W)
    fd = _decoder(hal, case, (dec, None, lm))
    want = fd.decode(f, il)
    assert all(torch.equal(x, y) for x, y in zip(dec.last_nbest, want))
    assert all(torch.equal(x, y) for x, y in zip(dec.last_parts, fd.last_parts))
    assert torch.equal(out[3], fd.last_logprobs[:, 0]) and not torch.equal(dec.last_nbest[0], plain_lists[0])
    _assert_lists_match(case, tuple(x.cpu() for x in dec.last_nbest + (fd.last_logprobs, fd.last_finished) + dec.last_parts))
    again = dec.decode(f, il, t)                                                     # greedy decoding does not use the LM
    assert torch.equal(again[1], greedy[1]) and torch.equal(again[3], greedy[3])
    dec.decode(f, il, t, beam_size=W, fusion=False)
    assert all(torch.equal(x, y) for x, y in zip(dec.last_nbest, plain_lists)) and dec.last_parts is None
    dec.set_fusion_lm(None)
    back = dec.decode(f, il, t, beam_size=W)
    assert all(torch.equal(x, y) for x, y in zip(dec.last_nbest, plain_lists)) and dec.last_parts is None
    assert torch.equal(back[1], plain[1]) and torch.equal(back[3], plain[3])


def test_ctc_attention_decoder_joint_decode_with_the_lm(hal):
    case = R.CASES[3]
    name, W, c, Ll, a, bonus, start, eos, _ = case
    _, feats, flen, tl = R.case_inputs(name)
    f, il, t = feats.to(DEV), flen.to(DEV), tl.to(DEV)
    model = _joint_model(hal, case)
    lm = _models(hal, case)[2]
    rerank = model.decode(f, il, t, beam_size=W, ctc_weight=c)
    rerank_lists, rerank_parts = tuple(x.clone() for x in model.last_nbest), tuple(x.clone() for x in model.last_parts)
    model.decode(f, il, t, beam_size=W, ctc_weight=c, joint=True)
    joint_lists = tuple(x.clone() for x in model.last_nbest)
    model.decoder.set_fusion_lm(lm, lm_weight=a, start_token=start, lm_eos=eos)
    out = model.decode(f, il, t, beam_size=W, ctc_weight=c, joint=True)
    assert len(out) == 5 and len(model.last_parts) == 3
    bd = model.decoder._beams['fusion']
    attention, ctc, lms = model.last_parts
    _assert_lists_match(case, tuple(x.cpu() for x in model.last_nbest + (bd.last_logprobs, bd.last_finished, attention, lms, ctc)))
    assert not torch.equal(model.last_nbest[0], joint_lists[0])
    again = model.decode(f, il, t, beam_size=W, ctc_weight=c)                        # the re-ranking route does not use the LM
    assert all(torch.equal(x, y) for x, y in zip(model.last_nbest, rerank_lists))
    assert all(torch.equal(x, y) for x, y in zip(model.last_parts, rerank_parts))
    assert torch.equal(again[1], rerank[1]) and torch.equal(again[3], rerank[3])
    model.decoder.set_fusion_lm(None)
    model.decode(f, il, t, beam_size=W, ctc_weight=c, joint=True)
    assert all(torch.equal(x, y) for x, y in zip(model.last_nbest, joint_lists)) and len(model.last_parts) == 2


def test_refusals_before_any_launch(hal):
    case, lib, fusion = R.CASES[1], hal['lib'], hal['fusion']
    name, W = case[0], case[1]
    V, hd, heads, L = A.CASES[name][:4]
    dec, _, lm = _models(hal, case)
    _, feats, flen, tl = R.case_inputs(name)
    f, il = feats.to(DEV), flen.to(DEV)
    other = LMR.make_lm(V + 1, 1, 1, emb=64, hidden=64).to(DEV)
    for bad in (dict(lm=other), dict(lm_weight=float('nan')), dict(lm_weight=float('inf')), dict(start_token=V), dict(start_token=-1),
                dict(lm_eos=V), dict(lm_eos=-1)):
        with pytest.raises(ValueError):
            _decoder(hal, case, **bad)
        with pytest.raises(ValueError):
            dec.set_fusion_lm(bad.get('lm', lm), **{k: v for k, v in bad.items() if k != 'lm'})
    assert 'lm' not in dec._beams
    fd = _decoder(hal, case)
    with pytest.raises(ValueError):
        fd.decode(f, il, lm_weight=float('nan'))
    hot_lm = copy.deepcopy(lm).train()
    with pytest.raises(NotImplementedError):
        _decoder(hal, case, lm=hot_lm).decode(f, il)
    hot = hal['tr'].Decoder(vocab=V, head_dim=hd, heads=heads, p_drop=0.2, layers=L).to(DEV).train()
    with pytest.raises(NotImplementedError):
        _decoder(hal, case, (hot, None, lm)).decode(f, il)
    with pytest.raises(lib.HaloError):
        _decoder(hal, case, lm=copy.deepcopy(lm).cpu()).decode(f, il)               # the LM on another device
    with pytest.raises(lib.HaloError):
        fd.decode(feats, flen)                                                       # the features on another device
    dec.set_fusion_lm(lm)
    try:
        with pytest.raises(NotImplementedError):
            dec.decode(f, il, tl.to(DEV), prompt=torch.tensor([[7, 9]] * feats.shape[0]), beam_size=W)
    finally:
        dec.set_fusion_lm(None)
