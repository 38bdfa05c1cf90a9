"""Float64 restatement of the attention decoder's beam search with LM shallow fusion (include/halo.h) over
oracle.transformer_ref's blocks, for tests/test_asr_lm_beam_cpu.py and tests/test_gpu_asr_lm_beam.py.  TEST INFRASTRUCTURE ONLY.

The search is tests/asr_joint_beam_ref.py's (the same slots, steps, candidates, order and `margin` bookkeeping; ctc_weight 0: the
attention-only search of tests/asr_beam_ref.py) with these additions.  Every slot carries lm, the LM's log-probability of its tokens, and
the LSTM state behind lp = log_softmax over all V classes after the LM consumed start_token and then the slot's tokens; the LM is
tests/ctc_lm_beam_ref.py's ``LM64``.  The LM score of candidate (j, k) is lmc = lm_j + lp_j[k] for a label, lm_j + lp_j[lm_eos] for
k == ETX (lm_j when lm_eos is None: closing costs nothing) and lm_j for a finished slot's one candidate; rank = base + lm_weight * lmc,
base the rank of the siblings.  A slot that took a label steps the LM from its parent's state with that label.

Which rows a GPU test compares: a prune compares two ranks, each within 2e-3 (the figure of tests/test_gpu_decode.py for this decoder)
plus lm_weight x 1e-4 (the fusion tests' bound for the same cell launches, lm_weight <= 0.7) of the restatement's: 2 x 2.07e-3 =
4.14e-3, rounded up to GAP = 4.5e-3.  A row whose smallest margin is below GAP is compared by no test.
"""
import functools

import torch
import torch.nn.functional as F

import asr_beam_ref as A
import asr_joint_beam_ref as J
import ctc_lm_beam_ref as LMR
from oracle import transformer_ref as tref

STX, ETX, NINF = A.STX, A.ETX, A.NINF
GAP = 4.5e-3
LM_SEED = 1


def lm_beam_search(p, features, input_lengths, lm, heads, W, capacity, length_bonus=0.0, lm_weight=0.5, start_token=0, lm_eos=None,
                   ctc_lp=None, ctc_weight=0.0, pre='decoder.', cache_dtype=torch.float16):
    """lm: an LM64.  -> asr_joint_beam_ref.joint_beam_search's dict (ctc: zeros of the present without ``ctc_lp``) plus lm [N, W]: each
    hypothesis's LM score (-inf absent).  lm_weight = 0 restates the siblings' searches (lm is carried along and takes no part)."""
    c, a = float(ctc_weight) if ctc_lp is not None else 0.0, float(lm_weight)
    p = {k: v.double() for k, v in p.items()}
    features = features.double()
    N, S, C = features.shape
    L, hd, V = tref.n_layers(p, pre), C // heads, p[pre + 'lm_head.weight'].shape[0]
    R = N * W
    rnd = lambda t: t.to(cache_dtype).to(torch.float64)
    utt = torch.arange(N).repeat_interleave(W)
    feats = features[utt]
    mem_k = [rnd(tref._heads(F.linear(feats, p[f'{pre}h.{i}.mix_memory.k.weight']), heads)) for i in range(L)]
    mem_v = [rnd(tref._heads(F.linear(feats, p[f'{pre}h.{i}.mix_memory.v.weight']), heads)) for i in range(L)]
    time_k = [torch.zeros(R, heads, capacity, hd, dtype=torch.float64) for _ in range(L)]
    time_v = [torch.zeros(R, heads, capacity, hd, dtype=torch.float64) for _ in range(L)]
    mem_mask = (torch.arange(S)[None, :] >= input_lengths[:, None])[utt]
    score = torch.full((N, W), NINF, dtype=torch.float64)
    score[:, 0] = 0.0
    length = torch.zeros(N, W, dtype=torch.long)
    fin = torch.zeros(N, W, dtype=torch.bool)
    tokens = torch.full((N, W, capacity), -1, dtype=torch.long)
    rank = torch.full((N, W), NINF, dtype=torch.float64)
    margin = torch.full((N,), float('inf'), dtype=torch.float64)
    cur = torch.full((R, 1), STX, dtype=torch.long)
    is_label = torch.arange(V) != ETX
    own = torch.arange(W)[None, :].expand(N, W)
    if ctc_lp is not None:
        xr, Tr = ctc_lp.double()[utt], input_lengths[utt]
        state = J.prefix_init(xr, Tr)                                                # [R, S, 2]
    last = torch.full((N, W), -1, dtype=torch.long)
    psi = torch.zeros(N, W, dtype=torch.float64)
    # the LM's records: every slot starts from the state after start_token (only slot 0 is live); lm stays finite in absent slots
    lms = torch.zeros(N, W, dtype=torch.float64)
    llp, lh, lc = lm.step(torch.full((R,), int(start_token), dtype=torch.long), *lm.zero_state(R))
    for t in range(capacity):
        y = F.embedding(cur, p[pre + 'wte.weight'])                                  # [R, 1, C]
        for i in range(L):
            bp = f'{pre}h.{i}.'
            xn = tref.layer_norm(y, p[bp + 'ln_time.weight'])
            q = tref._heads(F.linear(xn, p[bp + 'mix_memory.q.weight']), heads)
            m = F.scaled_dot_product_attention(q, mem_k[i], mem_v[i], attn_mask=~mem_mask[:, None, None, :])
            y = y + F.linear(m.transpose(1, 2).reshape(R, 1, C), p[bp + 'mix_memory.proj.weight'])
            q = tref._heads(F.linear(xn, p[bp + 'mix_time.q.weight']), heads)
            time_k[i][:, :, t] = rnd(tref._heads(F.linear(xn, p[bp + 'mix_time.k.weight']), heads))[:, :, 0]
            time_v[i][:, :, t] = rnd(tref._heads(F.linear(xn, p[bp + 'mix_time.v.weight']), heads))[:, :, 0]
            q = tref.rotate_interleaved(q, t0=t)
            k = tref.rotate_interleaved(time_k[i][:, :, :t + 1])
            s = F.scaled_dot_product_attention(q, k, time_v[i][:, :, :t + 1])
            y = y + F.linear(s.transpose(1, 2).reshape(R, 1, C), p[bp + 'mix_time.proj.weight'])
            h = F.gelu(F.linear(tref.layer_norm(y, p[bp + 'ln_chan.weight']), p[bp + 'mix_chan.0.weight']))
            y = y + F.linear(h, p[bp + 'mix_chan.2.weight'])
        lp = F.linear(tref.layer_norm(y[:, -1, :], p[pre + 'ln_f.weight']), p[pre + 'lm_head.weight']).log_softmax(-1).view(N, W, V)
        present = score > NINF
        live, done = present & ~fin, present & fin
        cand = torch.where(live[:, :, None], score[:, :, None] + lp, torch.full_like(lp, NINF))
        cand[:, :, ETX] = torch.where(done, score, cand[:, :, ETX])
        newlen = length[:, :, None] + (is_label[None, None, :] & live[:, :, None]).long()
        rk = cand + length_bonus * newlen.double()
        if ctc_lp is not None:
            pc = J.prefix_scores(xr, Tr, state, last.view(-1)).view(N, W, V)
            pc = torch.where(live[:, :, None], pc, torch.full_like(pc, NINF))
            pc[:, :, ETX] = torch.where(done, psi, pc[:, :, ETX])                     # a finished slot carries its psi
            if c != 0.0:
                rk = (1.0 - c) * rk + c * pc
                rk = torch.where(rk.isnan(), torch.full_like(rk, NINF), rk)
        else:
            pc = torch.zeros_like(rk)
        # the LM's score of every candidate: a label adds its log-probability, closing that of lm_eos (or nothing), a finished slot nothing
        lv = llp.view(N, W, V)
        lmc = lms[:, :, None] + lv
        lmc[:, :, ETX] = lms + lv[:, :, lm_eos] if lm_eos is not None else lms
        lmc[:, :, ETX] = torch.where(done, lms, lmc[:, :, ETX])
        rk = rk + a * lmc
        srt, idx = rk.view(N, W * V).sort(dim=1, descending=True, stable=True)
        if W * V > W:                                                                # the W-th taken against the best not taken
            decided = srt[:, W] > NINF
            margin = torch.where(decided, torch.minimum(margin, srt[:, W - 1] - srt[:, W]), margin)
        top, idx = srt[:, :W], idx[:, :W]
        taken = top > NINF
        par, k = torch.where(taken, idx // V, own), idx % V
        pfin, plen = done.gather(1, par), length.gather(1, par)
        grow = taken & ~pfin & (k != ETX)
        tokens = tokens.gather(1, par[:, :, None].expand(N, W, capacity))
        at = plen.clamp(max=capacity - 1)[:, :, None]
        tokens.scatter_(2, at, torch.where(grow[:, :, None], k[:, :, None], tokens.gather(2, at)))
        score = torch.where(taken, cand.view(N, W * V).gather(1, idx), torch.full_like(top, NINF))
        rank = torch.where(taken, top, torch.full_like(top, NINF))
        psi = torch.where(taken, pc.view(N, W * V).gather(1, idx), torch.full_like(top, NINF))
        lms = torch.where(taken, lmc.view(N, W * V).gather(1, idx), torch.zeros_like(top))
        length = torch.where(taken, plen + grow.long(), torch.zeros_like(plen))
        fin = taken & (pfin | (k == ETX))
        src = (torch.arange(N)[:, None] * W + par).view(-1)
        time_k = [cc[src] for cc in time_k]
        time_v = [cc[src] for cc in time_v]
        cur = torch.where(taken, k, torch.full_like(k, ETX)).view(R, 1)
        plast = last.gather(1, par)
        kk = torch.where(grow, k, torch.ones_like(k)).view(-1)
        if ctc_lp is not None:                                                       # a slot that took a label: from its parent's state
            grown = J.prefix_advance(xr, Tr, state[src], plast.view(-1), kk)
            state = torch.where(grow.view(-1)[:, None, None], grown, state[src])
        last = torch.where(grow, k, plast)
        g = grow.view(-1)
        nlp, nh, nc = lm.step(kk, lh[:, src], lc[:, src])                            # likewise the LM: one step from the parent's state
        llp = torch.where(g[:, None], nlp, llp[src])
        lh, lc = torch.where(g[None, :, None], nh, lh[:, src]), torch.where(g[None, :, None], nc, lc[:, src])
    present = score > NINF
    if W > 1:                                                                        # every adjacent pair of the final ranking
        d = rank[:, :-1] - rank[:, 1:]
        d = torch.where(present[:, 1:], d, torch.full_like(d, float('inf')))
        margin = torch.minimum(margin, d.min(dim=1).values)
    lengths = torch.where(present, length, torch.full_like(length, -1))
    past = torch.arange(capacity)[None, None, :] >= lengths[:, :, None]
    absent = torch.full_like(score, NINF)
    return dict(tokens=tokens.masked_fill(past, -1), lengths=lengths, ranks=rank, logprobs=score, finished=fin & present,
                counts=present.sum(1), margin=margin, ctc=torch.where(present, psi, absent),
                attention=torch.where(present, score + length_bonus * length.double(), absent), lm=torch.where(present, lms, absent))


# ---- the cases: (inputs, W, ctc_weight, LSTM layers, lm_weight, length_bonus, start_token, lm_eos, rows left out: margin < GAP).
#      'w16-s9' is asr_beam_ref's 'w16' with data seed 9 instead of 5.  The left-out rows were found on the CPU with this file's loop;
#      tests/test_asr_lm_beam_cpu.py asserts them.
CASES = (
    ('w4', 4, 0.0, 2, 0.5, 2.5, STX, None, ()),
    ('w4', 4, 0.0, 2, 0.5, 2.0, 0, ETX, (3, 7)),
    ('w8', 8, 0.0, 1, 0.7, 3.0, 0, ETX, (14, 16)),
    ('w8', 8, 0.3, 1, 0.7, 2.0, 0, None, (5,)),
    ('l3-w3', 3, 0.3, 2, 0.5, 2.0, 0, ETX, (1, 10)),
    ('c768', 4, 0.0, 2, 0.5, 0.0, 0, ETX, (1, 11, 18)),
    ('v4100', 3, 0.0, 2, 0.5, 0.0, 0, ETX, ()),                                       # 24600 table floats: both recomputed from L2
    ('t18', 3, 0.0, 1, 0.5, 2.0, 0, ETX, ()),                                         # 18 steps
    ('w16-s9', 16, 0.0, 2, 0.5, 0.0, 0, ETX, (1, 6, 8)),                              # BEAM_MAX; 9600 table floats, in LDS
)
MAX_LEFT_OUT = 15                                                                     # over all cases; per case: a third of its rows


def base_case(name):
    return 'w16' if name == 'w16-s9' else name


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """asr_beam_ref.case_inputs for its own cases; 'w16-s9': 'w16' drawn the same way from data seed 9."""
    if name != 'w16-s9':
        return A.case_inputs(name)
    V, hd, heads, L, S, N, pseed, dseed, W, bonus, sharp, T = A.CASES['w16']
    pd = A.case_inputs('w16')[0]
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(N, S, hd * heads, generator=g)
    flen = torch.randint(3, S + 1, (N,), generator=g)
    tl = torch.randint(4, 9, (N,), generator=g)
    tl[0] = T - 1
    tl.clamp_(max=T - 1)
    return pd, feats, flen, tl


def ctc_log_probs(case):
    """The CTC head's log-probabilities [N, S, V] of a joint case (None: the attention-only search)."""
    return J.ctc_log_probs(case[0]) if case[2] > 0.0 else None


def language_model(case):
    """-> (the rnn.Decoder on the CPU, its LM64) of a case; callers must not modify the module (copy it to the device)."""
    return LMR.language_model(A.CASES[base_case(case[0])][0], case[3], LM_SEED)


@functools.lru_cache(maxsize=None)
def case_result(case, lm_weight=None):
    """The restatement's lists of a case (``lm_weight``: another weight than the case's), computed once and shared (do not modify)."""
    name, W, c, Ll, a, bonus, start, eos, _ = case
    heads, T = A.CASES[base_case(name)][2], A.CASES[base_case(name)][11]
    pd, feats, flen, tl = case_inputs(name)
    return lm_beam_search(pd, feats, flen, language_model(case)[1], heads, W, T, bonus, a if lm_weight is None else lm_weight, start, eos,
                          ctc_log_probs(case), c)


def left_out(case):
    """Rows of a case with a decision whose margin was below GAP, from the restatement."""
    return (case_result(case)['margin'] < GAP).nonzero().view(-1).tolist()


def compared_rows(case):
    N = A.CASES[base_case(case[0])][5]
    return [n for n in range(N) if n not in case[8]]
