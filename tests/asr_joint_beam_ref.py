"""Float64 restatement of the joint CTC/attention beam search (include/halo.h) over oracle.transformer_ref's blocks, for
tests/test_asr_joint_beam_cpu.py and tests/test_gpu_asr_joint_beam.py.  TEST INFRASTRUCTURE ONLY.

The search is tests/asr_beam_ref.py's (the same slots, steps, candidates, order and `margin` bookkeeping) with one change: the rank of a
candidate is (1 - c) * (score + length_bonus * length) + c * psi, psi the CTC prefix score of the extended token sequence.

The prefix scorer, per utterance with x[t][k], t < T, the CTC head's log-probabilities (class 0 the blank): a prefix g carries r[t][2], the
log-mass of the CTC paths over frames 0 .. t that spell exactly g and end in a non-blank (r[t][0]) or a blank (r[t][1]).  `last` is g's
last token, -1 for the empty prefix.  The three functions are batched over a leading dimension B of (utterance, prefix) pairs; frames at
or past T hold -inf in what they return and are never read from x (x may hold NaN there).
"""
import functools
import math

import torch
import torch.nn.functional as F

import asr_beam_ref as A
from oracle import transformer_ref as tref

STX, ETX, GAP, NINF, CASES = A.STX, A.ETX, A.GAP, A.NINF, A.CASES
JOINT_CASES = (('w4', 0.3), ('w4-bonus', 0.3), ('w8', 0.3), ('w8', 0.5))     # (case of asr_beam_ref.CASES, ctc_weight)


def _past(S, T):
    return torch.arange(S)[None, :] >= T[:, None]                                   # [B, S]


def prefix_init(x, T):
    """x [B, S, V] float64, T [B] -> the empty prefix's state [B, S, 2]."""
    B, S, _ = x.shape
    r = torch.full((B, S, 2), NINF, dtype=torch.float64)
    r[:, :, 1] = torch.where(_past(S, T), torch.zeros((), dtype=torch.float64), x[:, :, 0].double()).cumsum(1)
    r[_past(S, T)] = NINF
    return r


def _phi(r, last, k=None):
    """phi[t] per class [B, S, V] (k None) or for the classes k [B] alone [B, S]."""
    both = torch.logaddexp(r[:, :, 0], r[:, :, 1])
    if k is not None:
        return torch.where(((last == k) & (last >= 0))[:, None], r[:, :, 1], both), both
    return both, both


def prefix_scores(x, T, r, last, etx=ETX):
    """-> psi [B, V]: psi(g, k) for every class, from g's state alone."""
    B, S, V = x.shape
    x = x.double()
    both, _ = _phi(r, last)
    phi = both[:, :, None].expand(B, S, V).clone()
    has = last >= 0
    rows = has.nonzero().view(-1)
    phi[rows, :, last[rows]] = r[rows, :, 1]
    ninf = torch.full((), NINF, dtype=torch.float64)
    ok = ~_past(S, T)[:, 1:, None]
    terms = torch.where(ok, phi[:, :-1] + torch.where(ok, x[:, 1:], ninf), ninf)    # frame t = 1 .. S - 1
    first = torch.where(~has[:, None], x[:, 0], ninf)
    psi = torch.cat([first[:, None], terms], 1).logsumexp(1)
    psi[:, 0] = NINF
    psi[:, etx] = both[torch.arange(B), T - 1]
    return psi


def prefix_advance(x, T, r, last, k):
    """-> the state of g.k [B, S, 2] for the labels k [B] (none 0 or ETX)."""
    B, S, V = x.shape
    x = x.double()
    phi, _ = _phi(r, last, k)
    xk, x0 = x.gather(2, k[:, None, None].expand(B, S, 1))[:, :, 0], x[:, :, 0]
    q = torch.full((B, S, 2), NINF, dtype=torch.float64)
    q[:, 0, 0] = torch.where(last < 0, xk[:, 0], torch.full((), NINF, dtype=torch.float64))
    for t in range(1, S):
        q[:, t, 0] = torch.logaddexp(q[:, t - 1, 0], phi[:, t - 1]) + xk[:, t]
        q[:, t, 1] = torch.logaddexp(q[:, t - 1, 0], q[:, t - 1, 1]) + x0[:, t]
    q[_past(S, T)] = NINF
    return q


def joint_beam_search(p, features, input_lengths, ctc_lp, heads, W, capacity, length_bonus=0.0, ctc_weight=0.3, pre='decoder.',
                      cache_dtype=torch.float16):
    """asr_beam_ref.beam_search's dict plus ctc [N, W] (each hypothesis's psi; -inf absent) and attention [N, W] (score + bonus * length).
    ctc_weight = 0 restates asr_beam_ref.beam_search (psi is carried along and takes no part)."""
    c = float(ctc_weight)
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
    # the prefix scorer's records: every slot starts from the empty prefix's state (only slot 0 is live)
    xr, Tr = ctc_lp.double()[utt], input_lengths[utt]
    state = prefix_init(xr, Tr)                                                      # [R, S, 2]
    last = torch.full((N, W), -1, dtype=torch.long)
    psi = torch.zeros(N, W, dtype=torch.float64)
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
        pc = prefix_scores(xr, Tr, state, last.view(-1)).view(N, W, V)
        pc = torch.where(live[:, :, None], pc, torch.full_like(pc, NINF))
        pc[:, :, ETX] = torch.where(done, psi, pc[:, :, ETX])                         # a finished slot carries its psi
        if c != 0.0:
            rk = (1.0 - c) * rk + c * pc
            rk = torch.where(rk.isnan(), torch.full_like(rk, NINF), rk)
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
        length = torch.where(taken, plen + grow.long(), torch.zeros_like(plen))
        fin = taken & (pfin | (k == ETX))
        src = (torch.arange(N)[:, None] * W + par).view(-1)
        time_k = [cc[src] for cc in time_k]
        time_v = [cc[src] for cc in time_v]
        cur = torch.where(taken, k, torch.full_like(k, ETX)).view(R, 1)
        # the kept slots' prefix states: a slot that took a label runs the recurrence from its parent's state
        plast = last.gather(1, par)
        kk = torch.where(grow, k, torch.ones_like(k)).view(-1)
        grown = prefix_advance(xr, Tr, state[src], plast.view(-1), kk)
        state = torch.where(grow.view(-1)[:, None, None], grown, state[src])
        last = torch.where(grow, k, plast)
    present = score > NINF
    if W > 1:                                                                        # every adjacent pair of the final ranking
        d = rank[:, :-1] - rank[:, 1:]
        d = torch.where(present[:, 1:], d, torch.full_like(d, float('inf')))
        margin = torch.minimum(margin, d.min(dim=1).values)
    lengths = torch.where(present, length, torch.full_like(length, -1))
    past = torch.arange(capacity)[None, None, :] >= lengths[:, :, None]
    attention = torch.where(present, score + length_bonus * length.double(), torch.full_like(score, NINF))
    return dict(tokens=tokens.masked_fill(past, -1), lengths=lengths, ranks=rank, logprobs=score, finished=fin & present,
                counts=present.sum(1), margin=margin, ctc=torch.where(present, psi, torch.full_like(psi, NINF)), attention=attention)


# ---- the cases of the GPU end-to-end tests: asr_beam_ref's decoder, features and lengths, and a CTC head drawn here ---------------------
@functools.lru_cache(maxsize=None)
def ctc_head_weight(name):
    """The weight [V, C] (float64; bias 0) of the case's TemporalClassifier."""
    V, hd, heads = CASES[name][:3]
    C = hd * heads
    g = torch.Generator().manual_seed(100 + CASES[name][6])
    return torch.randn(V, C, generator=g, dtype=torch.float64) * 2 / math.sqrt(C)


@functools.lru_cache(maxsize=None)
def ctc_log_probs(name):
    """The head's log-probabilities [N, S, V] of the case's features in float64 (do not modify)."""
    _, feats, _, _ = A.case_inputs(name)
    return F.linear(feats.double(), ctc_head_weight(name)).log_softmax(-1)


@functools.lru_cache(maxsize=None)
def case_result(name, c):
    """The restatement's lists of a case at ctc_weight c, computed once and shared (do not modify)."""
    V, hd, heads, L, S, N, pseed, dseed, W, bonus, sharp, T = CASES[name]
    pd, feats, flen, tl = A.case_inputs(name)
    return joint_beam_search(pd, feats, flen, ctc_log_probs(name), heads, W, T, bonus, c)


def compared_rows(name, c):
    """Rows of a case whose every decision had a margin of GAP or more."""
    return (case_result(name, c)['margin'] >= GAP).nonzero().view(-1).tolist()
