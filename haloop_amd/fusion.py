"""Shallow fusion of the LSTM language model (``rnn.Decoder``, the LM the reference trains with ``hal``) into CTC prefix beam search
(csrc/ctc_lm_beam.hip).  The reference has no fused decoder.

``CTCFusionDecoder`` runs ``ctc.ctc_prefix_beam_search``'s search with every candidate ranked by

    logaddexp(pb, pnb) + lm_weight * log P_LM(y) + insertion_bonus * len(y)

(the definition and the tie rules are in include/halo.h) and returns n-best lists in the format of ``transducer.BeamDecoder.decode``.  The
fused path costs ``num_layers + 3`` launches per frame for the whole batch (one ``halo_ctc_lm_beam_step``, the cell launches and
``out_layer`` of the transducer decoders on all N * W slots, ``halo_rnnt_beam_keep``) and reads nothing on the host between its first
launch and its last; the general path runs the same search on ``rnn.Decoder.forward`` at T = 1 over N * W rows, pruned on the host.

``lm_score`` is the teacher-forced LM log-probability of every hypothesis of an n-best list: a rescorer for any list (the transducer's
included) and the independent check on the decoder's ``lm_scores``.
"""
import math

import torch

from . import _lib, ops
from .transducer import BEAM_MAX, BeamDecoder, _HeadDecoder

NEG = float('-inf')


class _LMHead:
    """What ``_HeadDecoder`` reads of a head (its prediction network and its mode), for a bare language model."""

    def __init__(self, lm):
        self.lm = lm

    @property
    def training(self):
        return self.lm.training


def _lae(a, b):
    m = max(a, b)
    return m if m == NEG else m + math.log1p(math.exp(-abs(a - b)))


class CTCFusionDecoder(_HeadDecoder):
    """CTC prefix beam search with LM shallow fusion, with preallocated buffers for ``max_batch`` rows, ``beam`` members per row and
    ``capacity`` symbols per hypothesis.  ``lm``: an ``rnn.Decoder`` over the emissions' V classes, in eval mode, on the device of the
    emissions.  It shares the decode images and the ``fused`` rule of the transducer decoders (bf16x3 / bf16 modes, E == H, H % 512 == 0,
    HALO_RNNT_FUSED != 0); everything else takes the general path."""

    _cells = BeamDecoder._cells

    def __init__(self, lm, max_batch, capacity, beam=4, lm_weight=0.5, insertion_bonus=0.0, start_token=0):
        self.head = _LMHead(lm)
        self.max_batch, self.capacity, self.beam = int(max_batch), int(capacity), int(beam)
        self.lm_weight, self.insertion_bonus, self.start_token = float(lm_weight), float(insertion_bonus), int(start_token)
        if self.max_batch < 1 or self.capacity < 1:
            raise ValueError('CTCFusionDecoder: need max_batch >= 1 and capacity >= 1')
        if self.beam < 1 or self.beam > BEAM_MAX:
            raise ValueError(f'CTCFusionDecoder: beam {self.beam} outside 1 .. {BEAM_MAX}')
        if not (math.isfinite(self.lm_weight) and math.isfinite(self.insertion_bonus)):
            raise ValueError('CTCFusionDecoder: lm_weight and insertion_bonus must be finite')
        E, H, L, V = lm.embedding.weight.shape[1], lm.hidden_dim, lm.num_layers, lm.num_classes
        if self.start_token < 0 or self.start_token >= V:
            raise ValueError(f'CTCFusionDecoder: start_token {self.start_token} outside 0 .. {V - 1}')
        dev = lm.embedding.weight.device
        S, cap = self.max_batch * self.beam, self.capacity
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            if E == H and dev.type == 'cuda':
                # flat buffers, viewed per call at that call's N * W slots.  The beam's records and the state exist twice (frame parity).
                self._rec = [(torch.zeros(S * 4, **f32), torch.zeros(S * 4, **i32), torch.zeros(S * cap, **i32)) for _ in range(2)]
                self._parent, self._last = torch.zeros(S, **i32), torch.zeros(S, **i32)
                self._h, self._c = torch.zeros(2 * L * S * H, **f32), torch.zeros(2 * L * S * H, **f32)
                self._g = torch.zeros(2 * S * V, **f32)
                self._xh, self._top = torch.zeros(L * S * 2 * H, **f32), torch.zeros(S * H, **f32)
        self._device = dev      # of the buffers: an LM moved since needs a new decoder
        self._images = None
        self.iterations = 0     # frames of the last decode
        self.last_parts = None  # (ctc_scores [N, W], lm_scores [N, W]) of the last decode

    def decode(self, emissions, emission_lengths=None, capacity=None, beam=None, lm_weight=None, insertion_bonus=None):
        """emissions [T, N, V] log-probabilities, class 0 the blank (a strided view with a unit class stride is read in place),
        emission_lengths [N] (None: T; clamped to [0, T]) -> (tokens [N, W, capacity] int64, -1 past a hypothesis's length and in absent
        hypotheses; lengths [N, W] int64, -1: absent; scores [N, W] float32 = ctc + lm_weight * lm + insertion_bonus * length, best first,
        -inf: absent; counts [N] int64), and ``last_parts`` = (ctc_scores, lm_scores), both [N, W] float32.  ``capacity`` / ``beam``:
        search with less room than the buffers hold; ``lm_weight`` / ``insertion_bonus``: this call's instead of the decoder's."""
        lm = self.head.lm
        if emissions.dim() != 3 or emissions.shape[0] < 1 or emissions.shape[1] < 1:
            raise ValueError(f'CTCFusionDecoder: emissions must be [T >= 1, N >= 1, V], got {tuple(emissions.shape)}')
        T, N, V = emissions.shape
        if V != lm.num_classes:
            raise ValueError(f'CTCFusionDecoder: the LM has {lm.num_classes} classes, the emissions {V}')
        if N > self.max_batch:
            raise ValueError(f'CTCFusionDecoder: batch {N} outside 1 .. max_batch = {self.max_batch}')
        cap = self.capacity if capacity is None else int(capacity)
        if cap < 1 or cap > self.capacity:
            raise ValueError(f'CTCFusionDecoder: capacity {cap} outside 1 .. {self.capacity}')
        W = self.beam if beam is None else int(beam)
        if W < 1 or W > self.beam:
            raise ValueError(f'CTCFusionDecoder: beam {W} outside 1 .. {self.beam}')
        a = self.lm_weight if lm_weight is None else float(lm_weight)
        b = self.insertion_bonus if insertion_bonus is None else float(insertion_bonus)
        if not (math.isfinite(a) and math.isfinite(b)):
            raise ValueError('CTCFusionDecoder: lm_weight and insertion_bonus must be finite')
        if emission_lengths is not None and tuple(emission_lengths.shape) != (N,):
            raise ValueError(f'CTCFusionDecoder: emission_lengths must be [{N}]')
        if lm.training:
            raise NotImplementedError('CTCFusionDecoder is an inference path: put the LM in eval mode')
        if not emissions.is_cuda or not lm.embedding.weight.is_cuda:
            raise _lib.HaloError('haloop_amd.fusion.CTCFusionDecoder runs on the HIP device only (no CPU path)')
        if lm.embedding.weight.device != self._device or emissions.device != self._device:
            raise _lib.HaloError('CTCFusionDecoder: the LM and the emissions must be on the device the decoder was built on')
        with torch.no_grad():
            e = emissions.detach().float()
            if e.stride(-1) != 1:
                e = e.contiguous()
            if emission_lengths is None:
                il = torch.full((N,), T, device=e.device, dtype=torch.int32)
            else:
                il = emission_lengths.detach().to(device=e.device, dtype=torch.int64).clamp(0, T).int().contiguous()
            rec, lengths, tokens = (self._decode_fused if self.fused else self._decode_general)(e, il, N, W, cap, a, b)
            lengths = lengths.long()
            absent = lengths < 0
            minus = torch.full_like(rec[:, :, 0], NEG)
            ctc_scores = torch.where(absent, minus, torch.logaddexp(rec[:, :, 0], rec[:, :, 1]))
            self.last_parts = (ctc_scores, torch.where(absent, minus, rec[:, :, 2]))
            past = torch.arange(cap, device=tokens.device)[None, None, :] >= lengths[:, :, None]
            return tokens.long().masked_fill(past, -1), lengths, torch.where(absent, minus, rec[:, :, 3]), (~absent).sum(1)

    # ---- the fused path: num_layers + 3 launches per frame ---------------------------------------------------------------------------
    def _decode_fused(self, e, il, N, W, cap, a, b):
        lm = self.head.lm
        layers, head_image = self._decode_images()
        wte, H, L, V = lm.embedding.weight, lm.hidden_dim, lm.num_layers, lm.num_classes
        R, ld = N * W, self.capacity
        frames = max(1, int(il.max().item()))                  # the one host read, before the first launch
        rec = [(f[:R * 4].view(N, W, 4), m[:R * 4].view(N, W, 4), t[:R * ld].view(N, W, ld)) for f, m, t in self._rec]
        parent, last = self._parent[:R].view(N, W), self._last[:R].view(N, W)
        h, c = self._h[:2 * L * R * H].view(2, L, R, H), self._c[:2 * L * R * H].view(2, L, R, H)
        g = self._g[:2 * R * V].view(2, R, V)
        xh, top = self._xh[:L * R * 2 * H].view(L, R, 2 * H), self._top[:R * H].view(R, H)
        xh.zero_(); c[0].zero_()
        xh[0, :, :H] = wte[self.start_token]                   # the LM after the start token, in every slot
        self._cells(xh, c[0], h[0], top, g[0], layers, head_image)
        for t in range(frames):
            q = t & 1
            ops.ctc_lm_beam_step(e, il, t, cap, a, b, g[q], lm.out_layer.bias, rec[q], rec[1 - q], parent, last, wte, h[q], c[q], xh, c[1 - q])
            if t == frames - 1:
                break                                          # the last frame's members need no LM step: lm is in their records
            self._cells(xh, c[1 - q], h[1 - q], top, g[1 - q], layers, head_image)
            ops.rnnt_beam_keep(parent, last, h[q], c[q], g[q], h[1 - q], c[1 - q], g[1 - q])
        self.iterations = frames
        out = rec[frames & 1]
        return out[0].clone(), out[1][:, :, 0].clone(), out[2][:, :, :cap].clone()

    # ---- the general path: the same search on rnn.Decoder.forward at T = 1 over N * W rows, pruned on the host ---------------------------
    def _decode_general(self, e, il, N, W, cap, a, b):
        lm = self.head.lm
        dev, V = e.device, e.shape[2]
        R = N * W
        Ls = il.tolist()
        frames = max(Ls)
        ecpu = [e[:L, n].double().cpu() for n, L in enumerate(Ls)]              # the row's own frames alone
        start = torch.full((1, R), self.start_token, device=dev, dtype=torch.int64)
        g, state = lm.forward(start, lm.init_hidden(R))
        beams = [[dict(y=(), pb=0.0, pnb=NEG, lm=0.0, rank=0.0)] for _ in range(N)]     # member j of row n lives in slot n W + j
        self.iterations = 0
        for t in range(frames):
            self.iterations += 1
            lp = torch.log_softmax(g, -1).double().cpu()                        # one host read per frame
            src, tok = torch.arange(R), torch.zeros(R, dtype=torch.int64)
            for n, B in enumerate(beams):
                if t >= Ls[n]:
                    continue
                et, nb = ecpu[n][t], len(B)
                total = [_lae(m['pb'], m['pnb']) for m in B]
                spb = [total[j] + float(et[0]) for j in range(nb)]
                spnb = [m['pnb'] + float(et[m['y'][-1]]) if m['y'] else NEG for m in B]
                ctc = torch.full((nb, V), NEG, dtype=torch.float64)             # the extensions' CTC mass; -inf: no candidate
                lmn = torch.zeros(nb, V, dtype=torch.float64)
                for j, m in enumerate(B):
                    if len(m['y']) < cap:
                        ctc[j] = et + total[j]
                        if m['y']:
                            ctc[j, m['y'][-1]] = et[m['y'][-1]] + m['pb']
                        lmn[j] = m['lm'] + lp[n * W + j]
                ctc[:, 0] = NEG
                where = {m['y']: j for j, m in enumerate(B)}
                for s, m in enumerate(B):                                       # the extension of y[:-1] by y[-1] merges into y's stay
                    j = where.get(m['y'][:-1]) if m['y'] else None
                    if j is not None and ctc[j, m['y'][-1]] > NEG:
                        spnb[s] = _lae(spnb[s], float(ctc[j, m['y'][-1]]))
                        ctc[j, m['y'][-1]] = NEG
                sctc = torch.tensor([_lae(spb[j], spnb[j]) for j in range(nb)], dtype=torch.float64)
                slm = torch.tensor([m['lm'] for m in B], dtype=torch.float64)
                slen = torch.tensor([float(len(m['y'])) for m in B], dtype=torch.float64)
                stay = torch.where(sctc > NEG, sctc + a * slm + b * slen, torch.full_like(sctc, NEG))
                ext = torch.where(ctc > NEG, ctc + a * lmn + b * (slen[:, None] + 1), torch.full_like(ctc, NEG))
                vals = torch.cat([stay, ext.reshape(-1)])                       # in candidate order
                new = []
                for x in torch.sort(-vals, stable=True).indices[:W].tolist():
                    if not float(vals[x]) > NEG:
                        break
                    j, k = (x, 0) if x < nb else ((x - nb) // V, (x - nb) % V)
                    src[n * W + len(new)], tok[n * W + len(new)] = n * W + j, k
                    if k == 0:
                        new.append(dict(B[j], pb=spb[j], pnb=spnb[j], rank=float(vals[x])))
                    else:
                        new.append(dict(y=B[j]['y'] + (k,), pb=NEG, pnb=float(ctc[j, k]), lm=float(lmn[j, k]), rank=float(vals[x])))
                beams[n] = new
            if t == frames - 1:
                break
            src, tok = src.to(dev), tok.to(dev)
            g, state = g[src], (state[0][:, src].contiguous(), state[1][:, src].contiguous())
            g1, (h1, c1) = lm.forward(tok.view(1, R), state)
            emit = tok != 0
            g = torch.where(emit[:, None], g1, g)
            state = (torch.where(emit[None, :, None], h1, state[0]), torch.where(emit[None, :, None], c1, state[1]))
        rec = torch.full((N, W, 4), NEG, dtype=torch.float32)
        lengths = torch.full((N, W), -1, dtype=torch.int32)
        tokens = torch.zeros(N, W, cap, dtype=torch.int32)
        for n, B in enumerate(beams):
            for w, m in enumerate(B):
                rec[n, w] = torch.tensor([m['pb'], m['pnb'], m['lm'], m['rank']])
                lengths[n, w] = len(m['y'])
                tokens[n, w, :len(m['y'])] = torch.tensor(m['y'], dtype=torch.int32)
        return rec.to(dev), lengths.to(dev), tokens.to(dev)


def lm_score(lm, tokens, lengths, start_token=0):
    """The teacher-forced log-probability under ``lm`` (an ``rnn.Decoder`` in eval mode, on the device) of every hypothesis of an n-best
    list: tokens [..., capacity] int64 (anything past a hypothesis's length), lengths [...] (< 0: absent) -> scores [...] float32 =
    sum_i log_softmax(lm(start_token, y_0 .. y_{i-1}))[y_i]: -inf for an absent hypothesis, 0 for the empty one.  One batched
    ``rnn.Decoder.forward_batch_first``; not differentiable."""
    if tokens.dim() < 1 or tuple(lengths.shape) != tuple(tokens.shape[:-1]):
        raise ValueError(f'lm_score: tokens must be [..., capacity] and lengths [...], got {tuple(tokens.shape)} and {tuple(lengths.shape)}')
    if lm.training:
        raise NotImplementedError('lm_score is an inference path: put the LM in eval mode')
    if not tokens.is_cuda or not lm.embedding.weight.is_cuda:
        raise _lib.HaloError('haloop_amd.fusion.lm_score runs on the HIP device only (no CPU path)')
    dev, cap = tokens.device, tokens.shape[-1]
    with torch.no_grad():
        y = tokens.detach().reshape(-1, cap).long()
        n = lengths.detach().to(dev).reshape(-1).long()
        P = y.shape[0]
        valid = torch.arange(cap, device=dev)[None, :] < n[:, None]
        y = torch.where(valid, y, torch.zeros_like(y))
        inputs = torch.cat([torch.full((P, 1), int(start_token), device=dev, dtype=torch.int64), y[:, :-1]], 1)
        logits, _ = lm.forward_batch_first(inputs, lm.init_hidden(P))                     # [P, capacity, V]
        lp = torch.log_softmax(logits.float(), -1).gather(2, y[:, :, None])[:, :, 0]
        total = torch.where(valid, lp, torch.zeros_like(lp)).sum(1)
        return torch.where(n < 0, torch.full_like(total, NEG), total).view(lengths.shape)
