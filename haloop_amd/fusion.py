"""Shallow fusion of the LSTM language model (``rnn.Decoder``, the LM the reference trains with ``hal``) into CTC prefix beam search
(csrc/ctc_lm_beam.hip).  The reference has no fused decoder.

``CTCFusionDecoder`` runs ``ctc.ctc_prefix_beam_search``'s search with every candidate ranked by

    logaddexp(pb, pnb) + lm_weight * log P_LM(y) + insertion_bonus * len(y)

(the definition and the tie rules are in include/halo.h) and returns n-best lists in the format of ``transducer.BeamDecoder.decode``.  The
fused path costs ``num_layers + 3`` launches per frame for the whole batch (one ``halo_ctc_lm_beam_step``, the cell launches and
``out_layer`` of the transducer decoders on all N * W slots, ``halo_rnnt_beam_keep``) and reads nothing on the host between its first
launch and its last; the general path runs the same search on ``rnn.Decoder.forward`` at T = 1 over N * W rows, pruned on the host.

``TransducerFusionDecoder`` (csrc/rnnt_lm_beam.hip) fuses the same LM into the transducer head's beam search: the
search of ``transducer.BeamDecoder`` with every candidate ranked by its transducer mass + lm_weight * log P_LM(y) + insertion_bonus *
len(y), every hypothesis carrying the states of both the prediction network and the LM.

``AttentionFusionDecoder`` (csrc/decode_beam.hip) fuses the LM into the attention decoder's beam search
(``transformer.BeamDecoder``, with or without the CTC prefix scores): every candidate is ranked by fmaf(lm_weight, log P_LM, rank).  The
search is label-synchronous, so no ``keep`` launch is needed: ``Ll + 1`` launches a step on top of the decoder's.

``lm_score`` is the teacher-forced LM log-probability of every hypothesis of an n-best list: a rescorer for any list (the transducer's
included) and the independent check on the decoder's ``lm_scores``.
"""
import math

import torch

from . import _lib, _slots, functional as HF, ops
from .transducer import BEAM_MAX, SYNC_EVERY, _ranked_finals

NEG = float('-inf')


def _lae(a, b):
    m = max(a, b)
    return m if m == NEG else m + math.log1p(math.exp(-abs(a - b)))


class CTCFusionDecoder:
    """CTC prefix beam search with LM shallow fusion, with preallocated buffers for ``max_batch`` rows, ``beam`` members per row and
    ``capacity`` symbols per hypothesis.  ``lm``: an ``rnn.Decoder`` over the emissions' V classes, in eval mode, on the device of the
    emissions.  It shares the decode images and the ``fused`` rule of the transducer decoders (bf16x3 / bf16 modes, E == H, H % 512 == 0,
    HALO_RNNT_FUSED != 0); everything else takes the general path."""

    def __init__(self, lm, max_batch, capacity, beam=4, lm_weight=0.5, insertion_bonus=0.0, start_token=0):
        self.lm, self._net = lm, _slots.Network(lm)
        self.max_batch, self.capacity, self.beam = int(max_batch), int(capacity), int(beam)
        _slots.check_sizes('CTCFusionDecoder', self, BEAM_MAX)
        self.lm_weight, self.start_token, _, self.insertion_bonus = _fusion_settings('CTCFusionDecoder', lm, lm.num_classes, lm_weight,
                                                                                     start_token, None, insertion_bonus)
        dev = lm.embedding.weight.device
        S, cap = self.max_batch * self.beam, self.capacity
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        self._lstm = _slots.SlotState(self._net, S)               # the LM's state in every slot
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            if self._lstm.allocated:
                # flat buffers, viewed per call at that call's N * W slots.  The beam's records exist twice (frame parity), like the state.
                self._rec = [(torch.zeros(S * 4, **f32), torch.zeros(S * 4, **i32), torch.zeros(S * cap, **i32)) for _ in range(2)]
                self._parent, self._last = torch.zeros(S, **i32), torch.zeros(S, **i32)
        self._device = dev      # of the buffers: an LM moved since needs a new decoder
        self.iterations = 0     # frames of the last decode
        self.last_parts = None  # (ctc_scores [N, W], lm_scores [N, W]) of the last decode

    @property
    def head(self):
        """A compatibility alias for callers of the former ``head`` attribute, which read the LM as ``head.lm``: the decoder itself."""
        return self

    @property
    def fused(self):
        """Whether the fused launches are in use (decided from the LM, the math mode and HALO_RNNT_FUSED as they are now)."""
        return not self.lm.training and self._net.fused

    def decode(self, emissions, emission_lengths=None, capacity=None, beam=None, lm_weight=None, insertion_bonus=None):
        """emissions [T, N, V] log-probabilities, class 0 the blank (a strided view with a unit class stride is read in place),
        emission_lengths [N] (None: T; clamped to [0, T]) -> (tokens [N, W, capacity] int64, -1 past a hypothesis's length and in absent
        hypotheses; lengths [N, W] int64, -1: absent; scores [N, W] float32 = ctc + lm_weight * lm + insertion_bonus * length, best first,
        -inf: absent; counts [N] int64), and ``last_parts`` = (ctc_scores, lm_scores), both [N, W] float32.  ``capacity`` / ``beam``:
        search with less room than the buffers hold; ``lm_weight`` / ``insertion_bonus``: this call's instead of the decoder's."""
        lm = self.lm
        if emissions.dim() != 3 or emissions.shape[0] < 1 or emissions.shape[1] < 1:
            raise ValueError(f'CTCFusionDecoder: emissions must be [T >= 1, N >= 1, V], got {tuple(emissions.shape)}')
        T, N, V = emissions.shape
        if V != lm.num_classes:
            raise ValueError(f'CTCFusionDecoder: the LM has {lm.num_classes} classes, the emissions {V}')
        if N > self.max_batch:
            raise ValueError(f'CTCFusionDecoder: batch {N} outside 1 .. max_batch = {self.max_batch}')
        cap, W = _slots.room('CTCFusionDecoder', self, capacity, beam)
        a, _, _, b = _fusion_settings('CTCFusionDecoder', lm, V, self.lm_weight if lm_weight is None else lm_weight, self.start_token, None,
                                      self.insertion_bonus if insertion_bonus is None else insertion_bonus)
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
            return _slots.mask_tokens(tokens, lengths), lengths, torch.where(absent, minus, rec[:, :, 3]), (~absent).sum(1)

    # ---- the fused path: num_layers + 3 launches per frame ---------------------------------------------------------------------------
    def _decode_fused(self, e, il, N, W, cap, a, b):
        st = self._lstm.view(N, W)
        R, ld = N * W, self.capacity
        frames = max(1, int(il.max().item()))                  # the one host read, before the first launch
        rec = [(f[:R * 4].view(N, W, 4), m[:R * 4].view(N, W, 4), t[:R * ld].view(N, W, ld)) for f, m, t in self._rec]
        parent, last = self._parent[:R].view(N, W), self._last[:R].view(N, W)
        st.start(self.start_token)                             # the LM after the start token, in every slot
        for t in range(frames):
            q = t & 1
            ops.ctc_lm_beam_step(e, il, t, cap, a, b, st.g[q], st.bias, rec[q], rec[1 - q], parent, last, *st.gather(q))
            if t == frames - 1:
                break                                          # the last frame's members need no LM step: lm is in their records
            st.cells(1 - q)
            st.keep(parent, last, q)
        self.iterations = frames
        out = rec[frames & 1]
        return out[0].clone(), out[1][:, :, 0].clone(), out[2][:, :, :cap].clone()

    # ---- the general path: the same search on rnn.Decoder.forward at T = 1 over N * W rows, pruned on the host ---------------------------
    def _decode_general(self, e, il, N, W, cap, a, b):
        lm = self.lm
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
            g, state = _slots.step_general(lm, g, state, src, tok, tok != 0)
        rec = torch.full((N, W, 4), NEG, dtype=torch.float32)
        lengths = torch.full((N, W), -1, dtype=torch.int32)
        tokens = torch.zeros(N, W, cap, dtype=torch.int32)
        for n, B in enumerate(beams):
            for w, m in enumerate(B):
                rec[n, w] = torch.tensor([m['pb'], m['pnb'], m['lm'], m['rank']])
                lengths[n, w] = len(m['y'])
                tokens[n, w, :len(m['y'])] = torch.tensor(m['y'], dtype=torch.int32)
        return rec.to(dev), lengths.to(dev), tokens.to(dev)


class TransducerFusionDecoder:
    """Beam search for a ``recognizer.Transducer`` head with LM shallow fusion inside the search (csrc/rnnt_lm_beam.hip),
    with preallocated buffers for ``max_batch`` rows, ``beam`` hypotheses per row and ``capacity`` symbols per hypothesis.  ``lm``: an
    ``rnn.Decoder`` over the head's V classes, in eval mode, on the head's device; its hidden size and depth may differ from the
    prediction network's.  The search is ``transducer.BeamDecoder``'s with every candidate ranked by

        fma(lm_weight, log P_LM(y), s) + insertion_bonus * len(y)

    s the transducer mass ``BeamDecoder`` ranks by (the definition and the tie rules are in include/halo.h); a hypothesis carries the
    states of both networks, and a kept label steps both.  With both weights 0 it is ``BeamDecoder.decode``, token for token.  The
    fused path runs when both networks satisfy the fused rule of the transducer decoders and costs ``Lp + Ll + 5`` launches per
    alignment step for the whole batch (one ``halo_rnnt_lm_beam_step``; per network its cell launches, ``out_layer`` and
    ``halo_rnnt_beam_keep``); it reads the row lengths once before its first launch and one word every ``SYNC_EVERY`` steps.  Everything
    else takes the general path: the same search on ``rnn.Decoder.forward`` at T = 1 over N * W rows, pruned on the host."""

    def __init__(self, head, lm, max_batch, capacity, beam=4, lm_weight=0.5, insertion_bonus=0.0, start_token=0):
        self.head, self.lm = head, lm
        self.max_batch, self.capacity, self.beam = int(max_batch), int(capacity), int(beam)
        _slots.check_sizes('TransducerFusionDecoder', self, BEAM_MAX)
        self.lm_weight, self.start_token, _, self.insertion_bonus = _fusion_settings('TransducerFusionDecoder', lm, head.lm.num_classes,
                                                                                     lm_weight, start_token, None, insertion_bonus)
        dev = head.lm.embedding.weight.device
        S, cap = self.max_batch * self.beam, self.capacity
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        # the states of the prediction network and of the fusion LM in every slot
        self._lstms = tuple(_slots.SlotState(_slots.Network(net), S) for net in (head.lm, lm))
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            if lm.embedding.weight.device == dev and all(st.allocated for st in self._lstms):
                # flat buffers, viewed per call at that call's N * W slots.  The beam's records exist twice (step parity), like the states.
                self._rec = [(torch.zeros(S * 3, **f32), torch.zeros(S, **i32), torch.zeros(S * cap, **i32)) for _ in range(2)]
                self._parent, self._last = torch.zeros(S, **i32), torch.zeros(S, **i32)
                self._fin = (torch.zeros(S * 3, **f32), torch.zeros(S, **i32), torch.zeros(S, **i32), torch.zeros(S * cap, **i32),
                             torch.zeros(self.max_batch, **i32))
                self._live = torch.zeros(64, **i32)                    # one word per alignment step; grown to T + capacity
        self._device = dev      # of the buffers: a head moved since needs a new decoder
        self.iterations = 0     # alignment steps of the last decode
        self.last_parts = None  # (rnnt_scores [N, W], lm_scores [N, W]) of the last decode

    @property
    def fused(self):
        """Whether the fused launches are in use: both networks satisfy the rule of the transducer decoders, as they are now."""
        return not (self.head.training or self.lm.training) and all(st.network.fused for st in self._lstms)

    def decode(self, features, input_lengths, capacity=None, beam=None, lm_weight=None, insertion_bonus=None):
        """features [N, T, feat_dim], input_lengths [N] (clipped to T) -> (tokens [N, W, capacity] int64, -1 past a hypothesis's length
        and in absent hypotheses; lengths [N, W] int64, -1: absent; scores [N, W] float32 = the rank fma(lm_weight, lm, rnnt) +
        insertion_bonus * length, best first, -inf: absent; counts [N] int64), and ``last_parts`` = (rnnt_scores, lm_scores), both [N, W]
        float32.  ``capacity`` / ``beam``: search with less room than the buffers hold; ``lm_weight`` / ``insertion_bonus``: this
        call's instead of the decoder's."""
        name, lm = 'TransducerFusionDecoder', self.lm
        if features.dim() != 3 or features.shape[1] < 1:
            raise ValueError(f'{name}: features must be [N, T, feat_dim] with T >= 1')
        N, T, _ = features.shape
        if N < 1 or N > self.max_batch:
            raise ValueError(f'{name}: batch {N} outside 1 .. max_batch = {self.max_batch}')
        if tuple(input_lengths.shape) != (N,):
            raise ValueError(f'{name}: input_lengths must be [{N}]')
        cap, W = _slots.room(name, self, capacity, beam)
        a, _, _, b = _fusion_settings(name, lm, self.head.lm.num_classes, self.lm_weight if lm_weight is None else lm_weight,
                                      self.start_token, None, self.insertion_bonus if insertion_bonus is None else insertion_bonus)
        if self.head.training or lm.training:
            raise NotImplementedError(f'{name} is an inference path: put the head and the LM in eval mode')
        if not features.is_cuda or not lm.embedding.weight.is_cuda or not self.head.lm.embedding.weight.is_cuda:
            raise _lib.HaloError(f'haloop_amd.fusion.{name} runs on the HIP device only (no CPU path)')
        if any(x.device != self._device for x in (features, lm.embedding.weight, self.head.lm.embedding.weight)):
            raise _lib.HaloError(f'{name}: the head, the LM and the features must be on the device the decoder was built on')
        with torch.no_grad():
            cl = self.head.classifier
            f = HF.linear(features.float(), cl.weight, cl.bias).contiguous()                   # [N, T, V]
            il = input_lengths.to(device=features.device, dtype=torch.int32).clamp(0, T).contiguous()
            # the finals by (rank descending, order of completion), their records rank | s | lm along
            finals = (self._decode_fused if self.fused else self._decode_general)(f, il, N, W, cap, a, b)
            tokens, lengths, rec, counts = _ranked_finals(*finals, cap)
            rank, rnnt, lms = (x.contiguous() for x in rec.unbind(2))
            self.last_parts = (rnnt, lms)
            return tokens, lengths, rank, counts

    # ---- the fused path: Lp + Ll + 5 launches per alignment step ----------------------------------------------------------------------
    def _decode_fused(self, f, il, N, W, cap, a, b):
        pn, lm = (st.view(N, W) for st in self._lstms)
        R, ld = N * W, self.capacity
        frames = int(il.max().item())                          # the one host read before the first launch
        steps = frames + cap if frames else 1                  # a hypothesis at step i has t + u = i, t < L, u <= cap
        if self._live.numel() < steps:
            self._live = torch.zeros(steps, device=self._live.device, dtype=torch.int32)
        live = self._live[:steps]
        live.zero_()
        rec = [(r[:R * 3].view(N, W, 3), u[:R].view(N, W), t[:R * ld].view(N, W, ld)) for r, u, t in self._rec]
        parent, last = self._parent[:R].view(N, W), self._last[:R].view(N, W)
        fr, fq, fl, ft, fn = self._fin
        fin = (fr[:R * 3].view(N, W, 3), fq[:R].view(N, W), fl[:R].view(N, W), ft[:R * ld].view(N, W, ld), fn[:N])
        pn.start(0)                                            # the zero prefix of training, in every slot
        lm.start(self.start_token)                             # the LM after its start token
        for i in range(steps):
            q = i & 1
            ops.rnnt_lm_beam_step(f, pn.g[q], pn.bias, lm.g[q], lm.bias, il, i, cap, a, b, rec[q], rec[1 - q], parent, last, fin,
                                  *pn.gather(q), *lm.gather(q), live[i:])
            if i == steps - 1 or ((i + 1) % SYNC_EVERY == 0 and int(live[i].item()) == 0):
                break
            for st in (pn, lm):
                st.cells(1 - q)
                st.keep(parent, last, q)
        self.iterations = i + 1
        if int(live[i].item()) != 0:
            raise _lib.HaloError('TransducerFusionDecoder: rows still live after max(L) + capacity alignment steps')
        return fin[0].clone(), fin[1].clone(), fin[2].clone(), fin[3].clone()

    # ---- the general path: the same search on rnn.Decoder.forward at T = 1 over N * W rows, pruned on the host ---------------------------
    def _decode_general(self, f, il, N, W, cap, a, b):
        pn, lm = self.head.lm, self.lm
        dev, T, V = f.device, f.shape[1], f.shape[2]
        R = N * W
        Ls = il.tolist()
        g, state = pn.forward(torch.zeros(1, R, device=dev, dtype=torch.int64), pn.init_hidden(R))
        lg, lstate = lm.forward(torch.full((1, R), self.start_token, device=dev, dtype=torch.int64), lm.init_hidden(R))
        beams = [[((), 0.0, 0.0)] if Ls[n] > 0 else [] for n in range(N)]     # (y, s, lm); hypothesis j of row n lives in slot n W + j
        finals = [[((), 0.0, 0.0, 0.0)] if Ls[n] == 0 else [] for n in range(N)]           # (y, rank, s, lm)
        slot_row = torch.arange(R, device=dev) // W
        f64 = lambda x: torch.tensor(x, dtype=torch.float64)
        self.iterations = 0
        for i in range(T + cap):
            if not any(beams):
                break
            self.iterations += 1
            t = torch.zeros(R, dtype=torch.int64)
            for n, B in enumerate(beams):
                for j, (y, _, _) in enumerate(B):
                    t[n * W + j] = i - len(y)
            jp = torch.log_softmax(f[slot_row, t.to(dev)] + g, -1).double().cpu()      # the host reads of the alignment step
            lp = torch.log_softmax(lg, -1).double().cpu()
            src, tok = torch.arange(R), torch.zeros(R, dtype=torch.int64)
            for n, B in enumerate(beams):
                if not B:
                    continue
                where = {y: j for j, (y, _, _) in enumerate(B)}
                blank = [s + float(jp[n * W + j, 0]) for j, (_, s, _) in enumerate(B)]
                labels = [s + jp[n * W + j, 1:] for j, (_, s, _) in enumerate(B)]
                lms = [m + lp[n * W + j, 1:] for j, (_, _, m) in enumerate(B)]
                gone = [torch.zeros(V - 1, dtype=torch.bool) for _ in B]
                complete = [i - len(y) + 1 == Ls[n] for y, _, _ in B]
                for sidx, (y, _, _) in enumerate(B):         # the extension of y[:-1] by y[-1] merges into y's blank extension (mass only)
                    j = where.get(y[:-1]) if y and not complete[sidx] else None
                    if j is not None:
                        blank[sidx] = float(torch.logaddexp(f64(blank[sidx]), labels[j][y[-1] - 1]))
                        gone[j][y[-1] - 1] = True
                cand, vals = [], []                          # (parent, token, s', lm') in candidate order, and their ranks
                for j, (y, _, m) in enumerate(B):
                    rank = blank[j] + a * m + b * len(y)
                    if complete[j]:
                        finals[n].append((y, rank, blank[j], m))
                    else:
                        cand.append((j, 0, blank[j], m)); vals.append(f64([rank]))
                for j, (y, _, m) in enumerate(B):
                    if len(y) < cap:
                        ks = (~gone[j]).nonzero().view(-1)
                        cand += [(j, int(k) + 1, float(labels[j][k]), float(lms[j][k])) for k in ks]
                        vals.append(labels[j][ks] + a * lms[j][ks] + b * (len(y) + 1))
                new = []
                if cand:
                    vals = torch.cat(vals)
                    for x in torch.sort(-vals, stable=True).indices[:W].tolist():
                        j, k, s, m = cand[x]
                        src[n * W + len(new)], tok[n * W + len(new)] = n * W + j, k
                        new.append((B[j][0] + ((k,) if k else ()), s, m))
                beams[n] = new
            if not any(beams):
                break
            src, tok = src.to(dev), tok.to(dev)
            g, state = _slots.step_general(pn, g, state, src, tok, tok != 0)
            lg, lstate = _slots.step_general(lm, lg, lstate, src, tok, tok != 0)
        rec = torch.full((N, W, 3), NEG, dtype=torch.float32)
        seq, lengths = torch.zeros(N, W, dtype=torch.int32), torch.full((N, W), -1, dtype=torch.int32)
        tokens = torch.zeros(N, W, cap, dtype=torch.int32)
        for n, fin in enumerate(finals):
            best = sorted(range(len(fin)), key=lambda x: (-fin[x][1], x))[:W]
            for w, x in enumerate(best):
                rec[n, w], seq[n, w], lengths[n, w] = torch.tensor(fin[x][1:]), w, len(fin[x][0])
                tokens[n, w, :len(fin[x][0])] = torch.tensor(fin[x][0], dtype=torch.int32)
        return rec.to(dev), seq.to(dev), lengths.to(dev), tokens.to(dev)


class _LMSide:
    """The LM side of ``AttentionFusionDecoder``, as ``transformer.BeamDecoder``'s cores drive it: the slots' lm (two copies by step
    parity) and the LM's state in every slot (``state``: one copy of the logits, the search is label-synchronous), for ``slots`` =
    max_batch * beam rows; ``weight``, ``start_token`` and ``eos`` are those of the running call."""

    def __init__(self, lm, slots, etx):
        self.lm, self.etx = lm, etx
        self.state = _slots.SlotState(_slots.Network(lm), slots, copies=1)
        self.weight, self.start_token, self.eos = 0.0, 0, None
        dev = lm.embedding.weight.device
        self._buf = None
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            if self.state.allocated:               # flat buffers, viewed per call at that call's N * W slots
                self._buf = ([torch.zeros(slots, device=dev, dtype=torch.float32) for _ in range(2)],
                             torch.zeros(slots, device=dev, dtype=torch.int32), torch.zeros(slots, device=dev, dtype=torch.int32))

    @property
    def fused(self):
        return self.state.allocated and not self.lm.training and self.state.network.fused

    def key(self):
        """What a captured search depends on besides the shapes: the LM's parameters as they are now, and the call's three settings."""
        return self.state.network.stamp() + (self.weight, self.start_token, self.eos)

    def start(self, N, W):
        """The views of this search's N * W slots; the LM after the start token, in every slot."""
        lm, par, last = self._buf
        self._lm = [x[:N * W].view(N, W) for x in lm]
        self._par, self._last = par[:N * W].view(N, W), last[:N * W].view(N, W)
        self.state.view(N, W).start(self.start_token)

    def select(self, logits, t, cap, length_bonus, rec_in, rec_out, ranks, wte, y_next, par=None, last=None, c=0.0, psi_cand=None, psi_in=None,
               psi_out=None):
        """Step t's selection with the LM in the rank; the gather for the next LM step unless this is the last."""
        q, st = t & 1, self.state
        ops.decode_beam_select_lm(logits, t, cap, self.etx, length_bonus, st.g[q], st.bias, self._lm[q], self._lm[1 - q], self.weight,
                                  self.eos, rec_in, rec_out, ranks, self._par if par is None else par, self._last if last is None else last,
                                  *(st.gather(q) if t + 1 < cap else (None,) * 5), wte, y_next, c, psi_cand, psi_in, psi_out)

    def step(self, t, cap):
        """The LM's cell launches and out_layer on the rows the selection of step t gathered (the last step: nobody reads them)."""
        if t + 1 < cap:
            self.state.cells(1 - (t & 1))

    def scores(self, cap):
        return self._lm[cap & 1]


class AttentionFusionDecoder:
    """Beam search for a ``transformer.Decoder`` with LM shallow fusion inside the search (csrc/decode_beam.hip; the
    definition: include/halo.h), on ``transformer.BeamDecoder``'s buffers and launch sequence.  ``lm``: an ``rnn.Decoder`` over the
    decoder's V classes, in eval mode, on the decoder's device.  Every slot carries the LM's log-probability ``lm`` of its tokens and the
    LSTM state after ``start_token`` and those tokens; a candidate's rank is

        fmaf(lm_weight, lmc, base)

    ``base`` the rank of ``BeamDecoder`` (attention-only, or the mix with the CTC prefix score), lmc = lm + log P_LM(k) for a label k, lm +
    log P_LM(lm_eos) for ETX (``lm_eos=None``: closing costs nothing), lm for a finished slot.  With ``lm_weight`` 0 it is
    ``BeamDecoder.decode``.  The fused path runs when the decoder's fused decode applies and the LM passes the fused rule of the
    transducer decoders: per step the decoder's launches, ``halo_decode_beam_select_lm``, then ``Ll`` cell launches and one ``out_layer``
    launch for the next step -- ``5 * layers + Ll + 3`` launches (``+ 6`` with CTC), replayed from one captured graph per decode
    unless HALO_DECODE_GRAPH=0.  Everything else (f32 mode, an LM the fused cells refuse, HALO_DECODE_FUSED=0) takes the general path:
    the same search on ``Decoder._step_general`` and ``rnn.Decoder.forward`` at T = 1 over N * W rows."""

    def __init__(self, decoder, lm, max_batch, capacity, beam=4, lm_weight=0.5, length_bonus=0.0, start_token=0, lm_eos=None):
        V = decoder.lm_head.weight.shape[0]
        self.lm_weight, self.start_token, self.lm_eos, _ = _fusion_settings('AttentionFusionDecoder', lm, V, lm_weight, start_token, lm_eos)
        from .transformer import ETX, BeamDecoder as AttentionBeamDecoder     # (transformer imports this module through recognizer)
        self._beam = AttentionBeamDecoder(decoder, max_batch, capacity, beam, length_bonus)      # its buffers, cores and graphs
        self.lm = lm
        self._side = _LMSide(lm, self.max_batch * self.beam, ETX)
        self.last_parts = None  # (attention [N, W], lm_scores [N, W]) of the last decode

    def __getattr__(self, name):
        """decoder, max_batch, capacity, beam, length_bonus, last_logprobs, last_finished, last_ctc: the search's own."""
        if name == '_beam':
            raise AttributeError(name)
        return getattr(self._beam, name)

    @property
    def fused(self):
        """Whether the fused launches are in use: the decoder's rule and the LM's, as they are now."""
        return self._beam.fused and self._side.fused

    def decode(self, features, input_lengths, capacity=None, beam=None, ctc_log_probs=None, ctc_weight=0.0, lm_weight=None):
        """``BeamDecoder.decode`` with the LM in every rank: the same n-best format, scores = the fused rank; ``last_logprobs``,
        ``last_finished`` and ``last_ctc`` as there, and ``last_parts`` = (attention [N, W] = logprob + length_bonus * length, lm_scores
        [N, W]), -inf where absent.  ``lm_weight``: this call's instead of the decoder's."""
        name, lm, dec = 'AttentionFusionDecoder', self.lm, self.decoder
        a = _fusion_settings(name, lm, dec.lm_head.weight.shape[0], self.lm_weight if lm_weight is None else lm_weight, self.start_token,
                             self.lm_eos)[0]
        if lm.training or dec.training:
            raise NotImplementedError(f'{name} is an inference path: put the decoder and the LM in eval mode')
        if not features.is_cuda or not lm.embedding.weight.is_cuda or not dec.wte.weight.is_cuda:
            raise _lib.HaloError(f'haloop_amd.fusion.{name} runs on the HIP device only (no CPU path)')
        if any(x.device != self._beam._device for x in (features, lm.embedding.weight, dec.wte.weight)):
            raise _lib.HaloError(f'{name}: the decoder, the LM and the features must be on the device the decoder was built on')
        side = self._side
        side.weight, side.start_token, side.eos = a, self.start_token, self.lm_eos
        if self.fused:
            side.state.network.images()            # built (or rebuilt after an update) before any capture
        out = self._beam._search(features, input_lengths, capacity, beam, ctc_log_probs, ctc_weight, side)
        lengths = out[1]
        attention = self.last_logprobs + self.length_bonus * lengths.clamp(min=0).float()
        self.last_parts = (torch.where(lengths < 0, torch.full_like(attention, NEG), attention), self._last_lm)
        return out


def _fusion_settings(name, lm, V, lm_weight, start_token, lm_eos=None, insertion_bonus=0.0):
    """The checks of an LM and its settings against a decoder of V classes -> (lm_weight, start_token, lm_eos, insertion_bonus) as
    numbers."""
    if getattr(lm, 'num_classes', None) != V:
        raise ValueError(f'{name}: the LM has {getattr(lm, "num_classes", None)} classes, the decoder {V}')
    a, b, start, eos = float(lm_weight), float(insertion_bonus), int(start_token), None if lm_eos is None else int(lm_eos)
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError(f'{name}: lm_weight and insertion_bonus must be finite')
    if start < 0 or start >= V or (eos is not None and (eos < 0 or eos >= V)):
        raise ValueError(f'{name}: start_token {start} / lm_eos {eos} outside 0 .. {V - 1}')
    return a, start, eos, b


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
