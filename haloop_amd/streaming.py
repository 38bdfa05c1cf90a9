"""Streaming LSTM-CTC recognition: audio pushed chunk by chunk, a partial transcript after every chunk.

``rnn.Encoder`` is a stride-4 convolution (kernel 5, padding 3) under a unidirectional LSTM, so a step depends on one frame of
look-ahead and on nothing later: the whole-utterance forward can be cut into chunks that carry a small state.  The reference has no
streaming mode; what it computes on the whole utterance (``infer.LstmCtcRecognizer``) defines the result, and the concatenated steps
of a stream are the steps of the whole-utterance forward of the same frames.

Frame arithmetic (what makes the state small).  Step s of the convolution reads the padded frames 4s .. 4s+4, that is the frames
4s-3 .. 4s+1 of the utterance.  A push takes a multiple of 4 frames, so after any number of pushes a stream has consumed 4m frames
and emitted the steps 0 .. m-1, whose last one read up to frame 4m-3; step m needs the frames 4m-3 .. 4m+1: the last 3 consumed
frames -- the carry -- and the next two.  At ``begin`` the carry is 3 zero frames, the convolution's left padding.

    call                             convolution input             steps emitted
    push                             [carry | chunk], no padding   chunk_frames / 4
    finish with tail length tl       [carry | tail | 3 zeros]      floor((tl + 1) / 4) + 1

Over a stream of T = 4m + tl frames the steps add up to m + floor((tl + 1) / 4) + 1 = floor((T + 1) / 4) + 1, which is
``Encoder.subsampled_lengths(T)``.  Per stream the state is the carry [3, F], the LSTM's (h, c) [L, H], the label of the last step
(the greedy collapse merges a repeat across a call boundary), the hypothesis so far with its length and score.

A call is one short, static chain of launches for all ``max_streams`` slots: ``halo_stream_front`` (convolution, carry, resets),
``ops.lstm_fwd`` with the persistent state as h0 / c0, ``halo_stream_head`` (classifier, log-softmax, collapse, state commit); rows
that did not take part (``active`` False) are left bit-identical.  ``HALO_STREAM_FUSED=0`` runs the same computation on the general
operators (``ops.subsample_fwd`` on the concatenated input, ``ops.gemm``, ``ops.log_softmax_fwd``, ``ops.ctc_greedy`` and torch
operators for the merging), which is the comparator of tools/bench_streaming.py.  ``HALO_STREAM_GRAPH=1`` (or ``use_graph=True``)
replays the push chain from one HIP graph.

``beam=W`` (or ``HALO_STREAM_BEAM=W``, 1 .. 16) adds n-best partials: one more launch behind the head,
``halo_ctc_prefix_beam_advance`` on the call's log-probs, carries a width-W CTC prefix beam per slot, so ``nbest()`` after every call
is ``ctc.ctc_prefix_beam_search`` of the slot's log-probs so far.  The greedy path and ``last`` are unchanged by it.  ``context=graph``
(a ``biasing.ContextGraph``) makes that launch ``halo_ctc_prefix_beam_advance_biased``: phrase boosts inside the search.

``StreamingTransducer`` is the same object over a ``recognizer.Transducer``: the head launch is
``halo_stream_logits`` (the classifier product and the state commit, no softmax) and ``transducer.GreedyStream`` carries the head's
greedy search from call to call.  The two classes share their host side, ``_ChunkedStreams``.
"""
import os

import torch

from . import _lib, ops
from ._capture import capture
from .ctc import PrefixBeamStream
from .ops import NO_DROPOUT, STREAM_ACTIVE, STREAM_BEGIN, STREAM_FINAL
from .rnn import lstm_param_list

_NEVER, _OPEN, _CLOSED = 0, 1, 2
_RING = 16          # pinned host slots for the per-call flags: a slot is rewritten only after the copy that read it has run


class _ChunkedStreams:
    """The host side that ``StreamingRecognizer`` and ``StreamingTransducer`` share: the slot states, the checks of a push and of a
    finish, and the per-call flags and lengths sent through a ring of pinned host slots.  A subclass sets ``max_streams``,
    ``chunk_frames`` and ``_dims`` = (B, Tc, S, F, ...) and then calls ``_init_host``."""

    def _init_host(self, dev):
        B, Tc, _, F = self._dims[:4]
        self._meta = torch.zeros(2, B, device=dev, dtype=torch.int32)            # [0] flags, [1] lengths
        self._pin = torch.zeros(_RING, 2, B, dtype=torch.int32).pin_memory()
        self._pin_np = self._pin.numpy()
        self._pin_events = [None] * _RING
        self._pin_next = 0
        self._frames = torch.zeros(B, Tc, F, device=dev, dtype=torch.float32)    # the graph's input; the frames of a finish without a tail
        self._state = [_NEVER] * B

    @staticmethod
    def _check_geometry(name, conv, chunk_frames, max_streams, capacity):
        if (conv.kernel_size[0], conv.stride[0], conv.padding[0]) != (5, 4, 3) or conv.dilation[0] != 1 or conv.groups != 1:
            raise NotImplementedError(f'{name}: only the subsample geometry kernel 5, stride 4, padding 3 is streamed')
        if chunk_frames % 4 != 0 or not 4 <= chunk_frames <= 124:
            raise ValueError(f'{name}: chunk_frames {chunk_frames} must be a multiple of 4 in 4 .. 124')
        if max_streams < 1 or capacity < 1:
            raise ValueError(f'{name}: max_streams and capacity must be positive')

    def _bools(self, v, default, name):
        B = self.max_streams
        if v is None:
            return [default] * B
        if torch.is_tensor(v):
            if v.is_cuda:
                raise ValueError(f'{type(self).__name__}: {name} is host-side (a sequence of bools or a CPU bool tensor)')
            v = v.tolist()
        v = [bool(e) for e in v]
        if len(v) != B:
            raise ValueError(f'{type(self).__name__}: {name} has {len(v)} entries for {B} slots')
        return v

    def _send_meta(self, flags, lengths):
        """The call's flags and lengths -> the static device buffer, by an asynchronous copy from a pinned host slot."""
        i = self._pin_next
        self._pin_next = (i + 1) % _RING
        if self._pin_events[i] is not None:
            self._pin_events[i].synchronize()             # returns at once unless the device is _RING calls behind
        else:
            self._pin_events[i] = torch.cuda.Event()
        self._pin_np[i, 0, :] = flags
        self._pin_np[i, 1, :] = lengths
        self._meta.copy_(self._pin[i], non_blocking=True)
        self._pin_events[i].record()

    def _push_args(self, frames, active, begin):
        """Checks a push and opens the slots that begin -> (flags, lengths) of the call."""
        name = type(self).__name__
        B, Tc, S, F = self._dims[:4]
        if not torch.is_tensor(frames) or frames.shape != (B, Tc, F) or frames.dtype != torch.float32 or not frames.is_cuda:
            raise ValueError(f'{name}.push: frames must be a float32 HIP tensor [{B}, {Tc}, {F}]')
        active, begin = self._bools(active, True, 'active'), self._bools(begin, False, 'begin')
        flags = [0] * B
        for b in range(B):
            if begin[b] and not active[b]:
                raise ValueError(f'{name}.push: slot {b} begins without being active')
            if active[b] and not begin[b] and self._state[b] != _OPEN:
                raise ValueError(f'{name}.push: slot {b} is closed; pass begin to start a stream in it')
            flags[b] = (STREAM_ACTIVE if active[b] else 0) | (STREAM_BEGIN if begin[b] else 0)
        for b in range(B):
            if begin[b]:
                self._state[b] = _OPEN
        return flags, [Tc if a else 0 for a in active]

    def _finish_args(self, tail, tail_lengths, rows):
        """Checks a finish and closes its slots -> (tail, flags, lengths) of the call."""
        name = type(self).__name__
        B, Tc, S, F = self._dims[:4]
        rows = [s == _OPEN for s in self._state] if rows is None else self._bools(rows, False, 'rows')
        for b in range(B):
            if rows[b] and self._state[b] != _OPEN:
                raise ValueError(f'{name}.finish: slot {b} ' + ('was never begun' if self._state[b] == _NEVER else 'is closed already'))
        if tail is None:
            if tail_lengths is not None and any(int(t) != 0 for t in tail_lengths):
                raise ValueError(f'{name}.finish: tail_lengths without a tail')
            tail, lengths = self._frames, [0] * B
        else:
            if not torch.is_tensor(tail) or tail.dim() != 3 or tail.shape[0] != B or tail.shape[2] != F or tail.shape[1] > Tc - 1 \
                    or tail.dtype != torch.float32 or not tail.is_cuda:
                raise ValueError(f'{name}.finish: tail must be a float32 HIP tensor [{B}, <= {Tc - 1}, {F}]')
            if tail_lengths is None:
                lengths = [tail.shape[1]] * B
            else:
                lengths = [int(t) for t in (tail_lengths.tolist() if torch.is_tensor(tail_lengths) else tail_lengths)]
                if len(lengths) != B or any(not 0 <= t <= tail.shape[1] for b, t in enumerate(lengths) if rows[b]):
                    raise ValueError(f'{name}.finish: tail_lengths must give 0 .. tail.shape[1] frames for every closing slot')
            if tail.shape[1] == 0:
                tail = self._frames
        for b in range(B):
            if rows[b]:
                self._state[b] = _CLOSED
        return tail, [(STREAM_ACTIVE | STREAM_FINAL) if r else 0 for r in rows], [t if r else 0 for r, t in zip(rows, lengths)]

    def _stamp(self):
        """Changes whenever an LSTM weight may have changed (as ``infer.LstmCtcRecognizer._stamp``)."""
        key = (_lib.weights_epoch(),) + tuple((p.data_ptr(), p._version) for p in lstm_param_list(self.encoder.lstm))
        return (hash(key) & 0x7fffffffffffffff) | 1

    def _lstm(self, y, S, buf):
        B, H = self.max_streams, self._dims[6]
        p = lstm_param_list(self.encoder.lstm)
        _, hn, cn, _ = ops.lstm_fwd(y, p[0::4], p[1::4], p[2::4], p[3::4], h0=self._h, c0=self._c, y=buf['feats'], y_strides=(H, S * H),
                                    y_relu=True, want_state=True, expect_backward=False, reserve=buf['reserve'],
                                    weights_stamp=self._stamp())
        return hn, cn

    def _encode_general(self, frames, S, final, buf):
        """The encoder side of a call on the general operators: the reset of h / c of the slots that begin, the convolution on the
        concatenated input, the carry, the LSTM from the carried state -> (hn, cn, n [B] int32, live [B, S], act, beg, fin)."""
        conv = self.encoder.subsample
        B, _, _, F = self._dims[:4]
        dev = frames.device
        flags, length = self._meta[0], self._meta[1]
        act, beg, fin = (flags & STREAM_ACTIVE) != 0, (flags & STREAM_BEGIN) != 0, (flags & STREAM_FINAL) != 0
        self._h.masked_fill_(beg[None, :, None], 0.0)
        self._c.masked_fill_(beg[None, :, None], 0.0)
        Tc = frames.shape[1]
        carry = self._carry.masked_fill(beg[:, None, None], 0.0)
        fr = frames.masked_fill((torch.arange(Tc, device=dev)[None, :] >= length[:, None])[:, :, None], 0.0)
        parts = [carry, fr]
        if 4 * S + 1 > 3 + Tc:
            parts.append(torch.zeros(B, 4 * S + 1 - 3 - Tc, F, device=dev, dtype=torch.float32))
        y, _ = ops.subsample_fwd(torch.cat(parts, dim=1), conv.weight, conv.bias, NO_DROPOUT, pad=0)
        n = torch.where(fin, (length + 1) // 4 + 1, length // 4)
        n = torch.where(act, n, torch.zeros_like(n)).clamp(max=S).to(torch.int32)
        live = torch.arange(S, device=dev)[None, :] < n[:, None]                                  # [B, S]
        y = y.masked_fill(~live.t()[:, :, None], 0.0).contiguous()
        if not final:
            go = act & ~fin
            self._carry.copy_(torch.where(go[:, None, None], frames[:, Tc - 3:], self._carry))
        hn, cn = self._lstm(y, S, buf)
        return hn, cn, n, live, act, beg, fin

    def _commit_general(self, hn, cn, n, act, fin):
        go = (act & ~fin)[None, :, None]
        self._h.copy_(torch.where(go, hn, self._h))
        self._c.copy_(torch.where(go, cn, self._c))
        self._n_steps.copy_(n)


class StreamingRecognizer(_ChunkedStreams):
    """``max_streams`` slots of streaming greedy CTC recognition over ``encoder`` (an ``rnn.Encoder``) and ``recognizer`` (a
    ``recognizer.TemporalClassifier``), both in eval mode.  Every buffer is allocated here, once.

    push(frames [B, chunk_frames, F], active, begin): ``chunk_frames`` more frames for every active slot; ``begin`` starts a new
        stream in a slot (allowed on an open slot too: it abandons that stream).  ``active`` / ``begin`` are host-side sequences of B
        bools (or CPU bool tensors); ``active`` defaults to all slots, ``begin`` to none.
    finish(tail [B, <= chunk_frames - 1, F], tail_lengths, rows): the last frames of the slots in ``rows`` (B host-side bools like
        ``active``; default every open slot) and the convolution's right padding; the slots are closed and need ``begin`` again.
    partial(): copies of (hyp [B, capacity] int64, hyp_len [B] int64, scores [B] fp32, steps [B] int64, truncated [B] bool).  With a
        beam these describe the best hypothesis of ``nbest()``: hyp is tokens[:, 0] with 0 past its length, and scores is that
        hypothesis's log-mass -- the mass of every alignment of the prefix that the search kept, not the sum of the greedy path's step
        scores; truncated[b] says that some member of slot b's beam has reached ``capacity`` (its extensions are refused from then on).
    nbest(): with a beam, copies of (tokens [B, W, capacity] int64, lengths [B, W] int64, scores [B, W] fp32, counts [B] int64) in
        ``ctc.ctc_prefix_beam_search``'s format; a closed slot stays readable until it begins again, a slot never begun holds no
        hypothesis.  Without a beam: ValueError.
    last: (alignments [B, S] int64, step_scores [B, S] fp32, n_steps [B] int32[, log_probs [B, S, V]]) of the latest call, S =
        chunk_frames / 4 for a push and one more for a finish; alignments and step_scores are zeros past a row's n_steps (log_probs
        there mean nothing).  These are the recognizer's own buffers: the next call of the same kind overwrites them.

    Neither call reads from the device or waits for it (the flags travel through a ring of pinned host slots; a slot is waited for
    only if the device is a whole ring of calls behind).  ``use_graph``: None reads HALO_STREAM_GRAPH (default off).
    ``beam``: None reads HALO_STREAM_BEAM (0 .. 16, default 0: the greedy object, launch for launch).
    ``context`` (a ``biasing.ContextGraph`` over the recognizer's classes; needs a beam, else ValueError): the beam's
    launch is the biased one, eager and under graph replay; ``nbest()`` / ``partial()`` then score by CTC mass + boost, and
    nbest_parts() returns copies of (boosts [B, W] fp32, states [B, W] int64).  The greedy path and ``last`` are unchanged by it."""

    def __init__(self, encoder, recognizer, max_streams, chunk_frames=16, capacity=256, use_graph=None, beam=None, context=None):
        if encoder.training or recognizer.training:
            raise ValueError('StreamingRecognizer: put the encoder and the recognizer in eval mode')
        conv = encoder.subsample
        self._check_geometry('StreamingRecognizer', conv, chunk_frames, max_streams, capacity)
        self.encoder, self.recognizer = encoder, recognizer
        self.max_streams, self.chunk_frames, self.capacity = int(max_streams), int(chunk_frames), int(capacity)
        if use_graph is None:
            use_graph = os.environ.get('HALO_STREAM_GRAPH', '0') == '1'
        self.use_graph = bool(use_graph)
        self.fused = os.environ.get('HALO_STREAM_FUSED', '1') != '0'
        if beam is None:
            beam = os.environ.get('HALO_STREAM_BEAM', '0')
        try:
            self.beam = int(beam)
        except ValueError:
            raise ValueError(f'StreamingRecognizer: beam {beam!r} is not a number') from None
        if not 0 <= self.beam <= ops.BEAM_MAX:
            raise ValueError(f'StreamingRecognizer: beam {self.beam} outside 0 .. {ops.BEAM_MAX}')
        if self.beam and self.capacity > ops.PREFIX_BEAM_MAX_CAPACITY:
            raise ValueError(f'StreamingRecognizer: capacity {self.capacity} outside 1 .. {ops.PREFIX_BEAM_MAX_CAPACITY} with a beam')
        dev = conv.weight.device
        if dev.type != 'cuda':
            raise _lib.HaloError('haloop_amd.streaming.StreamingRecognizer runs on the HIP device only (no CPU path)')
        _lib.lend_scratch(device=dev)
        B, Tc, S = self.max_streams, self.chunk_frames, self.chunk_frames // 4
        F, C = conv.in_channels, conv.out_channels
        L, H, V = encoder.lstm.num_layers, encoder.lstm.hidden_size, recognizer.classifier.out_features
        self._dims = (B, Tc, S, F, C, L, H, V)
        f32 = dict(device=dev, dtype=torch.float32)
        self._carry = torch.zeros(B, 3, F, **f32)
        self._h, self._c = torch.zeros(L, B, H, **f32), torch.zeros(L, B, H, **f32)
        self._hyp = torch.zeros(B, self.capacity, device=dev, dtype=torch.int64)
        self._hyp_len = torch.zeros(B, device=dev, dtype=torch.int64)
        self._steps = torch.zeros(B, device=dev, dtype=torch.int64)
        self._score = torch.zeros(B, **f32)
        self._last_label = torch.full((B,), -1, device=dev, dtype=torch.int32)
        self._truncated = torch.zeros(B, device=dev, dtype=torch.bool)
        self._n_steps = torch.zeros(B, device=dev, dtype=torch.int32)
        self._init_host(dev)
        self._bufs = {}
        for s in (S, S + 1):                                                     # a push's launch shape and a finish's
            self._bufs[s] = dict(
                y=torch.zeros(s, B, C, **f32), feats=torch.zeros(B, s, H, **f32), ali=torch.zeros(B, s, device=dev, dtype=torch.int64),
                scores=torch.zeros(B, s, **f32), lp=torch.zeros(B, s, V, **f32), reserve=ops.lstm_reserve(s, B, C, H, L, dev))
        if context is not None and not self.beam:
            raise ValueError('StreamingRecognizer: a context biases the beam search: give a beam of 1 .. 16 with it')
        self._beam = PrefixBeamStream(B, V, self.beam, self.capacity, device=dev, context=context) if self.beam else None
        self._graphs = {}
        self._last = None

    # ---------------------------------------------------------------------------------------------------------------- host side
    def _check_modes(self):
        if self.encoder.training or self.recognizer.training:
            raise ValueError('StreamingRecognizer: put the encoder and the recognizer in eval mode')

    @torch.no_grad()
    def push(self, frames, active=None, begin=None, want_log_probs=False):
        self._check_modes()
        flags, lengths = self._push_args(frames, active, begin)
        self._call(frames.contiguous(), self._dims[2], False, want_log_probs, flags, lengths)

    @torch.no_grad()
    def finish(self, tail=None, tail_lengths=None, rows=None, want_log_probs=False):
        self._check_modes()
        tail, flags, lengths = self._finish_args(tail, tail_lengths, rows)
        self._call(tail.contiguous(), self._dims[2] + 1, True, want_log_probs, flags, lengths)

    def partial(self):
        if self._beam is None:
            return (self._hyp.clone(), self._hyp_len.clone(), self._score.clone(), self._steps.clone(), self._truncated.clone())
        bm = self._beam
        best, best_len = bm.tokens[:, 0], bm.lengths[:, 0].clamp(min=0)          # (-1: a slot that never began)
        hyp = best.masked_fill(torch.arange(self.capacity, device=best.device)[None, :] >= best_len[:, None], 0)
        return (hyp, best_len, bm.scores[:, 0].clone(), self._steps.clone(), (bm.lengths >= self.capacity).any(1))

    def nbest(self):
        if self._beam is None:
            raise ValueError('StreamingRecognizer.nbest: constructed without a beam (beam=0)')
        return self._beam.nbest()

    def nbest_parts(self):
        if self._beam is None or self._beam.context is None:
            raise ValueError('StreamingRecognizer.nbest_parts: constructed without a context')
        return self._beam.parts()

    @property
    def last(self):
        return self._last

    # -------------------------------------------------------------------------------------------------------------- device side
    def _call(self, frames, S, final, want_lp, flags, lengths):
        buf = self._bufs[S]
        graph = None
        if self.fused and self.use_graph and not final:
            key = (bool(want_lp), _lib.get_math_mode(), self._stamp())
            graph = self._graphs.get(key)
            if graph is None:
                graph = self._capture(S, want_lp, buf)
                self._graphs = {key: graph}              # (one at a time: a changed weight or mode captures again)
        self._send_meta(flags, lengths)
        if not self.fused:
            self._chain_general(frames, S, final, buf)
        elif graph is not None:
            if frames.data_ptr() != self._frames.data_ptr():
                self._frames.copy_(frames)
            graph.replay()
        else:
            self._chain(frames, S, want_lp, buf)
        self._last = (buf['ali'], buf['scores'], self._n_steps) + ((buf['lp'],) if want_lp or not self.fused else ())

    def _capture(self, S, want_lp, buf):
        """The push chain as one HIP graph.  The warm-up run and the capture see every slot inactive, so they change no stream."""
        self._meta.zero_()
        return capture(lambda: self._chain(self._frames, S, want_lp, buf))[0]

    def _chain(self, frames, S, want_lp, buf):
        conv, cls = self.encoder.subsample, self.recognizer.classifier
        flags, length = self._meta[0], self._meta[1]
        ops.stream_front(frames, self._carry, length, flags, conv.weight, conv.bias, buf['y'], self._n_steps, self._h, self._c,
                         self._hyp, self._hyp_len, self._steps, self._score, self._last_label, self._truncated)
        hn, cn = self._lstm(buf['y'], S, buf)
        ops.stream_head(buf['feats'], cls.weight, cls.bias, self._n_steps, flags, hn, cn, self._h, self._c, buf['ali'], buf['scores'],
                        self._hyp, self._hyp_len, self._steps, self._score, self._last_label, self._truncated,
                        lp_out=buf['lp'] if want_lp or self._beam is not None else None)
        self._advance_beam(buf['lp'], flags)

    def _advance_beam(self, lp, flags):
        """The beam's launch on the call's log-probs [B, S, V], read in place as [S, B, V]: slot b takes its n_steps[b] steps."""
        bm = self._beam
        if bm is not None:
            bm._launch(lp.permute(1, 0, 2), self._n_steps, flags)

    def _chain_general(self, frames, S, final, buf):
        """The same call on the general operators; the merging of the collapse and the choice of the state by torch operators."""
        cls = self.recognizer.classifier
        B, _, _, F, C, L, H, V = self._dims
        flags = self._meta[0]
        hn, cn, n, live, act, beg, fin = self._encode_general(frames, S, final, buf)
        self._hyp.masked_fill_(beg[:, None], 0)
        self._hyp_len.masked_fill_(beg, 0)
        self._steps.masked_fill_(beg, 0)
        self._score.masked_fill_(beg, 0.0)
        self._last_label.masked_fill_(beg, -1)
        self._truncated.masked_fill_(beg, False)
        feats = buf['feats']
        logits = ops.gemm(feats.view(B * S, H), cls.weight, True, True, B * S, V, H, bias1=cls.bias)
        lp = ops.log_softmax_fwd(logits).view(B, S, V)
        ali, scores, _, _ = ops.ctc_greedy(lp)
        prev = torch.cat([self._last_label[:, None].to(torch.int64), ali[:, :-1]], dim=1)
        keep = (ali != prev) & (ali != 0) & live
        pos = self._hyp_len[:, None] + keep.cumsum(1) - 1
        fits = keep & (pos < self.capacity)
        ext = torch.cat([self._hyp, self._hyp.new_zeros(B, 1)], dim=1)                          # a spare column takes what is not kept
        ext.scatter_(1, torch.where(fits, pos, torch.full_like(pos, self.capacity)), ali)
        self._hyp.copy_(ext[:, :self.capacity])
        self._truncated.logical_or_((keep & ~fits).any(1))
        self._hyp_len.copy_((self._hyp_len + keep.sum(1)).clamp(max=self.capacity))
        last = ali.gather(1, (n.to(torch.int64) - 1).clamp(min=0)[:, None])[:, 0].to(torch.int32)
        self._last_label.copy_(torch.where(n > 0, last, self._last_label))
        for s in range(S):                                                                      # in step order
            self._score.add_(torch.where(live[:, s], scores[:, s], torch.zeros_like(self._score)))
        self._steps.add_(n.to(torch.int64))
        self._commit_general(hn, cn, n, act, fin)
        buf['ali'].copy_(ali.masked_fill(~live, 0))
        buf['scores'].copy_(scores.masked_fill(~live, 0.0))
        buf['lp'].copy_(lp.masked_fill(~live[:, :, None], 0.0))
        self._advance_beam(buf['lp'], flags)


class StreamingTransducer(_ChunkedStreams):
    """``max_streams`` slots of streaming greedy transducer recognition over ``encoder`` (an ``rnn.Encoder``) and ``head`` (a
    ``recognizer.Transducer``), both in eval mode.  ``push`` / ``finish`` take what ``StreamingRecognizer``'s take, with
    the same slot states and argument checks; every buffer is allocated here, once.

    A call is ``halo_stream_front``, the persistent LSTM from the carried (h, c), ``halo_stream_logits`` (the classifier product, no
    softmax, and the commit of the LSTM state) and ``transducer.GreedyStream.advance`` on the call's logits with n_frames = n_steps:
    the head's frame-synchronous search needs nothing beyond the current frame, so a slot's hypothesis after every call is the
    whole-utterance greedy search of the steps it has been sent.  ``finish`` consumes the final steps, the convolution's right padding
    included, and closes the slot, which stays readable until it begins again.  ``HALO_STREAM_FUSED=0`` runs the encoder side on the
    general operators; the search's own path follows ``GreedyStream``'s rule (HALO_RNNT_FUSED, the math mode).

    partial(): copies of (hyp [B, capacity] int64, -1 past a slot's length; hyp_len [B] int64; scores [B] fp32: the sum of the
        log-probabilities of every move; steps [B] int64: encoder steps so far; truncated [B] bool: the slot emitted ``capacity`` symbols
        and ignores its later steps).
    last: (logits [B, S, V] fp32, zeros past a row's n_steps; n_steps [B] int32) of the latest call -- this object's buffers.

    ``beam=W`` (None reads HALO_STREAM_RNNT_BEAM, 0 .. 16, default 0: this object as described, launch for launch) puts a
    ``transducer.BeamStream`` in place of the greedy search: ``push`` marks no slot final, ``finish`` marks its rows
    final, ``partial()`` returns the best hypothesis with ``truncated`` all False, and ``nbest()`` the n-best lists.

    There is no graph replay: the number of rounds of a call depends on the data.  Unlike ``StreamingRecognizer``, a call waits for the
    device wherever ``GreedyStream`` reads its live word (every ``transducer.SYNC_EVERY`` rounds)."""

    def __init__(self, encoder, head, max_streams, chunk_frames=16, capacity=256, max_symbols_per_frame=10, beam=None):
        from .transducer import BEAM_MAX, BeamStream, GreedyStream
        if encoder.training or head.training:
            raise ValueError('StreamingTransducer: put the encoder and the head in eval mode')
        conv = encoder.subsample
        self._check_geometry('StreamingTransducer', conv, chunk_frames, max_streams, capacity)
        self.encoder, self.head = encoder, head
        self.max_streams, self.chunk_frames, self.capacity = int(max_streams), int(chunk_frames), int(capacity)
        self.fused = os.environ.get('HALO_STREAM_FUSED', '1') != '0'
        dev = conv.weight.device
        if dev.type != 'cuda':
            raise _lib.HaloError('haloop_amd.streaming.StreamingTransducer runs on the HIP device only (no CPU path)')
        _lib.lend_scratch(device=dev)
        B, Tc, S = self.max_streams, self.chunk_frames, self.chunk_frames // 4
        F, C = conv.in_channels, conv.out_channels
        L, H, V = encoder.lstm.num_layers, encoder.lstm.hidden_size, head.classifier.out_features
        if head.classifier.in_features != H:
            raise ValueError(f'StreamingTransducer: the head takes {head.classifier.in_features} features, the encoder gives {H}')
        self._dims = (B, Tc, S, F, C, L, H, V)
        f32 = dict(device=dev, dtype=torch.float32)
        self._carry = torch.zeros(B, 3, F, **f32)
        self._h, self._c = torch.zeros(L, B, H, **f32), torch.zeros(L, B, H, **f32)
        self._steps = torch.zeros(B, device=dev, dtype=torch.int64)
        self._n_steps = torch.zeros(B, device=dev, dtype=torch.int32)
        # halo_stream_front resets a CTC hypothesis of the slots that begin: small buffers of this object's own take that
        self._ctc = (torch.zeros(B, 1, device=dev, dtype=torch.int64), torch.zeros(B, device=dev, dtype=torch.int64), torch.zeros(B, **f32),
                     torch.zeros(B, device=dev, dtype=torch.int32), torch.zeros(B, device=dev, dtype=torch.bool))   # hyp, hyp_len, score, last_label, truncated
        self._init_host(dev)
        self._bufs = {}
        for s in (S, S + 1):
            self._bufs[s] = dict(y=torch.zeros(s, B, C, **f32), feats=torch.zeros(B, s, H, **f32), logits=torch.zeros(B, s, V, **f32),
                                 reserve=ops.lstm_reserve(s, B, C, H, L, dev))
        if beam is None:
            beam = os.environ.get('HALO_STREAM_RNNT_BEAM', '0')
        self.beam = int(beam)
        if self.beam < 0 or self.beam > BEAM_MAX:
            raise ValueError(f'StreamingTransducer: beam {self.beam} outside 0 .. {BEAM_MAX}')
        if self.beam:
            self.search = BeamStream(head, B, self.capacity, self.beam, max_chunk=S + 1)
        else:
            self.search = GreedyStream(head, B, self.capacity, max_symbols_per_frame)
        self._last = None

    def _check_modes(self):
        if self.encoder.training or self.head.training:
            raise ValueError('StreamingTransducer: put the encoder and the head in eval mode')

    @torch.no_grad()
    def push(self, frames, active=None, begin=None):
        self._check_modes()
        flags, lengths = self._push_args(frames, active, begin)
        self._call(frames.contiguous(), self._dims[2], False, flags, lengths)

    @torch.no_grad()
    def finish(self, tail=None, tail_lengths=None, rows=None):
        self._check_modes()
        tail, flags, lengths = self._finish_args(tail, tail_lengths, rows)
        self._call(tail.contiguous(), self._dims[2] + 1, True, flags, lengths)

    def partial(self):
        if self.beam:
            tokens, lengths, scores, counts = self.search.nbest()
            none = counts == 0                                           # a slot that never began: the empty hypothesis, as greedy
            return (tokens[:, 0], lengths[:, 0].clamp(min=0), scores[:, 0].masked_fill(none, 0.0), self._steps.clone(),
                    torch.zeros_like(none))
        tokens, lengths, _, scores, truncated = self.search.result()
        return tokens, lengths, scores, self._steps.clone(), truncated

    def nbest(self):
        """``transducer.BeamStream.nbest`` of every slot (beam >= 1): a closed slot's finals, an open slot's stalled beam."""
        if not self.beam:
            raise ValueError('StreamingTransducer.nbest: built without a beam (beam=W or HALO_STREAM_RNNT_BEAM)')
        return self.search.nbest()

    @property
    def last(self):
        return self._last

    def _call(self, frames, S, final, flags, lengths):
        buf = self._bufs[S]
        self._send_meta(flags, lengths)
        dflags, length = self._meta[0], self._meta[1]
        conv, cls = self.encoder.subsample, self.head.classifier
        if self.fused:
            ops.stream_front(frames, self._carry, length, dflags, conv.weight, conv.bias, buf['y'], self._n_steps, self._h, self._c,
                             self._ctc[0], self._ctc[1], self._steps, self._ctc[2], self._ctc[3], self._ctc[4])
            hn, cn = self._lstm(buf['y'], S, buf)
            ops.stream_logits(buf['feats'], cls.weight, cls.bias, buf['logits'], self._n_steps, dflags, hn, cn, self._h, self._c, self._steps)
        else:
            B, H, V = self._dims[0], self._dims[6], self._dims[7]
            hn, cn, n, live, act, beg, fin = self._encode_general(frames, S, final, buf)
            logits = ops.gemm(buf['feats'].view(B * S, H), cls.weight, True, True, B * S, V, H, bias1=cls.bias).view(B, S, V)
            buf['logits'].copy_(logits.masked_fill(~live[:, :, None], 0.0))
            self._steps.masked_fill_(beg, 0)
            self._steps.add_(n.to(torch.int64))
            self._commit_general(hn, cn, n, act, fin)
        self._last = (buf['logits'], self._n_steps)
        self.search._advance(buf['logits'], self._n_steps, dflags, any(f & STREAM_BEGIN for f in flags))
