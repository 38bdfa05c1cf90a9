"""Drop-in for the transducer lattice of ha/transducer.py ([Graves12] Sequence Transduction with Recurrent Neural Networks) on the
HIP lattice kernels (csrc/lattice.hip).

``transducer_forward_score(joint, targets, joint_lengths, target_lengths)`` = ha/transducer.py:175-207: joint [N, T, U+1, K]
log-probabilities ((f + g).log_softmax(-1)), symbol 0 blank, targets [N, U] -> losses [N]; differentiable w.r.t. ``joint`` (a backward
kernel that carries the cell posteriors through the local arc weights, where the reference uses autograd through its log-space scan).  ``transducer_forward_score4(joint, targets)``
(:145-172) is the single-sequence form.  Any T: the reference pads its scan to 2 ** round(log2(T)) (:194) and raises when that is
smaller than T; the recurrence it defines is computed here cell by cell along the anti-diagonals.  The probability-domain study
versions (transducer_forward_score1-3, :10-142) are not built.

``transducer_loss(f, g, targets, f_lengths, target_lengths)`` is the same score for the additive joint f[:, :, None] + g[:, None] of
``recognizer.Transducer``, taken from its two factors (what the reference's live branch gets from torchaudio's ``rnnt_loss(...,
fused_log_softmax=True)``, ha/recognizer.py:121-126): csrc/rnnt_loss.hip computes every cell's log-sum-exp and its blank / label
log-probabilities, the lattice kernels run on those, and the backward rebuilds the softmax for df and dg -- no [N, T, U+1, V] tensor in
either direction.

``transducer_viterbi(joint, ...)`` and ``transducer_align(f, g, ...)`` are forced alignment on the same two routes (the dense joint;
the two factors, no [N, T, U+1, V] tensor): the best path of the lattice and the frame at which it emits every target token
(csrc/viterbi.hip).  The reference has neither.

``nbest_risk(losses, errors)`` is the minimum-word-error-rate objective over an n-best list: the expected number of errors under the
hypotheses' renormalised posterior, less its plain mean (csrc/edit_distance.hip).  The reference has no such objective.

``GreedyDecoder`` is greedy transducer search ([Graves12]) for ``recognizer.Transducer``, which the reference leaves unbuilt
(ha/recognizer.py:92-93): per row, with F = classifier(features) and g the prediction network's logits for the symbols emitted so far
(the zero prefix of training first), take k = argmax log_softmax(F[n, t] + g) (lowest index on ties; blank forced once
``max_symbols_per_frame`` symbols were emitted at frame t); blank moves to the next frame, anything else is emitted and advances the
prediction network.  The score is the sum of the log-probabilities of every move.  The fused path (csrc/rnnt_decode.hip) costs
``1 + num_layers + 1`` launches per emitted symbol and none per blank frame; the general path runs the same search node by node on
``rnn.Decoder.forward`` at T = 1 with torch's log_softmax.

``GreedyStream`` is the same greedy search carried across calls: logits that arrive in chunks, every row's search entered from the
state its previous chunk left and left into it, so a row always holds ``GreedyDecoder.decode`` of its frames so far
(csrc/rnnt_decode.hip: the open launch, the carried advance, cells with a row mask).

``BeamDecoder`` is beam search for the same head: alignment-length synchronous decoding with exact merging ([Saon20]), n-best lists whose
scores sum the alignment paths of a hypothesis, on ``num_layers + 3`` launches per alignment step (csrc/rnnt_beam.hip).

``BeamStream`` is that beam search carried across calls: a row executes an alignment step only when every frame the step reads has
arrived and no blank extension could be complete, so after its final call a row holds ``BeamDecoder.decode`` of its whole utterance
(csrc/rnnt_beam.hip: the open launch and the carried instantiation of the step).
"""
import torch

from . import _lib, _slots, functional as HF, ops
from .rnn import lstm_param_list

SYNC_EVERY = 16          # GreedyDecoder.decode reads the live-row counter every this many advances
STREAM_BEAM_SYNC_EVERY = 4   # BeamStream.advance: after its first S rounds a call reads the live word every this many rounds


class _Transducer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, joint, targets, joint_lengths, target_lengths):
        j = joint.detach().float().contiguous()
        losses, workspace = ops.transducer_fwd(j, targets, joint_lengths, target_lengths, keep=joint.requires_grad)
        ctx.saved = (j, targets, joint_lengths, target_lengths, workspace, losses)
        return losses.clone()

    @staticmethod
    def backward(ctx, grad_losses):
        j, targets, joint_lengths, target_lengths, workspace, losses = ctx.saved
        return ops.transducer_bwd(j, targets, joint_lengths, target_lengths, workspace, losses, grad_losses.float().contiguous()), None, None, None


def transducer_forward_score(joint, targets, joint_lengths, target_lengths):
    """(N, T, U+1, K), (N, U), (N,), (N,) -> losses (N,)  (ha/transducer.py:175-207)."""
    if not joint.is_cuda:
        raise _lib.HaloError('haloop_amd.transducer.transducer_forward_score runs on the HIP device only (no CPU path)')
    dev = joint.device
    N, T, U1, K = joint.shape
    if targets.shape != (N, U1 - 1):
        raise ValueError(f'targets must be [N, U] = [{N}, {U1 - 1}], got {tuple(targets.shape)}')
    jl = joint_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    return _Transducer.apply(joint, targets.to(device=dev, dtype=torch.int64).contiguous(), jl, tl)


def transducer_forward_score4(joint, targets):
    """(T, U+1, K), (U,) -> scalar loss  (ha/transducer.py:145-172)."""
    T, U1, _ = joint.shape
    dev = joint.device
    return transducer_forward_score(joint[None], targets[None], torch.tensor([T], device=dev), torch.tensor([U1 - 1], device=dev))[0]


class _TransducerLoss(torch.autograd.Function):
    """csrc/rnnt_loss.hip around the lattice kernels: keeps f, g, lse [N, T, U+1], lp2 [N, T, U+1, 2], alpha and the losses."""

    @staticmethod
    def forward(ctx, f, g, targets, f_lengths, target_lengths):
        fd, gd = _rows_fp32(f.detach()), _rows_fp32(g.detach())
        lse, lp2 = ops.rnnt_joint_fwd(fd, gd, targets, f_lengths, target_lengths)
        ones = torch.ones_like(targets)                # lp2 is a joint with K = 2: blank 0, the cell's own label 1
        keep = f.requires_grad or g.requires_grad
        losses, workspace = ops.transducer_fwd(lp2, ones, f_lengths, target_lengths, keep=keep, checked=True)
        ctx.saved = (fd, gd, targets, ones, f_lengths, target_lengths, lse, lp2, workspace, losses) if keep else None
        return losses.clone()

    @staticmethod
    def backward(ctx, grad_losses):
        fd, gd, targets, ones, f_lengths, target_lengths, lse, lp2, workspace, losses = ctx.saved
        d = ops.transducer_bwd(lp2, ones, f_lengths, target_lengths, workspace, losses, grad_losses.float().contiguous())
        df, dg = ops.rnnt_joint_bwd(fd, gd, targets, f_lengths, target_lengths, lse, d)
        return df, dg, None, None, None


def _rows_fp32(x):
    """fp32 rows with unit stride along the last dimension and rows that do not overlap; anything else (an expanded view, say) is copied."""
    x = x.float()
    return x if (x.shape[2] == 1 or x.stride(2) == 1) and _disjoint_rows(x) else x.contiguous()


def _disjoint_rows(x):
    """Rows V apart or more, nested batch-major (contiguous; [:, :, :V] of a wider buffer) or row-major (a transposed time-major tensor)."""
    N, R, V = x.shape
    ns, rs = x.stride(0), x.stride(1)
    if (N > 1 and ns < V) or (R > 1 and rs < V):
        return False
    return N == 1 or R == 1 or ns >= (R - 1) * rs + V or rs >= (N - 1) * ns + V


def transducer_loss(f, g, targets, f_lengths, target_lengths):
    """f [N, T, V] transcription logits, g [N, U+1, V] prediction-network logits, targets [N, U], lengths [N] -> losses [N] =
    transducer_forward_score((f[:, :, None] + g[:, None]).log_softmax(-1), targets, f_lengths, target_lengths), differentiable w.r.t. f
    and g, without the [N, T, U+1, V] joint, its log-softmax or their gradients: every buffer is O(N T (U+1)) or the size of f / g.
    f and g may be strided views with a contiguous last dimension (a slice of a wider buffer; the transposed time-major rows of
    ``Decoder.forward_batch_first``): they are read, and g's gradient written, in place."""
    if not f.is_cuda or not g.is_cuda:
        raise _lib.HaloError('haloop_amd.transducer.transducer_loss runs on the HIP device only (no CPU path)')
    dev = f.device
    if f.dim() != 3 or g.dim() != 3 or f.shape[0] != g.shape[0] or f.shape[2] != g.shape[2]:
        raise ValueError(f'transducer_loss: f must be [N, T, V] and g [N, U+1, V], got {tuple(f.shape)} and {tuple(g.shape)}')
    N, U1 = g.shape[0], g.shape[1]
    if tuple(targets.shape) != (N, U1 - 1):
        raise ValueError(f'targets must be [N, U] = [{N}, {U1 - 1}], got {tuple(targets.shape)}')
    fl = f_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    return _TransducerLoss.apply(f, g, targets.to(device=dev, dtype=torch.int64).contiguous(), fl, tl)


def transducer_viterbi(joint, targets, joint_lengths, target_lengths):
    """Forced alignment on a dense joint: joint [N, T, U+1, K] log-probabilities ((f + g).log_softmax(-1)), targets [N, U],
    joint_lengths [N] (0: an empty row), target_lengths [N] -> (scores [N] float32: the log-probability of the best alignment, -inf for an
    empty row; frames [N, U] int32: the frame at which every target token is emitted -- ``GreedyDecoder``'s ``frames`` -- and -1 past the
    row's target length).  Among equally good paths the blank arc is taken first (include/halo.h).  Not differentiable."""
    if not joint.is_cuda:
        raise _lib.HaloError('haloop_amd.transducer.transducer_viterbi runs on the HIP device only (no CPU path)')
    dev = joint.device
    if joint.dim() != 4:
        raise ValueError(f'transducer_viterbi: joint must be [N, T, U+1, K], got {tuple(joint.shape)}')
    N, T, U1, K = joint.shape
    if tuple(targets.shape) != (N, U1 - 1):
        raise ValueError(f'targets must be [N, U] = [{N}, {U1 - 1}], got {tuple(targets.shape)}')
    jl = joint_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    return ops.transducer_viterbi(joint.detach().float().contiguous(), targets.to(device=dev, dtype=torch.int64).contiguous(), jl, tl)


def transducer_align(f, g, targets, f_lengths, target_lengths):
    """``transducer_viterbi((f[:, :, None] + g[:, None]).log_softmax(-1), ...)`` from the two factors of the additive joint, f [N, T, V]
    and g [N, U+1, V], under ``transducer_loss``'s input rules (strided views with a contiguous last dimension are read in place):
    csrc/rnnt_loss.hip computes every cell's blank / label log-probabilities, the Viterbi launch runs on those -- no [N, T, U+1, V]
    tensor.  -> (scores [N], frames [N, U])."""
    if not f.is_cuda or not g.is_cuda:
        raise _lib.HaloError('haloop_amd.transducer.transducer_align runs on the HIP device only (no CPU path)')
    dev = f.device
    if f.dim() != 3 or g.dim() != 3 or f.shape[0] != g.shape[0] or f.shape[2] != g.shape[2]:
        raise ValueError(f'transducer_align: f must be [N, T, V] and g [N, U+1, V], got {tuple(f.shape)} and {tuple(g.shape)}')
    N, U1 = g.shape[0], g.shape[1]
    if tuple(targets.shape) != (N, U1 - 1):
        raise ValueError(f'targets must be [N, U] = [{N}, {U1 - 1}], got {tuple(targets.shape)}')
    fl = f_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    targets = targets.to(device=dev, dtype=torch.int64).contiguous()
    _, lp2 = ops.rnnt_joint_fwd(_rows_fp32(f.detach()), _rows_fp32(g.detach()), targets, fl, tl, min_length=0)
    return ops.transducer_viterbi(lp2, torch.ones_like(targets), fl, tl, checked=True)   # lp2 is a joint with K = 2: the cell's label is 1


class _NbestRisk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, losses, errors):
        l = losses.detach().float().contiguous()
        ctx.saved = (l, errors)
        return ops.nbest_risk_fwd(l, errors)

    @staticmethod
    def backward(ctx, grad_risk):
        l, errors = ctx.saved
        return ops.nbest_risk_bwd(l, errors, grad_risk.float().contiguous()), None


def nbest_risk(losses, errors):
    """The minimum-word-error-rate risk of an n-best list ([Prabhavalkar18], [Guo20]; csrc/edit_distance.hip): losses
    [N, W] = -log P(hypothesis | x) (``transducer_loss`` on the N * W hypotheses), errors [N, W] integers (``wer.edit_distance``; < 0: an
    absent hypothesis), W <= ``BEAM_MAX`` -> risk [N] = sum_w p_w err_w - mean_w err_w with p = softmax(-losses) over the present
    hypotheses of a row (0 for a row without one).  Differentiable w.r.t. ``losses``: d risk / d losses_w = -p_w (err_w - sum_v p_v err_v),
    0 for an absent hypothesis; the mean is a baseline without a gradient.  fp32, bit-reproducible."""
    if not losses.is_cuda or not errors.is_cuda:
        raise _lib.HaloError('haloop_amd.transducer.nbest_risk runs on the HIP device only (no CPU path)')
    if losses.dim() != 2 or errors.shape != losses.shape:
        raise ValueError(f'nbest_risk: losses and errors must both be [N, W], got {tuple(losses.shape)} and {tuple(errors.shape)}')
    return _NbestRisk.apply(losses, errors.to(device=losses.device, dtype=torch.int32).contiguous())


class _HeadDecoder:
    """What the decoders of a ``recognizer.Transducer`` head (``self.head``) share; ``self._net``: its prediction network as the fused
    launches read it (``_slots.Network``: the decode images and the network's part of the fused rule)."""

    @property
    def fused(self):
        """Whether the fused launches are in use (decided from the head, the math mode and HALO_RNNT_FUSED as they are now)."""
        return not self.head.training and self._net.fused

    def _lm_step(self, N, p, layers, head_image, mask=None):
        """The prediction network on the input rows of copy p -> g (``GreedyDecoder`` and ``GreedyStream``: both keep ``_xh`` [2, L, rows,
        2 H], ``_c``, ``_top`` and ``_g``): every layer's cell launch reads copy p of its [x | h_prev] rows and writes h to copy 1 - p
        (its own next h_prev) and to copy p of the layer above (that layer's x).  ``mask`` (int32 [>= N] on the device): a row with 0
        sits the step out -- c kept, h_prev copied to copy 1 - p, its ``_top`` row untouched, so out_layer reproduces its g."""
        lm = self.head.lm
        H, L, w = lm.hidden_dim, lm.num_layers, lstm_param_list(lm.rnn)
        for l in range(L):
            h_up = self._xh[p, l + 1, :N, :H] if l + 1 < L else self._top[:N]
            ops.rnnt_lstm_cell(self._xh[p, l, :N], layers[l], w[4 * l + 2], w[4 * l + 3], self._c[l, :N], self._xh[1 - p, l, :N, H:], h_up,
                               row_mask=mask)
        ops.decode_linear(self._top[:N], head_image, lm.num_classes, self._g[:N])

    def _check(self, features, input_lengths):
        name = type(self).__name__
        if features.dim() != 3 or features.shape[1] < 1:
            raise ValueError(f'{name}: features must be [N, T, feat_dim] with T >= 1')
        N = features.shape[0]
        if N < 1 or N > self.max_batch:
            raise ValueError(f'{name}: batch {N} outside 1 .. max_batch = {self.max_batch}')
        if input_lengths.shape != (N,):
            raise ValueError(f'{name}: input_lengths must be [{N}]')
        if not features.is_cuda:
            raise _lib.HaloError(f'haloop_amd.transducer.{name} runs on the HIP device only (no CPU path)')
        if self.head.training:
            raise NotImplementedError(f'{name} is an inference path: put the head in eval mode')


class GreedyDecoder(_HeadDecoder):
    """Greedy search for a ``recognizer.Transducer`` head with preallocated row state and buffers for ``max_batch`` rows and
    ``capacity`` symbols per row.  ``max_symbols_per_frame`` bounds the symbols emitted at one frame (a guard that a trained model does
    not meet; it bounds an untrained one)."""

    def __init__(self, head, max_batch, capacity, max_symbols_per_frame=10):
        self.head, self._net = head, _slots.Network(head.lm)
        self.max_batch, self.capacity, self.max_symbols = int(max_batch), int(capacity), int(max_symbols_per_frame)
        if self.max_batch < 1 or self.capacity < 1 or self.max_symbols < 1:
            raise ValueError('GreedyDecoder: need max_batch >= 1, capacity >= 1 and max_symbols_per_frame >= 1')
        lm = head.lm
        E, H, L, V = lm.embedding.weight.shape[1], lm.hidden_dim, lm.num_layers, lm.num_classes
        dev = lm.embedding.weight.device
        mb = self.max_batch
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            self._state = torch.zeros(5, mb, device=dev, dtype=torch.int32)      # t | u | here | done | truncated, one word per row
            self._scores = torch.zeros(mb, device=dev, dtype=torch.float32)
            self._tokens = torch.zeros(mb, self.capacity, device=dev, dtype=torch.int64)
            self._frames = torch.zeros(mb, self.capacity, device=dev, dtype=torch.int64)
            self._live = torch.zeros(self.capacity, device=dev, dtype=torch.int32)   # one word per advance: rows still live after it
            if E == H:
                # [x | h_prev] rows of every layer, in two copies used alternately: a cell launch reads one and writes the other's h
                self._xh = torch.zeros(2, L, mb, 2 * H, device=dev, dtype=torch.float32)
                self._c = torch.zeros(L, mb, H, device=dev, dtype=torch.float32)
                self._top = torch.zeros(mb, H, device=dev, dtype=torch.float32)
                self._g = torch.zeros(mb, V, device=dev, dtype=torch.float32)
        self.iterations = 0    # of the last decode: advances (fused path) or lattice nodes visited in lockstep (general path)

    def decode(self, features, input_lengths, capacity=None):
        """features [N, T, feat_dim], input_lengths [N] (clipped to T) -> (tokens [N, capacity] int64, lengths [N] int64, frames
        [N, capacity] int64, scores [N] float32, truncated [N] bool); entries past a row's length are -1.  ``capacity``: search with
        room for fewer symbols than the buffers hold (default: all of them)."""
        self._check(features, input_lengths)
        cap = self.capacity if capacity is None else int(capacity)
        if cap < 1 or cap > self.capacity:
            raise ValueError(f'GreedyDecoder: capacity {cap} outside 1 .. {self.capacity}')
        with torch.no_grad():
            N, T, _ = features.shape
            dev = features.device
            cl = self.head.classifier
            f = HF.linear(features.float(), cl.weight, cl.bias).contiguous()                   # [N, T, V]
            il = input_lengths.to(device=dev, dtype=torch.int32).clamp(0, T).contiguous()
            self._state.zero_(); self._scores.zero_(); self._tokens.fill_(-1); self._frames.fill_(-1)
            (self._decode_fused if self.fused else self._decode_general)(f, il, N, cap)
            st = self._state
            return (self._tokens[:N, :cap].clone(), st[1, :N].long(), self._frames[:N, :cap].clone(), self._scores[:N].clone(),
                    st[4, :N] != 0)

    # ---- the fused path: 1 + num_layers + 1 launches per emitted symbol ------------------------------------------------------------
    def _decode_fused(self, f, il, N, cap):
        lm = self.head.lm
        layers, head_image = self._net.images()
        wte, E = lm.embedding.weight, lm.embedding.weight.shape[1]
        self._xh.zero_(); self._c.zero_(); self._live.zero_()
        self._xh[0, 0, :N, :E] = wte[0]                       # the zero prefix of training (recognizer.py:107)
        p = 0
        self._lm_step(N, p, layers, head_image)
        for it in range(cap):                                  # a live row emits once per advance: after `cap` of them none is live
            ops.rnnt_advance(f, self._g[:N], lm.out_layer.bias, il, self._state, self._scores, self._tokens[:N, :cap], self._frames[:N, :cap],
                             self.max_symbols, wte, self._xh[1 - p, 0, :N], self._live[it:])
            if it == cap - 1 or ((it + 1) % SYNC_EVERY == 0 and int(self._live[it].item()) == 0):
                break
            p = 1 - p
            self._lm_step(N, p, layers, head_image)
        self.iterations = it + 1
        if int(self._live[it].item()) != 0:
            raise _lib.HaloError('GreedyDecoder: rows still live after capacity advances')

    # ---- the general path: the same search node by node on rnn.Decoder.forward at T = 1 ------------------------------------------------
    def _decode_general(self, f, il, N, cap):
        lm = self.head.lm
        dev, V = f.device, f.shape[2]
        rows, cols = torch.arange(N, device=dev), torch.arange(V, device=dev)
        t, u, here = (torch.zeros(N, device=dev, dtype=torch.int64) for _ in range(3))
        il = il.long()
        done = il <= 0
        scores = torch.zeros(N, device=dev, dtype=torch.float32)
        g, state = lm.forward(torch.zeros(1, N, device=dev, dtype=torch.int64), lm.init_hidden(N))
        self.iterations = 0
        while not bool(done.all().item()):                      # one host read per lattice node
            self.iterations += 1
            lp = torch.log_softmax(f[rows, t.clamp(max=f.shape[1] - 1)] + g, -1)
            top = lp.max(-1).values
            k = torch.where(lp == top[:, None], cols, V).min(-1).values            # lowest index among equal maxima
            k = torch.where(here == self.max_symbols, torch.zeros_like(k), k)
            live = ~done
            scores += torch.where(live, lp[rows, k], torch.zeros_like(top))
            blank, emit = live & (k == 0), live & (k != 0)
            e = emit.nonzero().view(-1)
            self._tokens[e, u[e]] = k[e]
            self._frames[e, u[e]] = t[e]
            t, here, u = t + blank.long(), torch.where(blank, torch.zeros_like(here), here + emit.long()), u + emit.long()
            if e.numel():
                g1, (h1, c1) = lm.forward(torch.where(emit, k, torch.zeros_like(k)).view(1, N), state)
                g = torch.where(emit[:, None], g1, g)
                state = (torch.where(emit[None, :, None], h1, state[0]), torch.where(emit[None, :, None], c1, state[1]))
            done = done | (t >= il) | (u >= cap)
        st = self._state
        st[0, :N], st[1, :N], st[2, :N], st[3, :N], st[4, :N] = t.int(), u.int(), here.int(), 1, (u >= cap).int()
        self._scores[:N] = scores


class GreedyStream(_HeadDecoder):
    """``GreedyDecoder``'s search carried across calls: the transcription logits of ``max_rows`` rows arrive in chunks
    and every row's search goes on where its previous chunk ended, so after every call a row holds what ``GreedyDecoder.decode`` returns
    on the frames the row has been sent so far -- on the fused path bit for bit, scores included -- at the cost of the new frames alone.
    The logits may be of any origin (``streaming.StreamingTransducer`` feeds its encoder's).  Every buffer is allocated here, once.

    advance(f [B, S, V], n_frames=None, begin=None): B <= max_rows; f a float32 HIP tensor with a unit class stride (a slice of a wider
        buffer is read in place); row b takes its first clamp(n_frames[b], 0, S) frames (a device int32 tensor [B]; None: S).  ``begin``
        (host-side: a sequence of B bools or a CPU bool tensor; None: no row) starts a row from the empty hypothesis, whatever it held;
        a row must begin before its first frames.  A row without frames, a truncated row and the rows from B on keep their state, their
        outputs and g bit for bit.  A row that reaches ``capacity`` symbols is truncated until it begins again: its later frames are
        ignored.  Returns views of (tokens [B, capacity] int64, lengths [B] int64, frames [B, capacity] int64 -- counted from the row's
        begin --, scores [B] float32, truncated [B] bool) in ``GreedyDecoder.decode``'s format; the next call overwrites them.
    result(): copies of the same five for all ``max_rows`` rows.
    rounds: the advances of the last call.

    One call is the open launch, one masked step of the prediction network if a row begins, and rounds of (advance, masked cells,
    out_layer) until no row is live.  As in ``GreedyDecoder`` the live word is read every ``SYNC_EVERY`` rounds, so a call waits for the
    device there, and the rounds past the last live one change nothing.  A row emits at most ``max_symbols_per_frame`` symbols per frame
    and ``capacity`` in all and needs one more round to run out of frames: more than min(S * max_symbols_per_frame, capacity) + 1 rounds
    raise ``HaloError``.  The general path (f32 mode, HALO_RNNT_FUSED=0, a head the fused launches do not take) carries the same search
    on ``rnn.Decoder.forward`` at T = 1.  The path is chosen when a row begins; do not change it in the middle of a stream."""

    def __init__(self, head, max_rows, capacity, max_symbols_per_frame=10):
        self.head, self._net = head, _slots.Network(head.lm)
        self.max_rows, self.capacity, self.max_symbols = int(max_rows), int(capacity), int(max_symbols_per_frame)
        if self.max_rows < 1 or self.capacity < 1 or self.max_symbols < 1:
            raise ValueError('GreedyStream: need max_rows >= 1, capacity >= 1 and max_symbols_per_frame >= 1')
        lm = head.lm
        E, H, L, V = lm.embedding.weight.shape[1], lm.hidden_dim, lm.num_layers, lm.num_classes
        dev = lm.embedding.weight.device
        if dev.type != 'cuda':
            raise _lib.HaloError('haloop_amd.transducer.GreedyStream runs on the HIP device only (no CPU path)')
        mb = self.max_rows
        i32 = dict(device=dev, dtype=torch.int32)
        with torch.inference_mode(False):
            self._state = torch.zeros(5, mb, **i32)                # t | u | here | done | truncated; t counts the stream's frames
            self._state[3].fill_(1)
            self._pos, self._mask = torch.zeros(mb, **i32), torch.zeros(mb, **i32)
            self._nf, self._flags = torch.zeros(mb, **i32), torch.zeros(mb, **i32)
            self._scores = torch.zeros(mb, device=dev, dtype=torch.float32)
            self._tokens = torch.full((mb, self.capacity), -1, device=dev, dtype=torch.int64)
            self._frames = torch.full((mb, self.capacity), -1, device=dev, dtype=torch.int64)
            self._live = torch.zeros(self.capacity + 1, **i32)     # one word per advance of a call
            self._g = torch.zeros(mb, V, device=dev, dtype=torch.float32)
            if E == H:
                self._xh = torch.zeros(2, L, mb, 2 * H, device=dev, dtype=torch.float32)
                self._c = torch.zeros(L, mb, H, device=dev, dtype=torch.float32)
                self._top = torch.zeros(mb, H, device=dev, dtype=torch.float32)
            self._gh = torch.zeros(L, mb, H, device=dev, dtype=torch.float32)      # the general path's state
            self._gc = torch.zeros(L, mb, H, device=dev, dtype=torch.float32)
        self._cur = 0          # the [x | h] copy that holds every row's h: the one the next step reads.  Carried across calls.
        self.rounds = 0

    def advance(self, f, n_frames=None, begin=None):
        mb = self.max_rows
        V = self.head.lm.num_classes
        if not torch.is_tensor(f) or f.dim() != 3 or not 1 <= f.shape[0] <= mb or f.shape[1] < 1 or f.shape[2] != V or f.dtype != torch.float32:
            raise ValueError(f'GreedyStream.advance: f must be a float32 tensor [1 .. {mb}, S >= 1, {V}]')
        B, S = f.shape[0], f.shape[1]
        if n_frames is not None and (not torch.is_tensor(n_frames) or tuple(n_frames.shape) != (B,) or n_frames.dtype != torch.int32):
            raise ValueError(f'GreedyStream.advance: n_frames must be an int32 tensor [{B}]')
        if not f.is_cuda or (n_frames is not None and not n_frames.is_cuda):
            raise _lib.HaloError('haloop_amd.transducer.GreedyStream runs on the HIP device only (no CPU path)')
        if self.head.training:
            raise NotImplementedError('GreedyStream is an inference path: put the head in eval mode')
        if begin is not None:
            if torch.is_tensor(begin):
                if begin.is_cuda:
                    raise ValueError('GreedyStream.advance: begin is host-side (a sequence of bools or a CPU bool tensor)')
                begin = begin.tolist()
            begin = [bool(e) for e in begin]
            if len(begin) != B:
                raise ValueError(f'GreedyStream.advance: begin has {len(begin)} entries for {B} rows')
        with torch.no_grad():
            any_begin = begin is not None and any(begin)
            flags = None
            if any_begin:
                flags = self._flags[:B]
                flags.copy_(torch.tensor([ops.STREAM_BEGIN if e else 0 for e in begin], dtype=torch.int32))
            if n_frames is None:
                nf = self._nf[:B].fill_(S)
            else:
                nf = n_frames.detach().contiguous()
            return self._advance(f.detach(), nf, flags, any_begin)

    def _advance(self, f, nf, flags, any_begin):
        """f [B, S, V], nf int32 [B] and flags int32 [>= B] (or None) on the device; any_begin: whether a flag carries STREAM_BEGIN."""
        B, S, V = f.shape
        if f.stride(2) != 1 or f.stride(1) < V or f.stride(0) < (S - 1) * f.stride(1) + V:
            f = f.contiguous()
        (self._advance_fused if self.fused else self._advance_general)(f, nf, flags, any_begin)
        st = self._state
        return self._tokens[:B], st[1, :B].long(), self._frames[:B], self._scores[:B], st[4, :B] != 0

    def result(self):
        st = self._state
        return self._tokens.clone(), st[1].long(), self._frames.clone(), self._scores.clone(), st[4] != 0

    # ---- the fused path: per round 1 + num_layers + 1 launches over all max_rows rows, whatever B ------------------------------------
    def _advance_fused(self, f, nf, flags, any_begin):
        lm = self.head.lm
        layers, head_image = self._net.images()
        wte, E = lm.embedding.weight, lm.embedding.weight.shape[1]
        B, S = f.shape[0], f.shape[1]
        mb, cap = self.max_rows, self.capacity
        cur = self._cur
        ops.rnnt_stream_open(nf, flags, self._state, self._pos, self._mask, self._scores, self._tokens, self._frames, self._xh[cur], self._c,
                             wte, self._live)
        if any_begin:
            self._lm_step(mb, cur, layers, head_image, self._mask)
            cur = 1 - cur
        bound = min(S * self.max_symbols, cap) + 1
        try:
            for it in range(bound):
                ops.rnnt_advance_stream(f, self._g[:B], lm.out_layer.bias, nf, self._state, self._scores, self._tokens[:B], self._frames[:B],
                                        self.max_symbols, wte, self._xh[cur, 0, :B], self._live[it:], self._pos, self._mask)
                if it == bound - 1 or ((it + 1) % SYNC_EVERY == 0 and int(self._live[it].item()) == 0):
                    break
                self._lm_step(mb, cur, layers, head_image, self._mask)
                cur = 1 - cur
        finally:
            self._cur = cur
        self.rounds = it + 1
        if int(self._live[it].item()) != 0:
            raise _lib.HaloError('GreedyStream: rows still live after min(S * max_symbols_per_frame, capacity) + 1 rounds')

    # ---- the general path: the same carried search on rnn.Decoder.forward at T = 1, torch.where for the rows that sit out ----------
    def _advance_general(self, f, nf, flags, any_begin):
        lm = self.head.lm
        dev = f.device
        B, S, V = f.shape
        cap = self.capacity
        st = self._state
        g, h, c = self._g[:B], self._gh[:, :B], self._gc[:, :B]
        if any_begin:
            beg = (flags[:B] & ops.STREAM_BEGIN) != 0
            st[:, :B].masked_fill_(beg[None, :], 0)
            self._scores[:B].masked_fill_(beg, 0.0)
            self._tokens[:B].masked_fill_(beg[:, None], -1)
            self._frames[:B].masked_fill_(beg[:, None], -1)
            g0, (h0, c0) = lm.forward(torch.zeros(1, B, device=dev, dtype=torch.int64), lm.init_hidden(B))
            g.copy_(torch.where(beg[:, None], g0, g))
            h.copy_(torch.where(beg[None, :, None], h0, h))
            c.copy_(torch.where(beg[None, :, None], c0, c))
        rows, cols = torch.arange(B, device=dev), torch.arange(V, device=dev)
        t, u, here = st[0, :B].long(), st[1, :B].long(), st[2, :B].long()
        trunc = st[4, :B] != 0
        L = nf.long().clamp(0, S)
        pos = torch.zeros_like(t)
        done = (L <= 0) | trunc
        scores = self._scores[:B].clone()
        g, state = g.clone(), (h.clone(), c.clone())
        tokens, frames = self._tokens[:B], self._frames[:B]
        self.rounds = 0
        while not bool(done.all().item()):                      # one host read per lattice node
            self.rounds += 1
            live = ~done
            fr = f[rows, pos.clamp(max=S - 1)]
            fr = torch.where(live[:, None], fr, torch.zeros_like(fr))               # a row that sits out reads nothing of f
            lp = torch.log_softmax(fr + g, -1)
            top = lp.max(-1).values
            k = torch.where(lp == top[:, None], cols, V - 1).min(-1).values        # lowest index among equal maxima
            k = torch.where(here == self.max_symbols, torch.zeros_like(k), k)
            scores += torch.where(live, lp[rows, k], torch.zeros_like(top))
            blank, emit = live & (k == 0), live & (k != 0)
            e = emit.nonzero().view(-1)
            tokens[e, u[e]] = k[e]
            frames[e, u[e]] = t[e]
            step = blank.long()
            t, pos, here, u = t + step, pos + step, torch.where(blank, torch.zeros_like(here), here + emit.long()), u + emit.long()
            if e.numel():
                g1, (h1, c1) = lm.forward(torch.where(emit, k, torch.zeros_like(k)).view(1, B), state)
                g = torch.where(emit[:, None], g1, g)
                state = (torch.where(emit[None, :, None], h1, state[0]), torch.where(emit[None, :, None], c1, state[1]))
            trunc = trunc | (u >= cap)
            done = done | (pos >= L) | trunc
        st[0, :B], st[1, :B], st[2, :B], st[3, :B], st[4, :B] = t.int(), u.int(), here.int(), 1, trunc.int()
        self._scores[:B] = scores
        self._g[:B] = g
        self._gh[:, :B] = state[0]
        self._gc[:, :B] = state[1]


BEAM_MAX = 16            # csrc/rnnt_beam.hip keeps a row's records in LDS arrays of this many entries


def _prune_row(beam, finals, lp, i, L, W, cap):
    """Alignment step i of one row on the host (the general paths of ``BeamDecoder`` and ``BeamStream``): beam = [(tokens tuple, score)],
    lp [len(beam), V] float64 = the log-probabilities of its hypotheses at their frames, L the row's length.  Complete blank extensions
    are appended to ``finals`` -> (the new beam, [(parent j, token k; 0: blank)] of its members)."""
    V = lp.shape[1]
    where = {y: j for j, (y, _) in enumerate(beam)}
    blank, labels, gone = [], [], []
    for j, (y, s) in enumerate(beam):
        blank.append(s + float(lp[j, 0]))
        labels.append(s + lp[j, 1:])
        gone.append(torch.zeros(V - 1, dtype=torch.bool))
    complete = [i - len(y) + 1 == L for y, _ in beam]
    for sidx, (y, _) in enumerate(beam):                  # the extension of y[:-1] by y[-1] merges into y's blank extension
        j = where.get(y[:-1]) if y and not complete[sidx] else None
        if j is not None:
            a, b = torch.tensor(blank[sidx], dtype=torch.float64), labels[j][y[-1] - 1]
            blank[sidx] = float(torch.logaddexp(a, b))
            gone[j][y[-1] - 1] = True
    cand, vals = [], []                                  # (parent, token) in candidate order, and their scores
    for j, (y, _) in enumerate(beam):
        if complete[j]:
            finals.append((y, blank[j]))
        else:
            cand.append((j, 0)); vals.append(torch.tensor([blank[j]], dtype=torch.float64))
    for j, (y, _) in enumerate(beam):
        if len(y) < cap:
            ks = (~gone[j]).nonzero().view(-1)
            cand += [(j, int(k) + 1) for k in ks]
            vals.append(labels[j][ks])
    new, picks = [], []
    if cand:
        vals = torch.cat(vals)
        for a in torch.sort(-vals, stable=True).indices[:W].tolist():
            j, k = cand[a]
            picks.append((j, k))
            new.append((beam[j][0] + ((k,) if k else ()), float(vals[a])))
    return new, picks


def _ranked_finals(scores, seq, lengths, tokens, cap):
    """The finals of a beam search (scores [N, W], or records [N, W, K] whose column 0 ranks; order of completion, lengths [N, W], -1:
    absent; tokens [N, W, >= cap]) by (score descending, order of completion), absent ones last, in ``BeamDecoder.decode``'s format
    (the scores in their own shape, -inf where absent): two stable sorts."""
    N, W = lengths.shape
    cols = scores.reshape(N, W, -1)
    absent = lengths < 0
    o1 = torch.where(absent, torch.full_like(seq, 2 ** 31 - 1), seq).argsort(dim=1, stable=True)
    key = torch.where(absent, torch.full_like(cols[:, :, 0], float('inf')), -cols[:, :, 0]).gather(1, o1)
    order = o1.gather(1, key.argsort(dim=1, stable=True))
    lengths = lengths.gather(1, order).long()
    cols = torch.where(lengths[:, :, None] < 0, torch.full_like(cols, float('-inf')), cols.gather(1, order[:, :, None].expand_as(cols)))
    tokens = tokens[:, :, :cap].gather(1, order[:, :, None].expand(N, W, cap))
    return _slots.mask_tokens(tokens, lengths), lengths, cols.view(scores.shape), (lengths >= 0).sum(1)


class BeamDecoder(_HeadDecoder):
    """Beam search for a ``recognizer.Transducer`` head: alignment-length synchronous decoding with exact merging ([Saon20] Saon,
    Tueske, Audhkhasi, ICASSP 2020), with preallocated buffers for ``max_batch`` rows, ``beam`` hypotheses per row and
    ``capacity`` symbols per hypothesis.  Per row, with F = classifier(features), L = clamp(input_lengths, 0, T), W = beam:

        B = [the empty hypothesis, score 0, on the prediction network's output for the zero prefix of training]
        for i in 0 .. L + capacity - 1, while B is not empty:        # hypothesis j stands at frame t_j = i - len(y_j) < L
            lp_j = log_softmax(F[t_j] + g_j)
            candidates: the blank extension of every j (complete at t_j + 1 == L: it joins the finals instead), then for every j with
                        len(y_j) < capacity its extensions by k = 1 .. V-1; equal token sequences merge into the earliest (logaddexp)
            B = the W best by (score descending, candidate position ascending)
        the W best finals by (score descending, order of completion)

    so a score sums the alignment paths the search kept of its hypothesis (all of them when nothing was pruned).  W = 1 is not greedy
    search.  The fused path (csrc/rnnt_beam.hip) costs ``num_layers + 3`` launches per alignment step for the whole batch and reads one
    word every ``SYNC_EVERY`` steps; the general path runs the same search on ``rnn.Decoder.forward`` at T = 1 over N * W rows with
    torch operators, the candidates pruned on the host."""

    def __init__(self, head, max_batch, capacity, beam=4):
        self.head, self._net = head, _slots.Network(head.lm)
        self.max_batch, self.capacity, self.beam = int(max_batch), int(capacity), int(beam)
        _slots.check_sizes('BeamDecoder', self, BEAM_MAX)
        dev = head.lm.embedding.weight.device
        S, cap = self.max_batch * self.beam, self.capacity
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        self._lstm = _slots.SlotState(self._net, S)               # the prediction network's state in every slot
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            if self._lstm.allocated:
                # flat buffers, viewed per call at that call's N * W slots.  The beam's records exist twice (step parity), like the state.
                self._rec = [(torch.zeros(S, **f32), torch.zeros(S, **i32), torch.zeros(S * cap, **i32)) for _ in range(2)]
                self._parent, self._last = torch.zeros(S, **i32), torch.zeros(S, **i32)
                self._fin = (torch.zeros(S, **f32), torch.zeros(S, **i32), torch.zeros(S, **i32), torch.zeros(S * cap, **i32),
                             torch.zeros(self.max_batch, **i32))
                self._live = torch.zeros(64, **i32)                  # one word per alignment step; grown to T + capacity
        self._device = dev      # of the buffers: a head moved since needs a new decoder
        self.iterations = 0    # alignment steps of the last decode

    def decode(self, features, input_lengths, capacity=None, beam=None):
        """features [N, T, feat_dim], input_lengths [N] (clipped to T) -> (tokens [N, W, capacity] int64, -1 past a hypothesis's length
        and in absent hypotheses; lengths [N, W] int64, -1: absent; scores [N, W] float32, best first, -inf: absent; counts [N] int64).
        ``capacity`` / ``beam``: search with less room than the buffers hold (default: all of it)."""
        self._check(features, input_lengths)
        cap, W = _slots.room('BeamDecoder', self, capacity, beam)
        with torch.no_grad():
            N, T, _ = features.shape
            cl = self.head.classifier
            f = HF.linear(features.float(), cl.weight, cl.bias).contiguous()                   # [N, T, V]
            il = input_lengths.to(device=features.device, dtype=torch.int32).clamp(0, T).contiguous()
            return _ranked_finals(*(self._decode_fused if self.fused else self._decode_general)(f, il, N, W, cap), cap)

    # ---- the fused path: num_layers + 3 launches per alignment step --------------------------------------------------------------------
    def _decode_fused(self, f, il, N, W, cap):
        st = self._lstm.view(N, W)
        R, ld, steps = N * W, self.capacity, f.shape[1] + cap
        if self._live.numel() < steps:
            self._live = torch.zeros(steps, device=self._live.device, dtype=torch.int32)
        live = self._live[:steps]
        live.zero_()
        rec = [(s[:R].view(N, W), u[:R].view(N, W), t[:R * ld].view(N, W, ld)) for s, u, t in self._rec]
        parent, last = self._parent[:R].view(N, W), self._last[:R].view(N, W)
        fs, fq, fl, ft, fn = self._fin
        fin = (fs[:R].view(N, W), fq[:R].view(N, W), fl[:R].view(N, W), ft[:R * ld].view(N, W, ld), fn[:N])
        st.start(0)                                            # the zero prefix of training (recognizer.py:107), in every slot
        for i in range(steps):                                 # a hypothesis at step i has t + u = i, t < L, u <= cap: none after L + cap
            q = i & 1
            ops.rnnt_beam_step(f, st.g[q], st.bias, il, i, cap, rec[q], rec[1 - q], parent, last, fin, *st.gather(q), live[i:])
            if i == steps - 1 or ((i + 1) % SYNC_EVERY == 0 and int(live[i].item()) == 0):
                break
            st.cells(1 - q)
            st.keep(parent, last, q)
        self.iterations = i + 1
        if int(live[i].item()) != 0:
            raise _lib.HaloError('BeamDecoder: rows still live after T + capacity alignment steps')
        return fin[0].clone(), fin[1].clone(), fin[2].clone(), fin[3].clone()

    # ---- the general path: the same search on rnn.Decoder.forward at T = 1 over N * W rows, pruned on the host ----------------------------
    def _decode_general(self, f, il, N, W, cap):
        lm = self.head.lm
        dev, T, V = f.device, f.shape[1], f.shape[2]
        R = N * W
        Ls = il.tolist()
        g, state = lm.forward(torch.zeros(1, R, device=dev, dtype=torch.int64), lm.init_hidden(R))
        beams = [[((), 0.0)] if Ls[n] > 0 else [] for n in range(N)]          # hypothesis j of row n lives in slot n W + j
        finals = [[((), 0.0)] if Ls[n] == 0 else [] for n in range(N)]
        slot_row = torch.arange(R, device=dev) // W
        self.iterations = 0
        for i in range(T + cap):
            if not any(beams):
                break
            self.iterations += 1
            t = torch.zeros(R, dtype=torch.int64)
            for n, B in enumerate(beams):
                for j, (y, _) in enumerate(B):
                    t[n * W + j] = i - len(y)
            lp = torch.log_softmax(f[slot_row, t.to(dev)] + g, -1).double().cpu()       # one host read per alignment step
            src, tok = torch.arange(R), torch.zeros(R, dtype=torch.int64)
            for n, B in enumerate(beams):
                if not B:
                    continue
                beams[n], picks = _prune_row(B, finals[n], lp[n * W:n * W + len(B)], i, Ls[n], W, cap)
                for r, (j, k) in enumerate(picks):
                    src[n * W + r], tok[n * W + r] = n * W + j, k
            if not any(beams):
                break
            src, tok = src.to(dev), tok.to(dev)
            g, state = _slots.step_general(lm, g, state, src, tok, tok != 0)
        scores = torch.full((N, W), float('-inf'), dtype=torch.float32)
        seq, lengths = torch.zeros(N, W, dtype=torch.int32), torch.full((N, W), -1, dtype=torch.int32)
        tokens = torch.zeros(N, W, cap, dtype=torch.int32)
        for n, fin in enumerate(finals):
            best = sorted(range(len(fin)), key=lambda a: (-fin[a][1], a))[:W]
            for w, a in enumerate(best):
                scores[n, w], seq[n, w], lengths[n, w] = fin[a][1], w, len(fin[a][0])
                tokens[n, w, :len(fin[a][0])] = torch.tensor(fin[a][0], dtype=torch.int32)
        return scores.to(dev), seq.to(dev), lengths.to(dev), tokens.to(dev)


class BeamStream(_HeadDecoder):
    """``BeamDecoder``'s search carried across calls: the transcription logits of ``max_rows`` rows arrive in chunks,
    every row's beam stays in device memory between the calls, and after the call that marks a row final its n-best list is what
    ``BeamDecoder.decode`` returns on the row's whole utterance -- on the fused path bit for bit, scores included -- at the cost of the
    new frames alone.  The search is alignment-length synchronous: at step i hypothesis j stands at frame t_j = i - len(y_j), and a step
    depends on the row's length L only through t_j < L and t_j + 1 == L.  With R frames received a row that is not final executes step
    i iff max_j t_j + 1 < R: then every frame it reads has arrived and both tests come out as for any L > R.  Otherwise it stalls and
    keeps its beam; a final row runs on with L = R until its beam is empty.  Hypotheses with more symbols stand at earlier frames, so
    the rows keep their latest ``capacity + max_chunk + 1`` logit frames in a ring, which holds every frame a step can read.

    advance(f [B, S, V], n_frames=None, begin=None, final=None): ``GreedyStream.advance``'s arguments, S <= max_chunk, and ``final``
        (host-side like ``begin``): no frames follow this call's for the row.  A row must begin before its first frames; a row that is
        final (or never began) is closed until it begins again, and frames sent to it change nothing, as for the rows from B on.
        Returns nothing: ``nbest()`` reads the rows out.
    nbest(): (tokens [max_rows, W, capacity] int64, lengths [max_rows, W] int64, scores [max_rows, W] fp32, counts [max_rows] int64)
        in ``BeamDecoder.decode``'s format: a closed row's finals, ordered as ``BeamDecoder.decode`` orders them; an open row's
        stalled beam in slot order, which the selection leaves score-descending.
    rounds: the rounds of the last call.

    One call is the open launch, then rounds of (step, ``num_layers`` cells, out_layer, keep) over all max_rows * W slots until no row
    is live.  Records and state are double-buffered by the round's parity for all rows alike, so a row that cannot execute its step
    does an identity round, and the parity is carried across calls.  A round is always completed: the next call needs the kept slots'
    state.  The live word is read after S rounds and then every ``sync_every`` rounds (``STREAM_BEAM_SYNC_EVERY``; DESIGN.md 3.3aa
    has the measured cadences); the rounds past the last live one are identity rounds and change no result.  A call needs at most S + capacity + 2 rounds; more raise ``HaloError``.  The general path (f32 mode, HALO_RNNT_FUSED=0, a
    head the fused launches do not take) carries the same search on ``rnn.Decoder.forward`` at T = 1, pruned on the host.  The path is
    chosen when a row begins; do not change it in the middle of a stream."""

    def __init__(self, head, max_rows, capacity, beam=4, max_chunk=64):
        self.head, self._net = head, _slots.Network(head.lm)
        self.max_rows, self.capacity, self.beam, self.max_chunk = int(max_rows), int(capacity), int(beam), int(max_chunk)
        if self.max_rows < 1 or self.capacity < 1 or self.max_chunk < 1:
            raise ValueError('BeamStream: need max_rows >= 1, capacity >= 1 and max_chunk >= 1')
        if self.beam < 1 or self.beam > BEAM_MAX:
            raise ValueError(f'BeamStream: beam {self.beam} outside 1 .. {BEAM_MAX}')
        lm = head.lm
        H, L, V = lm.hidden_dim, lm.num_layers, lm.num_classes
        dev = lm.embedding.weight.device
        if dev.type != 'cuda':
            raise _lib.HaloError('haloop_amd.transducer.BeamStream runs on the HIP device only (no CPU path)')
        mb, W, cap = self.max_rows, self.beam, self.capacity
        R = mb * W
        self._lstm = _slots.SlotState(self._net, R)               # the prediction network's state in every slot
        self._zero = _slots.SlotState(self._net, 1)                # and after the zero prefix, on one slot: what a beginning row starts from
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.inference_mode(False):
            self._ring = torch.zeros(mb, cap + self.max_chunk + 1, V, **f32)
            self._meta = torch.zeros(4, mb, **i32)                 # step | frames received | final | closed, one word per row
            self._meta[3].fill_(1)
            self._nf, self._flags = torch.zeros(mb, **i32), torch.zeros(mb, **i32)
            self._live = torch.zeros(self.max_chunk + cap + 2, **i32)            # one word per round of a call
            if self._lstm.allocated:
                self._rec = [(torch.full((mb, W), float('-inf'), **f32), torch.full((mb, W), -1, **i32), torch.zeros(mb, W, cap, **i32))
                             for _ in range(2)]
                self._parent, self._last = torch.zeros(mb, W, **i32), torch.zeros(mb, W, **i32)
                self._fin = (torch.full((mb, W), float('-inf'), **f32), torch.zeros(mb, W, **i32), torch.full((mb, W), -1, **i32),
                             torch.zeros(mb, W, cap, **i32), torch.zeros(mb, **i32))
            self._gg = torch.zeros(R, V, **f32)                    # the general path's state
            self._gh, self._gc = torch.zeros(L, R, H, **f32), torch.zeros(L, R, H, **f32)
        self._rows = [dict(beam=[], finals=[], step=0, R=0, final=False, closed=True) for _ in range(mb)]     # the general path's records
        self._general = False  # which path holds the streams
        self._cur = 0          # the copy of records and state that the next round reads.  Carried across calls.
        self.sync_every = STREAM_BEAM_SYNC_EVERY
        self.rounds = 0

    def advance(self, f, n_frames=None, begin=None, final=None):
        mb = self.max_rows
        V = self.head.lm.num_classes
        if not torch.is_tensor(f) or f.dim() != 3 or not 1 <= f.shape[0] <= mb or not 1 <= f.shape[1] <= self.max_chunk \
                or f.shape[2] != V or f.dtype != torch.float32:
            raise ValueError(f'BeamStream.advance: f must be a float32 tensor [1 .. {mb}, 1 .. {self.max_chunk}, {V}]')
        B, S = f.shape[0], f.shape[1]
        if n_frames is not None and (not torch.is_tensor(n_frames) or tuple(n_frames.shape) != (B,) or n_frames.dtype != torch.int32):
            raise ValueError(f'BeamStream.advance: n_frames must be an int32 tensor [{B}]')
        if not f.is_cuda or (n_frames is not None and not n_frames.is_cuda):
            raise _lib.HaloError('haloop_amd.transducer.BeamStream runs on the HIP device only (no CPU path)')
        if self.head.training:
            raise NotImplementedError('BeamStream is an inference path: put the head in eval mode')
        marks = []
        for name, mark in (('begin', begin), ('final', final)):
            if mark is not None:
                if torch.is_tensor(mark):
                    if mark.is_cuda:
                        raise ValueError(f'BeamStream.advance: {name} is host-side (a sequence of bools or a CPU bool tensor)')
                    mark = mark.tolist()
                mark = [bool(e) for e in mark]
                if len(mark) != B:
                    raise ValueError(f'BeamStream.advance: {name} has {len(mark)} entries for {B} rows')
            marks.append(mark)
        begin, final = marks
        with torch.no_grad():
            any_begin = begin is not None and any(begin)
            flags = None
            if any_begin or (final is not None and any(final)):
                flags = self._flags[:B]
                flags.copy_(torch.tensor([(ops.STREAM_BEGIN if begin and begin[b] else 0) | (ops.STREAM_FINAL if final and final[b] else 0)
                                          for b in range(B)], dtype=torch.int32))
            if n_frames is None:
                nf = self._nf[:B].fill_(S)
            else:
                nf = n_frames.detach().contiguous()
            self._advance(f.detach(), nf, flags, any_begin)

    def _advance(self, f, nf, flags, any_begin):
        """f [B, S, V], nf int32 [B] and flags int32 [>= B] (or None; bits STREAM_BEGIN and STREAM_FINAL) on the device; any_begin:
        whether a flag carries STREAM_BEGIN."""
        B, S, V = f.shape
        if f.stride(2) != 1 or f.stride(1) < V or f.stride(0) < (S - 1) * f.stride(1) + V:
            f = f.contiguous()
        if any_begin:
            self._general = not self.fused
        (self._advance_general if self._general else self._advance_fused)(f, nf, flags)

    # ---- the fused path: per round num_layers + 3 launches over all max_rows * W slots, whatever B ---------------------------------
    def _advance_fused(self, f, nf, flags):
        st, zero = self._lstm.view(self.max_rows, self.beam), self._zero
        if zero.built is not st.built:             # the stamp moved: a weight changed.  The launches ``BeamDecoder`` starts with
            zero.view(1, 1).start(0)
        cap, S = self.capacity, f.shape[1]
        rec, fin = self._rec, self._fin
        q = self._cur
        ops.rnnt_beam_stream_open(f, nf, flags, self._ring, self._meta, rec[q], fin, (zero.h[0, :, 0], zero.c[0, :, 0], zero.g[0][0]),
                                  st.h[q], st.c[q], st.g[q], self._live)
        bound = S + cap + 2
        try:
            for it in range(bound):
                ops.rnnt_beam_step_stream(self._ring, st.g[q], st.bias, self._meta, cap, rec[q], rec[1 - q], self._parent, self._last, fin,
                                          *st.gather(q), self._live[it:])
                st.cells(1 - q)
                st.keep(self._parent, self._last, q)
                q = 1 - q
                # a row sent S frames needs S rounds: the first read comes after them, the next every ``sync_every`` rounds
                if it == bound - 1 or (it + 1 >= S and (it + 1 - S) % self.sync_every == 0 and int(self._live[it].item()) == 0):
                    break
        finally:
            self._cur = q
        self.rounds = it + 1
        if int(self._live[it].item()) != 0:
            raise _lib.HaloError('BeamStream: rows still live after S + capacity + 2 rounds')

    # ---- the general path: the same carried search on rnn.Decoder.forward at T = 1 over max_rows * W rows, pruned on the host --------
    def _advance_general(self, f, nf, flags):
        lm = self.head.lm
        dev = f.device
        B, S, V = f.shape
        mb, W, cap, ring = self.max_rows, self.beam, self.capacity, self._ring.shape[1]
        R = mb * W
        counts = nf.clamp(0, S).tolist()
        marks = [0] * B if flags is None else flags[:B].tolist()
        g, state = self._gg, (self._gh, self._gc)
        if any(m & ops.STREAM_BEGIN for m in marks):                    # the zero prefix of training
            g0, (h0, c0) = lm.forward(torch.zeros(1, 1, device=dev, dtype=torch.int64), lm.init_hidden(1))
        for n in range(B):
            r = self._rows[n]
            if marks[n] & ops.STREAM_BEGIN:
                g[n * W], state[0][:, n * W], state[1][:, n * W] = g0[0], h0[:, 0], c0[:, 0]
                r.update(beam=[((), 0.0)], finals=[], step=0, R=0, final=False, closed=False)
            elif r['closed'] or r['final']:
                continue
            if counts[n]:
                self._ring[n, (r['R'] + torch.arange(counts[n], device=dev)) % ring] = f[n, :counts[n]]
            r['R'] += counts[n]
            if marks[n] & ops.STREAM_FINAL:
                r['final'] = True
                if r['R'] == 0:
                    r.update(beam=[], finals=[((), 0.0)], closed=True)
        slot_row = torch.arange(R, device=dev) // W
        self.rounds = 0
        while True:
            runs = [n for n, r in enumerate(self._rows) if not r['closed'] and r['beam'] and
                    (r['final'] or r['step'] - min(len(y) for y, _ in r['beam']) + 1 < r['R'])]
            if not runs:
                break
            self.rounds += 1
            if self.rounds > S + cap + 2:
                raise _lib.HaloError('BeamStream: rows still live after S + capacity + 2 rounds')
            t = torch.zeros(R, dtype=torch.int64)
            for n in runs:
                for j, (y, _) in enumerate(self._rows[n]['beam']):
                    t[n * W + j] = (self._rows[n]['step'] - len(y)) % ring
            lp = torch.log_softmax(self._ring[slot_row, t.to(dev)] + g, -1).double().cpu()      # one host read per round
            src, tok = torch.arange(R), torch.zeros(R, dtype=torch.int64)
            for n in runs:
                r = self._rows[n]
                beam, i = r['beam'], r['step']
                new, picks = _prune_row(beam, r['finals'], lp[n * W:n * W + len(beam)], i, r['R'] if r['final'] else r['R'] + 1, W, cap)
                for w, (j, k) in enumerate(picks):
                    src[n * W + w], tok[n * W + w] = n * W + j, k
                r['beam'], r['step'] = new, i + 1
                if not new and r['final']:
                    r['closed'] = True
            src, tok = src.to(dev), tok.to(dev)
            g, state = _slots.step_general(lm, g, state, src, tok, tok != 0)
        self._gg.copy_(g); self._gh.copy_(state[0]); self._gc.copy_(state[1])

    def nbest(self):
        mb, W, cap = self.max_rows, self.beam, self.capacity
        with torch.no_grad():
            if self._general:
                tokens = torch.full((mb, W, cap), -1, dtype=torch.int64)
                lengths, scores = torch.full((mb, W), -1, dtype=torch.int64), torch.full((mb, W), float('-inf'), dtype=torch.float32)
                for n, r in enumerate(self._rows):
                    fin = r['finals']
                    hyps = [fin[a] for a in sorted(range(len(fin)), key=lambda a: (-fin[a][1], a))[:W]] if r['closed'] else r['beam']
                    for w, (y, s) in enumerate(hyps):
                        lengths[n, w], scores[n, w] = len(y), s
                        tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
                dev = self._ring.device
                return tokens.to(dev), lengths.to(dev), scores.to(dev), (lengths >= 0).sum(1).to(dev)
            ft, fl, fs, fc = _ranked_finals(self._fin[0], self._fin[1], self._fin[2], self._fin[3], cap)
            sc, u, tok = self._rec[self._cur]
            bl = u.long()
            bt = _slots.mask_tokens(tok, bl)
            bs = torch.where(bl < 0, torch.full_like(sc, float('-inf')), sc)
            closed = self._meta[3] != 0
            return (torch.where(closed[:, None, None], ft, bt), torch.where(closed[:, None], fl, bl), torch.where(closed[:, None], fs, bs),
                    torch.where(closed, fc, (bl >= 0).sum(1)))
