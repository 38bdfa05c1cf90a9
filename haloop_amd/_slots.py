"""What the beam searches that carry an ``rnn.Decoder`` across the N * W slots of a beam share on the host (``transducer.BeamDecoder`` /
``BeamStream``, ``fusion.CTCFusionDecoder`` / ``TransducerFusionDecoder`` / ``AttentionFusionDecoder``); the kernels' shared pieces are in
csrc/beam_common.h.

``Network``: one ``rnn.Decoder`` as the fused launches read it -- its decode images, their stamp and its share of the fused rule.
``SlotState``: the stepped LSTM state of every slot (h, c and g in two copies by step parity, the cells' input rows) with the launches
that move it: ``start``, ``cells``, ``keep`` and the gather arguments of the step kernels.
``step_general``: the same step on ``rnn.Decoder.forward`` at T = 1, for the general paths.
``check_sizes``, ``room`` and ``mask_tokens``: the sizes a decoder is built with, a call's capacity and beam within them, and the -1 past
a hypothesis's length.
"""
import os

import torch

from . import _lib, ops
from .rnn import lstm_param_list


def fused_default():
    """HALO_RNNT_FUSED=0: the general path even where the fused launches apply (the measured pair: DESIGN.md 3.3j)."""
    return os.environ.get('HALO_RNNT_FUSED', '1') != '0'


class Network:
    """An ``rnn.Decoder`` (a prediction network or a fusion LM) for the fused launches: ``images()`` and the network's part of the rule
    for when they apply.  Whether the module is in training mode is the decoders' to test."""

    def __init__(self, net):
        self.net = net
        self._images = None    # (stamp, per-layer gate images, out_layer image)

    @property
    def built(self):
        """The stamp the images were last built at (one object until a parameter changes): what state computed from them is keyed by."""
        return self._images and self._images[0]

    @property
    def fused(self):
        """Whether the fused launches take this network (decided from the network, the math mode and HALO_RNNT_FUSED as they are now)."""
        lm = self.net
        E, H = lm.embedding.weight.shape[1], lm.hidden_dim
        if not fused_default() or _lib.get_math_mode() == 'f32' or E != H or H % 512 != 0:
            return False
        return lm.num_classes <= 8192 and ops.decode_linear_supported(H, False) and ops.decode_linear_supported(2 * H, False)

    def stamp(self):
        return tuple((p._version, p.data_ptr()) for p in self.net.parameters()) + (_lib.weights_epoch(),)

    @torch.no_grad()
    def images(self):
        """Decode images of every layer's [W_ih | W_hh], rows permuted so that feature tile j holds the four gates of hidden units
        4 j .. 4 j + 3 (row 16 j + 4 q + i <- row q H + 4 j + i), and of the tied embedding; rebuilt when a parameter changes."""
        stamp = self.stamp()
        if self._images is None or self._images[0] != stamp:
            lm = self.net
            H, p = lm.hidden_dim, lstm_param_list(lm.rnn)
            layers = []
            for l in range(lm.num_layers):
                w = torch.cat([p[4 * l].detach().float(), p[4 * l + 1].detach().float()], 1)           # [4H, 2H]
                w = w.view(4, H // 4, 4, 2 * H).permute(1, 0, 2, 3).reshape(4 * H, 2 * H).contiguous()
                layers.append(ops.decode_image(w))
            self._images = (stamp, layers, ops.decode_image(lm.embedding.weight.detach().float().contiguous()))
        return self._images[1], self._images[2]


class SlotState:
    """The LSTM state of ``slots`` beam slots of one ``Network``: flat buffers allocated here, once (captured graphs hold their
    addresses), and viewed per decode at that decode's N * W slots.  h and c [2, L, R, H] exist twice (step parity); g [copies, R, V]
    twice where a ``keep`` launch follows the cells, once for a label-synchronous search; xh [L, R, 2 H] holds the cells' [x | h_prev]
    rows and top [R, H] the last layer's h.  ``allocated``: the network fits the fused cells (E == H) and is on the device."""

    def __init__(self, network, slots, copies=2):
        self.network, self.copies = network, copies
        lm = network.net
        wte = lm.embedding.weight
        S, E, H, L, V = slots, wte.shape[1], lm.hidden_dim, lm.num_layers, lm.num_classes
        f32 = dict(device=wte.device, dtype=torch.float32)
        self.allocated = E == H and wte.device.type == 'cuda'
        self.built, self._viewed = None, None      # the stamp of the images and the (N, W) the views were built with
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            if self.allocated:
                self._h, self._c = torch.zeros(2 * L * S * H, **f32), torch.zeros(2 * L * S * H, **f32)
                self._g = torch.zeros(copies * S * V, **f32)
                self._xh, self._top = torch.zeros(L * S * 2 * H, **f32), torch.zeros(S * H, **f32)

    def view(self, N, W):
        """The views of one decode's N * W slots and everything a step passes, built here and not per step -> self.  They are kept for
        the next decode of the same size on the same images: what is done before a search's first launch is not hidden behind the device."""
        lm, n = self.network.net, self.copies
        H, L, V, R = lm.hidden_dim, lm.num_layers, lm.num_classes, N * W
        layers, head_image = self.network.images()
        if self.built is self.network.built and (N, W) == self._viewed:
            return self
        self.built, self._viewed = self.network.built, (N, W)
        self.wte, self.bias = lm.embedding.weight, lm.out_layer.bias
        self.h, self.c = self._h[:2 * L * R * H].view(2, L, R, H), self._c[:2 * L * R * H].view(2, L, R, H)
        g = self._g[:n * R * V].view(n, R, V)
        self.g = [g[q % n] for q in range(2)]
        self.xh, top = self._xh[:L * R * 2 * H].view(L, R, 2 * H), self._top[:R * H].view(R, H)
        w = lstm_param_list(lm.rnn)
        self._cell = [[(self.xh[l], layers[l], w[4 * l + 2], w[4 * l + 3], self.c[q, l], self.h[q, l],
                        self.xh[l + 1, :, :H] if l + 1 < L else top) for l in range(L)] for q in range(2)]
        self._linear = [(top, head_image, V, self.g[q]) for q in range(2)]
        self._copy = [(self.h[q], self.c[q], self.g[q]) for q in range(2)]
        self._gather = [(self.wte, self.h[q], self.c[q], self.xh, self.c[1 - q]) for q in range(2)]
        return self

    def start(self, token):
        """The network after ``token`` (from the zero state) in every slot, into copy 0."""
        self.xh.zero_(); self.c[0].zero_()
        self.xh[0, :, :self.h.shape[3]] = self.wte[token]
        self.cells(0)

    def cells(self, q):
        """The network on the [x | h_prev] rows of every slot: c of copy q in place, h into copy q (and the x half of the layer above),
        out_layer into g of copy q -- ``L`` cell launches and one linear."""
        for args in self._cell[q]:
            ops.rnnt_lstm_cell(*args)
        ops.decode_linear(*self._linear[q])

    def keep(self, parent, last, q):
        """Blank-extended slots take their parent's h, c and g from copy q into copy 1 - q."""
        ops.rnnt_beam_keep(parent, last, *self._copy[q], *self._copy[1 - q])

    def gather(self, q):
        """(wte, h_in, c_in, xh, c_out) of a step that reads copy q: what its gather of the next cells' inputs takes."""
        return self._gather[q]


def step_general(net, g, state, src, tok, step_mask):
    """The general paths' step over R rows: row r continues row src[r]; where ``step_mask`` it takes ``tok`` through ``net.forward`` at
    T = 1, elsewhere it keeps its source's logits and state -> (g [R, V], (h, c) [L, R, H])."""
    g, (h, c) = g[src], tuple(z[:, src].contiguous() for z in state)
    g1, (h1, c1) = net.forward(tok.view(1, -1), (h, c))
    return torch.where(step_mask[:, None], g1, g), (torch.where(step_mask[None, :, None], h1, h), torch.where(step_mask[None, :, None], c1, c))


def check_sizes(name, decoder, beam_max):
    """The sizes a beam decoder is built with: ``beam_max``, what the step kernel's LDS records hold."""
    if decoder.max_batch < 1 or decoder.capacity < 1:
        raise ValueError(f'{name}: need max_batch >= 1 and capacity >= 1')
    if decoder.beam < 1 or decoder.beam > beam_max:
        raise ValueError(f'{name}: beam {decoder.beam} outside 1 .. {beam_max}')


def room(name, decoder, capacity, beam):
    """A call's (capacity, beam): the decoder's own by default, never more than its buffers hold."""
    cap = decoder.capacity if capacity is None else int(capacity)
    if cap < 1 or cap > decoder.capacity:
        raise ValueError(f'{name}: capacity {cap} outside 1 .. {decoder.capacity}')
    W = decoder.beam if beam is None else int(beam)
    if W < 1 or W > decoder.beam:
        raise ValueError(f'{name}: beam {W} outside 1 .. {decoder.beam}')
    return cap, W


def mask_tokens(tokens, lengths):
    """tokens [..., cap] as int64 with -1 past every hypothesis's length [...] (an absent hypothesis, length -1: everywhere)."""
    past = torch.arange(tokens.shape[-1], device=tokens.device) >= lengths[..., None]
    return tokens.long().masked_fill(past, -1)
