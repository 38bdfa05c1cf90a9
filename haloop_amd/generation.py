"""Batched sampling for haloop_amd.attention.GPT: a preallocated KV cache, one decode step as 5 n_layer + 2 fused HIP launches
(csrc/gpt_decode.hip) and the draw (temperature, top-k, multinomial, stop handling) on the device.

``attention.generate`` is the reference's loop (ha/attention.py:282-321) on ``GPT.forward(input_ids, past)``: it reallocates and copies
the whole cache per token, runs the general operators at M = B rows, draws with torch and reads the device once per token.  ``Sampler``
keeps the cache ``[L, 2, max_batch, nh, max_len, hs]`` (fp32, the reference's ``present`` layout) for its lifetime.  Every scalar a
step needs -- each row's position, draw counter, length and alive flag, and the draw's settings -- is a device word, so the launch
arguments of a step never change: with ``use_graph`` one captured step is replayed for every position.  ``sample`` reads the device
every 16 tokens (to stop once every row is dead) and at the end.

The fused step runs when the math mode is not ``f32``, ``config.bias`` is False, C is 512, 768 or 1024, head_dim is 64, there is no
``stable_embedding`` and no unmerged LoRA adapter, and the model is causal; everything else takes the general step: the existing
operators on the same preallocated cache (nothing reallocated per token) and the same device draw.  The draw is defined in
include/halo.h (halo_gpt_sample) so that a CPU restatement can follow it.
"""
import os

import torch

from . import _lib, lora, ops
from ._capture import capture

SYNC_EVERY = 16          # sample() reads the alive flags every this many tokens


def _graph_default():
    """HALO_GPT_DECODE_GRAPH=1: replay one captured step per token.  Default: eager launches -- the two measured within a percent of
    each other, eager ahead at more of the points, so the step ships without the capture."""
    return os.environ.get('HALO_GPT_DECODE_GRAPH', '0') == '1'


class Sampler:
    def __init__(self, model, max_batch, max_len=None, use_graph=None):
        cfg = model.config
        self.model = model
        self.max_batch = int(max_batch)
        self.max_len = int(cfg.block_size if max_len is None else max_len)
        if self.max_batch < 1 or self.max_len < 1 or self.max_len > cfg.block_size:
            raise ValueError(f'Sampler: need max_batch >= 1 and 1 <= max_len <= block_size ({cfg.block_size})')
        self.use_graph = _graph_default() if use_graph is None else bool(use_graph)
        C, H, V = cfg.n_embd, cfg.n_head, cfg.vocab_size
        dev = model.lm_head.weight.device
        mb = self.max_batch
        with torch.inference_mode(False):          # ordinary tensors: they are updated in place inside and outside inference mode
            self.cache = torch.zeros(cfg.n_layer, 2, mb, H, self.max_len, C // H, device=dev, dtype=torch.float32)
            f = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float32)
            self._x, self._qkv, self._att, self._hid, self._logits = f(mb, C), f(mb, 3 * C), f(mb, C), f(mb, 4 * C), f(mb, V)
            self._state = torch.zeros(4, mb, device=dev, dtype=torch.int32)      # pos | step | length | alive, one word per row
            self._tokens = torch.zeros(mb, self.max_len, device=dev, dtype=torch.int64)
            self._next = torch.zeros(mb, device=dev, dtype=torch.int64)
            self._cfg = torch.zeros(8, device=dev, dtype=torch.int32)            # the draw's settings (ops.gpt_sample_cfg)
        self._B = 0            # rows of the running generation
        self._t = 0            # positions the cache holds (host side: every row is at the same position)
        self._images = None    # (stamp, per-layer decode images, lm_head image)
        self._graphs = {}      # B -> (key, graph, held)

    # ---- which step ---------------------------------------------------------------------------------------------------
    @property
    def fused(self):
        """Whether the fused launches are in use (decided from the model and the math mode as they are now)."""
        cfg = self.model.config
        C = cfg.n_embd
        if _lib.get_math_mode() == 'f32' or cfg.bias or cfg.stable_embedding or not cfg.causal:
            return False
        if C not in (512, 768, 1024) or C % cfg.n_head != 0 or C // cfg.n_head != 64 or self.max_len > 8192:
            return False
        blocks = self.model.transformer.h
        if any(lora.is_active(blk.attn.c_attn) for blk in blocks):
            return False
        if any(lin.bias is not None for blk in blocks for lin in (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj)):
            return False
        return (ops.gpt_decode_linear_supported(C, True) and ops.gpt_decode_linear_supported(C, False)
                and ops.gpt_decode_linear_supported(4 * C, False))

    def _stamp(self):
        return tuple((p._version, p.data_ptr()) for p in self.model.parameters()) + (_lib.weights_epoch(),)

    @torch.no_grad()
    def _decode_images(self):
        """Decode images of the four Linears of every block and of lm_head, rebuilt when a parameter changes."""
        stamp = self._stamp()
        if self._images is None or self._images[0] != stamp:
            w = lambda lin: ops.decode_image(lin.weight.detach().float().contiguous())
            layers = [(w(blk.attn.c_attn), w(blk.attn.c_proj), w(blk.mlp.c_fc), w(blk.mlp.c_proj)) for blk in self.model.transformer.h]
            self._images = (stamp, layers, w(self.model.lm_head))
            self._graphs.clear()
        return self._images[1], self._images[2]

    # ---- checks, all on the host before any launch ----------------------------------------------------------------------
    def _check(self, input_ids, new_tokens, grad=True):
        if input_ids.dim() != 2 or input_ids.shape[1] < 1:
            raise ValueError('Sampler: input_ids must be [B, P] with P >= 1')
        B, P = input_ids.shape
        if B > self.max_batch:
            raise ValueError(f'Sampler: batch {B} exceeds max_batch {self.max_batch}')
        if P + new_tokens > self.max_len:
            raise ValueError(f'Sampler: prompt {P} + {new_tokens} new tokens exceed max_len {self.max_len}')
        if not input_ids.is_cuda:
            raise _lib.HaloError('haloop_amd.generation.Sampler runs on the HIP device only (no CPU path)')
        if grad and torch.is_grad_enabled() and any(p.requires_grad for p in self.model.parameters()):
            raise NotImplementedError('Sampler is an inference path: call under torch.no_grad() / inference_mode')

    # ---- the pieces -------------------------------------------------------------------------------------------------------
    def prefill(self, input_ids):
        """[B, P] -> logits of the last position [B, V] (a view of the Sampler's buffer: the next call overwrites it); resets the
        position.  The block forward of GPT.forward with keys and values written straight into the preallocated cache."""
        self._check(input_ids, 0)
        with torch.no_grad():
            return self._prefill(input_ids)

    def _prefill(self, input_ids):
        B, P = input_ids.shape
        m = self.model
        if self.fused:
            self._decode_images()                  # (built here, once per parameter version: the steps launch nothing else)
        x, _ = m._trunk(input_ids, cache=self.cache[:, :, :B], t0=0)
        last = x.view(B, P, -1)[:, -1, :].contiguous()
        logits = self._logits[:B]
        logits.copy_(m._linear(last, m.lm_head))
        self._B, self._t = B, P
        return logits

    def _fused_layers(self, B, layers, head):
        """5 n_layer + 1 launches: x [B, C] (the step's embedded input rows) -> logits; keys / values stored at each row's pos word."""
        m, cfgm = self.model, self.model.config
        C, V = cfgm.n_embd, cfgm.vocab_size
        x, qkv, att, hid, logits, pos = self._x[:B], self._qkv[:B], self._att[:B], self._hid[:B], self._logits[:B], self._state[0]
        for l, blk in enumerate(m.transformer.h):
            w_attn, w_proj, w_fc, w_fc2 = layers[l]
            ops.gpt_decode_linear(x, w_attn, 3 * C, qkv, ln_weight=blk.ln_1.weight)
            ops.gpt_decode_attention(qkv, self.cache[l, 0, :B], self.cache[l, 1, :B], pos, att)
            ops.gpt_decode_linear(att, w_proj, C, x, accumulate=True)
            ops.gpt_decode_linear(x, w_fc, 4 * C, hid, ln_weight=blk.ln_2.weight, gelu=True)
            ops.gpt_decode_linear(hid, w_fc2, C, x, accumulate=True)
        ops.gpt_decode_linear(x, head, V, logits, ln_weight=m.transformer.ln_f.weight)
        return logits

    def _general_layers(self, B, ids):
        """The existing operators at T = 1 on the preallocated cache: ids [B] -> logits."""
        m = self.model
        x, _ = m._trunk(ids.contiguous().view(B, 1), cache=self.cache[:, :, :B], t0=self._t)
        logits = self._logits[:B]
        logits.copy_(m._linear(x, m.lm_head))
        return logits

    def step(self, tokens):
        """Teacher-forced: tokens [B] int64 on the device, the input at the next position -> logits [B, V] (a view, as prefill's)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.model.parameters()):
            raise NotImplementedError('Sampler is an inference path: call under torch.no_grad() / inference_mode')
        with torch.no_grad():
            return self._step(tokens)

    def _step(self, tokens):
        B = self._B
        if B == 0:
            raise ValueError('Sampler.step: call prefill first')
        if tokens.shape != (B,):
            raise ValueError(f'Sampler.step: expected tokens of shape ({B},)')
        if not tokens.is_cuda:
            raise _lib.HaloError('haloop_amd.generation.Sampler runs on the HIP device only (no CPU path)')
        if self._t + 1 > self.max_len:
            raise ValueError(f'Sampler.step: the cache holds max_len = {self.max_len} positions')
        if self.fused:
            layers, head = self._decode_images()
            m = self.model
            self._x[:B].copy_(ops.embed_fwd(tokens.contiguous().view(B, 1), m.transformer.wte.weight, m.transformer.wpe.weight, self._t))
            self._state[0].fill_(self._t)
            logits = self._fused_layers(B, layers, head)
        else:
            logits = self._general_layers(B, tokens)
        self._t += 1
        return logits

    def _draw(self, B, fused):
        tr = self.model.transformer
        if fused:
            ops.gpt_sample(self._logits[:B], self._cfg, self._state, self._tokens[:B], self._next, tr.wte.weight, tr.wpe.weight, self._x)
        else:
            ops.gpt_sample(self._logits[:B], self._cfg, self._state, self._tokens[:B], self._next)

    def _graph(self, B, layers, head):
        """One captured step (5 n_layer + 1 launches and the draw, a strictly linear chain on one stream) per batch size and parameter
        version.  The warm-up run outside the capture is a real step at whatever the state words hold: sample() builds the graph before
        the prefill, with every word zero, and initialises the state after it."""
        key = (self._images[0], _lib.get_math_mode(), self._cfg.data_ptr())
        entry = self._graphs.get(B)
        if entry is None or entry[0] != key:
            def step():
                self._fused_layers(B, layers, head)
                self._draw(B, True)
            graph, _ = capture(step)
            entry = (key, graph, (layers, head, self._cfg))       # the graph reads the images and the settings by address
            self._graphs[B] = entry
        return entry[1]

    def sample(self, input_ids, max_new_tokens, temperature=1.0, top_k=None, stop_token=50256, seed=None):
        """-> (tokens [B, max_new_tokens] int64, lengths [B] int64).  A row that draws ``stop_token`` stops there: the stop token is
        not counted in its length (as the reference does not yield it) and its remaining slots hold ``stop_token``."""
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError('Sampler.sample: max_new_tokens must be positive')
        if top_k is not None and int(top_k) < 1:
            raise ValueError('Sampler.sample: top_k must be positive')
        if not float(temperature) > 0.0:
            raise ValueError('Sampler.sample: temperature must be positive')
        self._check(input_ids, max_new_tokens)
        with torch.no_grad():
            return self._sample(input_ids, max_new_tokens, temperature, top_k, stop_token, seed)

    def _sample(self, input_ids, max_new_tokens, temperature, top_k, stop_token, seed):
        B, P = input_ids.shape
        dev = input_ids.device
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())            # torch's CPU generator: torch.manual_seed makes a run repeatable
        fused = self.fused
        layers, head = self._decode_images() if fused else (None, None)
        cfg = ops.gpt_sample_cfg(temperature, top_k, stop_token, seed, dev)
        self._cfg.copy_(cfg)
        st = self._state
        graph = None
        if fused and self.use_graph and max_new_tokens > 1:
            st.zero_()
            graph = self._graph(B, layers, head)
        self._prefill(input_ids)
        stop_fill = int(stop_token) if -(1 << 31) <= int(stop_token) < (1 << 31) else -1
        self._tokens[:B, :max_new_tokens].fill_(stop_fill)
        st[0].fill_(P - 1); st[1].zero_(); st[2].zero_(); st[3].fill_(1)
        self._draw(B, fused)                                               # token 0, from the prompt's last logits
        for i in range(1, max_new_tokens):
            if i % SYNC_EVERY == 0 and not bool(st[3, :B].any().item()):
                break
            if graph is not None:
                graph.replay()
            else:
                if fused:
                    self._fused_layers(B, layers, head)
                else:
                    self._general_layers(B, self._next[:B])
                self._draw(B, fused)
            self._t += 1
        return self._tokens[:B, :max_new_tokens].clone(), st[2, :B].long()

    def past(self):
        """[L, 2, B, nh, t, hs]: what GPT.forward would have returned as ``present`` for the positions processed so far."""
        return self.cache[:, :, :self._B, :, :self._t].clone()


def generate(model, input_ids, max_new_tokens, temperature=1.0, top_k=None, stop_token=50256):
    """The reference's generator signature (ha/attention.py:285; B = 1, yields [1, 1] tensors) on a Sampler kept on the model.  The
    request is checked here, before the first ``next()``; it must fit the block size (the reference's re-forward of a cropped context
    past block_size is not built: ValueError).

    Two things a caller should know.  The Sampler stays on the model as ``model._generation_sampler`` (model and sampler refer to each
    other) with a cache of block_size positions -- 75 MB at GPT-2 small -- so that later calls reuse the cache, the decode images and
    the captured step; ``del model._generation_sampler`` gives it back.  And the whole request is generated at the first ``next()``:
    the tokens are then handed out one by one, so a consumer that stops early has still paid for ``max_new_tokens`` (or for the
    tokens up to the stop token, to the next multiple of 16).  Use ``Sampler.sample`` with a smaller ``max_new_tokens`` to bound that."""
    sampler = getattr(model, '_generation_sampler', None)
    if sampler is None or sampler.model is not model or sampler.cache.device != model.lm_head.weight.device:
        sampler = Sampler(model, 1)
        model._generation_sampler = sampler
    if input_ids.dim() != 2 or input_ids.shape[0] != 1:
        raise ValueError('generate: input_ids must be [1, P] (use Sampler.sample for a batch)')
    sampler._check(input_ids, int(max_new_tokens), grad=False)        # (the generator runs under inference_mode, as the reference's)

    def run():
        with torch.inference_mode():
            tokens, lengths = sampler.sample(input_ids, max_new_tokens, temperature, top_k, stop_token)
            n = int(lengths[0].item())
        for i in range(n):
            yield tokens[:, i:i + 1]
    return run()
