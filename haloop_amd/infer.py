"""Forward-only recognition (ha/loop.py:263-303 evaluate path for the CTC head): encoder forward ->
log-probs -> greedy collapse, straight on the C ABI and replayed from one HIP graph per input shape."""
import torch

from . import _lib, ops
from ._capture import capture
from .ops import NO_DROPOUT
from .rnn import lstm_param_list


class LstmCtcRecognizer:
    def __init__(self, encoder, recognizer, use_graph=True):
        """use_graph: True -- one HIP graph per input shape (default); False -- the six launches issued eagerly; 'auto' -- calls 4-23 are
        timed replayed and calls 27-46 eager, and the faster way stays (``auto_choice``; the host issues a batch's launches in ~55 us
        against ~140 us on the GPU, and a replay costs ~8 us more than it saves on ROCm 7.2)."""
        self._auto = {'n': 0} if use_graph == 'auto' else None
        self.auto_choice = None
        if use_graph == 'auto':
            use_graph = True
        self.encoder, self.recognizer, self.use_graph = encoder.eval(), recognizer.eval(), use_graph
        self._graph = None
        self._static = None
        self._out = None
        self._reserve = None          # owned between calls: the packed weight images stay in it while the weights do (see _stamp)
        self._graph_stamp = None
        _lib.lend_scratch(device=next(encoder.parameters()).device)

    def _stamp(self):
        """Changes whenever an LSTM weight may have changed: (storage address, torch version counter) of every parameter, and the
        process-wide count of optimizer launches, which write parameters behind torch's back (_lib.bump_weights_epoch)."""
        key = (_lib.weights_epoch(),) + tuple((p.data_ptr(), p._version) for p in lstm_param_list(self.encoder.lstm))
        return (hash(key) & 0x7fffffffffffffff) | 1

    def _run(self, x):
        enc, rec = self.encoder, self.recognizer
        B, T, F = x.shape
        p = lstm_param_list(enc.lstm)
        w_ih, w_hh, b_ih, b_hh = p[0::4], p[1::4], p[2::4], p[3::4]
        H, V = w_hh[0].shape[1], rec.classifier.weight.shape[0]
        y_sub, _ = ops.subsample_fwd(x, enc.subsample.weight, enc.subsample.bias, NO_DROPOUT)
        Tp = y_sub.shape[0]
        feats = torch.empty(B, Tp, H, device=x.device, dtype=torch.float32)
        need = (_lib.lib().halo_lstm_reserve_bytes(Tp, B, y_sub.shape[2], H, len(w_hh)) + 3) // 4
        if self._reserve is None or self._reserve.numel() != need or self._reserve.device != x.device:
            self._reserve = ops.lstm_reserve(Tp, B, y_sub.shape[2], H, len(w_hh), x.device)
        ops.lstm_fwd(y_sub, w_ih, w_hh, b_ih, b_hh, y=feats, y_strides=(H, Tp * H), y_relu=True, expect_backward=False,
                     reserve=self._reserve, weights_stamp=self._stamp())
        if ops.ctc_head_supported(Tp, H, V, 0):
            # classifier + log_softmax + greedy collapse in one launch, one workgroup per utterance (csrc/head.hip)
            return ops.ctc_head_greedy(feats, rec.classifier.weight, rec.classifier.bias)
        logits = ops.gemm(feats.view(B * Tp, H), rec.classifier.weight, True, True, B * Tp, V, H, bias1=rec.classifier.bias)
        lp = ops.log_softmax_fwd(logits).view(B, Tp, V)
        return ops.ctc_greedy(lp)          # alignments, scores, hyp (padded), hyp_len

    def static_input(self):
        """The graph's own input buffer (after the first call): fill it in place and pass it to recognize() to skip the copy."""
        return self._static

    @torch.no_grad()
    def recognize(self, x, clone=True):
        """x [B,T,F] on the HIP device -> (alignments [B,T'], scores [B,T'], hyp [B,T'] padded, hyp_len [B]).
        The results are copies the caller owns.  clone=False returns the graph's own output buffers instead, which the NEXT
        call overwrites (for loops that consume each result before asking for the next one)."""
        if self._auto is not None:
            return self._auto_recognize(x, clone)
        return self._recognize(x, clone)

    _AUTO = (3, 23, 26, 46)          # warm-up / timed calls replayed, warm-up / timed calls eager

    def _auto_recognize(self, x, clone):
        import time
        a, (w0, g1, w1, e1) = self._auto, self._AUTO
        a['n'] += 1
        n = a['n']
        if n == w0 + 1 or n == w1 + 1:
            torch.cuda.synchronize()
            a['t0'] = time.perf_counter()
        self.use_graph = n <= g1
        out = self._recognize(x, clone)
        if n == g1 or n == e1:
            torch.cuda.synchronize()
            a['graph' if n == g1 else 'eager'] = time.perf_counter() - a['t0']
        if n == e1:
            self.use_graph = not (a['eager'] / (e1 - w1) < 0.99 * a['graph'] / (g1 - w0))      # eager must win by 1 % to be kept
            self.auto_choice = {'graph_replay_ms': 1e3 * a['graph'] / (g1 - w0), 'eager_launches_ms': 1e3 * a['eager'] / (e1 - w1),
                                'use_graph': self.use_graph}
            self._auto = None
        return out

    def _recognize(self, x, clone):
        if not self.use_graph:
            return self._run(x.contiguous())
        stamp = self._stamp()
        if self._graph is None or self._static.shape != x.shape or self._graph_stamp != stamp:
            # (a changed weight: the graph replays launches that skip the weight packing, so it is captured again)
            self._graph_stamp = stamp
            self._static = x.contiguous().clone()        # private: refilling it must not write into the caller's tensor
            self._graph, self._out = capture(lambda: self._run(self._static))
        if x.data_ptr() != self._static.data_ptr():
            self._static.copy_(x)
        self._graph.replay()
        return tuple(o.clone() for o in self._out) if clone else self._out
