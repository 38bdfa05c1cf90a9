"""Drop-in for ha/grad_norm.py: the length of every utterance's own loss gradient (`hac --grad-norms`, ha/loop.py:540-554; the
expected-gradient-length queries of ha/active_loop.py:100-107 are built from the lines ``compute_grad_norm`` prints).

The reference differentiates one utterance at a time under ``vmap(grad_and_value(...))``, which has no batching rule for F.ctc_loss
(ha/grad_norm.py:14-16 strips the CTC loss for that reason), so it cannot score the LSTM-CTC model at all.  Here that model is the one
that is built: the rows of a batch are independent chains through the conv, the LSTM and the head, so ONE backward of sum_n loss_n leaves
every utterance's own back-propagated signal in buffers the library owns, and every parameter's per-utterance gradient is
dW_n = sum_t a_{n,t} b_{n,t}^T, whose squared norm is sum_{t,t'} <a_t, a_t'> <b_t, b_t'> -- two Gram matrices per utterance, never a
per-utterance weight gradient (csrc/ghost_norm.hip).  One forward, one backward, one Gram launch and its fixed-order sum.
"""
import torch
import torch.nn as nn

from . import _lib, ops
from .recognizer import TemporalClassifier
from .rnn import Encoder, lstm_param_list


class MiniSystem(nn.Module):
    """Encoder + recognizer under the reference's names (ha/grad_norm.py:10-25): ``forward`` is the batch's loss."""

    def __init__(self, encoder, recognizer):
        super().__init__()
        self.encoder = encoder
        self.recognizer = recognizer

    def forward(self, inputs, condtargets, input_lengths, condtarget_lengths):
        features, feature_lengths, _ = self.encoder(inputs, input_lengths)
        loss, _ = self.recognizer(features, condtargets, feature_lengths, condtarget_lengths)
        return loss


def norm_batched(x, p=2.0, eps=1e-6):
    """Row-wise p-norm of x [N, ...], each row scaled by its largest magnitude (+ eps) first so that the powers stay in range; the scale
    cancels, and an all-zero row gives exactly 0 (same values as ha/grad_norm.py:66-70)."""
    rows = x.reshape(x.shape[0], -1)
    scale = rows.abs().amax(dim=1) + eps
    return scale * (rows / scale[:, None]).abs().pow(p).sum(dim=1).pow(1.0 / p)


def _check_supported(system, star_penalty):
    enc, rec = getattr(system, 'encoder', None), getattr(system, 'recognizer', None)
    if type(enc) is not Encoder or type(rec) is not TemporalClassifier:
        raise NotImplementedError('haloop_amd.grad_norm.gradient_norms is built for rnn.Encoder + recognizer.TemporalClassifier (the LSTM-CTC '
                                  f'model); got {type(enc).__name__} + {type(rec).__name__}: the transformer family and the Transducer '
                                  'head have no per-utterance gradient-norm path')
    if star_penalty is not None:
        raise NotImplementedError('haloop_amd.grad_norm.gradient_norms: the star-CTC loss (star_penalty) has no per-utterance '
                                  'gradient-norm path; only the plain CTC loss of rnn.Encoder + TemporalClassifier is built')
    return enc, rec


def _split_terms(tm):
    """A term's parameters one by one: (a, b_j, no bias) per operand, then (a, no operand, one bias)."""
    out = []
    for j in range(tm.n_b):
        t = _lib.GhostTerm()
        t.a, t.n_b, t.n_bias = tm.a, 1, 0
        t.b[0] = tm.b[j]
        t.tensors = tm.tensors
        out.append(t)
    if tm.n_bias:
        t = _lib.GhostTerm()
        t.a, t.n_b, t.n_bias = tm.a, 0, 1
        t.tensors = tm.tensors
        out.append(t)
    return out


def _backward_terms(system, inputs, condtargets, input_lengths, condtarget_lengths, star_penalty=None):
    """One forward and one backward of sum_n loss_n on the operators -> (terms for ops.ghost_sqnorm, L, N, T', losses [N])."""
    enc, rec = _check_supported(system, star_penalty)
    system.train()
    if not inputs.is_cuda:
        raise _lib.HaloError('haloop_amd.grad_norm.gradient_norms runs on the HIP device only (no CPU path)')
    dev = inputs.device
    p_conv, p_lstm = enc.dropout.p, float(enc.lstm.dropout)
    L = enc.lstm.num_layers
    if p_conv != p_lstm and p_conv > 0 and p_lstm > 0 and L > 1:
        raise NotImplementedError('subsample and inter-layer dropout rates must agree (both 0.2 in ha/rnn.py)')
    params = [p.detach() for p in lstm_param_list(enc.lstm)]
    w_ih, w_hh, b_ih, b_hh = params[0::4], params[1::4], params[2::4], params[3::4]
    H = w_hh[0].shape[1]
    conv_w, conv_b = enc.subsample.weight.detach(), enc.subsample.bias.detach()
    cls_w, cls_b = rec.classifier.weight.detach(), rec.classifier.bias.detach()
    V = cls_w.shape[0]
    x = inputs.float().contiguous()
    B = x.shape[0]
    # 1. conv front end and LSTM (the forward of functional._Encoder)
    drop = enc.dropout_stream.next(max(p_conv, p_lstm), True)
    y_sub, col = ops.subsample_fwd(x, conv_w, conv_b, drop)
    Tp = y_sub.shape[0]
    feats = torch.empty(B, Tp, H, device=dev, dtype=torch.float32)
    _, _, _, reserve = ops.lstm_fwd(y_sub, w_ih, w_hh, b_ih, b_hh, y=feats, y_strides=(H, Tp * H), y_relu=True, drop=drop)
    flen = enc.subsampled_lengths(input_lengths.to(dev))
    # 2. dropout, head product, log-softmax, CTC (TemporalClassifier.forward)
    cdrop = rec.dropout_stream.next(rec.dropout.p, True)
    fd = feats if cdrop.p <= 0.0 else ops.dropout_fwd(feats, cdrop, _lib.HALO_STREAM_CLASSIFIER)
    logits = ops.gemm(fd.view(B * Tp, H), cls_w, True, True, B * Tp, V, H, bias1=cls_b)
    lp = ops.log_softmax_fwd(logits).view(B, Tp, V)
    tl = condtarget_lengths.to(dev)
    nll, alpha, saved = ops.ctc_fwd(lp, False, condtargets.to(dev), flen, tl, flags=0)
    per_row = 1.0 / tl.to(torch.float32).clamp_min(1)
    losses = nll * per_row
    # 3. d loss_n / d log-probs, d logits: the head's `a`
    dlp = ops.ctc_bwd(lp, False, saved, alpha, nll, per_row)
    dlogits = ops.log_softmax_bwd(dlp.view(B * Tp, V), lp.view(B * Tp, V))
    # 4. the head's input gradient
    dfeats = ops.gemm(dlogits, cls_w, True, False, B * Tp, H, V)
    if cdrop.p > 0.0:
        dfeats = ops.dropout_fwd(dfeats, cdrop, _lib.HALO_STREAM_CLASSIFIER)
    # 5. the LSTM backward, its gate gradients kept in the reserve
    keep = _lib.get_lstm_keep_gate_gradients()
    _lib.set_lstm_keep_gate_gradients(True)
    try:
        dy_sub, _ = ops.lstm_bwd(y_sub, w_ih, w_hh, dfeats, (H, Tp * H), True, reserve, want_dx=True, drop=drop)
        lstm_terms = ops.lstm_ghost_terms(y_sub, reserve, H, L, drop.p)
    finally:
        _lib.set_lstm_keep_gate_gradients(keep)
    # 6. the gradient at the convolution's pre-activation; its operand is the im2col image
    dpre = ops.relu_dropout_bwd(dy_sub, y_sub, drop.p)
    conv_term = ops.ghost_term(dpre, (col.view(Tp, B, -1),), n_bias=1, time_major=True)
    head_term = ops.ghost_term(dlogits.view(B, Tp, V), (fd.view(B, Tp, H),), n_bias=1)
    return [conv_term] + lstm_terms + [head_term], L, B, Tp, losses


def gradient_norms(system, inputs, condtargets, input_lengths, condtarget_lengths, per_parameter=False, star_penalty=None):
    """-> (norms [N], losses [N]) [, {state-dict name: squared norm [N]} when ``per_parameter``].

    loss_n is the recognizer's loss of utterance n as a batch of one (TemporalClassifier: nll_n / max(target_length_n, 1)) and
    norm_n = sqrt(sum_p ||d loss_n / d p||^2) over every parameter of encoder and recognizer -- what ``norm_batched`` of the
    per-parameter ``norm_batched``s evaluates to.  Like the reference (ha/grad_norm.py:85) the call puts the system in training mode
    ("test time dropout") and draws from the modules' DropoutStreams; it runs the operators directly, not autograd, and leaves no
    ``.grad`` anywhere.  The weight gradients the LSTM backward forms along the way are discarded."""
    with torch.no_grad():
        terms, L, N, Tp, losses = _backward_terms(system, inputs, condtargets, input_lengths, condtarget_lengths, star_penalty)
        _, norms = ops.ghost_sqnorm(terms, N, Tp, want_norm=True)
        if not per_parameter:
            return norms, losses
        names = ['encoder.subsample.weight', 'encoder.subsample.bias']
        for l in range(L):
            names += [f'encoder.lstm.weight_ih_l{l}', f'encoder.lstm.weight_hh_l{l}', f'encoder.lstm.bias_ih_l{l}']
        names += ['recognizer.classifier.weight', 'recognizer.classifier.bias']
        split = [s for tm in terms for s in _split_terms(tm)]
        sq = ops.ghost_sqnorm(split, N, Tp)
        per = {name: sq[i] for i, name in enumerate(names)}
        for l in range(L):      # both bias vectors of a layer receive sum_t dG_t
            per[f'encoder.lstm.bias_hh_l{l}'] = per[f'encoder.lstm.bias_ih_l{l}']
        return norms, losses, per


def compute_grad_norm(system, loader):
    """The loop of `hac --grad-norms` (ha/grad_norm.py:28-49): one ``grad_norm,loss`` line per utterance of every batch the loader yields
    as (dataset_indices, inputs, condtargets, input_lengths, condtarget_lengths)."""
    device = next(system.encoder.parameters()).device
    system.train()
    for dataset_indices, inputs, condtargets, input_lengths, condtarget_lengths in loader:
        norms, losses = gradient_norms(system, inputs.to(device), condtargets.to(device), input_lengths.to(device),
                                       condtarget_lengths.to(device).long())
        for index, norm, loss in zip(torch.as_tensor(dataset_indices).tolist(), norms.tolist(), losses.tolist()):
            print('grad_norm,loss', index, norm, loss, sep='\t', flush=True)
