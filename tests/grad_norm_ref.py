"""Per-utterance losses, gradients and gradient norms of the LSTM-CTC model on the CPU, for the tests of haloop_amd.grad_norm.

``per_utterance`` is the oracle: one batch forward through oracle.cpu_ref (the rows of a batch are independent), then one
``torch.autograd.grad(loss_n, params)`` per utterance, in float32 or float64.  ``term_table`` restates the same model with an explicit
LSTM cell so that the back-propagated signals the library reads from its own buffers (the gradient at the conv's pre-activation, every
layer's gate gradients, the logit gradients) and their partners (im2col rows, layer inputs, previous hidden states, dropped features)
exist as tensors: the Gram form over that table must reproduce the oracle's norms.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import cpu_ref


def norm_batched(x, p=2.0, eps=1e-6):
    """The formula of ha/grad_norm.py:66-70 restated: rows scaled by their largest magnitude + eps, p-norm, scaled back."""
    rows = x.reshape(x.shape[0], -1)
    scale = rows.abs().max(dim=1).values + eps
    return scale * ((rows / scale[:, None]).abs() ** p).sum(dim=1) ** (1.0 / p)


def _cast(d, dtype):
    return OrderedDict((k, v.detach().to(dtype).requires_grad_(True)) for k, v in d.items())


def per_utterance_losses(enc, rec, x, il, tg, tl, masks=None):
    feats, flen, _ = cpu_ref.encoder_forward(enc, x, il, masks)
    lp = cpu_ref.classifier_log_probs(rec, feats, None if masks is None else masks['classifier']).permute(1, 0, 2)
    nll = F.ctc_loss(lp, tg, flen.long(), tl, reduction='none')
    return nll / tl.clamp_min(1).to(nll.dtype)


def per_utterance(enc_p, rec_p, x, il, tg, tl, masks=None, dtype=torch.float64):
    """-> dict(norms [N], losses [N], sq {state-dict name: [N] float64}) computed in ``dtype``."""
    enc, rec = _cast(enc_p, dtype), _cast(rec_p, dtype)
    if masks is not None:
        masks = {k: v.to(dtype) for k, v in masks.items()}
    losses = per_utterance_losses(enc, rec, x.to(dtype), il, tg, tl, masks)
    names = ['encoder.' + k for k in enc] + ['recognizer.' + k for k in rec]
    params = list(enc.values()) + list(rec.values())
    rows = [torch.autograd.grad(losses[n], params, retain_graph=True) for n in range(x.shape[0])]
    stacked = [torch.stack([rows[n][i] for n in range(len(rows))]) for i in range(len(params))]        # per parameter [N, ...]
    norms = norm_batched(torch.stack([norm_batched(g) for g in stacked]).T)
    sq = {name: g.double().reshape(g.shape[0], -1).square().sum(dim=1) for name, g in zip(names, stacked)}
    return dict(norms=norms.detach(), losses=losses.detach(), sq=sq)


def im2col(x, ks=cpu_ref.CONV_KERNEL, stride=cpu_ref.CONV_STRIDE, pad=cpu_ref.CONV_PAD):
    """x [B, T, F] -> [B, T', F * ks], column f * ks + k = padded frame t' * stride + k of feature f (the conv weight [C, F, ks] flattened)."""
    return F.unfold(F.pad(x.mT, (pad, pad)).unsqueeze(2), (1, ks), stride=(1, stride)).mT


def term_table(enc_p, rec_p, x, il, tg, tl, masks=None, dtype=torch.float64):
    """-> (terms, losses): terms is a list of (names, a, [b...], n_bias) with a / b batch-first [N, T', K]; names are the state-dict names of
    the parameters the term covers.  One backward of sum_n loss_n."""
    enc, rec = _cast(enc_p, dtype), _cast(rec_p, dtype)
    x = x.to(dtype)
    L = cpu_ref.num_lstm_layers(enc)
    m = (lambda k: None) if masks is None else (lambda k: masks[k].to(dtype))
    kept = []

    def keep(t):
        t.retain_grad()
        kept.append(t)
        return t

    col = im2col(x)
    pre = keep(col @ enc['subsample.weight'].reshape(enc['subsample.weight'].shape[0], -1).T + enc['subsample.bias'])
    h = pre.relu()
    if masks is not None:
        h = h * m('subsample')
    table = [(['encoder.subsample.weight', 'encoder.subsample.bias'], pre, [col], 1)]
    B, Tp = h.shape[0], h.shape[1]
    inp = h
    for l in range(L):
        w_ih, w_hh = enc[f'lstm.weight_ih_l{l}'], enc[f'lstm.weight_hh_l{l}']
        b_ih, b_hh = enc[f'lstm.bias_ih_l{l}'], enc[f'lstm.bias_hh_l{l}']
        H = w_hh.shape[1]
        hs, c, gates = [x.new_zeros(B, H)], x.new_zeros(B, H), []
        for t in range(Tp):
            g = keep(inp[:, t] @ w_ih.T + hs[-1] @ w_hh.T + b_ih + b_hh)
            gates.append(g)
            i, f, gg, o = g.chunk(4, dim=1)
            c = f.sigmoid() * c + i.sigmoid() * gg.tanh()
            hs.append(o.sigmoid() * c.tanh())
        table.append(([f'encoder.lstm.weight_ih_l{l}', f'encoder.lstm.weight_hh_l{l}', f'encoder.lstm.bias_ih_l{l}', f'encoder.lstm.bias_hh_l{l}'],
                      gates, [inp.detach(), torch.stack(hs[:-1], dim=1).detach()], 2))
        out = torch.stack(hs[1:], dim=1)
        if l < L - 1 and masks is not None:          # the layer above reads the DROPPED output
            out = out * m(f'lstm{l}')
        inp = out
    feats = inp.relu()
    if masks is not None:
        feats = feats * m('classifier')
    logits = keep(feats @ rec['classifier.weight'].T + rec['classifier.bias'])
    table.append((['recognizer.classifier.weight', 'recognizer.classifier.bias'], logits, [feats.detach()], 1))
    flen = cpu_ref.subsampled_lengths(il)
    nll = F.ctc_loss(logits.log_softmax(dim=-1).permute(1, 0, 2), tg, flen.long(), tl, reduction='none')
    losses = nll / tl.clamp_min(1).to(dtype)
    losses.sum().backward()
    terms = []
    for names, a, bs, n_bias in table:
        a = torch.stack([g.grad for g in a], dim=1) if isinstance(a, list) else a.grad
        terms.append((names, a.detach(), [b.detach() for b in bs], n_bias))
    return terms, losses.detach()
