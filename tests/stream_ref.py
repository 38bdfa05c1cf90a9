"""CPU restatement of streamed LSTM-CTC recognition (haloop_amd/streaming.py) with the pieces of oracle/cpu_ref.py: F.conv1d on
[carry | chunk], ``_lstm_layer`` with a carried state, ``classifier_log_probs`` and a Python collapse.  Every stream is computed on its
own (no batching, no masking), in the dtype of the parameters it is given: float32 or float64.  TEST INFRASTRUCTURE ONLY."""
import torch
import torch.nn.functional as F

from oracle import cpu_ref


def finish_steps(tail_length):
    """Steps of the convolution over [3 carry | tail | 3 zeros]: floor((tl + 6 - 5) / 4) + 1."""
    return (tail_length + 1) // 4 + 1


def schedule(lengths, chunk_frames):
    """The calls that stream utterances of ``lengths`` frames through one slot each: a list of ('push', k, active) -- every active row
    sends its frames [k * chunk, (k + 1) * chunk), rows begin at k == 0 -- and ('finish', rows, tails) -- row b sends its last tails[b]
    frames, from (lengths[b] // chunk) * chunk on.  A row is finished right after its last push while the others go on."""
    n_push = [t // chunk_frames for t in lengths]
    assert min(n_push) >= 1, 'a stream begins with a push'
    calls = []
    for k in range(max(n_push)):
        calls.append(('push', k, [n > k for n in n_push]))
        rows = [n == k + 1 for n in n_push]
        if any(rows):
            calls.append(('finish', rows, [t % chunk_frames if r else 0 for t, r in zip(lengths, rows)]))
    return calls


def collapse(labels, last=-1):
    """Greedy CTC collapse of a label sequence continued from ``last``: repeats merged, blanks dropped -> (tokens, new last)."""
    out = []
    for lab in labels:
        if lab != last and lab != 0:
            out.append(lab)
        last = lab
    return out, last


class StreamRef:
    def __init__(self, enc, rec, n_streams, dtype=torch.float32):
        self.enc = {k: v.to(dtype) for k, v in enc.items()}
        self.rec = {k: v.to(dtype) for k, v in rec.items()}
        self.dtype, self.L = dtype, cpu_ref.num_lstm_layers(enc)
        self.F = enc['subsample.weight'].shape[1]
        self.H = enc['lstm.weight_hh_l0'].shape[1]
        self.rows = [None] * n_streams

    def _begin(self, b):
        z = lambda: torch.zeros(1, 1, self.H, dtype=self.dtype)
        self.rows[b] = dict(carry=torch.zeros(3, self.F, dtype=self.dtype), state=[(z(), z()) for _ in range(self.L)], last=-1, hyp=[],
                            score=0.0, lp=[], ali=[])

    def _steps(self, b, x_in, keep_state):
        """x_in [rows, F] -> the log-probs [n, V] of its steps; appends to the row's record."""
        r = self.rows[b]
        x = F.conv1d(x_in.t()[None], self.enc['subsample.weight'], self.enc['subsample.bias'], stride=cpu_ref.CONV_STRIDE).mT.relu()
        new_state = []
        for k in range(self.L):
            x, st = cpu_ref._lstm_layer(x, self.enc[f'lstm.weight_ih_l{k}'], self.enc[f'lstm.weight_hh_l{k}'],
                                        self.enc[f'lstm.bias_ih_l{k}'], self.enc[f'lstm.bias_hh_l{k}'], r['state'][k])
            new_state.append(st)
        if keep_state:
            r['state'] = new_state
        lp = cpu_ref.classifier_log_probs(self.rec, x.relu())[0]
        best, ali = lp.max(-1)
        tokens, r['last'] = collapse(ali.tolist(), r['last'])
        r['hyp'] += tokens
        for v in best.tolist():
            r['score'] += v
        r['lp'].append(lp)
        r['ali'] += ali.tolist()
        return lp

    @torch.no_grad()
    def push(self, frames, active, begin):
        """frames [B, chunk, F]; active / begin: sequences of bools."""
        for b, (a, g) in enumerate(zip(active, begin)):
            if not a:
                continue
            if g:
                self._begin(b)
            chunk = frames[b].to(self.dtype)
            self._steps(b, torch.cat([self.rows[b]['carry'], chunk]), True)
            self.rows[b]['carry'] = chunk[-3:].clone()

    @torch.no_grad()
    def finish(self, tail, tail_lengths, rows):
        for b, r in enumerate(rows):
            if r:
                t = tail[b, :tail_lengths[b]].to(self.dtype)
                self._steps(b, torch.cat([self.rows[b]['carry'], t, torch.zeros(3, self.F, dtype=self.dtype)]), False)

    def log_probs(self, b):
        return torch.cat(self.rows[b]['lp'])


def stream_all(ref, x, lengths, chunk_frames):
    """Stream x[b, :lengths[b]] through slot b of ``ref`` by ``schedule``."""
    for call in schedule(lengths, chunk_frames):
        if call[0] == 'push':
            _, k, active = call
            ref.push(x[:, k * chunk_frames:(k + 1) * chunk_frames], active, [a and k == 0 for a in active])
        else:
            _, rows, tails = call
            ref.finish(tail_tensor(x, lengths, chunk_frames, rows, tails), tails, rows)
    return ref


def tail_tensor(x, lengths, chunk_frames, rows, tails):
    """[B, max tail, F]: row b's last tails[b] frames (zeros elsewhere)."""
    tail = x.new_zeros(x.shape[0], max(tails), x.shape[2])
    for b, (r, tl) in enumerate(zip(rows, tails)):
        if r and tl:
            t0 = (lengths[b] // chunk_frames) * chunk_frames
            tail[b, :tl] = x[b, t0:t0 + tl]
    return tail
