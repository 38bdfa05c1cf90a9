"""Float64 restatement, on the CPU in plain torch, of the carried greedy transducer search (haloop_amd.transducer.GreedyStream,
DESIGN.md 3.3x), built on ``rnnt_greedy_ref.modules``, and the chunk schedules that tests/test_rnnt_stream_cpu.py and
tests/test_gpu_rnnt_stream.py share.  No tests in here.

Per row the search keeps the prediction network's LSTM state, g, t (frames of the stream consumed), u, here, the score, tokens,
frames and truncated.  ``begin`` resets a row; ``advance`` gives every row the first n_frames[n] frames of a chunk of logits and goes on
where the row stood:

    while frames of the chunk are left and the row is not truncated:
        lp = log_softmax(F[n, pos] + g)
        k = 0 if here == max_symbols_per_frame else argmax(lp)           # lowest index among equal maxima
        score += lp[k]
        if k == 0: t += 1; pos += 1; here = 0
        else:      tokens[u] = k; frames[u] = t; u += 1; here += 1; g = out_layer(lstm_step(embedding[k], state))
                   truncated = u == capacity                             # sticky until the row begins again

A row that runs out of the chunk's frames waits.  The rounds of a call are the advance launches the device needs until no row is live:
a row is live after a round in which it emitted without truncating, so a row that takes part needs its emissions of the call plus one
round to run out, a row that truncates in the call exactly its emissions, and the call the most any row needs.
"""
import torch

import rnnt_greedy_ref as R


def logits(sd, features):
    """classifier(features) in float64: [N, T, V]."""
    _, _, _, cw, cb = R.modules(sd)
    return torch.nn.functional.linear(features.double(), cw, cb)


class GreedyStreamRef:
    def __init__(self, sd, n_rows, capacity, max_symbols_per_frame=10):
        self.lstm, self.emb, self.ob, _, _ = R.modules(sd)
        self.N, self.capacity, self.max_symbols = n_rows, capacity, max_symbols_per_frame
        self.rows = [None] * n_rows
        self.tokens = torch.full((n_rows, capacity), -1, dtype=torch.int64)
        self.frames = torch.full((n_rows, capacity), -1, dtype=torch.int64)
        self.calls = []          # per advance: dict(rounds, emitted [N], took_part [N], truncated_here [N], forced [N])
        self.gap = float('inf')  # the smallest gap of a free argmax over everything visited

    def _step(self, k, state):
        out, state = self.lstm(self.emb[k].view(1, 1, R.E), state)
        return torch.nn.functional.linear(out.view(R.E), self.emb, self.ob), state

    @torch.no_grad()
    def begin(self, n):
        z = lambda: torch.zeros(R.LAYERS, 1, R.E, dtype=torch.float64)
        g, state = self._step(0, (z(), z()))
        self.rows[n] = dict(state=state, g=g, t=0, u=0, here=0, score=torch.zeros((), dtype=torch.float64), truncated=False)
        self.tokens[n] = -1
        self.frames[n] = -1

    @torch.no_grad()
    def advance(self, F, n_frames, begin=None):
        """F [B, S, V] float64 logits of this call's chunk, n_frames: B ints (clipped to 0 .. S), begin: B bools or None."""
        B, S, _ = F.shape
        emitted, took, trunc_here, forced = [0] * self.N, [False] * self.N, [False] * self.N, [0] * self.N
        rounds = 0
        for n in range(B):
            if begin is not None and begin[n]:
                self.begin(n)
            r = self.rows[n]
            L = max(0, min(int(n_frames[n]), S))
            if r is None or L == 0 or r['truncated']:
                continue
            took[n] = True
            pos = 0
            while pos < L and not r['truncated']:
                lp = (F[n, pos] + r['g']).log_softmax(-1)
                if r['here'] == self.max_symbols:
                    k = 0
                    forced[n] += 1
                else:
                    k = int((lp == lp.max()).nonzero()[0])
                    top = lp.topk(2).values
                    self.gap = min(self.gap, float(top[0] - top[1]))
                r['score'] = r['score'] + lp[k]
                if k == 0:
                    r['t'], pos, r['here'] = r['t'] + 1, pos + 1, 0
                else:
                    self.tokens[n, r['u']], self.frames[n, r['u']] = k, r['t']
                    r['u'], r['here'] = r['u'] + 1, r['here'] + 1
                    emitted[n] += 1
                    r['g'], r['state'] = self._step(k, r['state'])
                    if r['u'] == self.capacity:
                        r['truncated'] = trunc_here[n] = True
            rounds = max(rounds, emitted[n] + (0 if trunc_here[n] else 1))
        self.calls.append(dict(rounds=rounds, emitted=emitted, took_part=took, truncated_here=trunc_here, forced=forced))
        return rounds

    def result(self):
        """-> dict(tokens, lengths, frames, scores (float64), truncated) in ``rnnt_greedy_ref.greedy``'s format; a row never begun is empty."""
        rows = [r or dict(u=0, score=torch.zeros((), dtype=torch.float64), truncated=False) for r in self.rows]
        return dict(tokens=self.tokens.clone(), frames=self.frames.clone(), lengths=torch.tensor([r['u'] for r in rows]),
                    scores=torch.stack([r['score'] for r in rows]), truncated=torch.tensor([r['truncated'] for r in rows]))


# ---- schedules: a plan is a list of calls, a call the list of frame counts the rows get; row n's frames are consecutive from its cursor ----
SCHEDULES = ('ones', 'fours', 'mixed', 'whole', 'staggered')


def plan(kind, lengths, T):
    """lengths: the rows' frame counts (clipped to T).  'ones' / 'fours': chunks of 1 / 4 over 0 .. T; 'mixed': chunks of 5, 1, 7, 7, ...;
    'whole': one chunk of T -- a row takes part in a call while it has frames left.  'staggered': chunks of up to 4 in which row n gets
    no frames in call j when (j + n) % 3 == 0 and its frames shift later (rows pause and resume), until every row is through."""
    lengths = [max(0, min(int(l), T)) for l in lengths]
    if kind == 'staggered':
        left, calls, j = list(lengths), [], 0
        while any(left):
            counts = [0 if (j + n) % 3 == 0 else min(4, l) for n, l in enumerate(left)]
            left = [l - c for l, c in zip(left, counts)]
            calls.append(counts)
            j += 1
        return calls
    sizes = {'ones': [1] * T, 'fours': [4] * ((T + 3) // 4), 'whole': [T], 'mixed': [5, 1] + [7] * ((T + 6) // 7)}[kind]
    calls, a = [], 0
    for s in sizes:
        if a >= T:
            break
        s = min(s, T - a)
        calls.append([max(0, min(l - a, s)) for l in lengths])
        a += s
    return calls


def chunk(F, cursors, counts, fill=0.0):
    """The call's chunk [B, S, V] of F [B, T, V]: row n holds its frames [cursors[n], cursors[n] + counts[n]), ``fill`` everywhere else
    (the frames at or past its count, and every frame of a row that does not take part); S = max(counts), at least 1."""
    B, _, V = F.shape
    S = max(1, max(counts))
    out = F.new_full((B, S, V), fill)
    for n, (a, c) in enumerate(zip(cursors, counts)):
        out[n, :c] = F[n, a:a + c]
    return out


# ---- the streamed encoder in front of the search: 3.3v's fast-path shape under a transducer head ----
FAST = dict(F_=80, C=128, H=1024, L=2, V=32, B=5, T=80, chunk=16, lengths=[80, 80, 80, 80, 57], capacity=24,
            enc_seed=42, x_seed=43, head_seed=726, weight_scale=100.0)


def _logits_stream_ref():
    import stream_ref
    from oracle import cpu_ref

    class LogitsStreamRef(stream_ref.StreamRef):
        """``stream_ref.StreamRef`` with the transducer's transcription head behind the encoder: a call's steps -> logits, no softmax."""

        def _steps(self, b, x_in, keep_state):
            r = self.rows[b]
            x = torch.nn.functional.conv1d(x_in.t()[None], self.enc['subsample.weight'], self.enc['subsample.bias'],
                                           stride=cpu_ref.CONV_STRIDE).mT.relu()
            new_state = []
            for k in range(self.L):
                x, st = cpu_ref._lstm_layer(x, self.enc[f'lstm.weight_ih_l{k}'], self.enc[f'lstm.weight_hh_l{k}'],
                                            self.enc[f'lstm.bias_ih_l{k}'], self.enc[f'lstm.bias_hh_l{k}'], r['state'][k])
                new_state.append(st)
            if keep_state:
                r['state'] = new_state
            f = torch.nn.functional.linear(x.relu(), self.rec['classifier.weight'], self.rec['classifier.bias'])[0]
            r['lp'].append(f)
            return f
    return LogitsStreamRef


def head_state(feat, V, seed, weight_scale=1.0):
    """A random-initialised Transducer's state dict with the fixtures' raised blank bias (rnnt_greedy_ref.fixture's recipe);
    ``weight_scale`` multiplies the classifier's weight (tests/test_gpu_streaming.py's fast case does the same to its CTC head: the
    features of a random LC-2x1024 are small, and unscaled no frame's argmax ever leaves the blank)."""
    from haloop_amd import recognizer
    saved = torch.get_rng_state()
    torch.manual_seed(seed)
    head = recognizer.Transducer(feat, V).eval()
    torch.set_rng_state(saved)
    sd = {k: v.detach().clone() for k, v in head.state_dict().items()}
    sd['classifier.bias'][0] += 2.0
    sd['classifier.weight'] *= weight_scale
    return sd


_fast = {}


def fast_case(head_seed=None):
    """-> dict(enc_p, sd, x, calls: stream_ref.schedule's, logits: per row the float64 logits [steps, V] of the chunked encoder, search:
    the float64 carried search on them (result dict), gap, per_call: the search's result after every call).  Computed once per process;
    callers must not modify what they get."""
    import stream_ref
    from oracle import cpu_ref
    c = FAST
    seed = c['head_seed'] if head_seed is None else head_seed
    if seed in _fast:
        return _fast[seed]
    enc_p, _ = cpu_ref.make_params(c['F_'], c['C'], c['H'], c['L'], c['V'], seed=c['enc_seed'])
    sd = head_state(c['H'], c['V'], seed, c['weight_scale'])
    x = 8 * torch.randn(c['B'], c['T'], c['F_'], generator=torch.Generator().manual_seed(c['x_seed']))
    rec = {'classifier.weight': sd['classifier.weight'], 'classifier.bias': sd['classifier.bias']}
    enc = _logits_stream_ref()(enc_p, rec, c['B'], torch.float64)
    search = GreedyStreamRef(sd, c['B'], c['capacity'], R.MAX_SYMBOLS)
    calls, per_call = stream_ref.schedule(c['lengths'], c['chunk']), []
    for call in calls:
        before = [0 if r is None else len(r['lp']) for r in enc.rows]
        if call[0] == 'push':
            _, k, active = call
            begin = [a and k == 0 for a in active]
            enc.push(x[:, k * c['chunk']:(k + 1) * c['chunk']], active, begin)
            rows = active
        else:
            _, rows, tails = call
            begin = None
            enc.finish(stream_ref.tail_tensor(x, c['lengths'], c['chunk'], rows, tails), tails, rows)
        new = [enc.rows[b]['lp'][before[b]] if rows[b] else None for b in range(c['B'])]
        counts = [0 if f is None else f.shape[0] for f in new]
        F = torch.zeros(c['B'], max(1, max(counts)), c['V'], dtype=torch.float64)
        for b, f in enumerate(new):
            if f is not None:
                F[b, :counts[b]] = f
        search.advance(F, counts, begin)
        per_call.append(search.result())
    _fast[seed] = dict(enc_p=enc_p, sd=sd, x=x, calls=calls, logits=[enc.log_probs(b) for b in range(c['B'])], search=search.result(),
                       gap=search.gap, per_call=per_call, stats=search.calls)
    return _fast[seed]
