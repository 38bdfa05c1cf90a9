"""Float64 restatement, on the CPU in plain torch, of the carried transducer beam search (haloop_amd.transducer.BeamStream, DESIGN.md
3.3aa) on ``rnnt_beam_ref``'s modules and fixtures, and the call scripts that tests/test_rnnt_beam_stream_cpu.py and
tests/test_gpu_rnnt_beam_stream.py share.  No tests in here.

The search is ``rnnt_beam_ref.beam_row``'s, entered from a kept beam.  At alignment step i hypothesis j stands at frame
t_j = i - len(y_j), and a step depends on the row's length L only through t_j < L and t_j + 1 == L.  With R frames received

    a row executes step i  iff  its beam is not empty and (max_j t_j + 1 < R or the row is final)

with L = R when it is final and "L greater than R" otherwise: every frame read has arrived and no blank extension is complete.
Otherwise the row stalls and keeps its beam.  The executed steps are those of the whole search over the complete utterance.
"""
import torch

import rnnt_beam_ref as BR
import rnnt_greedy_ref as G
import rnnt_stream_ref as SR

E = G.E


class BeamStreamRef:
    def __init__(self, sd, n_rows, capacity, W):
        self.lstm, self.emb, self.ob, _, _ = G.modules(sd)
        self.N, self.capacity, self.W = n_rows, capacity, W
        self.rows = [None] * n_rows
        self.calls = []          # per advance: dict(executed [N]: steps of the call, stalled [N]: open with a beam after it, old_reads [N])
        self.reach = 0           # the most any step read behind the frames received: max R - t
        self.spread = 0          # max_j t_j - min_j t_j over every executed step

    def _lm(self, k, state):
        out, state = self.lstm(self.emb[k].view(1, 1, E), state)
        return torch.nn.functional.linear(out.view(E), self.emb, self.ob), state

    @torch.no_grad()
    def begin(self, n):
        z = lambda: torch.zeros(G.LAYERS, 1, E, dtype=torch.float64)
        g0, state0 = self._lm(0, (z(), z()))
        self.rows[n] = dict(beam=[((), 0.0, g0, state0)], finals=[], step=0, R=0, final=False, closed=False, frames=[], gap=float('inf'))

    @staticmethod
    def runnable(r):
        if r['closed'] or not r['beam']:
            return False
        return r['final'] or r['step'] - min(len(y) for y, _, _, _ in r['beam']) + 1 < r['R']

    def _step(self, r, R_old):
        """One alignment step of ``rnnt_beam_ref.beam_row`` -> the frames it read that arrived before this call."""
        W, cap, V = self.W, self.capacity, self.emb.shape[0]
        beam, i, R = r['beam'], r['step'], r['R']
        L = R if r['final'] else R + 1
        lps, old = [], 0
        ts = [i - len(y) for y, _, _, _ in beam]
        self.spread = max(self.spread, max(ts) - min(ts))
        for (y, s, g, state), t in zip(beam, ts):
            assert 0 <= t < R
            old += t < R_old
            self.reach = max(self.reach, R - t)
            lps.append((r['frames'][t] + g).log_softmax(-1))
        cands = []                                           # [tokens, score, parent j, k]
        for j, (y, s, g, state) in enumerate(beam):
            if ts[j] + 1 == L:
                r['finals'].append((y, s + float(lps[j][0])))
            else:
                cands.append([y, s + float(lps[j][0]), j, 0])
        for j, (y, s, g, state) in enumerate(beam):
            if len(y) < cap:
                lp = lps[j].tolist()
                for k in range(1, V):
                    cands.append([y + (k,), s + lp[k], j, k])
        first, merged = {}, []
        for c in cands:
            at = first.get(c[0])
            if at is None:
                first[c[0]] = len(merged)
                merged.append(c)
            else:
                m = merged[at]
                m[1] = float(torch.logaddexp(torch.tensor(m[1], dtype=torch.float64), torch.tensor(c[1], dtype=torch.float64)))
        order = sorted(range(len(merged)), key=lambda a: (-merged[a][1], a))
        if len(merged) > W:
            r['gap'] = min(r['gap'], merged[order[W - 1]][1] - merged[order[W]][1])
        new = []
        for a in order[:W]:
            y, s, j, k = merged[a]
            if k == 0:
                new.append((y, s, beam[j][2], beam[j][3]))
            else:
                g, state = self._lm(k, beam[j][3])
                new.append((y, s, g, state))
        r['beam'], r['step'] = new, i + 1
        if not new and r['final']:
            r['closed'] = True
        return old

    @torch.no_grad()
    def advance(self, F, n_frames, begin=None, final=None):
        """F [B, S, V] float64 logits of this call's chunk, n_frames: B ints (clipped to 0 .. S), begin / final: B bools or None ->
        the rounds the call needs: the most steps any row executes in it."""
        B, S, _ = F.shape
        executed, old_reads = [0] * self.N, [0] * self.N
        for n in range(B):
            if begin is not None and begin[n]:
                self.begin(n)
            r = self.rows[n]
            if r is None or r['closed'] or r['final']:
                continue
            L = max(0, min(int(n_frames[n]), S))
            R_old = r['R']
            r['frames'] += list(F[n, :L].unbind(0))
            r['R'] += L
            if final is not None and final[n]:
                r['final'] = True
                if r['R'] == 0:
                    r.update(beam=[], finals=[((), 0.0)], closed=True)
            while self.runnable(r):
                old_reads[n] += self._step(r, R_old)
                executed[n] += 1
        stalled = [r is not None and not r['closed'] and bool(r['beam']) for r in self.rows]
        self.calls.append(dict(rounds=max(executed), executed=executed, stalled=stalled, old_reads=old_reads))
        return max(executed)

    def hypotheses(self, n):
        """Row n -> (closed, [(tokens tuple, score)]): a closed row's finals by (score descending, order of completion), all of them;
        an open row's beam in slot order.  A row that never began is closed with no finals."""
        r = self.rows[n]
        if r is None:
            return True, []
        if r['closed']:
            fin = r['finals']
            return True, [fin[a] for a in sorted(range(len(fin)), key=lambda a: (-fin[a][1], a))]
        return False, [(y, s) for y, s, _, _ in r['beam']]

    def nbest(self):
        """-> dict(tokens [N, W, capacity], lengths [N, W], scores [N, W] float64, counts [N]) in ``rnnt_beam_ref.beam_search``'s format."""
        N, W, cap = self.N, self.W, self.capacity
        tokens = torch.full((N, W, cap), -1, dtype=torch.int64)
        lengths = torch.full((N, W), -1, dtype=torch.int64)
        scores = torch.full((N, W), float('-inf'), dtype=torch.float64)
        for n in range(N):
            for w, (y, s) in enumerate(self.hypotheses(n)[1][:W]):
                lengths[n, w], scores[n, w] = len(y), s
                tokens[n, w, :len(y)] = torch.tensor(y, dtype=torch.int64)
        return dict(tokens=tokens, lengths=lengths, scores=scores, counts=(lengths >= 0).sum(1))


# ---- scripts: a script is a list of calls (counts, begin, final), one entry per row each.  The frames follow ``rnnt_stream_ref.plan``;
#      every row begins in call 0; an even row is final in the call that brings its last frame (a row of no frames: in call 0, with its
#      begin), an odd row in one more call at the end that brings no frames. ----
SCHEDULES = ('ones', 'fours', 'mixed', 'staggered')


def script(kind, lengths, T):
    lengths = [max(0, min(int(l), T)) for l in lengths]
    N = len(lengths)
    cur, done, out = [0] * N, [False] * N, []
    for j, counts in enumerate(SR.plan(kind, lengths, T)):
        cur = [a + c for a, c in zip(cur, counts)]
        final = [n % 2 == 0 and not done[n] and cur[n] == lengths[n] for n in range(N)]
        done = [d or f for d, f in zip(done, final)]
        out.append((list(counts), [j == 0] * N, final))
    out.append(([0] * N, [False] * N, [not d for d in done]))
    return out


def max_chunk(calls):
    return max(1, max(max(counts) for counts, _, _ in calls))


def run(ref, F, calls, after_call=None):
    """Feeds F [N, T, V] (float64) to ``ref`` by the script ``calls`` -> the cursors."""
    cur = [0] * F.shape[0]
    for j, (counts, begin, final) in enumerate(calls):
        ref.advance(SR.chunk(F, cur, counts), counts, begin, final)
        cur = [a + c for a, c in zip(cur, counts)]
        if after_call:
            after_call(j, cur)
    return cur


def logits(name):
    """The fixture's classifier(features) in float64 [N, T, V]."""
    sd, features, _, _ = BR.inputs(name)
    return SR.logits(sd, features)
