"""Contextual biasing ("hotwords") for the beam searches: ``ContextGraph`` compiles a phrase list into the automaton tables that
csrc/ctc_prefix_beam.hip reads inside its one launch (``ctc.ctc_prefix_beam_search(context=...)``, ``ctc.PrefixBeamStream(context=...)``,
``TemporalClassifier.set_context``, ``StreamingRecognizer(context=...)``; include/halo.h).  Pure host code: Python and
torch on the CPU.  The object and its tables do not depend on the head; the CTC searches are the ones that take them today."""
import math
from collections import deque

import torch

MAX_STATES = 65535               # HALO_CONTEXT_MAX_STATES (include/halo.h)
MAX_TABLE_BYTES = 64 << 20       # next + gain


class ContextGraph:
    """``ContextGraph(phrases, vocab_size, bonus=1.0)``: ``phrases`` an iterable of non-empty token sequences over 1 .. vocab_size - 1
    (duplicates are dropped; an empty list is legal), ``bonus`` one finite float, negative allowed.  ValueError otherwise, above
    65535 states and above 64 MiB of tables.

    The phrases' trie has the root as state 0, depth d(s), and final(s) where a phrase ends; fail(s) is the Aho-Corasick failure link.
    goto(s, k) is the trie child of s by k if there is one, else the child by k of the first state on s's failure chain that has one,
    else the root.  Dictionary (output) links are NOT followed: a phrase is credited only along the active path, so a phrase that ends
    inside a longer match in progress earns nothing by itself.  With fa(s) the depth of the deepest final proper ancestor of s (0:
    none),

        held(s) = 0 if final(s) else bonus * (d(s) - fa(s))             what a hypothesis in s loses if its match breaks
        gain(s, k) = bonus * (d(s') - fa(s')) - held(s),  s' = goto(s, k)

    so every token that advances a match earns ``bonus``, a broken match gives back what it held, down to what the longest suffix that
    still matches holds, a completed phrase keeps what it earned, and a phrase that is a prefix of a longer one banks at its end while
    the longer one goes on earning.

    Tables (CPU tensors; ``to(device)`` returns and caches device copies, which this object keeps alive for captured graphs):
        columns [V] int32       0 for a token in no phrase, else its column 1 .. A (ascending by token)
        next [S, A + 1] int32   goto(s, k) at column columns[k]; column 0, any other token: 0
        gain [S, A + 1] float32 gain(s, k), computed in float64 and rounded once; column 0: -held(s)
        held [S] float32        ``scores - held[states]`` settles the matches a list left open
    ``gain64`` / ``held64`` are the float64 values the float32 ones were rounded from.

    step(state, token) -> (next state, gain as the float32 value the kernel adds, a Python float)
    boost(tokens) -> (state, boost): the gains added left to right in float32, the exact additions the kernel performs."""

    def __init__(self, phrases, vocab_size, bonus=1.0):
        V = int(vocab_size)
        if V < 2:
            raise ValueError(f'ContextGraph: vocab_size {V} must be at least 2')
        bonus = float(bonus)
        if not math.isfinite(bonus):
            raise ValueError(f'ContextGraph: bonus {bonus} is not finite')
        seen, plist = set(), []
        for ph in phrases:
            ph = tuple(int(k) for k in ph)
            if not ph:
                raise ValueError('ContextGraph: an empty phrase')
            if any(k < 1 or k >= V for k in ph):
                raise ValueError(f'ContextGraph: phrase {list(ph)} has a token outside 1 .. {V - 1}')
            if ph not in seen:
                seen.add(ph)
                plist.append(ph)
        self.vocab_size, self.bonus, self.phrases = V, bonus, tuple(plist)

        # the trie: children by token, depth, final, fa (the deepest final proper ancestor's depth), in creation order
        child, depth, final, parent = [{}], [0], [False], [0]
        for ph in plist:
            s = 0
            for k in ph:
                nxt = child[s].get(k)
                if nxt is None:
                    nxt = len(child)
                    if nxt >= MAX_STATES:
                        raise ValueError(f'ContextGraph: more than {MAX_STATES} states')
                    child[s][k] = nxt
                    child.append({}); depth.append(depth[s] + 1); final.append(False); parent.append(s)
                s = nxt
            final[s] = True
        S = len(child)
        alphabet = sorted({k for ph in plist for k in ph})
        A = len(alphabet)
        if 8 * S * (A + 1) > MAX_TABLE_BYTES:
            raise ValueError(f'ContextGraph: {S} states x {A + 1} columns need more than {MAX_TABLE_BYTES >> 20} MiB of tables')
        col = {k: a + 1 for a, k in enumerate(alphabet)}
        fa = [0] * S
        for s in range(1, S):                                           # (a parent is created before its children)
            p = parent[s]
            fa[s] = depth[p] if final[p] else fa[p]

        # failure links and the full transition table, breadth first: goto(s, k) of a state without the child is goto(fail(s), k)
        nxt_tab = [[0] * (A + 1) for _ in range(S)]
        fail = [0] * S
        queue = deque()
        for k, c in child[0].items():
            nxt_tab[0][col[k]] = c
            queue.append(c)
        while queue:
            s = queue.popleft()
            row, frow = nxt_tab[s], nxt_tab[fail[s]]
            row[1:] = frow[1:]
            for k, c in child[s].items():
                fail[c] = frow[col[k]]
                row[col[k]] = c
                queue.append(c)
        self.num_states, self.num_columns, self.width = S, A, A + 1
        self.depth, self.final, self.fail = tuple(depth), tuple(final), tuple(fail)
        value = torch.tensor([bonus * (depth[s] - fa[s]) for s in range(S)], dtype=torch.float64)    # bonus * (d(s) - fa(s))
        self.held64 = torch.where(torch.tensor(final), torch.zeros(S, dtype=torch.float64), value)
        self.next = torch.tensor(nxt_tab, dtype=torch.int32).view(S, A + 1)
        self.gain64 = value[self.next.long()] - self.held64[:, None]
        self.gain64[:, 0] = -self.held64                                # (value[0] is 0: the same number, stated)
        self.gain = self.gain64.float()
        self.held = self.held64.float()
        self.columns = torch.zeros(V, dtype=torch.int32)
        if A:
            self.columns[torch.tensor(alphabet)] = torch.arange(1, A + 1, dtype=torch.int32)
        self._next_rows, self._gain_rows, self._cols = self.next.tolist(), self.gain.tolist(), self.columns.tolist()
        self._device = {}

    def step(self, state, token):
        c = self._cols[token]
        return self._next_rows[state][c], self._gain_rows[state][c]

    def boost(self, tokens):
        state, z = 0, torch.zeros((), dtype=torch.float32)
        for k in tokens:
            state, g = self.step(state, int(k))
            z = z + torch.tensor(g, dtype=torch.float32)
        return state, float(z)

    def to(self, device):
        """-> (columns, next, gain) on ``device``, copied once per device and kept by this object."""
        dev = torch.device(device)
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        got = self._device.get(dev)
        if got is None:
            got = tuple(t.to(dev).contiguous() for t in (self.columns, self.next, self.gain))
            self._device[dev] = got
        return got
