"""Float64 restatement, in plain Python / NumPy loops, of the two forced-alignment recursions of csrc/viterbi.hip (haloop_amd.ctc.ctc_viterbi,
haloop_amd.transducer.transducer_viterbi / transducer_align), and the fixtures that tests/test_viterbi_cpu.py and
tests/test_gpu_viterbi.py share.  No tests in here.  The reference project has no aligner: this file is the yardstick, and
tests/test_viterbi_cpu.py validates it by brute-force enumeration.

CTC (F.ctc_loss's lattice).  ext = [0, y0, 0, y1, ..., 0], states 0 .. 2 tl, frames 0 .. il - 1:

    v[0][s] = lp[0][ext[s]] for s in {0, 1}, -inf elsewhere
    v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if s is a label that differs from the label two states back) + lp[t][ext[s]]
    score   = max(v[il-1][2 tl], v[il-1][2 tl - 1])

Ties: among equal predecessors the smallest shift (stay, then s-1, then s-2); at the end state 2 tl before 2 tl - 1.  il = 0: score 0 if
tl = 0, else infeasible.  An infeasible row has score -inf, no alignment.

Transducer.  Nodes (t, u), t < Tn, u <= Un:

    v[0][0] = 0;  v[t][u] = max(v[t-1][u] + joint[t-1][u][0], v[t][u-1] + joint[t][u-1][y[u-1]])
    score   = v[Tn-1][Un] + joint[Tn-1][Un][0]

Tie: the blank predecessor (t-1, u).  frames[u] = the t of the label arc (t, u) -> (t, u+1) on the best path.  Tn = 0: score -inf.

The gap of a row is its best score minus the best score of any path that leaves the best path: with a max-plus forward and backward
sweep, through[cell] = fwd[cell] + bwd[cell] (- the cell's emission for CTC, which both sweeps count) is the best score of a path
through that cell, and a monotone path of either lattice is determined by the cells it visits, so every other path visits a cell off
the best path: gap = score - max over off-path cells of through.  Rows with gap < GAP are not compared exactly on the GPU, the device
of tests/rnnt_beam_ref.py: fp32 summation error over these paths is below (terms) * 2^-23 * |score|, about 1e-4 at 63 terms, and the
fp32 log-sum-exp of halo_rnnt_joint_fwd adds about 1e-6 per cell, so 1e-3 separates the decisions the arithmetic can flip from those it
cannot.
"""
import functools
import math

import numpy as np
import torch

GAP = 1e-3
NINF = float('-inf')


# ---------------------------------------------------------------------------------------------------------------- CTC
def _ctc_lattice(lp, target, il):
    """-> (ext labels, skip flags, emissions em[t][s]) of one row; lp [T, C] float64."""
    ext = [0]
    for y in target:
        ext += [int(y), 0]
    skip = np.array([s >= 2 and ext[s] != 0 and ext[s] != ext[s - 2] for s in range(len(ext))])
    em = lp[:il][:, ext].reshape(il, len(ext))
    return ext, skip, em


def _shifted(row, k):
    """row[s - k], -inf where s < k."""
    return np.concatenate([np.full(k, NINF), row])[:len(row)]


def ctc_align_row(lp, target, il, want_gap=True):
    """lp [T, C] (anything np.float64 converts), target: the row's tl labels, il frames -> dict(score, alignment (il labels; None when
    infeasible), starts, ends (tl frames each; None when infeasible), states (the path), gap (None unless ``want_gap``)).  The loop over
    frames is Python's; a frame's states are updated together, each by the rule above."""
    lp = np.asarray(lp, dtype=np.float64)
    tl = len(target)
    none = dict(score=NINF, alignment=None, starts=None, ends=None, states=None, gap=math.inf if want_gap else None)
    if il == 0:
        return dict(score=0.0, alignment=[], starts=[], ends=[], states=[], gap=math.inf if want_gap else None) if tl == 0 else none
    ext, skip, em = _ctc_lattice(lp, target, il)
    ns = len(ext)
    row = np.full(ns, NINF)
    row[:2] = em[0][:2]
    fwd = [row]
    shift = np.zeros((il, ns), dtype=np.int8)
    for t in range(1, il):
        best, k = row, np.zeros(ns, dtype=np.int8)                # stay first ...
        b = _shifted(row, 1)
        take = b > best                                           # ... then s-1, only if strictly better ...
        best, k = np.where(take, b, best), np.where(take, 1, k)
        c = np.where(skip, _shifted(row, 2), NINF)
        take = c > best                                           # ... then s-2
        best, k = np.where(take, c, best), np.where(take, 2, k)
        row = best + em[t]
        shift[t] = k
        if want_gap:
            fwd.append(row)
    s_end, score = ns - 1, row[ns - 1]
    if ns >= 2 and row[ns - 2] > score:
        s_end, score = ns - 2, row[ns - 2]
    if score == NINF:
        return none
    states = [0] * il
    s = s_end
    for t in range(il - 1, -1, -1):
        states[t] = s
        s -= int(shift[t][s]) if t > 0 else 0
    starts, ends = [-1] * tl, [-1] * tl
    for t, s in enumerate(states):
        if s & 1:
            if starts[s >> 1] < 0:
                starts[s >> 1] = t
            ends[s >> 1] = t
    out = dict(score=float(score), alignment=[ext[s] for s in states], starts=starts, ends=ends, states=states, gap=None)
    if not want_gap:
        return out
    # max-plus backward sweep: the best completion from (t, s), the cell's own emission included
    fwd = np.stack(fwd)
    bwd = np.full((il, ns), NINF)
    bwd[il - 1][max(ns - 2, 0):] = em[il - 1][max(ns - 2, 0):]
    for t in range(il - 2, -1, -1):
        nxt = bwd[t + 1]
        one = np.concatenate([nxt[1:], [NINF]])[:ns]
        two = np.concatenate([np.where(skip, nxt, NINF)[2:], [NINF, NINF]])[:ns]
        bwd[t] = np.maximum(np.maximum(nxt, one), two) + em[t]
    with np.errstate(invalid='ignore'):
        through = fwd + bwd - em
    through[np.isnan(through)] = NINF
    for t, s in enumerate(states):
        through[t][s] = NINF
    off = float(through.max())
    out['gap'] = math.inf if off == NINF else float(score) - off
    return out


def ctc_log_sum_row(lp, target, il):
    """log of the sum over all alignments (the alpha sweep of the same lattice), float64."""
    lp = np.asarray(lp, dtype=np.float64)
    if il == 0:
        return 0.0 if len(target) == 0 else NINF
    ext, skip, em = _ctc_lattice(lp, target, il)
    ns = len(ext)
    a = np.full(ns, NINF)
    a[:2] = em[0][:2]
    for t in range(1, il):
        a = np.logaddexp(np.logaddexp(a, _shifted(a, 1)), np.where(skip, _shifted(a, 2), NINF)) + em[t]
    return float(np.logaddexp(a[ns - 1], a[ns - 2]) if ns >= 2 else a[ns - 1])


def ctc_align(lp_tnc, targets, input_lengths, target_lengths, want_gap=True):
    """lp_tnc [T, N, C] tensor, targets [N, S], lengths [N] -> list of ctc_align_row dicts (lengths clamped as the kernel clamps)."""
    T, N, _ = lp_tnc.shape
    lp = lp_tnc.detach().double().cpu().numpy()
    out = []
    for n in range(N):
        il = max(0, min(int(input_lengths[n]), T))
        tl = max(0, min(int(target_lengths[n]), targets.shape[1]))
        out.append(ctc_align_row(lp[:, n], [int(y) for y in targets[n, :tl]], il, want_gap))
    return out


def collapse(alignment):
    """unique_consecutive, blanks dropped."""
    out, last = [], None
    for a in alignment:
        if a != last and a != 0:
            out.append(a)
        last = a
    return out


# ---------------------------------------------------------------------------------------------------------------- transducer
def transducer_align_row(joint, target, Tn, want_gap=True):
    """joint [T, U1, K] (anything np.float64 converts), target: the row's Un labels, Tn frames -> dict(score, frames (Un entries; None
    for an empty row), path (the nodes (t, u)), gap (None unless ``want_gap``))."""
    Un = len(target)
    if Tn == 0:
        return dict(score=NINF, frames=None, path=None, gap=math.inf if want_gap else None)
    j = np.asarray(joint, dtype=np.float64)
    fwd = np.full((Tn, Un + 1), NINF)
    lab = np.zeros((Tn, Un + 1), dtype=np.int64)
    fwd[0][0] = 0.0
    for t in range(Tn):
        for u in range(Un + 1):
            if t == 0 and u == 0:
                continue
            a = fwd[t - 1][u] + j[t - 1][u][0] if t > 0 else NINF
            b = fwd[t][u - 1] + j[t][u - 1][target[u - 1]] if u > 0 else NINF
            fwd[t][u], lab[t][u] = (b, 1) if b > a else (a, 0)
    score = fwd[Tn - 1][Un] + j[Tn - 1][Un][0]
    frames, path = [-1] * Un, []
    t, u = Tn - 1, Un
    while True:
        path.append((t, u))
        if t == 0 and u == 0:
            break
        if lab[t][u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
    if not want_gap:
        return dict(score=float(score), frames=frames, path=path[::-1], gap=None)
    bwd = np.full((Tn, Un + 1), NINF)
    for t in range(Tn - 1, -1, -1):
        for u in range(Un, -1, -1):
            if t == Tn - 1 and u == Un:
                bwd[t][u] = j[t][u][0]
                continue
            a = j[t][u][0] + bwd[t + 1][u] if t + 1 < Tn else NINF
            b = j[t][u][target[u]] + bwd[t][u + 1] if u < Un else NINF
            bwd[t][u] = max(a, b)
    through = fwd + bwd
    for t, u in path:
        through[t][u] = NINF
    off = float(through.max())
    return dict(score=float(score), frames=frames, path=path[::-1], gap=math.inf if off == NINF else float(score) - off)


def transducer_log_sum_row(joint, target, Tn):
    Un = len(target)
    if Tn == 0:
        return NINF
    j = np.asarray(joint, dtype=np.float64)
    a = np.full((Tn, Un + 1), NINF)
    a[0][0] = 0.0
    for t in range(Tn):
        for u in range(Un + 1):
            if t == 0 and u == 0:
                continue
            x = a[t - 1][u] + j[t - 1][u][0] if t > 0 else NINF
            y = a[t][u - 1] + j[t][u - 1][target[u - 1]] if u > 0 else NINF
            a[t][u] = np.logaddexp(x, y)
    return float(a[Tn - 1][Un] + j[Tn - 1][Un][0])


def transducer_align(joint, targets, joint_lengths, target_lengths, want_gap=True):
    """joint [N, T, U1, K] tensor -> list of transducer_align_row dicts (lengths clamped as the kernel clamps)."""
    N, T, U1, _ = joint.shape
    j = joint.detach().double().cpu().numpy()
    out = []
    for n in range(N):
        Tn = max(0, min(int(joint_lengths[n]), T))
        Un = max(0, min(int(target_lengths[n]), U1 - 1))
        out.append(transducer_align_row(j[n], [int(y) for y in targets[n, :Un]], Tn, want_gap))
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
# Emissions are log_softmax(randn * 2) in float32 from torch.Generator().manual_seed(seed); the seeds were searched on the CPU with this
# file's loops for the conditions tests/test_viterbi_cpu.py asserts (every compared row's gap >= GAP).
GARBAGE = 1 << 40          # fills targets past a row's length: a label the kernel must not read (it is outside every vocabulary)

CTC_FIXTURES = {
    # name: seed, N, T, C, S, il range, tl range (row 0 takes the largest il and tl)
    'bench': dict(seed=0, N=16, T=21, C=32, S=10, il=(17, 21), tl=(5, 10)),          # the bench lattice: 21 states
    'small_vocab': dict(seed=0, N=17, T=40, C=8, S=12, il=(30, 40), tl=(4, 12)),     # repeated neighbours; the special rows below
    'one_wave': dict(seed=0, N=8, T=63, C=5, S=31, il=(55, 63), tl=(16, 31)),        # 63 states
    'two_waves': dict(seed=0, N=3, T=90, C=6, S=40, il=(80, 90), tl=(30, 40)),       # 81 states
    'past_block': dict(seed=1, N=2, T=300, C=4, S=140, il=(280, 300), tl=(100, 140)),  # 281 states: two states per thread of 256
}
# the special rows of 'small_vocab': (row, kind)
SPECIAL = {13: 'empty_target', 14: 'forced', 15: 'infeasible', 16: 'one_frame'}

TRANSDUCER_FIXTURES = {
    # name: seed, N, T, U, V, Tn range, Un range (row 0 takes the largest of both)
    'bench': dict(seed=0, N=16, T=21, U=10, V=32, tn=(11, 21), un=(0, 10)),
    'edges': dict(seed=0, N=17, T=9, U=5, V=7, tn=(2, 9), un=(1, 5)),                # rows 14, 15, 16: Tn = 1, Un = 0, Tn = 0
    'long_diagonal': dict(seed=0, N=3, T=3, U=299, V=2, tn=(2, 3), un=(200, 299)),   # a K = 2 joint, as lp2: 300 columns
}
TRANSDUCER_SPECIAL = {14: 'one_frame', 15: 'empty_target', 16: 'empty_row'}

# rows whose gap is below GAP: compared by no test (at most a quarter of a fixture's rows, never a special row)
LEFT_OUT = {}


def repeats(target):
    return sum(1 for a, b in zip(target, target[1:]) if a == b)


@functools.lru_cache(maxsize=None)
def ctc_inputs(name):
    """-> (lp [T, N, C] float32 log-probabilities, targets [N, S] int64 padded with GARBAGE, input_lengths [N], target_lengths [N]) on the
    CPU.  Computed once per process; callers must not modify what they get."""
    f = CTC_FIXTURES[name]
    N, T, C, S = f['N'], f['T'], f['C'], f['S']
    gen = torch.Generator().manual_seed(f['seed'])
    lp = (torch.randn(T, N, C, generator=gen) * 2).log_softmax(-1)
    labels = torch.randint(1, C, (N, S), generator=gen)
    tl = torch.randint(f['tl'][0], f['tl'][1] + 1, (N,), generator=gen)
    il = torch.randint(f['il'][0], f['il'][1] + 1, (N,), generator=gen)
    tl[0], il[0] = f['tl'][1], f['il'][1]
    if name == 'small_vocab':
        for row, kind in SPECIAL.items():
            if kind == 'empty_target':
                tl[row] = 0
            elif kind == 'forced':                   # as many frames as the target needs: one path
                tl[row] = S
                il[row] = S + repeats(labels[row].tolist())
            elif kind == 'infeasible':               # one frame short
                tl[row] = S
                il[row] = S + repeats(labels[row].tolist()) - 1
            elif kind == 'one_frame':
                tl[row], il[row] = 1, 1
    for n in range(N):                               # every other row is feasible
        need = int(tl[n]) + repeats(labels[n, :int(tl[n])].tolist())
        if not (name == 'small_vocab' and n in SPECIAL):
            il[n] = max(int(il[n]), need)
            assert int(il[n]) <= T
    targets = labels.clone()
    targets[torch.arange(S)[None, :] >= tl[:, None]] = GARBAGE
    return lp, targets, il, tl


@functools.lru_cache(maxsize=None)
def ctc_fixture(name):
    """-> (lp, targets, input_lengths, target_lengths, reference rows).  Computed once per process; callers must not modify it."""
    lp, targets, il, tl = ctc_inputs(name)
    return lp, targets, il, tl, ctc_align(lp, targets, il, tl)


@functools.lru_cache(maxsize=None)
def transducer_inputs(name):
    """-> (f [N, T, V], g [N, U+1, V] float32 logits, joint [N, T, U+1, V] = (f + g).log_softmax(-1) in float32, targets [N, U],
    joint_lengths [N], target_lengths [N]) on the CPU.  Computed once per process; callers must not modify what they get."""
    s = TRANSDUCER_FIXTURES[name]
    N, T, U, V = s['N'], s['T'], s['U'], s['V']
    gen = torch.Generator().manual_seed(s['seed'])
    f = torch.randn(N, T, V, generator=gen) * 2
    g = torch.randn(N, U + 1, V, generator=gen) * 2
    targets = torch.randint(1, V, (N, U), generator=gen)
    tn = torch.randint(s['tn'][0], s['tn'][1] + 1, (N,), generator=gen)
    un = torch.randint(s['un'][0], s['un'][1] + 1, (N,), generator=gen)
    tn[0], un[0] = s['tn'][1], s['un'][1]
    if name == 'edges':
        for row, kind in TRANSDUCER_SPECIAL.items():
            if kind == 'one_frame':
                tn[row] = 1
            elif kind == 'empty_target':
                un[row] = 0
            elif kind == 'empty_row':
                tn[row] = 0
    joint = (f[:, :, None, :] + g[:, None, :, :]).log_softmax(-1)
    return f, g, joint, targets, tn, un


@functools.lru_cache(maxsize=None)
def transducer_fixture(name):
    f, g, joint, targets, tn, un = transducer_inputs(name)
    return f, g, joint, targets, tn, un, transducer_align(joint, targets, tn, un)


def compared_rows(kind, name):
    N = (CTC_FIXTURES if kind == 'ctc' else TRANSDUCER_FIXTURES)[name]['N']
    return [n for n in range(N) if n not in LEFT_OUT.get((kind, name), ())]


# ---- wide lattices: one fixture per instantiation of the kernels above 512 states / columns (csrc/viterbi.hip keeps 4, 8, 16 and 30
#      states per thread of 256), the last at the bound of 7679.  Over thousands of frames fp32 rounding can flip decisions that 1e-3
#      separates, so these do without rounding instead of without close calls: their emissions are multiples of 2^-6 in [-8, 0] and a path
#      sums fewer than 2^14 of them, so every partial sum is a multiple of 2^-6 below 2^17 -- exact in fp32 as in float64.  The device
#      must equal the reference on every row, scores to the bit and ties included (quantised emissions tie often). ----
CTC_EXACT = {
    # name: seed, N, T, C, S (row 0: il = T, tl = S; a second row is shorter in both)
    'per4': dict(seed=0, N=2, T=340, C=12, S=300),             # 601 states
    'per8': dict(seed=0, N=2, T=600, C=16, S=520),             # 1041 states
    'per16': dict(seed=0, N=1, T=1130, C=24, S=1030),          # 2061 states
    'per30': dict(seed=0, N=1, T=4100, C=64, S=3839),          # 7679 states: the bound
}
TRANSDUCER_EXACT = {
    # name: seed, N, T, U (K = 2, targets of ones: the shape of lp2; row 0: Tn = T, Un = U; row 1 is shorter in both)
    'per4': dict(seed=0, N=2, T=3, U=600), 'per8': dict(seed=0, N=2, T=3, U=1100), 'per16': dict(seed=0, N=2, T=3, U=2100),
    'per30': dict(seed=0, N=2, T=3, U=4200), 'bound': dict(seed=0, N=2, T=3, U=7678),
}


def quantised(gen, *shape):
    """Multiples of 2^-6 in [-8, 0]."""
    return torch.round((torch.randn(*shape, generator=gen) * 2).clamp(-4, 4) * 64) / 64 - 4


@functools.lru_cache(maxsize=None)
def ctc_exact_fixture(name):
    """-> (lp [T, N, C] float32, targets, input_lengths, target_lengths, reference rows without gaps).  Callers must not modify it."""
    f = CTC_EXACT[name]
    N, T, C, S = f['N'], f['T'], f['C'], f['S']
    gen = torch.Generator().manual_seed(f['seed'])
    lp = quantised(gen, T, N, C)
    targets = torch.randint(1, C, (N, S), generator=gen)
    tl = torch.tensor([S, S - S // 3][:N])
    il = torch.tensor([T, T - 7][:N])
    for n in range(N):
        assert int(il[n]) >= int(tl[n]) + repeats(targets[n, :int(tl[n])].tolist())
    targets[torch.arange(S)[None, :] >= tl[:, None]] = GARBAGE
    return lp, targets, il, tl, ctc_align(lp, targets, il, tl, want_gap=False)


@functools.lru_cache(maxsize=None)
def transducer_exact_fixture(name):
    """-> (joint [N, T, U+1, 2] float32, targets (ones), joint_lengths, target_lengths, reference rows without gaps)."""
    f = TRANSDUCER_EXACT[name]
    N, T, U = f['N'], f['T'], f['U']
    gen = torch.Generator().manual_seed(f['seed'])
    joint = quantised(gen, N, T, U + 1, 2)
    targets = torch.ones(N, U, dtype=torch.long)
    tn, un = torch.tensor([T, T - 1][:N]), torch.tensor([U, U - U // 3][:N])
    return joint, targets, tn, un, transducer_align(joint, targets, tn, un, want_gap=False)


# the tie-rule cases: constant emissions of exactly -2.0, every sum exact in fp32 and float64
TIE_CTC = dict(T=7, C=3, target=[1, 1, 2], score=-14.0, alignment=[1, 0, 1, 2, 0, 0, 0], starts=[0, 2, 3], ends=[0, 2, 3])
TIE_TRANSDUCER = dict(T=4, U=2, K=3, target=[1, 2], score=-12.0, frames=[0, 0])
