"""Float64 restatements of the optimizer step on flat buffers (include/halo.h, "Optimizer step on flat buffers"; torch.optim.AdamW's
single-tensor definition; torch.nn.utils.clip_grad_norm_), the float32 restatement that sizes the gates, a set of subtly wrong variants
(MUTANTS) the gates must reject, and the inputs that tests/test_gpu_optim.py and tests/test_optim_ref_cpu.py share.  No tests in here.

Everything is numpy.  State is passed in and returned (p, m, v); nothing is updated in place.

Hyper-parameters reach the kernels as C floats, so the tests name the float32 values (``f32(1e-2)`` ...) and every restatement computes
with exactly those: 1 - float32(0.999) differs from 0.001 by 1e-5 of itself, which is not a rounding the kernels may be charged with."""
import functools

import numpy as np
import torch


def f32(x):
    """The float32 nearest to x, as a python float: what a C float argument carries."""
    return float(np.float32(x))


LR, WD, EPS = f32(1e-2), f32(0.1), f32(1e-8)
BETAS = {'b95': (f32(0.9), f32(0.95)), 'b999': (f32(0.9), f32(0.999))}


# ---- the comparison ---------------------------------------------------------------------------------------------------------------

def max_err(got, want, scale):
    """max over EVERY element of |got - want| / (|want| + scale).  ``scale`` (array or number, >= 0) is the magnitude of the operands the
    element was formed from: where a result cancels (p - update, m + (g - m) * w) the rounding error is relative to the operands, not to
    the result.  An element whose denominator is 0 must be matched exactly; a non-finite ``got`` or ``want`` counts as inf unless both
    are the same non-finite value."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    den = np.abs(want) + np.broadcast_to(np.asarray(scale, np.float64), want.shape)
    with np.errstate(all='ignore'):
        e = np.abs(got - want) / den
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    e = np.where(same, 0.0, e)
    e = np.where(np.isfinite(e), e, np.inf)
    return float(e.max())


def state_err(got, want, scales):
    """(err_p, err_m, err_v) of two (p, m, v) triples; scales = (scale_p, scale_m, scale_v)."""
    return tuple(max_err(a, b, s) for a, b, s in zip(got, want, scales))


def within(errs, gates):
    """The comparison every test uses: each output's max_err is at most its gate."""
    return all(e <= g for e, g in zip(errs, gates))


def mabs_next(mabs, g, b1, scale=None):
    """The first-moment recurrence on absolute values: M' = b1 * M + (1 - b1) * |g * scale| (unchanged under a NaN scale).  m is a weighted
    sum of every gradient so far, of either sign; the rounding error of such a sum is relative to the sum of the terms' magnitudes, which
    is M, and not to the (possibly cancelled) result."""
    mabs, g = np.asarray(mabs, np.float64), np.asarray(g, np.float64)
    if scale is not None and scale != scale:
        return mabs.copy()
    k = 1.0 if scale is None else abs(float(scale))
    with np.errstate(all='ignore'):
        return b1 * mabs + (1.0 - b1) * np.where(np.isfinite(g), np.abs(g) * k, 0.0)


def step_scales(mabs):
    """max_err's scales for (p, m, v) after a step: p' = p * decay - update is formed from numbers of the size of p ~ N(0, 1) (1); m' from
    terms whose magnitudes sum to ``mabs`` (mabs_next); v' is a sum of non-negative terms (0: purely relative)."""
    return (1.0, mabs, 0.0)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------

def _f64(*xs):
    return tuple(np.asarray(x, np.float64) for x in xs)


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, t, scale=None):
    """One torch.optim.AdamW update number t (1-based) in float64: decoupled decay, denom = sqrt(v) / sqrt(1 - b2^t) + eps.  The gradient is
    multiplied by ``scale`` first (None: 1); a NaN scale leaves p, m and v untouched."""
    p, g, m, v = _f64(p, g, m, v)
    if scale is not None:
        if scale != scale:
            return p.copy(), m.copy(), v.copy()
        g = g * float(scale)
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    p = p - (lr / (1.0 - b1 ** t)) * (m / denom)
    return p, m, v


def clip_coef(sumsq, max_norm):
    """(coef[0], coef[1], norm) of halo_clip_coef: min(1, max_norm / (norm + 1e-6)) and 1; NaN and NaN when the norm is not finite."""
    with np.errstate(all='ignore'):
        norm = float(np.sqrt(np.float64(sumsq)))
    if not np.isfinite(norm):
        return float('nan'), float('nan'), norm
    return min(1.0, max_norm / (norm + 1e-6)), 1.0, norm


def ranges_step(p, g, m, v, ranges, lr, b1, b2, eps, t, step_fn=None):
    """adamw_step on every [begin, end) of ``ranges`` = [(begin, end, wd, scale or None), ...]; everything outside is returned as it came."""
    step_fn = step_fn or adamw_step
    p, g, m, v = _f64(p, g, m, v)
    p, m, v = p.copy(), m.copy(), v.copy()
    for a, b, wd, scale in ranges:
        p[a:b], m[a:b], v[a:b] = step_fn(p[a:b], g[a:b], m[a:b], v[a:b], lr, b1, b2, eps, wd, t, scale)
    return p, m, v


def ranges_mabs(mabs, g, ranges, b1):
    """mabs_next for a ranged step (outside the ranges mabs stays as it is: 0 from the start, i.e. exact)."""
    mabs = np.array(mabs, np.float64)
    for a, b, _, scale in ranges:
        mabs[a:b] = mabs_next(mabs[a:b], g[a:b], b1, scale)
    return mabs


def ranges_scales(mabs, ranges):
    """max_err's scales for a ranged step: exact (0) outside the ranges."""
    sp = np.zeros(len(mabs), np.float64)
    for a, b, _, _ in ranges:
        sp[a:b] = 1.0
    return sp, mabs, 0.0


# ---- float32 restatement (sizes the gates; nothing else) ---------------------------------------------------------------------------------

def f32_restatement(p, g, m, v, lr, b1, b2, eps, wd, t, scale=None):
    """The same step in float32 on the CPU in the documented order (torch's _single_tensor_adamw: mul_, lerp_, mul_/addcmul_, sqrt / bias
    correction + eps, addcdiv_), every operation rounded separately; the scalars are prepared in double and rounded once, as torch's
    python side does."""
    F = np.float32
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    if scale is not None:
        if scale != scale:
            return p.copy(), m.copy(), v.copy()
        g = g * F(scale)
    decay, w1, w2 = F(1.0 - lr * wd), F(1.0 - b1), F(1.0 - b2)
    step_size, bc2_sqrt = F(lr / (1.0 - b1 ** t)), F(np.sqrt(1.0 - b2 ** t))
    p = p * decay
    m = m + (g - m) * w1
    v = v * F(b2) + (w2 * g) * g
    denom = np.sqrt(v) / bc2_sqrt + F(eps)
    p = p - step_size * (m / denom)
    return p, m, v


def f32_clip_coef(sumsq, max_norm):
    """clip_coef with every operation in float32 (sumsq: the float32 sum of squares)."""
    F = np.float32
    with np.errstate(all='ignore'):
        norm = np.sqrt(F(sumsq))
    if not np.isfinite(norm):
        return float('nan'), float('nan'), float(norm)
    c = F(max_norm) / (norm + F(1e-6))
    return float(min(F(1.0), c)), 1.0, float(norm)


def f32_sumsq(x):
    """float32 pairwise sum of float32 squares (numpy's add.reduce is pairwise)."""
    x = np.asarray(x, np.float32)
    return float(np.sum(x * x, dtype=np.float32))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
# Each is adamw_step with ONE thing wrong (mutant i: ranges_step with one thing wrong, see RANGE_MUTANTS).
#  ``prev_lr`` (mutant f) is the learning rate of the step before (None on the first one).

def _mutant(eps_inside=False, t_shift=0, no_bc2=False, coupled=False, decay_after=False, stale_decay=False, scale_m_only=False,
            swap_b2=False):
    def step(p, g, m, v, lr, b1, b2, eps, wd, t, scale=None, prev_lr=None):
        p, g, m, v = _f64(p, g, m, v)
        gm = gv = g
        if scale is not None:
            if scale != scale:
                return p.copy(), m.copy(), v.copy()
            gm = g * float(scale)
            gv = g if scale_m_only else gm
        decay = 1.0 - (prev_lr if stale_decay and prev_lr is not None else lr) * wd
        if coupled:
            gm, gv = gm + wd * p, gv + wd * p
        elif not decay_after:
            p = p * decay
        m = b1 * m + (1.0 - b1) * gm
        v = ((1.0 - b2) * v + b2 * gv * gv) if swap_b2 else (b2 * v + (1.0 - b2) * gv * gv)
        tt = t - t_shift if t > t_shift else t           # (a shifted count of 0 would divide by zero: the first step is taken right)
        with np.errstate(all='ignore'):
            bc2 = 1.0 if no_bc2 else 1.0 - b2 ** tt
            denom = (np.sqrt(v) + eps) / np.sqrt(bc2) if eps_inside else np.sqrt(v) / np.sqrt(bc2) + eps
            p = p - (lr / (1.0 - b1 ** tt)) * (m / denom)
        if decay_after and not coupled:
            p = p * decay
        return p, m, v
    return step


MUTANTS = {
    'a_eps_inside_correction': _mutant(eps_inside=True),
    'b_bias_correction_at_t_minus_1': _mutant(t_shift=1),          # from step 2 on; judged by the arithmetic, not by a 0 / 0
    'c_no_second_moment_correction': _mutant(no_bc2=True),
    'd_coupled_l2_decay': _mutant(coupled=True),
    'e_decay_after_step': _mutant(decay_after=True),
    'f_decay_from_previous_lr': _mutant(stale_decay=True),
    'g_scale_on_m_only': _mutant(scale_m_only=True),
    'h_b2_swapped_in_v': _mutant(swap_b2=True),
}


def ranges_step_neighbour(p, g, m, v, ranges, lr, b1, b2, eps, t):
    """Mutant (i): range r is updated with the weight decay and scale of range r + 1 (cyclically)."""
    n = len(ranges)
    wrong = [(a, b, ranges[(r + 1) % n][2], ranges[(r + 1) % n][3]) for r, (a, b, _, _) in enumerate(ranges)]
    return ranges_step(p, g, m, v, wrong, lr, b1, b2, eps, t)


MUTANTS['i_neighbours_wd_and_scale'] = ranges_step_neighbour
RANGE_MUTANTS = ('i_neighbours_wd_and_scale',)         # these have ranges_step's signature, the others adamw_step's


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def make_inputs(n, steps, seed):
    """(p [n], g [steps, n], s [n]) float32/float32/float64 from a seeded CPU generator: element i has its own scale s_i, log-uniform in
    [1e-10, 1e2]; g_t[i] = s_i * z, z ~ N(0, 1); about 1 % of the elements have g == 0 at every step; p ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    s = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 12.0 - 10.0)
    zero = torch.rand(n, generator=gen) < 0.01
    p = torch.randn(n, generator=gen, dtype=torch.float32)
    g = torch.empty(steps, n, dtype=torch.float32)
    for k in range(steps):
        g[k] = (s * torch.randn(n, generator=gen, dtype=torch.float64)).float()
        g[k][zero] = 0.0
    return p.numpy(), g.numpy(), s.numpy()


def make_moments(s, g0, seed):
    """A synthetic (m, v) consistent with gradients of scale s (|m| of the order of sqrt(v), both 0 where the gradient is always 0)."""
    gen = torch.Generator().manual_seed(seed)
    n = len(s)
    m = (torch.from_numpy(s) * 0.3 * torch.randn(n, generator=gen, dtype=torch.float64)).float().numpy()
    v = ((torch.from_numpy(s) ** 2) * (0.5 + torch.rand(n, generator=gen, dtype=torch.float64))).float().numpy()
    dead = np.asarray(g0) == 0
    m[dead] = 0.0
    v[dead] = 0.0
    return m, v


ADAMW_STEPS = 12
ADAMW_SIZES = (1, 3, 4, 5, 1023, 4097, 2048 * 256 * 4 + 4 * 256 * 3 + 3)
GATE_N = ADAMW_SIZES[-1]                 # the gates are measured where the maximum runs over the most elements
LATE_STEPS = (1000, 100000)


@functools.lru_cache(maxsize=2)
def adamw_inputs(n):
    return make_inputs(n, ADAMW_STEPS, 1000 + n % 997)


def run_steps(step_fn, p, g, lr, b1, b2, eps, wd, scale=None, m=None, v=None, t0=1):
    """Consecutive steps t0, t0+1, ... over the rows of g from (p, m, v) (zero moments by default); yields (p, m, v) after each."""
    m = np.zeros_like(p) if m is None else m
    v = np.zeros_like(p) if v is None else v
    for k in range(len(g)):
        p, m, v = step_fn(p, g[k], m, v, lr, b1, b2, eps, wd, t0 + k, scale)
        yield p, m, v


# ---- the 8-range buffer of the halo_adamw_ranges test ----------------------------------------------------------------------------------------

RANGES_BIG = 4096 * 256 * 4 + 4 * 256 * 5 + 8          # one full pass of the biggest grid (4096 workgroups), part of a second
#               length      wd    scale
RANGES_SPEC = [(1000,       0.1,  None),
               (0,          0.3,  0.25),               # empty
               (RANGES_BIG, 0.1,  0.25),
               (4,          0.3,  1.0),
               (2052,       0.0,  float('nan')),       # skipped; its neighbours in memory are updated
               (516,        0.0,  0.25),
               (260,        0.3,  None),
               (4096,       0.1,  1.0)]
RANGES_ORDER = (5, 2, 7, 0, 3, 1, 6, 4)                # the order the ranges are passed in: not ascending
RANGES_STEPS = 2


def ranges_layout():
    """(total, [(begin, end, wd, scale)] in RANGES_ORDER): the ranges lie in memory in RANGES_SPEC's order with gaps of 4 or 8 elements
    before each and 64 elements after the last."""
    out, at = [], 0
    for k, (ln, wd, sc) in enumerate(RANGES_SPEC):
        at += 8 if k % 2 else 4
        out.append((at, at + ln, f32(wd), sc))
        at += ln
    return at + 64, [out[k] for k in RANGES_ORDER]


@functools.lru_cache(maxsize=1)
def ranges_inputs():
    total, ranges = ranges_layout()
    p, g, s = make_inputs(total, RANGES_STEPS, 77)
    inside = np.zeros(total, bool)
    for a, b, _, _ in ranges:
        inside[a:b] = True
    g[:, ~inside] = np.nan                             # NaN canaries in the gaps of g: never read
    return p, g, s, ranges, inside


# ---- halo_adamw_ranges_dev: device step counts, a device lr that changes ------------------------------------------------------------------------

DEV_STEPS = (0, 1, 2, 37, 100000)
DEV_N = 1024 * 4 + 64
DEV_RANGES = [(2052, 4096, f32(0.3), 0.25), (0, 1024, f32(0.1), None), (1028, 2048, 0.0, 1.0)]
DEV_LRS = tuple(f32(x) for x in (1e-2, 3e-3, 2e-2, 5e-4))


@functools.lru_cache(maxsize=1)
def dev_inputs():
    p, g, s = make_inputs(DEV_N, len(DEV_LRS), 91)
    m, v = make_moments(s, g[0], 92)
    return p, g, m, v


def changing_lr_run(step_fn, stale=False):
    """len(DEV_LRS) consecutive ranged steps from zero moments, step k with DEV_LRS[k]; ``stale``: step_fn takes prev_lr (mutant f)."""
    p, g, _, _ = dev_inputs()
    b1, b2 = BETAS['b95']
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for k, lr in enumerate(DEV_LRS):
        fn = step_fn
        if stale:
            prev = DEV_LRS[k - 1] if k else None
            fn = functools.partial(step_fn, prev_lr=prev)
        p, m, v = ranges_step(p, g[k], m, v, DEV_RANGES, lr, b1, b2, EPS, k + 1, step_fn=fn)
        out.append((p, m, v))
    return out


# ---- the trainer's chain: sumsq -> clip_coef(applied_steps) -> adamw_ranges(step_dev, lr_dev, counter) ------------------------------------------------

CHAIN_STEPS = 25
CHAIN_INF_STEP = 9                                     # 0-based: this step's gradient carries an Inf inside the clipped range
CHAIN_MAX_NORM = f32(650.0)                            # about the median gradient norm of the clipped range (see chain_inputs)
#                 length  decays clipped               the trainer's four classes; the clipped ones are contiguous and come first
CHAIN_CLASSES = [(2048,   True,  True),
                 (260,    False, True),
                 (1028,   True,  False),
                 (64,     False, False)]
CHAIN_WD = f32(0.1)


def chain_layout():
    out, at = [], 0
    for ln, decays, clipped in CHAIN_CLASSES:
        out.append((at, at + ln, decays, clipped))
        at += ln
    return at, out


CHAIN_CLIPPED = (0, 2048 + 260)


def chain_lrs():
    """Warm-up over 5 steps to LR, then inverse-square-root decay; indexed by the number of applied updates so far."""
    return [f32(LR * min((k + 1) / 5.0, 1.0) * min(1.0, (5.0 / (k + 1)) ** 0.5)) for k in range(CHAIN_STEPS)]


@functools.lru_cache(maxsize=1)
def chain_inputs():
    """(p, g [steps, n]): the gradients of step k carry an amplitude 10^U(-1, 1), so that the clipped norm (about 650 * amplitude: 2308
    elements with E[s^2] = 1e4 / (24 ln 10)) lies above CHAIN_MAX_NORM on some steps and below it on others."""
    n, _ = chain_layout()
    p, g, _ = make_inputs(n, CHAIN_STEPS, 55)
    gen = torch.Generator().manual_seed(56)
    amp = 10.0 ** (torch.rand(CHAIN_STEPS, generator=gen, dtype=torch.float64) * 2.0 - 1.0)
    g = (g.astype(np.float64) * amp.numpy()[:, None]).astype(np.float32)
    g[CHAIN_INF_STEP, 17] = np.inf
    return p, g


def chain_run(ranges_fn=None, single=False):
    """The chain, each step's update applied by ``ranges_fn`` (ranges_step's signature; default: ranges_step in float64).  ``single``: the
    gate-sizing restatement, every operation of the norm, the coefficient and the step in float32.  The step is skipped the way
    ha/loop.py:184-191 skips it: a non-finite norm applies nothing, does not advance the update count and does not advance the
    schedule.  -> list per step of dict(p, m, v, coef, norm, applied, lr, scales); coef, norm and scales are the float64 ones."""
    n, classes = chain_layout()
    p, g = chain_inputs()
    b1, b2 = BETAS['b999']
    lrs = chain_lrs()
    if ranges_fn is None:
        ranges_fn = functools.partial(ranges_step, step_fn=f32_restatement) if single else ranges_step
    m, v, mabs = np.zeros(n), np.zeros(n), np.zeros(n)
    applied, out = 0, []
    lo, hi = CHAIN_CLIPPED
    for k in range(CHAIN_STEPS):
        with np.errstate(all='ignore'):
            ref = clip_coef(np.sum(g[k, lo:hi].astype(np.float64) ** 2), CHAIN_MAX_NORM)
            c0, c1, norm = f32_clip_coef(f32_sumsq(g[k, lo:hi]), CHAIN_MAX_NORM) if single else ref
        applied += bool(np.isfinite(norm))
        t = max(applied, 1)
        ranges = [(a, b, CHAIN_WD if decays else 0.0, c0 if clipped else c1) for a, b, decays, clipped in classes]
        mabs = ranges_mabs(mabs, g[k], [(a, b, 0.0, ref[0] if clipped else ref[1]) for a, b, _, clipped in classes], b1)
        with np.errstate(all='ignore'):
            p, m, v = ranges_fn(p, g[k], m, v, ranges, lrs[t - 1], b1, b2, EPS, t)
        out.append(dict(p=p, m=m, v=v, coef=ref[0], norm=ref[2], applied=applied, lr=lrs[t - 1], scales=ranges_scales(mabs, ranges)))
    return out


@functools.lru_cache(maxsize=1)
def torch_chain():
    """The chain in torch, float64: four parameters (one per class), torch.optim.AdamW with a decayed and an undecayed group,
    clip_grad_norm_ over the clipped ones, the step skipped as ha/loop.py:184-191 skips it (no optimizer.step(), no advance of the
    schedule).  -> per step dict(p, m, v, applied, norm), the tensors concatenated in buffer order."""
    n, classes = chain_layout()
    p0, g = chain_inputs()
    lrs = chain_lrs()
    params = [torch.nn.Parameter(torch.from_numpy(p0[a:b]).double()) for a, b, _, _ in classes]
    opt = torch.optim.AdamW([{'params': [q for q, c in zip(params, classes) if c[2]], 'weight_decay': CHAIN_WD},
                             {'params': [q for q, c in zip(params, classes) if not c[2]], 'weight_decay': 0.0}],
                            lr=lrs[0], betas=BETAS['b999'], eps=EPS)
    applied, out = 0, []
    for k in range(CHAIN_STEPS):
        for q, (a, b, _, _) in zip(params, classes):
            q.grad = torch.from_numpy(g[k, a:b]).double()
        norm = torch.nn.utils.clip_grad_norm_([q for q, c in zip(params, classes) if c[3]], CHAIN_MAX_NORM, error_if_nonfinite=False)
        if torch.isfinite(norm):
            for group in opt.param_groups:
                group['lr'] = lrs[applied]
            applied += 1
            opt.step()
        opt.zero_grad(set_to_none=True)
        state = [opt.state.get(q, {}) for q in params]
        cat = lambda key: np.concatenate([s[key].numpy() if key in s else np.zeros(q.numel()) for s, q in zip(state, params)])
        out.append(dict(p=np.concatenate([q.detach().numpy() for q in params]), m=cat('exp_avg'), v=cat('exp_avg_sq'), applied=applied,
                        norm=float(norm)))
    return out


# ---- halo_sumsq ------------------------------------------------------------------------------------------------------------------------------

SUMSQ_SIZES = (1, 3, 5, 1024 * 256 * 4 + 7)


@functools.lru_cache(maxsize=None)
def sumsq_case(n):
    """(x, float64 sum of squares, rtol): rtol = 4 x the error of numpy's float32 pairwise sum of the float32 squares on this x.  The
    figure is what ONE float32 summation happens to lose on this data (for n = 1 a single rounding of one square), so it belongs to the
    seed: change the seed or the generator only together with a fresh look at these figures (test_optim_ref_cpu.py holds them to
    [2^-26, 1e-6]; the docstring of test_gpu_optim.py lists them)."""
    _, g, _ = make_inputs(n, 1, 300 + n % 97)
    want = float(np.sum(g[0].astype(np.float64) ** 2))
    return g[0], want, 4.0 * abs(f32_sumsq(g[0]) - want) / want


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------------
# 4 x the float32 restatement's error against float64 in max_err, per output (p, m, v), measured on the CPU after the last step
# (adamw_*: 12 steps at GATE_N; chain: 25 steps).  test_optim_ref_cpu.py recomputes them; the table is in test_gpu_optim.py's docstring.

GATES = {'adamw_b95': (2.051e-06, 4.800e-07, 1.738e-06),
         'adamw_b999': (2.143e-06, 4.800e-07, 1.806e-06),
         'chain': (1.908e-06, 4.092e-07, 2.207e-06)}
