"""csrc/optim.hip through haloop_amd.ops against the float64 restatements of tests/optim_ref.py: halo_adamw, halo_adamw_ranges(_dev),
halo_adamw_multi off its aligned path, halo_sumsq, halo_clip_coef_step, the trainer's clip -> AdamW chain, halo_scale_add_guarded and the
bf16 wire casts.

Inputs (optim_ref.make_inputs): element i has its own scale s_i, log-uniform in [1e-10, 1e2]; g_t[i] = s_i * N(0, 1); 1 % of the elements
have g == 0 at every step; p ~ N(0, 1).  Below s_i = 1e-8 the eps of the denominator decides the update.  lr 1e-2, wd 0.1, eps 1e-8 and the
betas are the float32 values a C float argument carries (optim_ref.f32).

The comparison (optim_ref.max_err, one function for every test and for tests/test_optim_ref_cpu.py): max over EVERY element of
|got - want| / (|want| + scale), scale = 1 for p, the absolute-value first-moment recurrence for m (optim_ref.mabs_next), 0 for v.

Gates: 4 x the error of optim_ref.f32_restatement (the same step in float32 on the CPU, one rounding per operation) against float64,
measured on the CPU after the last step at the largest size (optim_ref.GATES; test_optim_ref_cpu.py recomputes them and fails if the
constants drift).
The GPU column is the worst error over every step, size and gradient scale of the tests that use the gate, on an MI355X (each test
prints its figures on lines beginning with GPUERR).  Every GPU figure is between 0.97 and 1.24 times the float32 restatement's own
error, i.e. about a quarter of its gate (0.31 at most, v under adamw_b95): the kernels round about as often as the restatement does.

    gate           output   f32 restatement   gate (4 x)    GPU measured
    adamw_b95      p        5.128e-07         2.051e-06     5.299e-07
    adamw_b95      m        1.200e-07         4.800e-07     1.164e-07
    adamw_b95      v        4.345e-07         1.738e-06     5.366e-07
    adamw_b999     p        5.358e-07         2.143e-06     5.502e-07
    adamw_b999     m        1.200e-07         4.800e-07     1.164e-07
    adamw_b999     v        4.516e-07         1.806e-06     4.779e-07
    chain (b999)   p        4.771e-07         1.908e-06     4.771e-07
    chain (b999)   m        1.023e-07         4.092e-07     1.197e-07
    chain (b999)   v        5.517e-07         2.207e-06     5.411e-07

halo_sumsq: rtol = 4 x the error of a float32 pairwise sum (numpy) of the same squares against float64, per size (optim_ref.sumsq_case):
    n = 1: 2.278e-07, n = 3: 1.079e-07, n = 5: 5.152e-08, n = 1048583: 6.738e-08
    GPU measured (at n = 1, 3 and 5 the kernel's sum is the numpy sum bit for bit, a quarter of the gate by construction):
                   n = 1: 5.695e-08, n = 3: 2.697e-08, n = 5: 1.288e-08, n = 1048583: 5.291e-10

Casts, skipped updates, gaps, canaries, counters and the launch forms against each other are compared bit for bit."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GATES = R.GATES
CANARY = 64
U = 2.0 ** -24            # float32 unit roundoff


@pytest.fixture(scope='module')
def ops():
    from haloop_amd import _lib, ops
    _lib.lib()
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def with_canary(host, dtype=torch.float32):
    """(whole, view of the first n): a device buffer of n + CANARY elements holding ``host`` (numpy or a number to fill with) and a canary
    pattern behind it."""
    n = len(host)
    whole = torch.empty(n + CANARY, dtype=dtype, device=DEV)
    whole[:n] = torch.as_tensor(np.asarray(host)).to(dtype)
    whole[n:] = (torch.arange(CANARY, dtype=torch.float32) * 1.25 - 37.5).to(dtype)
    return whole, whole[:n]


def canary_intact(whole):
    n = whole.numel() - CANARY
    return torch.equal(whole[n:].float().cpu(), (torch.arange(CANARY, dtype=torch.float32) * 1.25 - 37.5).to(whole.dtype).float())


def host(*ts):
    return tuple(t.detach().cpu().numpy() for t in ts)


def report(what, errs):
    print(f'GPUERR {what}: ' + ' '.join(f'{e:.4e}' for e in errs))


# ---- a. halo_adamw ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('scale', [None, 0.5, float('nan')], ids=['noscale', 'half', 'nan'])
@pytest.mark.parametrize('betas', list(R.BETAS))
@pytest.mark.parametrize('n', R.ADAMW_SIZES)
def test_adamw_twelve_steps_from_zero_moments_against_float64(ops, n, betas, scale):
    """p, m and v after EVERY one of 12 consecutive steps, no element left out (a zero gradient gives a zero update on both sides, so the
    reference has no sign ambiguity).  The largest size is one full pass of the 2048-workgroup grid, part of a second and a scalar tail.
    A NaN scale leaves all three buffers bit for bit unchanged."""
    p0, g, _ = R.adamw_inputs(n)
    b1, b2 = R.BETAS[betas]
    Pw, P = with_canary(p0)
    Mw, M = with_canary(np.zeros(n, np.float32))
    Vw, V = with_canary(np.zeros(n, np.float32))
    Gw, G = with_canary(g[0])
    gs = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
    skipped = scale is not None and scale != scale
    before = [x.clone() for x in (P, M, V)]
    mabs, worst = np.zeros(n), (0.0, 0.0, 0.0)
    for k, want in enumerate(R.run_steps(R.adamw_step, p0, g, R.LR, b1, b2, R.EPS, R.WD, scale)):
        G.copy_(torch.from_numpy(g[k]))
        ops.adamw(P, G, M, V, R.LR, b1, b2, R.EPS, R.WD, k + 1, gs)
        if skipped:
            assert all(same_bits(a, b) for a, b in zip((P, M, V), before)), k
            continue
        mabs = R.mabs_next(mabs, g[k], b1, scale)
        errs = R.state_err(host(P, M, V), want, R.step_scales(mabs))
        worst = tuple(max(a, b) for a, b in zip(worst, errs))
        assert R.within(errs, GATES['adamw_' + betas]), (k + 1, errs)
    report(f'adamw_{betas} n={n} scale={scale}', worst)
    assert all(canary_intact(w) for w in (Pw, Mw, Vw, Gw))
    assert torch.equal(G.cpu(), torch.from_numpy(g[-1]))                   # the gradient is read only


@pytest.mark.parametrize('betas', list(R.BETAS))
@pytest.mark.parametrize('t', R.LATE_STEPS)
def test_adamw_single_late_steps_from_consistent_moments(ops, t, betas):
    """One update at step 1000 and at step 100000 (b1^t underflows towards 0, the corrections towards 1) at every size."""
    b1, b2 = R.BETAS[betas]
    worst = (0.0, 0.0, 0.0)
    for n in R.ADAMW_SIZES:
        p0, g, s = R.adamw_inputs(n)
        m0, v0 = R.make_moments(s, g[0], 5)
        for scale in (None, 0.5, float('nan')):
            Pw, P = with_canary(p0)
            Mw, M = with_canary(m0)
            Vw, V = with_canary(v0)
            Gw, G = with_canary(g[0])
            gs = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
            ops.adamw(P, G, M, V, R.LR, b1, b2, R.EPS, R.WD, t, gs)
            if scale != scale and scale is not None:
                assert same_bits(P.cpu(), torch.from_numpy(p0)) and same_bits(M.cpu(), torch.from_numpy(m0)) and same_bits(V.cpu(), torch.from_numpy(v0))
            else:
                want = R.adamw_step(p0, g[0], m0, v0, R.LR, b1, b2, R.EPS, R.WD, t, scale)
                errs = R.state_err(host(P, M, V), want, R.step_scales(R.mabs_next(np.abs(m0), g[0], b1, scale)))
                worst = tuple(max(a, b) for a, b in zip(worst, errs))
                assert R.within(errs, GATES['adamw_' + betas]), (n, scale, errs)
            assert all(canary_intact(w) for w in (Pw, Mw, Vw, Gw))
    report(f'adamw_{betas} late t={t}', worst)


# ---- b. halo_adamw_ranges, host step -----------------------------------------------------------------------------------------------------

GAP_M, GAP_V = 3.25, 5.5           # what the gaps of m and v hold (the gaps of g hold NaN, those of p the initial p)


def _ranges_buffers():
    p0, g, _, ranges, inside = R.ranges_inputs()
    m0 = np.where(inside, 0.0, GAP_M).astype(np.float32)
    v0 = np.where(inside, 0.0, GAP_V).astype(np.float32)
    scales = {}
    dev_ranges = []
    for a, b, wd, sc in ranges:
        if sc is not None and repr(sc) not in scales:
            scales[repr(sc)] = torch.tensor([sc], dtype=torch.float32, device=DEV)
        dev_ranges.append((a, b, wd, None if sc is None else scales[repr(sc)]))
    dev = [torch.from_numpy(x).to(DEV) for x in (p0, g[0], m0, v0)]
    return p0, g, m0, v0, ranges, inside, dev_ranges, dev


def _ranges_launches(ops, on_step=None):
    """RANGES_STEPS launches of the 8-range buffer from zero moments -> (P, M, V, counter) on the device."""
    p0, g, m0, v0, ranges, inside, dev_ranges, (P, G, M, V) = _ranges_buffers()
    b1, b2 = R.BETAS['b95']
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(R.RANGES_STEPS):
        G.copy_(torch.from_numpy(g[k]))
        ops.adamw_ranges(P, G, M, V, dev_ranges, R.LR, b1, b2, R.EPS, k + 1, counter=ctr)
        if on_step:
            on_step(k, P, M, V, ctr)
    return P, M, V, ctr


def ranges_digest(ops=None):
    """sha256 over the bits of p, m and v after the launches of _ranges_launches (also what the HALO_ADAMW_NT=0 child prints)."""
    if ops is None:
        from haloop_amd import ops
    P, M, V, _ = _ranges_launches(ops)
    h = hashlib.sha256()
    for x in (P, M, V):
        h.update(x.cpu().numpy().tobytes())
    return h.hexdigest()


def test_adamw_ranges_eight_ranges_with_gaps_against_float64(ops):
    """8 ranges of one flat buffer passed out of order: one empty, one of 4 elements, one longer than a pass of the 4096-workgroup grid;
    weight decays {0, 0.1, 0.3}; scales NULL, 0.25, 1.0 and NaN (that range is skipped, its neighbours are not); the gaps' bits stay, NaN
    canaries in the gaps of g never arrive anywhere; the counter advances by 1 per launch."""
    p0, g, m0, v0, ranges, inside, _, _ = _ranges_buffers()
    b1, b2 = R.BETAS['b95']
    assert max(b - a for a, b, _, _ in ranges) > 4096 * 256 * 4 and any(a == b for a, b, _, _ in ranges)
    assert [r[0] for r in ranges] != sorted(r[0] for r in ranges)
    gaps = torch.from_numpy(~inside)
    nan_a, nan_b = [(a, b) for a, b, _, sc in ranges if sc is not None and sc != sc][0]
    state = {'ref': (p0, m0, v0), 'mabs': np.zeros(len(p0)), 'worst': (0.0, 0.0, 0.0)}

    def check(k, P, M, V, ctr):
        gk = np.where(inside, g[k], 0.0)
        pr, mr, vr = state['ref']
        state['ref'] = want = R.ranges_step(pr, gk, mr, vr, ranges, R.LR, b1, b2, R.EPS, k + 1)
        state['mabs'] = R.ranges_mabs(state['mabs'], gk, ranges, b1)
        got = host(P, M, V)
        errs = R.state_err(got, want, R.ranges_scales(state['mabs'], ranges))
        state['worst'] = tuple(max(a, b) for a, b in zip(state['worst'], errs))
        assert R.within(errs, GATES['adamw_b95']), (k, errs)
        for x, x0 in zip((P, M, V), (p0, m0, v0)):
            x, x0 = x.cpu(), torch.from_numpy(x0)
            assert same_bits(x[gaps], x0[gaps]) and same_bits(x[nan_a:nan_b], x0[nan_a:nan_b])
        assert not np.array_equal(got[0][nan_a - 8:nan_a], p0[nan_a - 8:nan_a]) and not np.array_equal(got[0][nan_b + 8:nan_b + 16], p0[nan_b + 8:nan_b + 16])
        assert int(ctr.item()) == k + 1

    _ranges_launches(ops, check)
    report('adamw_b95 ranges', state['worst'])


def test_adamw_ranges_counter_advances_when_every_range_is_skipped(ops):
    n = 1024
    p0, g, s = R.make_inputs(n, 1, 12)
    P, G, M, V = (torch.from_numpy(x).to(DEV) for x in (p0, g[0], p0 * 0.25, p0 * p0))
    before = [x.clone() for x in (P, M, V)]
    nan = torch.tensor([float('nan')], device=DEV)
    ctr = torch.full((1,), 41, dtype=torch.int32, device=DEV)
    for k in range(2):
        ops.adamw_ranges(P, G, M, V, [(0, 512, 0.1, nan), (512, 1024, 0.0, nan)], R.LR, 0.9, 0.95, R.EPS, 3, counter=ctr)
        assert int(ctr.item()) == 42 + k
    assert all(same_bits(a, b) for a, b in zip((P, M, V), before))
    ops.adamw_ranges(P, G, M, V, [(0, 512, 0.1, nan), (512, 1024, 0.0, None)], R.LR, 0.9, 0.95, R.EPS, 3)      # no counter: NULL is allowed
    assert same_bits(P[:512], before[0][:512]) and not torch.equal(P[512:], before[0][512:])


def test_adamw_ranges_plain_loads_give_the_same_bits_in_a_fresh_process(ops):
    """HALO_ADAMW_NT=0 (plain instead of non-temporal loads and stores) is read once per process, so the other setting needs a fresh one."""
    assert not os.environ.get('HALO_ADAMW_NT', '').startswith('0')
    mine = ranges_digest(ops)
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_optim as t; print("DIGEST", t.ranges_digest())'
            % (ROOT, os.path.join(ROOT, 'tests')))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, HALO_ADAMW_NT='0'), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith('DIGEST')]
    assert theirs == [mine]


def test_adamw_ranges_refusals_launch_nothing(ops):
    from haloop_amd._lib import HaloError
    n = 4096
    p0, g, s = R.make_inputs(n + 8, 1, 13)
    P, G, M, V = (torch.from_numpy(x).to(DEV) for x in (p0, g[0], p0 * 0.25, p0 * p0))
    before = [x.clone() for x in (P, M, V)]
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    step_dev = torch.ones(1, dtype=torch.int32, device=DEV)
    one = [(0, n, 0.1, None)]
    refused = [
        ('nine ranges', (P, G, M, V), [(8 * i, 8 * i + 8, 0.1, None) for i in range(9)]),
        ('begin % 4', (P, G, M, V), [(2, 10, 0.1, None)]),
        ('end % 4', (P, G, M, V), [(4, 10, 0.1, None)]),
        ('end < begin', (P, G, M, V), [(0, 8, 0.1, None), (16, 8, 0.1, None)]),
        ('p off 16 bytes', (P[1:], G, M, V), one),
        ('g off 16 bytes', (P, G[2:], M, V), one),
        ('m off 16 bytes', (P, G, M[3:], V), one),
        ('v off 16 bytes', (P, G, M, V[1:]), one),
    ]
    for what, bufs, ranges in refused:
        for step in (1, step_dev):
            with pytest.raises(HaloError):
                ops.adamw_ranges(*bufs, ranges, R.LR, 0.9, 0.95, R.EPS, step, counter=ctr)
    with pytest.raises(HaloError):
        ops.adamw_ranges(P, G, M, V, one, R.LR, 0.9, 0.95, R.EPS, 0, counter=ctr)           # a host step count is 1-based
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((P, M, V), before)) and int(ctr.item()) == 0
    ops.adamw_ranges(P, G, M, V, [(8 * i, 8 * i + 8, 0.1, None) for i in range(8)], R.LR, 0.9, 0.95, R.EPS, 1, counter=ctr)   # 8 are accepted
    assert int(ctr.item()) == 1 and not torch.equal(P[:64], before[0][:64]) and same_bits(P[64:], before[0][64:])


# ---- c. halo_adamw_ranges_dev ----------------------------------------------------------------------------------------------------------------

def _dev_ranges(tensors):
    return [(a, b, wd, None if sc is None else tensors[sc]) for a, b, wd, sc in R.DEV_RANGES]


@pytest.mark.parametrize('t', R.DEV_STEPS)
def test_adamw_ranges_device_step_count(ops, t):
    """The update count read from a device int32 (0 acts as 1): float64 at that t, and the host-step form's bits."""
    p0, g, m0, v0 = R.dev_inputs()
    b1, b2 = R.BETAS['b95']
    sc = {0.25: torch.tensor([0.25], device=DEV), 1.0: torch.tensor([1.0], device=DEV)}
    ranges = _dev_ranges(sc)
    forms = {}
    for form in ('dev', 'dev_lr', 'host'):
        P, G, M, V = (torch.from_numpy(x).to(DEV) for x in (p0, g[0], m0, v0))
        step = torch.tensor([t], dtype=torch.int32, device=DEV) if form != 'host' else max(t, 1)
        lr = torch.tensor([R.LR], dtype=torch.float32, device=DEV) if form == 'dev_lr' else R.LR
        ops.adamw_ranges(P, G, M, V, ranges, lr, b1, b2, R.EPS, step)
        forms[form] = (P, M, V)
        if form != 'host':
            assert int(step.item()) == t                                     # the count is read, never written
    want = R.ranges_step(p0, g[0], m0, v0, R.DEV_RANGES, R.LR, b1, b2, R.EPS, max(t, 1))
    mabs = R.ranges_mabs(np.abs(m0) * np.isin(np.arange(R.DEV_N), np.concatenate([np.arange(a, b) for a, b, _, _ in R.DEV_RANGES])),
                         g[0], R.DEV_RANGES, b1)
    errs = R.state_err(host(*forms['dev']), want, R.ranges_scales(mabs, R.DEV_RANGES))
    report(f'adamw_b95 ranges_dev t={t}', errs)
    assert R.within(errs, GATES['adamw_b95']), errs
    for form in ('dev_lr', 'host'):
        assert all(same_bits(a, b) for a, b in zip(forms['dev'], forms[form])), form


def test_adamw_ranges_device_lr_changes_between_launches(ops):
    """lr read from a device float that changes from launch to launch: the decay factor 1 - lr * wd follows the CURRENT lr (a factor formed
    from the previous one is off by |lr - lr'| * wd, 1.7e-3 here)."""
    p0, g, _, _ = R.dev_inputs()
    b1, b2 = R.BETAS['b95']
    sc = {0.25: torch.tensor([0.25], device=DEV), 1.0: torch.tensor([1.0], device=DEV)}
    ranges = _dev_ranges(sc)
    z = np.zeros_like(p0)
    P, M, V = (torch.from_numpy(x).to(DEV) for x in (p0, z, z))
    Ph, Mh, Vh = (torch.from_numpy(x).to(DEV) for x in (p0, z, z))
    G = torch.empty_like(P)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    mabs, worst = np.zeros(R.DEV_N), (0.0, 0.0, 0.0)
    for k, want in enumerate(R.changing_lr_run(R.adamw_step)):
        G.copy_(torch.from_numpy(g[k]))
        cnt.fill_(k + 1)
        lr_dev.fill_(R.DEV_LRS[k])
        ops.adamw_ranges(P, G, M, V, ranges, lr_dev, b1, b2, R.EPS, cnt)
        ops.adamw_ranges(Ph, G, Mh, Vh, ranges, R.DEV_LRS[k], b1, b2, R.EPS, k + 1)
        mabs = R.ranges_mabs(mabs, g[k], R.DEV_RANGES, b1)
        errs = R.state_err(host(P, M, V), want, R.ranges_scales(mabs, R.DEV_RANGES))
        worst = tuple(max(a, b) for a, b in zip(worst, errs))
        assert R.within(errs, GATES['adamw_b95']), (k, errs)
        assert all(same_bits(a, b) for a, b in zip((P, M, V), (Ph, Mh, Vh))), k
    report('adamw_b95 ranges_dev changing lr', worst)


# ---- d. halo_adamw_multi off the aligned path ------------------------------------------------------------------------------------------------

MULTI_SIZES = (5, 16384, 16384 + 1, 2 * 16384 + 5)
MULTI_STEPS = 3


def test_adamw_multi_on_four_byte_aligned_views(ops):
    """nn.Parameter views of one flat buffer at element offsets 1, 2 and 3 (the scalar path of the kernel: no tensor of the suite's other
    AdamWMulti test is off a 16-byte boundary), and parameters whose GRADIENT alone is misaligned: float64 within the gates, and the
    bits of halo_adamw on aligned copies of the same values."""
    b1, b2 = R.BETAS['b999']
    cases = [(n, off, 0) for n in MULTI_SIZES for off in (1, 2, 3)] + [(n, 0, 1 + i % 3) for i, n in enumerate(MULTI_SIZES)]
    wds = [R.f32((0.0, 0.1, 0.3)[i % 3]) for i in range(len(cases))]
    slot = lambda n: (n + 3) // 4 * 4 + 8                                  # a 16-byte aligned slot with room for the offset and a gap
    total = sum(slot(n) for n, _, _ in cases)
    p_all, g_all, _ = R.make_inputs(total, MULTI_STEPS, 31)
    flat_p = torch.from_numpy(p_all).to(DEV)
    flat_g = torch.zeros(total, device=DEV)
    where, at = [], 0
    for n, off, goff in cases:
        where.append((at + off, at + goff, n))
        at += slot(n)
    params = [torch.nn.Parameter(flat_p[a:a + n]) for a, _, n in where]
    assert all(q.data_ptr() % 16 == 4 * c[1] and q.data_ptr() % 4 == 0 for q, c in zip(params, cases))
    opt = ops.AdamWMulti(params, wds, R.LR, betas=(b1, b2), eps=R.EPS)
    gs = torch.tensor([0.5], device=DEV)
    # aligned twins, one halo_adamw launch each
    twins = [[torch.from_numpy(np.ascontiguousarray(x)).to(DEV).clone() for x in (p_all[a:a + n], np.zeros(n, np.float32), np.zeros(n, np.float32))]
             for a, _, n in where]
    ref = [(p_all[a:a + n], np.zeros(n), np.zeros(n)) for a, _, n in where]
    mabs = [np.zeros(n) for _, _, n in where]
    untouched = torch.ones(total, dtype=torch.bool)
    for a, _, n in where:
        untouched[a:a + n] = False
    worst = (0.0, 0.0, 0.0)
    for k in range(MULTI_STEPS):
        for q, (a, ga, n), c in zip(params, where, cases):
            flat_g[ga:ga + n] = torch.from_numpy(g_all[k, a:a + n]).to(DEV)
            q.grad = flat_g[ga:ga + n]
            assert q.grad.data_ptr() % 16 == 4 * c[2]
        opt.step(grad_scale=gs)
        for i, (q, (a, ga, n)) in enumerate(zip(params, where)):
            gk = g_all[k, a:a + n]
            tp, tm, tv = twins[i]
            ops.adamw(tp, torch.from_numpy(np.ascontiguousarray(gk)).to(DEV), tm, tv, R.LR, b1, b2, R.EPS, wds[i], k + 1, gs)
            got = (q.detach(), opt.m[i], opt.v[i])
            assert all(same_bits(x, y) for x, y in zip(got, (tp, tm, tv))), (k, cases[i])
            ref[i] = R.adamw_step(*ref[i][:1], gk, *ref[i][1:], R.LR, b1, b2, R.EPS, wds[i], k + 1, 0.5)
            mabs[i] = R.mabs_next(mabs[i], gk, b1, 0.5)
            errs = R.state_err(host(*got), ref[i], R.step_scales(mabs[i]))
            worst = tuple(max(x, y) for x, y in zip(worst, errs))
            assert R.within(errs, GATES['adamw_b999']), (k, cases[i], errs)
    report('adamw_b999 multi', worst)
    assert same_bits(flat_p.cpu()[untouched], torch.from_numpy(p_all)[untouched])          # nothing between the views moved


# ---- e. halo_sumsq, halo_clip_coef_step ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', R.SUMSQ_SIZES)
def test_sumsq_partials_against_float64(ops, n):
    from haloop_amd import _lib
    x, want, rtol = R.sumsq_case(n)
    Xw, X = with_canary(x)
    Xw[n:] = float('nan')                                                   # anything read past n poisons the sum
    a = ops.sumsq_partials(X, torch.full((_lib.HALO_SUMSQ_PARTS,), float('nan'), device=DEV))
    b = ops.sumsq_partials(X)
    assert same_bits(a, b)                                                  # fixed order: two launches, identical bits
    got = float(a.double().sum().item())
    print(f'GPUERR sumsq n={n}: {abs(got - want) / want:.4e} (rtol {rtol:.4e})')
    assert abs(got - want) <= rtol * want


def _clip(ops, partials, count, max_norm, with_norm=True, steps=7):
    parts = torch.full((1024,), 1e30, device=DEV)                           # what lies behind `count` must not be read
    parts[:count] = torch.as_tensor(partials, dtype=torch.float32)
    coef = torch.full((2,), -5.0, device=DEV)
    norm = torch.full((1,), -5.0, device=DEV) if with_norm else None
    cnt = torch.full((1,), steps, dtype=torch.int32, device=DEV)
    ops.clip_coef(parts, count, max_norm, coef, norm, applied_steps=cnt)
    return coef.cpu().numpy(), (None if norm is None else float(norm.item())), int(cnt.item())


@pytest.mark.parametrize('count', [1, 255, 256, 1024])
def test_clip_coef_on_known_partials(ops, count):
    """Small integer partials: their float32 sum is exact in any order, so what is left is sqrt, + 1e-6 and the division, half an ulp
    each: 4 * 2^-24 covers them with room."""
    gen = torch.Generator().manual_seed(count)
    ints = torch.randint(0, 8, (count,), generator=gen).float()
    ints[0] = 5.0
    total = float(ints.double().sum())
    norm64 = total ** 0.5
    # norm exactly 0
    coef, norm, cnt = _clip(ops, torch.zeros(count), count, 1.0)
    assert coef.tolist() == [1.0, 1.0] and norm == 0.0 and cnt == 8
    # below max_norm: 1
    coef, norm, cnt = _clip(ops, ints, count, R.f32(norm64 * 1.5))
    assert coef.tolist() == [1.0, 1.0] and cnt == 8 and abs(norm - norm64) <= U * norm64
    # above: max_norm / (norm + 1e-6)
    for max_norm in (R.f32(norm64 * 0.75), R.f32(1e-3), R.f32(norm64 * (1 - 1e-5))):
        for with_norm in (True, False):
            coef, norm, cnt = _clip(ops, ints, count, max_norm, with_norm)
            want = R.clip_coef(total, max_norm)[0]
            assert want < 1.0 and abs(float(coef[0]) - want) <= 4 * U * want, (coef, want)
            assert coef[1] == 1.0 and cnt == 8 and (norm is None) == (not with_norm)
    # the counter may be absent
    parts = torch.ones(1024, device=DEV)
    coef = torch.zeros(2, device=DEV)
    ops.clip_coef(parts, count, 1e9, coef, None)
    assert coef.tolist() == [1.0, 1.0]


@pytest.mark.parametrize('count', [1, 255, 256, 1024])
def test_clip_coef_non_finite_norms_poison_both_scales_and_keep_the_count(ops, count):
    big = 3.0e38
    cases = {'inf': [float('inf')] + [1.0] * (count - 1), 'nan': [1.0] * (count - 1) + [float('nan')]}
    if count > 1:
        cases['overflow'] = [big, big] + [1.0] * (count - 2)                 # finite partials, a sum past the largest float
        cases['inf in the middle'] = [1.0] * (count // 2) + [float('inf')] + [1.0] * (count - count // 2 - 1)
    for what, partials in cases.items():
        coef, norm, cnt = _clip(ops, partials, count, 1.0)
        assert np.isnan(coef).all() and cnt == 7 and not np.isfinite(norm), (what, coef, norm, cnt)


# ---- f. the trainer's chain ------------------------------------------------------------------------------------------------------------------

def test_clip_then_adamw_chain_over_25_steps_against_torch_float64(ops):
    """sumsq over the clipped range -> clip_coef(applied_steps) -> adamw_ranges(step and lr on the device, dropout counter) as
    train.py:_apply_update issues them, four ranges in the trainer's (decay, clip) classes, a warm-up / decay schedule written into the
    device lr, some steps clipped and some not, and one step whose gradient carries an Inf: nothing moves, the update count stays, the
    dropout counter advances, and the next step continues at the un-advanced count.  Against torch.optim.AdamW + clip_grad_norm_ in
    float64 (optim_ref.torch_chain)."""
    from haloop_amd import _lib
    want, ref = R.torch_chain(), R.chain_run()
    n, classes = R.chain_layout()
    p0, g = R.chain_inputs()
    b1, b2 = R.BETAS['b999']
    lo, hi = R.CHAIN_CLIPPED
    Pw, P = with_canary(p0)
    Mw, M = with_canary(np.zeros(n, np.float32))
    Vw, V = with_canary(np.zeros(n, np.float32))
    Gw, G = with_canary(g[0])
    parts = torch.zeros(_lib.HALO_SUMSQ_PARTS, device=DEV)
    coef, norm = torch.ones(2, device=DEV), torch.zeros(1, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.zeros(1, device=DEV)
    ranges = [(a, b, R.CHAIN_WD if decays else 0.0, coef[0:1] if clipped else coef[1:2]) for a, b, decays, clipped in classes]
    worst, clipped_steps = (0.0, 0.0, 0.0), 0
    for k in range(R.CHAIN_STEPS):
        before = [x.clone() for x in (P, M, V)]
        G.copy_(torch.from_numpy(g[k]))
        lr_dev.fill_(ref[k]['lr'])
        ops.sumsq_partials(G[lo:hi], parts)
        ops.clip_coef(parts, _lib.HALO_SUMSQ_PARTS, R.CHAIN_MAX_NORM, coef, norm, applied_steps=cnt)
        ops.adamw_ranges(P, G, M, V, ranges, lr_dev, b1, b2, R.EPS, cnt, counter=ctr)
        assert int(cnt.item()) == want[k]['applied'] and int(ctr.item()) == k + 1
        if k == R.CHAIN_INF_STEP:
            assert all(same_bits(a, b) for a, b in zip((P, M, V), before)) and torch.isnan(coef).all()
            assert int(cnt.item()) == k
            continue
        c = float(coef[0].item())
        assert abs(c - ref[k]['coef']) <= 8 * U and float(coef[1].item()) == 1.0
        clipped_steps += c < 1.0
        errs = R.state_err(host(P, M, V), [want[k][x] for x in 'pmv'], ref[k]['scales'])
        worst = tuple(max(a, b) for a, b in zip(worst, errs))
        assert R.within(errs, GATES['chain']), (k, errs)
    assert 5 <= clipped_steps <= R.CHAIN_STEPS - 6
    assert int(cnt.item()) == R.CHAIN_STEPS - 1
    assert all(canary_intact(w) for w in (Pw, Mw, Vw, Gw))
    report('chain', worst)


# ---- g. halo_scale_add_guarded ---------------------------------------------------------------------------------------------------------------

SCALE_ADD_SIZES = (1, 3, 4, 5, 1024 * 4, 1024 * 4 + 3)


@pytest.mark.parametrize('n', SCALE_ADD_SIZES)
def test_scale_add_against_float64_and_its_guards(ops, n):
    """y <- alpha * y + beta * x.  Two products and a sum, half an ulp each relative to |alpha * y| + |beta * x| (less where the compiler
    fuses one): the gate is 2 * 2^-24 in optim_ref.max_err with that scale.  n = 4096: the tail thread i == n / 4 is alone in an extra
    workgroup."""
    y0, x0, _ = R.make_inputs(n, 1, 400 + n)
    x0 = x0[0]
    alpha, beta = R.f32(0.75), R.f32(-1.3)
    X = with_canary(x0)
    Yw, Y = with_canary(y0)
    ops.scale_add_(Y, X[1], alpha, beta)
    want = alpha * y0.astype(np.float64) + beta * x0.astype(np.float64)
    operands = np.abs(alpha * y0.astype(np.float64)) + np.abs(beta * x0.astype(np.float64))
    err = R.max_err(Y.cpu().numpy(), want, operands)
    print(f'GPUERR scale_add n={n}: {err:.4e} (gate {2 * U:.4e})')
    assert err <= 2 * U
    assert canary_intact(Yw) and canary_intact(X[0]) and torch.equal(X[1].cpu(), torch.from_numpy(x0))
    beta_x = torch.from_numpy(np.float32(beta) * x0)
    alpha_y = torch.from_numpy(np.float32(alpha) * y0)
    poison = np.where(np.arange(n) % 3 == 0, np.nan, np.where(np.arange(n) % 3 == 1, np.inf, -np.inf)).astype(np.float32)
    for guard, takes_x in ((None, True), (1.5, True), (0.0, True), (float('inf'), False), (float('-inf'), False), (float('nan'), False)):
        gd = None if guard is None else torch.tensor([guard], device=DEV)
        # alpha == 0 never reads y: a poisoned accumulator does not survive
        Yw, Y = with_canary(poison)
        ops.scale_add_(Y, X[1], 0.0, beta, guard=gd)
        assert torch.equal(Y.cpu(), beta_x if takes_x else torch.zeros(n)), guard
        assert canary_intact(Yw)
        # alpha != 0: a dropped x leaves alpha * y
        Yw, Y = with_canary(y0)
        ops.scale_add_(Y, X[1], alpha, beta, guard=gd)
        if takes_x:
            assert R.max_err(Y.cpu().numpy(), want, operands) <= 2 * U
        else:
            assert torch.equal(Y.cpu(), alpha_y), guard
        assert canary_intact(Yw)
    # y is x, in place, as lora.py scales its update: scale_add_(t, t, 0.0, s) == s * t
    Tw, T = with_canary(x0)
    ops.scale_add_(T, T, 0.0, beta)
    assert torch.equal(T.cpu(), beta_x) and canary_intact(Tw)


# ---- h. the wire casts -------------------------------------------------------------------------------------------------------------------------

CAST_SIZES = (1, 3, 4, 5, 2048 * 256 * 4 + 5)


def _cast_values(n):
    """Ties in both directions, signed zeros and infinities, NaN, the largest finite float (rounds to inf), float32 denormals, then
    random bit patterns; cycled to n (the small sizes begin at different specials)."""
    f = np.float32
    special = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, np.inf, -np.inf, np.nan,
                        np.finfo(f).max, -np.finfo(f).max, 1e-45, -1e-45, 1e-39, 5.9e-39, -3e-41, np.finfo(f).tiny,
                        1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 3.3895314e38], dtype=f)
    gen = torch.Generator().manual_seed(8)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (4096,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32).numpy()
    pool = np.concatenate([special, rnd])
    return np.resize(np.roll(pool, -2 * n if n < len(special) else 0), n)


def _same_bits_or_both_nan(got, want):
    nan = torch.isnan(want.float())
    return torch.equal(torch.isnan(got.float()), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.parametrize('n', CAST_SIZES)
def test_wire_casts_round_to_nearest_even_like_torch(ops, n):
    x = torch.from_numpy(_cast_values(n))
    want = x.to(torch.bfloat16)
    Xw, X = with_canary(x.numpy())
    Yw, Y = with_canary(np.zeros(n, np.float32), torch.bfloat16)
    ops.cast_f32_to_bf16_(Y, X)
    assert _same_bits_or_both_nan(Y.cpu(), want)
    assert canary_intact(Yw) and canary_intact(Xw)
    # and back: float32(x) * float32(scale), scale 1 exact
    for scale in (1.0, 1.0 / 3.0, 0.125):
        Bw, B = with_canary(np.zeros(n, np.float32), torch.bfloat16)
        B.copy_(want)
        Zw, Z = with_canary(np.full(n, 7.0, np.float32))
        ops.cast_bf16_to_f32_(Z, B, scale)
        back = want.float() * torch.tensor(scale, dtype=torch.float32)
        assert _same_bits_or_both_nan(Z.cpu(), back), scale
        assert canary_intact(Zw) and canary_intact(Bw)
