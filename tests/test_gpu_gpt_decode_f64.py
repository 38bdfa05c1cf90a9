"""The three launches of a GPT sampling step (csrc/gpt_decode.hip, csrc/decode_linear.h: halo_gpt_decode_linear, halo_gpt_decode_attention,
halo_gpt_sample) against float64 under each math mode's own operand rounding (tests/gpt_decode_ref.py), per dispatched
instantiation.

The linear and attention outputs are held to max(8 x the fp32 stand-in's own deviation from the float64 reference, 2^-22) in units of the
per-element scale S; operands sit in front of NaN guard bands and the output buffers are wider than what may be written; every draw of
every line must lie in the float64 CDF interval of its uniform.  Observed device / bound ratios: DESIGN.md 5e."""
import numpy as np
import pytest
import torch

import gpt_decode_ref as R
from test_gpu_decode import _nan_guarded_image, _nan_guarded_x
from test_gpu_generation import run_draws

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
I32 = torch.int32


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops
    _lib.lib()
    _lib.lend_scratch()
    return dict(ops=ops, lib=_lib)


class _Mode:
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.prev = self.lib.get_math_mode()
        self.lib.set_math_mode(self.mode)

    def __exit__(self, *exc):
        self.lib.set_math_mode(self.prev)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


def _guarded_rows(x, spare=4):
    """x [rows, K] as a view with row stride K + spare of a NaN-filled buffer with a NaN guard band behind the last row."""
    rows, K = x.shape
    wide = torch.full((rows, K + spare), float('nan'))
    wide[:, :K] = x
    v = _nan_guarded_x(wide)[:, :K]
    assert v.stride(0) == K + spare and v.data_ptr() % 16 == 0
    return v


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gpt_decode_linear
# ------------------------------------------------------------------------------------------------------------------------------
LIN = [(c, m) for c in R.LINEAR_CASES for m in R.MODES]


@pytest.mark.parametrize('case,mode', LIN, ids=[f'{c.name}-{m}' for c, m in LIN])
def test_linear_matches_float64_per_instantiation(hal, case, mode):
    ops = hal['ops']
    inp = R.linear_inputs(case.name)
    pl = R.plan(case.rows, case.K, case.n_out, case.ln)
    xg = _guarded_rows(inp['x'])
    with _Mode(hal['lib'], mode):
        assert ops.gpt_decode_linear_supported(case.K, case.ln)
        img = _nan_guarded_image(ops.decode_image(inp['w'].to(DEV)))
        lnw = inp['lnw'].to(DEV) if case.ln else None
        runs = []
        for _ in range(2):
            out = inp['out0'].to(DEV)
            ops.gpt_decode_linear(xg, img, case.n_out, out, ln_weight=lnw, eps=R.EPS, accumulate=case.accum, gelu=case.gelu)
            runs.append(out.cpu())
    got = runs[0]
    assert _same_bits(got, runs[1])                                                  # the same bits on every run
    assert _same_bits(got[:, case.n_out:], inp['out0'][:, case.n_out:])              # nothing written past the features
    ref, S, bound = R.linear_reference(case.name, mode), R.linear_scale(case, inp), R.linear_bound(case.name, mode)
    dev = R.deviation(got[:, :case.n_out], ref, S)
    print(f'\nlinear {case.name} [{mode}] {pl.label(mode)} walk {pl.walk}: device {dev:.2e} bound {bound:.2e} device/bound {dev / bound:.2f}')
    assert dev <= bound, (dev, bound, 'first (row, col, device, reference):', R.first_outside(got[:, :case.n_out], ref, S, bound))


@pytest.mark.parametrize('mode', R.MODES)
def test_linear_reads_the_image_bit_for_bit(hal, mode):
    """One-hot rows x = I_256 (K = 256, n_out = 40): the output is hi(W) + lo(W) (bf16x3; exact in fp32) or hi(W) (bf16), bit for bit.
    W carries magnitudes from 2^-60 to 2^60, exact ties of the bf16 rounding in hi and in lo, +-0."""
    ops = hal['ops']
    rows, K, n_out = R.BITCHECK
    g = torch.Generator().manual_seed(17)
    w = torch.randn(n_out, K, generator=g) * torch.exp2(torch.randint(-60, 61, (n_out, K), generator=g).float())
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -9 + 2.0 ** -17,
                            1 + 2.0 ** -9 + 3 * 2.0 ** -17, -(1 + 2.0 ** -9 + 2.0 ** -17), 0.0, -0.0])
    w.view(-1)[:len(special)] = special
    w.view(-1)[-len(special):] = special
    hi, lo = R.split(w)
    want = (hi + lo if mode == 'bf16x3' else hi).T.contiguous()                     # [K rows of x, n_out]
    xg = _guarded_rows(torch.eye(K))
    with _Mode(hal['lib'], mode):
        img = _nan_guarded_image(ops.decode_image(w.to(DEV)))
        out = torch.full((rows, n_out + 8), 3.0, device=DEV)
        ops.gpt_decode_linear(xg, img, n_out, out)
    got = out.cpu()
    assert bool((got[:, n_out:] == 3.0).all())
    assert torch.equal(got[:, :n_out], want), ('first difference (row, col):', torch.nonzero(got[:, :n_out] != want)[:1].tolist())


def test_linear_refuses_the_f32_mode(hal):
    ops, lib = hal['ops'], hal['lib']
    x = torch.zeros(4, 256, device=DEV)
    img = ops.decode_image(torch.zeros(16, 256, device=DEV))
    out = torch.full((4, 16), 5.0, device=DEV)
    with _Mode(lib, 'f32'):
        assert not ops.gpt_decode_linear_supported(256, False) and not ops.gpt_decode_linear_supported(768, True)
        with pytest.raises(lib.HaloError):
            ops.gpt_decode_linear(x, img, 16, out)
    assert bool((out == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gpt_decode_attention
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.ATTENTION_CASES, ids=[c.name for c in R.ATTENTION_CASES])
def test_attention_matches_float64_and_keeps_the_cache(hal, case):
    """Rows 0 .. p - 1 of the caches are random, row p and every row above it NaN before the launch: a finite output shows that no key above
    p is read and that row p comes from the registers.  Afterwards row p of both planes is the row's k / v bit for bit and every other cache
    row is what was written; the spare columns of y are untouched; a second run gives the same bits."""
    ops = hal['ops']
    inp = R.attention_inputs(case.name)
    B, H, Tc = case.B, case.heads, case.Tc
    C = H * 64
    p = R.clamped(case)
    above = (torch.arange(Tc)[None, :] >= p[:, None])[:, None, :, None]
    planes = [inp[k].masked_fill(above, float('nan')) for k in ('ck', 'cv')]
    want = []
    rows = torch.arange(B)
    for i, plane in enumerate(planes):
        w = plane.clone()
        w[rows, :, p] = inp['qkv'][:, (1 + i) * C:(2 + i) * C].reshape(B, H, 64)
        want.append(w)
    qkv = _guarded_rows(inp['qkv'])
    pos = inp['pos'].to(DEV)
    runs = []
    for _ in range(2):
        ck, cv = planes[0].to(DEV), planes[1].to(DEV)
        ybuf = torch.full((B, C + 4), float('nan'), device=DEV)
        ops.gpt_decode_attention(qkv, ck, cv, pos, ybuf[:, :C])
        runs.append((ybuf.cpu(), ck.cpu(), cv.cpu()))
        del ck, cv
    (y, ck, cv), second = runs
    assert all(_same_bits(a, b) for a, b in zip(runs[0], second))
    assert bool(torch.isnan(y[:, C:]).all()) and _same_bits(y[:, C:], torch.full((B, 4), float('nan')))
    assert _same_bits(ck, want[0]) and _same_bits(cv, want[1])
    got = y[:, :C]
    assert bool(torch.isfinite(got).all()), 'a key above p was read, or row p came from the cache'
    ref, S = R.attention_reference(case.name)
    bound = R.attention_bound(case.name)
    ratio = R.row_deviation(got, ref, S) / bound
    worst = int(ratio.argmax())
    print(f'\nattention {case.name} <{R.attention_plan(B, H, Tc)}>: worst device/bound {ratio.max().item():.2f} at row {worst} (pos {case.pos[worst]}, '
          f'bound {bound[worst].item():.2e})')
    assert bool((ratio <= 1.0).all()), [(b, case.pos[b], ratio[b].item()) for b in torch.nonzero(ratio > 1.0).flatten().tolist()]


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gpt_sample
# ------------------------------------------------------------------------------------------------------------------------------
def _device_logits(line):
    lg = torch.from_numpy(R.draw_logits(line.name))
    if not line.ld:
        return lg.to(DEV)
    buf = torch.full((R.ROWS, line.ld), float('nan'), device=DEV)
    buf[:, :line.V] = lg.to(DEV)
    return buf[:, :line.V]


SAME_AS_NONE = ('v4100_kV', 'v4100_kVp5')


@pytest.mark.parametrize('line', R.DRAW_LINES, ids=[d.name for d in R.DRAW_LINES])
def test_every_draw_lies_in_the_float64_interval_of_its_uniform(line):
    logits = _device_logits(line)
    assert logits.stride(0) == (line.ld or line.V)
    tokens = run_draws(logits, R.STEPS, line.T, line.top_k, R.SEED)
    assert tokens.min() >= 0 and tokens.max() < line.V
    keep = R.kept(R.draw_logits(line.name), line)
    outside = ~keep[np.arange(R.ROWS)[:, None], tokens]
    assert not outside.any(), f'{int(outside.sum())} draws outside the kept set'
    ok = R.draws_accepted(line.name, tokens)
    delta, worst = R.draw_delta(line.name)
    rejected = int((~R.draws_accepted(line.name, tokens, 'uniform_of_next_step')).sum())
    print(f'\ndraw {line.name}: delta {delta:.1e}, accepted {int(ok.sum())} of {ok.size}; the next step\'s uniforms reject {rejected} '
          f'(wanted more than {R.rejections_wanted(line.name, ok.size)}; collision {R.collision(line.name):.2f})')
    assert bool(ok.all()), f'{int((~ok).sum())} of {ok.size} draws outside the restated CDF interval, first (row, step): {np.argwhere(~ok)[0].tolist()}'
    # teeth
    assert rejected > R.rejections_wanted(line.name, ok.size)
    assert np.array_equal(tokens, run_draws(logits, R.STEPS, line.T, line.top_k, R.SEED))
    assert not np.array_equal(tokens, run_draws(logits, R.STEPS, line.T, line.top_k, R.SEED + 1))
    if line.name in SAME_AS_NONE:                    # top_k >= V keeps every token: the bits of top_k none
        assert np.array_equal(tokens, run_draws(logits, R.STEPS, line.T, None, R.SEED))


def test_sample_bookkeeping_at_the_kernel(hal):
    """state_ld > B, tokens_ld > n_slots: a row that draws its stop token goes dead and its length stops; a dead row emits the stop token;
    step >= n_slots writes no token; x_next = wte[clamp(token)] + wpe[min(pos, n_pos - 1)] bit for bit, also where pos + 1 == n_pos."""
    ops = hal['ops']
    B, V, C, n_pos, n_slots = 6, 40, 8, 16, 4
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B, V, generator=g)
    arg = logits.argmax(1)
    stop = int(arg[0])
    for r in range(1, B):                                                            # only row 0 draws the stop token
        if int(arg[r]) == stop:
            logits[r, stop] = -9.0
    arg = logits.argmax(1)
    wte, wpe = torch.randn(V, C, generator=g), torch.randn(n_pos, C, generator=g)
    state0 = torch.full((4, B + 3), -77, dtype=I32)
    state0[0, :B] = torch.tensor([3, 4, 5, 6, n_pos - 2, n_pos - 1])                 # pos
    state0[1, :B] = torch.tensor([0, 1, 2, 4, 3, 7])                                 # step: rows 3 and 5 are past the slots
    state0[2, :B] = 2                                                                # length
    state0[3, :B] = torch.tensor([1, 1, 0, 1, 1, 1])                                 # alive: row 2 is dead
    for stop_token in (stop, -1):
        state = state0.to(DEV)
        slots = torch.full((B, n_slots + 3), -7, dtype=torch.int64, device=DEV)
        nxt = torch.full((B,), -5, dtype=torch.int64, device=DEV)
        x_next = torch.full((B, C), float('nan'), device=DEV)
        cfg = ops.gpt_sample_cfg(1.0, 1, stop_token, 5, DEV)
        ops.gpt_sample(logits.to(DEV), cfg, state[:, :B], slots[:, 1:1 + n_slots], nxt, wte.to(DEV), wpe.to(DEV), x_next)
        torch.cuda.synchronize()
        tok = arg.clone()
        alive = state0[3, :B].clone()
        length = state0[2, :B].clone()
        for r in range(B):
            if alive[r]:
                if int(tok[r]) == stop_token:
                    alive[r] = 0
                else:
                    length[r] += 1
            if not alive[r]:
                tok[r] = stop_token
        want_state = state0.clone()
        want_state[0, :B] += 1
        want_state[1, :B] += 1
        want_state[2, :B] = length
        want_state[3, :B] = alive
        assert torch.equal(state.cpu(), want_state), (stop_token, state.cpu().tolist())
        if stop_token == stop:
            assert alive.tolist() == [0, 1, 0, 1, 1, 1] and length.tolist() == [2, 3, 2, 3, 3, 3]
        want_slots = torch.full((B, n_slots + 3), -7, dtype=torch.int64)
        for r in range(B):
            step = int(state0[1, r])
            if step < n_slots:
                want_slots[r, 1 + step] = tok[r]
        assert torch.equal(slots.cpu(), want_slots), (stop_token, slots.cpu().tolist())
        ids = tok.clamp(0, V - 1)
        assert torch.equal(nxt.cpu(), ids)
        want_x = wte[ids] + wpe[want_state[0, :B].long().clamp(max=n_pos - 1)]
        assert int(want_state[0, 5]) == n_pos and int(want_state[0, 4]) == n_pos - 1
        assert torch.equal(x_next.cpu(), want_x), stop_token
