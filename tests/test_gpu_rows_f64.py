"""The small row-wise and elementwise launches (csrc/gpt.hip: embedding, LayerNorm forward / backward, cross-entropy, GELU;
csrc/elementwise.hip: log_softmax_fwd / bwd, colsum; csrc/conv.hip: im2col_cl, col2im_cl, dwconv1d_cl and its backward) against float64, per
launch, at their dispatch edges (tests/rows_ref.py; DESIGN.md "Row kernels against float64").

Every element of every random case is held to max(4 x the fp32 stand-in's own deviation from the float64 reference, 2^-22) in units of
the per-element scale S; the small-integer cases, the pure copies and embed_bwd_ordered bit for bit; the backward launches with partial
sums twice for equal bits; the bf16 rows of the LayerNorm backward equal to its fp32 rows rounded; the columns between V and ld untouched.
Inputs sit at the head of NaN-filled allocations, the outputs a test allocates are carved out of NaN: a stray read shows, and stays
inside the test's own memory.  No target outside [0, V) is ever handed to a cross-entropy launch (the kernels read row[target] unchecked).

Observed on an MI355X: DESIGN.md 5g."""
import pytest
import torch

import rows_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
CASES = R.ALL_CASES


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops
    _lib.lib()
    return _lib, ops


@pytest.fixture(scope='module')
def ratios():
    """launch -> [(case, worst error / allowed error, share of elements equal to the stand-in)]; printed per launch when the module is done."""
    seen = {}
    yield seen
    for launch, rows in seen.items():
        worst = max(rows, key=lambda t: t[1])
        print(f'\nROWS {launch}: {len(rows)} cases, worst error / allowed {worst[1]:.3f} ({worst[0]}), '
              f'elements equal to the stand-in bit for bit {min(t[2] for t in rows):.3f} .. {max(t[2] for t in rows):.3f}')


@pytest.fixture(autouse=True)
def _nothing_more_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                                # a fault is sticky: every later launch of the process would fail too
        pytest.exit(f'the device reported an error ({e}): no further test of this module is started', returncode=3)


def guard(t, offset=0):
    """t on the device at the head (``offset`` floats in) of a NaN-filled allocation with 128 more NaNs behind it."""
    if t is None:
        return None
    if not t.dtype.is_floating_point:
        return t.to(DEV)
    n = t.numel()
    buf = torch.full((offset + n + 128,), NAN, dtype=t.dtype, device=DEV)
    buf[offset:offset + n] = t.reshape(-1).to(DEV)
    v = buf[offset:offset + n].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * offset) % 16
    return v


def host(d):
    return {k: v.float().cpu().contiguous() if v.dtype != torch.float32 else v.cpu().contiguous() for k, v in d.items() if v is not None}


def twice(fn):
    """fn() -> dict of device tensors; run twice, equal bits."""
    a, b = host(fn()), host(fn())
    for k in a:
        assert R.same_bits(a[k], b[k]), (k, 'two runs differ')
    return a


# ------------------------------------------------------------------------------------------------------------------------------
# one runner per launch family: the case through the library -> {output: host tensor}
# ------------------------------------------------------------------------------------------------------------------------------
def run_ln_fwd(hal, c, i):
    _, ops = hal
    return host({'y': ops.layernorm_fwd(guard(i['x']), guard(i['w']), guard(i['b']), R.EPS)})


def run_ln_bwd(hal, c, i):
    _, ops = hal
    dy, x, w, dres = guard(i['dy']), guard(i['x'], 1 if c.offset else 0), guard(i['w']), guard(i['dres'])

    def go():
        out = ops.layernorm_bwd(dy, x, w, dres, has_bias=c.has_bias, eps=R.EPS, want_bf16=c.bf16)
        if c.bf16:
            assert R.same_bits(out[3], out[0].bfloat16()), 'the bf16 rows are not the fp32 rows rounded'
        assert (out[2] is None) == (not c.has_bias)
        return {'dx': out[0], 'dw': out[1], 'db': out[2]}
    return twice(go)


def run_ce(hal, c, i):
    _lib, ops = hal
    rows, V, ld = c.rows, c.V, c.ld
    off = 1 if c.offset else 0

    def logits():
        wide = torch.full((rows, ld), NAN)
        wide[:, :V] = i['x']
        return guard(wide, off)
    tgt = i['tgt'].to(DEV)
    if ld == V:
        x = logits()
        loss = ops.cross_entropy_fwd(x, tgt, c.ignore)
        loss2, lse = ops.cross_entropy_fwd_lse(x, tgt, c.ignore)
        d = ops.cross_entropy_bwd_(logits(), tgt, guard(i['lse']), guard(i['grad']), c.ignore)
    else:                                                                    # ld > V: through the library handle
        lib, st = _lib.lib(), ops._stream()
        x, d = logits(), logits()
        loss, loss2, lse = (torch.full((rows,), NAN, device=DEV) for _ in range(3))
        _lib.check(lib.halo_cross_entropy_fwd(_lib.ptr(x), _lib.ptr(tgt), _lib.ptr(loss), rows, V, ld, c.ignore, st), 'halo_cross_entropy_fwd')
        _lib.check(lib.halo_cross_entropy_fwd_lse(_lib.ptr(x), _lib.ptr(tgt), _lib.ptr(loss2), _lib.ptr(lse), rows, V, ld, c.ignore, st),
                   'halo_cross_entropy_fwd_lse')
        gl, gg = guard(i['lse']), guard(i['grad'])
        _lib.check(lib.halo_cross_entropy_bwd(_lib.ptr(d), _lib.ptr(tgt), _lib.ptr(gl), _lib.ptr(gg), 0 if c.grad1 else 1, rows, V, ld, c.ignore, st),
                   'halo_cross_entropy_bwd')
        assert bool(torch.isnan(d[:, V:]).all()), 'columns between V and ld were written'
    assert R.same_bits(loss.cpu(), loss2.cpu()), 'cross_entropy_fwd and _fwd_lse give different losses'
    return host({'loss': loss, 'lse': lse, 'dlogits': d[:, :V]})


def run_lsm_fwd(hal, c, i):
    _, ops = hal
    return host({'y': ops.log_softmax_fwd(guard(i['x']))})


def run_lsm_bwd(hal, c, i):
    """The backward is handed the device's own y (returned too: the reference is fed the same)."""
    _, ops = hal
    y = ops.log_softmax_fwd(guard(R.make_inputs(c.name.replace('lsm_bwd', 'lsm_fwd'))['x']))
    ynan = guard(y.cpu())
    return host({'dx': ops.log_softmax_bwd(guard(i['dy']), ynan), '_y': y})


def run_colsum(hal, c, i):
    _, ops = hal
    out = torch.full((c.cols + 8,), NAN, device=DEV)
    ops.colsum(guard(i['x']), out=out[:c.cols])
    assert bool(torch.isnan(out[c.cols:]).all())
    return host({'out': out[:c.cols]})


def run_gelu_fwd(hal, c, i):
    _, ops = hal
    return host({'y': ops.gelu_fwd(guard(i['a']), exact=c.kind == 'erf')})


def run_gelu_bwd(hal, c, i):
    _, ops = hal
    out = torch.full((c.n + 8,), NAN, device=DEV)
    ops.gelu_bwd(guard(i['dy']), guard(i['a']), exact=c.kind == 'erf', out=out[:c.n])
    assert bool(torch.isnan(out[c.n:]).all())
    return host({'da': out[:c.n]})


def run_embed_fwd(hal, c, i):
    _, ops = hal
    return host({'x': ops.embed_fwd(i['ids'].to(DEV), guard(i['wte']), guard(i['wpe']), c.pos0)})


def run_add_rows(hal, c, i):
    _, ops = hal
    x = guard(i['x'])
    assert ops.add_rows_bcast_(x, guard(i['p']), c.T) is x
    return host({'x': x})


def run_embed_bwd(hal, c, i):
    _, ops = hal
    dwte, dwpe = guard(i['dwte0']), guard(i['dwpe0'])
    ops.embed_bwd(i['ids'].to(DEV), guard(i['dx']), dwte, dwpe, c.pos0, c.acc)
    return host({'dwte': dwte, 'dwpe': dwpe})


def run_embed_ord(hal, c, i):
    _, ops = hal
    return twice(lambda: {'dwte': ops.embed_bwd_ordered(i['ids'].to(DEV), guard(i['dx']), R.VOCAB)})


def run_im2col(hal, c, i):
    _, ops = hal
    col, To = ops.im2col_cl(guard(i['x']), c.ks, c.stride, c.pad)
    assert To == R.conv_out(c.T, c.ks, c.stride, c.pad)
    got = host({'col': col})
    assert R.same_bits(got['col'], R.im2col_unfold(c, i['x'])), 'im2col_cl differs from F.unfold'
    return got


def run_col2im(hal, c, i):
    _, ops = hal
    return host({'dx': ops.col2im_cl(guard(i['dcol']), c.N, c.T, c.C, c.ks, c.stride, c.pad)})


def run_dw_fwd(hal, c, i):
    _, ops = hal
    return host({'y': ops.dwconv1d_cl(guard(i['x']), guard(i['w']), guard(i['b']), c.stride, c.pad)})


def run_dw_bwd(hal, c, i):
    _, ops = hal
    dy, x, w = guard(i['dy']), guard(i['x']), guard(i['w'])

    def go():
        dx, dw, db = ops.dwconv1d_cl_bwd(dy, x, w, c.stride, c.pad, want_dx=c.want_dx, has_bias=c.has_bias)
        assert (dx is None) == (not c.want_dx) and (db is None) == (not c.has_bias)
        return {'dx': dx, 'dw': dw, 'db': db}
    return twice(go)


RUNNERS = {'ln_fwd': run_ln_fwd, 'ln_bwd': run_ln_bwd, 'ce': run_ce, 'lsm_fwd': run_lsm_fwd, 'lsm_bwd': run_lsm_bwd, 'colsum': run_colsum,
           'gelu_fwd': run_gelu_fwd, 'gelu_bwd': run_gelu_bwd, 'embed_fwd': run_embed_fwd, 'add_rows': run_add_rows, 'embed_bwd': run_embed_bwd,
           'embed_ord': run_embed_ord, 'im2col': run_im2col, 'col2im': run_col2im, 'dw_fwd': run_dw_fwd, 'dw_bwd': run_dw_bwd}


def _first_difference(got, want):
    idx = torch.nonzero((got.double() != want.double()) & ~(torch.isnan(got) & torch.isnan(want)))
    if not len(idx):
        return 'the sign of a zero'
    k = tuple(idx[0].tolist())
    return k, got[k].item(), want[k].item()


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_launch_matches_float64(hal, ratios, case):
    """Observed ratios: DESIGN.md 5g."""
    c = case
    got = RUNNERS[c.launch](hal, c, R.make_inputs(c.name))
    over = {'y': got.pop('_y')} if '_y' in got else {}
    ref, st = R.reference(c, **over), R.stand_in(c, **over)
    assert got.keys() == ref.keys()
    if c.mode in ('exact', 'standin'):
        for k in ref:
            want = ref[k].float() if c.mode == 'exact' else st[k]
            assert got[k].shape == want.shape
            assert R.same_bits(got[k], want), (c.name, k, 'first difference (index, device, wanted):', _first_difference(got[k], want))
        print(f'\nROWS {c.name}: bit for bit')
        return
    S = R.scale(c, **over)
    bounds = R.bounds_of(st, ref, S) if over else R.bounds(c)
    worst, share = 0.0, 1.0
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32
        e = R.excess(got[k], ref[k], S[k], bounds[k][1])
        eq = (got[k].double() == st[k].double()).double().mean().item() if ref[k].numel() else 1.0
        print(f'\nROWS {c.name} {k}: worst error / allowed {e:.3f} (bound {bounds[k][1]:.2e} S, the stand-in {bounds[k][0]:.2e} S), '
              f'equal to the stand-in {eq:.3f}')
        worst, share = max(worst, e), min(share, eq)
    ratios.setdefault(c.launch, []).append((c.name, worst, share))
    for k in ref:
        e = R.excess(got[k], ref[k], S[k], bounds[k][1])
        assert e <= 1.0, (c.name, c.reach, k, e, 'first (index, device, reference):', R.first_outside(got[k], ref[k], S[k], bounds[k][1]))


def test_refused_arguments_are_refused_on_the_host(hal):
    """Host-side argument checks only: each raises the library's invalid-argument error before any launch.  The buffers of the direct
    calls are large enough for the launch the C arithmetic would size (T + 2 pad - ks = -1 at stride 2 truncates to one window)."""
    _lib, ops = hal
    refused = pytest.raises(_lib.HaloError, match='invalid argument')
    ones = lambda *s: torch.ones(*s, device=DEV)
    with refused:                                                            # ks = 9: the kernel keeps 8 taps in registers
        ops.dwconv1d_cl_bwd(ones(2, 12, 4), ones(2, 20, 4), ones(4, 9), 1, 0)
    with refused:                                                            # the bf16 LayerNorm backward beyond the fused kernel's 2048 columns
        ops.layernorm_bwd(ones(2, 2052), ones(2, 2052), ones(2052), want_bf16=True)
    lib, st, p = _lib.lib(), ops._stream(), _lib.ptr
    x, big, w, ws = ones(1, 2, 4), torch.full((64,), NAN, device=DEV), ones(4, 3), torch.full((4096,), NAN, device=DEV)
    for stride in (1, 2):                                                    # T = 2, pad = 0, ks = 3: T + 2 pad < ks
        with refused:
            _lib.check(lib.halo_im2col_cl(p(x), p(big), 1, 2, 4, 3, stride, 0, st), 'halo_im2col_cl')
        with refused:
            _lib.check(lib.halo_col2im_cl(p(big), p(big[32:]), 1, 2, 4, 3, stride, 0, st), 'halo_col2im_cl')
        with refused:
            _lib.check(lib.halo_dwconv1d_cl(p(x), p(w), None, p(big), 1, 2, 4, 3, stride, 0, st), 'halo_dwconv1d_cl')
        with refused:
            _lib.check(lib.halo_dwconv1d_cl_bwd(p(ones(1, 1, 4)), p(x), p(w), p(big), p(big[16:]), p(big[32:]), p(ws), 1, 2, 4, 3, stride, 0, st),
                       'halo_dwconv1d_cl_bwd')
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all()) and bool(torch.isnan(ws).all())
