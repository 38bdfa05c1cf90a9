"""The four rank-16 LoRA launches (csrc/lora.hip: halo_lora_pack, halo_lora_down, halo_lora_up, halo_lora_tn) against float64, per launch, at
their tile edges (tests/lora_rows_ref.py; DESIGN.md "LoRA launches against float64").

Every random case is held to max(8 x the fp32 stand-in's own deviation from the float64 reference, 2^-22) in units of the per-element scale
S, a bf16 output to that plus half a bf16 ulp of its own store; the small-integer cases and the packed images bit for bit; lora_tn twice for
equal bits; the columns between N and ldy untouched; the mask the host's Philox stream; one composed forward / backward pass launch by
launch; the refused shapes refused on the host.

Observed on an MI355X, worst error / allowed error per launch family (and, as information, the share of elements equal to the stand-in bit
for bit): halo_lora_down 0.998 (every element); halo_lora_up onto bf16 rows 1.000 (every element), onto fp32 rows 0.148 (95.8 % .. 99.0 %);
halo_lora_tn 0.176 (62 % .. 100 %); the composed pass down 0.996 / 0.997, up 1.000 (bf16 qkv) and 0.125 (fp32 d_h), tn 0.125 / 0.114.  On the
bf16 outputs the device is the stand-in, and the ratio sits at 1 because nearly all of the allowed error is the half ulp of the bf16 store
itself, which some element always uses up."""
import pytest
import torch

import lora_rows_ref as R
from test_gpu_gpt_rows_oracle import counted

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from haloop_amd import _lib, ops
    _lib.lib()
    return ops


@pytest.fixture(scope='module')
def ratios():
    """launch family -> [(case, error / allowed, share of elements equal to the stand-in)]; printed per family when the module is done."""
    seen = {}
    yield seen
    for family, rows in seen.items():
        worst = max(rows, key=lambda t: t[1])
        print(f'\n{family}: {len(rows)} cases, worst deviation / bound {worst[1]:.3f} ({worst[0]}), '
              f'elements equal to the stand-in bit for bit {min(t[2] for t in rows):.3f} .. {max(t[2] for t in rows):.3f}')


def _carve(t, pad):
    """(the buffer [M, W + pad] on the device, its [M, W] column slice holding t): the columns beyond W hold NaN."""
    if not pad:
        d = t.to(DEV).contiguous()
        return d, d
    buf = torch.full((t.shape[0], t.shape[1] + pad), float('nan'), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    view = buf[:, :t.shape[1]]
    assert view.stride(0) == t.shape[1] + pad and view.data_ptr() % 16 == 0
    return buf, view


def _drop(ops, c):
    """(ops.Dropout of the case -- part of the offset in a device counter where the case says so --, the counter tensor or None)."""
    d = c.drop
    if d.p <= 0:
        return ops.NO_DROPOUT, None
    counter = torch.tensor([d.counter], dtype=torch.int32, device=DEV) if d.counter else None
    return ops.Dropout(d.p, d.seed, d.offset, counter=counter), counter


def _run(ops, c):
    """The case through its launch -> the result on the host.  up: the columns beyond N inside ldy keep their bits; tn: two runs, equal bits."""
    inp = R.make_inputs(c.name)
    drop, counter = _drop(ops, c)
    sid = c.drop.stream_id
    if c.launch == 'down':
        _, x = _carve(inp['x'], c.pad)
        got = ops.lora_down(x, inp['P'].to(DEV), c.scale, drop, sid)
        assert got.shape == (c.M, R.RP) and got.dtype == torch.bfloat16
    elif c.launch == 'up':
        buf, y = _carve(inp['y0'], c.pad)
        before = buf.clone()
        assert ops.lora_up_(y, inp['u'].to(DEV), inp['P'].to(DEV), c.scale, drop, sid) is y
        assert R.same_bits(buf[:, c.W:], before[:, c.W:]), 'columns beyond N were written'
        assert not R.same_bits(buf[:, :c.W], before[:, :c.W])
        got = y
    else:
        _, x = _carve(inp['x'], c.pad)
        u = inp['u'].to(DEV)
        got = ops.lora_tn(u, x, c.r, c.scale, c.transpose, drop, sid)
        again = ops.lora_tn(u, x, c.r, c.scale, c.transpose, drop, sid)
        assert got.shape == ((c.W, c.r) if c.transpose else (c.r, c.W)) and got.dtype == torch.float32
        assert R.same_bits(got, again), 'two runs of lora_tn differ'
    if counter is not None:
        assert counter.item() == c.drop.counter
    return got.cpu().contiguous()


def _equal_share(got, want):
    return (got.double() == want.double()).double().mean().item()


RANDOM = {launch: R.of(launch, exact=False) for launch in ('down', 'up', 'tn')}


def _hold_case(ops, ratios, c):
    got = _run(ops, c)
    ref, S, bound = R.reference(c), R.scale(c), R.bound(c)
    e = R.excess(got, ref, S, bound, c.bf16_out)
    share = _equal_share(got, R.stand_in(c))
    print(f'\n{c.name}: deviation / bound {e:.3f} (bound {bound:.2e} S), equal to the stand-in {share:.3f}')
    rows = '' if c.launch != 'up' else ' (fp32 rows)' if c.f32 else ' (bf16 rows)'
    ratios.setdefault(f'halo_lora_{c.launch}{rows}', []).append((c.name, e, share))
    assert e <= 1.0, (c.name, c.why, e, 'first (row, col, device, reference):', R.first_outside(got, ref, S, bound, c.bf16_out))


@pytest.mark.parametrize('case', RANDOM['down'], ids=[c.name for c in RANDOM['down']])
def test_lora_down_matches_float64(ops, ratios, case):
    """Observed ratios: the module docstring and DESIGN.md."""
    _hold_case(ops, ratios, case)


@pytest.mark.parametrize('case', RANDOM['up'], ids=[c.name for c in RANDOM['up']])
def test_lora_up_matches_float64_and_leaves_the_columns_beyond_n(ops, ratios, case):
    _hold_case(ops, ratios, case)


@pytest.mark.parametrize('case', RANDOM['tn'], ids=[c.name for c in RANDOM['tn']])
def test_lora_tn_matches_float64_and_repeats_its_bits(ops, ratios, case):
    _hold_case(ops, ratios, case)


@pytest.mark.parametrize('case', R.EXACT_CASES, ids=[c.name for c in R.EXACT_CASES])
def test_exact_cases_bit_for_bit(ops, case):
    """Small integers, scale a power of two, p = 0.5: no rounding anywhere, so any wrong lane, block or mask bit changes a result."""
    got = _run(ops, case)
    want = R.reference(case).to(got.dtype)
    if not R.same_bits(got, want):
        i = tuple(torch.nonzero(got.double() != want.double())[0].tolist()) if not torch.equal(got, want) else None
        raise AssertionError((case.name, 'first difference (index, device, wanted):', i, None if i is None else (got[i].item(), want[i].item())))


@pytest.mark.parametrize('r,n_in,n_out', R.PACK_CASES)
def test_lora_pack_bit_for_bit(ops, r, n_in, n_out):
    A, B = R.pack_inputs(r, n_in, n_out)
    got = ops.lora_pack(A.to(DEV), B.to(DEV))
    for name, g, w in zip(('A16', 'At16', 'B16', 'Bt16'), got, R.pack_ref(A, B)):
        assert R.same_bits(g.cpu(), w), name


@pytest.mark.parametrize('name', ['down_48x160_ld+8_p0.25', 'up_80x288_bf16_p0.25_counter'])
def test_the_device_mask_is_the_host_mask(ops, name):
    """ops.dropout_fwd of ones at the case's (seed, stream_id, offset [+ counter]) is the host's multiplier matrix: the reference and the
    kernels speak of the same stream."""
    c = R.BY_NAME[name]
    drop, _ = _drop(ops, c)
    got = ops.dropout_fwd(torch.ones(c.M, c.W, device=DEV), drop, c.drop.stream_id).cpu()
    want = R.mult(c.M, c.W, c.drop)
    assert R.same_bits(got, want) and 0.15 < (want == 0).float().mean().item() < 0.35


def test_composed_forward_and_backward_launch_by_launch(ops, ratios, monkeypatch):
    """lora.lora_rows_forward / lora_rows_backward at M = 64, n_in = 64, n_out = 192, r = 5, alpha = 32, p = 0.1 with fp32 d_h: each launch
    against its float64 reference fed the device's own bf16 u / du of the launch before; with d_h=None no halo_lora_up call."""
    from haloop_amd import _linear, lora
    M, n_in, n_out, r = 64, 64, 192, 5
    g = torch.Generator().manual_seed(64)
    lin = lora.Linear(n_in, n_out, bias=False, r=r, lora_alpha=32, lora_dropout=0.1)
    with torch.no_grad():
        lin.lora_B.weight.copy_(torch.randn(n_out, r, generator=g) * 0.2)
    lin.to(DEV)
    s = lin.scaling
    assert s == 6.4
    rd = R.Drop(0.1, 4242, 4097, 6)
    site = (ops.Dropout(rd.p, rd.seed, rd.offset), rd.stream_id)
    h = torch.randn(M, n_in, generator=g).bfloat16()
    qkv0 = torch.randn(M, n_out, generator=g).bfloat16()
    dqkv = (torch.randn(M, n_out, generator=g) * n_out ** -0.5).bfloat16()
    dh0 = torch.randn(M, n_in, generator=g)
    images = _linear.WeightImages()

    downs = []
    real_down = ops.lora_down
    monkeypatch.setattr(ops, 'lora_down', lambda *a, **k: downs.append(real_down(*a, **k)) or downs[-1])

    def hold(what, got, ref, pre, S, bf16_out):
        bound = R.bound_of(pre, ref, S)
        e = R.excess(got, ref, S, bound, bf16_out)
        print(f'\ncomposed {what}: deviation / bound {e:.3f} (bound {bound:.2e} S)')
        ratios.setdefault('composed pass', []).append((what, e, _equal_share(got, pre.to(got.dtype))))
        assert e <= 1.0, (what, e, R.first_outside(got, ref, S, bound, bf16_out))

    # forward
    qkv = qkv0.to(DEV)
    hd = h.to(DEV)
    u = lora.lora_rows_forward(images, lin, hd, qkv, site)
    A16, At16, B16, Bt16 = R.pack_ref(lin.lora_A.weight.detach().cpu(), lin.lora_B.weight.detach().cpu())
    for name, got, want in zip(('A16', 'At16', 'B16', 'Bt16'), lora.packed(images, lin), (A16, At16, B16, Bt16)):
        assert R.same_bits(got.cpu(), want), name
    assert len(downs) == 1 and downs[0] is u
    uh = u.cpu()
    assert bool((uh[:, r:] == 0).all())
    hold('down (u)', uh, R.down64(h, A16, 1.0, rd), R.down32(h, A16, 1.0, rd)[0], R.down_scale(h, A16, 1.0, rd), True)
    hold('up (qkv)', qkv.cpu(), R.up64(uh, B16, qkv0, s), R.up32(uh, B16, qkv0, s)[0], R.up_scale(uh, B16, qkv0, s), True)

    # backward
    grads = {}
    put = lambda p, t: grads.__setitem__(id(p), t)
    d_h = dh0.to(DEV)
    dq = dqkv.to(DEV)
    with counted(('halo_lora_up', 'halo_lora_down', 'halo_lora_tn')) as calls:
        lora.lora_rows_backward(images, lin, hd, u, dq, d_h, put, site)
    assert calls == {'halo_lora_up': 1, 'halo_lora_down': 1, 'halo_lora_tn': 2} and len(downs) == 2
    du = downs[1].cpu()
    hold('down (du)', du, R.down64(dqkv, Bt16, s), R.down32(dqkv, Bt16, s)[0], R.down_scale(dqkv, Bt16, s), True)
    dB, dA = grads[id(lin.lora_B.weight)].cpu(), grads[id(lin.lora_A.weight)].cpu()
    assert dB.shape == (n_out, r) and dA.shape == (r, n_in)
    hold('tn (dB)', dB, R.tn64(uh, dqkv, r, s, True), R.tn32(uh, dqkv, r, s, True), R.tn_scale(uh, dqkv, r, s, True), False)
    hold('tn (dA)', dA, R.tn64(du, h, r, 1.0, False, rd), R.tn32(du, h, r, 1.0, False, rd), R.tn_scale(du, h, r, 1.0, False, rd), False)
    hold('up (d_h)', d_h.cpu(), R.up64(du, At16, dh0, 1.0, rd), R.up32(du, At16, dh0, 1.0, rd)[0], R.up_scale(du, At16, dh0, 1.0, rd), False)

    # nobody reads d_h: no up launch, the same gradients
    grads2 = {}
    with counted(('halo_lora_up', 'halo_lora_down', 'halo_lora_tn')) as calls:
        lora.lora_rows_backward(images, lin, hd, u, dq, None, lambda p, t: grads2.__setitem__(id(p), t), site)
    assert calls == {'halo_lora_up': 0, 'halo_lora_down': 1, 'halo_lora_tn': 2}
    assert R.same_bits(grads2[id(lin.lora_B.weight)].cpu(), dB) and R.same_bits(grads2[id(lin.lora_A.weight)].cpu(), dA)


def test_refused_shapes_are_refused_on_the_host(ops):
    """Host-side argument checks only: each raises the library's invalid-argument error before any launch."""
    from haloop_amd import _lib
    bf = lambda *s: torch.ones(*s, device=DEV, dtype=torch.bfloat16)
    refused = pytest.raises(_lib.HaloError, match='invalid argument')
    with refused:
        ops.lora_down(bf(8, 32), bf(16, 32))                                 # M % 16
    with refused:
        ops.lora_down(bf(16, 48), bf(16, 48))                                # K % 32
    with refused:
        ops.lora_tn(bf(32, 16), bf(32, 16), 17)                              # r > 16
    with refused:
        ops.lora_tn(bf(48, 16), bf(48, 16), 4)                               # M % 32
    u, p16, yb, yf = bf(16, 16), bf(32, 16), bf(16, 32), torch.ones(16, 32, device=DEV)
    with refused:                                                            # both y pointers set
        _lib.check(_lib.lib().halo_lora_up(_lib.ptr(u), _lib.ptr(p16), 16, 32, 1.0, _lib.ptr(yb), _lib.ptr(yf), 32, 0.0, 0, 0, 0, None,
                                           ops._stream()), 'halo_lora_up')
    with refused:                                                            # ... and neither
        _lib.check(_lib.lib().halo_lora_up(_lib.ptr(u), _lib.ptr(p16), 16, 32, 1.0, None, None, 32, 0.0, 0, 0, 0, None, ops._stream()),
                   'halo_lora_up')
    torch.cuda.synchronize()
    assert bool((yb == 1).all()) and bool((yf == 1).all())
