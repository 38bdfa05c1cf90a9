"""halo_rope_rows (csrc/rope_rows.hip, ops.rope_rows_): the interleaved rotation of the q and k column blocks of packed q | k | v rows in one
launch, fp32 and bf16 rows, against a float64 rotation on the host that uses the device table's own cos / sin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (B, T, heads, head_dim): T divides no power of two, so a wrong row-to-position map shows; two head dimensions; more than one workgroup
SHAPES = [(3, 13, 2, 64), (2, 5, 3, 32)]
PAD = 16                                                      # columns beyond 3C in the wider buffer the rows are carved from


def _rows(B, T, H, hd, dtype, seed):
    """(the wider buffer [M, 3C + PAD] on the device, its [M, 3C] column slice): the row stride differs from the width."""
    C = H * hd
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B * T, 3 * C + PAD, generator=g).to(dtype).to(DEV)
    return buf, buf[:, :3 * C]


def _rotate64(x, table, T, H, hd, t0, inverse=False):
    """float64 rotation of the q and k blocks of x [M, 3C] (float64, host) with the table's fp32 cos / sin; v as it is.
    -> (rotated, |x0| + |x1| per element of the q and k blocks)."""
    M, C = x.shape[0], H * hd
    pos = t0 + torch.arange(M) % T
    cos = table.cos.cpu().double()[pos].repeat_interleave(2, -1)[:, None, :]          # [M, 1, hd]
    sin = table.sin.cpu().double()[pos].repeat_interleave(2, -1)[:, None, :] * (-1.0 if inverse else 1.0)
    qk = x[:, :2 * C].reshape(M, 2 * H, hd)
    x0, x1 = qk[..., 0::2], qk[..., 1::2]
    swapped = torch.stack([-x1, x0], dim=-1).flatten(-2, -1)
    out = x.clone()
    out[:, :2 * C] = (qk * cos + swapped * sin).reshape(M, 2 * C)
    mag = (x0.abs() + x1.abs()).repeat_interleave(2, -1).reshape(M, 2 * C)
    return out, mag


@pytest.mark.parametrize('t0', [0, 7])
@pytest.mark.parametrize('shape', SHAPES)
def test_fp32_rows_against_float64(shape, t0):
    from haloop_amd import ops
    B, T, H, hd = shape
    C = H * hd
    buf, rows = _rows(B, T, H, hd, torch.float32, 1)
    before = buf.clone()
    table = ops.RopeTable(t0 + T, hd, DEV)
    ref, mag = _rotate64(before[:, :3 * C].cpu().double(), table, T, H, hd, t0)
    ops.rope_rows_(rows, T, H, hd, table, t0=t0)
    got = buf[:, :2 * C].cpu().double()
    # three fp32 roundings of terms bounded by the inputs
    bound = 2.0 ** -22 * mag
    err = (got - ref[:, :2 * C]).abs()
    print(f'fp32 {shape} t0={t0}: max err / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
    assert float((got - before[:, :2 * C].cpu().double()).abs().max()) > 0.1            # (it did rotate)
    # v and the bytes beyond 3C: bit-identical
    assert torch.equal(buf[:, 2 * C:].view(torch.int32), before[:, 2 * C:].view(torch.int32))
    # forward then inverse restores the input within twice the bound
    ops.rope_rows_(rows, T, H, hd, table, t0=t0, inverse=True)
    back = (buf[:, :2 * C].cpu().double() - before[:, :2 * C].cpu().double()).abs()
    print(f'     forward + inverse: max err / bound {float((back / bound).max()):.3f}')
    assert bool((back <= 2 * bound).all())
    assert torch.equal(buf[:, 2 * C:].view(torch.int32), before[:, 2 * C:].view(torch.int32))


def _ordered(bits):
    """bf16 bit patterns (int16) -> integers ordered like the values: neighbours differ by one."""
    b = bits.to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, 0x8000 - b, b)


@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('t0', [0, 7])
@pytest.mark.parametrize('shape', SHAPES)
def test_bf16_rows_round_the_float64_rotation(shape, t0, inverse):
    from haloop_amd import ops
    B, T, H, hd = shape
    C = H * hd
    buf, rows = _rows(B, T, H, hd, torch.bfloat16, 2)
    before = buf.clone()
    table = ops.RopeTable(t0 + T, hd, DEV)
    ref, _ = _rotate64(before[:, :3 * C].cpu().double(), table, T, H, hd, t0, inverse)
    want = ref[:, :2 * C].to(torch.bfloat16)                  # one rounding of the float64 result
    ops.rope_rows_(rows, T, H, hd, table, t0=t0, inverse=inverse)
    got = buf[:, :2 * C].cpu()
    d = (_ordered(got.view(torch.int16)) - _ordered(want.view(torch.int16))).abs()
    print(f'bf16 {shape} t0={t0} inverse={inverse}: {int((d > 0).sum())} of {d.numel()} differ, max {int(d.max())} ulp')
    assert int(d.max()) <= 1
    assert int((d > 0).sum()) <= d.numel() // 100
    assert torch.equal(buf[:, 2 * C:].view(torch.int16), before[:, 2 * C:].view(torch.int16))


def test_argument_errors_launch_nothing():
    from haloop_amd import _lib, ops
    B, T, H, hd = 2, 5, 2, 32
    C = H * hd
    table = ops.RopeTable(T, hd, DEV)
    # a row stride that is no multiple of 16 bytes
    buf = torch.randn(B * T, 3 * C + 2, device=DEV)
    keep = buf.clone()
    with pytest.raises(_lib.HaloError, match='invalid argument'):
        ops.rope_rows_(buf[:, :3 * C], T, H, hd, table)
    bufb = torch.randn(B * T, 3 * C + 4, device=DEV).bfloat16()
    with pytest.raises(_lib.HaloError, match='invalid argument'):
        ops.rope_rows_(bufb[:, :3 * C], T, H, hd, table)
    # rows that start off a 16-byte boundary
    with pytest.raises(_lib.HaloError, match='invalid argument'):
        ops.rope_rows_(torch.randn(B * T, 3 * C + 4, device=DEV)[:, 1:3 * C + 1], T, H, hd, table)
    # head_dim % 8 != 0
    x12 = torch.randn(B * T, 3 * 24, device=DEV)
    with pytest.raises(_lib.HaloError, match='invalid argument'):
        ops.rope_rows_(x12, T, 2, 12, ops.RopeTable(T, 12, DEV))
    # a table that does not cover t0 + T
    x = torch.randn(B * T, 3 * C, device=DEV)
    keepx = x.clone()
    with pytest.raises(_lib.HaloError, match='invalid argument'):
        ops.rope_rows_(x, T, H, hd, table, t0=1)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and torch.equal(x, keepx)
