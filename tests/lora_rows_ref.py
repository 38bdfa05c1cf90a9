"""Yardstick of the four rank-16 LoRA launches (haloop_amd.ops.lora_pack / lora_down / lora_up_ / lora_tn; csrc/lora.hip, include/halo.h:269-293):
each launch restated in float64 on the exact bf16 operand values, an fp32 stand-in advanced in the kernel's own order, the per-element scale,
the bound a device is held to, the case lists at the kernels' tile edges, exact small-integer cases and the mutants.  Shared by
tests/test_lora_rows_ref_cpu.py and tests/test_gpu_lora_rows_f64.py; holds no tests.  CPU only (torch on the host + oracle/philox).

The launches, restated from the code (line numbers: haloop_amd/csrc/lora.hip at the commit that added this file).  keep = the 0 / 1 part of
oracle.philox.dropout_mask over the [M, width] rows, element row * width + col -- the row width, never the leading dimension
(include/halo.h:279-281); mult = keep / (1 - p):

  pack  (lora.hip:30-52)    A [r, n_in], B [n_out, r] fp32 -> A16 [16, n_in] | At16 [n_in, 16] | B16 [n_out, 16] | Bt16 [16, n_out]: each element
                            rounded to nearest even to bf16 (``(__bf16)v``, :51), rank rows / columns r..15 zero.
  down  (lora.hip:56-83)    U [M, 16] = scale / (1 - p) * (keep * X [M, K]) P [16, K]^T as bf16.  One workgroup per 16 rows; wave w takes the
                            32-deep k-blocks k0 = 32 w, 32 w + 128, ... (:63), one v_mfma_f32_16x16x32_bf16 each (:75); the mask zeroes bf16
                            operands, eight columns per lane as two Philox groups (:67-73); the four partial tiles meet in LDS as
                            ((w0 + w1) + (w2 + w3)) * scale, rounded to bf16 (:81-82); scale arrives as fp32 scale * fp32 1 / (1 - p) (:231).
  up    (lora.hip:88-130)   Y [M, N] += scale * mult * (U [M, 16] P [N, 16]^T) on bf16 or fp32 rows.  One wave per 16 rows (the waves of the
                            last workgroup beyond M return, :93) and 256 columns (:96), 32 columns per step as two MFMAs from a zero
                            accumulator (:100-105: one rounding of the 16-deep product), a lane ending with 8 consecutive columns;
                            upd = acc * scale (:109), * mult (:111-114), y + upd in fp32 (:120), bf16 rows as bf16(float(y) + upd) (:126).
  tn    (lora.hip:138-202)  G = scale / (1 - p) * U[:, :r]^T (keep * X [M, K]): fp32 [r, K], or [K, r] with transpose_out.  One workgroup per
                            (64 columns, slab of 256 rows); wave w takes the 32-row steps m0 = slab + 32 w, + 128 (:150), one MFMA per step
                            and 16-column tile (:176), nt = min(4, (K - c0) / 16) tiles (:145); the mask: lane q of a quad draws rows q and
                            q + 4 of the quad's four columns and the quad exchanges the keep bits (:162-174); the waves meet as
                            (w0 + w1) + (w2 + w3), rows < r only (:186-189); the reduce kernel adds the slabs in slab order from zero and
                            multiplies by fp32 scale * fp32 1 / (1 - p) (:193-202, :266).

Two readings of a case:

``reference(case)``  float64 throughout; the mutants are switches on it.
``stand_in(case)``   the same operands, fp32 accumulators advanced in the order above: one rounding per wave and MFMA (emulated as
                     float32(float64(acc) + the float64 product of the block)), the waves and slabs added in fp32 in the kernels' order, the
                     scales applied in fp32, bf16 outputs rounded once from the fp32 value.

Deviations are max |got - ref| / S with the per-element scale S: down |scale| / (1 - p) (keep |X|) |P|^T; up |Y0| + |scale| mult |U| |P|^T;
tn |scale| / (1 - p) |U[:, :r]|^T (keep |X|).  A device is held to ``bound`` = max(FACTOR x the stand-in's own deviation on the same case
(taken on its fp32 value, before any bf16 rounding), FLOOR), both constants gemm_ref's: 8 covers the undocumented order in which a bf16 MFMA
adds its products, 2^-22 is two fp32 half-ulps of a value of size S.  A bf16 output (down, up onto bf16 rows) may add its own rounding:
|got - ref| <= bound S + halfulp_bf16(|ref| + bound S), halfulp_bf16(v) = 2^(floor(log2 v) - 8).  Nothing in a bound comes from a device.

The exact cases (operands in {-2..2}, scale a power of two, p = 0.5) make every partial sum and every result exactly representable:
reference == stand_in bit for bit, and a device must match bit for bit -- they pin the lane maps and the mask without a tolerance."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from gemm_ref import FACTOR, FLOOR
from oracle import philox

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
RP = 16                                      # the padded rank (lora.hip:18)
SLAB = 256                                   # TN_SLAB_ROWS (lora.hip:19)
SPAN = 256                                   # UP_SPAN (lora.hip:20)
P_DROP = 0.25


# ------------------------------------------------------------------------------------------------------------------------------
# the dropout stream
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Drop:
    p: float = 0.0
    seed: int = 0
    stream_id: int = 0
    offset: int = 0
    counter: int = 0                   # > 0: that much of the offset comes from a device counter (ops.Dropout(counter=...))

    @property
    def at(self):
        return self.offset + self.counter


NO_DROP = Drop()


def keep_scale(drop):
    """1 / (1 - p) as the reference takes it (float64 of the fp32 p)."""
    return 1.0 / (1.0 - float(np.float32(drop.p))) if drop.p > 0 else 1.0


def scale32(scale, drop=NO_DROP):
    """fp32 scale * fp32 1 / (1 - p): what halo_lora_down / halo_lora_tn hand to their kernels (lora.hip:231, :266; d.scale: halo_common.h:64)."""
    s = np.float32(scale)
    return float(s * philox.dropout_scale(drop.p)) if drop.p > 0 else float(s)


def mult(M, W, drop, ld=None):
    """float32 [M, W]: the multipliers 0 | 1 / (1 - p) of the [M, W] rows, element row * W + col.  ld: indexed row * ld + col instead (what
    the mask_ld* mutants do)."""
    if drop.p <= 0:
        return torch.ones(M, W)
    ld = W if ld is None else ld
    m = philox.dropout_mask(M * ld, drop.p, drop.seed, drop.stream_id, drop.at)
    return torch.from_numpy(m).view(M, ld)[:, :W].contiguous()


def keep(M, W, drop, ld=None):
    """float64 [M, W] of 0 / 1."""
    return (mult(M, W, drop, ld) != 0).double()


# ------------------------------------------------------------------------------------------------------------------------------
# mutants
# ------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    'down': {
        'kblock_dropped': 'the fifth 32-deep k-block (wave 0\'s second) dropped',
        'mask_ldx': 'the mask indexed row * ldx + col',
        'mask_groups_swapped': 'the two 4-wide mask groups of an 8-column piece exchanged',
        'keep_scale_missing': '1 / (1 - p) missing',
        'tile_transposed': 'the 16 x 16 output tile transposed',
    },
    'up': {
        'halves_swapped': 'the two 4-column halves of an 8-column group exchanged',
        'rank_hi_ignored': 'rank entries 8..15 ignored',
        'mask_ldy': 'the mask indexed row * ldy + col',
        'last_span_skipped': 'the partial last span of 256 columns not updated',
        'row_tiles_ge4_skipped': 'row tiles >= 4 (the second workgroup\'s) not updated',
    },
    'tn': {
        'slab_omitted': 'the last slab omitted',
        'rows_128_255_omitted': 'rows 128..255 of every slab omitted (each wave\'s second step)',
        'mask_rows_jj4_swapped': 'mask rows jj and jj + 4 exchanged',
        'mask_quad_transposed': 'the mask\'s row / column roles within a 4 x 4 quad block transposed',
        'rank_row_off_by_one': 'rank row i takes U column i + 1',
        'transpose_ignored': 'transpose_out ignored: [r, K] written into the [K, r] result',
    },
}


def mutant_applies(mutant, c):
    """Whether the fault can show on case c at all (a mutant that applies must then be caught: tests/test_lora_rows_ref_cpu.py)."""
    masked = c.drop.p > 0
    return {'kblock_dropped': c.W >= 160, 'mask_ldx': masked and c.pad > 0, 'mask_groups_swapped': masked, 'keep_scale_missing': masked,
            'tile_transposed': True,
            'halves_swapped': True, 'rank_hi_ignored': True, 'mask_ldy': masked and c.pad > 0, 'last_span_skipped': c.W % SPAN != 0,
            'row_tiles_ge4_skipped': c.M > 64,
            'slab_omitted': c.M > SLAB, 'rows_128_255_omitted': c.M % SLAB > 128 or c.M >= SLAB, 'mask_rows_jj4_swapped': masked,
            'mask_quad_transposed': masked, 'rank_row_off_by_one': True, 'transpose_ignored': c.transpose and c.r > 1}[mutant]


# ------------------------------------------------------------------------------------------------------------------------------
# the launches on plain tensors: float64 reference (with mutants), fp32 stand-in, scale
# ------------------------------------------------------------------------------------------------------------------------------
def pack_ref(A, B):
    """(A16, At16, B16, Bt16) bf16 of A [r, n_in], B [n_out, r] fp32."""
    r, n_in = A.shape
    n_out = B.shape[0]
    A16 = torch.zeros(RP, n_in, dtype=BF16)
    A16[:r] = A.bfloat16()
    B16 = torch.zeros(n_out, RP, dtype=BF16)
    B16[:, :r] = B.bfloat16()
    return A16, A16.t().contiguous(), B16, B16.t().contiguous()


def down64(x, P, scale, drop=NO_DROP, mutant=None, ld=None):
    """float64 [M, 16].  x [M, K], P [16, K] bf16."""
    M, K = x.shape
    k = keep(M, K, drop, ld if mutant == 'mask_ldx' else None)
    if mutant == 'mask_groups_swapped':
        k = k[:, torch.arange(K) ^ 4]
    xs = x.double() * k
    if mutant == 'kblock_dropped':
        xs[:, 128:160] = 0
    s = float(np.float32(scale)) * (1.0 if mutant == 'keep_scale_missing' else keep_scale(drop))
    out = s * (xs @ P.double().T)
    if mutant == 'tile_transposed':
        out = out.view(M // 16, 16, RP).transpose(1, 2).reshape(M, RP)
    return out


def down32(x, P, scale, drop=NO_DROP):
    """The stand-in: (the fp32 value before the store, the bf16 result)."""
    M, K = x.shape
    xs, P64 = x.double() * keep(M, K, drop), P.double()
    w = []
    for wave in range(4):
        acc = torch.zeros(M, RP, dtype=F32)
        for k0 in range(32 * wave, K, 128):
            acc = (acc.double() + xs[:, k0:k0 + 32] @ P64[:, k0:k0 + 32].T).float()
        w.append(acc)
    pre = ((w[0] + w[1]) + (w[2] + w[3])) * scale32(scale, drop)
    return pre, pre.bfloat16()


def down_scale(x, P, scale, drop=NO_DROP):
    M, K = x.shape
    return abs(float(np.float32(scale))) * keep_scale(drop) * ((x.double().abs() * keep(M, K, drop)) @ P.double().abs().T)


def up64(u, P, y0, scale, drop=NO_DROP, mutant=None, ld=None):
    """float64 [M, N].  u [M, 16], P [N, 16] bf16, y0 [M, N] bf16 or fp32."""
    M, N = y0.shape
    m = mult(M, N, drop, ld if mutant == 'mask_ldy' else None).double()
    uu = u.double()
    if mutant == 'rank_hi_ignored':
        uu[:, 8:] = 0
    prod = uu @ P.double().T
    if mutant == 'halves_swapped':
        prod = prod[:, torch.arange(N) ^ 4]
    upd = float(np.float32(scale)) * m * prod
    if mutant == 'last_span_skipped' and N % SPAN:
        upd[:, (N // SPAN) * SPAN:] = 0
    if mutant == 'row_tiles_ge4_skipped':
        upd[64:] = 0
    return y0.double() + upd


def up32(u, P, y0, scale, drop=NO_DROP):
    """The stand-in: (the fp32 value before the store, the result in y0's dtype)."""
    M, N = y0.shape
    acc = (u.double() @ P.double().T).float()
    upd = acc * float(np.float32(scale))
    if drop.p > 0:
        upd = upd * mult(M, N, drop)
    pre = y0.float() + upd
    return pre, pre.to(y0.dtype)


def up_scale(u, P, y0, scale, drop=NO_DROP):
    M, N = y0.shape
    return y0.double().abs() + abs(float(np.float32(scale))) * mult(M, N, drop).double() * (u.double().abs() @ P.double().abs().T)


def tn64(u, x, r, scale, transpose=False, drop=NO_DROP, mutant=None):
    """float64 [r, K], or [K, r] with transpose.  u [M, 16], x [M, K] bf16."""
    M, K = x.shape
    k = keep(M, K, drop)
    if mutant == 'mask_rows_jj4_swapped':
        k = k[torch.arange(M) ^ 4]
    if mutant == 'mask_quad_transposed':
        k = k.view(M // 4, 4, K // 4, 4).transpose(1, 3).reshape(M, K)
    xs = x.double() * k
    if mutant == 'slab_omitted' and M > SLAB:
        xs[((M - 1) // SLAB) * SLAB:] = 0
    if mutant == 'rows_128_255_omitted':
        for s0 in range(0, M, SLAB):
            xs[s0 + 128:s0 + SLAB] = 0
    full = u.double().T @ xs
    if mutant == 'rank_row_off_by_one':
        full = torch.cat([full[1:], torch.zeros(1, K, dtype=F64)])
    g = float(np.float32(scale)) * keep_scale(drop) * full[:r]
    if transpose:
        g = g.contiguous().view(K, r) if mutant == 'transpose_ignored' else g.T.contiguous()
    return g


def tn32(u, x, r, scale, transpose=False, drop=NO_DROP):
    """The stand-in: fp32 [r, K] or [K, r]."""
    M, K = x.shape
    xs, ut = x.double() * keep(M, K, drop), u.double().T.contiguous()
    total = torch.zeros(RP, K, dtype=F32)
    for s0 in range(0, M, SLAB):
        m_end = min(s0 + SLAB, M)
        w = []
        for wave in range(4):
            acc = torch.zeros(RP, K, dtype=F32)
            for m0 in range(s0 + 32 * wave, m_end, 128):
                acc = (acc.double() + ut[:, m0:m0 + 32] @ xs[m0:m0 + 32]).float()
            w.append(acc)
        total = total + ((w[0] + w[1]) + (w[2] + w[3]))
    g = (total * scale32(scale, drop))[:r]
    return g.T.contiguous() if transpose else g.contiguous()


def tn_scale(u, x, r, scale, transpose=False, drop=NO_DROP):
    M, K = x.shape
    s = abs(float(np.float32(scale))) * keep_scale(drop) * (u.double().abs().T[:r] @ (x.double().abs() * keep(M, K, drop)))
    return s.T.contiguous() if transpose else s


# ------------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------------
def halfulp_bf16(v):
    """2^(floor(log2 v) - 8) (0 at v = 0): half the spacing of bf16 at the magnitude v."""
    return torch.exp2(torch.floor(torch.log2(v.double())) - 8)


def deviation(got, ref, S):
    """max |got - ref| / S; an element with S = 0 must be met exactly."""
    err = (got.to(F64) - ref.to(F64)).abs()
    q = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return q.max().item()


def allowed(ref, S, bound, bf16_out):
    """The error a result may have per element: bound S, plus the bf16 store's own rounding."""
    a = bound * S
    return a + halfulp_bf16(ref.abs() + a) if bf16_out else a


def excess(got, ref, S, bound, bf16_out):
    """max |got - ref| / allowed (<= 1: inside); an element that allows nothing must be met exactly."""
    err = (got.to(F64) - ref.to(F64)).abs()
    a = allowed(ref, S, bound, bf16_out)
    q = torch.where(a > 0, err / a.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return q.max().item()


def first_outside(got, ref, S, bound, bf16_out):
    """(row, col, device, reference) of the first element (row-major) outside, or None."""
    idx = torch.nonzero((got.to(F64) - ref.to(F64)).abs() > allowed(ref, S, bound, bf16_out))
    if not len(idx):
        return None
    i, j = idx[0].tolist()
    return i, j, got[i, j].item(), ref[i, j].item()


def same_bits(a, b):
    """Equal bit patterns (not values: -0.0 differs from +0.0, a NaN equals itself)."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def bound_of(pre, ref, S):
    """max(FACTOR x the stand-in's deviation (its fp32 value ``pre``), FLOOR)."""
    return max(FACTOR * deviation(pre, ref, S), FLOOR)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    launch: str                        # down | up | tn
    M: int
    W: int                             # the row width: K (down, tn) or N (up)
    pad: int = 0                       # leading dimension - W: the rows are a column slice of a buffer that much wider
    drop: Drop = NO_DROP
    scale: float = 1.0
    f32: bool = False                  # up: onto fp32 rows
    r: int = RP                        # tn
    transpose: bool = False            # tn
    exact: bool = False                # small integers: bit for bit
    why: str = ''

    @property
    def name(self):
        s = f'{self.launch}_{self.M}x{self.W}'
        if self.launch == 'tn':
            s += f'_r{self.r}' + ('_t' if self.transpose else '')
        if self.launch == 'up':
            s += '_f32' if self.f32 else '_bf16'
        return s + (f'_ld+{self.pad}' if self.pad else '') + (f'_p{self.drop.p}' if self.drop.p > 0 else '') + \
            ('_counter' if self.drop.counter else '') + ('_exact' if self.exact else '')

    @property
    def bf16_out(self):
        return self.launch == 'down' or (self.launch == 'up' and not self.f32)


def _d(seed, stream_id=7, offset=3, counter=0, p=P_DROP):
    return Drop(p, seed, stream_id, offset, counter)


# The seeds of the masked tn cases are the first for which every 4 x 4 block of the mask holds a kept and a dropped element
# (tests/test_lora_rows_ref_cpu.py asserts it): every quad exchange of lora_tn_kernel then moves bits that matter.
CASES = [
    # ---- halo_lora_down ----
    Case('down', 16, 32, why='only wave 0 has a block: the other three add zeros'),
    Case('down', 16, 32, pad=8, drop=_d(11), scale=0.75, why='... masked, out of a wider buffer'),
    Case('down', 48, 32, drop=_d(12), why='three workgroups'),
    Case('down', 48, 96, drop=_d(13), scale=1.5, why='wave 3 idle'),
    Case('down', 16, 96, pad=8, why='wave 3 idle, ldx > K'),
    Case('down', 48, 128, scale=0.75, why='one block per wave'),
    Case('down', 16, 128, pad=8, drop=_d(14), why='one block per wave, masked, ldx > K'),
    Case('down', 16, 160, scale=1.5, why='wave 0 takes a second block'),
    Case('down', 48, 160, pad=8, drop=_d(15), scale=0.75, why='... masked, ldx > K'),
    Case('down', 48, 160, drop=_d(16, counter=5), why='... the offset partly from a device counter'),
    # ---- halo_lora_up ----
    Case('up', 16, 32, why='one wave, one step'),
    Case('up', 16, 32, pad=8, f32=True, drop=_d(21), scale=0.75, why='... fp32 rows, masked, ldy > N'),
    Case('up', 80, 32, pad=8, scale=1.5, why='five row tiles: the second workgroup\'s waves 1-3 return'),
    Case('up', 80, 256, drop=_d(22), scale=0.75, why='a whole span, masked'),
    Case('up', 80, 256, f32=True, scale=1.5, why='a whole span, fp32 rows'),
    Case('up', 16, 256, pad=8, f32=True, drop=_d(23), why='a whole span, ldy > N'),
    Case('up', 16, 288, pad=8, scale=0.75, why='a second span of 32 columns'),
    Case('up', 16, 288, f32=True, why='... fp32 rows'),
    Case('up', 80, 288, pad=8, drop=_d(24), scale=1.5, why='both edges, masked, ldy > N'),
    Case('up', 80, 288, pad=8, f32=True, drop=_d(25), scale=0.75, why='... fp32 rows'),
    Case('up', 80, 288, drop=_d(26, counter=5), why='... the offset partly from a device counter'),
    # ---- halo_lora_tn ----
    Case('tn', 32, 16, r=1, drop=_d(1), why='one wave steps once; nt = 1'),
    Case('tn', 32, 64, r=16, drop=_d(2), scale=0.75, why='a whole chunk of four tiles, masked'),
    Case('tn', 32, 80, pad=8, r=4, transpose=True, drop=_d(14), scale=1.5, why='a second chunk with nt = 1, masked, ldx > K'),
    Case('tn', 32, 144, pad=8, r=4, drop=_d(8), why='three chunks, the last of one tile: the mask index at a row width of 144'),
    Case('tn', 96, 48, r=7, transpose=True, drop=_d(31), scale=0.75, why='three waves step; nt = 3'),
    Case('tn', 256, 16, pad=8, r=16, drop=_d(4), scale=1.5, why='a whole slab: every wave steps twice, masked'),
    Case('tn', 288, 16, r=4, transpose=True, drop=_d(14), why='a second slab of 32 rows, masked'),
    Case('tn', 544, 16, pad=8, r=7, drop=_d(159, counter=5), scale=0.75, why='three slabs, masked; the offset partly from a device counter'),
    Case('tn', 96, 144, pad=8, r=4, scale=1.5, why='three waves, three chunks'),
    Case('tn', 256, 64, r=7, transpose=True, why='a whole slab, a whole chunk'),
    Case('tn', 288, 80, pad=8, r=16, transpose=True, scale=0.75, why='two slabs, two chunks'),
    Case('tn', 544, 144, r=1, scale=1.5, why='three slabs, three chunks, rank 1'),
    Case('tn', 544, 48, r=16, transpose=True, why='three slabs, nt = 3, every rank row'),
]

_X = Drop(0.5, 77, 9, 2)                   # 1 / (1 - p) = 2
EXACT_CASES = [
    Case('down', 48, 160, pad=8, scale=0.5, exact=True),
    Case('down', 48, 160, pad=8, scale=0.5, drop=_X, exact=True),
    Case('up', 80, 288, pad=8, scale=0.5, exact=True),
    Case('up', 80, 288, pad=8, scale=0.5, drop=_X, exact=True),
    Case('up', 80, 288, pad=8, f32=True, scale=0.5, exact=True),
    Case('up', 80, 288, pad=8, f32=True, scale=0.5, drop=_X, exact=True),
    Case('tn', 544, 144, pad=8, r=7, scale=0.25, exact=True),
    Case('tn', 544, 144, pad=8, r=7, transpose=True, scale=0.25, drop=_X, exact=True),
]
ALL_CASES = CASES + EXACT_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# (r, n_in, n_out)
PACK_CASES = [(1, 8, 24), (7, 64, 192), (16, 32, 96)]


def of(launch, exact=None):
    return [c for c in ALL_CASES if c.launch == launch and (exact is None or c.exact == exact)]


def _operand(shape, g, exact, spread=1.0):
    if exact:
        return torch.randint(-2, 3, shape, generator=g).float().bfloat16()
    t = (torch.randn(shape, generator=g) * spread).bfloat16()
    assert bool((t.float().abs() >= 2.0 ** -126).all())                      # no subnormals (and no zeros)
    return t


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """CPU tensors of a case (deterministic).  down: x [M, K], P [16, K]; up: u [M, 16], P [N, 16], y0 [M, N] (bf16 or fp32); tn: u [M, 16],
    x [M, K] -- bf16 from randn (P / sqrt(K), so that the results are of order 1; every rank entry non-zero, also those beyond r), or small
    integers for an exact case."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(977 + sum(map(ord, name)))
    if c.launch == 'down':
        return {'x': _operand((c.M, c.W), g, c.exact), 'P': _operand((RP, c.W), g, c.exact, c.W ** -0.5)}
    if c.launch == 'up':
        y0 = _operand((c.M, c.W), g, c.exact)
        return {'u': _operand((c.M, RP), g, c.exact), 'P': _operand((c.W, RP), g, c.exact, 0.25), 'y0': y0.float() if c.f32 else y0}
    return {'u': _operand((c.M, RP), g, c.exact, c.M ** -0.5), 'x': _operand((c.M, c.W), g, c.exact)}


def pack_inputs(r, n_in, n_out):
    """A [r, n_in], B [n_out, r] fp32: randn over a wide range of magnitudes; up front and at the end exact ties of the bf16 rounding (both
    parities, both signs), +-0 and the largest finite bf16."""
    g = torch.Generator().manual_seed(r * 1000 + n_in)
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 3.3895313892515355e38,
                            (1 + 2.0 ** -8) * 2.0 ** -90])
    out = []
    for shape in ((r, n_in), (n_out, r)):
        t = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-40, 41, shape, generator=g).float())
        flat = t.view(-1)
        flat[:8] = special
        if flat.numel() >= 16:
            flat[-8:] = -special
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the two readings of a case
# ------------------------------------------------------------------------------------------------------------------------------
def reference(case, mutant=None):
    """float64.  ``mutant``: one of MUTANTS[case.launch]."""
    i, c = make_inputs(case.name), case
    if c.launch == 'down':
        return down64(i['x'], i['P'], c.scale, c.drop, mutant, c.W + c.pad)
    if c.launch == 'up':
        return up64(i['u'], i['P'], i['y0'], c.scale, c.drop, mutant, c.W + c.pad)
    return tn64(i['u'], i['x'], c.r, c.scale, c.transpose, c.drop, mutant)


@functools.lru_cache(maxsize=None)
def _stand_in(name):
    i, c = make_inputs(name), BY_NAME[name]
    if c.launch == 'down':
        return down32(i['x'], i['P'], c.scale, c.drop)
    if c.launch == 'up':
        return up32(i['u'], i['P'], i['y0'], c.scale, c.drop)
    g = tn32(i['u'], i['x'], c.r, c.scale, c.transpose, c.drop)
    return g, g


def stand_in(case):
    """In the output's dtype (bf16 for down and up onto bf16 rows)."""
    return _stand_in(case.name)[1]


def stand_in_f32(case):
    """The stand-in's fp32 value before the store."""
    return _stand_in(case.name)[0]


def scale(case):
    i, c = make_inputs(case.name), case
    if c.launch == 'down':
        return down_scale(i['x'], i['P'], c.scale, c.drop)
    if c.launch == 'up':
        return up_scale(i['u'], i['P'], i['y0'], c.scale, c.drop)
    return tn_scale(i['u'], i['x'], c.r, c.scale, c.transpose, c.drop)


@functools.lru_cache(maxsize=None)
def noise(name):
    """The stand-in's own deviation from the float64 reference on the case."""
    c = BY_NAME[name]
    return deviation(stand_in_f32(c), reference(c), scale(c))


def bound(case):
    return max(FACTOR * noise(case.name), FLOOR)
