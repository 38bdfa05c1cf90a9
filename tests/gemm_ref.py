"""Yardstick of the GEMM core (haloop_amd.ops.gemm / gemm_split / gemm_split_io / gemm_split_ce; csrc/gemm_f32.hip, csrc/gemm_bf16x3.hip,
csrc/tiled_image.h): the product in a chosen precision under each math mode's OWN operand rounding, the epilogue in the kernels' order, and
the dispatch restated as a pure function.  Shared by tests/test_gemm_ref_cpu.py and tests/test_gpu_gemm_f64.py; holds no tests.  CPU only
(torch on the host + oracle/philox).

Product model, restated from the code (line numbers: haloop_amd/csrc/ at the commit that added this file).  rb = round-to-nearest-even to
bf16 (``(__bf16)x``, split8 tiled_image.h:17-24), hi = rb(x), lo = rb(x - hi):

  kind    product of a [M, K] and b [N, K]                  where
  ------  ------------------------------------------------  ------------------------------------------------------------------------
  exact   a b^T on fp32 operands                            halo_gemm_f32 in EVERY math mode (v_mfma_f32_32x32x2_f32, gemm_f32.hip:156)
  bf16    hi(a) hi(b)^T                                     the split entries in HALO_MATH_BF16 (PASSES == 1, gemm_bf16x3.hip:445)
  x3      lo(a) hi(b)^T + hi(a) lo(b)^T + hi(a) hi(b)^T     the split entries in HALO_MATH_BF16X3, in that order per 16-wide k-step
                                                            (gemm_bf16x3.hip:441-445); lo(a) lo(b) is dropped

halo_gemm_split_io with a row-major A takes the GIVEN (hi, lo) as A's two parts (stage_rowmajor, gemm_bf16x3.hip:228-238).

Epilogue, in the kernels' order (fused: gemm_bf16x3.hip:564-593, gemm_f32.hip:181-194; after split-K: halo_splitk_reduce_kernel and
halo_splitk_reduce4_kernel, gemm_f32.hip:202-247): v = sum + bias1 + bias2; activation (ReLU, tanh-GELU, erf-GELU: gemm_activation,
halo_common.h:167-172); v *= the dropout multiplier of element row * ldc + col (oracle.philox, stream ``STREAM_ID``; ldc = N in every
wrapper of haloop_amd/ops.py); v += the addend (``accumulate``: the output's previous contents, ``residual``: another matrix).

Two readings of a case:

``reference(...)``   float64 throughout (``product64`` + ``epilogue``); the mutants are switches on it.
``stand_in(...)``    the same operands, a float32 accumulator advanced in the device's order: for 'exact' one rounding per k (the f32 MFMA
                     is documented as a bit-for-bit k-ordered fmaf chain; fma(a, b, c) is emulated as float32(float64(a) float64(b) +
                     float64(c))), for 'bf16' / 'x3' one rounding per 16-wide k-step and per term (one v_mfma_f32_32x32x16_bf16 each).
                     K is cut into slices as the dispatch cuts it (``plan``), each slice accumulated from zero, the slices summed in slice
                     order in fp32 (the reduce kernels), the epilogue in fp32 with torch's formulas -- fused: sum + (bias1 + bias2);
                     reduce: (sum + bias1) + bias2.

Deviations are max_ij |got - ref| / S_ij with the per-element scale S = |a| |b|^T + |bias1| + |bias2| (+ |addend|), times 1 / (1 - p) under
dropout.  A device is held to ``bound`` = max(8 x the stand-in's own deviation on the same case, 2^-22): 8 is the margin lstm_ref.bounds
uses and covers the undocumented order in which a bf16 MFMA sums its 16 products; 2^-22 is two fp32 half-ulps of a value of size S (the
final rounding of the sum plus one bias add).  Nothing in a bound comes from a device.

``plan`` restates halo_pick_ksplit (gemm_f32.hip:267-292), launch_tile / launch_gemm (gemm_f32.hip:296-319), gemm_bf16x3_tiled_impl
(gemm_bf16x3.hip:856-933), half_tiles_wanted (gemm_bf16x3.hip:829-833), launch_io / gemm_bf16x3_io (gemm_bf16x3.hip:1009-1047) and
halo_splitk_reduce's choice (gemm_f32.hip:249-264) for the default environment: HALO_KSPLIT, HALO_GEMM_STAGES and HALO_GEMM_STAGES_BF16 are
read once per process and stay unset; HALO_GEMM_HALF_TILES is read on every call and is ``plan``'s ``half_tiles`` argument."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import philox

F32, F64 = torch.float32, torch.float64

RELU, GELU, ACCUM, ERF = 1, 2, 4, 8        # HALO_GEMM_* (include/halo.h, haloop_amd/_lib.py:17-20)
DROP = 16                                   # the yardstick's own bit: p_drop > 0
A_ROWMAJOR, OUT_BF16 = 32, 64               # ... and halo_gemm_split_io's two forms (IO & 1, IO & 2)

SCRATCH = 64 << 20                          # what _lib.lend_scratch() lends
SEED, OFFSET, STREAM_ID, P_DROP = 1234, 3, 5, 0.3
FLOOR = 2.0 ** -22
FACTOR = 8.0
KIND = {'f32': 'exact', 'bf16': 'bf16', 'bf16x3': 'x3'}


# ------------------------------------------------------------------------------------------------------------------------------
# cases and epilogue sets
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Epi:
    name: str
    bias1: bool = False
    bias2: bool = False
    relu: bool = False
    gelu: object = False               # False | 'tanh' | 'erf'
    addend: str = ''                   # '' | 'accumulate' | 'residual'
    p: float = 0.0

    @property
    def flags(self):
        return ((RELU if self.relu else 0) | (GELU if self.gelu == 'tanh' else 0) | (ERF if self.gelu == 'erf' else 0) |
                (ACCUM if self.addend else 0) | (DROP if self.p > 0 else 0))


EPILOGUES = [
    Epi('plain'),
    Epi('bias1', bias1=True),
    Epi('bias12_relu', bias1=True, bias2=True, relu=True),
    Epi('bias1_gelu', bias1=True, gelu='tanh'),
    Epi('bias1_erf', bias1=True, gelu='erf'),
    Epi('bias1_accumulate', bias1=True, addend='accumulate'),
    Epi('bias1_residual', bias1=True, addend='residual'),          # the split entry only (halo_gemm_split_residual)
    Epi('bias1_gelu_drop_accumulate', bias1=True, gelu='tanh', addend='accumulate', p=P_DROP),
]
EPI_BY_NAME = {e.name: e for e in EPILOGUES}


@dataclass(frozen=True)
class Case:
    entry: str                         # f32 | split | io (A row-major) | ioout (bf16 row-major output) | ce
    M: int
    N: int
    K: int
    modes: tuple
    half_tiles: bool = True            # False: run under HALO_GEMM_HALF_TILES=0
    why: str = ''

    @property
    def name(self):
        return f'{self.entry}_{self.M}x{self.N}x{self.K}' + ('' if self.half_tiles else '_whole_tiles')

    @property
    def epilogues(self):
        if self.entry == 'f32':
            return [e for e in EPILOGUES if e.addend != 'residual']
        return EPILOGUES if self.entry == 'split' else []


SPLIT_MODES = ('bf16x3', 'bf16')
CASES = [
    # ---- halo_gemm_f32 (each in all four (a_kcontig, b_kcontig) layouts on the device; one reference: the layouts share the k order) ----
    Case('f32', 65, 67, 33, ('f32', 'bf16x3', 'bf16'), why='odd leading dimensions: scalar loads; one k past a k-step'),
    Case('f32', 96, 64, 64, ('f32',), why='also read from views buf[:, 1:1+K] (a_vec = b_vec = 0) against the aligned run'),
    Case('f32', 70, 32, 1024, ('f32',), why='split-K, vector reduce'),
    Case('f32', 70, 33, 1000, ('f32',), why='split-K, scalar reduce, short last slice'),
    Case('f32', 1800, 1700, 40, ('f32',), why='128 x 128 tile, ragged both ways'),
    Case('f32', 1800, 1700, 2048, ('f32',), why='128 x 128 tile, two K-slices'),
    # ---- halo_gemm_split / halo_gemm_split_residual ----
    Case('split', 130, 70, 96, SPLIT_MODES, why='no split'),
    Case('split', 256, 128, 2048, SPLIT_MODES, why='16 even slices, vector reduce'),
    Case('split', 200, 130, 2100, SPLIT_MODES, why='ktper 5: 14 slices, the last of one ragged k-tile; scalar reduce'),
    Case('split', 1536, 1280, 2048, SPLIT_MODES, why='120 tiles: three uneven slices by the 448 / tiles rule'),
    Case('split', 4100, 3080, 40, SPLIT_MODES, why='825 tiles: the one-slot three-pass ring in bf16x3'),
    Case('split', 2100, 2000, 72, SPLIT_MODES, why='272 tiles: in bf16 the 64-row half tiles, last one of 52 rows (lean, lean-add)'),
    Case('split', 2100, 2000, 72, ('bf16',), half_tiles=False, why='the same on whole tiles'),
    # ---- halo_gemm_split_io ----
    Case('io', 300, 224, 96, SPLIT_MODES, why='A as a row-major (hi, lo) pair out of a wider buffer (lda = K + 8)'),
    Case('ioout', 300, 224, 96, SPLIT_MODES, why='A as an image, the result as row-major bf16 (hi, lo) beside the fp32'),
    # ---- halo_gemm_split_ce ----
    Case('ce', 200, 333, 64, SPLIT_MODES, why='ragged last strip'),
    Case('ce', 130, 1000, 96, SPLIT_MODES, why='16 strips'),
    Case('ce', 4100, 3080, 32, SPLIT_MODES, why='825 tiles: the one-slot ring in bf16x3'),
]
BY_NAME = {c.name: c for c in CASES}
IGNORE_INDEX = 0


def sample_rows(case):
    """None (every row), or for a case of more than a million outputs the fixed row sample: of every 128-row tile its first row, its last
    row, rows 63 and 64 and one seeded random row."""
    if case.M * case.N <= 1_000_000:
        return None
    g = torch.Generator().manual_seed(case.M + case.N)
    rows = []
    for r0 in range(0, case.M, 128):
        r1 = min(r0 + 128, case.M)
        rows += [r0, r1 - 1] + [r for r in (r0 + 63, r0 + 64) if r < r1] + [r0 + int(torch.randint(0, r1 - r0, (1,), generator=g))]
    return torch.tensor(sorted(set(rows)))


@functools.lru_cache(maxsize=3)
def make_inputs(name):
    """CPU float32 tensors of a case (deterministic): a [M, K], b [N, K] (randn / sqrt(K): outputs of order 1, like the biases and the
    addend), bias1, bias2 [N], addend [M, N]; 'io': a_hi, a_lo bf16 (lo an INDEPENDENT small matrix: the product must take the given
    parts, not re-derive them); 'ce': bias1 and targets."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(131 + sum(map(ord, f'{c.entry}{c.M}{c.N}{c.K}')))
    inp = {'a': torch.randn(c.M, c.K, generator=g), 'b': torch.randn(c.N, c.K, generator=g) / c.K ** 0.5,
           'bias1': torch.randn(c.N, generator=g), 'bias2': torch.randn(c.N, generator=g)}
    if c.entry in ('f32', 'split', 'io', 'ioout'):
        inp['addend'] = torch.randn(c.M, c.N, generator=g)
    if c.entry == 'io':
        inp['a_hi'] = inp['a'].bfloat16()
        inp['a_lo'] = (torch.randn(c.M, c.K, generator=g) * inp['a'].abs() * 2.0 ** -9).bfloat16()
    if c.entry == 'ce':
        tg = torch.randint(0, c.N, (c.M,), generator=g)
        last = ((c.N - 1) // 64) * 64                         # the last, ragged 64-column strip
        tg[1::5] = torch.randint(last, c.N, (len(tg[1::5]),), generator=g)
        tg[::7] = IGNORE_INDEX
        inp['targets'] = tg
    return inp


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    tile: tuple                        # (rows, columns) of a workgroup's output tile
    ntiles: int
    ksplit: int
    kper: int                          # k per slice (f32 entry: a multiple of 32; split entries: 32 * ktper)
    ktper: int                         # 32-wide k-tiles per slice
    reduce: str                        # '' | 'vector' | 'scalar'
    label: str                         # the instantiation


def pick_ksplit(tiles, k_steps, out_elems, scratch_bytes):
    """halo_pick_ksplit, gemm_f32.hip:267-292 (HALO_KSPLIT unset)."""
    if tiles >= 512 or k_steps < 8:
        return 1
    if tiles >= 128 and k_steps < 64:
        return 1
    if scratch_bytes <= 0:
        return 1
    if tiles >= 256:
        return 2 if k_steps >= 1024 and scratch_bytes >= 2 * 4 * out_elems else 1
    s = 256 // tiles
    if tiles >= 100 and k_steps >= 64 and 448 // tiles > s:
        s = 448 // tiles
    s = min(s, k_steps // 4, scratch_bytes // (4 * out_elems), 32)
    return 1 if s < 2 else s


def reduce_kind(M, N, ldc=None):
    """halo_splitk_reduce, gemm_f32.hip:249-264 (operands from torch's allocator: 16-byte aligned)."""
    ldc = N if ldc is None else ldc
    return 'vector' if N % 4 == 0 and ldc % 4 == 0 and M * N < 2 ** 31 else 'scalar'


def plan(entry, mode, M, N, K, flags=0, scratch_bytes=SCRATCH, half_tiles=True):
    cdiv = lambda x, y: (x + y - 1) // y
    if entry == 'f32':
        big = cdiv(M, 128) * cdiv(N, 128) >= 200 and M >= 128 and N >= 128               # launch_gemm
        t = 128 if big else 64
        ntiles = cdiv(M, t) * cdiv(N, t)
        k_steps = cdiv(K, 32)
        ks = pick_ksplit(ntiles, k_steps, M * N, scratch_bytes)
        kper = cdiv(k_steps, ks) * 32
        ks = cdiv(K, kper)
        red = reduce_kind(M, N) if ks > 1 else ''
        return Plan((t, t), ntiles, ks, kper, kper // 32, red, f'f32 {t}x{t}' + (f' + {red} reduce' if red else ''))
    one_pass = KIND[mode] == 'bf16'
    tiles_n = cdiv(N, 128)
    ntiles = cdiv(M, 128) * tiles_n
    KT = cdiv(K, 32)
    ks = 1 if entry in ('ce', 'io') else pick_ksplit(ntiles, KT, M * N, scratch_bytes)
    ktper = cdiv(KT, ks)
    ks = cdiv(KT, ktper)
    act, add, drop = flags & (RELU | GELU | ERF), flags & ACCUM, flags & DROP
    lean_any = ks == 1 and not drop and not act
    halves = half_tiles and ks == 1 and 256 < ntiles < 512 and M >= 128                  # half_tiles_wanted
    ring = 'bf16 three-slot' if one_pass else ('x3 one-slot' if ntiles * ks >= 768 else 'x3 two-slot')
    whole = (128, 128)
    if entry == 'ce':
        return Plan(whole, ntiles, 1, 32 * KT, KT, '', f'{ring} ce')
    if entry == 'io':
        rowmajor, out16 = bool(flags & A_ROWMAJOR), bool(flags & OUT_BF16)
        assert rowmajor != out16 and not drop and not (rowmajor and act) and not (out16 and add)       # gemm_bf16x3_io: anything else is ENOTSUP
        epi = 'full' if act else ('lean-add' if add else 'lean')
        io = 'A row-major' if rowmajor else 'bf16 out'
        if rowmajor and one_pass and halves:
            return Plan((64, 128), cdiv(M, 64) * tiles_n, 1, 32 * KT, KT, '', f'bf16 half-tile {epi} io {io}')
        return Plan(whole, ntiles, 1, 32 * KT, KT, '', f'{ring} {epi} io {io}')
    assert entry == 'split'
    if one_pass and lean_any and halves:
        return Plan((64, 128), cdiv(M, 64) * tiles_n, 1, 32 * KT, KT, '', 'bf16 half-tile ' + ('lean-add' if add else 'lean'))
    if lean_any:
        epi = 'lean-add' if add else 'lean'
    elif ks > 1 and ring != 'x3 one-slot':
        epi = 'slice'
    else:
        epi = 'full'
    red = reduce_kind(M, N) if ks > 1 else ''
    return Plan(whole, ntiles, ks, 32 * ktper, ktper, red, f'{ring} {epi}' + (f' + {red} reduce' if red else ''))


def case_plan(case, mode, epi=None, scratch_bytes=SCRATCH, io_flags=0):
    if case.entry in ('io', 'ioout') and not io_flags:
        io_flags = A_ROWMAJOR if case.entry == 'io' else OUT_BF16
    return plan('io' if case.entry == 'ioout' else case.entry, mode, case.M, case.N, case.K, (epi.flags if epi else 0) | io_flags, scratch_bytes, case.half_tiles)


# ------------------------------------------------------------------------------------------------------------------------------
# the product model
# ------------------------------------------------------------------------------------------------------------------------------
def rb(x, trunc=False):
    """x (any float dtype, holding fp32 values) rounded to bf16, back in x's dtype.  trunc: the low 16 bits cut off instead (a mutant)."""
    x32 = x.to(F32)
    if trunc:
        r = (x32.contiguous().view(torch.int32) & -65536).view(F32)
    else:
        r = x32.to(torch.bfloat16).to(F32)
    return r.to(x.dtype)


def split(x, trunc=False):
    hi = rb(x, trunc)
    return hi, rb(x - hi, trunc)


PRODUCT_MUTANTS = ('truncated', 'lohi_dropped', 'last_ktile_dropped', 'kchunks_swapped')
EPILOGUE_MUTANTS = ('bias_per_slice', 'dropout_after_addend', 'addend_dropped_on_splitk')
MUTANTS = {
    'truncated': 'operands truncated to bf16 instead of rounded to nearest even',
    'lohi_dropped': 'the lo(a) hi(b) term dropped',
    'last_ktile_dropped': 'the last 32-wide k-tile of the last K-slice dropped',
    'kchunks_swapped': 'columns c and c ^ 8 of one k-tile of A swapped (a swizzle slip)',
    'bias_per_slice': 'the biases added once per K-slice instead of once',
    'dropout_after_addend': 'the dropout multiplier applied after the addend instead of before',
    'addend_dropped_on_splitk': 'the addend dropped when the product is split over K',
}


def mutant_applies(mutant, case, mode, epi, pl):
    kind = KIND[mode] if case.entry != 'f32' else 'exact'
    return {'truncated': kind != 'exact' and case.K <= 96,      # beyond, rounding noise per element sinks under accumulation noise: the
                                                                 # bitwise image checks pin the rounding mode at every K
            'lohi_dropped': kind == 'x3',
            'last_ktile_dropped': True,
            'kchunks_swapped': kind != 'exact',
            'bias_per_slice': pl.ksplit > 1 and bool(epi and (epi.bias1 or epi.bias2)),
            'dropout_after_addend': bool(epi and epi.p > 0 and epi.addend),
            'addend_dropped_on_splitk': pl.ksplit > 1 and bool(epi and epi.addend)}[mutant]


def terms(case, mode, inp, rows=None, mutant=None):
    """The product's terms [(A [R, K], B [N, K]), ...] as float32 tensors, in the device's order inside a k-step."""
    kind = KIND[mode] if case.entry != 'f32' else 'exact'
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    a, b = sel(inp['a']), inp['b']
    trunc = mutant == 'truncated'
    if kind == 'exact':
        out = [(a, b)]
    else:
        ah, al = (sel(inp['a_hi']).float(), sel(inp['a_lo']).float()) if case.entry == 'io' else split(a, trunc)
        bh, bl = split(b, trunc)
        out = [(ah, bh)] if kind == 'bf16' else [(al, bh), (ah, bl), (ah, bh)]
        if mutant == 'lohi_dropped':
            out = out[1:]
    if mutant in ('last_ktile_dropped', 'kchunks_swapped'):
        K = case.K
        fixed = []
        for x, y in out:
            x = x.clone()
            if mutant == 'last_ktile_dropped':
                x[:, ((K - 1) // 32) * 32:] = 0
            else:
                kt = 32 if K >= 64 else 0                          # the second k-tile where it is a whole one, else the first
                idx = torch.arange(32 if K - kt >= 32 else 16) ^ 8 # (K >= 32 in every case of the split entries)
                w = len(idx)
                x[:, kt:kt + w] = x[:, kt + idx]
            fixed.append((x, y))
        out = fixed
    return out


def product64(case, mode, inp, rows=None, mutant=None):
    return sum(x.double() @ y.double().T for x, y in terms(case, mode, inp, rows, mutant))


def product32(case, mode, inp, pl, rows=None):
    """The stand-in's accumulator: float32, the device's order (module docstring); the slices summed in slice order."""
    tm = terms(case, mode, inp, rows)
    K = case.K
    total = None
    for s in range(pl.ksplit):
        k0, k1 = s * pl.kper, min(K, (s + 1) * pl.kper)
        acc = torch.zeros(tm[0][0].shape[0], case.N, dtype=F32)
        if len(tm) == 1 and case.entry == 'f32':
            a64, b64 = tm[0][0].double(), tm[0][1].double().T.contiguous()
            for k in range(k0, k1):
                acc = torch.addcmul(acc.double(), a64[:, k:k + 1], b64[k:k + 1]).float()
        else:
            t64 = [(x.double(), y.double().T.contiguous()) for x, y in tm]
            for k in range(k0, k1, 16):
                for x, y in t64:
                    acc = (acc.double() + x[:, k:min(k + 16, k1)] @ y[k:min(k + 16, k1)]).float()
        total = acc if total is None else total + acc
    return total


def dropout_at(elements, p, seed=SEED, stream_id=STREAM_ID, offset=OFFSET):
    """oracle.philox.dropout_mask at the given flat element indices only (an int64 tensor of any shape) -> float32 multipliers."""
    e = elements.reshape(-1).numpy().astype(np.uint64)
    q = e >> np.uint64(2)
    n = len(e)
    r = philox.philox4x32_10((q & np.uint64(0xFFFFFFFF)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                             np.full(n, stream_id, dtype=np.uint32), np.full(n, offset, dtype=np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    rr = np.choose((e & np.uint64(3)).astype(np.int64), r)
    m = np.where(rr >= philox.dropout_threshold(p), philox.dropout_scale(p), np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(m).reshape(elements.shape)


def _elements(case, rows):
    r = torch.arange(case.M) if rows is None else rows
    return r[:, None] * case.N + torch.arange(case.N)[None, :]


def _activation(v, epi):
    if epi.relu:
        v = v.clamp_min(0)
    if epi.gelu:
        v = torch.nn.functional.gelu(v, approximate='tanh' if epi.gelu == 'tanh' else 'none')
    return v


def epilogue(acc, case, epi, inp, pl, rows=None, mutant=None, offset=OFFSET):
    """The epilogue on an accumulator [R, N] in acc's dtype.  float64: the reference.  float32: the stand-in, in the order of the fused
    epilogue (sum + (bias1 + bias2)) or of the reduce kernels ((sum + bias1) + bias2)."""
    dt = acc.dtype
    b1 = inp['bias1'].to(dt) if epi.bias1 else None
    b2 = inp['bias2'].to(dt) if epi.bias2 else None
    v = acc
    if mutant == 'bias_per_slice':
        for b in (b1, b2):
            if b is not None:
                v = v + pl.ksplit * b
    elif pl.ksplit > 1:
        for b in (b1, b2):
            if b is not None:
                v = v + b
    elif b1 is not None or b2 is not None:
        v = v + (b1 if b2 is None else (b2 if b1 is None else b1 + b2))
    v = _activation(v, epi)
    m = dropout_at(_elements(case, rows), epi.p, offset=offset).to(dt) if epi.p > 0 else None
    if m is not None and mutant != 'dropout_after_addend':
        v = v * m
    if epi.addend and not (mutant == 'addend_dropped_on_splitk' and pl.ksplit > 1):
        add = inp['addend'] if rows is None else inp['addend'][rows]
        v = v + add.to(dt)
    if m is not None and mutant == 'dropout_after_addend':
        v = v * m
    return v


def scale(case, epi, inp, rows=None):
    """S [R, N] float64."""
    a = inp['a'] if rows is None else inp['a'][rows]
    s = a.double().abs() @ inp['b'].double().abs().T
    if epi is not None:
        if epi.bias1:
            s = s + inp['bias1'].double().abs()
        if epi.bias2:
            s = s + inp['bias2'].double().abs()
        if epi.addend:
            s = s + (inp['addend'] if rows is None else inp['addend'][rows]).double().abs()
        if epi.p > 0:
            s = s / (1.0 - epi.p)
    return s


def deviation(got, ref, S):
    return ((got.to(F64) - ref.to(F64)).abs() / S).max().item()


def first_outside(got, ref, S, bound, rows=None):
    """(row, col, device, reference) of the first element (row-major) outside the bound, or None."""
    idx = torch.nonzero((got.to(F64) - ref.to(F64)).abs() / S > bound)
    if not len(idx):
        return None
    i, j = idx[0].tolist()
    return (i if rows is None else int(rows[i])), j, got[i, j].item(), ref[i, j].item()


@functools.lru_cache(maxsize=None)
def core(name, mode, scratch_bytes=SCRATCH, mutant=None):
    """What a (case, mode, lent scratch) shares over its epilogue sets: the row sample, the float64 product, the stand-in's accumulator
    (none for a mutant), the plan of the plain epilogue (ksplit / kper do not depend on the epilogue set)."""
    case = BY_NAME[name]
    inp = make_inputs(name)
    rows = sample_rows(case)
    pl = case_plan(case, mode, None, scratch_bytes)
    return {'rows': rows, 'plan': pl, 'acc64': product64(case, mode, inp, rows, mutant if mutant in PRODUCT_MUTANTS else None),
            'acc32': product32(case, mode, inp, pl, rows) if mutant is None else None}


def reference(name, mode, epi, scratch_bytes=SCRATCH, mutant=None):
    """float64 [R, N] (R: the row sample).  Without a mutant the lent scratch does not enter it."""
    case, inp = BY_NAME[name], make_inputs(name)
    c = core(name, mode, scratch_bytes, mutant if mutant in PRODUCT_MUTANTS else None)
    return epilogue(c['acc64'], case, epi, inp, c['plan'], c['rows'], mutant)


def stand_in(name, mode, epi, scratch_bytes=SCRATCH):
    case, inp = BY_NAME[name], make_inputs(name)
    c = core(name, mode, scratch_bytes)
    return epilogue(c['acc32'], case, epi, inp, c['plan'], c['rows'])


@functools.lru_cache(maxsize=None)
def noise(name, mode, epi_name, scratch_bytes=SCRATCH):
    """The stand-in's own deviation from the float64 reference on the case."""
    epi = EPI_BY_NAME[epi_name]
    case, inp = BY_NAME[name], make_inputs(name)
    rows = core(name, mode, scratch_bytes)['rows']
    return deviation(stand_in(name, mode, epi, scratch_bytes), reference(name, mode, epi, scratch_bytes), scale(case, epi, inp, rows))


def bound(name, mode, epi_name, scratch_bytes=SCRATCH):
    return max(FACTOR * noise(name, mode, epi_name, scratch_bytes), FLOOR)


# ------------------------------------------------------------------------------------------------------------------------------
# the cross-entropy epilogue
# ------------------------------------------------------------------------------------------------------------------------------
CE_EPI = Epi('ce_bias', bias1=True)


def cross_entropy(logits, targets):
    """(loss, lse) per row in logits' dtype; 0 and 0 on the rows whose target is IGNORE_INDEX (ce_merge_kernel, gemm_bf16x3.hip:784-805)."""
    lse = torch.logsumexp(logits, 1)
    loss = lse - logits.gather(1, targets[:, None])[:, 0]
    keep = (targets != IGNORE_INDEX).to(logits.dtype)
    return loss * keep, lse * keep


@functools.lru_cache(maxsize=None)
def ce_reference(name, mode):
    """{'rows', 'logits' (float64), 'loss', 'lse', 'S' (of the logits), 'bound_logits', 'bound_rows'}: the float64 cross-entropy of the
    reference logits; bound_rows = max(8 x the stand-in's deviation, 2^-22), both in units of max(1, |lse|) per row (the stand-in: its fp32
    logits through torch's fp32 logsumexp)."""
    case, inp = BY_NAME[name], make_inputs(name)
    c = core(name, mode)
    rows = c['rows']
    tg = inp['targets'] if rows is None else inp['targets'][rows]
    ref = epilogue(c['acc64'], case, CE_EPI, inp, c['plan'], rows)
    sin = epilogue(c['acc32'], case, CE_EPI, inp, c['plan'], rows)
    S = scale(case, CE_EPI, inp, rows)
    loss, lse = cross_entropy(ref, tg)
    loss32, lse32 = cross_entropy(sin, tg)
    unit = lse.abs().clamp_min(1.0)
    dev = max(((loss32.double() - loss).abs() / unit).max().item(), ((lse32.double() - lse).abs() / unit).max().item())
    return {'rows': rows, 'targets': tg, 'logits': ref, 'loss': loss, 'lse': lse, 'unit': unit, 'S': S,
            'bound_logits': max(FACTOR * deviation(sin, ref, S), FLOOR), 'bound_rows': max(FACTOR * dev, FLOOR)}
