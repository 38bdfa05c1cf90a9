"""Yardstick of the three launches of a GPT sampling step (haloop_amd.ops.gpt_decode_linear / gpt_decode_attention / gpt_sample;
csrc/gpt_decode.hip, csrc/decode_linear.h): each operation in float64 under the math mode's OWN operand rounding, a float32 stand-in in the
device's order, the dispatch restated as pure functions, the case tables and the mutants.  Shared by tests/test_gpt_decode_ref_cpu.py and
tests/test_gpu_gpt_decode_f64.py; holds no tests.  CPU only (torch and numpy on the host + oracle/philox through restated_u).

Linear (dec_linear_kernel<NT, KSW_LN, PASSES, 2>).  rb / split and the product kinds are gemm_ref's: 'bf16' = hi(x) hi(W)^T, 'x3' =
lo(x) hi(W)^T + hi(x) lo(W)^T + hi(x) hi(W)^T in that order per 32-wide k-step (decode_linear.h:70-74), lo lo dropped.  LayerNorm: no bias,
biased variance, eps inside the square root, applied BEFORE the split (decode_linear.h:99-130).  Epilogue in the kernel's order
(decode_linear.h:184-190): the four waves' sums (w0 + w1) + (w2 + w3), tanh-GELU if flagged, + out if ACCUM.
  ``linear_reference``  float64 throughout: float64 LayerNorm, the mode's rounding of the normalised row, the float64 product.
  ``linear_stand_in``   float32 in the device's order: the LayerNorm statistics summed in fp32 the way the lanes sum them (a lane's 8 KSW_LN
                        values left to right, the variance as an fma chain, the four lanes of a row, the four waves as (0 + 1) + (2 + 3)),
                        one rounding per 32-wide k-step and per term, each wave's ksw = K / 128 k-steps from zero, the waves summed as above.
  Deviations are max |got - ref| / S, S = |xn| |W|^T (+ |out|) with xn the float64 normalised row.  A device is held to
  max(8 x the stand-in's own deviation on the case, 2^-22): gemm_ref's rule with gemm_ref's two justifications.  Because the stand-in does
  its LayerNorm in fp32, a bf16 rounding of a normalised element flipped by the fp32 statistics would enter the bound through the stand-in
  -- and only there: a device that flips another element than the stand-in sits 2^-8 / K of S (thirty bounds) out without a defect, and a
  stand-in that flips lifts the case's bound three hundredfold (measured before the inputs were fixed: 130 x 512 x 904 in bf16, 7.1e-5,
  the exact GELU in place of the tanh form then INSIDE the bound).  So the LayerNorm cases' x keep every normalised element further from
  a bf16 rounding boundary than fp32 statistics can move it (``away_from_ties``): no flip, on the stand-in or on a device.
  ``plan`` restates halo_gpt_decode_linear's dispatch (gpt_decode.hip:387-405) and the k-step walk (decode_linear.h:157-163).

Attention (gpt_attention_kernel<MAXK, NW>).  ``attention_reference``: float64 softmax(q K^T / 8) V over keys 0 .. p on the fp32 inputs,
p = clamp(pos, 0, Tc - 1), key and value p taken from the qkv row, not from the cache.  The stand-in: the same in fp32 (torch's
order).  S = sum_j p_j |v_j|; bound as above but per ROW (never wider than the case's).  ``attention_plan`` restates the choice of <MAXK, NW> (gpt_decode.hip:424-433, default
environment).

Draw (gpt_sample_kernel).  ``draw_reference``: the kept set and the CDF exactly as include/halo.h states them -- l_v = fl32(logits[v] *
fl32(1 / T)) formed in float32 and then carried in float64, the kept set by float >= against the min(top_k, V)-th largest (ties stay), u
from oracle/philox.py (test_gpu_generation.restated_u).  ``stand_in_draw``: the definition in fp32 -- chunk = 4 ceil(V / 1024), chunk sums
left to right, prefixes left to right, the smallest kept v whose mass exceeds u * total.  ``accepted`` is test_gpu_generation's with
delta = max(1e-5, 8 x the stand-in's worst |cdf32 - cdf64| / total on the line) (``draw_delta``).

Mutants are switches on the references (``*_MUTANTS``), each with a ``*_mutant_applies``.  Nothing in a bound comes from a device."""
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from gemm_ref import rb, split, deviation, first_outside, FLOOR, FACTOR      # noqa: F401  (re-exported for the two test files)

F32, F64 = torch.float32, torch.float64


def restated_u(rows, steps, seed):
    """test_gpu_generation.restated_u, unchanged (imported on use: a suite run collects that module itself first)."""
    from test_gpu_generation import restated_u as f
    return f(rows, steps, seed)


def accepted(tokens, u, keep, cdf, delta):
    """test_gpu_generation.accepted, unchanged."""
    from test_gpu_generation import accepted as f
    return f(tokens, u, keep, cdf, delta=delta)


MODES = ('bf16x3', 'bf16')
KIND = {'bf16': 'bf16', 'bf16x3': 'x3'}
EPS = 1e-5
SEED = 0x1234567887654321


# ------------------------------------------------------------------------------------------------------------------------------
# linear: cases, dispatch
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lin:
    rows: int
    K: int
    n_out: int
    ln: bool = False
    accum: bool = False
    gelu: bool = False
    why: str = ''

    @property
    def name(self):
        return f'{self.rows}x{self.K}x{self.n_out}' + ('_L' if self.ln else '') + ('_A' if self.accum else '') + ('_G' if self.gelu else '')


LINEAR_CASES = [
    Lin(5, 512, 40, ln=True, why='KSW_LN 4'),
    Lin(16, 768, 112, ln=True, gelu=True, why='KSW_LN 6'),
    Lin(33, 1024, 100, ln=True, why='KSW_LN 8'),
    Lin(7, 256, 48, accum=True, why='lone group of 2'),
    Lin(20, 768, 72, accum=True, why='4 + 2'),
    Lin(16, 1280, 64, why='4 + 4 + 2'),
    Lin(9, 2048, 32, gelu=True, why='8 + 8'),
    Lin(3, 3072, 48, accum=True, why='8 x 3'),
    Lin(130, 512, 904, ln=True, gelu=True, why='NT 2; 57 tiles (odd); 9 row groups; n_out % 16 = 8'),
    Lin(130, 768, 904, accum=True, why='NT 2; accumulate'),
    Lin(4, 1024, 8200, ln=True, why='NT 2 from the tile count alone; 513 tiles'),
    # two beyond the issue's table: without them NT 2 x KSW_LN 6 (the lm_head's own instantiation) is reached only at an even tile count
    # by the model-level tests, and no case has ACCUM and GELU together (the order of the two)
    Lin(130, 768, 904, ln=True, why='NT 2 with KSW_LN 6; odd tile count'),
    Lin(6, 256, 24, accum=True, gelu=True, why='ACCUM and GELU together; n_out % 16 = 8 on a lone tile pair'),
]
LINEAR_BY_NAME = {c.name: c for c in LINEAR_CASES}
assert len(LINEAR_BY_NAME) == len(LINEAR_CASES)
BITCHECK = (256, 256, 40)            # rows, K, n_out of the image bit check: x = I_256


@dataclass(frozen=True)
class LinPlan:
    NT: int
    ksw_ln: int                       # 0 | 4 | 6 | 8
    ksw: int                          # 32-wide k-steps per wave
    walk: tuple                       # the group sizes a wave walks
    n_tiles: int
    row_groups: int

    def label(self, mode):
        return f'NT{self.NT} LN{self.ksw_ln} P{3 if KIND[mode] == "x3" else 1}'


def linear_supported(K, ln):
    """halo_gpt_decode_linear_supported in the bf16 / bf16x3 modes."""
    return K in (512, 768, 1024) if ln else (K > 0 and K % 256 == 0)


def plan(rows, K, n_out, ln):
    assert linear_supported(K, ln)
    n_tiles, row_groups = (n_out + 15) // 16, (rows + 15) // 16
    NT = 2 if ((n_tiles + 1) // 2) * row_groups >= 256 else 1
    ksw = K // 128
    if ln:
        walk = (ksw,)
    elif ksw % 8 == 0:
        walk = (8,) * (ksw // 8)
    else:
        walk = (4,) * (ksw // 4) + ((2,) if ksw % 4 else ())
    assert sum(walk) == ksw
    return LinPlan(NT, ksw if ln else 0, ksw, walk, n_tiles, row_groups)


@functools.lru_cache(maxsize=4)
def linear_inputs(name):
    """CPU float32 tensors, as test_gpu_decode.test_decode_linear makes them: x ~ 1.5 N + 0.3, W ~ N / sqrt(K), lnw ~ U + 0.5, out0
    [rows, n_out + 8] ~ N.  The last row of a LayerNorm case is ~ 1.5 N / 16 + 0.3: at a variance of 2.25 the place of eps = 1e-5 moves the
    result by 1e-6 of S, the size of the bound itself; at 0.009 it moves it by some 1e-4 of S."""
    c = LINEAR_BY_NAME[name]
    g = torch.Generator().manual_seed(977 + sum(map(ord, name)))
    inp = {'x': torch.randn(c.rows, c.K, generator=g) * 1.5 + 0.3, 'w': torch.randn(c.n_out, c.K, generator=g) / c.K ** 0.5,
           'lnw': torch.rand(c.K, generator=g) + 0.5 if c.ln else None, 'out0': torch.randn(c.rows, c.n_out + 8, generator=g)}
    if c.ln:
        inp['x'][-1] = (inp['x'][-1] - 0.3) / 16 + 0.3
        inp['x'] = away_from_ties(inp['x'], inp['lnw'], g)
    return inp


TIE_MARGIN = 2.0 ** -17


def tie_distance(x, lnw):
    """(distance of every float64 normalised element from the nearest point where its rounding to bf16 changes, the margin fp32 statistics
    are granted: TIE_MARGIN (|x| + |mean|) rstd lnw -- 2^-22 (|x| + |mean|) covers the fp32 roundings of the mean, of x - mean, of rstd and
    of the two products; the margin is 32 times that)."""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = 1.0 / ((xd - mean).pow(2).mean(1, keepdim=True) + EPS).sqrt()
    xn = (xd - mean) * rstd * lnw.double()
    hi = rb(xn)
    ulp = torch.exp2(torch.frexp(hi)[1].double() - 8)                  # bf16: 8 significant bits
    dist = torch.stack([(xn - (hi + ulp / 2)).abs(), (xn - (hi - ulp / 2)).abs(), (xn - (hi - ulp / 4)).abs()]).min(0).values          # (ulp / 4: below a power of two)
    return dist, TIE_MARGIN * (xd.abs() + mean.abs()) * rstd * lnw.double()


def away_from_ties(x, lnw, g):
    """x with the few elements nudged (by up to 1e-3) whose normalised value sits within the margin of a bf16 rounding boundary: the fp32
    statistics of a stand-in or a device then cannot flip a rounding of the bf16 mode (a flip moves an output by 2^-8 / K of S, thirty times
    the bound, and is no defect), so the bound of a LayerNorm case is fp32 accumulation noise in both modes.  An element closer to its
    row's mean than 0.02 (where the margin is wider than the bf16 spacing itself) is first moved to 0.02 .. 0.04 from it."""
    x = x.clone()
    for _ in range(200):
        dist, margin = tie_distance(x, lnw)
        bad = dist < margin
        if not bool(bad.any()):
            return x
        mean = x.double().mean(1, keepdim=True).float().expand_as(x)
        near = bad & ((x - mean).abs() < 0.02)
        step = torch.rand(x.shape, generator=g)
        x = torch.where(near, mean + torch.where(x >= mean, 1.0, -1.0) * (0.02 + 0.02 * step), torch.where(bad, x + (step - 0.5) * 2e-3, x))
    raise AssertionError('away_from_ties did not settle')


# ------------------------------------------------------------------------------------------------------------------------------
# linear: the model
# ------------------------------------------------------------------------------------------------------------------------------
LINEAR_MUTANTS = {
    'truncated': 'operands truncated to bf16 instead of rounded to nearest even',
    'lohi_dropped': 'the lo(x) hi(W) term dropped',
    'last_kstep_dropped': 'the last 32-wide k-step of one wave (wave 1) dropped',
    'variance_unbiased': 'the variance over K - 1',
    'eps_outside_sqrt': '1 / (sqrt(var) + eps)',
    'erf_for_tanh': 'the exact GELU in place of the tanh form',
    'accumulate_before_activation': 'out added before the GELU',
}


def linear_mutant_applies(mutant, case, mode):
    return {'truncated': case.K <= 256,       # beyond, rounding noise per element sinks under accumulation noise; the bit check pins it
            'lohi_dropped': KIND[mode] == 'x3',
            'last_kstep_dropped': True,
            'variance_unbiased': case.ln,
            'eps_outside_sqrt': case.ln,
            'erf_for_tanh': case.gelu,
            'accumulate_before_activation': case.gelu and case.accum}[mutant]


def layer_norm64(x, lnw, eps=EPS, mutant=None):
    x = x.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / (x.shape[1] - (1 if mutant == 'variance_unbiased' else 0))
    rstd = 1.0 / (var.sqrt() + eps) if mutant == 'eps_outside_sqrt' else 1.0 / (var + eps).sqrt()
    return d * rstd * lnw.double()


def _lanes(x):
    """x [R, K] -> [R, 4 waves, 4 lanes of a row, 8 KSW_LN] in the order a lane walks its values (decode_linear.h:100-104): element k is
    held by wave k / (K / 4), k-step i of that wave, lane group g = (k % 32) / 8, slot j = k % 8; a lane walks i outer, j inner."""
    R, K = x.shape
    nk = K // 128
    return x.reshape(R, 4, nk, 4, 8).permute(0, 1, 3, 2, 4).reshape(R, 4, 4, nk * 8)


def _tree(s):
    """[R, 4 waves, 4 lanes] fp32 -> [R, 1]: the lanes (0 + 1) + (2 + 3) by two shuffles, the waves (0 + 1) + (2 + 3)."""
    s = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    return ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3]))[:, None]


def layer_norm32(x, lnw, eps=EPS):
    """The kernel's LayerNorm in fp32, in its order."""
    K = x.shape[1]
    v = _lanes(x)
    s = torch.zeros(v.shape[:3], dtype=F32)
    for i in range(v.shape[3]):
        s = s + v[..., i]
    mean = _tree(s) / torch.tensor(float(K), dtype=F32)
    d = _lanes(x - mean).double()
    s = torch.zeros(v.shape[:3], dtype=F32)
    for i in range(v.shape[3]):
        s = (d[..., i] * d[..., i] + s.double()).float()               # v += d * d contracts to an fma
    rstd = 1.0 / torch.sqrt(_tree(s) / torch.tensor(float(K), dtype=F32) + torch.tensor(eps, dtype=F32))
    return (x - mean) * rstd * lnw


def linear_terms(xn, w, mode, mutant=None):
    trunc = mutant == 'truncated'
    xh, xl = split(xn, trunc)
    wh, wl = split(w.to(xn.dtype), trunc)
    out = [(xh, wh)] if KIND[mode] == 'bf16' else [(xl, wh), (xh, wl), (xh, wh)]
    if mutant == 'lohi_dropped':
        out = out[1:]
    if mutant == 'last_kstep_dropped':
        ksw = xn.shape[1] // 128
        k0 = (2 * ksw - 1) * 32
        fixed = []
        for a, b in out:
            a = a.clone()
            a[:, k0:k0 + 32] = 0
            fixed.append((a, b))
        out = fixed
    return out


def _gelu(v, exact=False):
    return F.gelu(v, approximate='none' if exact else 'tanh')


def linear_epilogue(v, case, inp, mutant=None):
    add = inp['out0'][:, :case.n_out].to(v.dtype) if case.accum else None
    if add is not None and mutant == 'accumulate_before_activation':
        v = v + add
    if case.gelu:
        v = _gelu(v, exact=mutant == 'erf_for_tanh')
    if add is not None and mutant != 'accumulate_before_activation':
        v = v + add
    return v


def _linear_reference(case, inp, mode, mutant=None):
    xn = layer_norm64(inp['x'], inp['lnw'], EPS, mutant) if case.ln else inp['x'].double()
    acc = sum(a @ b.T for a, b in linear_terms(xn, inp['w'], mode, mutant))
    return linear_epilogue(acc, case, inp, mutant)


def _linear_stand_in(case, inp, mode):
    xn = layer_norm32(inp['x'], inp['lnw']) if case.ln else inp['x']
    t64 = [(a.double(), b.double().T.contiguous()) for a, b in linear_terms(xn, inp['w'], mode)]
    ksw = case.K // 128
    waves = []
    for wv in range(4):
        acc = torch.zeros(case.rows, case.n_out, dtype=F32)
        for ks in range(wv * ksw, (wv + 1) * ksw):
            for a, b in t64:
                acc = (acc.double() + a[:, ks * 32:ks * 32 + 32] @ b[ks * 32:ks * 32 + 32]).float()
        waves.append(acc)
    return linear_epilogue((waves[0] + waves[1]) + (waves[2] + waves[3]), case, inp)


def linear_scale(case, inp):
    xn = layer_norm64(inp['x'], inp['lnw']) if case.ln else inp['x'].double()
    s = xn.abs() @ inp['w'].double().abs().T
    return s + inp['out0'][:, :case.n_out].double().abs() if case.accum else s


@functools.lru_cache(maxsize=None)
def linear_reference(name, mode, mutant=None):
    return _linear_reference(LINEAR_BY_NAME[name], linear_inputs(name), mode, mutant)


@functools.lru_cache(maxsize=None)
def linear_stand_in(name, mode):
    return _linear_stand_in(LINEAR_BY_NAME[name], linear_inputs(name), mode)


@functools.lru_cache(maxsize=None)
def linear_noise(name, mode):
    return deviation(linear_stand_in(name, mode), linear_reference(name, mode), linear_scale(LINEAR_BY_NAME[name], linear_inputs(name)))


def linear_bound(name, mode):
    return max(FACTOR * linear_noise(name, mode), FLOOR)


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Attn:
    name: str
    B: int
    heads: int
    Tc: int
    pos: tuple                        # one position per row
    sharp_row: int = -1               # q and the keys scaled: scores of order +-60
    equal_row: int = -1               # every key of the row the same vector
    why: str = ''


ATTENTION_CASES = [
    Attn('4x2x1024', 4, 2, 1024, (0, 511, 512, 1023), why='sixteen waves; one pass exactly, one key into the second pass, the full cache'),
    # the issue's thirteen positions and four more: two keys, a whole number of 32-key passes short of a group, and the two special rows
    Attn('17x8x320', 17, 8, 320, (0, 7, 8, 31, 32, 127, 128, 129, 255, 256, 319, -3, 325, 1, 63, 200, 300), sharp_row=15, equal_row=16,
         why='four waves (136 pairs); the 8-key, 32-key and 128-key boundaries; the documented clamp'),
    Attn('1x2x8192', 1, 2, 8192, (8191,), why='<8192, 16> at the far end'),
    Attn('65x2x1025', 65, 2, 1025, tuple(1024 if b % 3 != 1 else 5 for b in range(65)), why='<8192, 4>; the smallest cache that selects it'),
]
ATTENTION_BY_NAME = {c.name: c for c in ATTENTION_CASES}
HD = 64


def attention_plan(B, heads, Tc):
    """(MAXK, NW) of the launched gpt_attention_kernel (HALO_GPT_ATTN_WAVES unset)."""
    return (1024 if Tc <= 1024 else 8192), (16 if B * heads <= 128 else 4)


def clamped(case):
    return torch.tensor(case.pos).clamp(0, case.Tc - 1)


@functools.lru_cache(maxsize=2)
def attention_inputs(name):
    """qkv [B, 3C]; ck, cv [B, heads, Tc, 64]: the caches' FULL random contents (the GPU test overwrites rows p and above with NaN before the
    launch; the stale_row_p mutant reads row p from here); pos int32 [B]."""
    c = ATTENTION_BY_NAME[name]
    g = torch.Generator().manual_seed(31 + c.B + c.Tc)
    C = c.heads * HD
    qkv = torch.randn(c.B, 3 * C, generator=g)
    ck = torch.randn(c.B, c.heads, c.Tc, HD, generator=g)
    cv = torch.randn(c.B, c.heads, c.Tc, HD, generator=g)
    if c.sharp_row >= 0:
        s = 20.0 ** 0.5                                   # q k / 8 then has standard deviation 20: scores of order +-60
        qkv[c.sharp_row, :2 * C] *= s
        ck[c.sharp_row] *= s
    if c.equal_row >= 0:
        ck[c.equal_row] = ck[c.equal_row, :, :1].clone()
        qkv[c.equal_row, C:2 * C] = ck[c.equal_row, :, 0].reshape(-1)
    return {'qkv': qkv, 'ck': ck, 'cv': cv, 'pos': torch.tensor(c.pos, dtype=torch.int32)}


ATTENTION_MUTANTS = {
    'keys_exclusive': 'attends 0 .. p - 1',
    'pass_tail_dropped': 'the keys after the last whole group of 4 * KPP dropped',
    'stale_row_p': 'key and value p read from the cache\'s old contents',
    'scale_dropped': 'no division by 8',
}


def attention_mutant_applies(mutant, case):
    if mutant == 'pass_tail_dropped':
        group = 32 * attention_plan(case.B, case.heads, case.Tc)[1]
        return bool(((clamped(case) + 1) % group != 0).any())
    return True


def attention(case, inp, dtype=F64, mutant=None):
    """(out [B, C], S [B, C]) in ``dtype``; a row that a mutant leaves without keys gives zeros."""
    B, H, Tc = case.B, case.heads, case.Tc
    C = H * HD
    p = clamped(case)
    qkv = inp['qkv'].to(dtype)
    q, kq, vq = (qkv[:, i * C:(i + 1) * C].reshape(B, H, HD) for i in range(3))
    K, V = inp['ck'].to(dtype), inp['cv'].to(dtype)
    if mutant != 'stale_row_p':
        K, V = K.clone() if K is inp['ck'] else K, V.clone() if V is inp['cv'] else V
        rows = torch.arange(B)
        K[rows, :, p] = kq
        V[rows, :, p] = vq
    j = torch.arange(Tc)[None, :]
    valid = j < p[:, None] if mutant == 'keys_exclusive' else j <= p[:, None]
    if mutant == 'pass_tail_dropped':
        group = 32 * attention_plan(B, H, Tc)[1]
        valid = valid & (j < ((p + 1) // group * group)[:, None])
    s = torch.einsum('bhd,bhjd->bhj', q, K)
    if mutant != 'scale_dropped':
        s = s * 0.125
    s = s.masked_fill(~valid[:, None, :], float('-inf'))
    P = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    return torch.einsum('bhj,bhjd->bhd', P, V).reshape(B, C), torch.einsum('bhj,bhjd->bhd', P, V.abs()).reshape(B, C)


@functools.lru_cache(maxsize=None)
def attention_reference(name, mutant=None):
    """(out, S) float64."""
    return attention(ATTENTION_BY_NAME[name], attention_inputs(name), F64, mutant)


def row_deviation(got, ref, S):
    """max_j |got - ref| / S per row."""
    return ((got.to(F64) - ref.to(F64)).abs() / S).max(1).values


@functools.lru_cache(maxsize=None)
def attention_noise(name):
    """The stand-in's own deviation, per row [B]."""
    ref, S = attention_reference(name)
    return row_deviation(attention(ATTENTION_BY_NAME[name], attention_inputs(name), F32)[0], ref, S)


def attention_bound(name):
    """Per ROW [B] (no wider than the per-case rule: every row's bound is at most the case's): the row with scores of order +-60 carries
    thirty times the fp32 noise of the others and would otherwise set the bound of all seventeen."""
    return (FACTOR * attention_noise(name)).clamp_min(FLOOR)


# ------------------------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Draw:
    name: str
    V: int
    top_k: object                     # None | int
    T: float
    ld: int = 0                       # > V: the logits are a view of a wider buffer
    kind: str = 'randn'               # randn | quarter (rounded to multiples of 0.25) | zeros (the +-0 row) | ninf (a quarter -inf)
    why: str = ''


ROWS, STEPS = 8, 64
DRAW_LINES = [
    Draw('v40_k20', 40, 20, 1.0, why='threads without elements; top_k above the count of non-idle threads'),
    Draw('v1000_none_t0.7', 1000, None, 0.7, why='V < 1024, vector path'),
    Draw('v1023_k256', 1023, 256, 1.0, why='scalar path; floor key at its limit'),
    Draw('v1028_k257', 1028, 257, 1.0, why='no floor key'),
    Draw('v4100_k2_t5', 4100, 2, 5.0),
    Draw('v4100_none', 4100, None, 1.0, why='what the last two of the next three must equal'),
    Draw('v4100_kVm1', 4100, 4099, 1.0),
    Draw('v4100_kV', 4100, 4100, 1.0),
    Draw('v4100_kVp5', 4100, 4105, 1.0),
    Draw('v50257_k40_t0.05', 50257, 40, 0.05, why='GPT-2\'s vocabulary; scalar path; sharp'),
    Draw('v2048_ld2050_k40', 2048, 40, 1.0, ld=2050, why='a view of a wider buffer; ld % 4 != 0'),
    Draw('v2048_k100_quarter', 2048, 100, 1.0, kind='quarter', why='many ties at the threshold; the kept set is larger than top_k'),
    Draw('v1000_k100_zeros', 1000, 100, 1.0, kind='zeros', why='30 entries > 0, 200 of +0.0 and 200 of -0.0 interleaved: the definition keeps 430'),
    Draw('v2048_k40_ninf', 2048, 40, 1.0, kind='ninf', why='a quarter of each row is -inf; those tokens are never drawn'),
]
DRAW_BY_NAME = {d.name: d for d in DRAW_LINES}


@functools.lru_cache(maxsize=None)
def draw_logits(name):
    """float32 numpy [ROWS, V]."""
    d = DRAW_BY_NAME[name]
    g = torch.Generator().manual_seed(d.V + 7)
    lg = torch.randn(ROWS, d.V, generator=g) * 2.0
    if d.kind == 'quarter':
        lg = (lg * 2).round() / 4                          # N(0, 1) rounded to multiples of 0.25: some fifty ties at the 100th largest
    elif d.kind == 'ninf':
        for r in range(ROWS):
            lg[r, torch.randperm(d.V, generator=g)[:d.V // 4]] = float('-inf')
    elif d.kind == 'zeros':
        lg = -lg.abs() - 0.01
        for r in range(ROWS):
            idx = torch.randperm(d.V, generator=g)[:430]
            lg[r, idx[:30]] = torch.rand(30, generator=g) * 1.5 + 0.5
            z = idx[30:].sort().values
            lg[r, z[0::2]] = 0.0
            lg[r, z[1::2]] = -0.0
    out = lg.numpy().copy()
    if d.kind == 'zeros':
        assert (np.signbit(out) & (out == 0)).sum() == 200 * ROWS and (~np.signbit(out) & (out == 0)).sum() == 200 * ROWS
    return out


DRAW_MUTANTS = {
    'uniform_of_next_step': 'the uniforms of step + 1',
    'threshold_strict': '> in place of >= against the k-th largest',
    'signed_zero_split': '-0.0 ordered below +0.0',
}


def _kth(logits, line):
    return np.sort(logits, axis=1)[:, -min(line.top_k, line.V)][:, None]


def draw_mutant_applies(mutant, line):
    """threshold_strict needs ties at the threshold to move more than one token's mass; signed_zero_split a threshold of +-0."""
    if mutant == 'uniform_of_next_step':
        return line.top_k != 1 and collision(line.name) <= COLLISION_CAP
    if line.top_k is None or line.top_k >= line.V:
        return False
    lg = draw_logits(line.name)
    kth = _kth(lg, line)
    if mutant == 'threshold_strict':
        return bool(((lg == kth).sum(1) >= 8).all())
    return bool((kth == 0).all())


COLLISION_CAP = 0.4


@functools.lru_cache(maxsize=None)
def collision(name):
    """sum_v p_v^2 of the float64 definition, averaged over the rows: the probability that an INDEPENDENT uniform accepts a draw.  It is at
    least 1 / (kept tokens): with top_k = 2 no check can reject more than half of the draws under foreign uniforms, and the sharp line
    (T = 0.05) keeps nearly all mass on one token.  Where it exceeds COLLISION_CAP the tooth "the next step's uniforms reject more than
    half" is replaced by "at least half of the expected (1 - collision) share"."""
    _, cdf, _ = draw_reference(name)
    p = np.diff(cdf, axis=1, prepend=0.0) / cdf[:, -1:]
    return float((p * p).sum(1).mean())


def rejections_wanted(name, n):
    """How many of n draws the next step's uniforms must reject (strictly more than)."""
    c = collision(name)
    return n // 2 if c <= COLLISION_CAP else int(0.5 * (1.0 - c) * n)


def inv_temperature(T):
    return np.float32(1.0 / float(T))                      # ops.gpt_sample_cfg: 1 / T rounded to float32


def kept(logits, line, mutant=None):
    if line.top_k is None:
        return np.ones(logits.shape, dtype=bool)
    kth = _kth(logits, line)
    if mutant == 'threshold_strict':
        return logits > kth
    keep = logits >= kth
    if mutant == 'signed_zero_split':                      # with the zeros ordered apart, the k-th largest of the +-0 row is a +0.0
        keep = keep & ~(np.signbit(logits) & (logits == 0) & (kth == 0))
    return keep


def draw_reference(name, mutant=None):
    """(keep [ROWS, V], cdf float64 [ROWS, V], u [ROWS, STEPS])."""
    line = DRAW_BY_NAME[name]
    lg = draw_logits(name)
    keep = kept(lg, line, mutant)
    with np.errstate(invalid='ignore'):
        l = (lg * inv_temperature(line.T)).astype(np.float32).astype(np.float64)
        e = np.where(keep, np.exp(l - l.max(1, keepdims=True)), 0.0)
    u = restated_u(ROWS, STEPS + 1, SEED)
    return keep, np.cumsum(e, axis=1), (u[:, 1:] if mutant == 'uniform_of_next_step' else u[:, :STEPS])


def _stand_in_masses(name):
    """Per row: (kept indices in vocabulary order, their fp32 cumulative masses pre + run, the per-chunk sums, total) by the definition."""
    line = DRAW_BY_NAME[name]
    lg = draw_logits(name)
    keep = kept(lg, line)
    inv_t = inv_temperature(line.T)
    chunk = 4 * ((line.V + 1023) // 1024)
    out = []
    for r in range(ROWS):
        with np.errstate(invalid='ignore'):
            l = (lg[r] * inv_t).astype(np.float32)
            ms = np.float32(lg[r].max() * inv_t)
            e = np.where(keep[r], np.exp((l - ms).astype(np.float32)).astype(np.float32), np.float32(0)).astype(np.float32)
        pad = np.zeros(256 * chunk, dtype=np.float32)
        pad[:line.V] = e
        run = np.cumsum(pad.reshape(256, chunk), axis=1, dtype=np.float32)         # left to right inside a chunk (adding 0 changes nothing)
        part = run[:, -1]
        incl = np.cumsum(part, dtype=np.float32)                                    # the chunk sums accumulated left to right
        pre = np.concatenate([np.zeros(1, np.float32), incl[:-1]])
        mass = (pre[:, None] + run).astype(np.float32).reshape(-1)[:line.V]
        idx = np.nonzero(keep[r])[0]
        out.append((idx, mass[idx], part, incl[-1], chunk))
    return out


@functools.lru_cache(maxsize=None)
def stand_in_draw(name):
    """tokens int64 [ROWS, STEPS]: the definition of include/halo.h in fp32."""
    line = DRAW_BY_NAME[name]
    u = restated_u(ROWS, STEPS, SEED).astype(np.float32)                            # (r >> 8) * 2^-24 is exact in fp32
    tokens = np.zeros((ROWS, STEPS), dtype=np.int64)
    lg = draw_logits(name)
    for r, (idx, mass, part, total, chunk) in enumerate(_stand_in_masses(name)):
        if line.top_k == 1:
            tokens[r] = int(np.argmax(lg[r]))
            continue
        target = (u[r] * total).astype(np.float32)
        at = np.searchsorted(mass, target, side='right')                           # the first kept v with mass > target (mass is monotone)
        # rounding left nothing above the target: the last kept index of the last chunk with mass
        last = int(np.nonzero(part > 0)[0][-1])
        fallback = idx[idx < (last + 1) * chunk][-1]
        tokens[r] = np.where(at < len(idx), idx[np.minimum(at, len(idx) - 1)], fallback)
    return tokens


@functools.lru_cache(maxsize=None)
def draw_delta(name):
    """(delta, the stand-in's worst |cdf32 - cdf64| / total on the line)."""
    keep, cdf, _ = draw_reference(name)
    worst = 0.0
    for r, (idx, mass, part, total, chunk) in enumerate(_stand_in_masses(name)):
        worst = max(worst, float(np.abs(mass.astype(np.float64) / np.float64(total) - cdf[r, idx] / cdf[r, -1]).max()))
    return max(1e-5, FACTOR * worst), worst


def draws_accepted(name, tokens, mutant=None):
    """bool [ROWS, STEPS]: ``tokens`` against the (mutated) float64 definition at the line's delta."""
    keep, cdf, u = draw_reference(name, mutant)
    return accepted(tokens, u, keep, cdf, delta=draw_delta(name)[0])
