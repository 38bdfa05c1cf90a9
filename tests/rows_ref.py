"""Yardstick of the small row-wise and elementwise launches every model path goes through (csrc/gpt.hip: embedding, LayerNorm forward and
backward, cross-entropy, GELU; csrc/elementwise.hip: log_softmax_fwd / bwd, colsum; csrc/conv.hip: im2col_cl, col2im_cl, dwconv1d_cl,
dwconv1d_cl_bwd): each launch restated in float64 on the exact fp32 inputs, an fp32 stand-in advanced in the kernel's own order with one
rounding per operation, the per-element scale S, the bound a device is held to, the case tables at the kernels' dispatch edges, the exact
small-integer cases and the mutants.  Shared by tests/test_rows_ref_cpu.py and tests/test_gpu_rows_f64.py; holds no tests.  CPU only.

Three readings of a case, each a dict output name -> tensor:

``reference(case)``  float64 throughout; the mutants are switches on it.
``stand_in(case)``   fp32 in the kernel's order: lane-strided partial sums (c = lane, lane + 64, ...) met by the wave's butterfly
                     (halo_common.h wave_sum: four DPP rotations inside a row of 16 lanes, then the two row exchanges), the 32 slices and 4
                     accumulators of colsum_kernel, the chunk order of the LayerNorm-backward and dwconv1d_cl_bwd partials, the 256 running
                     (max, sum) pairs of cross_entropy_kernel and their merges, ``__expf(x)`` as exp2(fp32(x log2 e)), the tanh of the GELU as
                     m = exp2(-2.88539 |u|), (1 - m) * (1 / (1 + m)), fmaf where the kernel says fmaf.
``scale(case)``      S per output element: the sum of the absolute values of the terms the kernel adds, plus the conditioning terms written
                     next to each launch below (an fp32 rounding of a mean in front of a subtraction, of an argument in front of an exp).

A device is held, on EVERY element, to |got - ref| <= max(FACTOR x the stand-in's own deviation on the case, FLOOR) x S; where the reference
is not finite (-inf logits) the device must give the same value.  FACTOR = 4 is the factor tests/test_gpu_optim.py holds plain fp32 VALU
kernels to; FLOOR = 2^-22 is gemm_ref's (two fp32 half-ulps of a value of size S).  Nothing in a bound comes from a device.

Case modes: ``bound`` as above; ``exact`` -- small integers or pure copies, every partial sum representable, reference == stand-in bit for
bit and a device must give the same bits whatever its order (the float atomics of embed_bwd included); ``standin`` -- embed_bwd_ordered
promises the fp32 sum in token order, so a device must equal the stand-in bit for bit (and the stand-in stays inside the rail)."""
import functools
import zlib
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from gemm_ref import FLOOR

F32, F64 = torch.float32, torch.float64
FACTOR = 4.0                               # tests/test_gpu_optim.py: 4 x the fp32 restatement's own error, for plain fp32 VALU kernels
TINY = 2.0 ** -126                         # the smallest normal fp32: a result that underflows is rounded at this magnitude
NINF = float('-inf')
EPS = 1e-5
LN_CHUNKS = 512                            # HALO_LN_BWD_CHUNKS (gpt.hip:7)
DW_CHUNKS = 64                             # HALO_DWCONV_BWD_CHUNKS (conv.hip:143)


def f32(v):
    return torch.tensor(v, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------------------
# the kernels' summation orders in fp32
# ------------------------------------------------------------------------------------------------------------------------------
def wave_sum32(v):
    """halo_common.h wave_sum on [..., 64] lanes: row_ror 8, 4, 2, 1 inside each row of 16, then rows r + (r ^ 1), then + (r ^ 2)."""
    a = v.reshape(*v.shape[:-1], 4, 16)
    for n in (8, 4, 2, 1):
        a = a + torch.roll(a, n, -1)
    a = a + a[..., [1, 0, 3, 2], :]
    a = a + a[..., [2, 3, 0, 1], :]
    return a[..., 0, 0]


def strided(x, fill=0.0):
    """[rows, C] -> [rows, trips, 64]: trip t holds columns 64 t + lane; the last trip filled up."""
    rows, C = x.shape
    trips = (C + 63) // 64
    p = torch.full((rows, trips * 64), fill, dtype=x.dtype)
    p[:, :C] = x
    return p.view(rows, trips, 64)


def lane_sum32(x):
    """One wave per row: s += x[c] over c = lane, lane + 64, ...; wave_sum."""
    p = strided(x)
    s = torch.zeros(x.shape[0], 64, dtype=F32)
    for t in range(p.shape[1]):
        s = s + p[:, t]
    return wave_sum32(s)


def colsum32(x):
    """colsum_kernel (elementwise.hip:300-326) on [rows, cols]: slice = r % 32; while r + 96 < rows the four accumulators take rows r, r + 32,
    r + 64, r + 96 (r += 128); the rest goes to s0 (r += 32); (s0 + s1) + (s2 + s3); the 32 slices added in order from zero."""
    rows, cols = x.shape
    blocks = (rows + 127) // 128
    p = torch.zeros(blocks * 128, cols, dtype=F32)
    p[:rows] = x
    s = [torch.zeros(32, cols, dtype=F32) for _ in range(4)]
    sl = torch.arange(32)[:, None]
    for k in range(blocks):
        xb = p[128 * k:128 * k + 128].view(4, 32, cols)
        whole = (sl + 128 * k + 96 < rows).expand(32, cols)
        tail = ((s[0] + xb[0]) + xb[1]) + xb[2]                              # rows beyond ``rows`` are zeros
        for j in range(1, 4):
            s[j] = torch.where(whole, s[j] + xb[j], s[j])
        s[0] = torch.where(whole, s[0] + xb[0], tail)
    part = (s[0] + s[1]) + (s[2] + s[3])
    t = torch.zeros(cols, dtype=F32)
    for i in range(32):
        t = t + part[i]
    return t


def fma32(a, b, c):
    """fmaf: the product of two fp32 is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


L2E = f32(1.4426950408889634)


def fast_exp32(x):
    """__expf: the hardware exp2 of fp32(x * log2 e)."""
    return torch.exp2(x * L2E)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class Case:
    launch: str
    tag: str
    p: dict = field(default_factory=dict)
    mode: str = 'bound'                    # bound | exact | standin
    reach: str = ''

    @property
    def name(self):
        return f'{self.launch}-{self.tag}'

    def __getattr__(self, k):
        try:
            return self.__dict__['p'][k]
        except KeyError:
            raise AttributeError(k)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).float()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward (gpt.hip:24-42).  S = |w| (|x - mean| + |mean|) rstd + |b|: the |mean| term is the conditioning of x - mean under the
# fp32 rounding of the mean.
# ------------------------------------------------------------------------------------------------------------------------------
def _ln_case(C, rows, bias, dist):
    reach = []
    if C < 64:
        reach.append('idle lanes')
    if C % 64:
        reach.append('partial last trip')
    if rows % 4:
        reach.append('waves of the last workgroup return')
    if rows >= 5:
        reach.append('row 3 constant (variance 0)')
    return Case('ln_fwd', f'C{C}_r{rows}_{"b" if bias else "nb"}_{dist}', dict(C=C, rows=rows, bias=bias, dist=dist), reach=', '.join(reach))


LN_FWD = [_ln_case(*a) for a in [
    (1, 1, True, 'wide'), (1, 5, False, 'far'), (3, 5, False, 'wide'), (3, 1, True, 'far'), (63, 37, True, 'wide'), (63, 5, True, 'far'),
    (64, 1, False, 'wide'), (64, 5, True, 'far'), (65, 1, False, 'wide'), (65, 5, True, 'far'), (200, 37, True, 'wide'),
    (200, 5, False, 'far'), (768, 5, True, 'wide'), (768, 1, True, 'far'), (1028, 5, True, 'wide'), (1028, 37, False, 'far')]]


def _ln_x(g, rows, C, dist):
    x = _randn(g, rows, C) * 2 + 0.5 if dist == 'wide' else 30 + 0.5 * _randn(g, rows, C)
    if rows >= 5:
        x[3] = 1.7
    return x


def ln_fwd_inputs(c, g):
    return {'x': _ln_x(g, c.rows, c.C, c.dist), 'w': _randn(g, c.C) * 0.5 + 1, 'b': _randn(g, c.C) * 0.5 + 0.25 if c.bias else None}


def _ln_stats64(x, eps=EPS, mutant=None):
    X = x.double()
    C = X.shape[1]
    mean = X.mean(1, keepdim=True)
    d = X - mean
    var = (d * d).sum(1, keepdim=True) / (C - 1 if mutant == 'var_cm1' and C > 1 else C)
    e = float(f32(eps))
    rstd = 1.0 / (var.sqrt() + e) if mutant == 'eps_outside' else 1.0 / (var + e).sqrt()
    return mean, d, rstd


def ln_fwd_ref(c, i, mutant=None):
    mean, d, rstd = _ln_stats64(i['x'], EPS, mutant)
    o = d * rstd * i['w'].double()
    if i['b'] is not None:
        b = i['b'].double().expand_as(o).clone()
        if mutant == 'tail_no_bias' and c.C % 64:
            b[:, c.C // 64 * 64:] = 0
        o = o + b
    return {'y': o}


def _ln_stats32(x, eps=EPS):
    Cf = f32(float(x.shape[1]))
    mean = (lane_sum32(x) / Cf)[:, None]
    d = x - mean
    rstd = torch.rsqrt(lane_sum32(d * d) / Cf + eps)[:, None]
    return mean, d, rstd


def ln_fwd_stand(c, i):
    mean, d, rstd = _ln_stats32(i['x'])
    o = d * rstd * i['w']
    return {'y': o + i['b'] if i['b'] is not None else o}


def ln_fwd_scale(c, i):
    mean, d, rstd = _ln_stats64(i['x'])
    S = i['w'].double().abs() * (d.abs() + mean.abs()) * rstd
    return {'y': S + i['b'].double().abs() if i['b'] is not None else S}


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward (gpt.hip:93-250, :374-395).  dx = dres + rstd (g - mean g - xhat mean(g xhat)), g = dy w; dw = sum dy xhat; db = sum dy.
# S(dx) = |dres| + rstd (|g| + mean |g| + |xhat| mean |g xhat|) + rstd k (mean |g xhat| + |xhat| mean |g|), k = |mean| rstd the
# conditioning of xhat under the rounding of the mean; S(dw) = sum |dy| (|xhat| + k); S(db) = sum |dy|.
# ------------------------------------------------------------------------------------------------------------------------------
def ln_bwd_path(c):
    return 'fused' if c.C % 4 == 0 and c.C <= 2048 and not c.offset else 'twopass'


def _lnb(C, rows, dres=True, has_bias=True, offset=False, bf16=False):
    p = dict(C=C, rows=rows, dres=dres, has_bias=has_bias, offset=offset, bf16=bf16)
    tag = f'C{C}_r{rows}' + ('' if dres else '_nodres') + ('' if has_bias else '_nobias') + ('_offset' if offset else '') + ('_bf16' if bf16 else '')
    c = Case('ln_bwd', tag, p)
    path = ln_bwd_path(c)
    reach = [f'fused<{4 if C <= 1024 else 8}>' if path == 'fused' else 'two-pass fallback' + (' via aligned' if offset else '')]
    if rows > 2048:
        reach.append("a wave's second row under the 512-workgroup cap")
    if bf16:
        reach.append('bf16 rows == the fp32 rows rounded')
    c.reach = ', '.join(reach)
    return c


LN_BWD = [_lnb(4, 1), _lnb(252, 5, dres=False), _lnb(256, 3), _lnb(260, 5, has_bias=False), _lnb(1024, 3), _lnb(1028, 5, dres=False),
          _lnb(2048, 3), _lnb(2052, 5), _lnb(201, 5, has_bias=False), _lnb(2052, 3, dres=False), _lnb(8, 1), _lnb(8, 3, dres=False),
          _lnb(8, 5), _lnb(8, 2049), _lnb(8, 2053, dres=False, has_bias=False), _lnb(256, 5, offset=True), _lnb(256, 5, bf16=True),
          _lnb(1028, 3, bf16=True, dres=False)]


def ln_bwd_inputs(c, g):
    return {'dy': _randn(g, c.rows, c.C), 'x': _randn(g, c.rows, c.C) * 2 + 0.5, 'w': _randn(g, c.C) * 0.5 + 1,
            'dres': _randn(g, c.rows, c.C) if c.dres else None}


def _ln_last_rows(c):
    """The rows whose dw / db contribution sits in the last partial row the column sums read."""
    r = torch.arange(c.rows)
    if ln_bwd_path(c) == 'fused':
        wgs = min(LN_CHUNKS, (c.rows + 3) // 4)
        return (r // 4) % wgs == wgs - 1
    chunks = min(c.rows, LN_CHUNKS)
    rpc = -(-c.rows // chunks)
    return r >= (-(-c.rows // rpc) - 1) * rpc


def ln_bwd_ref(c, i, mutant=None):
    mean, d, rstd = _ln_stats64(i['x'])
    xh, dy = d * rstd, i['dy'].double()
    g = dy * i['w'].double()
    mg, mgx = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = rstd * (g - mg - (0 if mutant == 'proj_dropped' else xh * mgx))
    if i['dres'] is not None and mutant != 'dres_dropped':
        dx = dx + i['dres'].double()
    keep = torch.ones(c.rows, dtype=torch.bool)
    if mutant == 'rows_ge_2048_skipped':
        keep = torch.arange(c.rows) < 2048
        dx = dx * keep[:, None]
    if mutant == 'last_partial_dropped':
        keep = ~_ln_last_rows(c)
    out = {'dx': dx, 'dw': (dy * xh)[keep].sum(0)}
    if c.has_bias:
        out['db'] = dy[keep].sum(0)
    return out


def _rows_view(t, lead):
    """[rows, W] -> zero rows appended -> [lead..., W]."""
    n = 1
    for v in lead:
        n *= v
    p = torch.zeros(n, t.shape[1], dtype=t.dtype)
    p[:t.shape[0]] = t
    return p.view(*lead, t.shape[1])


def _ln_bwd_fused32(dy, x, w, dres):
    rows, C = x.shape
    MAXV = 4 if C <= 1024 else 8
    W = 256 * MAXV

    def lanes(t):                                                            # [rows, C] -> [rows, MAXV, 64, 4], zeros beyond C
        p = torch.zeros(t.shape[0], W, dtype=F32)
        p[:, :C] = t
        return p.view(t.shape[0], MAXV, 64, 4)
    xv, dv, wv = lanes(x), lanes(dy), lanes(w[None])
    inside = (torch.arange(W) < C).view(1, MAXV, 64, 4)
    inv_c = f32(1.0) / f32(float(C))
    s = torch.zeros(rows, 64)
    for v in range(MAXV):
        s = s + ((xv[:, v, :, 0] + xv[:, v, :, 1]) + (xv[:, v, :, 2] + xv[:, v, :, 3]))
    mean = (wave_sum32(s) * inv_c).view(rows, 1, 1, 1)
    d = torch.where(inside, xv - mean, torch.zeros(()))
    var = torch.zeros(rows, 64)
    for v in range(MAXV):
        for e in range(4):
            var = var + d[:, v, :, e] * d[:, v, :, e]
    rstd = torch.rsqrt(wave_sum32(var) * inv_c + EPS).view(rows, 1, 1, 1)
    xh = d * rstd
    g = dv * wv
    gx = g * xh
    sg, sgx = torch.zeros(rows, 64), torch.zeros(rows, 64)
    for v in range(MAXV):
        for e in range(4):
            sg = sg + g[:, v, :, e]
            sgx = sgx + gx[:, v, :, e]
    mg, mgx = (wave_sum32(sg) * inv_c).view(rows, 1, 1, 1), (wave_sum32(sgx) * inv_c).view(rows, 1, 1, 1)
    dd = rstd * (g - mg - xh * mgx)
    if dres is not None:
        dd = dd + lanes(dres)
    dx = dd.view(rows, W)[:, :C].contiguous()
    # the partials: workgroup b's wave k walks rows 4 b + k, + 4 wgs, ...; the waves are added in wave order; colsum over the workgroups
    wgs = min(LN_CHUNKS, (rows + 3) // 4)
    trips = -(-rows // (4 * wgs))
    out = []
    for t in ((dv * xh).view(rows, W), dv.view(rows, W)):
        p = _rows_view(t, (trips, wgs, 4))
        a = torch.zeros(wgs, 4, W)
        for k in range(trips):
            a = a + p[k]
        out.append(colsum32((((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3])[:, :C]))
    return dx, out[0], out[1]


def _ln_bwd_twopass32(dy, x, w, dres):
    rows, C = x.shape
    Cf = f32(float(C))
    mean, d, rstd = _ln_stats32(x)
    g = dy * w
    mg, mgx = (lane_sum32(g) / Cf)[:, None], (lane_sum32(g * d * rstd) / Cf)[:, None]
    dd = rstd * (g - mg - d * rstd * mgx)
    dx = dres + dd if dres is not None else dd
    chunks = min(rows, LN_CHUNKS)
    rpc = -(-rows // chunks)
    used = -(-rows // rpc)
    out = []
    for t in (dy * d * rstd, dy):
        p = _rows_view(t, (used, rpc))
        a = torch.zeros(used, C)
        for k in range(rpc):
            a = a + p[:, k]
        out.append(colsum32(a))
    return dx, out[0], out[1]


def ln_bwd_stand(c, i):
    fn = _ln_bwd_fused32 if ln_bwd_path(c) == 'fused' else _ln_bwd_twopass32
    dx, dw, db = fn(i['dy'], i['x'], i['w'], i['dres'])
    out = {'dx': dx, 'dw': dw}
    if c.has_bias:
        out['db'] = db
    return out


def ln_bwd_scale(c, i):
    mean, d, rstd = _ln_stats64(i['x'])
    xh, dy = d * rstd, i['dy'].double().abs()
    g = dy * i['w'].double().abs()
    k = mean.abs() * rstd
    mg, mgx = g.mean(1, keepdim=True), (g * xh.abs()).mean(1, keepdim=True)
    S = rstd * (g + mg + xh.abs() * mgx) + rstd * k * (mgx + xh.abs() * mg)
    if i['dres'] is not None:
        S = S + i['dres'].double().abs()
    out = {'dx': S, 'dw': (dy * (xh.abs() + k)).sum(0)}
    if c.has_bias:
        out['db'] = dy.sum(0)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# cross-entropy (gpt.hip:44-88, :264-277).  lse = m + log s, s = sum exp(x - m) >= 1: S(lse) = |m| + |log s| + 1 (the 1: a relative error
# of s, whose terms are all positive, is an absolute error of log s); S(loss) = S(lse) + |x[target]|; ignored rows are 0 exactly.
# bwd: (exp(x - lse) - onehot) g with the fp32 lse an input: S = (p (1 + |x - lse|) + onehot) |g| + TINY (1 + |g|), p = exp(x - lse); |x - lse| is
# the conditioning of the exp under the rounding of its argument, TINY the underflow of p and of the product.
# PRECONDITION of all three launches: every target is ignore_index or inside [0, V) -- the kernels read row[target] unchecked.
# ------------------------------------------------------------------------------------------------------------------------------
def _ce(V, ignore, scale=1.0, ld=None, offset=False, ninf=None, grad1=False):
    ld = V if ld is None else ld
    p = dict(V=V, ld=ld, ignore=ignore, scale=scale, offset=offset, ninf=ninf, grad1=grad1, rows=9)
    vec = ld % 4 == 0 and not offset
    p['vec'] = vec
    tag = f'V{V}' + (f'_ld{ld}' if ld != V else '') + f'_ign{ignore}_s{scale:g}' + ('_offset' if offset else '') + (f'_{ninf}' if ninf else '') + \
        ('_g1' if grad1 else '')
    reach = ('vector body' + (' with a scalar tail' if V % 4 else '')) if vec and V >= 4 else 'scalar path'
    if ninf == 'half':
        reach += '; threads whose first groups are all -inf'
    return Case('ce', tag, p, reach=reach)


CE = [_ce(1, -100), _ce(3, 0, 30.0), _ce(4, -100), _ce(333, 0, ninf='scattered'), _ce(1024, -100, 30.0), _ce(1028, 0, ninf='scattered', grad1=True),
      _ce(5000, 0), _ce(1030, 0, ld=1032, ninf='scattered'), _ce(1024, -100, 30.0, ld=1025), _ce(1024, 0, offset=True, ninf='scattered'),
      _ce(2048, -100, ninf='half'), _ce(333, -100, 30.0, grad1=True)]


def ce_wave(c, col):
    """The wave (0..3) of the workgroup that reads column ``col``."""
    V4 = c.V // 4 if c.vec else 0
    t = (col // 4) % 256 if col < 4 * V4 else (col - 4 * V4) % 256
    return t // 64


def ce_inputs(c, g):
    rows, V = c.rows, c.V
    x = _randn(g, rows, V) * c.scale
    lo = 1 if c.ignore == 0 else 0
    if c.ninf == 'half':
        lo = 1024
    tgt = torch.randint(lo, V, (rows,), generator=g) if V > lo else torch.zeros(rows, dtype=torch.int64)
    if c.ignore != 0:
        tgt[0] = 0 if c.ninf != 'half' else 1024
    tgt[5] = V - 1
    if c.ninf == 'scattered':
        x[torch.rand(rows, V, generator=g) < 0.3] = NINF
    if c.ninf == 'half':
        x[:, :1024] = NINF
    fin = torch.where(torch.isinf(x), torch.full_like(x, -1e30), x)
    w1 = [col for col in range(V) if ce_wave(c, col) == 1 and not (c.ninf == 'half' and col < 1024)]
    x[1, w1[-1] if w1 else 0] = fin[1].max() + 80                  # one logit far above the rest, in wave 1's share where it has one
    x[2] = 1.25                                                              # a row of equal logits
    if c.ninf == 'half':
        x[2, :1024] = NINF
    x[3, V - 1] = fin[3].max() + 20                                # the last column carries the row
    x[torch.arange(rows), tgt] = torch.where(torch.isinf(x[torch.arange(rows), tgt]), torch.zeros(rows), x[torch.arange(rows), tgt])
    tgt[4] = tgt[7] = c.ignore                                               # ignored rows
    lse = ce_ref(c, {'x': x, 'tgt': tgt}, None, fwd_only=True)['lse'].float()
    grad = _randn(g, 1) + 2 if c.grad1 else _randn(g, rows)
    return {'x': x, 'tgt': tgt, 'lse': lse, 'grad': grad}


def ce_ref(c, i, mutant=None, fwd_only=False):
    X, tgt = i['x'].double(), i['tgt']
    rows, V = X.shape
    live = tgt != c.ignore
    cols = torch.arange(V)
    seen = torch.ones(V, dtype=torch.bool)
    if mutant == 'tail_ignored':
        seen = cols < V - V % 4
    if mutant == 'wave_dropped':
        seen = torch.tensor([ce_wave(c, col) != 1 for col in range(V)])
    t = torch.where(live, tgt, torch.zeros_like(tgt))
    if mutant == 'target_off_by_one':
        t = (t + 1) % V
    lse = torch.logsumexp(torch.where(seen, X, torch.full_like(X, NINF)), 1)
    out = {'loss': torch.where(live, lse - X[torch.arange(rows), t], torch.zeros(rows, dtype=F64)),
           'lse': torch.where(live, lse, torch.zeros(rows, dtype=F64))}
    if fwd_only:
        return out
    gr = i['grad'].double().expand(rows)[:, None]
    d = (torch.exp(X - i['lse'].double()[:, None]) - F.one_hot(t, V).double()) * gr
    if mutant in ('tail_ignored', 'wave_dropped'):
        d = torch.where(seen, d, X)
    d = torch.where(live[:, None], d, X if mutant == 'ignored_not_zeroed' else torch.zeros_like(d))
    out['dlogits'] = d
    return out


def _merge32(m, s, om, os):
    nm = torch.maximum(m, om)
    dead = nm == NINF
    s2 = s * fast_exp32(m - nm) + os * fast_exp32(om - nm)
    return torch.where(dead, m, nm), torch.where(dead, s, s2)


def _online32(m, s, v):
    """One step of a thread's running (max, sum): v [rows, 256, k] (k = 4: a 16-byte group, 1: a scalar); a group that is all -inf is
    skipped, as the kernel skips it (with the max still -inf, -inf - max would be NaN)."""
    vm = v.max(-1).values
    livegroup, up = vm > NINF, vm > m
    s = torch.where(up, s * fast_exp32(m - vm), s)
    m = torch.where(up, vm, m)
    e = fast_exp32(v - m[..., None])
    add = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3]) if v.shape[-1] == 4 else e[..., 0]
    return m, torch.where(livegroup, s + add, s)


def ce_stand(c, i):
    x, tgt = i['x'], i['tgt']
    rows, V = x.shape
    V4 = V // 4 if c.vec else 0
    m, s = torch.full((rows, 256), NINF), torch.zeros(rows, 256)
    for width, part in ((4, x[:, :4 * V4]), (1, x[:, 4 * V4:])):
        n = part.shape[1] // width
        trips = -(-n // 256)
        p = torch.full((rows, trips * 256 * width), NINF)
        p[:, :n * width] = part
        p = p.view(rows, trips, 256, width)
        for t in range(trips):
            m, s = _online32(m, s, p[:, t])
    m, s = m.view(rows, 4, 64), s.view(rows, 4, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = _merge32(m, s, m[..., lanes ^ o], s[..., lanes ^ o])
    M, Sm = m[:, 0, 0], s[:, 0, 0]
    for w in range(1, 4):
        M, Sm = _merge32(M, Sm, m[:, w, 0], s[:, w, 0])
    lse = M + torch.log(Sm)
    live = tgt != c.ignore
    t = torch.where(live, tgt, torch.zeros_like(tgt))
    z = torch.zeros(rows)
    out = {'loss': torch.where(live, lse - x[torch.arange(rows), t], z), 'lse': torch.where(live, lse, z)}
    d = (torch.exp(x - i['lse'][:, None]) - F.one_hot(t, V).float()) * i['grad'].expand(rows)[:, None]
    out['dlogits'] = torch.where(live[:, None], d, torch.zeros_like(d))
    return out


def ce_scale(c, i):
    X, tgt = i['x'].double(), i['tgt']
    rows, V = X.shape
    live = tgt != c.ignore
    t = torch.where(live, tgt, torch.zeros_like(tgt))
    m = X.max(1).values
    S = m.abs() + torch.log(torch.exp(X - m[:, None]).sum(1)).abs() + 1
    z = torch.zeros(rows, dtype=F64)
    arg = X - i['lse'].double()[:, None]
    p = torch.exp(arg)
    cond = torch.where(p > 0, 1 + arg.abs(), torch.ones_like(p))
    gr = i['grad'].double().abs().expand(rows)[:, None]
    Sd = (p * cond + F.one_hot(t, V).double()) * gr + TINY * (1 + gr)
    return {'loss': torch.where(live, S + X[torch.arange(rows), t].abs(), z), 'lse': torch.where(live, S, z),
            'dlogits': torch.where(live[:, None], Sd, torch.zeros_like(Sd))}


# ------------------------------------------------------------------------------------------------------------------------------
# log-softmax (elementwise.hip:268-297).  fwd y = x - (m + log s): S = |x| + |m| + |log s| + 1.  bwd dx = dy - exp(y) sum dy on the y it is
# handed (the device's own on the device): S = |dy| + exp(y) sum |dy| + TINY (1 + sum |dy|): exp(y) and its product may underflow.
# ------------------------------------------------------------------------------------------------------------------------------
def _lsm(cols, rows, scale=1.0, ninf=False):
    tag = f'c{cols}_r{rows}_s{scale:g}' + ('_ninf' if ninf else '')
    return dict(tag=tag, p=dict(cols=cols, rows=rows, scale=scale, ninf=ninf),
                reach=('idle lanes' if cols < 64 else 'partial last trip' if cols % 64 else 'whole trips'))


_LSM = [_lsm(1, 1), _lsm(29, 6, 30.0), _lsm(64, 1, 1.0, True), _lsm(64, 6, 30.0), _lsm(65, 6, 1.0, True), _lsm(65, 1, 30.0), _lsm(1000, 6),
        _lsm(1000, 1, 30.0, True), _lsm(29, 1, 1.0, True)]
LSM_FWD = [Case('lsm_fwd', **d) for d in _LSM]
LSM_BWD = [Case('lsm_bwd', **d) for d in _LSM]


def lsm_fwd_inputs(c, g):
    x = _randn(g, c.rows, c.cols) * c.scale
    if c.ninf and c.cols > 1:
        x[torch.rand(c.rows, c.cols, generator=g) < 0.3] = NINF
        x[:, 0] = 0.5
    x[0, c.cols - 1] = torch.where(torch.isinf(x[0]), torch.full_like(x[0], -1e30), x[0]).max() + 1        # the last column leads row 0
    return {'x': x}


def _tail_seen(cols, mutant):
    return torch.arange(cols) < cols // 64 * 64 if mutant == 'tail_dropped' else torch.ones(cols, dtype=torch.bool)


def lsm_fwd_ref(c, i, mutant=None):
    X = i['x'].double()
    lse = torch.logsumexp(torch.where(_tail_seen(c.cols, mutant), X, torch.full_like(X, NINF)), 1, keepdim=True)
    return {'y': X - lse}


def lsm_fwd_stand(c, i):
    x = i['x']
    m = strided(x, NINF).max(1).values.max(1, keepdim=True).values
    lse = m + torch.log(lane_sum32(torch.exp(x - m)))[:, None]
    return {'y': x - lse}


def lsm_fwd_scale(c, i):
    X = i['x'].double()
    m = X.max(1, keepdim=True).values
    S = X.abs() + m.abs() + torch.log(torch.exp(X - m).sum(1, keepdim=True)).abs() + 1
    return {'y': torch.where(torch.isinf(X), torch.ones_like(S), S)}


def lsm_bwd_inputs(c, g):
    i = lsm_fwd_inputs(c, g)
    return {'y': lsm_fwd_stand(c, i)['y'], 'dy': _randn(g, c.rows, c.cols)}


def lsm_bwd_ref(c, i, mutant=None):
    dy = i['dy'].double()
    s = (dy * _tail_seen(c.cols, mutant)).sum(1, keepdim=True)
    return {'dx': dy - torch.exp(i['y'].double()) * s}


def lsm_bwd_stand(c, i):
    return {'dx': i['dy'] - torch.exp(i['y']) * lane_sum32(i['dy'])[:, None]}


def lsm_bwd_scale(c, i):
    dy = i['dy'].double().abs()
    s = dy.sum(1, keepdim=True)
    return {'dx': dy + torch.exp(i['y'].double()) * s + TINY * (1 + s)}


# ------------------------------------------------------------------------------------------------------------------------------
# colsum (elementwise.hip:300-326).  S = sum |x| per column.
# ------------------------------------------------------------------------------------------------------------------------------
def _cs(rows, cols, mode='bound'):
    reach = ('the 128-row unrolled loop' if rows > 96 else 'the tail loop only') + (' and its tail' if rows > 96 and rows % 128 else '') + \
        ('; partial column block' if cols % 32 else '')
    return Case('colsum', f'r{rows}_c{cols}' + ('_int' if mode == 'exact' else ''), dict(rows=rows, cols=cols), mode, reach)


COLSUM = [_cs(1, 1), _cs(31, 33), _cs(32, 200), _cs(33, 31), _cs(127, 1), _cs(128, 31), _cs(129, 33), _cs(300, 33), _cs(300, 31, 'exact'),
          _cs(129, 200, 'exact')]


def colsum_inputs(c, g):
    return {'x': _ints(g, c.rows, c.cols) if c.mode == 'exact' else _randn(g, c.rows, c.cols)}


def colsum_ref(c, i, mutant=None):
    X = i['x'].double()
    r = torch.arange(c.rows)
    if mutant == 'rows_past_128_dropped':
        X = X * (r < c.rows // 128 * 128)[:, None]
    if mutant == 'slice31_dropped':
        X = X * (r % 32 != 31)[:, None]
    return {'out': X.sum(0)}


def colsum_stand(c, i):
    return {'out': colsum32(i['x'])}


def colsum_scale(c, i):
    return {'out': i['x'].double().abs().sum(0)}


# ------------------------------------------------------------------------------------------------------------------------------
# GELU (gpt.hip:253-262, halo_common.h:105-121, :167-172).  fwd y = 0.5 v (1 + t), t = tanh(k (v + 0.044715 v^3)) or erf(v / sqrt 2):
# S = 0.5 |v| (1 + |t|) + TINY -- in the negative tail 1 + t cancels in fp32 (torch's fp32 GELU shares that; float64 does not), and S keeps
# the 1.  bwd da = dy (0.5 (1 + t) + v t'/2): S = |dy| (0.5 (1 + |t|) + |second term| (1 + z)) + TINY, z = 2 |u| resp. v^2 / 2 the
# conditioning of the exp inside t' under the rounding of its argument.
# ------------------------------------------------------------------------------------------------------------------------------
K0, K1 = 0.7978845608028654, 0.044715


def _gelu_cases(launch):
    out = []
    for kind in ('tanh', 'erf'):
        for n in (1, 255, 257):
            out.append(Case(launch, f'{kind}_n{n}', dict(kind=kind, n=n), reach='one workgroup' if n < 256 else 'a second workgroup of one element'))
    return out


GELU_FWD, GELU_BWD = _gelu_cases('gelu_fwd'), _gelu_cases('gelu_bwd')


def gelu_inputs(c, g):
    if c.n == 1:
        a = torch.tensor([-2.25])
    else:
        grid = torch.linspace(-12, 12, 193)
        sub = torch.tensor([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, -2.0 ** -127, 2.0 ** -126, 3 * 2.0 ** -149])
        a = torch.cat([grid, sub, _randn(g, c.n - 201) * 3])
    return {'a': a, 'dy': _randn(g, c.n) + 0.1 * torch.sign(_randn(g, c.n))}


def _gelu64(a, kind):
    """(t, second term of the derivative, its conditioning)."""
    A = a.double()
    if kind == 'tanh':
        u = K0 * (A + K1 * A ** 3)
        t = torch.tanh(u)
        return t, 0.5 * A * (1 - t * t) * K0 * (1 + 3 * K1 * A * A), 2 * u.abs()
    return torch.erf(A * 0.7071067811865476), A * torch.exp(-0.5 * A * A) * 0.3989422804014327, 0.5 * A * A


def _kind(c, mutant):
    return {'tanh': 'erf', 'erf': 'tanh'}[c.kind] if mutant == 'kinds_swapped' else c.kind


def gelu_fwd_ref(c, i, mutant=None):
    t, _, _ = _gelu64(i['a'], _kind(c, mutant))
    return {'y': 0.5 * i['a'].double() * (1 + t)}


def gelu_bwd_ref(c, i, mutant=None):
    t, second, _ = _gelu64(i['a'], _kind(c, mutant))
    return {'da': i['dy'].double() * (0.5 * (1 + t) + second)}


def _gelu_tanh32(u):
    m = torch.exp2(f32(-2.8853900817779268) * u.abs())
    r = f32(1.0) / (1.0 + m)
    return torch.copysign((1.0 - m) * r, u), 4.0 * m * r * r


def gelu_fwd_stand(c, i):
    v = i['a']
    if c.kind == 'tanh':
        t, _ = _gelu_tanh32(f32(K0) * (v + f32(K1) * v * v * v))
    else:
        t = torch.erf(v * f32(0.7071067811865476))
    return {'y': 0.5 * v * (1.0 + t)}


def gelu_bwd_stand(c, i):
    x = i['a']
    if c.kind == 'tanh':
        t, s2 = _gelu_tanh32(f32(K0) * (x + f32(K1) * x * x * x))
        grad = 0.5 * (1.0 + t) + 0.5 * x * s2 * f32(K0) * (1.0 + f32(3.0) * f32(K1) * x * x)
    else:
        grad = 0.5 * (1.0 + torch.erf(x * f32(0.7071067811865476))) + x * torch.exp(-0.5 * x * x) * f32(0.3989422804014327)
    return {'da': i['dy'] * grad}


def gelu_fwd_scale(c, i):
    t, _, _ = _gelu64(i['a'], c.kind)
    return {'y': 0.5 * i['a'].double().abs() * (1 + t.abs()) + TINY}


def gelu_bwd_scale(c, i):
    t, second, z = _gelu64(i['a'], c.kind)
    return {'da': i['dy'].double().abs() * (0.5 * (1 + t.abs()) + second.abs() * (1 + z)) + TINY}


# ------------------------------------------------------------------------------------------------------------------------------
# embedding (gpt.hip:11-21, :279-318).  Forward and add_rows_bcast_ are one fp32 add: bit for bit.
# ------------------------------------------------------------------------------------------------------------------------------
VOCAB = 11


def _ids(g, B, T):
    ids = torch.randint(0, VOCAB - 2, (B, T), generator=g)                   # row VOCAB - 2 never has a token
    ids.view(-1)[-1] = VOCAB + 2                                             # clamped to vocab - 1
    if B * T > 1:
        ids.view(-1)[0] = -3                                                 # clamped to 0
    return ids


def _emb(B, T, C, wpe, pos0):
    return Case('embed_fwd', f'B{B}_T{T}_C{C}' + (f'_wpe_pos{pos0}' if wpe else ''), dict(B=B, T=T, C=C, wpe=wpe, pos0=pos0), 'exact',
                'ids -3 and vocab + 2 clamp' + (f'; positions pos0 + n % T' if wpe else '; no position table'))


EMBED_FWD = [_emb(1, 1, 4, False, 0), _emb(1, 1, 100, True, 5), _emb(3, 7, 4, True, 0), _emb(3, 7, 100, False, 0), _emb(3, 7, 300, True, 5),
             _emb(1, 1, 300, True, 0), _emb(3, 7, 100, True, 5)]
ADD_ROWS = [Case('add_rows', f'r{r}_T{T}_C{C}', dict(rows=r, T=T, C=C), 'exact', 'rows n % T') for r, T, C in
            [(1, 1, 4), (21, 7, 100), (21, 7, 300), (21, 3, 4)]]


def embed_fwd_inputs(c, g):
    return {'ids': _ids(g, c.B, c.T), 'wte': _randn(g, VOCAB, c.C), 'wpe': _randn(g, c.pos0 + c.T + 2, c.C) if c.wpe else None}


def _pos(n, T, pos0, mutant):
    return (0 if mutant == 'pos0_ignored' else pos0) + ((n // T) % T if mutant == 'pos_div' else n % T)


def embed_fwd_ref(c, i, mutant=None, dt=F64):
    ids = i['ids'].view(-1).clamp(0, VOCAB - 1)
    x = i['wte'].to(dt)[ids]
    if c.wpe:
        x = x + i['wpe'].to(dt)[_pos(torch.arange(ids.numel()), c.T, c.pos0, mutant)]
    return {'x': x}


def embed_fwd_stand(c, i):
    return embed_fwd_ref(c, i, None, F32)


def add_rows_inputs(c, g):
    return {'x': _randn(g, c.rows, c.C), 'p': _randn(g, c.T, c.C)}


def add_rows_ref(c, i, mutant=None, dt=F64):
    return {'x': i['x'].to(dt) + i['p'].to(dt)[_pos(torch.arange(c.rows), c.T, 0, mutant)]}


def add_rows_stand(c, i):
    return add_rows_ref(c, i, None, F32)


def _exact_scale(c, i):
    return None


# embed_bwd: dwte[id] += dx[n] (float atomics, any order: S = |dwte0| + sum |dx| per row); dwpe[pos0 + t] (+)= sum_b dx[b T + t] in order
def _eb(B, T, C, ids, wte=True, wpe=True, acc=False, pos0=5, mode='bound'):
    tag = f'B{B}_T{T}_C{C}_{ids}' + ('' if wte else '_nowte') + ('' if wpe else '_nowpe') + ('_acc' if acc else '') + f'_pos{pos0}' + \
        ('_int' if mode == 'exact' else '')
    return Case('embed_bwd', tag, dict(B=B, T=T, C=C, ids=ids, wte=wte, wpe=wpe, acc=acc, pos0=pos0), mode,
                {'same': 'every token the same id', 'mixed': 'mixed and clamped ids'}[ids])


EMBED_BWD = [_eb(3, 7, 100, 'same'), _eb(3, 7, 300, 'mixed', acc=True), _eb(1, 1, 4, 'mixed', pos0=0), _eb(3, 7, 4, 'mixed', wpe=False),
             _eb(3, 7, 100, 'mixed', wte=False, acc=True), _eb(3, 7, 100, 'mixed', wte=False), _eb(3, 7, 300, 'same', acc=True, mode='exact'),
             _eb(3, 7, 100, 'mixed', mode='exact'), _eb(3, 7, 4, 'mixed', acc=True, pos0=0, mode='exact')]


def embed_bwd_inputs(c, g):
    ids = torch.full((c.B, c.T), 4) if c.ids == 'same' else _ids(g, c.B, c.T)
    r = _ints if c.mode == 'exact' else _randn
    return {'ids': ids, 'dx': r(g, c.B * c.T, c.C), 'dwte0': r(g, VOCAB, c.C) if c.wte else None,
            'dwpe0': r(g, c.pos0 + c.T + 2, c.C) if c.wpe else None}


def embed_bwd_ref(c, i, mutant=None, dt=F64):
    ids, dx = i['ids'].view(-1).clamp(0, VOCAB - 1), i['dx'].to(dt)
    n = torch.arange(ids.numel())
    out = {}
    if c.wte:
        w = i['dwte0'].to(dt).clone()
        if mutant == 'overwrite':
            w[ids] = i['dwte0'].to(dt)[ids] + dx                             # the last token of an id wins
        else:
            for k in n.tolist():                                             # token order: the stand-in's order
                w[ids[k]] = w[ids[k]] + dx[k]
        out['dwte'] = w
    if c.wpe:
        s = torch.zeros(c.T, c.C, dtype=dt)
        where = _pos(n, c.T, 0, mutant if mutant == 'pos_div' else None)
        for k in n.tolist():                                                 # t fixed: b ascending
            if where[k] < c.T:
                s[where[k]] = s[where[k]] + dx[k]
        p = i['dwpe0'].to(dt).clone()
        p0 = 0 if mutant == 'pos0_ignored' else c.pos0
        p[p0:p0 + c.T] = p[p0:p0 + c.T] + s if c.acc and mutant != 'accumulate_ignored' else s
        out['dwpe'] = p
    return out


def embed_bwd_stand(c, i):
    return embed_bwd_ref(c, i, None, F32)


def embed_bwd_scale(c, i):
    ids, dx = i['ids'].view(-1).clamp(0, VOCAB - 1), i['dx'].double().abs()
    out = {}
    if c.wte:
        out['dwte'] = i['dwte0'].double().abs().index_add(0, ids, dx)
    if c.wpe:
        p = i['dwpe0'].double().abs().clone()                                # rows the launch leaves alone keep their bits: S only where it writes
        keep = torch.zeros_like(p)
        keep[c.pos0:c.pos0 + c.T] = (p[c.pos0:c.pos0 + c.T] if c.acc else 0) + dx.view(c.B, c.T, c.C).sum(0)
        out['dwpe'] = keep
    return out


# embed_bwd_ordered: the fp32 sum in token order, rows without a token 0: a device equals the stand-in bit for bit
def _eo(n, C, ids, mode='standin'):
    return Case('embed_ord', f'n{n}_C{C}_{ids}' + ('_int' if mode == 'exact' else ''), dict(n=n, C=C, ids=ids), mode,
                'vocab rows with no token are 0' + ('; a second block of columns' if C > 256 else ''))


EMBED_ORD = [_eo(21, 100, 'same'), _eo(21, 300, 'mixed'), _eo(1, 4, 'mixed'), _eo(21, 4, 'mixed'), _eo(21, 300, 'same', 'exact'),
             _eo(21, 100, 'mixed', 'exact')]


def embed_ord_inputs(c, g):
    ids = torch.full((c.n,), 4) if c.ids == 'same' else _ids(g, 1, c.n).view(-1)
    return {'ids': ids, 'dx': (_ints if c.mode == 'exact' else _randn)(g, c.n, c.C)}


def embed_ord_ref(c, i, mutant=None, dt=F64):
    ids, dx = i['ids'].clamp(0, VOCAB - 1), i['dx'].to(dt)
    w = torch.zeros(VOCAB, c.C, dtype=dt)
    for k in range(c.n):
        w[ids[k]] = dx[k] if mutant == 'overwrite' else w[ids[k]] + dx[k]
    return {'dwte': w}


def embed_ord_stand(c, i):
    return embed_ord_ref(c, i, None, F32)


def embed_ord_scale(c, i):
    return {'dwte': torch.zeros(VOCAB, c.C, dtype=F64).index_add(0, i['ids'].clamp(0, VOCAB - 1), i['dx'].double().abs())}


# ------------------------------------------------------------------------------------------------------------------------------
# the channels-last conv front-end (conv.hip).  col[(n, t'), cin ks + k] = x[n, t' stride + k - pad, cin]; col2im_cl its transpose, taps in
# ascending k; dwconv1d_cl y = bias + sum_k w[c, k] x[n, t' stride + k - pad, c] by fmaf in ascending k; its backward dx likewise, dw / db as
# min(rows, 64) chunk partials (fmaf in row order) met by colsum.  S = the same sums over absolute values.
# ------------------------------------------------------------------------------------------------------------------------------
def conv_out(T, ks, stride, pad):
    return (T + 2 * pad - ks) // stride + 1


def tap_frames(c, mutant=None):
    """frame [To, ks] read by tap k of window t', valid [To, ks]; ``right_pad_ignored`` lets a tap beyond T read on (into the next row)."""
    To = conv_out(c.T, c.ks, c.stride, c.pad)
    t = torch.arange(To)[:, None] * c.stride + torch.arange(c.ks)[None] - c.pad
    if mutant == 'taps_reversed':
        t = t.flip(1)
    return t, (t >= 0) & ((t < c.T) | (mutant == 'right_pad_ignored'))


def _unfold(c, x, mutant=None):
    """x [N, T, Cin] -> [N, To, Cin, ks] (zeros where invalid)."""
    N, T, Cin = x.shape
    t, ok = tap_frames(c, mutant)
    flat = x.reshape(N * T, Cin)
    idx = (torch.arange(N)[:, None, None] * T + t[None]) % (N * T)          # a tap let past T reads the next sample's frames
    return torch.where(ok[None, :, None, :], flat[idx].permute(0, 1, 3, 2), torch.zeros((), dtype=x.dtype))       # [N, To, Cin, ks]


def _fold(c, d, mutant=None):
    """d [N, To, Cin, ks] -> [N, T, Cin]: the transpose of _unfold; ``no_stride_test`` also adds tap k of window (t + pad - k) // stride
    where stride does not divide."""
    N, To, Cin, ks = d.shape
    out = torch.zeros(N, c.T, Cin, dtype=d.dtype)
    for t in range(c.T):
        for k in range(ks):                                                  # ascending k: the kernel's order
            kk = ks - 1 - k if mutant == 'taps_reversed' else k
            u = t + c.pad - k
            if u < 0 or (u % c.stride and mutant != 'no_stride_test') or u // c.stride >= To:
                continue
            out[:, t] = out[:, t] + d[:, u // c.stride, :, kk]
    return out


def _geo(ks, stride, pad, T, N, C):
    return dict(ks=ks, stride=stride, pad=pad, T=T, N=N, C=C), f'k{ks}_s{stride}_p{pad}_T{T}_N{N}_C{C}'


_GEOS = [(3, 2, 1, 1, 1, 3), (3, 2, 1, 2, 3, 1), (3, 2, 1, 7, 3, 80), (3, 2, 1, 8, 1, 3), (3, 1, 1, 5, 3, 3), (5, 4, 3, 43, 1, 80), (2, 3, 0, 11, 3, 3),
         (1, 1, 0, 4, 1, 1), (4, 2, 0, 9, 3, 80)]


def _unread(p):
    t, ok = tap_frames(Case('x', 'x', p))
    return sorted(set(range(p['T'])) - set(t[ok].tolist()))


def _conv_cases(launch, mode, ints=()):
    out = []
    for geo in _GEOS:
        p, tag = _geo(*geo)
        un = _unread(p)
        out.append(Case(launch, tag, p, mode, f'frames no window reads: {un}' if un else ''))
    for geo in ints:
        p, tag = _geo(*geo)
        out.append(Case(launch, tag + '_int', p, 'exact'))
    return out


IM2COL = _conv_cases('im2col', 'exact')
COL2IM = _conv_cases('col2im', 'bound', [(3, 2, 1, 7, 3, 80), (5, 4, 3, 43, 1, 3), (4, 2, 0, 9, 3, 3)])


def im2col_inputs(c, g):
    return {'x': _randn(g, c.N, c.T, c.C)}


def _cols(c, u, mutant=None):
    """[N, To, Cin, ks] -> the [N To, Cin ks] matrix (``kmajor``: column k Cin + cin)."""
    N, To, Cin, ks = u.shape
    return (u.permute(0, 1, 3, 2) if mutant == 'kmajor' else u).reshape(N * To, Cin * ks)


def _uncols(c, m, N, mutant=None):
    To = m.shape[0] // N
    return m.view(N, To, c.ks, c.C).permute(0, 1, 3, 2) if mutant == 'kmajor' else m.view(N, To, c.C, c.ks)


def im2col_ref(c, i, mutant=None, dt=F64):
    return {'col': _cols(c, _unfold(c, i['x'].to(dt), mutant), mutant)}


def im2col_stand(c, i):
    return im2col_ref(c, i, None, F32)


def im2col_unfold(c, x):
    """F.unfold's reading of the same matrix: what im2col_cl is held to bit for bit."""
    u = F.unfold(x.permute(0, 2, 1)[..., None], (c.ks, 1), padding=(c.pad, 0), stride=(c.stride, 1))         # [N, Cin ks, To]
    return u.transpose(1, 2).reshape(-1, c.C * c.ks)


def col2im_inputs(c, g):
    To = conv_out(c.T, c.ks, c.stride, c.pad)
    return {'dcol': (_ints if c.mode == 'exact' else _randn)(g, c.N * To, c.C * c.ks)}


def col2im_ref(c, i, mutant=None, dt=F64):
    fold_mutant = mutant if mutant in ('no_stride_test', 'taps_reversed') else None
    return {'dx': _fold(c, _uncols(c, i['dcol'].to(dt), c.N, mutant), fold_mutant)}


def col2im_stand(c, i):
    return col2im_ref(c, i, None, F32)


def col2im_scale(c, i):
    return {'dx': _fold(c, _uncols(c, i['dcol'].double().abs(), c.N))}


def _dw(ks, stride, pad, T, N, C, bias=True, want_dx=True, has_bias=True, mode='bound'):
    p, tag = _geo(ks, stride, pad, T, N, C)
    p.update(bias=bias, want_dx=want_dx, has_bias=has_bias)
    rows = N * conv_out(T, ks, stride, pad)
    chunks = min(rows, DW_CHUNKS)
    rpc = -(-rows // chunks)
    p.update(rows=rows, used=-(-rows // rpc), rpc=rpc)
    tag += ('' if bias else '_nobias') + ('' if want_dx else '_nodx') + ('' if has_bias else '_nodb') + ('_int' if mode == 'exact' else '')
    return p, tag, f'{rows} rows -> {p["used"]} chunks of {rpc}' + ('; second channel block' if C > 256 else '')


_DWS = [(8, 1, 0, 8, 1, 48), (3, 2, 1, 41, 3, 300), (1, 1, 0, 64, 1, 1), (3, 1, 1, 13, 5, 48), (8, 4, 3, 398, 2, 48), (3, 3, 0, 11, 1, 1),
        (8, 2, 0, 9, 3, 48), (3, 2, 1, 8, 1, 48)]
_DW_KW = [dict(), dict(bias=False, has_bias=False), dict(), dict(want_dx=False), dict(), dict(bias=False), dict(want_dx=False, has_bias=False), dict()]
_DW_INT = [(3, 2, 1, 41, 3, 300), (8, 4, 3, 398, 2, 48)]


def _dw_cases(launch):
    out = []
    for geo, kw in zip(_DWS, _DW_KW):
        p, tag, reach = _dw(*geo, **kw)
        out.append(Case(launch, tag, p, 'bound', reach))
    for geo in _DW_INT:
        p, tag, reach = _dw(*geo, mode='exact')
        out.append(Case(launch, tag, p, 'exact', reach))
    return out


DW_FWD, DW_BWD = _dw_cases('dw_fwd'), _dw_cases('dw_bwd')


def dw_inputs(c, g):
    r = _ints if c.mode == 'exact' else _randn
    To = conv_out(c.T, c.ks, c.stride, c.pad)
    return {'x': r(g, c.N, c.T, c.C), 'w': r(g, c.C, c.ks), 'b': r(g, c.C) if c.bias else None, 'dy': r(g, c.N, To, c.C)}


def dw_fwd_ref(c, i, mutant=None, dt=F64):
    u = _unfold(c, i['x'].to(dt), mutant)                                    # [N, To, C, ks]
    w = i['w'].to(dt)
    if dt == F64:
        y = (u * w).sum(-1)
    else:
        y = torch.zeros(u.shape[:3])
        for k in range(c.ks):
            y = fma32(w[:, k].expand_as(y), u[..., k], y)
    return {'y': y + i['b'].to(dt) if i['b'] is not None else y}


def dw_fwd_stand(c, i):
    return dw_fwd_ref(c, i, None, F32)


def dw_fwd_scale(c, i):
    S = (_unfold(c, i['x'].double().abs()) * i['w'].double().abs()).sum(-1)
    return {'y': S + i['b'].double().abs() if i['b'] is not None else S}


def dw_bwd_ref(c, i, mutant=None):
    dy, w = i['dy'].double(), i['w'].double()
    out = {}
    if c.want_dx:
        fold_mutant = mutant if mutant in ('no_stride_test', 'taps_reversed') else None
        out['dx'] = _fold(c, dy[..., None] * w, fold_mutant)
    u = _unfold(c, i['x'].double(), mutant if mutant in ('right_pad_ignored', 'taps_reversed') else None)
    out['dw'] = (dy[..., None] * u).sum((0, 1))
    if c.has_bias:
        out['db'] = dy.sum((0, 1))
    return out


def dw_bwd_stand(c, i):
    dy, w, x = i['dy'], i['w'], i['x']
    N, To, C = dy.shape
    out = {}
    if c.want_dx:
        dx = torch.zeros(N, c.T, C)
        for t in range(c.T):
            for k in range(c.ks):
                u = t + c.pad - k
                if u < 0 or u % c.stride or u // c.stride >= To:
                    continue
                dx[:, t] = fma32(w[:, k].expand(N, C), dy[:, u // c.stride], dx[:, t])
        out['dx'] = dx
    u = _unfold(c, x).reshape(N * To, C * c.ks)
    d = dy.reshape(N * To, C)
    pu, pd = _rows_view(u, (c.used, c.rpc)), _rows_view(d, (c.used, c.rpc))
    aw, ab = torch.zeros(c.used, C * c.ks), torch.zeros(c.used, C)
    for r in range(c.rpc):
        aw = fma32(pd[:, r].repeat_interleave(c.ks, 1), pu[:, r], aw)
        ab = ab + pd[:, r]
    out['dw'] = colsum32(aw).view(C, c.ks)
    if c.has_bias:
        out['db'] = colsum32(ab)
    return out


def dw_bwd_scale(c, i):
    dy, w = i['dy'].double().abs(), i['w'].double().abs()
    out = {}
    if c.want_dx:
        out['dx'] = _fold(c, dy[..., None] * w)
    out['dw'] = (dy[..., None] * _unfold(c, i['x'].double().abs())).sum((0, 1))
    if c.has_bias:
        out['db'] = dy.sum((0, 1))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------------
FAMILIES = {'ln_fwd': LN_FWD, 'ln_bwd': LN_BWD, 'ce': CE, 'lsm_fwd': LSM_FWD, 'lsm_bwd': LSM_BWD, 'colsum': COLSUM, 'gelu_fwd': GELU_FWD,
            'gelu_bwd': GELU_BWD, 'embed_fwd': EMBED_FWD, 'add_rows': ADD_ROWS, 'embed_bwd': EMBED_BWD, 'embed_ord': EMBED_ORD, 'im2col': IM2COL,
            'col2im': COL2IM, 'dw_fwd': DW_FWD, 'dw_bwd': DW_BWD}
ALL_CASES = [c for cases in FAMILIES.values() for c in cases]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

_FN = {'ln_fwd': (ln_fwd_inputs, ln_fwd_ref, ln_fwd_stand, ln_fwd_scale), 'ln_bwd': (ln_bwd_inputs, ln_bwd_ref, ln_bwd_stand, ln_bwd_scale),
       'ce': (ce_inputs, ce_ref, ce_stand, ce_scale), 'lsm_fwd': (lsm_fwd_inputs, lsm_fwd_ref, lsm_fwd_stand, lsm_fwd_scale),
       'lsm_bwd': (lsm_bwd_inputs, lsm_bwd_ref, lsm_bwd_stand, lsm_bwd_scale), 'colsum': (colsum_inputs, colsum_ref, colsum_stand, colsum_scale),
       'gelu_fwd': (gelu_inputs, gelu_fwd_ref, gelu_fwd_stand, gelu_fwd_scale), 'gelu_bwd': (gelu_inputs, gelu_bwd_ref, gelu_bwd_stand, gelu_bwd_scale),
       'embed_fwd': (embed_fwd_inputs, embed_fwd_ref, embed_fwd_stand, _exact_scale), 'add_rows': (add_rows_inputs, add_rows_ref, add_rows_stand, _exact_scale),
       'embed_bwd': (embed_bwd_inputs, embed_bwd_ref, embed_bwd_stand, embed_bwd_scale),
       'embed_ord': (embed_ord_inputs, embed_ord_ref, embed_ord_stand, embed_ord_scale),
       'im2col': (im2col_inputs, im2col_ref, im2col_stand, _exact_scale), 'col2im': (col2im_inputs, col2im_ref, col2im_stand, col2im_scale),
       'dw_fwd': (dw_inputs, dw_fwd_ref, dw_fwd_stand, dw_fwd_scale), 'dw_bwd': (dw_inputs, dw_bwd_ref, dw_bwd_stand, dw_bwd_scale)}


def _right_pad_reached(c):
    t, _ = tap_frames(c)
    return bool((t >= c.T).any())


def _off_stride_taps(c):
    """Whether some (t, k) has t + pad - k >= 0 off the stride grid with a window index below To: what the % stride test keeps out."""
    To = conv_out(c.T, c.ks, c.stride, c.pad)
    return any(u >= 0 and u % c.stride and u // c.stride < To for u in (t + c.pad - k for t in range(c.T) for k in range(c.ks)))


def _repeats(c):
    ids = make_inputs(c.name)['ids'].view(-1).clamp(0, VOCAB - 1)
    return len(ids.unique()) < ids.numel()


# launch -> mutant -> (what it is, the cases it can show on)
MUTANTS = {
    'ln_fwd': {'var_cm1': ('variance over C - 1', lambda c: c.C > 1),
               'eps_outside': ('eps outside the root', lambda c: c.C > 1 and c.dist == 'wide'),
               'tail_no_bias': ('last partial 64-column trip without bias', lambda c: c.bias and c.C % 64 != 0)},
    'ln_bwd': {'dres_dropped': ('dres not added', lambda c: c.dres),
               'proj_dropped': ('the xhat mean(g xhat) term dropped', lambda c: c.C > 1),
               'last_partial_dropped': ("the last workgroup's dw / db partial dropped", lambda c: True),
               'rows_ge_2048_skipped': ('rows >= 2048 skipped', lambda c: c.rows > 2048)},
    'ce': {'tail_ignored': ('columns >= V - V % 4 ignored', lambda c: c.V % 4 != 0),
           'wave_dropped': ("one wave's share of the columns dropped", lambda c: any(ce_wave(c, col) == 1 for col in range(c.V))),
           'ignored_not_zeroed': ("an ignored row's gradient not zeroed", lambda c: True),
           'target_off_by_one': ('target column off by one', lambda c: c.V > 1)},
    'lsm_fwd': {'tail_dropped': ('last partial trip dropped', lambda c: c.cols % 64 != 0)},
    'lsm_bwd': {'tail_dropped': ('last partial trip dropped', lambda c: c.cols % 64 != 0)},
    'colsum': {'rows_past_128_dropped': ('rows beyond the last whole 128 dropped', lambda c: c.rows % 128 != 0),
               'slice31_dropped': ('slice 31 dropped', lambda c: c.rows >= 32)},
    'gelu_fwd': {'kinds_swapped': ('kinds swapped', lambda c: True)},
    'gelu_bwd': {'kinds_swapped': ('kinds swapped', lambda c: True)},
    'embed_fwd': {'pos_div': ('position n / T', lambda c: c.wpe and c.B > 1), 'pos0_ignored': ('pos0 ignored', lambda c: c.wpe and c.pos0 > 0)},
    'add_rows': {'pos_div': ('position n / T', lambda c: c.rows > c.T)},
    'embed_bwd': {'pos_div': ('position n / T', lambda c: c.wpe and c.B > 1), 'pos0_ignored': ('pos0 ignored', lambda c: c.wpe and c.pos0 > 0),
                  'overwrite': ('repeated ids overwritten instead of added', lambda c: c.wte and _repeats(c)),
                  'accumulate_ignored': ('accumulate_wpe ignored', lambda c: c.wpe and c.acc)},
    'embed_ord': {'overwrite': ('repeated ids overwritten instead of added', _repeats)},
    'im2col': {'right_pad_ignored': ('right padding ignored', _right_pad_reached), 'taps_reversed': ('kernel taps reversed', lambda c: c.ks > 1 and c.T > 1),
               'kmajor': ('column index k Cin + cin', lambda c: c.ks > 1 and c.C > 1)},
    'col2im': {'no_stride_test': ('without the % stride test', _off_stride_taps),
               'taps_reversed': ('kernel taps reversed', lambda c: c.ks > 1 and c.T > 1),
               'kmajor': ('column index k Cin + cin', lambda c: c.ks > 1 and c.C > 1)},
    'dw_fwd': {'right_pad_ignored': ('right padding ignored', _right_pad_reached), 'taps_reversed': ('kernel taps reversed', lambda c: c.ks > 1 and c.T > 1)},
    'dw_bwd': {'right_pad_ignored': ('right padding ignored', _right_pad_reached),
               'no_stride_test': ('dx without the % stride test', lambda c: c.want_dx and _off_stride_taps(c)),
               'taps_reversed': ('kernel taps reversed', lambda c: c.ks > 1 and c.T > 1)},
}


# listed for the cases on which they show; elsewhere they change the value by less than a bound (eps outside the root where sqrt(var) = 0.5:
# d sqrt(v + eps) / d eps = 1 there, so eps inside or outside the root is the same to first order)
NUMERIC_ONLY = {('ln_fwd', 'eps_outside')}


def mutant_applies(mutant, c):
    return bool(MUTANTS[c.launch][mutant][1](c))


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """CPU tensors of a case (seeded by its name)."""
    c = BY_NAME[name]
    return _FN[c.launch][0](c, _gen(name))


def _with(c, over):
    i = make_inputs(c.name)
    return {**i, **over} if over else i


def reference(c, mutant=None, **over):
    """float64, output name -> tensor.  ``over`` replaces inputs (lsm_bwd: y = the device's own)."""
    return _FN[c.launch][1](c, _with(c, over), mutant)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return reference(BY_NAME[name])


def stand_in(c, **over):
    return _FN[c.launch][2](c, _with(c, over))


@functools.lru_cache(maxsize=None)
def _stand_in(name):
    return stand_in(BY_NAME[name])


def scale(c, **over):
    return _FN[c.launch][3](c, _with(c, over))


# ------------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, allow):
    """|got - ref| / allow per element: inf where nothing is allowed and something differs, where the reference is not finite and the value
    is another, and where the value is NaN."""
    got, ref = got.to(F64), ref.to(F64)
    fin = torch.isfinite(ref)
    err = (got - ref).abs()
    inf, zero = torch.full_like(err, float('inf')), torch.zeros_like(err)
    q = torch.where(allow > 0, err / allow.clamp_min(1e-300), torch.where(err > 0, inf, zero))
    q = torch.where(fin, q, torch.where(got == ref, zero, inf))
    return torch.where(torch.isnan(q), inf, q)


def deviation(got, ref, S):
    """max |got - ref| / S over every element."""
    return _ratio(got, ref, S.expand_as(ref)).max().item() if ref.numel() else 0.0


def excess(got, ref, S, bound):
    """max |got - ref| / (bound S) (<= 1: inside)."""
    return _ratio(got, ref, bound * S.expand_as(ref)).max().item() if ref.numel() else 0.0


def first_outside(got, ref, S, bound):
    idx = torch.nonzero(_ratio(got, ref, bound * S.expand_as(ref)) > 1)
    if not len(idx):
        return None
    k = tuple(idx[0].tolist())
    return k, got[k].item(), ref[k].item()


def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def bounds_of(st, ref, S):
    """output -> (the stand-in's deviation, max(FACTOR x it, FLOOR))."""
    out = {}
    for k in ref:
        n = deviation(st[k], ref[k], S[k])
        out[k] = (n, max(FACTOR * n, FLOOR))
    return out


@functools.lru_cache(maxsize=None)
def _bounds(name):
    c = BY_NAME[name]
    return bounds_of(_stand_in(name), _reference(name), scale(c))


def bounds(c):
    """output -> (the stand-in's own deviation from the float64 reference, what a device is held to), in units of S."""
    return _bounds(c.name)


def noise(c):
    """output -> the stand-in's own deviation from the float64 reference."""
    return {k: v[0] for k, v in _bounds(c.name).items()}


def bound(c):
    """output -> what a device is held to, in units of S."""
    return {k: v[1] for k, v in _bounds(c.name).items()}
