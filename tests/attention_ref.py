"""Float64 restatement of the tiled attention operators (ops.attention_fwd / attention_bwd and their bf16 twins) on the packed row
layouts the ops take, with the dropout multipliers as an explicit input, plus what tests/test_gpu_attention_ref.py and
tests/test_attention_ref_cpu.py share: the case tables, the gates, the peaked inputs and a float64 emulation of the kernels' softmax
re-reference rule.  CPU only, no HIP.

Layouts: q rows [N * Tq, heads * hd], k / v rows [N * Tk, heads * hd] (head h at columns hd * h ..), lse [N, heads, Tq], the dropout
multipliers [N, heads, Tq, Tk] (0 where dropped, 1 / (1 - p) where kept)."""
import math

import numpy as np
import torch

from oracle import philox

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
TILE = 64               # keys per tile of every tiled kernel (attn.hip, attn_mx.hip, attn_b16.hip)
BLOCK = 16              # queries per MFMA block: the unit that decides to move the softmax reference
REBASE = 8.0            # log2 units (attn_mx.hip, attn_b16.hip)


def _t64(x):
    return (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).detach().cpu().double()


def split_heads(x, N, T, heads, hd):
    """rows [N * T, heads * hd] -> [N, heads, T, hd]"""
    return x.reshape(N, T, heads, hd).permute(0, 2, 1, 3)


def merge_heads(x):
    """[N, heads, T, hd] -> rows [N * T, heads * hd]"""
    N, H, T, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(N * T, H * hd)


def visible(N, Tq, Tk, causal, lens):
    """bool [N, 1, Tq, Tk]: key j is visible to query i of batch n.  The causal mask is tril(Tk - Tq), the kernels' coff."""
    vis = torch.ones(N, 1, Tq, Tk, dtype=torch.bool)
    if causal:
        vis &= torch.ones(Tq, Tk, dtype=torch.bool).tril(Tk - Tq)
    if lens is not None:
        ln = torch.as_tensor(np.asarray(lens, dtype=np.int64))
        vis &= (torch.arange(Tk)[None, :] < ln[:, None])[:, None, None, :]
    return vis


def _attention(q, k, v, N, heads, hd, Tq, Tk, causal, lens, mult, log2_units):
    qh, kh, vh = split_heads(q, N, Tq, heads, hd), split_heads(k, N, Tk, heads, hd), split_heads(v, N, Tk, heads, hd)
    s = (qh @ kh.transpose(-1, -2)) * (LN2 if log2_units else 1.0 / math.sqrt(hd))        # nats
    s = s.masked_fill(~visible(N, Tq, Tk, causal, lens), float('-inf'))
    lse = torch.logsumexp(s, -1)                                  # over the undropped scores
    p = torch.exp(s - lse[..., None])                             # the normaliser keeps the undropped sum
    if mult is not None:
        p = p * _t64(mult)                                        # the multipliers act after the softmax
    return merge_heads(p @ vh), lse


def attention_ref(q, k, v, N, heads, hd, Tq, Tk, causal, lens, mult=None, log2_units=False):
    """-> (y rows [N * Tq, heads * hd], lse [N, heads, Tq] in nats), float64.  log2_units: q already carries 1 / sqrt(hd) and log2(e)
    (round_like_bf16_mode), the scores are base-2 exponents."""
    with torch.no_grad():
        return _attention(_t64(q), _t64(k), _t64(v), N, heads, hd, Tq, Tk, causal, lens, mult, log2_units)


def attention_grads_ref(q, k, v, N, heads, hd, Tq, Tk, causal, lens, dy, mult=None, log2_units=False):
    """-> (dq, dk, dv) of sum(y * dy) by float64 autograd, the multipliers held constant.  With log2_units, dq is the gradient with
    respect to the UNSCALED q (times 1 / sqrt(hd) * log2(e)), which is what the kernels return."""
    q, k, v = (_t64(t).clone().requires_grad_(True) for t in (q, k, v))
    y, _ = _attention(q, k, v, N, heads, hd, Tq, Tk, causal, lens, mult, log2_units)
    y.backward(_t64(dy))
    dq = q.grad * (LOG2E / math.sqrt(hd)) if log2_units else q.grad
    return dq, k.grad, v.grad


def drop_mult(N, heads, Tq, Tk, p, seed, stream_id, offset):
    """The multipliers the kernels draw (oracle.philox restates csrc/attn_args.h).  A device step counter adds to `offset`."""
    return philox.attention_dropout_mask(N, heads, Tq, Tk, p, seed, stream_id, offset)


WRONG_MASKS = ('tile+1', 'floor_tiles', 'stream+1')


def drop_mult_variant(kind, N, heads, Tq, Tk, p, seed, stream_id, offset, batches=None):
    """The multipliers under a deliberately wrong index ('right': the true one, for checking this function against drop_mult):
    'tile+1' the key-tile number shifted by one, 'floor_tiles' Tk // 64 tiles per row instead of ceil(Tk / 64), 'stream+1' the next
    stream.  batches: only these batch entries (the index of an element does not depend on which others are asked for)."""
    assert kind in WRONG_MASKS + ('right',)
    KT = Tk // TILE if kind == 'floor_tiles' else (Tk + TILE - 1) // TILE
    n = np.arange(N)[batches if batches is not None else slice(None)].astype(np.int64)
    j = np.arange(Tk, dtype=np.int64)
    row = (n[:, None, None] * heads + np.arange(heads, dtype=np.int64)[None, :, None]) * Tq + np.arange(Tq, dtype=np.int64)[None, None, :]
    kt = j // TILE + (1 if kind == 'tile+1' else 0)
    e = (row[..., None] * KT + kt) * TILE + 4 * (j % 16) + (j % TILE) // 16
    # philox.dropout_mask at the elements asked for only
    g = (e >> 2).astype(np.uint64)
    r = philox.philox4x32_10((g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                             np.full(e.shape, stream_id + (1 if kind == 'stream+1' else 0), dtype=np.uint32), np.full(e.shape, offset, dtype=np.uint32),
                             seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    keep = np.choose(e & 3, r) >= philox.dropout_threshold(p)
    return np.where(keep, philox.dropout_scale(p), np.float32(0.0)).astype(np.float32)


def round_like_bf16_mode(q, k, v, hd):
    """The operands as the single-pass (bf16 mode, attn_b16) forward and dQ sweep see them: q times float32(1 / sqrtf(hd)) * float32(log2 e)
    (one float32 constant, as the kernels form it) rounded to bf16, k and v rounded to bf16.  Scores of these are in log2 units."""
    c = np.float32(1.0) / np.sqrt(np.float32(hd)) * np.float32(LOG2E)
    assert c.dtype == np.float32
    q = torch.as_tensor(q).detach().cpu().float()
    return ((q * float(c)).bfloat16().double(), torch.as_tensor(k).detach().cpu().float().bfloat16().double(),
            torch.as_tensor(v).detach().cpu().float().bfloat16().double())


PEAKED_KINDS = ('ramp', 'spike', 'descend')


def peaked_inputs(kind, N, heads, Tq, Tk, hd, seed):
    """float32 rows q, k, v: randn plus a rank-one term along u (unit vector on the even dimensions), a = 3 hd^(1/4):
    q_i += a s_i u, k_j += a c_j u.  'ramp': s_i = (-1)^i, c_j = floor(j / 64); 'spike': s_i = (-1)^i, c = 0 but c[Tk - 3] = 3 and
    c[70] = 2; 'descend': s_i = 1, c_j = -floor(j / 64); 'randn' is the baseline (q, k untouched).  The scores gain 3^2 s_i c_j nats.
    ramp / spike: half the queries of every 16-query block climb past REBASE from tile to tile while the other half fall.  descend:
    every query falls 9 nats per tile -- no block re-references, the later tiles underflow against the first.  (With the alternating
    sign a descent is a ramp for the odd queries: s_i = 1 is what makes it a descent for all of them.)"""
    assert kind in PEAKED_KINDS + ('randn',)
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    q, k, v = torch.randn(N * Tq, C, generator=g), torch.randn(N * Tk, C, generator=g), torch.randn(N * Tk, C, generator=g)
    if kind == 'randn':
        return q, k, v
    u = torch.zeros(hd)
    u[0::2] = 1.0 / math.sqrt(hd // 2)
    a = 3.0 * hd ** 0.25
    j = torch.arange(Tk)
    if kind == 'ramp':
        c = (j // TILE).float()
    elif kind == 'descend':
        c = -(j // TILE).float()
    else:
        c = torch.zeros(Tk)
        c[Tk - 3], c[70] = 3.0, 2.0
    sign = torch.ones(Tq) if kind == 'descend' else 1.0 - 2.0 * (torch.arange(Tq) % 2).float()
    q = (q.view(N, Tq, heads, hd) + a * sign[None, :, None, None] * u).reshape(N * Tq, C)
    k = (k.view(N, Tk, heads, hd) + a * c[None, :, None, None] * u).reshape(N * Tk, C)
    return q.contiguous(), k.contiguous(), v


def _shape_of(q, k, hd, lens, N):
    N = len(lens) if lens is not None else N
    assert N, 'without key lengths the batch size has to be given'
    return N, q.shape[1] // hd, q.shape[0] // N, k.shape[0] // N


def later_rebase_blocks(q, k, hd, causal, lens, N=None):
    """The kernels' re-reference rule in float64, scores in log2 units: a 16-query block moves its references on a 64-key tile when any
    of its queries meets its first finite maximum or a maximum more than REBASE above its reference; every query of the block then
    moves up to its maximum (never down).  -> (blocks that re-reference after their first tile, blocks)."""
    N, heads, Tq, Tk = _shape_of(q, k, hd, lens, N)
    qh, kh = split_heads(_t64(q), N, Tq, heads, hd), split_heads(_t64(k), N, Tk, heads, hd)
    s = (qh @ kh.transpose(-1, -2)) * (LOG2E / math.sqrt(hd))
    s = s.masked_fill(~visible(N, Tq, Tk, causal, lens), float('-inf')).numpy()
    later = total = 0
    for n in range(N):
        for h in range(heads):
            for q0 in range(0, Tq, BLOCK):
                blk = s[n, h, q0:q0 + BLOCK]
                mref = np.full(blk.shape[0], -np.inf)
                moved = 0
                for kt in range((Tk + TILE - 1) // TILE):
                    mx = blk[:, kt * TILE:(kt + 1) * TILE].max(axis=1)
                    fresh = np.isinf(mref)
                    with np.errstate(invalid='ignore'):
                        rel = np.where(fresh, mx, mx - mref)
                    if np.any((fresh & (mx > -np.inf)) | (~fresh & (rel > REBASE))):
                        mref = np.where(fresh, mx, mref + np.maximum(rel, 0.0))
                        moved += 1
                assert moved >= 1
                later += moved > 1
                total += 1
    return later, total


def score_magnitude(q, k, hd, causal, lens, N=None):
    """A = max over visible (i, j) of scale * sum_d |q_id k_jd|: the quantity the rounding error of a score grows with."""
    N, heads, Tq, Tk = _shape_of(q, k, hd, lens, N)
    qh, kh = split_heads(_t64(q), N, Tq, heads, hd).abs(), split_heads(_t64(k), N, Tk, heads, hd).abs()
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(hd)
    return float(s.masked_fill(~visible(N, Tq, Tk, causal, lens), 0.0).max())


# ---------------------------------------------------------------------------------------------------- the GPU file's cases and gates
MODES = ('f32', 'bf16x3', 'bf16')
# the project's gates for unit-scale randn operands (test_attention_fwd_against_sdpa, test_attention_bwd_against_autograd)
FWD_ATOL = {'f32': 3e-6, 'bf16x3': 3e-5}
FWD_RTOL = 1e-5
BWD_ATOL = {'f32': 2e-5, 'bf16x3': 1e-4, 'bf16': 1e-1}
BWD_RTOL = 1e-4
LSE_RTOL = 1e-6

# the backward's forced dispatch forms per mode: (HALO_ATTN_BWD_QB, HALO_ATTN_DKV_LF); None leaves the variable unset
BWD_FORMS = {'f32': [(None, None)],
             'bf16x3': [(None, '0'), (None, '1')],
             'bf16': [('1', '0'), ('1', '1'), ('2', '0'), ('2', '1')]}

SEED = (0x5DEECE66 << 32) | 0x1234ABCD          # both 32-bit halves non-zero
STREAM_ID, OFFSET = 7, 11

# B: (hd, heads, N, Tq, Tk, causal, key lengths)
DROPOUT_CASES = [
    (64, 2, 2, 150, 150, True, None),
    (64, 2, 3, 70, 150, False, (150, 64, 5)),
    (32, 3, 2, 200, 200, True, (200, 131)),              # four tiles: an even pairing of the causal sweeps
    (16, 2, 2, 9, 130, False, (130, 77)),                # head dimension 16: the exact-f32 kernels in every mode
    (64, 1, 2, 129, 129, False, None),                   # one row into a third query tile
]
DROPOUT_PS = (0.1, 0.2)
BIG_CASE = (32, 9, 19, 257, 257, True, None)             # bf16, default dispatch: the two-query-block forward and dQ sweep
BIG_P = 0.1

# C: (kind, hd, Tq, Tk, causal, key lengths) at N = 2, heads = 2
PEAKED_N, PEAKED_HEADS, PEAKED_SEED = 2, 2, 5
PEAKED_CASES = [(kind, hd, 150, 150, causal, None) for kind in PEAKED_KINDS for hd in (64, 32) for causal in (False, True)] + \
               [('ramp', hd, 70, 150, False, (150, 70)) for hd in (64, 32)]


def kernel_class(mode, hd):
    """Which arithmetic a mode runs at a head dimension: 16 is always the exact-f32 kernels of attn.hip."""
    return 'f32' if hd == 16 else mode


def fwd_gate(mode, hd, p, vmax):
    """(atol, rtol) of y against the reference (bf16: the reference on round_like_bf16_mode operands).  f32 / bf16x3: the project's
    gate times 1 / (1 - p), the factor the kept probabilities carry.  bf16: the probabilities are rounded to bf16, 2^-9 each, and
    sum_j p_ij m_ij |v_j| <= max|v| / (1 - p); a factor two of margin."""
    cls = kernel_class(mode, hd)
    if cls == 'bf16':
        return 2.0 ** -8 * vmax / (1.0 - p), 0.0
    return FWD_ATOL[cls] / (1.0 - p), FWD_RTOL


def lse_gate(mode, hd):
    """(atol, rtol) of lse, which dropout does not touch: the project's 4 max(tol, 1e-5).  bf16 against the rounded-operand reference:
    products of bf16 operands are exact in fp32, what is left is the fp32 accumulation that the exact-f32 kernels have as well --
    the f32 gate."""
    cls = kernel_class(mode, hd)
    return 4 * max(FWD_ATOL['f32' if cls == 'bf16' else cls], 1e-5), LSE_RTOL


def bwd_gate(mode, hd, p):
    cls = kernel_class(mode, hd)
    return BWD_ATOL[cls] / (1.0 - p), BWD_RTOL


def exceeds(got, ref, atol, rtol):
    """True when np.testing.assert_allclose(got, ref, atol, rtol) would fail."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool((np.abs(got - ref) > atol + rtol * np.abs(ref)).any())


def case_inputs(hd, heads, N, Tq, Tk, seed=None):
    """Unit-scale randn rows q, k, v, dy (float32) of a dropout case."""
    g = torch.Generator().manual_seed(hd + 3 * Tq + Tk + 1000 * N if seed is None else seed)
    C = heads * hd
    return (torch.randn(N * Tq, C, generator=g), torch.randn(N * Tk, C, generator=g), torch.randn(N * Tk, C, generator=g),
            torch.randn(N * Tq, C, generator=g))


def reference_operands(mode, hd, q, k, v, dy):
    """(q, k, v, dy, log2_units) the reference of a mode reads: bf16 mode sees rounded operands."""
    if kernel_class(mode, hd) == 'bf16':
        qr, kr, vr = round_like_bf16_mode(q, k, v, hd)
        return qr, kr, vr, dy.bfloat16().double(), True
    return q, k, v, dy, False


# ---------------------------------------------------------------------------------------------------- mask probes (head dimension 64)
# With q = 0 every visible key of query i has probability u_i = 1 / visible_i, and one-hot operands make single multipliers come out
# as single output elements.  Each builder returns float32 rows; each decoder returns the multipliers [N, heads, Tq, Tk] it can see
# (NaN elsewhere), thresholded at half the kept value.
PROBE_HD = 64
PROBE_P = 0.2
PROBE_CASES = [(2, 2, 150, 150, True, None), (3, 2, 70, 150, False, (150, 64, 5))]      # (N, heads, Tq, Tk, causal, key lengths)


def _onehot_rows(N, T, heads, tile):
    """rows [N * T, heads * 64]: row r of the tile is e_{r mod 64} in every head, rows outside the tile are zero."""
    x = torch.zeros(N, T, heads, PROBE_HD)
    r = torch.arange(tile * TILE, min(T, (tile + 1) * TILE))
    x[:, r, :, r % TILE] = 1.0
    return x.reshape(N * T, heads * PROBE_HD)


def _e0_rows(N, T, heads):
    x = torch.zeros(N, T, heads, PROBE_HD)
    x[..., 0] = 1.0
    return x.reshape(N * T, heads * PROBE_HD)


def probe_inputs(which, N, heads, Tq, Tk, tile):
    """(q, k, v, dy) of one probe launch.  'fwd': v one-hot on key tile `tile`; 'dq': dy_i = e_0, v_j = e_0, k one-hot on key tile
    `tile`; 'dkv': dy one-hot on QUERY tile `tile`."""
    C = heads * PROBE_HD
    q, k, v, dy = torch.zeros(N * Tq, C), torch.zeros(N * Tk, C), torch.zeros(N * Tk, C), torch.zeros(N * Tq, C)
    if which == 'fwd':
        v = _onehot_rows(N, Tk, heads, tile)
    elif which == 'dq':
        dy, v, k = _e0_rows(N, Tq, heads), _e0_rows(N, Tk, heads), _onehot_rows(N, Tk, heads, tile)
    else:
        assert which == 'dkv'
        dy = _onehot_rows(N, Tq, heads, tile)
    return q, k, v, dy


def _threshold(x, p):
    kept = np.float32(philox.dropout_scale(p))
    return np.where(x > 0.5 * float(kept), kept, np.float32(0.0)).astype(np.float32)


def probe_decode(which, out, y, N, heads, Tq, Tk, causal, lens, p, tile, est):
    """Writes the multipliers that launch `tile` of probe `which` exposes into est [N, heads, Tq, Tk].  out: y ('fwd'), dq ('dq') or
    dv ('dkv') of the launch; y: the forward output of the same launch (the dQ sweep's delta_i = dy_i . y_i = y[i, 0])."""
    u = 1.0 / visible(N, Tq, Tk, causal, lens).sum(-1, keepdim=True).double().numpy()            # [N, 1, Tq, 1]
    lo = tile * TILE
    if which == 'fwd':            # y[i, d] = u_i mult[i, 64 t + d]
        hi = min(Tk, lo + TILE)
        val = split_heads(_t64(out), N, Tq, heads, PROBE_HD).numpy()[..., :hi - lo] / u
        est[:, :, :, lo:hi] = _threshold(val, p)
    elif which == 'dq':           # dq[i, d] = scale u_i (mult[i, 64 t + d] - delta_i)
        hi = min(Tk, lo + TILE)
        delta = split_heads(_t64(y), N, Tq, heads, PROBE_HD).numpy()[..., :1]
        val = split_heads(_t64(out), N, Tq, heads, PROBE_HD).numpy()[..., :hi - lo] * math.sqrt(PROBE_HD) / u + delta
        est[:, :, :, lo:hi] = _threshold(val, p)
    else:                         # dv[j, d] = u_{64 t' + d} mult[64 t' + d, j]
        hi = min(Tq, lo + TILE)
        val = split_heads(_t64(out), N, Tk, heads, PROBE_HD).numpy()[..., :hi - lo].transpose(0, 1, 3, 2) / u[:, :, lo:hi]
        est[:, :, lo:hi, :] = _threshold(val, p)


def probe_tiles(which, Tq, Tk):
    return range(((Tq if which == 'dkv' else Tk) + TILE - 1) // TILE)


TILED_BUGS = ('o', 'lsum', 'mref')


def tiled_forward_emulation(q, k, v, hd, causal, lens, N=None, bug=None):
    """The forward of attn_mx.hip / attn_b16.hip tile by tile in float64: scores in log2 units relative to a per-query reference that a
    16-query block moves by the rule of later_rebase_blocks, the output and the normaliser rescaled only then.  -> (y rows, lse).
    bug: what a broken re-reference would do -- 'o' / 'lsum' leaves the output / the normaliser unscaled, 'mref' shifts the tile's
    scores but keeps the old reference for the tiles behind it.  Without a bug this is attention_ref up to float64 rounding."""
    assert bug is None or bug in TILED_BUGS
    N, heads, Tq, Tk = _shape_of(q, k, hd, lens, N)
    qh, kh = split_heads(_t64(q), N, Tq, heads, hd), split_heads(_t64(k), N, Tk, heads, hd)
    vh = split_heads(_t64(v), N, Tk, heads, hd).numpy()
    s = (qh @ kh.transpose(-1, -2)) * (LOG2E / math.sqrt(hd))
    s = s.masked_fill(~visible(N, Tq, Tk, causal, lens), float('-inf')).numpy()
    y, lse = np.zeros((N, heads, Tq, hd)), np.zeros((N, heads, Tq))
    for n in range(N):
        for h in range(heads):
            for q0 in range(0, Tq, BLOCK):
                blk = s[n, h, q0:q0 + BLOCK]
                rows = blk.shape[0]
                mref, lsum, o = np.full(rows, -np.inf), np.zeros(rows), np.zeros((rows, hd))
                for kt in range((Tk + TILE - 1) // TILE):
                    fresh = np.isinf(mref)
                    rel = blk[:, kt * TILE:(kt + 1) * TILE] - np.where(fresh, 0.0, mref)[:, None]
                    mx = rel.max(axis=1)
                    if np.any((fresh & (mx > -np.inf)) | (mx > REBASE)):
                        shift = np.where(fresh, np.where(np.isinf(mx), 0.0, mx), np.maximum(mx, 0.0))
                        alpha = np.exp2(-shift)
                        if bug != 'lsum':
                            lsum = np.where(fresh, lsum, lsum * alpha)
                        if bug != 'o':
                            o = np.where(fresh[:, None], o, o * alpha[:, None])
                        rel = rel - shift[:, None]
                        moved = np.where(fresh, np.where(np.isinf(mx), -np.inf, mx), mref + shift)
                        mref = np.where(fresh, moved, mref) if bug == 'mref' else moved
                    p = np.exp2(rel)
                    lsum = lsum + p.sum(axis=1)
                    o = o + p @ vh[n, h, kt * TILE:(kt + 1) * TILE]
                y[n, h, q0:q0 + BLOCK] = o / lsum[:, None]
                lse[n, h, q0:q0 + BLOCK] = mref * LN2 + np.log(lsum)
    return merge_heads(torch.from_numpy(y)), torch.from_numpy(lse)
