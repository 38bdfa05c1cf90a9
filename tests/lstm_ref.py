"""Yardstick of the LSTM launches (haloop_amd.ops.lstm_fwd / lstm_bwd; csrc/lstm.hip, lstm_persist*.hip): the recurrence in a chosen
precision under the kernels' OWN operand rounding.  Shared by tests/test_lstm_ref_cpu.py and tests/test_gpu_lstm_f64.py; holds no tests.
CPU only (torch on the host + oracle/philox).

The contract of a math mode is exact: operands of a product rounded as the table below says, fp32 sums, fp32 state.  Two readings:

``free_running(inp, mode, dtype)``      the whole forward + backward on its own state.  dtype=float64, mode='f32' is plain float64
                                        nn.LSTM (tests/test_lstm_ref_cpu.py ties it to torch's).  dtype=float32 is the STAND-IN for a
                                        device: every intermediate in float32, the kernels' activation forms (``act``).
``teacher_forced(inp, state, mode)``    float64, but every step takes the DEVICE's own operands (h_{t-1}, the layer input, dG_{t+1},
                                        the layer above's dG_t) from ``state``: a bf16 rounding flip of the device's state then
                                        cannot propagate into the reference, and what is left between the two is fp32 rounding of
                                        one step.  By induction over t and the layers the per-step gates still pin every output.

Product model, restated from the code (line numbers: csrc/ at the commit that added this file).  rb = round-to-nearest-even to bf16
(``(__bf16)x``: Packed<>::store lstm.hip:51, split8 dev_util.h:20, lstm_persist2.hip:197/555, tiled_image.h);
'bf16' = rb(a) rb(b); 'x3' = hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b), hi = rb(a), lo = rb(a - hi) (mma_chunk3 lstm.hip:104-113,
lstm_persist.hip:120-124, gemm_bf16x3.hip:290); 'exact' = fp32 operands (v_mfma_f32_16x16x4_f32: lstm.hip:78, gemm_f32.hip).
M = the mode's kind: f32 -> exact, bf16 -> bf16, bf16x3 -> x3.

  product                                 operands                      kind                                      source
  --------------------------------------  ----------------------------  ----------------------------------------  ---------------------------
  input projection, layer l               in_t, W_ih                    M if in_dim >= 64 else exact              lstm.hip:1626-1634, 1347-1351
  recurrent h_{t-1} W_hh^T                h_{t-1}, W_hh                 M if H % 32 == 0 else exact               use_x3 lstm.hip:942, 984
  layer 1's projection inside persist2    h0_t or dropout(h0_t), W_ih1  bf16 (H >= 256: the rule above)           lstm_persist2.hip:197-203, 339
  dG_{t+1} W_hh (backward recurrence)     dG_{t+1}, W_hh                as the recurrent product                  lstm.hip:999, persist.hip:277
  inter-layer gradient dG^{l}_t W_ih^{l}  dG_t, W_ih                    M if in_dim >= 64 (= H) else exact,       ``tiled`` lstm.hip:1275, 1295-1300;
    (then * mask / (1 - p) of layer l-1)                                  bf16 inside persist2                      lstm_persist2.hip:521-537
  dx = dG^0 W_ih^0                        dG, W_ih                      M if in0 >= 64 else exact                 lstm.hip:1275, 1295-1300
  dW_ih = dG^T in,  dW_hh = dG^T h_prev   dG, in / h_{t-1}              M if in_dim >= 64 else exact (BOTH: a      lstm.hip:1275, 1304-1325
                                                                          narrow layer's dW_hh is exact too)
  db_ih = db_hh = sum_t,b dG              --                            fp32 sums of the fp32 dG                  lstm.hip:1327, persist.hip:322
  layer-diagonal schedule (fusion on)     recurrent, layers >= 1's      x3 in BOTH non-f32 modes                  packed_dot<true> lstm.hip:742,
                                          projection, inter-layer grad    (the diag kernels never run one pass)      754, 848

Sums are float64 in the reference and float32 (torch's order) in the stand-in.  Dropout: ydrop = h * m, m = 0 or float32(1)/(1-p) from
oracle/philox.dropout_mask on stream HALO_STREAM_LSTM_LAYER0 + l, element (t, b, j) of the time-major [T, B, H] output
(lstm.hip:1654, 1687; lstm_persist2.hip:108, 249).  The backward takes c_t, c_{t-1} and the activated gates the forward saved
(lstm.hip:394-396); tanh(c_t) is recomputed."""
import functools
from dataclasses import dataclass

import torch

from oracle import philox

STREAM_LSTM_LAYER0 = 16            # include/halo.h HALO_STREAM_LSTM_LAYER0 (haloop_amd/_lib.py:27)
SEED, OFFSET = 1234, 3             # the dropout stream of every case

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    group: str                     # step | persist | persist32 | persist2 | persist2x | l3 | fused | split
    T: int
    B: int
    in0: int
    H: int
    L: int
    p: float = 0.0
    state: bool = False            # h0 / c0 given, dhn / dcn flow back
    y_relu: bool = False           # ... and y written batch-first through y_strides
    modes: tuple = ('bf16',)
    persistent2: bool = True       # _lib.set_lstm_persistent2
    interleave: bool = True        # _lib.set_lstm_interleave
    fusion: bool = False           # _lib.set_lstm_fusion
    fwd_kernel: str = ''           # what lstm_chain_info must name
    bwd_kernel: str = ''
    act: str = 'fast'              # the kernels' activation forms: 'fast' (exp2 + rcp, lstm_persist_dev.h:90-114) | 'libm' (expf / tanhf)


ALL3 = ('f32', 'bf16x3', 'bf16')
STEP = dict(group='step', modes=ALL3, fwd_kernel='lstm_step_fwd_kernel', bwd_kernel='lstm_step_bwd_kernel', act='libm')
PERS = dict(group='persist', persistent2=False, fwd_kernel='lstm_persist_fwd_kernel', bwd_kernel='lstm_persist_bwd_kernel')
P2 = dict(group='persist2', fwd_kernel='lstm_persist2_fwd_kernel', bwd_kernel='lstm_persist2_bwd_kernel')

CASES = [
    # ---- step chain (not persistent-eligible) ----
    Case('step_h48_state', T=5, B=3, in0=24, H=48, L=2, state=True, **STEP),               # H % 16 only: exact recurrence in every mode
    Case('step_h96_drop', T=6, B=17, in0=40, H=96, L=2, p=0.25, **STEP),                   # in < 64 (exact projection), ragged 2nd batch tile
    Case('step_h160_k72', T=4, B=16, in0=72, H=160, L=1, y_relu=True, **STEP),             # in >= 64, K no multiple of 32
    # ---- one persistent launch per layer ----
    Case('persist_h256_state', T=7, B=5, in0=40, H=256, L=2, state=True, modes=('bf16x3', 'bf16'), **PERS),
    Case('persist_h512_b33', T=3, B=33, in0=64, H=512, L=1, y_relu=True, modes=('bf16x3', 'bf16'), **PERS),
    Case('persist_h768_drop', T=4, B=16, in0=40, H=768, L=2, p=0.25, modes=('bf16x3', 'bf16'), **PERS),
    Case('persist_h1024_b64', T=3, B=64, in0=128, H=1024, L=2, p=0.2, modes=('bf16x3', 'bf16'), **PERS),     # B % 32 == 0: the chain emits the images
    Case('persist_h1280', T=3, B=16, in0=40, H=1280, L=1, **PERS),                         # template instance 5
    Case('persist_h1536', T=3, B=16, in0=64, H=1536, L=1, **PERS),                         # template instance 6
    # ---- 32 batch rows per workgroup ----
    Case('persist32_h512_b144', T=3, B=144, in0=40, H=512, L=1, **{**PERS, 'group': 'persist32'}),
    Case('persist32_h1536_b64', T=3, B=64, in0=128, H=1536, L=1, **{**PERS, 'group': 'persist32'}),
    # ---- both layers in one launch ----
    Case('persist2_t1_state', T=1, B=5, in0=40, H=256, L=2, state=True, **P2),             # combined steps 0 and 1 only
    Case('persist2_t2', T=2, B=16, in0=40, H=256, L=2, y_relu=True, **P2),
    Case('persist2_h768_drop', T=6, B=16, in0=40, H=768, L=2, p=0.25, **P2),
    Case('persist2_h1024_b64', T=5, B=64, in0=128, H=1024, L=2, p=0.2, **P2),              # the benchmarked configuration's launches
    Case('persist2_h1024_b88', T=4, B=88, in0=40, H=1024, L=2, state=True, interleave=False, **P2),     # launches of 4 + 2 tiles, last one ragged
    Case('persist2_t40', T=40, B=33, in0=40, H=512, L=2, **P2),                            # epochs and image offsets away from the small ones
    # ---- two batch tiles per workgroup, interleaved ----
    Case('persist2x_h1024_b104', T=3, B=104, in0=40, H=1024, L=2, p=0.2, **{**P2, 'group': 'persist2x'}),    # 6 tiles interleaved + one plain
    Case('persist2x_h256_b320', T=3, B=320, in0=64, H=256, L=2, **{**P2, 'group': 'persist2x'}),
    # ---- three layers: the top pair as one launch over a single per-layer launch ----
    Case('l3_h256_drop', T=4, B=16, in0=40, H=256, L=3, p=0.2, group='l3', fwd_kernel='lstm_persist2_fwd_kernel',
         bwd_kernel='lstm_persist_bwd_kernel'),
    # ---- no state exposed: outputs only, against free_running(float64) ----
    Case('fused_h64', T=5, B=5, in0=24, H=64, L=2, state=True, group='fused', fusion=True, modes=('bf16x3', 'bf16'), act='libm'),
    Case('fused_h256', T=4, B=17, in0=72, H=256, L=2, state=True, group='fused', fusion=True, modes=('bf16x3', 'bf16'), act='libm'),
    Case('split_h256', T=4, B=5, in0=40, H=256, L=2, state=True, group='split', fwd_kernel='lstm_persist2_fwd_kernel',
         bwd_kernel='lstm_persist_bwd_kernel'),
]
BY_NAME = {c.name: c for c in CASES}
TEACHER_FORCED = [c for c in CASES if c.group not in ('fused', 'split')]
OUTPUTS_ONLY = [c for c in CASES if c.group in ('fused', 'split')]


def make_inputs(case):
    """CPU float32 tensors of a case (deterministic): x, weights (nn.LSTM's U(-1/sqrt(H), 1/sqrt(H))), initial state, dy, dhn, dcn."""
    T, B, in0, H, L = case.T, case.B, case.in0, case.H, case.L
    g = torch.Generator().manual_seed(97 + sum(map(ord, case.name)))
    k = 1.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    inp = {
        'x': torch.randn(T, B, in0, generator=g),
        'w_ih': [u(4 * H, in0 if l == 0 else H) for l in range(L)],
        'w_hh': [u(4 * H, H) for l in range(L)],
        'b_ih': [u(4 * H) for l in range(L)],
        'b_hh': [u(4 * H) for l in range(L)],
        'h0': torch.randn(L, B, H, generator=g) * 0.3 if case.state else None,
        'c0': torch.randn(L, B, H, generator=g) * 0.3 if case.state else None,
        'dy': torch.randn(T, B, H, generator=g),
        'dhn': torch.randn(L, B, H, generator=g) * 0.1 if case.state else None,
        'dcn': torch.randn(L, B, H, generator=g) * 0.1 if case.state else None,
    }
    return inp


def masks(case):
    """[l] -> float32 [T, B, H] multipliers (0 or 1 / (1 - p)) of layer l's output, l < L - 1; None without dropout."""
    if case.p <= 0:
        return [None] * case.L
    n = case.T * case.B * case.H
    return [torch.from_numpy(philox.dropout_mask(n, case.p, SEED, STREAM_LSTM_LAYER0 + l, OFFSET)).reshape(case.T, case.B, case.H)
            if l < case.L - 1 else None for l in range(case.L)]


# ------------------------------------------------------------------------------------------------------------------------------
# the product model
# ------------------------------------------------------------------------------------------------------------------------------
def kinds(case, mode):
    """Per layer: the kind ('exact' | 'bf16' | 'x3') of each product (module docstring's table)."""
    M = {'f32': 'exact', 'bf16': 'bf16', 'bf16x3': 'x3'}[mode]
    out = []
    for l in range(case.L):
        in_dim = case.in0 if l == 0 else case.H
        wide = M if in_dim >= 64 else 'exact'
        rec = M if case.H % 32 == 0 else 'exact'
        k = {'in': wide, 'rec': rec, 'din': wide, 'dw': wide}
        if case.fusion and mode != 'f32':          # the layer-diagonal kernels: three passes whatever the mode
            k['rec'] = 'x3'
            if l > 0:
                k['in'] = k['din'] = 'x3'
        out.append(k)
    return out


def rb(x, trunc=False):
    """x (any float dtype, holding fp32 values) rounded to bf16, back in x's dtype.  trunc: the low 16 bits cut off instead (a mutant)."""
    x32 = x.to(F32)
    if trunc:
        r = (x32.contiguous().view(torch.int32) & -65536).view(F32)
    else:
        r = x32.to(torch.bfloat16).to(F32)
    return r.to(x.dtype)


def product(a, b, kind, dtype, a_trunc=False, a_exact=False):
    """a [M, K] x b [N, K]^T -> [M, N] in ``dtype`` under the product model."""
    a, b = a.to(dtype), b.to(dtype)
    if kind == 'exact':
        return a @ b.T
    ah = a if a_exact else rb(a, a_trunc)
    bh = rb(b)
    if kind == 'bf16':
        return ah @ bh.T
    al, bl = rb(a - ah), rb(b - bh)
    return ah @ bh.T + ah @ bl.T + al @ bh.T


def _sigmoid(x, act):
    if act == 'exact':
        return torch.sigmoid(x)
    if act == 'fast':       # fast_sigmoid, lstm_persist_dev.h:92-94
        return 1.0 / (1.0 + torch.exp2(x * x.new_tensor(-1.4426950408889634)))
    return 1.0 / (1.0 + torch.exp(-x))         # sigmoidf_, halo_common.h:95


def _tanh(x, act):
    if act == 'fast':       # fast_tanh / persist2_tanh, lstm_persist_dev.h:95-107
        return 1.0 - 2.0 / (1.0 + torch.exp2(x * x.new_tensor(2.8853900817779268)))
    return torch.tanh(x)


def cell_fwd(pre, c_prev, act):
    """pre [B, 4H] -> (activated gates [B, 4H], c, h)."""
    H = c_prev.shape[-1]
    i, f, o = (_sigmoid(pre[..., s * H:(s + 1) * H], act) for s in (0, 1, 3))
    g = _tanh(pre[..., 2 * H:3 * H], act)
    c = f * c_prev + i * g
    return torch.cat([i, f, g, o], -1), c, o * _tanh(c, act)


def cell_bwd(gates, c, c_prev, dh, dc_in, act, c_for_forget=None):
    """-> (dG [B, 4H] w.r.t. the pre-activations, dc carried to the step before)   (lstm.hip:421-435)."""
    H = c.shape[-1]
    i, f, g, o = (gates[..., s * H:(s + 1) * H] for s in range(4))
    tc = _tanh(c, act)
    dcc = dc_in + dh * o * (1.0 - tc * tc)
    d_o = dh * tc
    d_i, d_f, d_g = dcc * g, dcc * (c_prev if c_for_forget is None else c_for_forget), dcc * i
    dG = torch.cat([d_i * i * (1.0 - i), d_f * f * (1.0 - f), d_g * (1.0 - g * g), d_o * o * (1.0 - o)], -1)
    return dG, dcc * f


def _layer_grads(case, inp, kd, l, dG, lin, hprev, dtype, mutant=None):
    """dW_ih, dW_hh, db of layer l from its dG [T, B, 4H], its input and h_{t-1} (all [T, B, .])."""
    T, B = case.T, case.B
    g2 = dG.reshape(T * B, -1)
    hp = hprev
    if mutant == 'dwhh_pairs_h_t':
        hp = torch.cat([hprev[1:], hprev[-1:] * 0 + inp['_h_last'][l]], 0)
    dw_ih = product(g2.T, lin.reshape(T * B, -1).T, kd[l]['dw'], dtype)
    dw_hh = product(g2.T, hp.reshape(T * B, -1).T, kd[l]['dw'], dtype)
    db = (dG[1:] if mutant == 'db_skips_step0' else dG).to(dtype).sum((0, 1))
    return dw_ih, dw_hh, db


# ------------------------------------------------------------------------------------------------------------------------------
# free running: the reference on its own state (float64), the stand-in for a device (float32), the mutants
# ------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    # name: (the case it is run on -- one the GPU test runs too --, what the defect is)
    'h_truncated': ('persist_h256_state', 'h truncated to bf16 instead of rounded to nearest even'),
    'layer1_input_unrounded': ('persist_h256_state', "layer 1's input enters its projection unrounded"),
    'k_block_dropped': ('persist_h256_state', 'the last 32-wide K block of the recurrent sum dropped'),
    'ragged_rows_leak': ('persist_h256_state', "rows >= B of the ragged 16-row tile leak into row B-1's recurrent sums"),
    'mask_one_step_late': ('step_h96_drop', 'the dropout mask of step t applied at t + 1'),
    'mask_unscaled': ('step_h96_drop', 'the dropout mask applied without 1 / (1 - p)'),
    'mask_missing_on_gradient': ('step_h96_drop', 'no dropout mask on the gradient arriving from layer 1'),
    'dhn_dropped': ('persist_h256_state', 'dhn not added at t = T - 1'),
    'dcn_dropped': ('persist_h256_state', 'dcn not the start of the dc carry'),
    'forget_gate_uses_c_t': ('persist_h256_state', "c_t in place of c_{t-1} in the forget gate's gradient"),
    'db_skips_step0': ('persist_h256_state', 'db without step 0'),
    'dwhh_pairs_h_t': ('persist_h256_state', 'dW_hh pairs dG_t with h_t instead of h_{t-1}'),
    'layer1_state_from_layer0': ('persist_h256_state', "layer 1's initial state taken from layer 0's"),
    'relu_mask_from_dy': ('step_h160_k72', "the y_relu mask taken from dy's sign instead of y's"),
}


def free_running(case, inp, mode, dtype=F64, act='exact', mutant=None):
    """Forward and backward on the routine's own state.  Returns a ``state`` dict (the layout tests/test_gpu_lstm_f64.py reads off a
    device): per layer hprev [T, B, H] (h_{t-1}), lin [T, B, K] (the layer's input), dG [T, B, 4H]; y [T, B, H], hn, cn [L, B, H], dx,
    dw_ih / dw_hh / db_ih / db_hh lists."""
    T, B, H, L = case.T, case.B, case.H, case.L
    kd, mk = kinds(case, mode), masks(case)
    zeros = torch.zeros(B, H, dtype=dtype)
    st = {'hprev': [], 'lin': [], 'dG': [], 'gates': [], 'c': []}
    lin = inp['x'].to(dtype)
    hn, cn = [], []
    for l in range(L):
        src = 0 if (mutant == 'layer1_state_from_layer0' and l == 1) else l
        h = inp['h0'][src].to(dtype) if inp['h0'] is not None else zeros
        c = inp['c0'][src].to(dtype) if inp['c0'] is not None else zeros
        bias = (inp['b_ih'][l].to(dtype) + inp['b_hh'][l].to(dtype))
        proj = product(lin.reshape(T * B, -1), inp['w_ih'][l], kd[l]['in'], dtype,
                       a_exact=(mutant == 'layer1_input_unrounded' and l == 1)).reshape(T, B, 4 * H) + bias
        hs, cs, gs = [h], [c], []
        for t in range(T):
            ha = h
            if mutant == 'k_block_dropped':
                ha = h.clone(); ha[:, H - 32:] = 0
            rec = product(ha, inp['w_hh'][l], kd[l]['rec'], dtype, a_trunc=(mutant == 'h_truncated'))
            if mutant == 'ragged_rows_leak' and B % 16:
                rec[B - 1] += rec[0]
            gates, c, h = cell_fwd(proj[t] + rec, c, act)
            hs.append(h); cs.append(c); gs.append(gates)
        hs, cs = torch.stack(hs), torch.stack(cs)
        st['hprev'].append(hs[:-1]); st['lin'].append(lin); st['gates'].append(torch.stack(gs)); st['c'].append(cs)
        hn.append(hs[-1]); cn.append(cs[-1])
        if l < L - 1:
            lin = hs[1:]
            if mk[l] is not None:
                m = mk[l].to(dtype)
                if mutant == 'mask_one_step_late':
                    m = torch.roll(m, 1, 0)
                if mutant == 'mask_unscaled':
                    m = (m > 0).to(dtype)
                lin = lin * m
    top = hs[1:]
    st['y'] = torch.relu(top) if case.y_relu else top
    st['hn'], st['cn'] = torch.stack(hn), torch.stack(cn)
    # ---- backward, top layer first ----
    st['dG'] = [None] * L
    grads = {k: [None] * L for k in ('dw_ih', 'dw_hh', 'db_ih', 'db_hh')}
    din = None
    for l in range(L - 1, -1, -1):
        if l == L - 1:
            dyl = inp['dy'].to(dtype)
            if case.y_relu:
                dyl = dyl * ((inp['dy'] > 0) if mutant == 'relu_mask_from_dy' else (st['y'] > 0)).to(dtype)
        else:
            dyl = din
        dc = inp['dcn'][l].to(dtype) if (inp['dcn'] is not None and mutant != 'dcn_dropped') else zeros
        dGs = [None] * T
        for t in range(T - 1, -1, -1):
            dh = dyl[t]
            if t == T - 1:
                if inp['dhn'] is not None and mutant != 'dhn_dropped':
                    dh = dh + inp['dhn'][l].to(dtype)
            else:
                dh = dh + product(dGs[t + 1], inp['w_hh'][l].T, kd[l]['rec'], dtype)
            dGs[t], dc = cell_bwd(st['gates'][l][t], st['c'][l][t + 1], st['c'][l][t], dh, dc, act,
                                  c_for_forget=st['c'][l][t + 1] if mutant == 'forget_gate_uses_c_t' else None)
        dG = torch.stack(dGs)
        st['dG'][l] = dG
        inp_m = dict(inp, _h_last=hn)
        grads['dw_ih'][l], grads['dw_hh'][l], db = _layer_grads(case, inp_m, kd, l, dG, st['lin'][l], st['hprev'][l], dtype, mutant)
        grads['db_ih'][l] = grads['db_hh'][l] = db
        din = product(dG.reshape(T * B, 4 * H), inp['w_ih'][l].T, kd[l]['din'], dtype).reshape(T, B, -1)
        if l > 0 and mk[l - 1] is not None and mutant != 'mask_missing_on_gradient':
            din = din * mk[l - 1].to(dtype)
    st['dx'] = din
    st.update(grads)
    del st['gates'], st['c']
    return st


# ------------------------------------------------------------------------------------------------------------------------------
# teacher forced: float64 on the device's own operands
# ------------------------------------------------------------------------------------------------------------------------------
def teacher_forced(case, inp, state, mode, dtype=F64):
    """The reference value of every quantity ``quantities(state)`` names, each step computed from the DEVICE's operands in ``state``; only
    c and dc (which no record exposes) are carried by the reference itself."""
    T, B, H, L = case.T, case.B, case.H, case.L
    kd, mk = kinds(case, mode), masks(case)
    zeros = torch.zeros(B, H, dtype=dtype)
    ref, gates_l, c_l = {}, [], []
    for l in range(L):
        lin, hprev = state['lin'][l].to(dtype), state['hprev'][l].to(dtype)
        bias = inp['b_ih'][l].to(dtype) + inp['b_hh'][l].to(dtype)
        pre = (product(lin.reshape(T * B, -1), inp['w_ih'][l], kd[l]['in'], dtype) +
               product(hprev.reshape(T * B, H), inp['w_hh'][l], kd[l]['rec'], dtype) + bias).reshape(T, B, 4 * H)
        c = inp['c0'][l].to(dtype) if inp['c0'] is not None else zeros
        hs, cs, gs = [], [c], []
        for t in range(T):
            gates, c, h = cell_fwd(pre[t], c, 'exact')
            hs.append(h); cs.append(c); gs.append(gates)
        ref[f'h{l}'] = torch.stack(hs)
        ref[f'cn{l}'] = c
        gates_l.append(torch.stack(gs)); c_l.append(torch.stack(cs))
        if l < L - 1 and mk[l] is not None:
            ref[f'ydrop{l}'] = ref[f'h{l}'] * mk[l].to(dtype)
    top = ref[f'h{L - 1}']
    ref['y'] = torch.relu(top) if case.y_relu else top
    for l in range(L - 1, -1, -1):
        dG_dev = state['dG'][l].to(dtype)
        if l == L - 1:
            dh = inp['dy'].to(dtype)
            if case.y_relu:
                dh = dh * (state['y'] > 0).to(dtype)          # the device's own mask: a sign flip of an h near 0 must not propagate either
        else:
            dh = product(state['dG'][l + 1].to(dtype).reshape(T * B, 4 * H), inp['w_ih'][l + 1].T, kd[l + 1]['din'], dtype).reshape(T, B, H)
            if mk[l] is not None:
                dh = dh * mk[l].to(dtype)
        dh = dh.clone()
        if T > 1:
            dh[:-1] += product(dG_dev[1:].reshape((T - 1) * B, 4 * H), inp['w_hh'][l].T, kd[l]['rec'], dtype).reshape(T - 1, B, H)
        if inp['dhn'] is not None:
            dh[-1] += inp['dhn'][l].to(dtype)
        dc = inp['dcn'][l].to(dtype) if inp['dcn'] is not None else zeros
        dGs = [None] * T
        for t in range(T - 1, -1, -1):
            dGs[t], dc = cell_bwd(gates_l[l][t], c_l[l][t + 1], c_l[l][t], dh[t], dc, 'exact')
        ref[f'dG{l}'] = torch.stack(dGs)
        ref[f'dw_ih{l}'], ref[f'dw_hh{l}'], db = _layer_grads(case, inp, kd, l, dG_dev, state['lin'][l], state['hprev'][l], dtype)
        ref[f'db_ih{l}'] = ref[f'db_hh{l}'] = db
    ref['dx'] = product(state['dG'][0].to(dtype).reshape(T * B, 4 * H), inp['w_ih'][0].T, kd[0]['din'], dtype).reshape(T, B, -1)
    return ref


def quantities(case, state):
    """What teacher_forced's keys are compared with, read off a state."""
    L = case.L
    q = {'y': state['y'], 'dx': state['dx']}
    for l in range(L):
        q[f'h{l}'] = torch.cat([state['hprev'][l][1:], state['hn'][l][None]], 0)          # h_0 .. h_{T-1}
        q[f'cn{l}'] = state['cn'][l]
        if l < L - 1 and case.p > 0:
            q[f'ydrop{l}'] = state['lin'][l + 1]
        q[f'dG{l}'] = state['dG'][l]
        for k in ('dw_ih', 'dw_hh', 'db_ih', 'db_hh'):
            q[f'{k}{l}'] = state[k][l]
    return q


def outputs(case, state):
    """The outputs a caller sees (the paths that expose no state are held to these only)."""
    q = {'y': state['y'], 'hn': state['hn'], 'cn': state['cn'], 'dx': state['dx']}
    for l in range(case.L):
        for k in ('dw_ih', 'dw_hh', 'db_ih', 'db_hh'):
            q[f'{k}{l}'] = state[k][l]
    return q


ABSOLUTE = ('h', 'y', 'cn', 'hn', 'ydrop')       # forward quantities: absolute deviation; gradients: of the reference's max-abs


def deviations(got, ref):
    """{key: max |got - ref|, absolute for the forward quantities, divided by max |ref| for the gradients}."""
    out = {}
    for k, r in ref.items():
        d = (got[k].to(F64) - r.to(F64)).abs().max().item()
        if not k.startswith(ABSOLUTE):
            d /= max(r.abs().max().item(), 1e-300)
        out[k] = d
    return out


def first_outside(got, ref, key, bound):
    """(index, got, ref) of the first element (in memory order: time step first) of ``key`` outside the bound."""
    r = ref[key].to(F64)
    d = (got[key].to(F64) - r).abs()
    if not key.startswith(ABSOLUTE):
        d = d / max(r.abs().max().item(), 1e-300)
    idx = torch.nonzero(d > bound)
    if not len(idx):
        return None
    i = tuple(idx[0].tolist())
    return i, got[key][i].item(), r[i].item()


FLOOR = 1e-6       # five activations at the 2e-7 lstm_persist_dev.h:91 states (h, y, c: absolute); 1e-6 of max-abs for the gradients


def bounds(noise, factor=8.0, floor=FLOOR):
    """bound_q = max(factor * worst32_q, floor): worst32 is the fp32 stand-in's deviation from the reference on the same case."""
    return {k: max(factor * v, floor) for k, v in noise.items()}


@functools.lru_cache(maxsize=None)
def stand_in_noise(name, mode):
    """worst32 per quantity: the faithful fp32 stand-in against teacher_forced(float64) on its own state."""
    case = BY_NAME[name]
    inp = make_inputs(case)
    st = free_running(case, inp, mode, F32, case.act)
    return deviations(quantities(case, st), teacher_forced(case, inp, st, mode))


@functools.lru_cache(maxsize=None)
def stand_in_output_noise(name, mode):
    """The same for the outputs-only paths: the fp32 stand-in against free_running(float64)."""
    case = BY_NAME[name]
    inp = make_inputs(case)
    st = free_running(case, inp, mode, F32, case.act)
    return deviations(outputs(case, st), outputs(case, free_running(case, inp, mode, F64)))
