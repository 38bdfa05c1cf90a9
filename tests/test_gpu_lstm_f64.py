"""Every LSTM launch path (csrc/lstm.hip step chain, lstm_persist.hip, lstm_persist32.hip, lstm_persist2.hip, lstm_persist2x.hip, the
layer-diagonal schedule) against float64 under the kernels' own operand rounding (tests/lstm_ref.py; DESIGN.md "LSTM against float64").

Where the state is exposed (ops.lstm_ghost_terms after a whole backward under the keep flag: dG, the layer inputs, h_{t-1}) the float64
reference is TEACHER-FORCED on the device's own operands, so every h_t, y, hn, cn, dG_t, dW, db and dx is held to
max(8 x the fp32 stand-in's own deviation from that reference, 1e-6): fp32 rounding of one step, nothing else.  Where it is not (the
layer-diagonal schedule, a split backward) the outputs are held to 4 x the stand-in's deviation from the free-running float64 reference."""
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops
    _lib.lib()
    _lib.lend_scratch()
    return dict(ops=ops, lib=_lib)


class _Switches:
    """Math mode and the launch-path switches of a case; everything back to the defaults on exit."""

    def __init__(self, lib, case, mode):
        self.lib, self.case, self.mode = lib, case, mode

    def __enter__(self):
        self.prev_mode = self.lib.get_math_mode()
        self.prev_keep = self.lib.get_lstm_keep_gate_gradients()
        self.lib.set_math_mode(self.mode)
        self.lib.set_lstm_persistent2(self.case.persistent2)
        self.lib.set_lstm_interleave(self.case.interleave)
        self.lib.set_lstm_fusion(self.case.fusion)

    def __exit__(self, *exc):
        self.lib.set_lstm_keep_gate_gradients(self.prev_keep)
        self.lib.set_lstm_fusion(False)
        self.lib.set_lstm_interleave(True)
        self.lib.set_lstm_persistent2(True)
        self.lib.set_math_mode(self.prev_mode)


def _to_dev(inp):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else (v.to(DEV) if v is not None else None)) for k, v in inp.items()}


POISON = 3.0e4      # finite in bf16 too: a product that reached it would be off by orders, not NaN


def _status_word(hal, buf, backward, case):
    off = hal['lib'].lib().halo_lstm_status_offset(int(backward), case.T, case.B, case.in0, case.H, case.L)
    return buf.view(torch.int32)[off // 4:off // 4 + 1]


def _status(hal, buf, backward, case):
    return int(_status_word(hal, buf, backward, case).item())


def _same_bits(a, b, what):
    assert torch.equal(a, b), (what, 'max |difference|', (a.double() - b.double()).abs().max().item())


def _view(rec, T, B, x, reserve):
    """[T, B, K] view of a ghost operand record: its pointer lies in x (layer 0's input) or in the reserve; strides are the record's."""
    for base in (x, reserve):
        lo = base.data_ptr()
        if lo <= rec.ptr < lo + base.numel() * 4:
            assert (rec.ptr - lo) % 4 == 0
            return base.as_strided((T, B, rec.K), (rec.stride_t, rec.stride_n, 1), (rec.ptr - lo) // 4 + base.storage_offset())
    raise AssertionError('a ghost operand points outside x and the reserve')


def _run(hal, case, d, keep, split=False):
    """One forward + backward of the case; returns (outputs on the CPU, state on the CPU or None, kernel names)."""
    ops, lib = hal['ops'], hal['lib']
    T, B, H, L = case.T, case.B, case.H, case.L
    drop = ops.Dropout(case.p, R.SEED, R.OFFSET) if case.p > 0 else ops.NO_DROPOUT
    lib.set_lstm_keep_gate_gradients(keep)
    if case.y_relu:      # batch-first output through y_strides
        ybuf = torch.full((B, T, H), float('nan'), device=DEV)
        y_strides, y_tm = (H, T * H), ybuf.transpose(0, 1)
    else:
        ybuf, y_strides, y_tm = None, None, None
    # reserve and workspace arrive holding whatever the allocation held: here a finite poison (no launch may depend on it), except for
    # the two status words, which the persistent launches raise on a timed-out wait and the step chains never touch
    reserve = ops.lstm_reserve(T, B, case.in0, H, L, DEV).fill_(POISON)
    _status_word(hal, reserve, False, case).zero_()
    y, hn, cn, reserve = ops.lstm_fwd(d['x'], d['w_ih'], d['w_hh'], d['b_ih'], d['b_hh'], h0=d['h0'], c0=d['c0'], y=ybuf, y_strides=y_strides,
                                      y_relu=case.y_relu, want_state=True, drop=drop, reserve=reserve)
    if y_tm is None:
        y_tm, y_strides = y, (B * H, H)
    torch.cuda.synchronize()
    assert _status(hal, reserve, False, case) == 0
    names = [lib.lstm_chain_info('fwd')['kernel']]
    ws = ops.lstm_bwd_workspace(d['x'], d['w_hh']).fill_(POISON)
    _status_word(hal, ws, True, case).zero_()
    dy_arg = d['dy'].transpose(0, 1).contiguous() if case.y_relu else d['dy']                     # dy laid out as y is
    kw = dict(dhn=d['dhn'], dcn=d['dcn'], want_dx=True, drop=drop, workspace=ws)
    if split:
        _, grads = ops.lstm_bwd(d['x'], d['w_ih'], d['w_hh'], dy_arg, y_strides, case.y_relu, reserve, layers=(L - 1, L), **kw)
        dx, grads = ops.lstm_bwd(d['x'], d['w_ih'], d['w_hh'], dy_arg, y_strides, case.y_relu, reserve, layers=(0, L - 1), grads=grads, **kw)
    else:
        dx, grads = ops.lstm_bwd(d['x'], d['w_ih'], d['w_hh'], dy_arg, y_strides, case.y_relu, reserve, **kw)
    torch.cuda.synchronize()
    assert _status(hal, ws, True, case) == 0
    names.append(lib.lstm_chain_info('bwd')['kernel'])
    out = {'y': y_tm.cpu().contiguous(), 'hn': hn.cpu(), 'cn': cn.cpu(), 'dx': dx.cpu()}
    for k, lst in grads.items():
        out[k] = [t.cpu() for t in lst]
    state = None
    if keep and not split and not case.fusion:
        terms = ops.lstm_ghost_terms(d['x'], reserve, H, L, p_drop=case.p)
        state = dict(out)
        state['dG'] = [_view(tm.a, T, B, d['x'], reserve).cpu().contiguous() for tm in terms]
        state['lin'] = [_view(tm.b[0], T, B, d['x'], reserve).cpu().contiguous() for tm in terms]
        state['hprev'] = [_view(tm.b[1], T, B, d['x'], reserve).cpu().contiguous() for tm in terms]
    return out, state, names, reserve


def _path(case, names):
    """The launch path the case is here for, from lstm_chain_info and the launchers' own rules (the 32-row and the interleaved kernels run
    under their 16-row siblings' names: lstm_persist.hip:437, lstm_persist2.hip:792-821)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nj, nbt = case.H // 16, (case.B + 15) // 16
    label = list(names)
    if case.group == 'persist32':
        assert nj * nbt > cus >= nj * ((case.B + 31) // 32)
        label = [n.replace('persist_', 'persist_(32 rows)_') for n in names]
    elif case.group in ('persist', 'l3'):
        assert nj * nbt <= cus
    if case.group == 'persist2x':
        assert case.interleave and nbt > max(1, cus // nj)
        label = [n.replace('persist2_', 'persist2x_') for n in names]
    elif case.group == 'persist2':
        assert nbt <= max(1, cus // nj) or not case.interleave
    return label


def _report(case, mode, label, ratios):
    worst = {}
    for k, v in ratios.items():
        q = k.rstrip('0123456789')
        worst[q] = max(worst.get(q, 0.0), v)
    print(f'\n{case.name} [{mode}] {" / ".join(label)}: device/bound ' + '  '.join(f'{q} {v:.2f}' for q, v in worst.items()))


TF = [(c, m) for c in R.TEACHER_FORCED for m in c.modes]


@pytest.mark.parametrize('case,mode', TF, ids=[f'{c.name}-{m}' for c, m in TF])
def test_launch_matches_teacher_forced_float64(hal, case, mode):
    """Observed device/bound ratios per path: DESIGN.md "LSTM against float64"."""
    inp = R.make_inputs(case)
    with _Switches(hal['lib'], case, mode):
        d = _to_dev(inp)
        out, state, names, _ = _run(hal, case, d, keep=True)
        assert names == [case.fwd_kernel, case.bwd_kernel], names
        label = _path(case, names)
        # the benchmarked configuration: keep flag off, the chains skip the fp32 dG stores no launch reads (skip_dg).  No output is summed
        # in another order there (the chains emit the same operand images either way: lstm.hip:1762-1816, 1935-1966): bit-identical
        plain, _, names2, _ = _run(hal, case, d, keep=False)
        assert names2 == names
    for k in ('y', 'hn', 'cn', 'dx'):
        _same_bits(plain[k], out[k], k)
    for k in ('dw_ih', 'dw_hh', 'db_ih', 'db_hh'):
        for l in range(case.L):
            _same_bits(plain[k][l], out[k][l], (k, l))
    for l in range(case.L):         # h_{-1}: the given initial state, or zeros, bit for bit
        want = inp['h0'][l] if case.state else torch.zeros(case.B, case.H)
        assert torch.equal(state['hprev'][l][0], want), l
    got = R.quantities(case, state)
    ref = R.teacher_forced(case, inp, state, mode)
    dev = R.deviations(got, ref)
    bound = R.bounds(R.stand_in_noise(case.name, mode))
    ratios = {k: dev[k] / bound[k] for k in dev}
    _report(case, mode, label, ratios)
    for k in dev:
        assert dev[k] <= bound[k], (k, dev[k], bound[k], 'first (index, device, reference):', R.first_outside(got, ref, k, bound[k]))


OO = [(c, m) for c in R.OUTPUTS_ONLY for m in c.modes]


@pytest.mark.parametrize('case,mode', OO, ids=[f'{c.name}-{m}' for c, m in OO])
def test_stateless_path_outputs_match_free_running_float64(hal, case, mode):
    """The layer-diagonal schedule and a split backward leave no complete state to teacher-force on: outputs only, 4 x the fp32 stand-in's own
    deviation from the free-running float64 reference (rounding flips propagate in both, a random draw each: the factor)."""
    inp = R.make_inputs(case)
    with _Switches(hal['lib'], case, mode):
        d = _to_dev(inp)
        out, _, names, reserve = _run(hal, case, d, keep=True, split=case.group == 'split')
        with pytest.raises(hal['lib'].HaloError):         # ... and the library says so itself (the fused schedule; a partial layer range)
            hal['ops'].lstm_ghost_terms(d['x'], reserve, case.H, case.L, p_drop=case.p)
        if case.fusion:
            label = ['lstm_diag_fwd_kernel', 'lstm_diag_bwd_kernel']     # (no chain record: what set_lstm_fusion selects at H % 64 == 0, lstm.hip:1043)
            assert case.H % 64 == 0 and mode != 'f32' and 2 <= case.L <= 4
        else:
            assert names == [case.fwd_kernel, case.bwd_kernel], names
            label = names
    ref = R.outputs(case, R.free_running(case, inp, mode, R.F64))
    got = R.outputs(case, out)
    dev = R.deviations(got, ref)
    bound = R.bounds(R.stand_in_output_noise(case.name, mode), factor=4.0, floor=0.0)
    _report(case, mode, label, {k: dev[k] / bound[k] for k in dev})
    for k in dev:
        assert dev[k] <= bound[k], (k, dev[k], bound[k])
