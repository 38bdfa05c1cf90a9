"""tests/lstm_ref.py before anything is tied to it: the float64 reference against torch.nn.LSTM with autograd, the faithful fp32 stand-in
inside the teacher-forced gates of tests/test_gpu_lstm_f64.py on every case, and every mutant stand-in rejected by a gate with a margin
of at least 10x.  No GPU."""
import pytest
import torch

import lstm_ref as R

F32, F64 = torch.float32, torch.float64


def _loss_terms(inp, y, hn, cn):
    loss = (y * inp['dy'].to(F64)).sum()
    if inp['dhn'] is not None:
        loss = loss + (hn * inp['dhn'].to(F64)).sum() + (cn * inp['dcn'].to(F64)).sum()
    return loss


def _check(ours, theirs, tol, what):
    d = (ours.to(F64) - theirs.to(F64)).abs().max().item()
    assert d <= tol, (what, d)


def test_reference_equals_float64_nn_lstm_with_autograd():
    """free_running(float64, 'f32' mode) == torch.nn.LSTM in float64, outputs and every gradient, 2 layers with carried state."""
    case = R.Case('nn_lstm', 'step', T=6, B=4, in0=24, H=48, L=2, state=True, modes=('f32',))
    inp = R.make_inputs(case)
    st = R.free_running(case, inp, 'f32', F64)
    net = torch.nn.LSTM(case.in0, case.H, num_layers=case.L).double()
    with torch.no_grad():
        for l in range(case.L):
            for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh'):
                getattr(net, f"{k.replace('w_', 'weight_').replace('b_', 'bias_')}_l{l}").copy_(inp[k][l].double())
    x = inp['x'].double().requires_grad_(True)
    y, (hn, cn) = net(x, (inp['h0'].double(), inp['c0'].double()))
    _loss_terms(inp, y, hn, cn).backward()
    _check(st['y'], y.detach(), 1e-12, 'y'); _check(st['hn'], hn.detach(), 1e-12, 'hn'); _check(st['cn'], cn.detach(), 1e-12, 'cn')
    _check(st['dx'], x.grad, 1e-12, 'dx')
    for l in range(case.L):
        _check(st['dw_ih'][l], getattr(net, f'weight_ih_l{l}').grad, 1e-12, f'dw_ih{l}')
        _check(st['dw_hh'][l], getattr(net, f'weight_hh_l{l}').grad, 1e-12, f'dw_hh{l}')
        _check(st['db_ih'][l], getattr(net, f'bias_ih_l{l}').grad, 1e-12, f'db_ih{l}')
        _check(st['db_hh'][l], getattr(net, f'bias_hh_l{l}').grad, 1e-12, f'db_hh{l}')


@pytest.mark.parametrize('y_relu', [False, True])
def test_reference_with_dropout_equals_autograd_restatement(y_relu):
    """With inter-layer dropout (and the relu'd output): an nn.LSTMCell-style restatement under autograd, fed the Philox masks."""
    case = R.Case('autograd_drop', 'step', T=5, B=3, in0=24, H=32, L=3, p=0.25, state=True, y_relu=y_relu, modes=('f32',))
    inp = R.make_inputs(case)
    st = R.free_running(case, inp, 'f32', F64)
    mk = R.masks(case)
    leaves = {k: [t.double().requires_grad_(True) for t in inp[k]] for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')}
    x = inp['x'].double().requires_grad_(True)
    lin, hn, cn = x, [], []
    for l in range(case.L):
        h, c = inp['h0'][l].double(), inp['c0'][l].double()
        out = []
        for t in range(case.T):
            i, f, g, o = (lin[t] @ leaves['w_ih'][l].T + h @ leaves['w_hh'][l].T + leaves['b_ih'][l] + leaves['b_hh'][l]).chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out.append(h)
        lin = torch.stack(out)
        hn.append(h); cn.append(c)
        if l < case.L - 1:
            lin = lin * mk[l].double()
    y = torch.relu(lin) if y_relu else lin
    _loss_terms(inp, y, torch.stack(hn), torch.stack(cn)).backward()
    _check(st['y'], y.detach(), 1e-12, 'y'); _check(st['dx'], x.grad, 1e-12, 'dx')
    for l in range(case.L):
        for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh'):
            _check(st['d' + k][l], leaves[k][l].grad, 1e-12, f'd{k}{l}')


def test_float64_teacher_forced_on_its_own_state_is_a_fixed_point():
    """teacher_forced on the float64 free-running state reproduces that state in every mode: the two restate the same arithmetic."""
    for name, mode in (('step_h96_drop', 'bf16'), ('step_h160_k72', 'bf16x3'), ('step_h48_state', 'f32')):
        case = R.BY_NAME[name]
        inp = R.make_inputs(case)
        st = R.free_running(case, inp, mode, F64)
        dev = R.deviations(R.quantities(case, st), R.teacher_forced(case, inp, st, mode))
        assert max(dev.values()) <= 1e-12, (name, mode, dev)


def test_product_model_follows_the_table():
    k = R.kinds(R.BY_NAME['step_h48_state'], 'bf16')           # H % 32 != 0, every width < 64: exact throughout
    assert all(v == 'exact' for layer in k for v in layer.values())
    k = R.kinds(R.BY_NAME['step_h96_drop'], 'bf16')
    assert k[0] == {'in': 'exact', 'rec': 'bf16', 'din': 'exact', 'dw': 'exact'} and k[1] == {'in': 'bf16', 'rec': 'bf16', 'din': 'bf16', 'dw': 'bf16'}
    k = R.kinds(R.BY_NAME['fused_h256'], 'bf16')
    assert k[0] == {'in': 'bf16', 'rec': 'x3', 'din': 'bf16', 'dw': 'bf16'} and k[1] == {'in': 'x3', 'rec': 'x3', 'din': 'x3', 'dw': 'bf16'}
    a = torch.tensor([[1.0 + 2.0 ** -8, 3.0]]); b = torch.tensor([[1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0]])      # bf16: 8 significant bits
    assert R.rb(a)[0, 0].item() == 1.0 and R.rb(b)[0, 0].item() == 1.0 + 2.0 ** -6      # ties to even, both ways
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -9])
    assert R.rb(v).item() == 1.0 + 2.0 ** -7 and R.rb(v, trunc=True).item() == 1.0
    assert R.product(a, b, 'bf16', F64).item() == 1.0 * (1.0 + 2.0 ** -6) + 3.0
    exact = (1.0 + 2.0 ** -8) * (1.0 + 2.0 ** -7 + 2.0 ** -8) + 3.0
    assert R.product(a, b, 'exact', F64).item() == exact
    assert R.product(a, b, 'x3', F64).item() == exact + 2.0 ** -16                      # all but lo(a) lo(b) = -2^-8 * 2^-8


CASE_MODES = [(c.name, m) for c in R.TEACHER_FORCED for m in c.modes]


@pytest.mark.parametrize('name,mode', CASE_MODES, ids=[f'{n}-{m}' for n, m in CASE_MODES])
def test_faithful_stand_in_passes_every_gate(name, mode):
    """The gate of tests/test_gpu_lstm_f64.py is max(8 * worst32, floor) with worst32 the stand-in's own deviation, so the stand-in passes
    by construction; what this pins is that worst32 is fp32 NOISE on every case, i.e. that no bound a device is held to grows past a
    tenth of the smallest deviation a mutant shows on its rejecting gate (1.26e-4, layer 1's input unrounded: test below):
    8 x worst32 <= 1.2e-5."""
    noise = R.stand_in_noise(name, mode)
    bound = R.bounds(noise)
    print(name, mode, {k: f'{v:.1e}' for k, v in noise.items()})
    for k, v in noise.items():
        assert v <= bound[k]
        assert bound[k] <= 1.2e-5, (k, v)


@pytest.mark.parametrize('name,mode', [(c.name, m) for c in R.OUTPUTS_ONLY for m in c.modes])
def test_outputs_only_bound_is_flip_noise(name, mode):
    """Free-running against free-running: rounding flips propagate, so the bound is orders wider than the teacher-forced gates (and is
    recorded for what it is); it must still be far below the coarse kernel-against-kernel bounds it sits beside."""
    noise = R.stand_in_output_noise(name, mode)
    print(name, mode, {k: f'{v:.1e}' for k, v in noise.items()})
    assert 0 < max(noise.values()) <= 5e-4


@pytest.mark.parametrize('mutant', list(R.MUTANTS))
def test_every_mutant_is_rejected_with_margin(mutant):
    """A stand-in with one defect leaves a gate by at least 10x that gate's bound, on a case the GPU test runs in bf16 mode."""
    name, _ = R.MUTANTS[mutant]
    case = R.BY_NAME[name]
    inp = R.make_inputs(case)
    bound = R.bounds(R.stand_in_noise(name, 'bf16'))
    st = R.free_running(case, inp, 'bf16', F32, case.act, mutant=mutant)
    dev = R.deviations(R.quantities(case, st), R.teacher_forced(case, inp, st, 'bf16'))
    margins = {k: dev[k] / bound[k] for k in dev}
    worst = max(margins, key=margins.get)
    print(mutant, worst, f'deviation {dev[worst]:.2e}  bound {bound[worst]:.2e}  margin {margins[worst]:.0f}x')
    if mutant == 'layer1_state_from_layer0':
        # the bit-for-bit gate on h_{-1} sees it as well
        assert not torch.equal(st['hprev'][1][0], inp['h0'][1])
    assert margins[worst] >= 10.0, margins
