"""The two-layer persistent forward's data-flag hand-off (csrc/lstm_persist2.hip, HALO_PERSIST_DATAFLAG, default on) against the
epoch-word hand-off it replaces (HALO_PERSIST_DATAFLAG=0): the same bits for the LSTM op over batch, length, width and dropout, and
for three full LstmCtcTrainer steps at the benchmark's shape; images re-armed by every call; a workgroup that never publishes ends the
launch loudly and boundedly.  The switch is read once per process, so each setting runs in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import sys, os
sys.path.insert(0, os.environ['DF_ROOT'])
import numpy as np
import torch
from haloop_amd import _lib, ops
_lib.lib(); _lib.lend_scratch()
_lib.set_math_mode('bf16')
out, what = sys.argv[1], sys.argv[2]
dev = 'cuda'
res = {}

def lstm_case(T, B, H, p_drop, seed, tag):
    L, in0 = 2, 128
    assert _lib.lib().halo_lstm_persistent2_eligible(T, B, H, L) == 1, (T, B, H)
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    x = torch.randn(T, B, in0, generator=g).to(dev)
    w_ih = [((torch.rand(4 * H, in0 if l == 0 else H, generator=g) * 2 - 1) * k).to(dev) for l in range(L)]
    w_hh = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(dev) for l in range(L)]
    b_ih = [((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(dev) for l in range(L)]
    b_hh = [((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(dev) for l in range(L)]
    dy = torch.randn(T, B, H, generator=g).to(dev)
    drop = ops.Dropout(p_drop, seed, 1) if p_drop > 0 else ops.NO_DROPOUT
    y, hn, cn, reserve = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, want_state=True, drop=drop)
    dx, gr = ops.lstm_bwd(x, w_ih, w_hh, dy, (B * H, H), False, reserve, want_dx=True, drop=drop)
    torch.cuda.synchronize()
    res[tag + '/y'] = y.cpu().numpy(); res[tag + '/hn'] = hn.cpu().numpy(); res[tag + '/cn'] = cn.cpu().numpy()
    res[tag + '/dx'] = dx.cpu().numpy()
    for name, vals in gr.items():
        for l, v in enumerate(vals):
            res[f'{tag}/{name}{l}'] = v.cpu().numpy()

if what == 'grid':
    for H in (256, 1024):
        for B in (16, 48, 64):
            for T in (1, 2, 21):
                for p in (0.0, 0.2):
                    lstm_case(T, B, H, p, 1000 + T * 7 + B + H, f'{H}/{B}/{T}/{p}')
elif what == 'twice':          # two calls of one shape, different inputs, in ONE process
    lstm_case(21, 64, 1024, 0.2, 5, 'first')
    lstm_case(21, 64, 1024, 0.2, 6, 'second')
elif what == 'once':           # the second of them alone, fresh
    lstm_case(21, 64, 1024, 0.2, 6, 'second')
elif what == 'trainer':        # three steps of the benchmark's training step
    sys.path.insert(0, os.environ['DF_ROOT'])
    import bench
    from haloop_amd import synth
    from haloop_amd.train import LstmCtcTrainer
    enc, rec, _ = bench.build_model(torch.device(dev))
    tr = LstmCtcTrainer(enc, rec, seed=1337, use_graph=True, alias_loss=True)
    x, il, tg, tl = (t.to(dev) for t in synth.synthetic_batch(bench.B_PER_GPU, bench.T, bench.F, bench.V, bench.S, 42))
    for i in range(3):
        tr.step(x, il, tg, tl)
        torch.cuda.synchronize()
        res[f'loss{i}'] = tr.loss.detach().cpu().numpy().reshape(1)
    tr.check_status()
    named = [(pfx + n, p) for pfx, m in (('encoder.', tr.encoder), ('recognizer.', tr.recognizer)) for n, p in m.named_parameters()]
    res['params'] = torch.cat([p.detach().reshape(-1) for _, p in named]).cpu().numpy()
    res['exp_avg'] = tr.flat.exp_avg.cpu().numpy()
    res['exp_avg_sq'] = tr.flat.exp_avg_sq.cpu().numpy()
elif what == 'mute':           # a workgroup of the forward never publishes: bounded, loud; the next call is clean
    T, B, in0, H, L = 3, 64, 128, 1024, 2
    g = torch.Generator().manual_seed(31)
    k = 1.0 / H ** 0.5
    x = torch.randn(T, B, in0, generator=g).to(dev)
    w_ih = [((torch.rand(4 * H, in0 if l == 0 else H, generator=g) * 2 - 1) * k).to(dev) for l in range(L)]
    w_hh = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(dev) for l in range(L)]
    b = [torch.zeros(4 * H, device=dev) for l in range(L)]
    assert _lib.lib().halo_lstm_persistent2_eligible(T, B, H, L) == 1
    clean = ops.lstm_fwd(x, w_ih, w_hh, b, b)[0].clone()
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.set_status_word(status)
    def abort_word(reserve):
        off = _lib.lib().halo_lstm_status_offset(0, T, B, in0, H, L)
        return int(reserve.view(torch.int32)[off // 4].item())
    try:
        _lib.check(_lib.lib().halo_debug_mute_workgroup(5), 'mute')
        y, _, _, reserve = ops.lstm_fwd(x, w_ih, w_hh, b, b)
        torch.cuda.synchronize()
        res['muted_abort'] = np.array([abort_word(reserve)]); res['muted_status'] = np.array([int(status.item())])
        _lib.check(_lib.lib().halo_debug_mute_workgroup(-1), 'unmute')
        status.zero_()
        y, _, _, reserve = ops.lstm_fwd(x, w_ih, w_hh, b, b)
        torch.cuda.synchronize()
        res['next_abort'] = np.array([abort_word(reserve)]); res['next_status'] = np.array([int(status.item())])
        res['next_equal'] = np.array([int(torch.equal(y, clean))])
    finally:
        _lib.lib().halo_debug_mute_workgroup(-1)
        _lib.set_status_word(None)
np.savez(out, **res)
'''


def _run(tmp_path, what, dataflag, timeout=600):
    out = str(tmp_path / f'{what}_{dataflag}.npz')
    env = dict(os.environ, DF_ROOT=ROOT, HALO_PERSIST_DATAFLAG=str(dataflag))
    r = subprocess.run([sys.executable, '-c', _CHILD, out, what], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    return dict(np.load(out))


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


def test_lstm_op_bitwise_equal_to_epoch_words(tmp_path):
    """H in {256, 1024}, B in {16, 48, 64}, T in {1, 2, 21}, dropout off and on, one process per setting running the 36 calls in a row
    (every change of B or T re-arms): outputs, final states, input and weight gradients bit for bit."""
    _same_bits(_run(tmp_path, 'grid', 1), _run(tmp_path, 'grid', 0))


def test_trainer_steps_bitwise_equal_to_epoch_words(tmp_path):
    """Three full LstmCtcTrainer steps at the benchmark's shape (LC-2x1024, B = 64, ragged lengths, graph replay): every step's loss,
    the parameters and both Adam moments bit for bit."""
    _same_bits(_run(tmp_path, 'trainer', 1), _run(tmp_path, 'trainer', 0))


def test_each_call_rearms(tmp_path):
    """Two calls of one shape with different inputs in one process: the second gives what it gives alone in a fresh process."""
    twice, once = _run(tmp_path, 'twice', 1), _run(tmp_path, 'once', 1)
    second = {k: v for k, v in twice.items() if k.startswith('second/')}
    _same_bits(second, once)


def test_mute_workgroup_is_bounded_and_loud(tmp_path):
    """A forward workgroup that never stores its pieces (halo_debug_mute_workgroup): its peers' bounded reloads give up, the call's
    abort word and the caller's sticky status word are raised, the call returns; the next, unmuted call is clean and exact."""
    r = _run(tmp_path, 'mute', 1)
    assert int(r['muted_abort'][0]) != 0 and int(r['muted_status'][0]) != 0
    assert int(r['next_abort'][0]) == 0 and int(r['next_status'][0]) == 0
    assert int(r['next_equal'][0]) == 1
