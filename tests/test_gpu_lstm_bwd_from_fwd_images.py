"""The two-layer LSTM backward building its W^T fragments from the FORWARD weight images (csrc/lstm_persist2.hip, wT_from_fwd;
halo_set_lstm_bwd_from_fwd_images, default on) against the launch that reads the three transposed images (switch off): the fragments
are the same bf16 values in the same registers and LDS slots, so every gradient is the same bits -- for the LSTM op, and for three
LstmCtcTrainer steps, whose packing launch then writes three images instead of six and must still feed every reader."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture
def bf16():
    from haloop_amd import _lib
    _lib.lib(); _lib.lend_scratch()
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16')
    yield _lib
    _lib.set_lstm_bwd_from_fwd_images(True)
    _lib.set_math_mode(prev)


# H = 256: the smallest eligible width, B = 20: a ragged last batch tile; H = 1024: the KC = 8 register and LDS layout of the benchmark
@pytest.mark.parametrize('T,B,H', [(3, 20, 256), (2, 16, 1024)])
def test_lstm_gradients_bitwise_equal_to_the_transposed_images(bf16, T, B, H):
    from haloop_amd import ops
    _lib = bf16
    L, in0 = 2, 128
    assert _lib.lib().halo_lstm_persistent2_eligible(T, B, H, L) == 1
    g = torch.Generator().manual_seed(100 + T + B + H)
    k = 1.0 / H ** 0.5
    x = torch.randn(T, B, in0, generator=g).to(DEV)
    w_ih = [((torch.rand(4 * H, in0 if l == 0 else H, generator=g) * 2 - 1) * k).to(DEV) for l in range(L)]
    w_hh = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(DEV) for l in range(L)]
    b_ih = [((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(DEV) for l in range(L)]
    b_hh = [((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(DEV) for l in range(L)]
    dy = torch.randn(T, B, H, generator=g).to(DEV)
    dhn = torch.randn(L, B, H, generator=g).to(DEV)
    dcn = torch.randn(L, B, H, generator=g).to(DEV)
    drop = ops.Dropout(0.2, 77, 1)
    outs = []
    for on in (True, False):
        _lib.set_lstm_bwd_from_fwd_images(on)
        y, hn, cn, reserve = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, want_state=True, drop=drop)
        dx, grads = ops.lstm_bwd(x, w_ih, w_hh, dy, (B * H, H), False, reserve, dhn=dhn, dcn=dcn, want_dx=True, drop=drop)
        torch.cuda.synchronize()
        assert 'lstm_persist2_bwd_kernel' in _lib.lstm_chain_info('bwd')['kernel']        # not a fallback path
        out = {'y': y, 'hn': hn, 'cn': cn, 'dx': dx}
        for name, lst in grads.items():
            for l, t in enumerate(lst):
                out[f'{name}{l}'] = t
        outs.append({n: t.clone() for n, t in out.items()})
    assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]) == 4 + 4 * L
    for n in outs[0]:
        assert torch.isfinite(outs[0][n]).all(), n
        assert torch.equal(outs[0][n], outs[1][n]), n
    assert outs[0]['dw_hh0'].abs().max().item() > 0 and outs[0]['dw_ih1'].abs().max().item() > 0


def test_three_trainer_steps_bitwise_equal_to_the_transposed_images(bf16):
    """H = 256, B = 20, 16 frames (T' = 5), graph replay: losses, parameters and both Adam moments after three steps."""
    from haloop_amd import rnn, recognizer, synth
    from haloop_amd.train import LstmCtcTrainer
    _lib = bf16
    F_, C, H, L, V, B, T, S = 80, 128, 256, 2, 32, 20, 16, 2
    res = []
    for on in (True, False):
        _lib.set_lstm_bwd_from_fwd_images(on)
        enc_p, rec_p = synth.make_params(F_, C, H, L, V, 7)
        enc = rnn.Encoder(F_, C, H, num_layers=L); rec = recognizer.TemporalClassifier(H, V)
        enc.load_state_dict(enc_p); rec.load_state_dict(rec_p)
        enc.to(DEV).train(); rec.to(DEV).train()
        tr = LstmCtcTrainer(enc, rec, lr=1e-3, seed=11, use_graph=True)
        x, il, tg, tl = (t.to(DEV) for t in synth.synthetic_batch(B, T, F_, V, S, 3))
        first = tr.flat.params.clone()
        losses = []
        for _ in range(3):
            tr.step(x, il, tg, tl)
            torch.cuda.synchronize()
            losses.append(tr.loss.detach().clone().reshape(-1))
        tr.check_status()
        assert 'lstm_persist2_bwd_kernel' in _lib.lstm_chain_info('bwd')['kernel']
        assert int(tr.adam_step.item()) == 3 and not torch.equal(tr.flat.params, first)
        res.append((torch.cat(losses), tr.flat.params.clone(), tr.flat.exp_avg.clone(), tr.flat.exp_avg_sq.clone()))
    for a, b in zip(*res):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
