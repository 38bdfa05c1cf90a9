"""tests/attention_ref.py checked on the CPU: the float64 reference equals scaled_dot_product_attention / autograd in float64; the dropout
multipliers have the right share and move with stream and offset; on every dropout case of tests/test_gpu_attention_ref.py each
deliberately wrong dropout index is rejected by that case's gates in every mode, output by output; the peaked inputs make the blocks
re-reference (and their randn baselines do not); and the mask probes recover the multipliers exactly from the reference's outputs."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import attention_ref as R


@pytest.mark.parametrize('hd,heads,N,Tq,Tk,causal,lens', [(16, 2, 2, 9, 70, False, (70, 3)), (32, 3, 2, 40, 40, True, None),
                                                          (64, 1, 3, 20, 33, True, (33, 20, 14)), (8, 2, 1, 5, 5, False, None)])
def test_reference_equals_float64_sdpa_and_autograd(hd, heads, N, Tq, Tk, causal, lens):
    g = torch.Generator().manual_seed(Tq + Tk)
    C = heads * hd
    q, k, v, dy = (torch.randn(N * n, C, generator=g, dtype=torch.float64) for n in (Tq, Tk, Tk, Tq))
    y, lse = R.attention_ref(q, k, v, N, heads, hd, Tq, Tk, causal, lens)
    dq, dk, dv = R.attention_grads_ref(q, k, v, N, heads, hd, Tq, Tk, causal, lens, dy)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    vis = R.visible(N, Tq, Tk, causal, lens)
    want = Fn.scaled_dot_product_attention(R.split_heads(ql, N, Tq, heads, hd), R.split_heads(kl, N, Tk, heads, hd),
                                           R.split_heads(vl, N, Tk, heads, hd), attn_mask=vis)
    want = R.merge_heads(want)
    want.backward(dy)
    s = (R.split_heads(q, N, Tq, heads, hd) @ R.split_heads(k, N, Tk, heads, hd).transpose(-1, -2)) / math.sqrt(hd)
    np.testing.assert_allclose(y.numpy(), want.detach().numpy(), atol=1e-13, rtol=1e-12)
    np.testing.assert_allclose(lse.numpy(), torch.logsumexp(s.masked_fill(~vis, float('-inf')), -1).numpy(), atol=1e-13)
    for got, w in ((dq, ql.grad), (dk, kl.grad), (dv, vl.grad)):
        np.testing.assert_allclose(got.numpy(), w.numpy(), atol=1e-13, rtol=1e-12)
    # the same attention stated in log2 units on a pre-scaled q
    c = R.LOG2E / math.sqrt(hd)
    y2, lse2 = R.attention_ref(q * c, k, v, N, heads, hd, Tq, Tk, causal, lens, log2_units=True)
    g2 = R.attention_grads_ref(q * c, k, v, N, heads, hd, Tq, Tk, causal, lens, dy, log2_units=True)
    np.testing.assert_allclose(y2.numpy(), y.numpy(), atol=1e-12)
    np.testing.assert_allclose(lse2.numpy(), lse.numpy(), atol=1e-12)
    for got, w in zip(g2, (dq, dk, dv)):
        np.testing.assert_allclose(got.numpy(), w.numpy(), atol=1e-12)


def test_multipliers_act_after_the_softmax_and_stay_constant():
    """y = (softmax(s) * mult) v with lse of the undropped scores; dv = (softmax(s) * mult)^T dy."""
    N, heads, hd, Tq, Tk = 1, 1, 8, 4, 6
    g = torch.Generator().manual_seed(0)
    q, k, v, dy = (torch.randn(n, hd, generator=g, dtype=torch.float64) for n in (Tq, Tk, Tk, Tq))
    mult = R.drop_mult(N, heads, Tq, Tk, 0.5, 3, 1, 0)
    assert 0 < (mult == 0).sum() < mult.size
    y, lse = R.attention_ref(q, k, v, N, heads, hd, Tq, Tk, False, None, mult)
    p = torch.softmax(q @ k.T / math.sqrt(hd), -1) * torch.from_numpy(mult[0, 0]).double()
    np.testing.assert_allclose(y.numpy(), (p @ v).numpy(), atol=1e-14)
    np.testing.assert_allclose(lse.numpy()[0, 0], torch.logsumexp(q @ k.T / math.sqrt(hd), -1).numpy(), atol=1e-14)
    _, _, dv = R.attention_grads_ref(q, k, v, N, heads, hd, Tq, Tk, False, None, dy, mult)
    np.testing.assert_allclose(dv.numpy(), (p.T @ dy).numpy(), atol=1e-14)


@pytest.mark.parametrize('p', [0.1, 0.2])
def test_drop_mult_share_streams_offsets_and_variants(p):
    N, heads, Tq, Tk = 2, 3, 70, 150
    m = R.drop_mult(N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET)
    assert m.shape == (N, heads, Tq, Tk) and set(np.unique(m)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    n = m.size
    assert abs((m == 0).mean() - p) <= 4 * math.sqrt(p * (1 - p) / n)                   # within 4 sigma of p
    for other in (R.drop_mult(N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID + 1, R.OFFSET), R.drop_mult(N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET + 1),
                  R.drop_mult(N, heads, Tq, Tk, p, R.SEED + 1, R.STREAM_ID, R.OFFSET)):
        # independent draws disagree on a share 2 p (1 - p); 4 sigma around it
        d = (other != m).mean()
        assert abs(d - 2 * p * (1 - p)) <= 4 * math.sqrt(2 * p * (1 - p) / n), d
    assert np.array_equal(R.drop_mult_variant('right', N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET), m)
    assert np.array_equal(R.drop_mult_variant('right', N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET, batches=[1]), m[1:2])
    assert np.array_equal(R.drop_mult_variant('stream+1', N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET),
                          R.drop_mult(N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID + 1, R.OFFSET))
    for kind in R.WRONG_MASKS:
        assert not np.array_equal(R.drop_mult_variant(kind, N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET), m)
    # the wrong tile number moves tile t + 1's draws to tile t
    w = R.drop_mult_variant('tile+1', N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET)
    assert np.array_equal(w[..., :64], m[..., 64:128])


def _teeth(case, p, batch=None):
    """Every wrong mask moves EVERY output (y, dq, dk, dv) past the case's gate, in every mode: a wrong index in one kernel alone
    (the forward, the dQ sweep or the dK/dV sweep) cannot hide behind the others."""
    hd, heads, N, Tq, Tk, causal, lens = case
    q, k, v, dy = R.case_inputs(hd, heads, N, Tq, Tk)
    sub = None
    if batch is not None:                                        # one batch entry of a large case: its own rows, its own multipliers
        q, k, v, dy = (t[batch * n:(batch + 1) * n] for t, n in ((q, Tq), (k, Tk), (v, Tk), (dy, Tq)))
        sub, Nr = [batch], 1
        lens = None if lens is None else lens[batch:batch + 1]
    else:
        Nr = N
    masks = {kind: R.drop_mult_variant(kind, N, heads, Tq, Tk, p, R.SEED, R.STREAM_ID, R.OFFSET, batches=sub) for kind in ('right',) + R.WRONG_MASKS}
    for mode in R.MODES if batch is None else ('bf16',):
        qr, kr, vr, dyr, l2 = R.reference_operands(mode, hd, q, k, v, dy)
        outs = {}
        for kind, m in masks.items():
            y, _ = R.attention_ref(qr, kr, vr, Nr, heads, hd, Tq, Tk, causal, lens, m, l2)
            outs[kind] = (y,) + tuple(R.attention_grads_ref(qr, kr, vr, Nr, heads, hd, Tq, Tk, causal, lens, dyr, m, l2))
        gates = (R.fwd_gate(mode, hd, p, float(torch.as_tensor(vr).abs().max())),) + (R.bwd_gate(mode, hd, p),) * 3
        for kind in R.WRONG_MASKS:
            for name, got, want, (atol, rtol) in zip(('y', 'dq', 'dk', 'dv'), outs[kind], outs['right'], gates):
                assert R.exceeds(got.numpy(), want.numpy(), atol, rtol), (mode, kind, name)
                assert float((got - want).abs().max()) > 2 * atol, (mode, kind, name)


@pytest.mark.parametrize('p', R.DROPOUT_PS)
@pytest.mark.parametrize('case', R.DROPOUT_CASES, ids=lambda c: 'hd%d-%dx%d' % (c[0], c[3], c[4]))
def test_wrong_dropout_indices_are_rejected_by_the_gpu_gates(case, p):
    _teeth(case, p)


def test_wrong_dropout_indices_are_rejected_on_the_default_dispatch_case():
    """The 257-token bf16 case, on its last batch entry (the largest Philox indices)."""
    _teeth(R.BIG_CASE, R.BIG_P, batch=R.BIG_CASE[2] - 1)


@pytest.mark.parametrize('case', R.PEAKED_CASES, ids=lambda c: '%s-hd%d-%dx%d-%s' % (c[0], c[1], c[2], c[3], 'causal' if c[4] else 'full'))
def test_peaked_inputs_re_reference_and_their_baselines_do_not(case):
    kind, hd, Tq, Tk, causal, lens = case
    N, heads = R.PEAKED_N, R.PEAKED_HEADS
    q, k, v = R.peaked_inputs(kind, N, heads, Tq, Tk, hd, R.PEAKED_SEED)
    q0, k0, v0 = R.peaked_inputs('randn', N, heads, Tq, Tk, hd, R.PEAKED_SEED)
    assert torch.equal(v, v0) and float(q.abs().max()) < 8 and float(k.abs().max()) < 8
    blocks = N * heads * ((Tq + R.BLOCK - 1) // R.BLOCK)
    assert R.later_rebase_blocks(q0, k0, hd, causal, lens, N) == (0, blocks)
    later, total = R.later_rebase_blocks(q, k, hd, causal, lens, N)
    assert total == blocks
    if kind == 'descend':
        assert later == 0                                        # underflow of the later tiles, not rescaling
    elif causal:
        assert 2 * later >= blocks                               # the blocks of the first query tile see one key tile only
    else:
        assert later == blocks
    # the scores are as peaked as stated: some query's best key leads by tens of nats
    _, lse = R.attention_ref(q, k, v, N, heads, hd, Tq, Tk, causal, lens)
    _, lse0 = R.attention_ref(q0, k0, v0, N, heads, hd, Tq, Tk, causal, lens)
    if kind == 'descend':
        first = tuple(min(64, n) for n in (lens or (Tk,) * N))
        _, lse1 = R.attention_ref(q, k, v, N, heads, hd, Tq, Tk, causal, first)
        assert 0 < float((lse - lse1).max()) < 1e-2              # the first tile decides every row: the later ones underflow against it
    else:
        assert 25 < float(lse.max()) < 40 and float(lse0.max()) < 8
    ratio = R.score_magnitude(q, k, hd, causal, lens, N) / R.score_magnitude(q0, k0, hd, causal, lens, N)
    assert 3 <= ratio <= 5, ratio


def test_rebase_rule_emulation_on_hand_made_scores():
    """One head of dimension 1 (scores = q k * log2 e), two tiles: the rule per block, a single lane, a hidden tile."""
    def run(qv, kv, causal=False, lens=None):
        q = torch.tensor(qv, dtype=torch.float64)[:, None] / R.LOG2E         # scores in log2 units = qv * kv
        return R.later_rebase_blocks(q, torch.tensor(kv, dtype=torch.float64)[:, None], 1, causal, lens, 1)
    k = [0.0] * 64 + [1.0] * 64
    assert run([8.0] * 16, k) == (0, 1)                          # exactly REBASE above: stays
    assert run([8.01] * 16, k) == (1, 1)
    assert run([0.0] * 15 + [9.0], k) == (1, 1)                  # any lane of the block
    assert run([0.0] * 16 + [9.0] * 3, k) == (1, 2)              # the second block alone
    assert run([-9.0] * 16, k) == (0, 1)                         # falling scores never move the reference
    assert run([9.0] * 16, k, lens=[64]) == (0, 1)               # the second tile is hidden


@functools.lru_cache(maxsize=None)
def _probe_mult(N, heads, Tq, Tk):
    return R.drop_mult(N, heads, Tq, Tk, R.PROBE_P, R.SEED, R.STREAM_ID, R.OFFSET)


@pytest.mark.parametrize('which', ['fwd', 'dq', 'dkv'])
@pytest.mark.parametrize('case', R.PROBE_CASES, ids=lambda c: '%dx%d' % (c[2], c[3]))
def test_probe_algebra_recovers_the_multipliers_from_the_reference(case, which):
    N, heads, Tq, Tk, causal, lens = case
    mult = _probe_mult(N, heads, Tq, Tk)
    est = np.full(mult.shape, np.nan, dtype=np.float32)
    for tile in R.probe_tiles(which, Tq, Tk):
        q, k, v, dy = R.probe_inputs(which, N, heads, Tq, Tk, tile)
        y, lse = R.attention_ref(q, k, v, N, heads, R.PROBE_HD, Tq, Tk, causal, lens, mult)
        np.testing.assert_allclose(lse.numpy(), np.log(R.visible(N, Tq, Tk, causal, lens).sum(-1).double().numpy()).repeat(heads, 1), atol=1e-13)
        dq, dk, dv = R.attention_grads_ref(q, k, v, N, heads, R.PROBE_HD, Tq, Tk, causal, lens, dy, mult)
        R.probe_decode(which, {'fwd': y, 'dq': dq, 'dkv': dv}[which], y, N, heads, Tq, Tk, causal, lens, R.PROBE_P, tile, est)
    vis = np.broadcast_to(R.visible(N, Tq, Tk, causal, lens).numpy(), mult.shape)
    assert not np.isnan(est[vis]).any()
    np.testing.assert_array_equal(est[vis], mult[vis])
    # and a wrong index does not pass: the probes are exact, one flipped element is a failure
    wrong = R.drop_mult_variant('tile+1', N, heads, Tq, Tk, R.PROBE_P, R.SEED, R.STREAM_ID, R.OFFSET)
    assert (est[vis] != wrong[vis]).any()


@pytest.mark.parametrize('case', R.PEAKED_CASES, ids=lambda c: '%s-hd%d-%dx%d-%s' % (c[0], c[1], c[2], c[3], 'causal' if c[4] else 'full'))
def test_a_broken_re_reference_is_rejected_by_the_peaked_gates(case):
    """The tiled forward with the kernels' re-reference rule, in float64: equal to the reference as it stands; with the rescale of the
    output or of the normaliser left out y is further from it than the loosest gate of the GPU file (bf16: 2^-8 max|v|), with the moved
    reference lost lse is (the loosest lse gate times A / A0, relative to max|lse|), on every case that re-references -- and nothing changes
    on 'descend', which never does."""
    kind, hd, Tq, Tk, causal, lens = case
    N, heads = R.PEAKED_N, R.PEAKED_HEADS
    q, k, v = R.peaked_inputs(kind, N, heads, Tq, Tk, hd, R.PEAKED_SEED)
    y, lse = R.attention_ref(q, k, v, N, heads, hd, Tq, Tk, causal, lens)
    y0, lse0 = R.tiled_forward_emulation(q, k, v, hd, causal, lens, N)
    np.testing.assert_allclose(y0.numpy(), y.numpy(), atol=1e-12)
    np.testing.assert_allclose(lse0.numpy(), lse.numpy(), atol=1e-12)
    gate = R.fwd_gate('bf16', hd, 0.0, float(v.abs().max()))[0]
    q0, k0, _ = R.peaked_inputs('randn', N, heads, Tq, Tk, hd, R.PEAKED_SEED)
    lse_gate = max(R.lse_gate(m, hd)[0] for m in R.MODES) * max(1.0, R.score_magnitude(q, k, hd, causal, lens, N) / R.score_magnitude(q0, k0, hd, causal, lens, N))
    for bug in R.TILED_BUGS:
        yb, lseb = R.tiled_forward_emulation(q, k, v, hd, causal, lens, N, bug=bug)
        if kind == 'descend':
            assert torch.equal(yb, y0) and torch.equal(lseb, lse0)
        elif bug == 'mref':                                      # the lost reference shows in lse = m_ref ln 2 + log(sum)
            assert float((lseb - lse).abs().max()) > 2 * lse_gate * float(lse.abs().max()), bug
        else:
            assert float((yb - y).abs().max()) > 2 * gate, bug
