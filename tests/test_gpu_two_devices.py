"""The dynamic-LDS opt-in is per device (csrc/dyn_lds.h): a large-LDS kernel that has already run on cuda:0 must launch on cuda:1 of the
same process, and give the same bits there."""
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs in one process: the opt-in is per device')]


def _on_both_devices(mode, run):
    """run(device) under ``mode`` on cuda:0, then with cuda:1 current; the math mode and the current device are restored."""
    from haloop_amd import _lib
    _lib.lib()
    prev_mode, prev_dev = _lib.get_math_mode(), torch.cuda.current_device()
    _lib.set_math_mode(mode)
    try:
        torch.cuda.set_device(0)
        first = run('cuda:0')
        with torch.cuda.device(1):
            second = run('cuda:1')
        return first, second
    finally:
        _lib.set_math_mode(prev_mode)
        torch.cuda.set_device(prev_dev)


def test_head_greedy_on_a_second_device():
    """ctc_head_fwd_kernel<true> (exact-f32 mode) asks for 131,328 bytes of dynamic LDS."""
    from haloop_amd import ops
    from oracle import lattice
    B, T, H, V = 3, 5, 64, 8
    g = torch.Generator().manual_seed(B * 7 + T)
    feats = torch.randn(B, T, H, generator=g)
    W = torch.randn(V, H, generator=g) * H ** -0.5
    W[0] += 0.02 * feats.mean((0, 1))            # some blanks among the winners
    b = 0.1 * torch.randn(V, generator=g)

    def run(dev):
        out = ops.ctc_head_greedy(feats.to(dev), W.to(dev), b.to(dev), want_lp=True)
        torch.cuda.synchronize()
        return out

    first, second = _on_both_devices('f32', run)
    for x0, x1 in zip(first, second):
        assert x1.device.index == 1 and torch.equal(x0.cpu(), x1.cpu())
    ali, scores, hyp, hyp_len, lp = second
    hyps, lengths, alignments, best = lattice.greedy_decode(lp.cpu())
    assert torch.equal(ali.cpu(), alignments) and torch.equal(hyp_len.cpu(), lengths) and torch.equal(scores.cpu(), best)
    for n in range(B):
        assert hyp[n, :lengths[n]].tolist() == hyps[n] and not hyp[n, lengths[n]:].any()


def test_split_gemm_on_a_second_device():
    """One 128 x 128 tile, one k-tile (no split-K, no scratch): gemm_bf16x3_kernel<2, 3, false, 1> on its two-slot ring of 64 KiB."""
    from haloop_amd import ops
    M, N, K = 128, 128, 32
    g = torch.Generator().manual_seed(M + N + K)
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)

    def run(dev):
        out = ops.gemm_split(ops.split_image(a.to(dev)), ops.split_image(b.to(dev)), M, N, K)
        torch.cuda.synchronize()
        return out

    first, second = _on_both_devices('bf16x3', run)
    assert second.device.index == 1 and torch.equal(first.cpu(), second.cpu())
    ref = (a.double() @ b.double().t()).float()
    tol = 3e-5 * float(ref.abs().max())          # the bound of test_split_gemm_many_tiles_ring_variants in bf16x3 mode
    assert float((second.cpu() - ref).abs().max()) <= tol
