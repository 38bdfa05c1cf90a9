"""The front-end convolution's backward with its serial load latencies taken out (csrc/elementwise.hip: subsample_bwd_reduce_kernel adds
the row chunks' partials from eight loads in flight at a time, subsample_bwd_partial_kernel builds its masked-gradient tile three elements
per thread at a time and sums the bias columns under its matrix loads, eight LDS reads at a time): the additions keep their order, so the
results keep their bits -- ragged last chunks (84 and 420 rows), one and eight K-slices of dy -- checked against a float64 product
at the bound of test_gpu_lstm_b64.py::test_front_end_backward_in_two_launches (3e-6 of the largest entry), and byte for byte against
what the kernels gave before the change (tests/golden/subsample_bwd_b20_slabs8.npy, recorded on an MI355X)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'subsample_bwd_b20_slabs8.npy')
F_, C, KS, T_IN, P_DROP = 80, 128, 5, 80, 0.2          # 80 frames -> T' = 21 rows per utterance
GOLDEN_CASE = (20, 8)


def make_case(B, slabs):
    """dy as `slabs` K-slices [slabs, T', B, C], the conv's saved output y (its sign pattern is the mask) and im2col image, on the CPU."""
    Tp = (T_IN + 6 - KS) // 4 + 1
    g = torch.Generator().manual_seed(1000 + 10 * B + slabs)
    y = torch.relu(torch.randn(Tp, B, C, generator=g))
    col = torch.randn(Tp * B, F_ * KS, generator=g)
    dy = torch.randn(slabs, Tp, B, C, generator=g)
    return dy, y, col


def run_case(B, slabs):
    from haloop_amd import _lib, ops
    _lib.lib(); _lib.lend_scratch()
    dy, y, col = make_case(B, slabs)
    dw, db = ops.subsample_bwd(dy.to(DEV), y.to(DEV), col.to(DEV), B, T_IN, F_, C, P_DROP, slabs=slabs)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


@pytest.mark.parametrize('B', [4, 20])
@pytest.mark.parametrize('slabs', [1, 8])
def test_conv_backward_matches_float64(B, slabs):
    dy, y, col = make_case(B, slabs)
    dpre = dy.double().sum(0) * (y > 0).double() * (1.0 / (1.0 - P_DROP))
    dpre = dpre.reshape(-1, C)
    dw_ref, db_ref = dpre.t() @ col.double(), dpre.sum(0)
    dw, db = run_case(B, slabs)
    assert dw.shape == (C, F_, KS) and db.shape == (C,)
    np.testing.assert_allclose(dw.double().reshape(C, -1).numpy(), dw_ref.numpy(), rtol=0, atol=3e-6 * float(dw_ref.abs().max()))
    np.testing.assert_allclose(db.double().numpy(), db_ref.numpy(), rtol=0, atol=3e-6 * float(db_ref.abs().max()))


def test_conv_backward_keeps_its_bits():
    dw, db = run_case(*GOLDEN_CASE)
    want = np.load(GOLDEN)
    got = np.concatenate([dw.reshape(-1).numpy(), db.numpy()])
    assert want.dtype == np.float32 and want.shape == got.shape
    assert got.tobytes() == want.tobytes()
