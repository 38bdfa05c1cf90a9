"""The float64 yardstick of the fused transducer loss (tests/rnnt_loss_ref.py) against the pinned fp32 oracle lattice
(oracle/star_ref.py), before a GPU is involved, and the argument checks of the two entry points of csrc/rnnt_loss.hip, which return
before any launch.  CPU only.

    losses: the helper's agree with star_ref.transducer_forward_score on the dense fp32 log-softmax joint (rtol 1e-5, atol 1e-4)
    df, dg: equal the broadcast sums of star_ref.transducer_grad pushed through a log-softmax backward (rtol 1e-4, atol 5e-6)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rnnt_loss_ref as R
from oracle import star_ref

CASES = {
    # N, T, U1, V, f_lengths, target_lengths, seed, repeat_label
    'ragged': (3, 7, 5, 37, [7, 1, 4], [4, 0, 2], 41, True),
    'full': (2, 9, 4, 12, None, None, 42, False),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_helper_matches_the_fp32_oracle_lattice(name):
    N, T, U1, V, fl_, tl_, seed, rep = CASES[name]
    f, g, tg, fl, tl, w = R.make_case(N, T, U1, V, fl_, tl_, seed, rep)
    losses, df, dg = R.transducer_loss_ref(f, g, tg, fl, tl, w)
    f32, g32 = f.clone().requires_grad_(True), g.clone().requires_grad_(True)
    joint = (f32[:, :, None, :] + g32[:, None, :, :]).log_softmax(-1)
    ref_l = star_ref.transducer_forward_score(joint.detach(), tg, fl, tl)
    joint.backward(gradient=star_ref.transducer_grad(joint.detach(), tg, fl, tl) * w[:, None, None, None])
    np.testing.assert_allclose(losses.numpy(), ref_l.numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(df.numpy(), f32.grad.numpy(), rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(dg.numpy(), g32.grad.numpy(), rtol=1e-4, atol=5e-6)
    # rows past the lengths carry no gradient in the yardstick either
    for n in range(N):
        assert not df[n, int(fl[n]):].any() and not dg[n, int(tl[n]) + 1:].any()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from haloop_amd import _lib
    lib = _lib.lib()
    N, T, U1, V = 2, 3, 3, 8
    fbuf, gbuf = (C.c_float * (N * T * V))(), (C.c_float * (N * U1 * V))()
    tg, fl, tl = (C.c_int64 * (N * (U1 - 1)))(), (C.c_int * N)(), (C.c_int * N)()
    lse, lp2 = (C.c_float * (N * T * U1))(), (C.c_float * (2 * N * T * U1))()
    a = lambda b: C.addressof(b)

    def fwd(f=a(fbuf), f_ns=T * V, f_ts=V, g=a(gbuf), g_ns=U1 * V, g_us=V, N=N, T=T, U1=U1, V=V, lse=a(lse), lp2=a(lp2)):
        return lib.halo_rnnt_joint_fwd(f, f_ns, f_ts, g, g_ns, g_us, N, T, U1, V, a(tg), a(fl), a(tl), lse, lp2, None)

    def bwd(V=V, d=a(lp2), df=a(fbuf), dg=a(gbuf), dg_ns=U1 * V, dg_us=V):
        return lib.halo_rnnt_joint_bwd(a(fbuf), T * V, V, a(gbuf), U1 * V, V, N, T, U1, V, a(tg), a(fl), a(tl), a(lse), d, df, T * V, V,
                                       dg, dg_ns, dg_us, None)

    EINVAL = -22
    assert fwd(f=None) == EINVAL and fwd(g=None) == EINVAL and fwd(lse=None) == EINVAL and fwd(lp2=None) == EINVAL
    assert fwd(N=0) == EINVAL and fwd(T=0) == EINVAL and fwd(U1=1) == EINVAL and fwd(V=0) == EINVAL and fwd(V=8193) == EINVAL
    assert fwd(U1=7680) == EINVAL                              # past the lattice kernels' bound
    assert fwd(f_ts=V - 1) == EINVAL and fwd(g_ns=V, g_us=V) == EINVAL        # rows that overlap
    assert bwd(d=None) == EINVAL and bwd(df=None) == EINVAL and bwd(dg=None) == EINVAL and bwd(V=0) == EINVAL
    assert bwd(dg_ns=V, dg_us=V) == EINVAL


def test_the_switch_defaults_to_off_and_is_read_when_the_head_is_built(monkeypatch):
    from haloop_amd import recognizer
    monkeypatch.delenv('HALO_RNNT_LOSS_FUSED', raising=False)
    assert recognizer.Transducer(8, 5).fused_loss is False
    monkeypatch.setenv('HALO_RNNT_LOSS_FUSED', '1')
    head = recognizer.Transducer(8, 5)
    assert head.fused_loss is True and 'fused_loss' not in head.state_dict()
