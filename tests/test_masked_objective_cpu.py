"""CPU-side checks of the masked objective: the capacity rule, GPT.set_target_capacity's footprint, the stream constant, and the counts
of the draws' numpy restatement (tests/test_gpu_mlm.py) that the GPU tests compare the kernels with."""
import numpy as np
import pytest
import torch

from test_gpu_mlm import SEED, masked_batch


def test_target_capacity_arithmetic():
    from haloop_amd import symbol_tape
    assert symbol_tape.target_capacity(64, 128) == 1536
    assert symbol_tape.target_capacity(64, 128, 0.15) == 1536
    for B, T, p in [(1, 1, 0.15), (4, 32, 0.15), (8, 1024, 0.15), (64, 128, 0.3), (3, 130, 0.5), (32, 512, 0.05)]:
        M = B * T
        cap = symbol_tape.target_capacity(B, T, p)
        bound = p * M + 8.0 * (M * p * (1.0 - p)) ** 0.5
        assert cap % 256 == 0 and cap >= bound and cap - 256 < bound, (B, T, p, cap)


def test_set_target_capacity_is_not_state():
    from haloop_amd import attention
    model = attention.GPT(attention.GPTConfig(block_size=16, vocab_size=32, n_layer=1, n_head=2, n_embd=16, causal=False))
    keys = list(model.state_dict())
    assert model._target_capacity is None
    model.set_target_capacity(100)
    assert model._target_capacity == 100
    assert model._compact_rows(8192) == (128, 100)                    # rounded up to the weight-gradient products' contraction step
    assert list(model.state_dict()) == keys
    model.set_target_capacity(16)
    K, limit = model._compact_rows(128)                               # never down to the small-M kernels while the dense head is above them
    assert limit == 16 and K % 32 == 0 and K > attention.SMALL_M
    assert model._compact_rows(32) == (32, 16)
    model.set_target_capacity(None)
    assert model._target_capacity is None and list(model.state_dict()) == keys
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError):
            model.set_target_capacity(bad)


def test_mlm_stream_constant_and_cpu_refusal():
    from haloop_amd import _lib, mlm
    assert _lib.HALO_MLM_STREAM == 0x4D4C4D31 and _lib.HALO_MLM_STREAM != _lib.HALO_GPT_SAMPLE_STREAM
    text = open(_lib.LIB_PATH.replace('haloop_amd/csrc/libhalo.so', 'include/halo.h')).read()
    assert f'#define HALO_MLM_STREAM 0x{_lib.HALO_MLM_STREAM:08X}u' in text
    with pytest.raises(_lib.HaloError):
        mlm.mask_tokens(torch.ones(2, 8, dtype=torch.long), seed=1)


@pytest.mark.parametrize('B,T,V,selected', [(64, 128, 2048, (1198, 1230)), (4, 32, 97, (21, 20)), (3, 130, 50257, (49, 61))])
def test_restatement_counts(B, T, V, selected):
    """The counts the GPU tests' shapes rest on (capacities 32 and 1536 hold them; 16 does not), from the restatement alone."""
    for step, want in zip((0, 3), selected):
        tokens, inputs, labels, masks = masked_batch(B, T, V, step)
        sel = masks['selected']
        assert int(sel.sum()) == want == int((labels != 0).sum())
        assert not sel[(tokens == V - 1).numpy()].any()
        assert int(inputs.max()) <= V - 1 and int(inputs.min()) >= 0
        if (B, T, V) == (64, 128, 2048):
            rep, rnd = masks['replaced'].sum() / sel.sum(), masks['random'].sum() / sel.sum()
            assert abs(rep - (0.776, 0.807)[step == 3]) < 1e-3 and abs(rnd - (0.123, 0.098)[step == 3]) < 1e-3
            assert int(inputs.max()) == 2047
