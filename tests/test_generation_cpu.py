"""CPU-side checks of haloop_amd.generation: the draw as include/halo.h defines it (restated in float64 on oracle/philox.py, the same
restatement tests/test_gpu_generation.py holds the kernel to) samples the softmax, and the documented errors are raised on the host."""
import numpy as np
import pytest
import torch


def restated_draws(logits, steps, temperature, top_k, seed, row=0):
    """Tokens of row ``row`` at steps 0 .. steps - 1: u = (philox4x32_10(ctr = (row, 0, stream, step), key = seed)[0] >> 8) * 2^-24, the
    token is the smallest index whose cumulative kept mass exceeds u * total."""
    from haloop_amd import _lib
    from oracle import philox
    s = np.arange(steps, dtype=np.uint32)
    z = np.zeros_like(s)
    r = philox.philox4x32_10(np.full_like(s, row), z, np.full_like(s, _lib.HALO_GPT_SAMPLE_STREAM), s, seed & 0xFFFFFFFF, seed >> 32)[0]
    u = (r >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    l = np.asarray(logits, dtype=np.float64)
    keep = np.ones_like(l, dtype=bool) if top_k is None else l >= np.sort(l)[-min(top_k, len(l))]
    e = np.where(keep, np.exp(l / temperature - (l / temperature).max()), 0.0)
    cdf = np.cumsum(e)
    return np.searchsorted(cdf, u * cdf[-1], side='right'), e / cdf[-1]


def test_restated_draw_samples_the_softmax():
    logits = np.array([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.9, -2.5])
    n = 20000
    tokens, probs = restated_draws(logits, n, 0.8, None, 0xC0FFEE1234)
    counts = np.bincount(tokens, minlength=8)
    chi2 = float(((counts - n * probs) ** 2 / (n * probs)).sum())
    assert chi2 < 24.32, (chi2, counts)               # 7 degrees of freedom, p = 0.001
    # top-k keeps the k largest (ties at the threshold stay) and never draws the rest
    tied = np.array([1.0, 3.0, 2.0, 2.0, 0.5, 2.0, -1.0, 0.0])
    tokens, probs = restated_draws(tied, 4000, 1.0, 2, 5)
    assert set(np.unique(tokens)) == {1, 2, 3, 5} and probs[[0, 4, 6, 7]].sum() == 0.0
    tokens, _ = restated_draws(tied, 64, 1.0, 1, 5)
    assert (tokens == 1).all()
    # the stream is a function of (seed, row, step)
    a, _ = restated_draws(logits, 256, 1.0, None, 9)
    b, _ = restated_draws(logits, 256, 1.0, None, 9)
    c, _ = restated_draws(logits, 256, 1.0, None, 10)
    d, _ = restated_draws(logits, 256, 1.0, None, 9, row=1)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)


def tiny_model():
    from haloop_amd import attention
    return attention.GPT(attention.GPTConfig(block_size=32, vocab_size=64, n_layer=1, n_head=2, n_embd=64)).eval()


def test_sampler_errors_on_the_host():
    from haloop_amd import _lib, generation
    model = tiny_model()
    sampler = generation.Sampler(model, 2, max_len=24)
    assert sampler.cache.shape == (1, 2, 2, 2, 24, 32) and sampler.cache.dtype == torch.float32
    ids = torch.ones(2, 8, dtype=torch.long)
    with pytest.raises(ValueError):
        sampler.sample(torch.ones(3, 8, dtype=torch.long), 4)         # B > max_batch
    with pytest.raises(ValueError):
        sampler.sample(ids, 17)                                       # P + max_new_tokens > max_len
    with pytest.raises(ValueError):
        sampler.prefill(torch.ones(2, 25, dtype=torch.long))
    with pytest.raises(_lib.HaloError):
        sampler.sample(ids, 4)                                        # a CPU tensor
    with pytest.raises(_lib.HaloError):
        sampler.prefill(ids)
    with pytest.raises(ValueError):
        generation.Sampler(model, 2, max_len=64)                      # beyond the position table


def test_generate_checks_before_the_first_next():
    from haloop_amd import _lib, generation
    model = tiny_model()
    ids = torch.ones(1, 8, dtype=torch.long)
    with pytest.raises(ValueError):
        generation.generate(model, ids, 25)                           # raised by the call, not by the first next()
    with pytest.raises(ValueError):
        generation.generate(model, torch.ones(2, 8, dtype=torch.long), 4)
    with pytest.raises(_lib.HaloError):
        generation.generate(model, ids, 4)


def test_sample_stream_id_is_outside_the_other_sites():
    from haloop_amd import _lib
    assert _lib.HALO_ABI_VERSION == 21
    assert _lib.HALO_GPT_SAMPLE_STREAM > 4096 + 4096                  # dropout sites: small integers; LoRA sites: 4096 + layer
    text = open(_lib.LIB_PATH.replace('haloop_amd/csrc/libhalo.so', 'include/halo.h')).read()
    assert f'#define HALO_GPT_SAMPLE_STREAM 0x{_lib.HALO_GPT_SAMPLE_STREAM:08X}u' in text
