"""Token masking on the device (haloop_amd.mlm.mask_tokens, symbol_tape.get_batch(..., 'denoise')) against a numpy restatement of the draws
that include/halo.h defines ("Token masking"), built on oracle/philox.py: bit-exact inputs and labels, the stream's behaviour under
(seed, step), and the refusals.  ``mlm_restatement`` and ``masked_batch`` are shared with tests/test_gpu_sparse_head.py and the CPU test of
the restatement's own counts (tests/test_masked_objective_cpu.py)."""
import numpy as np
import pytest
import torch

DEV = 'cuda'
SEED = 0x5EED0D15EA5E


def mlm_restatement(tokens, mlm_probability=0.15, mask_token=50254, endoftext_token=50256, max_token=50257, *, seed, step=0):
    """tokens: int64 numpy [B, T] -> (inputs, labels, masks) as include/halo.h states them; masks: selected / replaced / random."""
    from haloop_amd import _lib
    from oracle import philox
    tok = np.asarray(tokens, dtype=np.int64)
    e = np.arange(tok.size, dtype=np.uint64)
    r0, r1, r2, r3 = philox.philox4x32_10((e & np.uint64(0xFFFFFFFF)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32),
                                          np.full(tok.size, _lib.HALO_MLM_STREAM, dtype=np.uint32), np.full(tok.size, step, dtype=np.uint32),
                                          seed & 0xFFFFFFFF, seed >> 32)
    flat = tok.reshape(-1)
    selected = (flat != endoftext_token) & (r0 < philox.dropout_threshold(mlm_probability))
    replaced = selected & (r1 < philox.dropout_threshold(0.8))
    random = selected & ~replaced & (r2 < philox.dropout_threshold(0.5))
    words = ((r3.astype(np.uint64) * np.uint64(max_token)) >> np.uint64(32)).astype(np.int64)
    inputs = np.where(replaced, np.int64(mask_token), np.where(random, words, flat))
    labels = np.where(selected, flat, np.int64(0))
    masks = dict(selected=selected.reshape(tok.shape), replaced=replaced.reshape(tok.shape), random=random.reshape(tok.shape))
    return inputs.reshape(tok.shape), labels.reshape(tok.shape), masks


def raw_tokens(B, T, V):
    """The batch every masked-objective test starts from: tokens in [1, V), every 97th flat position the end-of-text token V - 1."""
    tokens = torch.randint(1, V, (B, T), generator=torch.Generator().manual_seed(18))
    tokens.view(-1)[::97] = V - 1
    return tokens


def masked_batch(B, T, V, step):
    """(raw tokens, masked inputs, labels, masks) of the restatement with mask_token = V - 3, endoftext = V - 1, max_token = V."""
    tokens = raw_tokens(B, T, V)
    inputs, labels, masks = mlm_restatement(tokens.numpy(), 0.15, V - 3, V - 1, V, seed=SEED, step=step)
    return tokens, torch.from_numpy(inputs), torch.from_numpy(labels), masks


@pytest.fixture(scope='module')
def lib():
    from haloop_amd import _lib
    _lib.lib()
    return _lib


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,V', [(3, 130, 50257), (64, 128, 2048)])
@pytest.mark.parametrize('step', [0, 3])
def test_mask_tokens_bit_exact(lib, B, T, V, step):
    from haloop_amd import mlm
    tokens = raw_tokens(B, T, V)
    kw = {} if V == 50257 else dict(mask_token=V - 3, endoftext_token=V - 1, max_token=V)        # (3, 130): ha/mlm.py's defaults
    want_in, want_lb, masks = mlm_restatement(tokens.numpy(), seed=SEED, step=step, **kw)
    x = tokens.to(DEV)
    out, labels = mlm.mask_tokens(x, seed=SEED, step=step, **kw)
    assert out is x and labels.dtype == torch.int64 and labels.shape == x.shape              # in place, as the reference
    assert np.array_equal(x.cpu().numpy(), want_in) and np.array_equal(labels.cpu().numpy(), want_lb)
    sel = torch.from_numpy(masks['selected'])
    assert sel.any() and torch.equal(labels.cpu(), torch.where(sel, tokens, torch.zeros_like(tokens)))
    assert not sel[tokens == V - 1].any() and (tokens == V - 1).any()                          # endoftext is never selected
    assert torch.equal(x.cpu()[~sel], tokens[~sel])
    assert int(x.max()) < V and int(x.min()) >= 0


@pytest.mark.gpu
def test_get_batch_denoise_bit_exact(lib, tmp_path):
    """One launch == the lm gather's x through mask_tokens with the same (seed, step): the tape and offsets of
    test_lm_get_batch_u16_bit_exact, and a row that runs past the tape's end."""
    from haloop_amd import mlm, symbol_tape
    from oracle import tape_ref
    rng = np.random.default_rng(5)
    tokens = rng.integers(0, 50257, size=20000).astype(np.uint16)
    tokens[rng.integers(0, 20000, size=3000)] = 0
    path = tmp_path / 'tokens.u16'
    tokens.tofile(path)
    data = symbol_tape.load_u16(path, DEV)
    offsets = torch.tensor([0, 17, 19000, 19999 - 64, 4242])
    plain = {}
    for objective in ('lm', 'cond'):                                                          # unchanged by the new keywords' defaults
        x, y = symbol_tape.get_batch(data, offsets, 64, objective)
        xr, yr = tape_ref.get_batch(tokens, offsets.tolist(), 64, objective)
        assert np.array_equal(x.cpu().numpy(), xr) and np.array_equal(y.cpu().numpy(), yr), objective
        plain[objective] = x
    past = torch.tensor([19990, 3])                                                           # a row that runs past the tape's end: zeros, which draw too
    xp, _ = symbol_tape.get_batch(data, past, 64, 'lm')
    assert (xp[0, 10:] == 0).all()
    for step in (0, 3):
        x, y = symbol_tape.get_batch(data, past, 64, 'denoise', seed=SEED, step=step, endoftext_token=50256)
        want_in, want_lb, masks = mlm_restatement(xp.cpu().numpy(), seed=SEED, step=step)
        assert np.array_equal(x.cpu().numpy(), want_in) and np.array_equal(y.cpu().numpy(), want_lb)
        assert masks['replaced'][0, 10:].any() and (x[0, 10:] == 50254).any()
    for step in (0, 3):
        x, y = symbol_tape.get_batch(data, offsets, 64, 'denoise', seed=SEED, step=step)
        xm, ym = mlm.mask_tokens(plain['lm'].clone(), seed=SEED, step=step)
        assert x.dtype == torch.int64 and torch.equal(x, xm) and torch.equal(y, ym)
        want_in, want_lb, _ = mlm_restatement(plain['lm'].cpu().numpy(), seed=SEED, step=step)
        assert np.array_equal(x.cpu().numpy(), want_in) and np.array_equal(y.cpu().numpy(), want_lb)
    x, y = symbol_tape.get_batch(data, offsets, 64, 'denoise', seed=SEED, step=1, mlm_probability=0.5, mask_token=7, endoftext_token=0, max_token=11)
    want_in, want_lb, _ = mlm_restatement(plain['lm'].cpu().numpy(), 0.5, 7, 0, 11, seed=SEED, step=1)
    assert np.array_equal(x.cpu().numpy(), want_in) and np.array_equal(y.cpu().numpy(), want_lb)


@pytest.mark.gpu
def test_stream_behaviour_and_refusals(lib):
    from haloop_amd import mlm, symbol_tape
    tokens = raw_tokens(4, 32, 97).to(DEV)
    kw = dict(mask_token=94, endoftext_token=96, max_token=97)
    a, la = mlm.mask_tokens(tokens.clone(), seed=SEED, step=0, **kw)
    b, lb = mlm.mask_tokens(tokens.clone(), seed=SEED, step=0, **kw)
    c, lc = mlm.mask_tokens(tokens.clone(), seed=SEED, step=1, **kw)
    d, ld = mlm.mask_tokens(tokens.clone(), seed=SEED + 1, step=0, **kw)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert not torch.equal(la, lc) and not torch.equal(la, ld)
    with pytest.raises(lib.HaloError):
        mlm.mask_tokens(tokens.cpu(), seed=SEED)
    data = torch.zeros(256, dtype=torch.int16, device=DEV)
    with pytest.raises(NotImplementedError):
        symbol_tape.get_batch(data, torch.tensor([0]), 16, 'foo')
    with pytest.raises(ValueError):
        symbol_tape.get_batch(data, torch.tensor([0]), 16, 'denoise')                         # no seed: no silent default stream


@pytest.mark.gpu
def test_masking_rates(lib):
    """(64, 128), V = 2048, step 0: the restatement on the CPU gives a selected share of 0.1462 and a replaced share of 0.776."""
    from haloop_amd import mlm
    B, T, V = 64, 128, 2048
    tokens = raw_tokens(B, T, V)
    x, labels = mlm.mask_tokens(tokens.to(DEV), mask_token=V - 3, endoftext_token=V - 1, max_token=V, seed=SEED, step=0)
    x, labels = x.cpu(), labels.cpu()
    selected = labels != 0
    share = float(selected.float().mean())
    replaced = float((x[selected] == V - 3).float().mean())
    print(f'selected share {share:.4f}, replaced share of selected {replaced:.4f}')
    assert abs(share - 0.15) <= 0.02
    assert abs(replaced - 0.8) <= 0.05
