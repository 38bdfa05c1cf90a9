"""Drop-in for ha/mlm.py: BERT-style token masking (80 % mask token, 10 % random token, 10 % unchanged) on the HIP device.

torch's CPU generator cannot be reproduced on the device, so the draws come from the library's own counter stream, keyed by
``(seed, step)`` -- the policy of the dropout masks (oracle/philox.py).  include/halo.h states the draw ("Token masking")."""
import torch

from . import _lib, ops


def mask_tokens(inputs, mlm_probability=0.15, mask_token=50254, endoftext_token=50256, max_token=50257, *, seed, step=0):
    """inputs [B, T] int64 on the device, modified in place and returned with labels [B, T] int64 (the original token where a
    position was selected, else 0), as ha/mlm.py:11-40 returns them."""
    if not isinstance(inputs, torch.Tensor) or not inputs.is_cuda:
        raise _lib.HaloError('haloop_amd.mlm.mask_tokens runs on the HIP device only (no CPU path)')
    if inputs.dtype != torch.int64 or not inputs.is_contiguous():
        raise ValueError('mask_tokens: inputs must be a contiguous int64 tensor')
    labels = ops.mask_tokens_(inputs, mlm_probability, mask_token, endoftext_token, max_token, seed, step)
    return inputs, labels
