"""The reference's feature pipeline for a whole batch on the HIP device (ha/data.py:103-151, the combinators ``fbank:``, ``mfcc:`` and
``mask:``): a ragged batch of waveforms in, padded features + lengths out, ready for ``Encoder.forward(inputs, input_lengths)``.

    fbank_batch(waveforms [N, L], lengths [N])   80-mel kaldi log filterbank                    1 launch
    mfcc_batch(waveforms, lengths)               kaldi MFCC (13 of 23) + utterance CMVN         2 launches
    spec_mask_(features, feature_lengths, seed=) the ``mask:`` augmentation, in place           1 launch
    mfcc(waveform)                               one utterance under torchaudio's signature
    FrontEnd('mask:fbank')                       the feature part of a reference dataset string as an nn.Module

``lengths`` stays on the device: every shape follows from the padded width L (``M = 1 + (L - 400) // 160`` frames), the per-utterance
frame counts are written by the feature launch itself, and nothing on the path reads a value back (it captures into a graph).  Rows
past an utterance's own frames are exact zeros, as ``pad_sequence`` leaves them.  csrc/frontend.hip holds the kernels, include/halo.h
("Batched feature front-end") the contract and the mask's draw; ``fbank.fbank`` -- one utterance, two launches -- stays as it is.

Parity: torchaudio is not part of this build, so MFCC PARITY IS UNPINNED (tests/frontend_ref.py restates kaldi's DCT and lifter on
oracle/fbank_ref.py); only the log-mel stage underneath is pinned, to the g11_fbank vectors.
"""
import math

import torch
from torch import nn

from . import _lib, ops
from ._lib import check, lib, ptr

PADDED = 512                 # the FFT length csrc/frontend.hip is built for
_EPS = float(torch.finfo(torch.float32).eps)
_TABLES = {}
_SPECS = ('fbank', 'mfcc', 'mask:fbank', 'mask:mfcc')


def _twiddles():
    """[770] float64, the layout include/halo.h states: packed radix-2 stages (entry h - 1 + j = e^{-i pi j / h}), then e^{-2 pi i k / 512}."""
    re, im = torch.zeros(256, dtype=torch.float64), torch.zeros(256, dtype=torch.float64)
    h = 1
    while h <= 128:
        ang = math.pi * torch.arange(h, dtype=torch.float64) / h
        re[h - 1:2 * h - 1], im[h - 1:2 * h - 1] = torch.cos(ang), -torch.sin(ang)
        h *= 2
    ang = 2 * math.pi * torch.arange(PADDED // 4 + 1, dtype=torch.float64) / PADDED
    return torch.cat([re, im, torch.cos(ang), -torch.sin(ang)])


def mel_filters(num_mel_bins, padded, sample_frequency, low_freq, high_freq):
    """kaldi's triangles as ([3, num_mel_bins] int32: first bin, bin count, offset; packed float64 weights): each touches a contiguous
    range of the padded // 2 spectrum bins (the Nyquist bin has weight zero in kaldi's [num_bins, padded // 2] matrix)."""
    nyquist = 0.5 * sample_frequency
    hi = high_freq + nyquist if high_freq <= 0.0 else high_freq
    mel = lambda f: 1127.0 * torch.log(1.0 + f / 700.0)
    mlo, mhi = mel(torch.tensor(low_freq, dtype=torch.float64)), mel(torch.tensor(hi, dtype=torch.float64))
    delta = (mhi - mlo) / (num_mel_bins + 1)
    b = torch.arange(num_mel_bins, dtype=torch.float64)[:, None]
    left, center, right = mlo + b * delta, mlo + (b + 1) * delta, mlo + (b + 2) * delta
    m = mel(sample_frequency / padded * torch.arange(padded // 2, dtype=torch.float64))[None, :]
    w = torch.clamp(torch.minimum((m - left) / (center - left), (right - m) / (right - center)), min=0.0)
    ranges, weights = torch.zeros(3, num_mel_bins, dtype=torch.int32), []
    offset = 0
    for i in range(num_mel_bins):
        nz = torch.nonzero(w[i] > 0.0)[:, 0]
        lo, count = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if nz.numel() else (0, 0)
        ranges[:, i] = torch.tensor([lo, count, offset], dtype=torch.int32)
        weights.append(w[i, lo:lo + count])
        offset += count
    return ranges, torch.cat(weights + [torch.zeros(1, dtype=torch.float64)])        # never empty


def dct_lifter(num_ceps, num_mel_bins, cepstral_lifter):
    """[num_ceps, num_mel_bins] float64: kaldi's orthonormal DCT-II (first row sqrt(1 / num_mel_bins), the others
    sqrt(2 / num_mel_bins) cos(pi / num_mel_bins (n + 0.5) k)), row k times the lifter 1 + 0.5 Q sin(pi k / Q)."""
    n = torch.arange(num_mel_bins, dtype=torch.float64)[None, :]
    k = torch.arange(num_ceps, dtype=torch.float64)[:, None]
    dct = math.sqrt(2.0 / num_mel_bins) * torch.cos(math.pi / num_mel_bins * (n + 0.5) * k)
    dct[0] = math.sqrt(1.0 / num_mel_bins)
    if cepstral_lifter != 0.0:
        dct = dct * (1.0 + 0.5 * cepstral_lifter * torch.sin(math.pi * k / cepstral_lifter))
    return dct.contiguous()


def _tables(num_mel_bins, frame_len, sample_frequency, low_freq, high_freq, num_ceps, cepstral_lifter, device):
    """The launch's constant tables, built once per configuration on the host and kept on the device (as fbank._constants)."""
    key = (num_mel_bins, frame_len, float(sample_frequency), float(low_freq), float(high_freq), num_ceps, float(cepstral_lifter), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        n = torch.arange(frame_len, dtype=torch.float64)
        window = (0.5 - 0.5 * torch.cos(2 * math.pi * n / (frame_len - 1))) ** 0.85                      # povey: symmetric hann ** 0.85
        ranges, weights = mel_filters(num_mel_bins, PADDED, sample_frequency, low_freq, high_freq)
        dct = dct_lifter(num_ceps, num_mel_bins, cepstral_lifter).to(device) if num_ceps else None
        hit = (window.float().to(device), _twiddles().to(device), ranges.contiguous().to(device), weights.to(device), dct)
        _TABLES[key] = hit
    return hit


def _check_inputs(what, waveforms, lengths):
    if not isinstance(waveforms, torch.Tensor) or not waveforms.is_cuda or not isinstance(lengths, torch.Tensor) or not lengths.is_cuda:
        raise _lib.HaloError(f'haloop_amd.features.{what} runs on the HIP device only (no CPU path)')
    if waveforms.dim() != 2 or lengths.dim() != 1 or lengths.shape[0] != waveforms.shape[0]:
        raise ValueError(f'{what}: expected waveforms [N, L] and lengths [N], got {tuple(waveforms.shape)} and {tuple(lengths.shape)}')
    return waveforms.float().contiguous(), lengths.to(torch.int64).contiguous()


def _features(what, kind, waveforms, lengths, num_mel_bins, num_ceps, cepstral_lifter, blackman_coeff=0.42, channel=-1, dither=0.0,
              energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, min_duration=0.0,
              preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0,
              snip_edges=True, subtract_mean=False, use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0,
              vtln_warp=1.0, window_type='povey'):
    if (dither != 0.0 or htk_compat or not round_to_power_of_two or not snip_edges or subtract_mean or use_energy or not use_log_fbank
            or not use_power or vtln_warp != 1.0 or window_type != 'povey' or min_duration != 0.0):
        raise NotImplementedError(f'haloop_amd.features.{what} builds the default path of torchaudio.compliance.kaldi only')
    frame_len, shift = int(sample_frequency * frame_length * 0.001), int(sample_frequency * frame_shift * 0.001)
    if not 2 <= frame_len <= PADDED or not 1 <= shift <= PADDED or 1 << (frame_len - 1).bit_length() != PADDED:
        raise NotImplementedError(f'haloop_amd.features.{what} is built for frames that pad to {PADDED} samples')
    wav, lengths = _check_inputs(what, waveforms, lengths)
    N, L = wav.shape
    M = 1 + (L - frame_len) // shift if L >= frame_len else 0
    window, twiddle, ranges, weights, dct = _tables(num_mel_bins, frame_len, sample_frequency, low_freq, high_freq, num_ceps,
                                                    cepstral_lifter, wav.device)
    out = torch.empty(N, M, num_ceps if kind == _lib.HALO_FEATURES_MFCC else num_mel_bins, device=wav.device)
    feature_lengths = torch.empty(N, dtype=torch.int64, device=wav.device)
    check(lib().halo_features_batch(ptr(wav), ptr(lengths), N, L, kind, frame_len, shift, preemphasis_coefficient, int(remove_dc_offset),
                                    ptr(window), ptr(twiddle), ptr(ranges), ptr(weights), weights.numel(), num_mel_bins, ptr(dct), num_ceps,
                                    _EPS, ptr(out), M, ptr(feature_lengths), ops._stream()), 'halo_features_batch')
    return out, feature_lengths


def fbank_batch(waveforms, lengths, num_mel_bins=80, **kaldi_kwargs):
    """waveforms [N, L] (row n valid up to lengths[n]; anything may stand behind), lengths [N] on the device ->
    (log-mels [N, M, num_mel_bins] float32, feature_lengths [N] int64).  ``kaldi_kwargs``: the keywords of ``fbank.fbank``."""
    return _features('fbank_batch', _lib.HALO_FEATURES_FBANK, waveforms, lengths, num_mel_bins, 0, 0.0, **kaldi_kwargs)


def cmvn_(features, feature_lengths):
    """Utterance-level mean / variance normalisation (ha/data.py:148-150) in place on [N, M, D]; returns its argument."""
    N, M, D = ops._f32c(features, 'cmvn_').shape
    check(lib().halo_cmvn_batch(ptr(features), ptr(feature_lengths), N, M, D, ops._stream()), 'halo_cmvn_batch')
    return features


def mfcc_batch(waveforms, lengths, num_ceps=13, num_mel_bins=23, cepstral_lifter=22.0, cmvn=True, **kaldi_kwargs):
    """torchaudio.compliance.kaldi.mfcc's defaults for a batch -> (MFCCs [N, M, num_ceps] float32, feature_lengths [N] int64);
    ``cmvn=True`` normalises every utterance's columns over its own frames (one frame: a NaN row, as the reference's expression)."""
    if not 1 <= num_ceps <= num_mel_bins:
        raise ValueError(f'mfcc_batch: num_ceps {num_ceps} must lie in [1, num_mel_bins = {num_mel_bins}]')
    out, feature_lengths = _features('mfcc_batch', _lib.HALO_FEATURES_MFCC, waveforms, lengths, num_mel_bins, num_ceps, cepstral_lifter,
                                     **kaldi_kwargs)
    return (cmvn_(out, feature_lengths) if cmvn else out), feature_lengths


def mfcc(waveform, channel=-1, **kwargs):
    """waveform [c, n] (channel ``channel``, -1 = first) or [n] -> [n_frames, num_ceps]: torchaudio.compliance.kaldi.mfcc for one
    utterance, a batch of one on the batched launch (no CMVN, as that function)."""
    if not waveform.is_cuda:
        raise _lib.HaloError('haloop_amd.features.mfcc runs on the HIP device only (no CPU path)')
    wav = (waveform[max(channel, 0)] if waveform.dim() == 2 else waveform)[None]
    lengths = torch.full((1,), wav.shape[1], dtype=torch.int64, device=wav.device)
    return mfcc_batch(wav, lengths, cmvn=False, **kwargs)[0][0]


def spec_mask_(features, feature_lengths, *, seed, step=0, freq_param=None, time_param=7):
    """The ``mask:`` combinator (ha/data.py:103-123) in place on [N, M, D]: per utterance one band of at most ``freq_param`` (default
    D // 6) columns and one band of at most ``time_param`` of its own frames set to 0, drawn from the library's Philox stream keyed by
    ``(seed, step)`` (include/halo.h).  Returns its argument."""
    if not isinstance(features, torch.Tensor) or not features.is_cuda or not feature_lengths.is_cuda:
        raise _lib.HaloError('haloop_amd.features.spec_mask_ runs on the HIP device only (no CPU path)')
    N, M, D = ops._f32c(features, 'spec_mask_').shape
    if feature_lengths.dtype != torch.int64 or feature_lengths.shape != (N,) or not feature_lengths.is_contiguous():
        raise ValueError('spec_mask_: feature_lengths must be a contiguous int64 tensor [N]')
    freq_param = D // 6 if freq_param is None else freq_param
    check(lib().halo_spec_mask(ptr(features), ptr(feature_lengths), N, M, D, freq_param, time_param, seed & 0xFFFFFFFFFFFFFFFF,
                               step & 0xFFFFFFFF, ops._stream()), 'halo_spec_mask')
    return features


class FrontEnd(nn.Module):
    """The feature part of a reference dataset string -- 'fbank', 'mfcc', 'mask:fbank', 'mask:mfcc' -- on the device.
    ``front(waveforms [N, L], lengths [N], seed=, step=) -> (features [N, M, D], feature_lengths [N])``: at most three launches, and the
    result goes straight into ``rnn.Encoder.forward`` / the AudioEncoders.  The masks are applied in training mode only."""

    def __init__(self, spec):
        super().__init__()
        if spec not in _SPECS:
            raise ValueError(f'FrontEnd: unknown feature spec {spec!r}; supported: ' + ', '.join(repr(s) for s in _SPECS))
        self.spec = spec
        self.mask, self.kind = spec.startswith('mask:'), spec.split(':')[-1]

    def forward(self, waveforms, lengths, *, seed=0, step=0):
        features, feature_lengths = (fbank_batch if self.kind == 'fbank' else mfcc_batch)(waveforms, lengths)
        if self.mask and self.training:
            spec_mask_(features, feature_lengths, seed=seed, step=step)
        return features, feature_lengths

    def extra_repr(self):
        return repr(self.spec)
