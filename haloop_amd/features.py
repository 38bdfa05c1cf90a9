"""The reference's feature pipeline for a whole batch on the HIP device (ha/data.py:103-151, the combinators ``fbank:``, ``mfcc:`` and
``mask:``): a ragged batch of waveforms in, padded features + lengths out, ready for ``Encoder.forward(inputs, input_lengths)``.

    fbank_batch(waveforms [N, L], lengths [N])   80-mel kaldi log filterbank                    1 launch
    mfcc_batch(waveforms, lengths)               kaldi MFCC (13 of 23) + utterance CMVN         2 launches
    spec_mask_(features, feature_lengths, seed=) the ``mask:`` augmentation, in place           1 launch
    mfcc(waveform)                               one utterance under torchaudio's signature
    resample_batch(waveforms, lengths, orig_freq)  sinc resampling to 16 kHz (LabelFile's)      1 launch
    speed_perturb(waveforms, lengths, seed=)     the ``speed:`` augmentation, drawn per utterance 1 launch
    FrontEnd('mask:fbank:speed')                 a reference dataset string from the waveform up, as an nn.Module

``lengths`` stays on the device: every shape follows from the padded width L (``M = 1 + (L - 400) // 160`` frames), the per-utterance
frame counts are written by the feature launch itself, and nothing on the path reads a value back (it captures into a graph).  Rows
past an utterance's own frames are exact zeros, as ``pad_sequence`` leaves them.  csrc/frontend.hip holds the kernels, include/halo.h
("Batched feature front-end") the contract and the mask's draw; ``fbank.fbank`` -- one utterance, two launches -- stays as it is.

Parity: torchaudio is not part of this build, so MFCC PARITY IS UNPINNED (tests/frontend_ref.py restates kaldi's DCT and lifter on
oracle/fbank_ref.py); only the log-mel stage underneath is pinned, to the g11_fbank vectors.  RESAMPLING PARITY IS UNPINNED for the same
reason: include/halo.h ("Waveform stage") states the arithmetic, torchaudio.functional.resample's defaults, and tests/resample_ref.py
restates it in float64.  csrc/resample.hip holds that kernel.
"""
import ctypes
import math

import torch
from torch import nn

from . import _lib, ops
from ._lib import check, lib, ptr

PADDED = 512                 # the FFT length csrc/frontend.hip is built for
_EPS = float(torch.finfo(torch.float32).eps)
_TABLES = {}
_SPECS = ('fbank', 'mfcc', 'mask:fbank', 'mask:mfcc', 'fbank:speed', 'mfcc:speed', 'mask:fbank:speed', 'mask:mfcc:speed')


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


def resample_taps(orig, new):
    """One reduced ratio's packed filter, the layout include/halo.h states: (width, stride, phases [2, new] int32 -- first non-zero tap
    and count of each phase --, taps [new, stride] float32).  torchaudio.functional.resample's defaults (sinc_interp_hann,
    lowpass_filter_width 6, rolloff 0.99) evaluated in float64 and rounded once; the clamp zeroes every tap outside |t| < 6, and only the
    run between a phase's first and last non-zero tap is kept.  orig == new is a copy: one tap of 1."""
    if orig == new:
        return 0, 1, torch.tensor([[0], [1]], dtype=torch.int32), torch.ones(1, 1)
    base = min(orig, new) * 0.99
    width = int(math.ceil(6 * orig / base))
    k = torch.arange(-width, width + orig, dtype=torch.float64)[None, :] / orig
    p = torch.arange(new, dtype=torch.float64)[:, None] / new
    t = ((k - p) * base).clamp(-6.0, 6.0)
    pt = math.pi * torch.where(t == 0, torch.ones_like(t), t)
    dense = (torch.where(t == 0, torch.ones_like(t), torch.sin(pt) / pt) * torch.cos(math.pi * t / 12.0) ** 2 * (base / orig)).float()
    nz = dense != 0
    first = nz.int().argmax(dim=1)
    count = dense.shape[1] - nz.flip(1).int().argmax(dim=1) - first
    stride = int(count.max()) | 1                            # odd: consecutive phases on different LDS banks
    cols = first[:, None] + torch.arange(stride)[None, :]
    taps = torch.where(torch.arange(stride)[None, :] < count[:, None], dense.gather(1, cols.clamp(max=dense.shape[1] - 1)), torch.zeros(()))
    return width, stride, torch.stack([first, count]).to(torch.int32), taps.contiguous()


def _resample_tables(ratios, device):
    """The launch's tables for a tuple of reduced ratios, built once per configuration on the host and kept on the device (as _tables):
    (host int32 [R][6] descriptors, phases, taps).  ValueError where a ratio's table and input span do not fit the kernel's LDS."""
    key = ('resample', tuple(ratios), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        desc, phases, taps = [], [], []
        n_phases = n_taps = 0
        for orig, new in ratios:
            width, stride, ph, tp = resample_taps(orig, new)
            desc += [orig, new, width, stride, n_phases, n_taps]
            phases.append(ph.reshape(-1)); taps.append(tp.reshape(-1))
            n_phases += ph.numel(); n_taps += tp.numel()
            one = (ctypes.c_int * 6)(orig, new, width, stride, 0, 0)
            if not 0 <= lib().halo_resample_lds_bytes(one, 1) <= 64 * 1024:
                raise ValueError(f'resample: the ratio {orig}/{new} needs more LDS than the kernel has (its {new} x {stride} taps and the '
                                 'input span of a tile must fit 64 KiB)')
        hit = ((ctypes.c_int * len(desc))(*desc), torch.cat(phases).to(device), torch.cat(taps).to(device))
        _TABLES[key] = hit
    return hit


def _resample(what, waveforms, lengths, ratios, index=None, draw=False, seed=0, step=0, want_indices=False):
    wav, lengths = _check_inputs(what, waveforms, lengths)
    N, L = wav.shape
    desc, phases, taps = _resample_tables(ratios, wav.device)
    L_out = max((new * L + orig - 1) // orig for orig, new in ratios)
    out = torch.empty(N, L_out, device=wav.device)
    out_lengths = torch.empty(N, dtype=torch.int64, device=wav.device)
    indices = torch.empty(N, dtype=torch.int32, device=wav.device) if want_indices else None
    check(lib().halo_resample_batch(ptr(wav), ptr(lengths), N, L, desc, len(ratios), ptr(phases), phases.numel(), ptr(taps), taps.numel(),
                                    ptr(index), int(draw), seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, ptr(out), L_out,
                                    ptr(out_lengths), ptr(indices), ops._stream()), 'halo_resample_batch')
    return out, out_lengths, indices


def _reduced(orig_freq, new_freq):
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq < 1 or new_freq < 1:
        raise ValueError(f'resample: the rates must be positive integers, got {orig_freq} and {new_freq}')
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def _resample_defaults(what, lowpass_filter_width, rolloff, resampling_method):
    if lowpass_filter_width != 6 or rolloff != 0.99 or resampling_method != 'sinc_interp_hann':
        raise NotImplementedError(f'haloop_amd.features.{what} builds the default filter of torchaudio.functional.resample only')


def resample_batch(waveforms, lengths, orig_freq, new_freq=16000, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann'):
    """torchaudio.functional.resample's defaults for a ragged batch, one launch (what LabelFile does to 22050 / 32000 / 44100 / 48000 Hz
    audio, ha/data.py:33-39): waveforms [N, L] (row n valid up to lengths[n]; anything may stand behind), lengths [N] on the device ->
    (out [N, ceil(L * new / orig)] float32, out_lengths [N] int64 = ceil(lengths * new / orig)).  Samples past out_lengths[n] are exact
    zeros; equal rates give a copy.  Parity with torchaudio is unpinned (include/halo.h states the arithmetic)."""
    _resample_defaults('resample_batch', lowpass_filter_width, rolloff, resampling_method)
    return _resample('resample_batch', waveforms, lengths, (_reduced(orig_freq, new_freq),))[:2]


def speed_perturb(waveforms, lengths, *, seed, step=0, factors=(0.95, 0.98, 1.0, 1.02, 1.05), sample_rate=16000, indices=None):
    """The ``speed:`` combinator (ha/data.py:126-133, torchaudio.transforms.SpeedPerturbation(sample_rate, factors)) for a ragged batch, one
    launch: every utterance draws one factor f on the device -- the library's Philox stream HALO_SPEED_STREAM keyed by ``(seed, step)``,
    include/halo.h; ``indices`` (device int32 [N]) overrides the draw -- and is resampled from int(f * sample_rate) Hz to sample_rate.
    -> (out [N, L_out] float32, out_lengths [N] int64, indices [N] int32: the factor each row took).  L_out follows from L and the
    slowest factor alone ((20 L + 18) // 19 for the defaults), so nothing is read back and the call captures into a graph."""
    factors = tuple(factors)
    if not 1 <= len(factors) <= _lib.HALO_RESAMPLE_MAX_RATIOS:
        raise ValueError(f'speed_perturb: 1 to {_lib.HALO_RESAMPLE_MAX_RATIOS} factors, got {len(factors)}')
    if any(int(f * sample_rate) < 1 for f in factors):
        raise ValueError(f'speed_perturb: every factor must be positive, got {factors}')
    ratios = tuple(_reduced(int(f * sample_rate), sample_rate) for f in factors)
    if indices is not None and (not indices.is_cuda or indices.dtype != torch.int32 or indices.shape != lengths.shape or not indices.is_contiguous()):
        raise ValueError('speed_perturb: indices must be a contiguous int32 tensor [N] on the device')
    if len(ratios) == 1:                                     # one factor: nothing to draw (the kernel reports index 0)
        indices = None
    return _resample('speed_perturb', waveforms, lengths, ratios, index=indices, draw=indices is None, seed=seed, step=step, want_indices=True)


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
    """A reference dataset string from the waveform up -- 'fbank', 'mfcc', 'mask:fbank', 'mask:mfcc', and each of them over 'speed'
    ('mask:fbank:speed': combinators apply right to left, speed over the waveforms) -- on the device.
    ``front(waveforms [N, L], lengths [N], seed=, step=) -> (features [N, M, D], feature_lengths [N])``: at most four launches, and the
    result goes straight into ``rnn.Encoder.forward`` / the AudioEncoders.  Speed perturbation and the masks are applied in training
    mode only; ``(seed, step)`` keys both draws, on distinct streams."""

    def __init__(self, spec):
        super().__init__()
        if spec not in _SPECS:
            raise ValueError(f'FrontEnd: unknown feature spec {spec!r}; supported: ' + ', '.join(repr(s) for s in _SPECS))
        self.spec = spec
        parts = spec.split(':')
        self.mask, self.speed = parts[0] == 'mask', parts[-1] == 'speed'
        self.kind = parts[1 if self.mask else 0]

    def forward(self, waveforms, lengths, *, seed=0, step=0):
        if self.speed and self.training:
            waveforms, lengths, _ = speed_perturb(waveforms, lengths, seed=seed, step=step)
        features, feature_lengths = (fbank_batch if self.kind == 'fbank' else mfcc_batch)(waveforms, lengths)
        if self.mask and self.training:
            spec_mask_(features, feature_lengths, seed=seed, step=step)
        return features, feature_lengths

    def extra_repr(self):
        return repr(self.spec)
