"""CPU restatement (numpy) of the batched feature front-end, haloop_amd.features / csrc/frontend.hip -- TEST INFRASTRUCTURE ONLY.

Built on oracle/fbank_ref.py and oracle/philox.py as they are:
    fbank_batch   fbank_ref.fbank per utterance, zero-padded to the batch's frame count (what pad_sequence leaves)
    mfcc          torchaudio.compliance.kaldi.mfcc's defaults: fbank_ref.fbank(num_mel_bins=23) times kaldi's DCT-II (orthonormal over
                  num_mel_bins, first basis vector sqrt(1 / num_mel_bins), the first num_ceps coefficients) times the lifter
                  1 + 0.5 Q sin(pi i / Q), in float64; use_energy=False
    cmvn          ha/data.py:148-150: frames -= frames.mean(dim=0); frames /= frames.std(dim=0) (unbiased), in float64
    spec_mask     ha/data.py:103-123 (torchaudio.functional.mask_along_axis_iid on the columns, then on the frames, of the unpadded
                  utterance) with the draws include/halo.h defines under HALO_SPECMASK_STREAM, the float32 arithmetic step for step

PARITY UNPINNED for MFCC: torchaudio is not installed where this project is built and the reference ships no feature vectors, so the
DCT, the lifter and the CMVN restate the published algorithm (kaldi's ComputeDctMatrix / ComputeLifterCoeffs as torchaudio ports them)
without vectors to check them against.  Only the log-mel stage underneath is pinned: oracle/fbank_ref.py to g11_fbank, the vectors of
the Hugging Face transformers port of torchaudio.compliance.kaldi.fbank (tests/test_oracle_golden.py).  The mask's draws are the
library's own stream by design (torch's generator cannot be reproduced on the device); what is restated is mask_along_axis_iid's
arithmetic on them, with one stated departure: the mask parameter is clamped to the axis size.
"""
import numpy as np

from oracle import fbank_ref, philox

SPECMASK_STREAM = 0x53504D4B


def n_frames(n, frame_len=400, shift=160):
    return 1 + (n - frame_len) // shift if n >= frame_len else 0


def pad_batch(rows, M, D):
    out = np.zeros((len(rows), M, D), dtype=np.float32)
    for n, r in enumerate(rows):
        out[n, :r.shape[0]] = r
    return out


def fbank_batch(waveforms, lengths, num_mel_bins=80):
    """waveforms [N, L], lengths [N] -> (features [N, M, num_mel_bins] float32 zero-padded, feature_lengths [N] int64)."""
    rows = [fbank_ref.fbank(np.asarray(w)[:int(n)], num_mel_bins=num_mel_bins) for w, n in zip(waveforms, lengths)]
    return pad_batch(rows, n_frames(np.asarray(waveforms).shape[1]), num_mel_bins), np.array([r.shape[0] for r in rows], dtype=np.int64)


def dct_matrix(num_ceps=13, num_mel_bins=23):
    """[num_ceps, num_mel_bins] float64, kaldi's DCT-II rows."""
    n = np.arange(num_mel_bins, dtype=np.float64)[None, :]
    k = np.arange(num_ceps, dtype=np.float64)[:, None]
    dct = np.sqrt(2.0 / num_mel_bins) * np.cos(np.pi / num_mel_bins * (n + 0.5) * k)
    dct[0] = np.sqrt(1.0 / num_mel_bins)
    return dct


def lifter(num_ceps=13, cepstral_lifter=22.0):
    i = np.arange(num_ceps, dtype=np.float64)
    return 1.0 + 0.5 * cepstral_lifter * np.sin(np.pi * i / cepstral_lifter) if cepstral_lifter != 0.0 else np.ones(num_ceps)


def mfcc(wav, num_ceps=13, num_mel_bins=23, cepstral_lifter=22.0):
    """One utterance -> [m, num_ceps] float32."""
    mel = fbank_ref.fbank(wav, num_mel_bins=num_mel_bins).astype(np.float64)
    return ((mel @ dct_matrix(num_ceps, num_mel_bins).T) * lifter(num_ceps, cepstral_lifter)[None, :]).astype(np.float32)


def cmvn(frames):
    """[m, D] float32 -> float32; one frame gives NaN (0 / 0), none gives none."""
    x = np.asarray(frames, dtype=np.float64)
    if x.shape[0] == 0:
        return x.astype(np.float32)
    c = x - x.mean(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (c / np.sqrt((c * c).sum(axis=0) / np.float64(x.shape[0] - 1))).astype(np.float32)


def mfcc_batch(waveforms, lengths, apply_cmvn=True):
    rows = [mfcc(np.asarray(w)[:int(n)]) for w, n in zip(waveforms, lengths)]
    if apply_cmvn:
        rows = [cmvn(r) for r in rows]
    return pad_batch(rows, n_frames(np.asarray(waveforms).shape[1]), 13), np.array([r.shape[0] for r in rows], dtype=np.int64)


def _band(ra, rb, param, size):
    """(start, width) of one mask, float32 throughout: u = float32(r >> 8) * 2^-24, v = ua * min(param, size), width = int(v),
    start = int(ub * (size - v))."""
    ua = np.float32(int(ra) >> 8) * np.float32(2.0 ** -24)
    ub = np.float32(int(rb) >> 8) * np.float32(2.0 ** -24)
    v = np.float32(ua * np.float32(min(param, size)))
    return int(np.float32(ub * np.float32(np.float32(size) - v))), int(v)


def spec_mask_bands(n, D, m_n, seed, step, freq_param=None, time_param=7):
    """((column start, width), (frame start, width)) of utterance n."""
    one = lambda v: np.array([v], dtype=np.uint32)
    r = philox.philox4x32_10(one(n), one(0), one(SPECMASK_STREAM), one(step & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    r = [int(x[0]) for x in r]
    return _band(r[0], r[1], D // 6 if freq_param is None else freq_param, D), _band(r[2], r[3], time_param, m_n)


def spec_mask(features, feature_lengths, seed, step=0, freq_param=None, time_param=7):
    """features [N, M, D] -> boolean [N, M, D], True where the mask sets 0: the two bands, on the utterance's own m_n frames only."""
    N, M, D = features.shape
    zero = np.zeros((N, M, D), dtype=bool)
    for n in range(N):
        m = int(feature_lengths[n])
        (cs, cw), (ts, tw) = spec_mask_bands(n, D, m, seed, step, freq_param, time_param)
        zero[n, :m, cs:cs + cw] = True
        zero[n, :m][ts:ts + tw, :] = True
    return zero
