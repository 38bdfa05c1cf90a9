"""CPU restatement (numpy, float64) of the waveform stage, haloop_amd.features.resample_batch / speed_perturb / csrc/resample.hip --
TEST INFRASTRUCTURE ONLY.

The definition is include/halo.h's ("Waveform stage"): torchaudio.functional.resample with its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99) as a polyphase filter, the taps evaluated in float64 and rounded to float32, everything else in
float64.  PARITY WITH TORCHAUDIO IS UNPINNED: torchaudio is not installed where this project is built, so the formula restates the
published algorithm without vectors to check it against; tests/test_resample_ref.py pins what can be pinned without them (the polyphase
form against the direct sum over the continuous kernel, the lengths, the tap sums, a tone).

    ratio(orig_freq, new_freq)     the two rates divided by their gcd
    taps(orig, new)                ([new, K] float32, width)
    resample(x, orig, new)         one utterance -> float64 [ceil(new * len / orig)]; orig == new is a copy
    direct(x, orig, new)           the same by out[o] = sum_j x[j] f(j / orig - o / new): no phases, no padding
    resample_batch(w, lengths, ..) rows zero-padded to ceil(new * L / orig), and the lengths
    speed_ratio(factor, rate)      a factor f is the ratio (int(f * rate), rate): the source is taken as sampled at int(f * rate) Hz
    speed_index(n, seed, step, F)  the factor utterance n draws: include/halo.h's HALO_SPEED_STREAM, restated on oracle/philox.py
"""
import math

import numpy as np

from oracle import philox

SPEED_STREAM = 0x53504544
FACTORS = (0.95, 0.98, 1.0, 1.02, 1.05)
WIDTH, ROLLOFF = 6, 0.99


def ratio(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def kernel(t, orig, new):
    """The continuous filter f at offsets t (in seconds of the rate-1 grid: j / orig - o / new), float64."""
    base = min(orig, new) * ROLLOFF
    t = np.clip(np.asarray(t, dtype=np.float64) * base, -WIDTH, WIDTH)
    safe = np.where(t == 0.0, 1.0, t)
    sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    return sinc * np.cos(np.pi * t / (2.0 * WIDTH)) ** 2 * (base / orig)


def taps(orig, new):
    """([new, K] float32, width), K = 2 * width + orig."""
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(WIDTH * orig / base))
    k = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    p = np.arange(new, dtype=np.float64)[:, None] / new
    return kernel(k - p, orig, new).astype(np.float32), width


def out_length(length, orig, new):
    return (new * int(length) + orig - 1) // orig


def resample(x, orig, new):
    x = np.asarray(x, dtype=np.float64)
    if orig == new:
        return x.copy()
    h, width = taps(orig, new)
    K = h.shape[1]
    n_out = out_length(x.shape[0], orig, new)
    Q = (n_out + new - 1) // new
    xpad = np.zeros(max(Q - 1, 0) * orig + K + width + x.shape[0], dtype=np.float64)
    xpad[width:width + x.shape[0]] = x
    frames = np.lib.stride_tricks.as_strided(xpad, (Q, K), (orig * xpad.strides[0], xpad.strides[0]))
    return (frames @ h.astype(np.float64).T).reshape(-1)[:n_out]


def direct(x, orig, new):
    x = np.asarray(x, dtype=np.float64)
    j = np.arange(x.shape[0], dtype=np.float64) / orig
    return np.array([np.sum(x * kernel(j - o / new, orig, new)) for o in range(out_length(x.shape[0], orig, new))])


def resample_batch(waveforms, lengths, orig, new):
    """waveforms [N, L], lengths [N] -> (float64 [N, ceil(new * L / orig)] zero-padded, out_lengths [N] int64)."""
    waveforms = np.asarray(waveforms)
    out = np.zeros((waveforms.shape[0], out_length(waveforms.shape[1], orig, new)), dtype=np.float64)
    for n, ln in enumerate(lengths):
        y = resample(waveforms[n, :int(ln)], orig, new)
        out[n, :y.shape[0]] = y
    return out, np.array([out_length(ln, orig, new) for ln in lengths], dtype=np.int64)


def speed_ratio(factor, sample_rate=16000):
    return ratio(int(factor * sample_rate), sample_rate)


def speed_index(n, seed, step, num_factors=len(FACTORS)):
    """u0 = float32(r0 >> 8) * 2^-24; index = min(int(u0 * F), F - 1), the product rounded to float32."""
    one = lambda v: np.array([v], dtype=np.uint32)
    r = philox.philox4x32_10(one(n), one(0), one(SPEED_STREAM), one(step & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u0 = np.float32(int(r[0][0]) >> 8) * np.float32(2.0 ** -24)
    return min(int(np.float32(u0 * np.float32(num_factors))), num_factors - 1)


def tolerance(orig, new, max_abs_x):
    """The forward error bound of an fp32 dot product in any order, n u / (1 - n u) * max_p sum_k |taps[p, k]| * max |x|, with u = 2^-24
    and n one more than the largest count of non-zero taps in a phase."""
    if orig == new:
        return 0.0
    h = taps(orig, new)[0].astype(np.float64)
    n = int((h != 0.0).sum(axis=1).max()) + 1
    u = 2.0 ** -24
    return n * u / (1.0 - n * u) * float(np.abs(h).sum(axis=1).max()) * max_abs_x
