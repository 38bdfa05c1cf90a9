// The batched feature front-end (ha/data.py:103-151, the combinators fbank: / mfcc: / mask:): a ragged batch of waveforms in, padded
// features + lengths out, in a constant number of launches and without a host read (include/halo.h, "Batched feature front-end").
//   halo_features_batch   waveforms [N, L] -> log-mels or MFCCs [N, M, D] + feature_lengths [N], ONE launch
//   halo_cmvn_batch       utterance-level mean / variance normalisation in place, float64 sums in a fixed order
//   halo_spec_mask        one band of columns and one band of frames per utterance set to 0, draws from the Philox stream
//
// halo_features_batch: a workgroup owns FE_F consecutive frames of one utterance.  It loads the tables (window, FFT twiddles, packed
// mel filters, DCT) and the samples its frames span into LDS once, frames them in fp32 with the arithmetic of fbank_frames_kernel
// (csrc/fbank.hip: the same summation order for the mean, so the framed samples are the same bits), and transforms each frame with a
// 256-point complex FFT of z[j] = x[2j] + i x[2j+1] plus the split step, in float64 (csrc/fbank.hip says why not fp32).
//
// LDS layout of the transform (banks: 32 of 4 bytes for a 4-byte read and for writes, 64 for an 8-byte read):
//   * decimation in time, in place, on separate re[256] / im[256] arrays per frame.  The input is written in bit-reversed order while
//     framing; the gather that needs (sample 2 * bitrev(p)) reads a staging buffer padded by one float per 32 (pad32), which spreads
//     its stride of 16 floats over all 32 banks.
//   * consecutive lanes handle consecutive butterflies.  In a stage of half-size h the upper elements of a run of butterflies lie on
//     every other block of h positions (the indices with bit log2(h) clear), the lower ones on the blocks between.  So lanes 16-31
//     of every 32 READ their lower element first and the upper one second (32 lanes then cover 32 distinct doubles, all 64 banks),
//     and lanes 8-15 of every 16 WRITE theirs in that order (a write is serviced 16 lanes at a time on 16 doubles).  Which swap
//     goes with which access was settled by measurement, three variants timed alternately in one run: the compiler
//     pairs re[a] / im[a] into ds_read2st64_b64 / ds_write2st64_b64, and the variant with the fewest SQ_LDS_BANK_CONFLICT cycles
//     (both swaps per 8 lanes) is not the fastest.
//   * the twiddles of stage h are the h consecutive entries [h - 1, 2h - 1) of one packed table, so a half-wave reads consecutive (or
//     identical) addresses -- not a stride-(256 / h) walk through one table of 256, which puts 4 .. 16 lanes on one bank.
#include "halo_common.h"

namespace {

constexpr int FE_F = 8;                 // frames per workgroup
constexpr int FE_PADDED = 512;          // real FFT length (25 ms of 16 kHz audio rounded up to a power of two)
constexpr int FE_HALF = FE_PADDED / 2;  // complex FFT length; also the number of spectrum bins the filters see (Nyquist has weight 0)
constexpr int FE_MAX_BINS = 128;
constexpr int FE_MAX_WEIGHTS = 1024;
constexpr int FE_MAX_DCT = 1024;

__host__ __device__ __forceinline__ int pad32(int i) { return i + (i >> 5); }

struct FeArgs {
    const float *wav;
    const int64_t *lengths;
    long L;
    int M, bpu;                         // padded frame count; workgroups per utterance
    int kind, frame_len, shift, remove_dc;
    float preemph, eps;
    const float *window;
    const double *twiddle;              // [256 re | 256 im] packed FFT stages, then [129 re | 129 im] split-step twiddles
    const int *filt;                    // [num_bins] lo, [num_bins] count, [num_bins] offset into weights
    const double *weights;
    int n_weights, num_bins;
    const double *dct;                  // [num_ceps][num_bins], lifter folded in (MFCC only)
    int num_ceps;
    float *out;
    int64_t *feature_lengths;
};

__global__ __launch_bounds__(256) void features_batch_kernel(FeArgs a) {
    extern __shared__ double sh[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x / a.bpu, f0 = (blockIdx.x % a.bpu) * FE_F;
    const int D = a.kind ? a.num_ceps : a.num_bins;
    const long len = min(max((long)a.lengths[n], 0L), a.L);
    const int m_n = len >= a.frame_len ? 1 + (int)((len - a.frame_len) / a.shift) : 0;
    if (f0 == 0 && tid == 0) a.feature_lengths[n] = m_n;
    float *out = a.out + ((long)n * a.M + f0) * D;
    const int rows = min(FE_F, a.M - f0);                    // rows of the output this workgroup writes (<= 0: none)
    if (f0 >= m_n) {                                         // nothing but padding: exact zeros, no sample is read
        for (int i = tid; i < rows * D; i += 256) out[i] = 0.f;
        return;
    }

    const int span = (FE_F - 1) * a.shift + a.frame_len;
    double *z = sh;                                          // [FE_F][re 256 | im 256]
    double *twr = z + FE_F * FE_PADDED, *twi = twr + FE_HALF;
    double *spr = twi + FE_HALF, *spi = spr + FE_HALF / 2 + 1;
    double *fw = spi + FE_HALF / 2 + 1;
    double *lm = fw + a.n_weights;                           // [FE_F][num_bins] log-mels (MFCC only)
    double *dct = lm + (a.kind ? FE_F * a.num_bins : 0);
    float *stage = (float *)(dct + (a.kind ? a.num_ceps * a.num_bins : 0));
    float *win = stage + pad32(span) + 1;
    float *mean = win + pad32(a.frame_len) + 1;
    int *flo = (int *)(mean + FE_F), *fcnt = flo + a.num_bins, *foff = fcnt + a.num_bins;

    // ---- tables and samples, once per workgroup ------------------------------------------------------------------------------
    for (int i = tid; i < 2 * FE_HALF; i += 256) twr[i] = a.twiddle[i];
    for (int i = tid; i < 2 * (FE_HALF / 2 + 1); i += 256) spr[i] = a.twiddle[2 * FE_HALF + i];
    for (int i = tid; i < a.n_weights; i += 256) fw[i] = a.weights[i];
    if (a.kind)
        for (int i = tid; i < a.num_ceps * a.num_bins; i += 256) dct[i] = a.dct[i];
    for (int i = tid; i < a.frame_len; i += 256) win[pad32(i)] = a.window[i];
    for (int i = tid; i < a.num_bins; i += 256) {            // clamped: a table can never index past the spectrum or the weights
        const int lo = min(max(a.filt[i], 0), FE_HALF), off = min(max(a.filt[2 * a.num_bins + i], 0), a.n_weights);
        flo[i] = lo;
        foff[i] = off;
        fcnt[i] = min(max(a.filt[a.num_bins + i], 0), min(FE_HALF - lo, a.n_weights - off));
    }
    {
        const float *w = a.wav + (long)n * a.L;
        const long g0 = (long)f0 * a.shift;
        for (int i = tid; i < span; i += 256) stage[pad32(i)] = g0 + i < len ? w[g0 + i] : 0.f;   // a sample past lengths[n] is never read
    }
    __syncthreads();

    // ---- the frames' means: the summation order of fbank_frames_kernel (256 strided partial sums, four wave sums, (0+1)+(2+3)) --
    for (int fr = wave; fr < FE_F; fr += 4) {
        float mu = 0.f;
        if (a.remove_dc) {
            float r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float s = 0.f;
                for (int i = q * 64 + lane; i < a.frame_len; i += 256) s += stage[pad32(fr * a.shift + i)];
                r[q] = wave_sum(s);
            }
            mu = ((r[0] + r[1]) + (r[2] + r[3])) / (float)a.frame_len;
        }
        if (lane == 0) mean[fr] = mu;
    }
    __syncthreads();

    // ---- framing in fp32, written as z[bitrev(j)] = x[2j] + i x[2j+1]: thread p holds position p and gathers j = bitrev8(p) -------
    for (int fr = 0; fr < FE_F; ++fr) {
        const int j = (int)(__brev((unsigned)tid) >> 24);
        const float mu = mean[fr];
        float v[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int i = 2 * j + c;
            v[c] = 0.f;
            if (i < a.frame_len) {
                const float cur = stage[pad32(fr * a.shift + i)] - mu, prev = stage[pad32(fr * a.shift + (i > 0 ? i - 1 : 0))] - mu;
                v[c] = (cur - a.preemph * prev) * win[pad32(i)];                  // the first sample is pre-emphasised against itself
            }
        }
        z[fr * FE_PADDED + tid] = (double)v[0];
        z[fr * FE_PADDED + FE_HALF + tid] = (double)v[1];
    }
    __syncthreads();

    // ---- 256-point complex FFT of every frame: 8 radix-2 stages x (FE_F * 128) butterflies, 4 per thread and stage -------------
    const int flip = (lane >> 4) & 1, wflip = (lane >> 3) & 1;   // which of its two elements a lane reads / writes first
    for (int s = 0; s < 8; ++s) {
        const int h = 1 << s;
#pragma unroll
        for (int it = 0; it < FE_F / 2; ++it) {
            const int flat = it * 256 + tid, fr = flat >> 7, b = flat & 127;
            const int k = b & (h - 1), top = ((b >> s) << (s + 1)) | k;
            double *re = z + fr * FE_PADDED, *im = re + FE_HALF;
            const int a0 = top + (flip ? h : 0), a1 = a0 ^ h;
            const double r0 = re[a0], i0 = im[a0], r1 = re[a1], i1 = im[a1];
            const double wr = twr[h - 1 + k], wi = twi[h - 1 + k];
            const double xr = flip ? r1 : r0, xi = flip ? i1 : i0, yr = flip ? r0 : r1, yi = flip ? i0 : i1;
            const double tr = wr * yr - wi * yi, ti = wr * yi + wi * yr;
            const int b0 = top + (wflip ? h : 0), b1 = b0 ^ h;
            re[b0] = wflip ? xr - tr : xr + tr;
            im[b0] = wflip ? xi - ti : xi + ti;
            re[b1] = wflip ? xr + tr : xr - tr;
            im[b1] = wflip ? xi + ti : xi - ti;
        }
        __syncthreads();
    }

    // ---- split step and |X|^2: X[k] = E + W^k O, X[256 - k] = conj(E - W^k O) with E, O the transforms of the even / odd samples.
    //      Item (frame, k), k = 0 .. 128, reads Z[k] and Z[256 - k] and overwrites re[k] and re[256 - k] with the two powers.
    for (int flat = tid; flat < FE_F * (FE_HALF / 2 + 1); flat += 256) {
        const int fr = flat / (FE_HALF / 2 + 1), k = flat % (FE_HALF / 2 + 1), kc = (FE_HALF - k) & (FE_HALF - 1);
        double *re = z + fr * FE_PADDED, *im = re + FE_HALF;
        const double ar = re[k], ai = im[k], cr = re[kc], ci = im[kc];
        const double er = 0.5 * (ar + cr), ei = 0.5 * (ai - ci), orr = 0.5 * (ai + ci), oi = -0.5 * (ar - cr);
        const double wr = spr[k], wi = spi[k];
        const double tr = wr * orr - wi * oi, ti = wr * oi + wi * orr;
        const double pr = er + tr, pi = ei + ti, qr = er - tr, qi = ei - ti;
        re[k] = pr * pr + pi * pi;
        if (kc != k) re[kc] = qr * qr + qi * qi;
    }
    __syncthreads();

    // ---- the triangular filters on their own bins only, and the floored log ---------------------------------------------------
    for (int flat = tid; flat < FE_F * a.num_bins; flat += 256) {
        const int fr = flat / a.num_bins, b = flat % a.num_bins;
        const double *pw = z + fr * FE_PADDED + flo[b], *w = fw + foff[b];
        double e = 0.0;
        for (int i = 0; i < fcnt[b]; ++i) e += pw[i] * w[i];
        const float v = (float)log(fmax(e, (double)a.eps));
        if (a.kind)
            lm[flat] = (double)v;
        else if (fr < rows)
            out[flat] = f0 + fr < m_n ? v : 0.f;
    }
    if (!a.kind) return;
    __syncthreads();

    // ---- MFCC: DCT-II and lifter (one table) on the frame's log-mels --------------------------------------------------------------
    for (int flat = tid; flat < rows * a.num_ceps; flat += 256) {
        const int fr = flat / a.num_ceps, c = flat % a.num_ceps;
        const double *x = lm + fr * a.num_bins, *w = dct + c * a.num_bins;
        double e = 0.0;
        for (int i = 0; i < a.num_bins; ++i) e += x[i] * w[i];
        out[flat] = f0 + fr < m_n ? (float)e : 0.f;
    }
}

size_t features_lds_bytes(int kind, int frame_len, int shift, int n_weights, int num_bins, int num_ceps) {
    const int span = (FE_F - 1) * shift + frame_len;
    size_t doubles = (size_t)FE_F * FE_PADDED + 2 * FE_HALF + 2 * (FE_HALF / 2 + 1) + n_weights;
    if (kind) doubles += (size_t)FE_F * num_bins + (size_t)num_ceps * num_bins;
    const size_t words = (size_t)(pad32(span) + 1) + (pad32(frame_len) + 1) + FE_F + 3 * (size_t)num_bins;
    return doubles * sizeof(double) + words * 4;
}

// ---- CMVN -------------------------------------------------------------------------------------------------------------------------
// Workgroup (utterance, 16 columns): thread (g, d) sums the rows g, g + 16, ... of its column in float64, thread (0, d) adds the 16
// partial sums in order.  One pass for the mean, one for the centred squares, one to write: no atomics, one summation order.
__global__ __launch_bounds__(256) void cmvn_batch_kernel(float *__restrict__ x, const int64_t *__restrict__ feature_lengths, int M, int D) {
    __shared__ double part[16][17];
    __shared__ double stat[2][16];
    const int n = blockIdx.x, d = threadIdx.x & 15, g = threadIdx.x >> 4, col = blockIdx.y * 16 + d;
    const int m = (int)min(max((long)feature_lengths[n], 0L), (long)M);
    if (m == 0) return;
    float *xn = x + (long)n * M * D;
    const bool live = col < D;
    double s = 0.0;
    if (live)
        for (int r = g; r < m; r += 16) s += (double)xn[(long)r * D + col];
    part[g][d] = s;
    __syncthreads();
    if (g == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += part[i][d];
        stat[0][d] = t / (double)m;
    }
    __syncthreads();
    const double mu = stat[0][d];
    s = 0.0;
    if (live)
        for (int r = g; r < m; r += 16) {
            const double c = (double)xn[(long)r * D + col] - mu;
            s += c * c;
        }
    part[g][d] = s;
    __syncthreads();
    if (g == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += part[i][d];
        stat[1][d] = sqrt(t / (double)(m - 1));              // unbiased; one frame: 0 / 0, a NaN row as frames.std(dim=0) gives
    }
    __syncthreads();
    const double sd = stat[1][d];
    if (live)
        for (int r = g; r < m; r += 16) xn[(long)r * D + col] = (float)(((double)xn[(long)r * D + col] - mu) / sd);
}

// ---- mask: ------------------------------------------------------------------------------------------------------------------------
// (start, width) of one band, float32 step for step as include/halo.h states it (no contraction: each product and difference rounds)
__device__ __forceinline__ void mask_band(uint32_t ra, uint32_t rb, int param, int size, int &start, int &width) {
    const float ua = (float)(ra >> 8) * 5.9604644775390625e-8f, ub = (float)(rb >> 8) * 5.9604644775390625e-8f;
    const float v = __fmul_rn(ua, (float)min(param, size));
    width = (int)v;
    start = (int)__fmul_rn(ub, __fsub_rn((float)size, v));
}

__global__ __launch_bounds__(256) void spec_mask_kernel(float *__restrict__ x, const int64_t *__restrict__ feature_lengths, int M, int D,
                                                        int freq_param, int time_param, uint32_t k0, uint32_t k1, uint32_t step) {
    const int n = blockIdx.x;
    const int m = (int)min(max((long)feature_lengths[n], 0L), (long)M);
    if (m == 0) return;
    const Philox4 r = philox4x32_10((uint32_t)n, 0u, HALO_SPECMASK_STREAM, step, k0, k1);
    int cs, cw, ts, tw;
    mask_band(r.v[0], r.v[1], freq_param, D, cs, cw);
    mask_band(r.v[2], r.v[3], time_param, m, ts, tw);
    float *xn = x + (long)n * M * D;
    const int c1 = min(cs + cw, D), t1 = min(ts + tw, m);   // the writes stay inside the utterance's own frames
    cw = max(c1 - cs, 0);
    tw = max(t1 - ts, 0);
    for (int i = threadIdx.x; i < m * cw; i += 256) xn[(long)(i / cw) * D + cs + i % cw] = 0.f;
    for (int i = threadIdx.x; i < tw * D; i += 256) xn[(long)ts * D + i] = 0.f;
}

}  // namespace

extern "C" {

int halo_features_batch(const float *waveforms, const int64_t *lengths, int N, long L, int kind, int frame_len, int shift,
                        float preemphasis, int remove_dc, const float *window, const double *twiddle, const int *filters,
                        const double *weights, int n_weights, int num_bins, const double *dct, int num_ceps, float eps, float *out, int M,
                        int64_t *feature_lengths, halo_stream_t stream) {
    HALO_CHECK_ARG(lengths && window && twiddle && filters && weights && feature_lengths && N >= 0 && L >= 0);
    HALO_CHECK_ARG(kind == HALO_FEATURES_FBANK || kind == HALO_FEATURES_MFCC);
    HALO_CHECK_ARG(frame_len >= 2 && frame_len <= FE_PADDED && shift >= 1 && shift <= FE_PADDED);
    HALO_CHECK_ARG(num_bins >= 1 && num_bins <= FE_MAX_BINS && n_weights >= 1 && n_weights <= FE_MAX_WEIGHTS);
    if (kind == HALO_FEATURES_MFCC) HALO_CHECK_ARG(dct && num_ceps >= 1 && num_ceps <= num_bins && num_ceps * num_bins <= FE_MAX_DCT);
    HALO_CHECK_ARG((long)M == (L >= frame_len ? 1 + (L - frame_len) / shift : 0));
    HALO_CHECK_ARG((waveforms || L == 0) && (out || M == 0));
    if (N == 0) return HALO_OK;
    const int bpu = M > 0 ? (M + FE_F - 1) / FE_F : 1;       // an utterance always has one workgroup: it writes feature_lengths
    HALO_CHECK_ARG((long)N * bpu <= 0x7fffffffL);
    const size_t lds = features_lds_bytes(kind, frame_len, shift, n_weights, num_bins, num_ceps);
    HALO_CHECK_ARG(lds <= 64 * 1024);
    FeArgs a;
    a.wav = waveforms; a.lengths = lengths; a.L = L; a.M = M; a.bpu = bpu;
    a.kind = kind; a.frame_len = frame_len; a.shift = shift; a.remove_dc = remove_dc; a.preemph = preemphasis; a.eps = eps;
    a.window = window; a.twiddle = twiddle; a.filt = filters; a.weights = weights; a.n_weights = n_weights; a.num_bins = num_bins;
    a.dct = dct; a.num_ceps = kind == HALO_FEATURES_MFCC ? num_ceps : 0; a.out = out; a.feature_lengths = feature_lengths;
    hipLaunchKernelGGL(features_batch_kernel, dim3((unsigned)(N * bpu)), dim3(256), lds, (hipStream_t)stream, a);
    return halo_launch_status();
}

int halo_cmvn_batch(float *features, const int64_t *feature_lengths, int N, int M, int D, halo_stream_t stream) {
    HALO_CHECK_ARG(feature_lengths && N >= 0 && M >= 0 && D >= 1 && (features || N == 0 || M == 0));
    HALO_CHECK_ARG(N <= 0x7fffffff && (D + 15) / 16 <= 65535);
    if (N == 0 || M == 0) return HALO_OK;
    hipLaunchKernelGGL(cmvn_batch_kernel, dim3((unsigned)N, (unsigned)((D + 15) / 16)), dim3(256), 0, (hipStream_t)stream, features,
                       feature_lengths, M, D);
    return halo_launch_status();
}

int halo_spec_mask(float *features, const int64_t *feature_lengths, int N, int M, int D, int freq_param, int time_param, uint64_t seed,
                   uint32_t step, halo_stream_t stream) {
    HALO_CHECK_ARG(feature_lengths && N >= 0 && M >= 0 && D >= 1 && (features || N == 0 || M == 0));
    HALO_CHECK_ARG(freq_param >= 0 && time_param >= 0 && (long)M * D <= 0x7fffffffL);
    if (N == 0 || M == 0) return HALO_OK;
    hipLaunchKernelGGL(spec_mask_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, features, feature_lengths, M, D, freq_param,
                       time_param, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), step);
    return halo_launch_status();
}

}  // extern "C"
