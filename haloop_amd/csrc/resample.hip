// The waveform stage of a reference dataset string (ha/data.py:33-39, 59-62: LabelFile resamples to 16 kHz; :126-133, 186-187: the
// speed: combinator, torchaudio's SpeedPerturbation): band-limited sinc resampling of a ragged batch in ONE launch
// (include/halo.h, "Waveform stage").
//   halo_resample_batch   waveforms [N, L] -> out [N, L_out] + out_lengths [N]; the ratio of a row is the single table's, or one of up
//                         to 8 tables chosen by a device int32 [N] tensor or by the row's own Philox draw, made in the kernel
//
// A workgroup owns RS_TILE consecutive output samples of one utterance.  With o = q * new + p, output o is the dot product of phase
// p's taps with the input samples q * orig + k - width: the workgroup stages its ratio's packed taps (per phase: first non-zero tap,
// count, the taps at a fixed odd stride, so that consecutive phases fall on different LDS banks) and the input span its tile needs into
// LDS, coalesced, and every thread walks 4 outputs 256 apart.  A row's position in the span is 32-bit arithmetic relative to the tile's
// first input sample; only that first sample (q0 * orig - width) and the lengths are 64-bit.  The sum runs over the taps in ascending
// order with one fmaf each, started from the first product, so the identity table (one tap of 1) copies the bits of its input.
#include <algorithm>

#include "halo_common.h"

namespace {

constexpr int RS_TILE = 1024;           // output samples per workgroup
constexpr int RS_THREADS = 256;
constexpr size_t RS_MAX_LDS = 64 * 1024;

struct RsRatio {
    int orig, fresh, width, stride;     // fresh: the ratio's `new`; K = 2 * width + orig taps a phase, `stride` floats kept of them
    int phase_off, tap_off;             // into phases (ints) and taps (floats)
};

struct RsArgs {
    const float *wav;
    const int64_t *lengths;
    long L, L_out;
    int bpu, R;                         // workgroups per utterance; number of ratios
    const int *index;                   // [N] ratio of each row, or null
    int draw;                           // index == null and R > 1: the row's own draw
    uint32_t k0, k1, step;
    const int *phases;
    const float *taps;
    float *out;
    int64_t *out_lengths;
    int *indices;                       // [N] the ratio each row took, or null
    RsRatio ratio[HALO_RESAMPLE_MAX_RATIOS];
};

__host__ __device__ __forceinline__ int rs_span(const RsRatio &r) {           // input samples a tile can touch, whatever its first phase
    return ((r.fresh - 1 + RS_TILE - 1) / r.fresh) * r.orig + 2 * r.width + r.orig;
}

size_t rs_lds_bytes(const RsRatio &r) { return ((size_t)r.fresh * r.stride + 2 * (size_t)r.fresh + (size_t)rs_span(r)) * 4; }

__global__ __launch_bounds__(RS_THREADS) void resample_batch_kernel(RsArgs a) {
    extern __shared__ float rs_sh[];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / a.bpu, tile = blockIdx.x % a.bpu;

    int which = 0;
    if (a.R > 1) {
        if (a.index)
            which = a.index[n];
        else if (a.draw) {
            const Philox4 r = philox4x32_10((uint32_t)n, 0u, HALO_SPEED_STREAM, a.step, a.k0, a.k1);
            which = (int)__fmul_rn((float)(r.v[0] >> 8) * 5.9604644775390625e-8f, (float)a.R);
        }
        which = min(max(which, 0), a.R - 1);
    }
    RsRatio rr = a.ratio[0];
#pragma unroll
    for (int i = 1; i < HALO_RESAMPLE_MAX_RATIOS; ++i)
        if (i == which) rr = a.ratio[i];

    const long len = min(max((long)a.lengths[n], 0L), a.L);
    const long out_len = min(((long)rr.fresh * len + rr.orig - 1) / rr.orig, a.L_out);
    if (tile == 0 && tid == 0) {
        a.out_lengths[n] = out_len;
        if (a.indices) a.indices[n] = which;
    }
    const long o0 = (long)tile * RS_TILE;
    const int cols = (int)min((long)RS_TILE, a.L_out - o0);   // elements of out this workgroup writes (<= 0: none)
    float *out = a.out + n * a.L_out + o0;
    if (o0 >= out_len) {                                     // nothing but padding: exact zeros, no sample and no table is read
        for (int i = tid; i < cols; i += RS_THREADS) out[i] = 0.f;
        return;
    }

    const int K = 2 * rr.width + rr.orig;
    float *taps = rs_sh;                                     // [fresh][stride]
    int *first = (int *)(taps + rr.fresh * rr.stride), *count = first + rr.fresh;
    float *stage = (float *)(count + rr.fresh);              // [span]
    const long q0 = o0 / rr.fresh;
    const int p0 = (int)(o0 % rr.fresh);
    const int span = ((p0 + RS_TILE - 1) / rr.fresh) * rr.orig + K;      // <= rs_span(rr), which sized the LDS

    for (int i = tid; i < rr.fresh * rr.stride; i += RS_THREADS) taps[i] = a.taps[rr.tap_off + i];
    for (int i = tid; i < rr.fresh; i += RS_THREADS) {       // clamped: a table can never index past a phase's K taps or its packed row
        const int lo = min(max(a.phases[rr.phase_off + i], 0), K);
        first[i] = lo;
        count[i] = min(max(a.phases[rr.phase_off + rr.fresh + i], 0), min(K - lo, rr.stride));
    }
    {
        const float *w = a.wav + n * a.L;
        const long g0 = q0 * rr.orig - rr.width;             // the input sample stage[0] stands for (negative: left padding)
        for (int i = tid; i < span; i += RS_THREADS) {
            const long g = g0 + i;
            stage[i] = g >= 0 && g < len ? w[g] : 0.f;       // a sample past lengths[n] is never read
        }
    }
    __syncthreads();

    for (int i = tid; i < cols; i += RS_THREADS) {
        float v = 0.f;
        if (o0 + i < out_len) {
            const int t = p0 + i, ql = t / rr.fresh, p = t - ql * rr.fresh;
            const float *x = stage + ql * rr.orig + first[p], *h = taps + p * rr.stride;
            const int c = count[p];
            if (c > 0) v = h[0] * x[0];
            for (int k = 1; k < c; ++k) v = fmaf(h[k], x[k], v);
        }
        out[i] = v;
    }
}

// The descriptors come from the host, so everything the launch and the kernel's indexing rest on is checked here.
int rs_read_ratios(const int *ratios, int R, long n_phases, long n_taps, RsRatio *out, size_t *lds) {
    HALO_CHECK_ARG(ratios && R >= 1 && R <= HALO_RESAMPLE_MAX_RATIOS);
    *lds = 0;
    for (int i = 0; i < HALO_RESAMPLE_MAX_RATIOS; ++i) {
        const int *d = ratios + 6 * (i < R ? i : 0);
        RsRatio r;
        r.orig = d[0]; r.fresh = d[1]; r.width = d[2]; r.stride = d[3]; r.phase_off = d[4]; r.tap_off = d[5];
        HALO_CHECK_ARG(r.orig >= 1 && r.fresh >= 1 && r.width >= 0 && r.stride >= 1 && r.phase_off >= 0 && r.tap_off >= 0);
        HALO_CHECK_ARG(r.orig <= (1 << 16) && r.fresh <= (1 << 16) && r.width <= (1 << 16) && r.stride <= (1 << 16));
        HALO_CHECK_ARG(r.phase_off + 2L * r.fresh <= n_phases && r.tap_off + (long)r.fresh * r.stride <= n_taps);
        const size_t b = rs_lds_bytes(r);
        if (b > *lds) *lds = b;
        out[i] = r;
    }
    return HALO_OK;
}

}  // namespace

extern "C" {

long halo_resample_lds_bytes(const int *ratios, int R) {
    RsRatio r[HALO_RESAMPLE_MAX_RATIOS];
    size_t lds;
    if (rs_read_ratios(ratios, R, 1L << 40, 1L << 40, r, &lds) != HALO_OK) return -1;
    return (long)lds;
}

int halo_resample_batch(const float *waveforms, const int64_t *lengths, int N, long L, const int *ratios, int R, const int *phases,
                        long n_phases, const float *taps, long n_taps, const int *index, int draw, uint64_t seed, uint32_t step,
                        float *out, long L_out, int64_t *out_lengths, int *indices, halo_stream_t stream) {
    HALO_CHECK_ARG(lengths && phases && taps && out_lengths && N >= 0 && L >= 0 && L <= (1L << 40));
    RsArgs a;
    size_t lds;
    if (rs_read_ratios(ratios, R, n_phases, n_taps, a.ratio, &lds) != HALO_OK) return HALO_EINVAL;
    HALO_CHECK_ARG(R == 1 || index || draw);
    if (lds > RS_MAX_LDS) return HALO_ENOTSUP;
    long want = 0;
    for (int i = 0; i < R; ++i) want = std::max(want, ((long)a.ratio[i].fresh * L + a.ratio[i].orig - 1) / a.ratio[i].orig);
    HALO_CHECK_ARG(L_out == want);
    HALO_CHECK_ARG((waveforms || L == 0) && (out || L_out == 0));
    if (N == 0) return HALO_OK;
    const long bpu = L_out > 0 ? (L_out + RS_TILE - 1) / RS_TILE : 1;   // an utterance always has one workgroup: it writes out_lengths
    HALO_CHECK_ARG((long)N * bpu <= 0x7fffffffL);
    a.wav = waveforms; a.lengths = lengths; a.L = L; a.L_out = L_out; a.bpu = (int)bpu; a.R = R;
    a.index = index; a.draw = draw != 0; a.k0 = (uint32_t)(seed & 0xffffffffu); a.k1 = (uint32_t)(seed >> 32); a.step = step;
    a.phases = phases; a.taps = taps; a.out = out; a.out_lengths = out_lengths; a.indices = indices;
    hipLaunchKernelGGL(resample_batch_kernel, dim3((unsigned)(N * bpu)), dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    return halo_launch_status();
}

}  // extern "C"
