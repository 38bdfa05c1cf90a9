// The RNN transducer's training loss over the additive joint z[n, t, u, k] = f[n, t, k] + g[n, u, k] (haloop_amd/recognizer.py Transducer,
// ha/recognizer.py:104-126; [Graves12]) without any [N, T, U+1, V] tensor: the lattice (csrc/lattice.hip) reads two log-probabilities per
// cell, so the forward stores only those and the cell's log-sum-exp, and the backward rebuilds the softmax from f, g and lse.
//
//   1. rnnt_joint_fwd_kernel   workgroup = one n and a tile of frames, its f rows in LDS, the g rows streamed through LDS one u at a time;
//                              a wave takes a cell: lse = max + log sum exp(z - max) over the cell's own maximum, then
//                              lp2[.., 0] = z[0] - lse, lp2[.., 1] = z[y_u] - lse
//   2. halo_transducer_fwd / halo_transducer_bwd on lp2 as a K = 2 joint with targets of ones -> losses, alpha, d loss / d lp2 = (gb, gy)
//   3. rnnt_joint_bwd_kernel   dz[k] = gb [k = 0] + gy [k = y_u] - (gb + gy) exp(z[k] - lse), never stored: one launch owns (n, t) rows
//                              and sums over u in u order -> df, one owns (n, u) rows and sums over t in t order -> dg.  The owned rows
//                              and their accumulators live in LDS, the other operand's rows stream through LDS; every output element
//                              is summed by one thread in a fixed order (no atomics: bit-reproducible), the exponentials are computed
//                              twice.
// Every launch is finite (no grid barrier, no polling) and no workgroup reads what another workgroup of its launch writes.
// Exact fp32 in every math mode (no matrix product here).
#include "halo_common.h"
#include "halo_internal.h"

namespace {

constexpr int RJ_THREADS = 256, RJ_WAVES = RJ_THREADS / 64;
constexpr int RJ_MAX_TILE = 8;            // owned rows per workgroup, at most
constexpr int RJ_LDS_FLOATS = 16384;      // 64 KiB: what a tile is sized to (a single row set of a larger V takes more: the opt-in of dyn_lds.h)
constexpr int RJ_MAX_V = 8192;

struct RnntJointArgs {
    const float *f;              // [N][T][V], strides f_ns (n) and f_ts (t) in floats
    const float *g;              // [N][U1][V], strides g_ns and g_us
    long f_ns, f_ts, g_ns, g_us;
    int N, T, U1, V;
    const int64_t *targets;      // [N][U1 - 1]
    const int *f_len, *t_len;    // [N]
    float *lse;                  // [N][T][U1]
    float *lp2;                  // [N][T][U1][2]        (forward)
    const float *dlp2;           // [N][T][U1][2]        (backward)
    float *dout;                 // df or dg, strides d_ns (n) and d_rs (row)
    long d_ns, d_rs;
    int tile;                    // owned rows per workgroup
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// label of lattice row u (-1: none, or outside the vocabulary -- the host refuses those; never index with one)
__device__ __forceinline__ int label_at(const RnntJointArgs &p, int n, int u, int Un) {
    if (u >= Un) return -1;
    const int64_t y = p.targets[(long)n * (p.U1 - 1) + u];
    return (y < 0 || y >= p.V) ? -1 : (int)y;
}

// dynamic LDS: fs[tile][V] | gs[V]
__global__ __launch_bounds__(RJ_THREADS) void rnnt_joint_fwd_kernel(const RnntJointArgs p) {
    extern __shared__ float lds[];
    const int n = blockIdx.y, t0 = blockIdx.x * p.tile, V = p.V, U1 = p.U1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tn = clampi(p.f_len[n], 0, p.T), Un = clampi(p.t_len[n], 0, U1 - 1);
    const int rows = min(p.tile, p.T - t0), live = clampi(Tn - t0, 0, rows);
    float *fs = lds, *gs = lds + (long)p.tile * V;
    // cells outside the row's lengths: a fixed finite fill (the alpha sweep walks the whole lattice; nothing reads these as data)
    for (int c = threadIdx.x; c < rows * U1; c += RJ_THREADS) {
        const int r = c / U1, u = c - r * U1;
        if (r < live && u <= Un) continue;
        const long cell = ((long)n * p.T + t0 + r) * U1 + u;
        p.lse[cell] = 0.f; p.lp2[2 * cell] = 0.f; p.lp2[2 * cell + 1] = 0.f;
    }
    if (live == 0) return;
    for (int r = 0; r < live; ++r) {
        const float *src = p.f + (long)n * p.f_ns + (long)(t0 + r) * p.f_ts;
        for (int k = threadIdx.x; k < V; k += RJ_THREADS) fs[(long)r * V + k] = src[k];
    }
    for (int u = 0; u <= Un; ++u) {
        __syncthreads();                                    // the waves are done with the previous g row (first pass: nothing yet)
        const float *src = p.g + (long)n * p.g_ns + (long)u * p.g_us;
        for (int k = threadIdx.x; k < V; k += RJ_THREADS) gs[k] = src[k];
        __syncthreads();
        const int y = label_at(p, n, u, Un);
        for (int r = wave; r < live; r += RJ_WAVES) {
            const float *fr = fs + (long)r * V;
            float m = -INFINITY;
            for (int k = lane; k < V; k += 64) m = fmaxf(m, fr[k] + gs[k]);
            m = wave_max(m);
            float s = 0.f;
            for (int k = lane; k < V; k += 64) s += expf((fr[k] + gs[k]) - m);
            const float l = m + logf(wave_sum(s));
            if (lane == 0) {
                const long cell = ((long)n * p.T + t0 + r) * U1 + u;
                p.lse[cell] = l;
                p.lp2[2 * cell] = (fr[0] + gs[0]) - l;
                p.lp2[2 * cell + 1] = y >= 0 ? (fr[y] + gs[y]) - l : 0.f;
            }
        }
    }
}

// OWN_T: the workgroup owns a tile of frames of row n and writes df, streaming the g rows in u order; otherwise it owns a tile of u rows
// and writes dg, streaming the f rows in t order.  dynamic LDS: as[tile][V] | acc[tile][V] | bs[V]
template <bool OWN_T>
__global__ __launch_bounds__(RJ_THREADS) void rnnt_joint_bwd_kernel(const RnntJointArgs p) {
    extern __shared__ float lds[];
    const int n = blockIdx.y, a0 = blockIdx.x * p.tile, V = p.V, U1 = p.U1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tn = clampi(p.f_len[n], 0, p.T), Un = clampi(p.t_len[n], 0, U1 - 1);
    const int n_a = OWN_T ? p.T : U1, live_a = Tn == 0 ? 0 : (OWN_T ? Tn : Un + 1), live_b = OWN_T ? Un + 1 : Tn;
    const int rows = min(p.tile, n_a - a0), live = clampi(live_a - a0, 0, rows);
    const float *A = OWN_T ? p.f + (long)n * p.f_ns : p.g + (long)n * p.g_ns, *B = OWN_T ? p.g + (long)n * p.g_ns : p.f + (long)n * p.f_ns;
    const long a_rs = OWN_T ? p.f_ts : p.g_us, b_rs = OWN_T ? p.g_us : p.f_ts;
    float *as = lds, *acc = as + (long)p.tile * V, *bs = acc + (long)p.tile * V;
    float *out = p.dout + (long)n * p.d_ns;
    // rows past the utterance's lengths carry no gradient
    for (int r = live; r < rows; ++r)
        for (int k = threadIdx.x; k < V; k += RJ_THREADS) out[(long)(a0 + r) * p.d_rs + k] = 0.f;
    if (live == 0) return;
    for (int r = 0; r < live; ++r) {
        const float *src = A + (long)(a0 + r) * a_rs;
        for (int k = threadIdx.x; k < V; k += RJ_THREADS) { as[(long)r * V + k] = src[k]; acc[(long)r * V + k] = 0.f; }
    }
    for (int b = 0; b < live_b; ++b) {
        __syncthreads();
        const float *src = B + (long)b * b_rs;
        for (int k = threadIdx.x; k < V; k += RJ_THREADS) bs[k] = src[k];
        __syncthreads();
        // a wave owns rows wave, wave + RJ_WAVES, ... of the tile and a lane the symbols lane, lane + 64, ...: every acc element has one
        // owner, which adds the cells in the order of b
        for (int r = wave; r < live; r += RJ_WAVES) {
            const int t = OWN_T ? a0 + r : b, u = OWN_T ? b : a0 + r;
            const long cell = ((long)n * p.T + t) * U1 + u;
            const float l = p.lse[cell], gb = p.dlp2[2 * cell], gy = p.dlp2[2 * cell + 1], s = gb + gy;
            const int y = label_at(p, n, u, Un);
            const float *ar = as + (long)r * V;
            float *cr = acc + (long)r * V;
            for (int k = lane; k < V; k += 64) {
                float v = cr[k] - s * expf((ar[k] + bs[k]) - l);
                if (k == 0) v += gb;
                if (k == y) v += gy;
                cr[k] = v;
            }
        }
    }
    __syncthreads();
    for (int r = 0; r < live; ++r)
        for (int k = threadIdx.x; k < V; k += RJ_THREADS) out[(long)(a0 + r) * p.d_rs + k] = acc[(long)r * V + k];
}

// [n][r][V] rows addressed by (n stride, row stride): every row inside its own V floats, no two rows sharing an element
bool rows_disjoint(long ns, long rs, int N, int R, int V) {
    if ((N > 1 && ns < V) || (R > 1 && rs < V)) return false;
    if (N == 1 || R == 1) return true;
    return ns >= (long)(R - 1) * rs + V || rs >= (long)(N - 1) * ns + V;
}

int tile_rows(int V, int per_row_sets) {   // rows per workgroup with per_row_sets [tile][V] arrays and one streamed row in RJ_LDS_FLOATS
    return min(RJ_MAX_TILE, max(1, (RJ_LDS_FLOATS / V - 1) / per_row_sets));
}

bool joint_args(RnntJointArgs &p, const float *f, long f_ns, long f_ts, const float *g, long g_ns, long g_us, int N, int T, int U1, int V,
                const int64_t *targets, const int *f_lengths, const int *target_lengths, float *lse) {
    if (!f || !g || !targets || !f_lengths || !target_lengths || !lse) return false;
    if (N <= 0 || N > 65535 || T <= 0 || U1 < 2 || V < 1 || V > RJ_MAX_V) return false;
    if (2 * ((size_t)U1 + 1) * sizeof(float) > 60 * 1024) return false;          // what the lattice kernels accept
    if (!rows_disjoint(f_ns, f_ts, N, T, V) || !rows_disjoint(g_ns, g_us, N, U1, V)) return false;
    p.f = f; p.f_ns = f_ns; p.f_ts = f_ts; p.g = g; p.g_ns = g_ns; p.g_us = g_us; p.N = N; p.T = T; p.U1 = U1; p.V = V;
    p.targets = targets; p.f_len = f_lengths; p.t_len = target_lengths; p.lse = lse;
    p.lp2 = nullptr; p.dlp2 = nullptr; p.dout = nullptr; p.d_ns = p.d_rs = 0; p.tile = 1;
    return true;
}

}  // namespace

extern "C" {

int halo_rnnt_joint_fwd(const float *f, long f_n_stride, long f_t_stride, const float *g, long g_n_stride, long g_u_stride, int N, int T,
                        int U1, int V, const int64_t *targets, const int *f_lengths, const int *target_lengths, float *lse, float *lp2,
                        halo_stream_t stream) {
    RnntJointArgs p;
    HALO_CHECK_ARG(lp2);
    HALO_CHECK_ARG(joint_args(p, f, f_n_stride, f_t_stride, g, g_n_stride, g_u_stride, N, T, U1, V, targets, f_lengths, target_lengths, lse));
    p.lp2 = lp2;
    p.tile = tile_rows(V, 1);
    const int bytes = (int)(((size_t)p.tile + 1) * V * sizeof(float));
    const dim3 grid((unsigned)((T + p.tile - 1) / p.tile), (unsigned)N);
    if (halo_launch_lds<rnnt_joint_fwd_kernel>(grid, dim3(RJ_THREADS), bytes, (hipStream_t)stream, p) != HALO_OK) return HALO_ELAUNCH;
    return halo_launch_status();
}

int halo_rnnt_joint_bwd(const float *f, long f_n_stride, long f_t_stride, const float *g, long g_n_stride, long g_u_stride, int N, int T,
                        int U1, int V, const int64_t *targets, const int *f_lengths, const int *target_lengths, const float *lse,
                        const float *grad_lp2, float *df, long df_n_stride, long df_t_stride, float *dg, long dg_n_stride,
                        long dg_u_stride, halo_stream_t stream) {
    RnntJointArgs p;
    HALO_CHECK_ARG(grad_lp2 && df && dg);
    HALO_CHECK_ARG(joint_args(p, f, f_n_stride, f_t_stride, g, g_n_stride, g_u_stride, N, T, U1, V, targets, f_lengths, target_lengths,
                              (float *)lse));
    HALO_CHECK_ARG(rows_disjoint(df_n_stride, df_t_stride, N, T, V) && rows_disjoint(dg_n_stride, dg_u_stride, N, U1, V));
    p.dlp2 = grad_lp2;
    p.tile = tile_rows(V, 2);
    const int bytes = (int)((2 * (size_t)p.tile + 1) * V * sizeof(float));
    p.dout = df; p.d_ns = df_n_stride; p.d_rs = df_t_stride;
    if (halo_launch_lds<rnnt_joint_bwd_kernel<true>>(dim3((unsigned)((T + p.tile - 1) / p.tile), (unsigned)N), dim3(RJ_THREADS), bytes,
                                                     (hipStream_t)stream, p) != HALO_OK) return HALO_ELAUNCH;
    p.dout = dg; p.d_ns = dg_n_stride; p.d_rs = dg_u_stride;
    if (halo_launch_lds<rnnt_joint_bwd_kernel<false>>(dim3((unsigned)((U1 + p.tile - 1) / p.tile), (unsigned)N), dim3(RJ_THREADS), bytes,
                                                      (hipStream_t)stream, p) != HALO_OK) return HALO_ELAUNCH;
    return halo_launch_status();
}

}  // extern "C"
