// Edit distance on the device, and the minimum-word-error-rate risk built on it, for gfx950.  Integer throughout (the
// risk: fp32), no atomics, no workspace, finite launches: no workgroup reads what another workgroup writes.
//
// halo_edit_distance: one workgroup per (hypothesis, reference) pair walks the Levenshtein table D[i][j] (i hypothesis tokens against j
// reference tokens) along its anti-diagonals.  The pair count is small and the chain is Lh + Lr steps long, so what counts is the latency
// of one step, as in viterbi.hip:
//   - a thread owns PER consecutive columns j; at step s it takes the cells (s - j, j).  Of the three predecessors, (i-1, j) is the
//     thread's own value of step s-1, and (i, j-1) / (i-1, j-1) are the left column's values of steps s-1 / s-2: the left column is the
//     thread's own register for all but its first column, whose left neighbour arrives by one wave shuffle per step (up to 64 columns: one
//     wave, no LDS and no barrier on the chain) or through one LDS word per thread, double buffered, one barrier per step.  The value of
//     step s-2 is the one received a step earlier, kept in a register.
//   - a cell is one 32-bit word, cost << 18 | ins: with the predecessor's rank (0 diagonal, 1 deletion, 2 insertion) put into bits 16-17
//     of the three candidates, one unsigned min3 selects the smallest cost and, among equal costs, the tie order of include/halo.h, and
//     carries the insertion count of the chosen path with it.  The other two counts follow from identities every path obeys:
//     del = ins + j - i, sub = cost - ins - del.  No back-pointers, no backtrace.
//   - column 0 (D[i][0] = i insertions) and row 0 (D[0][j] = j deletions) are formed in registers, so the columns of the threads are
//     j = 1 .. Lr and 64 lanes hold Lr = 64.
//   - token loads are off the chain: a thread's reference tokens are loaded once; the hypothesis token of its first column is requested
//     D steps ahead of its use and then handed from column to column in registers.  Every load is issued unconditionally from a clamped
//     index inside the pair's own lengths (a cell outside the table computes a value nobody reads), so padding is never loaded.
#include "halo_common.h"

namespace {

constexpr unsigned COST_ONE = 1u << 18, RANK_MASK = 3u << 16;
constexpr unsigned STEP_DEL = COST_ONE | (1u << 16), STEP_INS = COST_ONE | (2u << 16) | 1u;
constexpr int MAX_LEN = HALO_EDIT_DISTANCE_MAX_LEN;      // 4 columns per thread of 256; costs stay far below 2^14, counts below 2^16

__device__ __forceinline__ unsigned cell(int cost, int ins) { return ((unsigned)cost << 18) | (unsigned)ins; }

struct EditArgs {
    const int64_t *hyp;
    long hyp_stride;
    const int *hyp_len;
    int Lh;
    const int64_t *ref;
    long ref_stride;
    const int *ref_len;
    int Lr, group;
    int *errors, *counts;
};

template <int BLK, int PER, int D>
__global__ __launch_bounds__(BLK) void edit_distance_kernel(const EditArgs p) {
    constexpr bool ONE_WAVE = BLK == 64;
    __shared__ unsigned edge[2][BLK + 1];                // [step parity][1 + tid]: the thread's last column, for the thread to its right
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int hl = p.hyp_len[pair];
    const int lh = min(hl, p.Lh), lr = max(0, min(p.ref_len[pair / p.group], p.Lr));
    if (hl < 0 || lh == 0 || lr == 0) {                  // absent, or one side empty: nothing to walk, and no token is loaded
        if (tid == 0) {
            p.errors[pair] = hl < 0 ? -1 : lh + lr;
            int *cnt = p.counts + (long)pair * 3;
            cnt[0] = hl < 0 ? 0 : lh; cnt[1] = hl < 0 ? 0 : lr; cnt[2] = 0;
        }
        return;
    }
    const int64_t *hyp = p.hyp + (long)pair * p.hyp_stride, *ref = p.ref + (long)(pair / p.group) * p.ref_stride;
    const int col0 = tid * PER;                          // this thread's columns: j = col0 + k + 1
    auto token = [&](int s) { return hyp[min(max(s - col0 - 2, 0), lh - 1)]; };      // of the first column's cell at step s

    int64_t r[PER], h[PER];
    unsigned a[PER], c[PER];                             // own column at step s-1; left column at step s-2
    const int64_t h0 = hyp[0];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        r[k] = ref[min(col0 + k, lr - 1)];
        h[k] = h0;
        a[k] = cell(col0 + k + 1, 0);                    // step 1: every column is still in row 0 (or above it)
        c[k] = cell(col0 + k, 0);
    }
    int64_t nxt[D];
#pragma unroll
    for (int j = 0; j < D; ++j) nxt[j] = token(2 + j);
    if (!ONE_WAVE) {
        edge[0][tid + 1] = 0; edge[1][tid + 1] = a[PER - 1];
        if (tid == 0) edge[0][0] = edge[1][0] = 0;       // column 0 is formed in registers: the word is read and dropped
        __syncthreads();
    }

    const int last = lh + lr;
    for (int s0 = 2; s0 <= last; s0 += D) {
        int64_t e[D];
#pragma unroll
        for (int j = 0; j < D; ++j) e[j] = nxt[j];
        // the next chunk's hypothesis tokens are requested here, a whole chunk of steps before the chain needs them
#pragma unroll
        for (int j = 0; j < D; ++j) nxt[j] = token(s0 + D + j);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int s = s0 + j;
            if (s > last) break;
#pragma unroll
            for (int k = PER - 1; k > 0; --k) h[k] = h[k - 1];
            h[0] = e[j];
            unsigned b[PER];                             // left column at step s-1
            b[0] = ONE_WAVE ? __shfl_up(a[PER - 1], 1, 64) : edge[(s - 1) & 1][tid];
            if (tid == 0) b[0] = cell(s - 1, s - 1);     // column 0: cell (s - 1, 0), all insertions
#pragma unroll
            for (int k = 1; k < PER; ++k) b[k] = a[k - 1];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int col = col0 + k + 1;
                const unsigned diag = c[k] + (h[k] != r[k] ? COST_ONE : 0u);
                const unsigned v = min(min(diag, b[k] + STEP_DEL), a[k] + STEP_INS) & ~RANK_MASK;
                a[k] = s - col <= 0 ? cell(col, 0) : v;  // row 0, and the steps before the column enters the table
                c[k] = b[k];
            }
            if (!ONE_WAVE) {
                edge[s & 1][tid + 1] = a[PER - 1];
                __syncthreads();
            }
        }
    }
    if (tid == (lr - 1) / PER) {
        unsigned v = a[0];
#pragma unroll
        for (int k = 1; k < PER; ++k)
            if (k == (lr - 1) % PER) v = a[k];
        const int cost = (int)(v >> 18), ins = (int)(v & 0xffffu), del = ins + lr - lh;
        p.errors[pair] = cost;
        int *cnt = p.counts + (long)pair * 3;
        cnt[0] = ins; cnt[1] = del; cnt[2] = cost - ins - del;
    }
}

constexpr int RISK_MAX = 16;     // hypotheses of a row: transducer.BEAM_MAX

// One thread per row; the sums run in hypothesis order, so the result does not depend on the launch shape.
__global__ __launch_bounds__(64) void nbest_risk_kernel(const float *losses, const int *errors, int N, int W, const float *grad_risk,
                                                        float *risk, float *dlosses) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const float *l = losses + (long)n * W;
    const int *er = errors + (long)n * W;
    float lmin = INFINITY, esum = 0.f;
    int present = 0;
    for (int w = 0; w < W; ++w)
        if (er[w] >= 0) {
            lmin = fminf(lmin, l[w]);
            esum += (float)er[w];
            ++present;
        }
    float z = 0.f, num = 0.f;
    for (int w = 0; w < W; ++w) {
        const float ex = er[w] >= 0 ? expf(lmin - l[w]) : 0.f;       // the largest -loss is taken out before the exponentials
        z += ex;
        num += ex * (float)max(er[w], 0);
    }
    const float expected = present ? num / z : 0.f;
    if (risk) risk[n] = present ? expected - esum / (float)present : 0.f;
    if (dlosses) {
        const float go = grad_risk[n];
        for (int w = 0; w < W; ++w)
            dlosses[(long)n * W + w] = er[w] >= 0 ? go * (-(expf(lmin - l[w]) / z) * ((float)er[w] - expected)) : 0.f;
    }
}

}  // namespace

extern "C" {

int halo_edit_distance(const int64_t *hyp, long hyp_stride, const int *hyp_lengths, int P, int Lh, const int64_t *ref, long ref_stride,
                       const int *ref_lengths, int R, int Lr, int group, int *errors, int *counts, halo_stream_t stream) {
    HALO_CHECK_ARG(hyp_lengths && ref_lengths && errors && counts);
    HALO_CHECK_ARG(P > 0 && R > 0 && group > 0 && (long)R * group == (long)P && Lh >= 0 && Lr >= 0);
    HALO_CHECK_ARG((hyp || Lh == 0) && (ref || Lr == 0) && hyp_stride >= Lh && ref_stride >= Lr);
    if (Lh > MAX_LEN || Lr > MAX_LEN) return HALO_ENOTSUP;
    EditArgs a;
    a.hyp = hyp; a.hyp_stride = hyp_stride; a.hyp_len = hyp_lengths; a.Lh = Lh; a.ref = ref; a.ref_stride = ref_stride;
    a.ref_len = ref_lengths; a.Lr = Lr; a.group = group; a.errors = errors; a.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    // columns per thread and steps of hypothesis tokens in flight, by the reference's width: one wave up to 64, then 256 threads
    if (Lr <= 64) hipLaunchKernelGGL((edit_distance_kernel<64, 1, 8>), dim3(P), dim3(64), 0, st, a);
    else if (Lr <= 256) hipLaunchKernelGGL((edit_distance_kernel<256, 1, 8>), dim3(P), dim3(256), 0, st, a);
    else if (Lr <= 512) hipLaunchKernelGGL((edit_distance_kernel<256, 2, 8>), dim3(P), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((edit_distance_kernel<256, 4, 8>), dim3(P), dim3(256), 0, st, a);
    return halo_launch_status();
}

int halo_nbest_risk_fwd(const float *losses, const int *errors, int N, int W, float *risk, halo_stream_t stream) {
    HALO_CHECK_ARG(losses && errors && risk && N > 0 && W >= 1);
    if (W > RISK_MAX) return HALO_ENOTSUP;
    hipLaunchKernelGGL(nbest_risk_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, losses, errors, N, W, nullptr, risk, nullptr);
    return halo_launch_status();
}

int halo_nbest_risk_bwd(const float *losses, const int *errors, int N, int W, const float *grad_risk, float *dlosses, halo_stream_t stream) {
    HALO_CHECK_ARG(losses && errors && grad_risk && dlosses && N > 0 && W >= 1);
    if (W > RISK_MAX) return HALO_ENOTSUP;
    hipLaunchKernelGGL(nbest_risk_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, losses, errors, N, W, grad_risk, nullptr, dlosses);
    return halo_launch_status();
}

}  // extern "C"
