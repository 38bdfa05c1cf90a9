// Greedy decode of the RNN transducer head (haloop_amd/recognizer.py Transducer; [Graves12] greedy search) as a sequence of short
// launches: per emitted symbol
//   1. rnnt_advance_kernel   one workgroup per row: walk the row's frames from t with the prediction network's output g fixed, the waves
//                            taking consecutive frames, until a frame's argmax of F[n, t] + g is not blank; consume the blanks, emit
//                            the symbol (or finish the row) and write its embedding as layer 0's next input
//   2. one launch per LSTM layer: gates = [x | h_prev] [W_ih | W_hh]^T over a decode image (the split three-MFMA product of
//      decode_linear.h, K = E + H) and the cell behind it in the same launch
//   3. out_layer: halo_decode_linear (csrc/decode.hip) on the image of the tied embedding -> g
// Blank frames cost no launch.  No grid barrier, no polling: every launch is finite.  No launch reads a buffer it writes, except a
// thread its own element (c of the cell; a row's state words by that row's workgroup).
//
// The carried search (haloop_amd/transducer.py GreedyStream) runs the same rounds over logits that arrive in chunks:
//   rnnt_stream_open_kernel       once per call, one workgroup per row: pos = 0, which rows take part, the reset of the rows that begin
//   rnnt_advance_kernel<true>     the advance over the call's chunk from pos; a row that runs out of frames waits (its state stays) and
//                                 every row gets a mask word: whether it emitted and needs the prediction network's step
//   the cell with a row mask      a row with mask 0 keeps c, has its h_prev copied to the other [x | h] copy and writes no h_up
#include <type_traits>
#include "halo_common.h"
#include "halo_internal.h"
#include "decode_linear.h"

namespace {

// ---- the cell behind the gate product.  The image's rows are permuted (haloop_amd/transducer.py) so that feature tile j holds, at
//      column 4 * q + i, gate q (i, f, g, o: nn.LSTM's order) of hidden unit 4 * j + i: one tile is everything four units need. ----
struct DecCellArgs : DecLinearArgs {
    const float *b_ih, *b_hh;   // [4H], nn.LSTM's layout (gate-major)
    float *c;                   // [rows][H], read and written by the same thread
    float *h_next;              // this layer's h for the NEXT step (the h half of the other [x | h] copy), leading dimension ld_next
    float *h_up;                // the same h as the x of the layer above in THIS step (or out_layer's input), leading dimension ld_up
    long ld_next, ld_up;
    int H;
    const int *row_mask;        // [rows] or NULL: a row with 0 sits this step out (c kept, h_prev copied to h_next, no h_up)

    template <int NT>
    __device__ __forceinline__ void finish(float (*red)[NT][64][4], int nt0) const {
        // D layout of the 16x16 MFMA: column = lane % 16, rows 4 * (lane / 16) + e
        for (int u = threadIdx.x; u < NT * 64; u += 256) {
            const int nt = u >> 6, l = u & 63;
            if (nt0 + nt >= n_tiles) continue;
            const int i = l & 3, rr = l >> 2;
            const int row = blockIdx.y * 16 + rr, unit = (nt0 + nt) * 4 + i;
            if (row >= rows || unit >= H) continue;
            if (row_mask && !row_mask[row]) {               // both [x | h] copies hold the row's h: either parity may read it next
                h_next[(long)row * ld_next + unit] = x[(long)row * ldx + H + unit];
                continue;
            }
            float gate[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int src = (rr >> 2) * 16 + 4 * q + i, e = rr & 3;
                const float v = (red[0][nt][src][e] + red[1][nt][src][e]) + (red[2][nt][src][e] + red[3][nt][src][e]);
                gate[q] = (v + b_ih[q * H + unit]) + b_hh[q * H + unit];
            }
            const float ig = sigmoidf_(gate[0]), fg = sigmoidf_(gate[1]), gg = tanhf(gate[2]), og = sigmoidf_(gate[3]);
            float *cp = c + (long)row * H + unit;
            const float cn = fg * *cp + ig * gg, hn = og * tanhf(cn);
            *cp = cn;
            h_next[(long)row * ld_next + unit] = hn;
            h_up[(long)row * ld_up + unit] = hn;
        }
    }
};

// ---- the advance.  state: int32 [5][state_ld] = t | u | here | done | truncated, one word of each per row. ----
struct RnntAdvanceArgs {
    const float *f;          // [N][T][V] transcription logits, strides f_rs (row) and f_ts (frame)
    long f_rs, f_ts;
    int T, V;
    const float *g, *g_bias; // [N][ldg] prediction logits without their bias; the bias [V] (may be NULL)
    long ldg;
    const int *il;           // [N] frames of each row (clipped to [0, T] here)
    int *state;
    long state_ld;
    float *score;            // [N]
    int64_t *tokens, *frames;   // [N][tok_ld], slots [0, capacity)
    long tok_ld;
    int capacity, max_symbols;
    const float *wte;        // [V][E] the embedding
    int E;
    float *x_next;           // [N][ldx]: layer 0's next input row
    long ldx;
    int *live;               // one word: += 1 per row that is not done after this launch
    int *pos, *row_mask;     // CARRIED: [N] the row's frame of this call's chunk; [N] whether the row emitted and goes on
};

constexpr int ADV_WAVES = 4;

// CARRIED: f is this call's chunk, il its frame counts; the row's word t counts the frames of the whole stream and pos those of the
// chunk.  `done` then means "sits out the rest of this call": rnnt_stream_open_kernel clears it for the rows of the next call that
// have frames and are not truncated.
template <bool CARRIED>
__global__ __launch_bounds__(64 * ADV_WAVES) void rnnt_advance_kernel(const RnntAdvanceArgs p) {
    extern __shared__ float gs[];                       // g[n, :] + bias, loaded once
    __shared__ int s_k[ADV_WAVES];
    __shared__ float s_lpk[ADV_WAVES], s_lp0[ADV_WAVES];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int *st_t = p.state + n, *st_u = st_t + p.state_ld, *st_here = st_u + p.state_ld, *st_done = st_here + p.state_ld,
        *st_trunc = st_done + p.state_ld;
    if (*st_done) {                                     // (uniform: one row per workgroup)
        if (CARRIED && threadIdx.x == 0) p.row_mask[n] = 0;
        return;
    }
    const int L = min(max(p.il[n], 0), p.T);
    // t: the row's frame of f; t0 + t: its frame of the stream
    int t = min(max(CARRIED ? p.pos[n] : *st_t, 0), L), u = *st_u, here = *st_here;
    const int t0 = CARRIED ? *st_t - t : 0;
    float score = p.score[n];
    __syncthreads();                                    // every thread has read the row's words before thread 0 rewrites them
    if (u < 0 || u >= p.capacity) {                     // cannot happen under the host's loop; never index past the slots
        if (threadIdx.x == 0) {
            *st_done = 1; *st_trunc = 1;
            if (CARRIED) p.row_mask[n] = 0;
        }
        return;
    }
    for (int v = threadIdx.x; v < p.V; v += 64 * ADV_WAVES) gs[v] = p.g[(long)n * p.ldg + v] + (p.g_bias ? p.g_bias[v] : 0.f);
    __syncthreads();
    int k = 0;                                          // the emitted symbol; 0: the row ran out of frames
    float lpk = 0.f;
    while (t < L) {
        // wave w: argmax (lowest index on ties) and log-sum-exp of frame t + w
        const int tw = t + wave;
        if (tw < L) {
            const float *row = p.f + (long)n * p.f_rs + (long)tw * p.f_ts;
            float m = -INFINITY;
            int am = 0x7fffffff;
            for (int v = lane; v < p.V; v += 64) {
                const float x = row[v] + gs[v];
                if (x > m) { m = x; am = v; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float om = __shfl_xor(m, o, 64);
                const int oa = __shfl_xor(am, o, 64);
                if (om > m || (om == m && oa < am)) { m = om; am = oa; }
            }
            float s = 0.f;
            for (int v = lane; v < p.V; v += 64) s += expf(row[v] + gs[v] - m);
            const float lse = m + logf(wave_sum(s));
            if (lane == 0) {
                s_k[wave] = am < p.V ? am : 0;
                s_lpk[wave] = m - lse;
                s_lp0[wave] = row[0] + gs[0] - lse;
            }
        }
        __syncthreads();
        // every thread walks the chunk's frames in order (the same arithmetic in every thread: uniform)
        bool emit = false;
        for (int w = 0; w < ADV_WAVES && t < L; ++w) {
            const bool forced = here == p.max_symbols;          // only at the first frame of a launch: a blank resets `here`
            if (s_k[w] == 0 || forced) {
                score += s_lp0[w];
                t += 1; here = 0;
            } else {
                k = s_k[w]; lpk = s_lpk[w];
                emit = true;
                break;
            }
        }
        __syncthreads();
        if (emit) break;
    }
    int done = 0, trunc = 0;
    if (k == 0) {
        done = 1;                                       // t == L
    } else {
        score += lpk;
        if (threadIdx.x == 0) {
            p.tokens[(long)n * p.tok_ld + u] = k;
            p.frames[(long)n * p.tok_ld + u] = t0 + t;
        }
        u += 1; here += 1;
        if (u == p.capacity) done = trunc = 1;
    }
    if (threadIdx.x == 0) {
        *st_t = t0 + t; *st_u = u; *st_here = here; *st_done = done; *st_trunc = trunc;
        p.score[n] = score;
        if (CARRIED) { p.pos[n] = t; p.row_mask[n] = !done; }
        if (!done) atomicAdd(p.live, 1);
    }
    if (done) return;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(p.wte + (long)k * p.E);
    f32x4 *dst = reinterpret_cast<f32x4 *>(p.x_next + (long)n * p.ldx);
    for (int i = threadIdx.x; i < p.E / 4; i += 64 * ADV_WAVES) dst[i] = src[i];
}

// ---- opening a call of the carried search: one workgroup per row of the state (rows >= B take no part in the call) ----
struct RnntOpenArgs {
    const int *n_frames, *flags;   // [B]; flags may be NULL (no row begins)
    int B;
    int *state;
    long state_ld;
    int *pos, *row_mask;           // [rows]
    float *score;
    int64_t *tokens, *frames;      // [rows][tok_ld], all `capacity` slots of a beginning row are reset
    long tok_ld;
    int capacity;
    float *xh;                     // the [x | h] copy the next step reads: [L][.][ldx], layers xh_ls floats apart
    long xh_ls, ldx;
    float *c;                      // [L][.][H], layers c_ls floats apart
    long c_ls;
    const float *wte;
    int E, H, L;
    int *live, n_live;             // the call's live words, zeroed here
};

constexpr int STREAM_FLAG_BEGIN = 2;   // include/halo.h: bit 1 of the per-stream flags

__global__ __launch_bounds__(256) void rnnt_stream_open_kernel(const RnntOpenArgs p) {
    const int n = blockIdx.x, tid = threadIdx.x;
    if (n == 0)
        for (int i = tid; i < p.n_live; i += 256) p.live[i] = 0;
    int *st_t = p.state + n, *st_u = st_t + p.state_ld, *st_here = st_u + p.state_ld, *st_done = st_here + p.state_ld,
        *st_trunc = st_done + p.state_ld;
    const bool in = n < p.B;
    const bool begin = in && p.flags && (p.flags[n] & STREAM_FLAG_BEGIN);
    const int nf = in ? p.n_frames[n] : 0;
    const int trunc = begin ? 0 : *st_trunc;
    if (begin) {
        for (int i = tid; i < p.capacity; i += 256) {
            p.tokens[(long)n * p.tok_ld + i] = -1;
            p.frames[(long)n * p.tok_ld + i] = -1;
        }
        for (int i = tid; i < p.L * p.H; i += 256) {
            const int l = i / p.H, j = i % p.H;
            p.xh[l * p.xh_ls + (long)n * p.ldx + p.H + j] = 0.f;
            p.c[l * p.c_ls + (long)n * p.H + j] = 0.f;
        }
        for (int i = tid; i < p.E; i += 256) p.xh[(long)n * p.ldx + i] = p.wte[i];     // the zero prefix of training
    }
    if (tid == 0) {
        if (begin) { *st_t = 0; *st_u = 0; *st_here = 0; *st_trunc = 0; p.score[n] = 0.f; }
        *st_done = (nf <= 0 || trunc) ? 1 : 0;
        p.pos[n] = 0;
        p.row_mask[n] = begin ? 1 : 0;          // one masked step of the prediction network gives a beginning row its g
    }
}

// [a, a + an) and [b, b + bn) floats share no element
bool disjoint(const float *a, long an, const float *b, long bn) { return a + an <= b || b + bn <= a; }

template <bool CARRIED>
int advance(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg, const float *g_bias,
            const int *input_lengths, int *state, long state_ld, float *scores, int64_t *tokens, int64_t *frames, long tokens_ld,
            int capacity, int max_symbols, const float *wte, int E, float *x_next, long ldx, int *live, int *pos, int *row_mask,
            halo_stream_t stream) {
    HALO_CHECK_ARG(f && g && input_lengths && state && scores && tokens && frames && wte && x_next && live);
    HALO_CHECK_ARG(N > 0 && T > 0 && V > 0 && V <= 8192 && capacity > 0 && max_symbols > 0);
    HALO_CHECK_ARG(f_frame_stride >= V && f_row_stride >= (long)(T - 1) * f_frame_stride + V && ldg >= V && state_ld >= N);
    HALO_CHECK_ARG(tokens_ld >= capacity && E > 0 && E % 4 == 0 && ldx >= E && ldx % 4 == 0);
    HALO_CHECK_ARG(((uintptr_t)wte | (uintptr_t)x_next) % 16 == 0);
    HALO_CHECK_ARG(!CARRIED || (pos && row_mask));
    RnntAdvanceArgs p;
    p.f = f; p.f_rs = f_row_stride; p.f_ts = f_frame_stride; p.T = T; p.V = V; p.g = g; p.g_bias = g_bias; p.ldg = ldg;
    p.il = input_lengths; p.state = state; p.state_ld = state_ld; p.score = scores; p.tokens = tokens; p.frames = frames;
    p.tok_ld = tokens_ld; p.capacity = capacity; p.max_symbols = max_symbols; p.wte = wte; p.E = E; p.x_next = x_next; p.ldx = ldx;
    p.live = live; p.pos = pos; p.row_mask = row_mask;
    hipLaunchKernelGGL(rnnt_advance_kernel<CARRIED>, dim3((unsigned)N), dim3(64 * ADV_WAVES), (size_t)V * sizeof(float), (hipStream_t)stream, p);
    return halo_launch_status();
}

int cell(const float *xh, long ldx, int rows, int hidden, const void *w_image, const float *b_ih, const float *b_hh, float *c,
         float *h_next, long ld_next, float *h_up, long ld_up, const int *row_mask, halo_stream_t stream) {
    HALO_CHECK_ARG(xh && w_image && b_ih && b_hh && c && h_next && h_up && rows > 0 && hidden > 0 && hidden % 4 == 0);
    const int K = 2 * hidden;
    HALO_CHECK_ARG(halo_decode_linear_supported(K, 0) && ldx >= K && ldx % 4 == 0 && ld_next >= hidden && ld_up >= hidden);
    HALO_CHECK_ARG(((uintptr_t)xh | (uintptr_t)w_image) % 16 == 0);
    // the launch reads xh and writes h_next / h_up from other workgroups: they may not overlap it (nor each other, nor c)
    const long xn = (long)(rows - 1) * ldx + K, nn = (long)(rows - 1) * ld_next + hidden, un = (long)(rows - 1) * ld_up + hidden;
    HALO_CHECK_ARG(disjoint(xh, xn, h_next, nn) && disjoint(xh, xn, h_up, un) && disjoint(xh, xn, c, (long)rows * hidden));
    HALO_CHECK_ARG(disjoint(h_next, nn, h_up, un) && disjoint(c, (long)rows * hidden, h_next, nn) && disjoint(c, (long)rows * hidden, h_up, un));
    DecCellArgs p;
    p.x = xh; p.ldx = ldx; p.rows = rows; p.K = K; p.lnw = nullptr; p.eps = 0.f; p.w = (const char *)w_image;
    p.n_tiles = hidden / 4; p.n_out = 4 * hidden; p.out = nullptr; p.ldo = 0; p.flags = 0;
    p.x2 = nullptr; p.side_in = nullptr; p.side_out = nullptr;
    p.b_ih = b_ih; p.b_hh = b_hh; p.c = c; p.h_next = h_next; p.h_up = h_up; p.ld_next = ld_next; p.ld_up = ld_up; p.H = hidden;
    p.row_mask = row_mask;
    const int row_groups = (rows + 15) / 16;
    // two feature tiles per workgroup while that still gives the chip a workgroup per CU, else one (as halo_decode_linear)
    const bool two = (long)((p.n_tiles + 1) / 2) * row_groups >= 256;
    const dim3 grid((unsigned)(two ? (p.n_tiles + 1) / 2 : p.n_tiles), (unsigned)row_groups);
    if (two) hipLaunchKernelGGL((dec_linear_kernel<2, 0, 3, 8, DecCellArgs>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((dec_linear_kernel<1, 0, 3, 8, DecCellArgs>), grid, dim3(256), 0, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // namespace

extern "C" {

int halo_rnnt_advance(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                      const float *g_bias, const int *input_lengths, int *state, long state_ld, float *scores, int64_t *tokens,
                      int64_t *frames, long tokens_ld, int capacity, int max_symbols, const float *wte, int E, float *x_next, long ldx,
                      int *live, halo_stream_t stream) {
    return advance<false>(f, f_row_stride, f_frame_stride, N, T, V, g, ldg, g_bias, input_lengths, state, state_ld, scores, tokens, frames,
                          tokens_ld, capacity, max_symbols, wte, E, x_next, ldx, live, nullptr, nullptr, stream);
}

int halo_rnnt_advance_stream(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                             const float *g_bias, const int *n_frames, int *state, long state_ld, float *scores, int64_t *tokens,
                             int64_t *frames, long tokens_ld, int capacity, int max_symbols, const float *wte, int E, float *x_next,
                             long ldx, int *live, int *pos, int *row_mask, halo_stream_t stream) {
    return advance<true>(f, f_row_stride, f_frame_stride, N, T, V, g, ldg, g_bias, n_frames, state, state_ld, scores, tokens, frames,
                         tokens_ld, capacity, max_symbols, wte, E, x_next, ldx, live, pos, row_mask, stream);
}

int halo_rnnt_stream_open(const int *n_frames, const int *flags, int B, int rows, int *state, long state_ld, int *pos, int *row_mask,
                          float *scores, int64_t *tokens, int64_t *frames, long tokens_ld, int capacity, float *xh, long xh_layer_stride,
                          long ldx, float *c, long c_layer_stride, const float *wte, int E, int hidden, int layers, int *live, int n_live,
                          halo_stream_t stream) {
    HALO_CHECK_ARG(n_frames && state && pos && row_mask && scores && tokens && frames && xh && c && wte && live);
    HALO_CHECK_ARG(B > 0 && rows >= B && state_ld >= rows && capacity > 0 && tokens_ld >= capacity && n_live >= 0);
    HALO_CHECK_ARG(E > 0 && hidden > 0 && layers > 0 && ldx >= 2 * (long)hidden && ldx >= E);
    HALO_CHECK_ARG(xh_layer_stride >= (long)rows * ldx && c_layer_stride >= (long)rows * hidden);
    RnntOpenArgs p;
    p.n_frames = n_frames; p.flags = flags; p.B = B; p.state = state; p.state_ld = state_ld; p.pos = pos; p.row_mask = row_mask;
    p.score = scores; p.tokens = tokens; p.frames = frames; p.tok_ld = tokens_ld; p.capacity = capacity; p.xh = xh;
    p.xh_ls = xh_layer_stride; p.ldx = ldx; p.c = c; p.c_ls = c_layer_stride; p.wte = wte; p.E = E; p.H = hidden; p.L = layers;
    p.live = live; p.n_live = n_live;
    hipLaunchKernelGGL(rnnt_stream_open_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p);
    return halo_launch_status();
}

int halo_rnnt_lstm_cell(const float *xh, long ldx, int rows, int hidden, const void *w_image, const float *b_ih, const float *b_hh,
                        float *c, float *h_next, long ld_next, float *h_up, long ld_up, halo_stream_t stream) {
    return cell(xh, ldx, rows, hidden, w_image, b_ih, b_hh, c, h_next, ld_next, h_up, ld_up, nullptr, stream);
}

int halo_rnnt_lstm_cell_rows(const float *xh, long ldx, int rows, int hidden, const void *w_image, const float *b_ih, const float *b_hh,
                             float *c, float *h_next, long ld_next, float *h_up, long ld_up, const int *row_mask, halo_stream_t stream) {
    return cell(xh, ldx, rows, hidden, w_image, b_ih, b_hh, c, h_next, ld_next, h_up, ld_up, row_mask, stream);
}

}  // extern "C"
