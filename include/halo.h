/*
 * halo.h -- C ABI of libhalo.so, the MI355X (gfx950) engine for haloop's acoustic hot path.
 *
 * The reference (proger/haloop, /root/reference) has no FFI: its "boundary" is the Python
 * surface of ha.rnn / ha.recognizer / ha.ctc / ha.beam, under which it calls stock torch
 * operators (cuDNN LSTM, ATen ctc_loss, ...).  Each entry point below replaces one of those
 * operator call sites; the citation after "replaces:" is the reference line that makes the call.
 * The modules under haloop_amd/ are the binding (ctypes) that keeps the reference's Python signatures.
 *
 * Conventions
 *   - plain pointers are DEVICE pointers unless a parameter is documented "host";
 *   - every buffer (outputs, reserve, workspace) is caller-allocated; *_bytes() queries sizes;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing here allocates,
 *     frees, synchronises or throws, so calls are capturable in a hipGraph;
 *   - return value: HALO_OK (0) or a negative HALO_E* code; halo_strerror() names it;
 *   - threads: every switch a halo_set_* entry changes lives in a settings record ("Contexts" below); calls from different threads are
 *     independent when each thread has selected its own context (and its own scratch buffer) and works on its own stream; calls that
 *     share a record -- the process-wide default one included -- must be serialised by the caller.  The persistent LSTM recurrences need
 *     every CU of the device while they run (~0.1 ms): other work on the GPU delays them, it cannot deadlock them (every wait is bounded);
 *   - dense fp32 math (arithmetic mode f32) runs on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32), i.e. k-ordered fmaf
 *     chains, no reduced precision; modes bf16x3 / bf16: halo_set_math_mode.
 */
#ifndef HALO_H
#define HALO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALO_ABI_VERSION 21

#define HALO_OK 0
#define HALO_EINVAL (-22)    /* bad argument (null pointer, non-positive size, unsupported shape) */
#define HALO_ENOTSUP (-95)   /* shape outside what the kernels were built for */
#define HALO_ELAUNCH (-5)    /* hipLaunchKernel reported an error */

typedef void *halo_stream_t; /* hipStream_t */

int halo_abi_version(void);
/* Measurement aid (tools/pmc_calibrate.py): one launch that READS exactly `bytes` bytes of src once with a chosen access shape, so that
 * rocprofv3's FETCH_SIZE counter can be calibrated per load width (MI355X_MICROARCH.md: "other access widths are uncalibrated").
 * pattern 0: 16 B per lane (global_load_dwordx4); 1: 4 B per lane, 256 B contiguous per wave instruction; 2: 4 B per lane in 64-byte
 * segments of four rows row_bytes apart (the saved-activation loads of the persistent recurrences); 3: 16 B per lane buffer loads
 * with sc1 (their fragment loads).  sink: one float nobody reads. */
int halo_debug_read(const void *src, size_t bytes, int pattern, size_t row_bytes, float *sink, void *stream);
const char *halo_strerror(int code);
/* Device sanity for the loader: returns HALO_OK and fills arch (e.g. "gfx950") and CU count. */
int halo_device_info(int device, char *arch, int arch_len, int *cu_count);

/* Arithmetic of the dense products (large GEMMs, the recurrent LSTM GEMM, attention Q.K^T / P.V and their gradients):
 *   HALO_MATH_F32     exact-f32 MFMA (default)
 *   HALO_MATH_BF16X3  operands split into bf16 hi+lo, three bf16 MFMAs per product, fp32 accumulate
 *                     (~2^-16 relative error per product; 5.3x the f32 matrix rate): fp32-grade results
 *   HALO_MATH_BF16    operands rounded to bf16, one MFMA per product, fp32 accumulate -- the arithmetic of the reference's
 *                     `torch.autocast(dtype=bfloat16)` runs (ha/attention_loop.py:87); GEMMs and attention only, the
 *                     recurrent LSTM step keeps the split form.  State, softmax, LayerNorm, losses stay fp32 in every mode.
 * Process-wide; set it before the first call / graph capture. */
#define HALO_MATH_F32 0
#define HALO_MATH_BF16X3 1
#define HALO_MATH_BF16 2
int halo_set_math_mode(int mode);
int halo_get_math_mode(void);

/* Multi-layer LSTM schedule (HALO_MATH_BF16X3, H % 64 == 0, 2..4 layers):
 *   0 (default)  per-layer: each layer's T steps in turn, input projections as batched GEMMs;
 *   1            layer-diagonal fusion: one launch per diagonal runs step d-l of every layer l, the
 *                upper layers' input projection (forward) and input gradient (backward) folded into
 *                the step as extra contraction depth.  Same results; measured 2.7 % slower at
 *                LC-2x1024/B=64 (the batched GEMMs move W_ih more efficiently than 21 folded steps),
 *                so it is off by default. */
int halo_set_lstm_fusion(int on);

/* Optional scratch for split-K partial sums.  The library never allocates: the caller may lend it
 * one persistent device buffer (16-byte aligned; 64 MiB is plenty for this model).  With it, GEMMs
 * whose output has too few tiles to fill 256 CUs are split along K into slabs that a second launch
 * sums in a fixed order (bitwise reproducible); without it they run unsplit.  Calls that use the
 * scratch must be ordered on one stream.  Pass NULL to withdraw it. */
int halo_set_scratch(void *device_ptr, size_t bytes);

/* ------------------------------------------------------------------------------------------
 * Dropout stream.  Philox4x32-10, counter = (lo32(e>>2), hi32(e>>2), stream_id, offset),
 * key = seed, value = out[e&3], keep iff value >= uint32(p*2^32), scale 1/(1-p).
 * e is the flat element index of the tensor the mask is applied to.  Every entry point that
 * takes `offset` also takes `offset_dev`, an optional DEVICE uint32 that is added to it when the
 * kernel runs, so a captured hipGraph draws fresh masks on every replay.
 * replaces: torch's nn.Dropout RNG at ha/rnn.py:8,24, nn.LSTM(dropout=) rnn.py:11 and
 * ha/recognizer.py:41,44 (the reference stream itself is not reproducible).
 * ------------------------------------------------------------------------------------------ */
#define HALO_STREAM_SUBSAMPLE 1u
#define HALO_STREAM_CLASSIFIER 2u
#define HALO_STREAM_LSTM_LAYER0 16u /* + layer index */

/* y[i] = x[i] * mask(i);  replaces: self.dropout(features) ha/recognizer.py:44 */
int halo_dropout_fwd(const float *x, float *y, size_t n, float p, uint64_t seed, uint32_t stream_id,
                     uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
/* *counter += 1 (the device-side step counter that offset_dev points at) */
int halo_counter_inc(uint32_t *counter, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dense GEMM on the exact-f32 MFMA.  C[M,N] = opA(A)[M,K] * opB(B)[K,N]  (+ epilogue)
 *   a_kcontig = 1: A stored [M,K] (row stride lda), 0: A stored [K,M]
 *   b_kcontig = 1: B stored [N,K] (row stride ldb), 0: B stored [K,N]
 * epilogue, in this order: + bias1[n] + bias2[n] (either may be NULL); relu / tanh-GELU per flags;
 *   * dropout mask(e = m*ldc + n) if p_drop > 0; + previous C if HALO_GEMM_ACCUM.
 * replaces: the ATen/oneDNN/cuBLAS matmuls under nn.Conv1d rnn.py:22, nn.LSTM input
 * projections rnn.py:25 and nn.Linear recognizer.py:45, and their autograd backward GEMMs.
 * ------------------------------------------------------------------------------------------ */
#define HALO_GEMM_RELU 1
#define HALO_GEMM_GELU 2   /* tanh-GELU ("new_gelu", ha/attention.py:12-17), applied after the bias */
#define HALO_GEMM_ACCUM 4  /* C += result (residual connections, ha/attention.py:178-179) */
#define HALO_GEMM_GELU_ERF 8 /* exact GELU (nn.GELU() ha/transformer.py:456, F.gelu ha/conv.py:46), after the bias */
int halo_gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K, const float *A, int lda,
                  const float *B, int ldb, float *C, int ldc, const float *bias1, const float *bias2,
                  int flags, float p_drop, uint64_t seed, uint32_t stream_id, uint32_t offset,
                  const uint32_t *offset_dev, halo_stream_t stream);

/* Split-bf16 GEMM on pre-tiled operand images (the HALO_MATH_BF16X3 path, usable on its own).
 *   halo_split_image: logical X[rows][k] (fp32; memory [rows][k], or [k][rows] when src_transposed,
 *     leading dimension ld) -> image of halo_split_image_bytes(rows, k) bytes holding bf16 hi/lo
 *     parts in 128x32 tiles laid out as the MFMA fragment reads want them (zero padded).
 *   halo_gemm_split: C[M,N] = A[M,K] * B[N,K]^T from two images (fp32 accumulate, three bf16 MFMAs
 *     per product), epilogue as halo_gemm_f32.  An operand used by several GEMMs is split once.
 * replaces: the same matmuls as halo_gemm_f32. */
size_t halo_split_image_bytes(int rows, int k);
int halo_split_image(const float *src, int rows, int k, int ld, int src_transposed, void *image,
                     halo_stream_t stream);
/* F.layer_norm(x, (C,), weight, bias|NULL, eps) written straight into the split image of its rows (the A operand of the Linear
 * that follows: ln_1 -> c_attn, ln_2 -> c_fc, ha/attention.py:175-179; ln_time / ln_chan, ha/transformer.py:476,495), and
 * optionally as fp32 rows y (NULL to skip).  C % 32 == 0. */
int halo_layernorm_image(const float *x, const float *weight, const float *bias, float *y, void *image, int rows, int C,
                         float eps, halo_stream_t stream);
/* The same LayerNorm with the normalised rows as ROW-MAJOR bf16 [rows][C] (C % 8 == 0) -- the operand form halo_gemm_split_io (a_hi) and
 * halo_gemm_tn_bf16 read; y (fp32 rows) and image (the tiled image as well, C % 32 == 0) are optional: a product that stages its A operand
 * from row-major rows fetches half cache lines and runs 10-15 % slower from cold caches than from the image, so the forward
 * product of a training step takes the image and the weight-gradient product the rows, both from this one launch. */
int halo_layernorm_bf16(const float *x, const float *weight, const float *bias, float *y, void *y_bf16, void *image, int rows, int C,
                        float eps, halo_stream_t stream);
/* n fp32 values -> bf16 (n % 8 == 0, 16-byte aligned): row-major bf16 operands from fp32 tensors no launch produced as bf16 */
int halo_cast_bf16(const float *x, void *y, size_t n, halo_stream_t stream);
/* The GPT MLP's two elementwise passes with a bf16 result (n % 8 == 0, 16-byte aligned): y = gelu(a) -- the c_proj input, never needed in
 * fp32 -- and da = dy * gelu'(a) (exact: 0 tanh form new_gelu ha/attention.py:12-17, 1 erf form).  Measured against the same math in the
 * producing GEMM's epilogue (GPT training direction): the separate pass is hidden under its HBM stream, the epilogue is not. */
int halo_gelu_bf16(const float *a, void *y_bf16, size_t n, int exact, halo_stream_t stream);
int halo_gelu_bwd_bf16(const float *dy, const float *a, void *da_bf16, size_t n, int exact, halo_stream_t stream);
/* ... and with bf16 on BOTH sides (round 5: the c_fc product and the c_proj input-gradient product leave their results as row-major
 * bf16, halo_gemm_rows -- what the reference's autocast path holds there, ha/attention_loop.py:164): fp32 arithmetic on the bf16 values. */
int halo_gelu_b16(const void *a_bf16, void *y_bf16, size_t n, int exact, halo_stream_t stream);
int halo_gelu_bwd_b16(const void *dy_bf16, const void *a_bf16, void *da_bf16, size_t n, int exact, halo_stream_t stream);
/* One read of an fp32 matrix src [rows][cols] (leading dimension ld), optionally through an elementwise operator, written as
 * BOTH split images a Linear's backward consumes: image_rows = halo_split_image(value [rows][cols]) (the A operand of
 * dx = dy W, ha/attention.py:117-129,141) and image_cols = halo_split_image(value^T [cols][rows]) (the operand of dW = dy^T x);
 * either may be NULL.  The fp32 value itself is never written.  op:
 *   HALO_PAIR_COPY            value = src
 *   HALO_PAIR_GELU_TANH/_ERF  value = gelu(src)                (forward of new_gelu ha/attention.py:12-17 / nn.GELU())
 *   HALO_PAIR_GELU_*_BWD      value = src * gelu'(src2)        (src = dy, src2 = the pre-activation [rows][cols], ld2)
 * halo_cross_entropy_bwd_images: value = d loss / d logits as halo_cross_entropy_bwd writes it (same arguments), as images of
 *   [rows][V] and [V][rows] for the lm_head's two backward products (ha/attention.py:266-269); logits are left untouched. */
#define HALO_PAIR_COPY 0
#define HALO_PAIR_GELU_TANH 1
#define HALO_PAIR_GELU_ERF 2
#define HALO_PAIR_GELU_TANH_BWD 3
#define HALO_PAIR_GELU_ERF_BWD 4
int halo_image_pair(const float *src, const float *src2, int rows, int cols, long ld, long ld2, int op, void *image_rows,
                    void *image_cols, halo_stream_t stream);
int halo_cross_entropy_bwd_images(const float *logits, const int64_t *targets, const float *lse, const float *grad,
                                  long grad_stride, int rows, int V, long ld, long ignore_index, void *image_rows,
                                  void *image_cols, halo_stream_t stream);
/* halo_image_pairs: HALO_PAIR_COPY image pairs of n matrices (src[i] [rows[i]][cols[i]], row stride ld[i]) in ceil(n / 6) launches
 * instead of n: the weights of a transformer block, whose forward and input-gradient products read one image each
 * (ha/attention.py:117-129,141-143), are split once per optimizer step. */
int halo_image_pairs(int n, const float *const *src, const int *rows, const int *cols, const long *ld, void *const *image_rows,
                     void *const *image_cols, halo_stream_t stream);
int halo_gemm_split(const void *a_image, const void *b_image, int M, int N, int K, float *C, int ldc,
                    const float *bias1, const float *bias2, int flags, float p_drop, uint64_t seed,
                    uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);

/* halo_gemm_split with the addend of the residual connection read from its own buffer: C = epilogue(A B^T) + residual (row stride
 * ldr), C need not hold x beforehand -- x1 = x0 + c_proj(y) (ha/attention.py:178-179) without first copying x0 into the output. */
int halo_gemm_split_residual(const void *a_image, const void *b_image, int M, int N, int K, float *C, int ldc, const float *residual,
                             int ldr, const float *bias1, const float *bias2, int flags, float p_drop, uint64_t seed,
                             uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);

/* C [M][N] (+)= A^T B with A [K][M] (leading dimension lda) and B [K][N] (ldb) ROW-MAJOR bf16, the contraction index as their row:
 * the weight gradient dW = dy^T x of a Linear (ha/attention.py's nn.Linear layers under autograd) straight from the row-major bf16
 * activations and output gradients the neighbouring launches wrote -- the operands are transposed on their way from LDS into the MFMA
 * (ds_read_b64_tr_b16), no transposed operand image is built.  Single-pass bf16 operands, fp32 accumulation; K % 32 == 0, M % 8 == 0,
 * N % 8 == 0, lda % 8 == 0, ldb % 8 == 0, 16-byte aligned operands.  flags: 0 or HALO_GEMM_ACCUM (C += result).  Split-K slices go
 * through the scratch lent by halo_set_scratch. */
int halo_gemm_tn_bf16(const void *a, long lda, const void *b, long ldb, int M, int N, int K, float *C, int ldc, int flags,
                      halo_stream_t stream);
/* n <= 4 such products over the SAME contraction length K in ONE launch, each on whole-K tiles (no K-slices, no scratch, no reduce
 * launches): the four weight gradients of a GPT block -- c_attn, attention c_proj, c_fc, MLP c_proj -- all contract over the B T token
 * rows and have 36 .. 144 output tiles each; together they fill the chip.  Arrays of n entries; flags: 0 or HALO_GEMM_ACCUM for all. */
int halo_gemm_tn_bf16_group(int n, const void *const *a, const long *lda, const void *const *b, const long *ldb, const int *M, const int *N, int K,
                            float *const *C, const int *ldc, int flags, halo_stream_t stream);

/* The same grouped weight-gradient products (C_i [M_i][N_i] = A_i^T B_i, A_i [K][M_i] and B_i [K][N_i] row-major bf16, fp32 results
 * overwritten; replaces: the autograd of a GPT block's Linear layers and of the tied lm_head, ha/attention.py:117-143,228-231) on 256-row
 * tiles of whole K -- 256 x 128 or 256 x 256, picked per group so that the tiles fill whole rounds of the CUs (csrc/gemm_tn_rows.hip:
 * LDS-DMA of whole operand rows, transposing LDS reads into the MFMA; twice the arithmetic per operand byte of the 128 x 128 tiles).
 * Single-pass bf16 arithmetic only (HALO_ENOTSUP otherwise); K % 32 == 0, M_i % 8 == 0, N_i % 8 == 0, lda / ldb % 8 == 0, ldc % 4 == 0,
 * 16-byte aligned operands and results; n <= 4. */
int halo_gemm_tn_rows_supported(int n, const int *M, const int *N, int K);
/* 1 where these tiles measured faster than halo_gemm_tn_bf16_group's (at least two rounds of 256 x 256 tiles over the CUs: the lm_head) */
int halo_gemm_tn_rows_preferred(int n, const int *M, const int *N, int K);
int halo_gemm_tn_rows_group(int n, const void *const *a, const long *lda, const void *const *b, const long *ldb, const int *M, const int *N, int K,
                            float *const *C, const long *ldc, halo_stream_t stream);

/* halo_gemm_split with row-major bf16 activations on either side, so that consecutive Linears hand their activations on without an
 * operand-image pass (ha/attention.py:136-143: c_fc -> gelu -> c_proj).  A comes either from an image (a_image) or from a row-major
 * bf16 matrix a_hi [M][lda] (and a_lo, its split remainder, in bf16x3 mode; K % 32 == 0, lda % 8 == 0, 16-byte aligned): the kernel's
 * LDS staging fetches each 16-byte chunk from where the swizzled image would hold it.  The result goes to fp32 C (may be NULL when
 * out_hi is given) and / or to row-major bf16 out_hi [M][ldo] = bf16(v) (and out_lo = bf16(v - out_hi) in bf16x3 mode).
 * flags: HALO_GEMM_RELU / GELU* / ACCUM (adds residual [M][ldr], or C itself when residual is NULL).  No dropout, no split-K.
 * Combinations built: image -> bf16 (with or without activation), bf16 -> fp32 (with or without ACCUM); others HALO_ENOTSUP.  */
int halo_gemm_split_io(const void *a_image, const void *a_hi, const void *a_lo, long lda, const void *b_image, int M, int N, int K, float *C,
                       int ldc, void *out_hi, void *out_lo, long ldo, const float *residual, int ldr, const float *bias1,
                       const float *bias2, int flags, halo_stream_t stream);

/* Round 5: softmax attention forward from ROW-MAJOR bf16 q / k / v (the c_attn product's bf16 result, heads packed inside a row: head h at
 * columns [64 h, 64 h + 64)), single-pass bf16 arithmetic, head_dim 64, causal or full, no key lengths, no dropout (csrc/attn_b16.hip: K / V
 * tiles straight from bf16 rows into the LDS images, two tiles in flight).  y (fp32) and y_bf16 are both optional outputs (at least one);
 * lse optional.  HALO_ENOTSUP outside bf16 mode / head_dim 64: the callers keep halo_attention_fwd_bf16.
 * replaces: F.scaled_dot_product_attention in MonitoredSelfAttention.forward (ha/attention.py:96-129) under the reference's autocast. */
int halo_attention_fwd_b16(const void *q, long q_row_stride, long q_batch_stride, const void *k, const void *v, long kv_row_stride,
                           long kv_batch_stride, float *y, long y_row_stride, long y_batch_stride, void *y_bf16, long yb_row_stride,
                           long yb_batch_stride, float *lse, int N, int heads, int head_dim, int Tq, int Tk, int causal, halo_stream_t stream);
/* ... and its backward: q / k / v, the forward's bf16 output y and the output gradient dy all as row-major bf16 rows (y and dy with one pair
 * of strides), lse from the forward; delta [N * heads * Tq] is scratch the first sweep writes (rowsum(dy * y)) and the second reads; dq / dk /
 * dv leave as row-major bf16 (one pair of strides), the operands of the c_attn Linear's two gradient products.  Same limits as the forward. */
int halo_attention_bwd_b16(const void *q, long q_row_stride, long q_batch_stride, const void *k, const void *v, long kv_row_stride,
                           long kv_batch_stride, const void *y_bf16, const void *dy_bf16, long y_row_stride, long y_batch_stride, const float *lse,
                           float *delta, void *dq_bf16, void *dk_bf16, void *dv_bf16, long d_row_stride, long d_batch_stride, int N, int heads,
                           int head_dim, int Tq, int Tk, int causal, halo_stream_t stream);

/* Round 5: the activation-by-weight products of the GPT path on 256-row x 96 / 192 / 288-column workgroup tiles (csrc/gemm_rows.h), single-pass
 * bf16 arithmetic only (HALO_ENOTSUP in the other modes; halo_gemm_rows_supported says so up front).  C [M][N] = A [M][K] x B [N][K]^T with
 * A either a tiled image (a_image) or ROW-MAJOR bf16 a_bf16 [M][lda] (lda % 8 == 0), B a tiled image (halo_split_image of the weight, or
 * of its transpose for an input gradient), K % 32 == 0, N % 8 == 0, and exactly one result: fp32 C [M][ldc] (+ residual [M][ldr] when
 * given: x1 = x0 + c_proj(y), ha/attention.py:178-179, no copy of x0 first), or row-major bf16 out_bf16 [M][ldo] (what the next launch's
 * operand staging, the GELU passes and the attention kernels read).  The tile width is chosen per shape so that the tiles fill whole
 * rounds of the device's CUs: N = 768 -> 96 columns, 2304 -> 288, 3072 -> 192 at M = 8192.
 * replaces: F.linear in nn.Linear.forward of c_attn / c_proj / c_fc (ha/attention.py:96-144) and its input-gradient matmul under autograd. */
int halo_gemm_rows_supported(int M, int N, int K);
int halo_gemm_rows(const void *a_image, const void *a_bf16, long lda, const void *b_image, int M, int N, int K, float *C, long ldc,
                   const float *residual, long ldr, void *out_bf16, long ldo, halo_stream_t stream);
/* ... with new_gelu / F.gelu in the epilogue (exact: 0 tanh form ha/attention.py:12-17, 1 erf form): out_bf16 = gelu(bf16(A B^T)), and, when
 * pre_bf16 is given, pre_bf16 = bf16(A B^T) as well (the pre-activation a training step keeps for the backward) -- bit for bit what
 * halo_gemm_rows (bf16 result) followed by halo_gelu_b16 writes, without the pass over the [M][N] rows between them.
 * replaces: self.c_fc + new_gelu in MLP.forward (ha/attention.py:136-140). */
int halo_gemm_rows_gelu(const void *a_image, const void *a_bf16, long lda, const void *b_image, int M, int N, int K, void *out_bf16,
                        void *pre_bf16, long ldo, int exact, halo_stream_t stream);
/* ... and the lm_head product with the cross-entropy statistics in its epilogue (as halo_gemm_split_ce: loss[m] = logsumexp(logits[m, :]) -
 * logits[m, targets[m]], 0 on ignored rows; lse optional) and the logits kept as ROW-MAJOR bf16 logits_bf16 [M][ldo] (NULL: scoring,
 * nothing of size M x N is written) -- the reference's autocast lm_head output, ha/attention.py:228-231.  The statistics and the target's
 * logit are taken from the fp32 accumulators, so the loss does not see the rounding of the stored logits.
 * halo_cross_entropy_bwd_bf16 then turns the stored logits IN PLACE into (softmax - onehot(target)) * grad[m * grad_stride] (0 on
 * ignored rows; V % 8 == 0): the row-major bf16 operand of the lm_head's two gradient products (halo_gemm_tn_bf16, halo_gemm_rows).
 * replaces: F.cross_entropy(lm_head(x), targets, ignore_index=0) and its backward to the logits. */
size_t halo_gemm_rows_ce_workspace_bytes(int M, int N);
int halo_gemm_rows_ce(const void *a_image, const void *a_bf16, long lda, const void *b_image, int M, int N, int K, const int64_t *targets,
                      long ignore_index, void *workspace, float *loss, float *lse, void *logits_bf16, long ldo, halo_stream_t stream);
int halo_cross_entropy_bwd_bf16(void *logits_bf16, const int64_t *targets, const float *lse, const float *grad, long grad_stride, int rows,
                                int V, long ld, long ignore_index, halo_stream_t stream);

/* LoRA adapters of the c_attn Linear on the row-major bf16 rows of the GPT `bf16` path (csrc/lora.hip), rank r <= 16 padded to 16 so that
 * one 16x16x32 bf16 MFMA spans it, fp32 accumulation.  With h = ln_1(x) [M][C], A [r][C], B [3C][r], s = lora_alpha / r and m the dropout
 * mask of the adapter's input:  u = (m*h) A^T,  qkv += s u B^T;  du = s dqkv B,  dB = s dqkv^T u,  dA = du^T (m*h),  d_ln1 += m * (du A).
 *   halo_lora_pack   A, B (fp32) -> the four padded bf16 operands in one buffer of halo_lora_pack_bytes(n_in, n_out):
 *                    A16 [16][n_in] | At16 [n_in][16] | B16 [n_out][16] | Bt16 [16][n_out]
 *   halo_lora_down   U [M][16] = scale * (mask * X [M][K]) P [16][K]^T, bf16 out (M % 16 == 0, K % 32 == 0, ldx % 8 == 0)
 *   halo_lora_up     Y [M][N] += scale * mask * (U [M][16] P [N][16]^T) onto bf16 rows (y_bf16) or fp32 rows (y_f32), exactly one (N % 32 == 0)
 *   halo_lora_tn     G = scale * U [M][16]^T (mask * X [M][K]): rows 0 .. r-1 as fp32 g [r][K], or [K][r] with transpose_out; M is cut into
 *                    slabs whose partial tiles go to workspace (halo_lora_tn_workspace_bytes(M, K)) and are summed in a fixed order (no
 *                    atomics: two runs give the same bits).  M % 32 == 0, K % 16 == 0.
 * The mask is recomputed inside each kernel from the dropout stream (above) at the flat index row * K + col (row * N + col for
 * halo_lora_up), i.e. what halo_dropout_fwd draws for the [M][K] rows; p_drop == 0: no mask.  The row width of that index is K (N), not the
 * leading dimension: X (Y) is taken to be the whole [M][K] matrix the mask belongs to, also when ldx (ldy) is larger.
 * replaces: lora_B(lora_A(lora_dropout(x))) * scaling in Linear.forward (ha/lora.py:84-91) and its autograd backward. */
int halo_lora_supported(int M, int n_in, int n_out, int r);
size_t halo_lora_pack_bytes(int n_in, int n_out);
int halo_lora_pack(const float *A, const float *B, int r, int n_in, int n_out, void *packed, halo_stream_t stream);
int halo_lora_down(const void *x_bf16, long ldx, const void *p16, int M, int K, float scale, void *u_bf16, float p_drop, uint64_t seed,
                   uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
int halo_lora_up(const void *u_bf16, const void *p16, int M, int N, float scale, void *y_bf16, float *y_f32, long ldy, float p_drop,
                 uint64_t seed, uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
size_t halo_lora_tn_workspace_bytes(int M, int K);
int halo_lora_tn(const void *u_bf16, const void *x_bf16, long ldx, int M, int K, int r, float scale, int transpose_out, float *g,
                 void *workspace, float p_drop, uint64_t seed, uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev,
                 halo_stream_t stream);

/* lm_head + cross-entropy without materialising the logits (ha/attention.py:228-231): the split GEMM
 * logits[M,N] = A B^T (+ bias[N]) whose epilogue reduces each 64-column strip of a row to (max, sum exp) and picks out the
 * target's logit; a second small kernel merges the strips into loss[m] = logsumexp(logits[m,:]) - logits[m, targets[m]]
 * (0 where targets[m] == ignore_index) and, when lse != NULL, the row log-sum-exp for the backward.  logits may be NULL
 * (scoring: nothing of size M x N is written) or a [M, ldc] buffer that also receives them (training keeps them for
 * halo_cross_entropy_bwd_images).  workspace: halo_gemm_split_ce_workspace_bytes(M, N).  Split modes only (HALO_EINVAL in f32). */
size_t halo_gemm_split_ce_workspace_bytes(int M, int N);
int halo_gemm_split_ce(const void *a_image, const void *b_image, int M, int N, int K, float *logits, int ldc, const float *bias,
                       const int64_t *targets, long ignore_index, void *workspace, float *loss, float *lse, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conv1d stride-s subsample + relu + dropout.   replaces: ha/rnn.py:22-24
 *   x [B,T,F] (N,T,C contiguous, as the caller holds it before .mT), w [C,F,ks], bias [C]
 *   y [T',B,C] TIME-MAJOR, T' = floor((T + 2*pad - ks)/stride) + 1
 *   col: workspace [T'*B, F*ks] floats (im2col image, also the saved input for backward)
 * ------------------------------------------------------------------------------------------ */
size_t halo_subsample_col_bytes(int B, int T, int F, int ks, int stride, int pad);
int halo_subsample_fwd(const float *x, const float *w, const float *bias, float *y, float *col, int B,
                       int T, int F, int C, int ks, int stride, int pad, float p_drop, uint64_t seed,
                       uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
/* dy [T',B,C] is the gradient w.r.t. y; y is the forward output (relu/dropout mask is read off it);
 * dpre: workspace [T'*B, C]; dw [C,F,ks], dbias [C] are overwritten.  Input gradient is not
 * produced (mel features are leaves without grad in ha/loop.py:116). */
int halo_subsample_bwd(const float *dy, const float *y, const float *col, float *dpre, float *dw,
                       float *dbias, int B, int T, int F, int C, int ks, int stride, int pad, float p_drop,
                       halo_stream_t stream);
/* The same with dy handed over as `slabs` K-slices of the product that formed it -- [slabs][T'*B][C] floats, dy = their sum in order --
 * which the kernel adds while it reads them (halo_set_lstm_dx_slabs below: the LSTM backward's input-gradient product then runs without
 * its split-K reduce launch).  slabs = 1 is halo_subsample_bwd.  The unfused fallback sums the slices into slice 0 first. */
int halo_subsample_bwd_slabs(float *dy, int slabs, const float *y, const float *col, float *dpre, float *dw,
                             float *dbias, int B, int T, int F, int C, int ks, int stride, int pad, float p_drop,
                             halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-layer LSTM, gate order i,f,g,o, two bias vectors per layer.
 * replaces: nn.LSTM forward/backward (cuDNN RNN / oneDNN) at ha/rnn.py:25 (batch_first encoder)
 * and ha/rnn.py:50,63 (time-major Decoder with carried state).
 *   x [T,B,in0] time-major.  w_ih[l] [4H,in_l], w_hh[l] [4H,H], b_ih[l], b_hh[l] [4H]: HOST arrays
 *   of L device pointers.  h0/c0 [L,B,H] or NULL (zeros).  hn/cn [L,B,H] or NULL.
 *   y: last layer's output h_t written at y + t*y_stride_t + b*y_stride_b + j (so the caller picks
 *   batch-first or time-major); relu applied when y_relu (the encoder's x.relu(), rnn.py:26).
 *   Inter-layer dropout p_drop (train only) uses stream HALO_STREAM_LSTM_LAYER0 + l on the
 *   time-major [T,B,H] index.
 *   reserve: halo_lstm_reserve_bytes(); holds per layer h[T+1,B,H], c[T+1,B,H], gates[T,B,4H],
 *   dropped output [T,B,H]; consumed (overwritten with gate gradients) by halo_lstm_bwd.
 * ------------------------------------------------------------------------------------------ */
size_t halo_lstm_reserve_bytes(int T, int B, int in0, int H, int L);
size_t halo_lstm_bwd_workspace_bytes(int T, int B, int in0, int H, int L);
int halo_lstm_fwd(const float *x, const float *const *w_ih, const float *const *w_hh,
                  const float *const *b_ih, const float *const *b_hh, const float *h0, const float *c0,
                  float *y, long y_stride_t, long y_stride_b, int y_relu, float *hn, float *cn,
                  float *reserve, int T, int B, int in0, int H, int L, float p_drop, uint64_t seed,
                  uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
/* dy has the strides of y; dhn/dcn [L,B,H] or NULL.  dx [T,B,in0] or NULL.
 * dw_ih/dw_hh/db_ih/db_hh: HOST arrays of L device pointers, overwritten.
 * Layers [layer_begin, layer_end) are processed, top down.  A whole backward is (0, L); a caller
 * that wants the upper layers' gradients early (to start their all-reduce) calls (k, L) and later
 * (0, k) with the SAME workspace, which carries the gradient between the two calls. */
int halo_lstm_bwd(const float *x, const float *const *w_ih, const float *const *w_hh, const float *dy,
                  long y_stride_t, long y_stride_b, int y_relu, const float *dhn, const float *dcn,
                  float *reserve, float *workspace, float *dx, float *const *dw_ih, float *const *dw_hh,
                  float *const *db_ih, float *const *db_hh, int T, int B, int in0, int H, int L,
                  int layer_begin, int layer_end, float p_drop, uint64_t seed, uint32_t offset,
                  const uint32_t *offset_dev, halo_stream_t stream);

/* Contexts.  Every halo_set_* switch (arithmetic mode, scratch, LSTM schedule switches, measurement hooks, the status word, the beam
 * search's reference ISA) lives in a settings record.  There is one process-wide default record; halo_ctx_create() makes a caller-owned
 * copy of the calling thread's current record, and halo_ctx_use(ctx) makes it the record that THIS thread's later halo_* calls read and
 * halo_set_* calls write (NULL: back to the default).  Two trainers, or a trainer and a recognizer, on different threads therefore do
 * not see each other's switches; within one thread, select the context before a group of calls.  Work launched on distinct streams from
 * distinct threads with distinct contexts (and distinct scratch buffers) is independent; calls that share one record, or the default
 * one, must be serialised by the caller. */
typedef struct halo_ctx halo_ctx;
halo_ctx *halo_ctx_create(void);
void halo_ctx_destroy(halo_ctx *ctx);
int halo_ctx_use(halo_ctx *ctx);
/* A caller-owned device uint32 that the persistent recurrences (csrc/lstm_persist*.hip) set to 1 when one of their bounded waits times
 * out (co-residency lost: a CU mask, another tenant, a profiler).  It is sticky -- the library only ever sets it -- and
 * halo_clip_coef_step treats a raised word like a non-finite gradient norm (no update is applied).  NULL (default): no word. */
int halo_set_status_word(uint32_t *device_word);
/* Test hook: the workgroup with this blockIdx of every persistent LSTM forward launched afterwards never publishes its epoch, so its
 * peers run into their bounded waits (0.2 s), raise the abort and status words and leave; -1 (default): none. */
int halo_debug_mute_workgroup(int block);
/* Diagnostic: `blocks` workgroups of 4 waves run `iters` rounds of a bare bf16 MFMA loop on random register operands (shape 0: four
 * 32x32x16 per round and wave, 1: eight 16x16x32 -- 131072 FLOP per wave and round either way) and report per workgroup
 * ticks[2 b] = shader clocks (s_memtime), ticks[2 b + 1] = 100 MHz ticks (s_memrealtime): the clock the chip holds under matrix load
 * (tools/mfma_clock.py).  sink: one float of device memory, never written in practice. */
int halo_debug_mfma_clock(unsigned long long *ticks, float *sink, int blocks, int iters, int shape, unsigned seed, halo_stream_t stream);

/* Weight-resident persistent recurrence (csrc/lstm_persist.hip): when the shape is eligible (split-bf16 arithmetic modes,
 * H in {256, 512, 768, 1024}, (H/16) * ceil(B/16) <= number of CUs) a layer's T dependent step launches become ONE launch
 * whose workgroups keep their W_hh slice in registers and hand h_t (forward) / the gate gradients (backward) to each other
 * through write-through stores and per-workgroup epoch words.  On by default; halo_set_lstm_persistent(0) selects the
 * per-step launch chain (also HALO_LSTM_PERSIST=0 in the environment).  The kernel needs every workgroup resident at once, so
 * nothing else should occupy the GPU's CUs for long while it runs; all its waits are bounded (0.2 s): on a timeout the u32 at
 * byte offset halo_lstm_status_offset() of the reserve (backward != 0: of the backward workspace) is set to 1 and the results
 * of that call are invalid.  It reads 0 after a good call. */
int halo_set_lstm_persistent(int on);
/* The persistent backward writes the gate gradients' split-bf16 GEMM operand images itself (B % 32 == 0, split-bf16 and bf16 modes) instead of
 * leaving them to the operand-image launch behind it (bf16 mode: the hi parts only): same bits, one 4H-wide fp32 re-read less per layer.  On by default
 * (HALO_PERSIST_EMIT=0 / halo_set_lstm_persistent_images(0): off). */
int halo_set_lstm_persistent_images(int on);
int halo_lstm_persistent_eligible(int B, int H);
/* Two-layer persistent recurrence (csrc/lstm_persist2.hip): for L >= 2 in the single-pass bf16 arithmetic mode (HALO_MATH_BF16) and a
 * shape the persistent recurrence takes, halo_lstm_fwd runs the stack's TOP TWO layers' T steps in one launch of T + 2 combined steps
 * (the lower layer at time s beside the upper at time s - 2: one hand-off per combined step, the upper layer's input projection inside
 * its step; the layers below them one launch each), and halo_lstm_bwd called with layer_end = L and layer_begin <= L - 2 likewise (the
 * upper layer's input gradient formed inside the launch).  Same reserve contents as the per-layer path, so either backward follows
 * either forward.  Any batch: the batch rows are independent chains, so more 16-row tiles than the chip has CUs for (H/16 workgroups per
 * tile) run as consecutive launches over the same buffers.  On by default (HALO_LSTM_PERSIST2=0 / halo_set_lstm_persistent2(0): off). */
int halo_set_lstm_persistent2(int on);
/* Two batch tiles per workgroup in the two-layer launches (csrc/lstm_persist2x.hip): a batch of more 16-row tiles than one launch holds
 * workgroups for (more than 64 rows at H = 1024) runs two tiles in each workgroup, interleaved -- while one tile's hand-off is in flight
 * the workgroup computes the other tile's step on the same register-resident weights -- instead of as consecutive launches.  Same
 * buffers, images and results as those launches but for the order in which the two tiles' bias-gradient rows are added.  On by
 * default (HALO_LSTM_INTERLEAVE=0 / halo_set_lstm_interleave(0): consecutive launches).  Per context. */
int halo_set_lstm_interleave(int on);
/* The two-layer launches' weight-gradient products on 256 x 256 workgroup tiles (csrc/gemm256.h): in single-pass `bf16` arithmetic both
 * layers' dW_hh | dW_ih and the K-slices of the caller's input gradient run as ONE launch of one workgroup per CU instead of two launches
 * of the 128 x 128-tile kernel.  Same operand images, same sums up to the order of the k-blocks' additions inside a tile.  On by default
 * (HALO_GEMM256=0 / halo_set_gemm256(0): the 128 x 128-tile launches).  Process-wide. */
int halo_set_gemm256(int on);
/* Data-parallel overlap hook.  event (a hipEvent_t, or NULL: off): halo_lstm_bwd records it on its stream right behind the launch that
 * stores the TOP layer's weight gradients (dw_ih[L-1], dw_hh[L-1]) when the call covers the top two layers as one two-layer launch --
 * the point from which a caller's side stream may start reducing those gradients over the ranks (ha/attention_loop.py:154:
 * DistributedDataParallel overlaps its buckets with backward) while the lower layer's products and the front end's backward still run.
 * Not recorded by any other path: halo_lstm_bwd_mid_event_recorded() tells (the caller then waits for the whole call).  Not for use inside a stream capture.  Per context. */
int halo_set_lstm_bwd_mid_event(void *event);
int halo_lstm_bwd_mid_event_recorded(void);     /* how many times the event has been recorded since it was set (0: this path has no such point) */
/* Inference with static weights.  stamp != 0 is the caller's promise that the LSTM weights change only when the stamp does: a forward-only
 * call (halo_set_lstm_expect_backward(0)) of the two-layer launch then KEEPS the packed weight images that the previous call with the same
 * reserve buffer, weight pointers, shape and stamp left in that reserve (24 MB read + 12 MB written per call at H = 1024 otherwise), so the
 * caller must own the reserve between the calls.  0 (default): every call packs.  Per context. */
int halo_set_lstm_weights_stamp(uint64_t stamp);
/* The two-layer forward packs its three weight images; when a backward of the same step will follow (the default) it writes the
 * backward's three transposed images from the same read of the weights, into the reserve, and halo_lstm_bwd called with that reserve
 * and those weight pointers packs nothing.  Inference callers switch it off (0): the forward then packs its own three only. */
int halo_set_lstm_expect_backward(int on);
/* The transposed images hold the forward images' bf16 values, permuted.  On (the default): that packing launch leaves them unwritten (a
 * fifth fewer bytes) and the two-layer backward launch builds its W^T fragments from the forward images instead, transposing 16 x 16 tiles
 * through LDS ahead of its first step.  Same fragments, same results.  Not for the interleaved launches (halo_set_lstm_interleave), which
 * keep their images.  HALO_LSTM_BWD_FROM_FWD=0 / halo_set_lstm_bwd_from_fwd_images(0): six images, as before.  Process-wide. */
int halo_set_lstm_bwd_from_fwd_images(int on);
/* n > 1: the caller's dx buffer of the NEXT halo_lstm_bwd calls has room for n matrices [T*B][in0] and its consumer can add K-slices
 * (halo_subsample_bwd_slabs): the two-layer launch's input-gradient product (layer_begin = 0) may then leave up to n unreduced slices there
 * instead of running a reduce launch.  halo_lstm_dx_slabs_left() after the call says how many it left (1: dx is the gradient itself, as
 * always on every other path).  1 <= n <= 64; default 1.  Per context. */
int halo_set_lstm_dx_slabs(int n);
int halo_lstm_dx_slabs_left(void);
/* Small reductions that ride in another launch.  on = 1: halo_ctc_head_bwd's second launch (the fixed-order sum of its per-utterance
 * partials) and the two-layer halo_lstm_bwd's bias-gradient sums are QUEUED on the context (at most 4; a full queue launches as before)
 * instead of launched, and the next halo_subsample_bwd[_slabs] runs them from the tail blocks of its reduce launch -- same arithmetic and
 * order, one ~5 us launch each less.  halo_flush_small_jobs launches whatever is queued (nothing: no launch).  The caller keeps the
 * workspaces those reductions read alive until then, calls everything on one stream, and reads the results (dweight / dbias, db_ih /
 * db_hh) only after the carrying launch.  Switching on clears the queue.  Default 0.  Per context. */
int halo_set_defer_small_jobs(int on);
int halo_flush_small_jobs(halo_stream_t stream);
/* The squared gradient norm without a pass over the gradients.  partials != NULL: the launches of the NEXT backward calls that store
 * clipped gradients also write the sums of their squares, one float per workgroup, into partials[0 .. count) -- the two-layer
 * halo_lstm_bwd's two weight-gradient launches (from the accumulators they store), its bias sums (when deferred: small jobs above), and
 * halo_subsample_bwd[_slabs]'s reduce launch.  halo_grad_sumsq_state reports how many slots were written and which producers
 * contributed: bit 0 / 1 the upper / lower layer's W_ih + W_hh, bit 2 / 3 their b_ih + b_hh, bit 4 the conv's weight + bias.  A caller whose
 * clipped parameters are exactly those (a 2-layer stack behind the conv front end) passes the partials to halo_clip_coef[_step] with that
 * count when all five bits are set, and runs halo_sumsq otherwise.  capacity: floats available (a producer without room does not
 * contribute).  NULL: off (default).  Setting it (to anything) resets count and bits.  Host bookkeeping, per context. */
int halo_set_grad_sumsq(float *partials, int capacity);
int halo_grad_sumsq_state(int *count, unsigned *covered);
int halo_lstm_persistent2_eligible(int T, int B, int H, int L);
size_t halo_lstm_status_offset(int backward, int T, int B, int in0, int H, int L);

/* ------------------------------------------------------------------------------------------
 * Per-utterance squared gradient norms from one backward pass (csrc/ghost_norm.hip).   replaces: ha/grad_norm.py
 * A term describes one group of parameters whose gradient for utterance n is sum_t a_t b_t^T (plus n_bias bias vectors with gradient
 * sum_t a_t); the kernel evaluates
 *     sq[term][n] = sum_{t,t' < T} <a_t, a_t'> * (n_bias + sum_j <b^j_t, b^j_t'>)
 * from the operands where they lie: element (n, t, k) of an operand is ptr[n * stride_n + t * stride_t + k] (strides in floats, unit
 * element stride, any K >= 1, any T >= 1; 16-byte loads where ptr and both strides allow them).  n_b in {0, 1, 2} operands b,
 * n_bias in {0, 1, 2}.  Exact-f32 MFMA in every arithmetic mode.  Two launches: one workgroup per (term, n, pair of
 * halo_ghost_tile()-frame tiles) writes one partial into workspace (halo_ghost_sqnorm_workspace_bytes), the second adds them in a
 * fixed order into sq [n_terms][N] (optional) and writes norm[n] = sqrt(sum over terms) (optional; one of the two must be given).
 * No atomics: the same inputs give the same bits.  HALO_ENOTSUP: N > 65535.
 * ------------------------------------------------------------------------------------------ */
typedef struct halo_ghost_operand {
    const float *ptr;
    long stride_n, stride_t;
    int K;
} halo_ghost_operand;
typedef struct halo_ghost_term {
    halo_ghost_operand a;
    halo_ghost_operand b[2];
    int n_b, n_bias;
} halo_ghost_term;
int halo_ghost_tile(void);
size_t halo_ghost_sqnorm_workspace_bytes(int n_terms, int N, int T);
int halo_ghost_sqnorm(const halo_ghost_term *terms, int n_terms, int N, int T, float *workspace, float *sq, float *norm,
                      halo_stream_t stream);
/* on = 1: the persistent backward launches of the NEXT halo_lstm_bwd calls store their fp32 gate gradients back into the reserve's gates
 * buffers even where they emit the GEMM operand images themselves (what HALO_LSTM_KEEP_DG=1 does process-wide).  Default 0.  Per context. */
int halo_set_lstm_keep_gate_gradients(int on);
int halo_get_lstm_keep_gate_gradients(void);
/* The LSTM's terms for halo_ghost_sqnorm, one per layer, read off the reserve that a halo_lstm_fwd + a whole halo_lstm_bwd (layers 0 .. L,
 * keep flag above set) of the same x / shape / p_drop have gone through: a = the layer's gate gradients [T][B][4H], b0 = the layer's input
 * (x for layer 0, the dropped output of the layer below otherwise), b1 = h_{t-1}, n_bias = 2 (b_ih, b_hh); all time-major.
 * terms_out: L records.  HALO_ENOTSUP when the last backward on this context did not leave complete gate gradients in this reserve
 * (keep flag off, a partial layer range, the layer-diagonal fused schedule, or another forward since). */
int halo_lstm_ghost_terms(const float *x, float *reserve, int T, int B, int in0, int H, int L, float p_drop, halo_ghost_term *terms_out);
/* dpre = dy * (y > 0 ? 1 / (1 - p_drop) : 0): the gradient at the pre-activation of relu followed by inverted dropout, the mask read
 * off the forward output y (what halo_subsample_bwd forms inside its product and need not store).  n floats each. */
int halo_relu_dropout_bwd(const float *dy, const float *y, float *dpre, size_t n, float p_drop, halo_stream_t stream);

/* Diagnostic: device buffer of uint64 [blocks][T][16] that the persistent forward fills with 100 MHz time stamps of its phases
 * (tools/persist_stamps.py reads them); NULL (default) turns the stamps off. */
int halo_lstm_persist_stamps(void *device_buffer);

/* Measurement hook (bench.py): while set, every layer's recurrent chain inside halo_lstm_fwd / halo_lstm_bwd is bracketed by
 * hipEventRecord(ev_begin) / hipEventRecord(ev_end) on the call's stream (hipEvent_t handles; NULL, NULL clears).  The
 * batched GEMMs and operand preparation of the same call stay outside the bracket.  Not for use under stream capture.
 * halo_lstm_chain_info: how the last forward (backward != 0: backward) chain ran: number of kernel launches
 * (1 = the persistent weight-resident kernel, T = one launch per time step) and the kernel's name. */
int halo_lstm_chain_events(void *ev_begin, void *ev_end);
int halo_lstm_chain_info(int backward, int *launches, char *kernel, int kernel_len);

/* ------------------------------------------------------------------------------------------
 * Row-wise log-softmax.   replaces: features.log_softmax(dim=-1) ha/recognizer.py:46
 * ------------------------------------------------------------------------------------------ */
int halo_log_softmax_fwd(const float *x, float *y, int rows, int cols, halo_stream_t stream);
int halo_log_softmax_bwd(const float *dy, const float *y, float *dx, int rows, int cols,
                         halo_stream_t stream);
/* column sums: out[n] = sum_m x[m*ld + n]  (bias gradients) */
int halo_colsum(const float *x, int rows, int cols, int ld, float *out, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CTC lattice, blank = 0, one workgroup per utterance.
 * replaces: F.ctc_loss (ATen ctc_loss_gpu alpha/beta kernels) at ha/recognizer.py:71 and the
 * pure-torch recursion ha/ctc.py:110-174 (ctc_forward_score3), ctc.py:4-107 (score1/score2).
 *   lp: log-probabilities, element (t,n,c) at lp + t*stride_t + n*stride_n + c
 *   targets [N,S] int64 (row stride tg_stride), input_lengths/target_lengths [N] int64
 *   alpha [N,T,2S+1] out;  nll [N] out (positive negative-log-likelihood)
 *   flags:
 *     HALO_CTC_FULL_LATTICE  run all T frames over all 2S+1 states and read out at
 *                            (il-1, 2*tl), (il-1, 2*tl-1) like ctc.py:131-174; otherwise restrict
 *                            to the utterance's own lengths like F.ctc_loss.
 *     HALO_CTC_FINITE_MIN    "log 0" is -FLT_MAX (ctc.py:135) instead of -inf
 *     HALO_CTC_NO_LEAD_BLANK_LOOP  state 0 is never updated after t=0 (ctc.py:26, :103)
 *     HALO_CTC_WRAP_SKIP     state 1 also receives alpha[t-1, last] (python index -1, ctc.py:29)
 * ------------------------------------------------------------------------------------------ */
#define HALO_CTC_FULL_LATTICE 1
#define HALO_CTC_FINITE_MIN 2
#define HALO_CTC_NO_LEAD_BLANK_LOOP 4
#define HALO_CTC_WRAP_SKIP 8
int halo_ctc_fwd(const float *lp, long stride_t, long stride_n, int T, int N, int C,
                 const int64_t *targets, long tg_stride, int S, const int64_t *input_lengths,
                 const int64_t *target_lengths, int flags, float *alpha, float *nll,
                 halo_stream_t stream);
/* Gradient in F.ctc_loss's convention (ATen ctc_loss_backward): for t < il
 *   grad(t,n,c) = grad_out[n] * (exp(lp) - exp(logsum_{s: l'_s=c}(alpha+beta) + nll - lp)), else 0.
 * beta: workspace [N,T,2S+1].  grad has lp's strides (gstride_t, gstride_n). */
int halo_ctc_bwd(const float *lp, long stride_t, long stride_n, int T, int N, int C,
                 const int64_t *targets, long tg_stride, int S, const int64_t *input_lengths,
                 const int64_t *target_lengths, const float *alpha, const float *nll,
                 const float *grad_out, float *beta, float *grad, long gstride_t, long gstride_n,
                 halo_stream_t stream);

/* Two scalar-glue launches of the training step (ha/rnn.py:13-18, ha/recognizer.py:71 reduction='mean'):
 *   halo_ctc_prepare: feature_lengths[n] = floor((il[n] + 2*pad - ks)/stride + 1) computed in float like
 *     the reference, grad_out[n] = 1 / (max(tl[n],1) * N) = d(mean loss)/d(nll[n]);
 *   halo_ctc_mean_loss: *loss = mean_n(nll[n] / max(tl[n],1)), fixed summation order. */
int halo_ctc_prepare(const int64_t *input_lengths, const int64_t *target_lengths, int n, int ks, int stride,
                     int pad, int64_t *feature_lengths, float *grad_out, halo_stream_t stream);
int halo_ctc_mean_loss(const float *nll, const int64_t *target_lengths, int n, float *loss,
                       halo_stream_t stream);

/* TemporalClassifier.decode (ha/recognizer.py:48-59) in ONE launch, one workgroup per utterance: Linear -> log_softmax -> per frame the
 * best class and its log-prob (alignments, scores [B][T]) -> unique_consecutive, blanks dropped (hyp [B][T] zero padded, hyp_len [B]);
 * lp (optional) receives the log-probs [B][T][V].  Same shape limits as halo_ctc_head_fwd (T <= 32, V <= 32). */
int halo_ctc_head_greedy(const float *features, const float *weight, const float *bias, float *lp, int64_t *alignments, float *scores,
                         int64_t *hyp, int64_t *hyp_len, int B, int T, int H, int V, halo_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * The whole CTC head of a training step (TemporalClassifier.forward and its backward) in three launches.
 * replaces: dropout -> nn.Linear -> log_softmax -> F.ctc_loss(mean) ha/recognizer.py:43-46,61-73 plus the feature-length arithmetic of
 *           ha/rnn.py:13-18, i.e. halo_dropout_fwd + halo_gemm_f32 + halo_log_softmax_fwd + halo_ctc_prepare + halo_ctc_fwd +
 *           halo_ctc_mean_loss, and in the backward halo_ctc_bwd + halo_log_softmax_bwd + 2 x halo_gemm_f32 + halo_colsum.
 * Fast path for T <= 32 frames, V <= 32 classes, 2S+1 <= 64 lattice states, H % 64 == 0 (halo_ctc_head_supported; otherwise
 * HALO_ENOTSUP and the caller uses the separate operators).  One workgroup per utterance, products on the exact-f32 MFMA.
 *   features [B,T,H] (the encoder's output), weight [V,H], bias [V]; the classifier dropout (p_drop, stream_id) is applied to the
 *   features as halo_dropout_fwd would (flat index of [B,T,H]) and again, from the same stream, to d features in the backward.
 *   input_lengths: frames BEFORE the subsample conv (ks, stride, pad); feature_lengths [B] int64 out.
 *   lp [B,T,V], alpha [B,T,2S+1], nll [B], grad_out [B] (= 1 / (max(tl,1) * B)), loss (scalar: reduction='mean') out;
 *   ticket: device uint32, 0 before the first call (the kernel leaves it 0).
 *   backward: dfeatures [B,T,H], dweight [V,H], dbias [V] out; workspace halo_ctc_head_workspace_bytes(). */
int halo_ctc_head_supported(int T, int H, int V, int S);
size_t halo_ctc_head_workspace_bytes(int B, int H, int V);
int halo_ctc_head_fwd(const float *features, const float *weight, const float *bias, float p_drop, uint64_t seed,
                      uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, const int64_t *input_lengths, int ks,
                      int stride, int pad, const int64_t *targets, long tg_stride, int S, const int64_t *target_lengths,
                      float *lp, float *alpha, float *nll, int64_t *feature_lengths, float *grad_out, float *loss,
                      uint32_t *ticket, int B, int T, int H, int V, halo_stream_t stream);
int halo_ctc_head_bwd(const float *features, const float *weight, float p_drop, uint64_t seed, uint32_t stream_id,
                      uint32_t offset, const uint32_t *offset_dev, const int64_t *feature_lengths, const int64_t *targets,
                      long tg_stride, int S, const int64_t *target_lengths, const float *lp, const float *alpha,
                      const float *nll, const float *grad_out, float *dfeatures, float *dweight, float *dbias,
                      void *workspace, int B, int T, int H, int V, halo_stream_t stream);

/* The same head, forward AND backward, in ONE launch -- for a caller that runs both every step (a training step: ha/loop.py:176-196
 * calls the loss and loss.backward() back to back).  replaces: halo_ctc_head_fwd + halo_ctc_head_bwd, i.e. ha/recognizer.py:43-46,61-73
 * and their autograd backward.  Same shape limits (halo_ctc_head_supported); products on split-bf16 MFMA (fp32-grade: the `bf16x3`
 * arithmetic), so HALO_ENOTSUP in the exact-f32 mode -- the caller then uses the two launches above.  grid = B x slices workgroups,
 * the slices of an utterance (H/slices feature columns each) exchanging their partial logits once; alpha and beta run side by side.
 *   lp [B,T,V]: optional (NULL: not written); nll [B], feature_lengths [B], loss out as halo_ctc_head_fwd;
 *   dfeatures [B,T,H], dweight [V,H], dbias [V] out as halo_ctc_head_bwd (the partials' sum may be deferred the same way);
 *   workspace: halo_ctc_head_train_workspace_bytes(); ticket: halo_ctc_head_train_ticket_words(B, H) device uint32 words (8-byte
 *   aligned), all 0 before the first call, the caller's to keep between calls: the loss ticket, the count of launches, and the
 *   slices' partial logits, each stored with that count as its tag.
 * A slice that never arrives (0.2 s) makes the loss NaN instead of hanging the launch. */
size_t halo_ctc_head_train_workspace_bytes(int B, int H, int V);
size_t halo_ctc_head_train_ticket_words(int B, int H);
int halo_ctc_head_train(const float *features, const float *weight, const float *bias, float p_drop, uint64_t seed,
                        uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, const int64_t *input_lengths, int ks,
                        int stride, int pad, const int64_t *targets, long tg_stride, int S, const int64_t *target_lengths,
                        float *lp, float *nll, int64_t *feature_lengths, float *loss, uint32_t *ticket, float *dfeatures,
                        float *dweight, float *dbias, void *workspace, int B, int T, int H, int V, halo_stream_t stream);

/* Greedy decode.   replaces: logits.max(-1) + unique_consecutive + drop-0 loop, recognizer.py:51-55
 *   lp [N,T,C] contiguous; alignments [N,T] int64, scores [N,T] f32, hyp [N,T] int64 (first
 *   hyp_len[n] entries valid), hyp_len [N] int64.  Input lengths are ignored, as in the reference. */
int halo_ctc_greedy(const float *lp, int N, int T, int C, int64_t *alignments, float *scores,
                    int64_t *hyp, int64_t *hyp_len, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streaming LSTM-CTC recognition (haloop_amd/streaming.py; the reference recognises whole utterances only): the two launches around
 * halo_lstm_fwd of one chunk of B streams.  Per-stream flags: bit 0 active, bit 1 begin, bit 2 final.  A stream that is not active is
 * left bit-identical by both launches.  fp32, no atomics, one workgroup per stream.
 *
 * halo_stream_front: the reference's subsample (kernel 5, stride 4, padding 3) over [carry | length[b] frames | zeros] with ReLU ->
 *   y [S,B,C] time-major (steps at or past n_steps[b], and every step of an inactive stream, are zeros);
 *   n_steps[b] = length/4, or floor((length + 1)/4) + 1 for a final stream (the right padding), 0 for an inactive one;
 *   carry [B,3,F] of an active stream that goes on <- its last 3 frames.  A beginning stream reads its carry as zeros (the left
 *   padding), and its rows of h / c [L,B,H], hyp [B,capacity], hyp_len, steps, score, last_label (-1) and truncated are reset.
 *   frames [B,Tc,F], weight [C,F,5], bias [C].  S <= 64.
 * halo_stream_head: per stream the first n_steps[b] steps of feats [B,S,H] -> Linear(H -> V) -> log_softmax -> first maximum per step
 *   (alignments, step_scores [B,S]; zeros past n_steps) -> the greedy collapse continued from last_label[b] (a label equal to the
 *   previous step's emits nothing, across calls too; blank = 0 emits nothing): tokens appended at hyp[b][hyp_len[b]] (row length
 *   `capacity`; a token that does not fit is dropped and sets truncated[b]), score[b] += the step scores in step order, steps[b] +=
 *   n_steps[b]; lp_out (optional) [B,S,V] receives the log-probs.  The rows of hn / cn [L,B,H] of active streams that are not final are
 *   copied into h / c.  The fused product needs halo_ctc_head_supported(S, H, V, 0) and a math mode other than HALO_MATH_F32
 *   (HALO_ENOTSUP otherwise).  Collapse-only mode: feats == NULL and lp_in [B,S,V] holds log-probs the caller computed (any V).
 * ------------------------------------------------------------------------------------------ */
int halo_stream_front(const float *frames, float *carry, const int *length, const int *flags, const float *weight, const float *bias,
                      float *y, int *n_steps, float *h, float *c, int64_t *hyp, int64_t *hyp_len, int64_t *steps, float *score,
                      int *last_label, unsigned char *truncated, int B, int Tc, int F, int C, int S, int L, int H, int capacity,
                      halo_stream_t stream);
int halo_stream_head(const float *feats, const float *weight, const float *bias, const float *lp_in, float *lp_out, const int *n_steps,
                     const int *flags, const float *hn, const float *cn, float *h, float *c, int64_t *alignments, float *step_scores,
                     int64_t *hyp, int64_t *hyp_len, int64_t *steps, float *score, int *last_label, unsigned char *truncated, int B,
                     int S, int H, int V, int L, int capacity, halo_stream_t stream);
/* halo_stream_logits: the head launch of a streamed transducer.  f [B,S,V] = Linear(H -> V) of the first n_steps[b]
 *   steps of feats [B,S,H], zeros past them (no softmax); steps[b] += n_steps[b]; the same commit of hn / cn into h / c as
 *   halo_stream_head.  The fused product has halo_stream_head's conditions (HALO_ENOTSUP otherwise).  Commit-only mode: feats == NULL and
 *   f holds the caller's product; only its steps past n_steps[b] are written. */
int halo_stream_logits(const float *feats, const float *weight, const float *bias, float *f, const int *n_steps, const int *flags,
                       const float *hn, const float *cn, float *h, float *c, int64_t *steps, int B, int S, int H, int V, int L,
                       halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 80-mel log filterbank front-end on the device (ha/data.py:136-140: torchaudio.compliance.kaldi.fbank(wav, num_mel_bins=80) with that
 * function's defaults; haloop_amd/fbank.py chains these with two halo_gemm_f32 products -- the real DFT and the mel filters).
 *   halo_fbank_frames  waveform [n_samples] -> frames [n_frames][padded]: frame f = samples [f*shift, f*shift + frame_len) (snip edges),
 *                      minus its mean (remove_dc), pre-emphasised x[i] - c*x[i-1] (x[0] - c*x[0]), times window[i], zero padded
 *   halo_fbank_power   spectrum [n_frames][2*bins] (real parts, then imaginary parts) -> power [n_frames][ld] (columns >= bins zero)
 *   halo_fbank_log     x = log(max(x, eps)) in place */
int halo_fbank_frames(const float *wav, long n_samples, int frame_len, int shift, int padded, float preemphasis, int remove_dc,
                      const float *window, float *frames, int n_frames, halo_stream_t stream);
int halo_fbank_power(const float *spectrum, int n_frames, int bins, float *power, int ld, halo_stream_t stream);
int halo_fbank_log(float *x, long n, float eps, halo_stream_t stream);
/* The rest of the front-end in ONE launch and in float64: the N-point real DFT of every frame against a table of the N twiddles
 * (twiddle[2 j] = cos(2 pi j / N), twiddle[2 j + 1] = sin(2 pi j / N), N = padded, a power of two <= 2048), |X|^2, the num_bins
 * triangular filters (banks [num_bins][N / 2 + 1], float64) and log(max(., eps)) -> out [n_frames][num_bins] float32.  Replaces
 * the two exact-f32 products + halo_fbank_power + halo_fbank_log where the log-mels must hold to 1e-4 far below a frame's peak. */
int halo_fbank_spectrum_mel(const float *frames, int n_frames, int padded, const double *twiddle, const double *banks, int num_bins,
                            float eps, float *out, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batched feature front-end.  replaces: the combinators fbank: / mfcc: / mask: of ha/data.py:103-151 (torchaudio.compliance.kaldi.fbank
 * and .mfcc with their defaults, utterance CMVN :148-150, mask_along_axis_iid twice :109-121), which the reference runs per utterance in
 * its DataLoader workers.  A ragged batch goes in, padded features and their lengths come out; every shape follows from N and the padded
 * width L, ``lengths`` (device int64 [N], clamped to [0, L]) is read on the device only, and no launch uses atomics.
 *   M   = 1 + (L - frame_len) / shift for L >= frame_len, else 0                     (the caller passes it; checked)
 *   m_n = 1 + (lengths[n] - frame_len) / shift for lengths[n] >= frame_len, else 0   (snip edges)
 *
 *   halo_features_batch  waveforms [N, L] fp32 (anything may stand past lengths[n]: such a sample is never read) -> out [N, M, D] fp32
 *                        and feature_lengths [N] int64 = m_n, ONE launch.  kind HALO_FEATURES_FBANK: D = num_bins log-mels;
 *                        HALO_FEATURES_MFCC: D = num_ceps.  Rows m >= m_n are exact zeros; every element of out is written.
 *                        Per frame: DC removal, pre-emphasis (the first sample against itself) and window in fp32 with the arithmetic
 *                        of halo_fbank_frames; a 512-point real FFT in float64 (frame_len, shift <= 512); the filters; (float)
 *                        log(max(., eps)); for MFCC the product with dct on those fp32 log-mels, in float64.  Tables (device):
 *                          window   [frame_len] fp32
 *                          twiddle  [770] float64: for the stage of half-size h = 1, 2, .. 128 and j < h, entry h - 1 + j holds
 *                                   cos(pi j / h) at [h - 1 + j] and -sin(pi j / h) at [256 + h - 1 + j] (entries 255, 511 unused);
 *                                   then cos(2 pi k / 512) at [512 + k] and -sin(2 pi k / 512) at [641 + k], k = 0 .. 128
 *                          filters  [3][num_bins] int32: first bin lo, bin count, offset into weights of each triangle; weights
 *                                   [n_weights] float64, the triangle's non-zero weights on bins lo .. lo + count - 1 (bins < 256)
 *                          dct      [num_ceps][num_bins] float64, the lifter folded in (MFCC; else NULL)
 *                        num_bins <= 128, n_weights <= 1024, num_ceps * num_bins <= 1024, and the tables must fit 64 KiB of LDS
 *                        beside the 8 frames a workgroup transforms.
 *   halo_cmvn_batch      in place on [N, M, D]: per utterance and column, minus the mean over the m_n valid rows, divided by the
 *                        unbiased standard deviation (frames.std(dim=0)); float64 sums in one fixed order.  Rows >= m_n are not
 *                        touched; m_n == 1 gives NaN in that row (0 / 0, as the reference's expression), m_n == 0 nothing.
 *   halo_spec_mask       in place on [N, M, D]: one band of columns and one band of frames of every utterance set to 0.  For utterance n
 *                            (r0, r1, r2, r3) = philox4x32_10(ctr = (n, 0, HALO_SPECMASK_STREAM, step), key = (lo32(seed), hi32(seed)))
 *                            u_i = float32(r_i >> 8) * 2^-24
 *                        and, every product and difference rounded to float32,
 *                            columns: P = min(freq_param, D),   v = u0 * P, width = int(v), start = int(u1 * (D - v))
 *                            frames:  P = min(time_param, m_n), v = u2 * P, width = int(v), start = int(u3 * (m_n - v))
 *                        [start, start + width) is masked, on the m_n valid frames only.  This is mask_along_axis_iid's arithmetic on
 *                        the unpadded utterance; the clamp of P to the axis size is the one departure (torchaudio refuses such a call). */
#define HALO_FEATURES_FBANK 0
#define HALO_FEATURES_MFCC 1
#define HALO_SPECMASK_STREAM 0x53504D4Bu     /* 'SPMK': distinct from the dropout sites, HALO_GPT_SAMPLE_STREAM and HALO_MLM_STREAM */
int halo_features_batch(const float *waveforms, const int64_t *lengths, int N, long L, int kind, int frame_len, int shift,
                        float preemphasis, int remove_dc, const float *window, const double *twiddle, const int *filters,
                        const double *weights, int n_weights, int num_bins, const double *dct, int num_ceps, float eps, float *out, int M,
                        int64_t *feature_lengths, halo_stream_t stream);
int halo_cmvn_batch(float *features, const int64_t *feature_lengths, int N, int M, int D, halo_stream_t stream);
int halo_spec_mask(float *features, const int64_t *feature_lengths, int N, int M, int D, int freq_param, int time_param, uint64_t seed,
                   uint32_t step, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Waveform stage.  replaces: the resampling of LabelFile (ha/data.py:33-39, 59-62: 22050 / 32000 / 44100 / 48000 Hz audio to 16 kHz)
 * and the speed: combinator (ha/data.py:126-133, 186-187, torchaudio.transforms.SpeedPerturbation(16000, [0.95, 0.98, 1.0, 1.02, 1.05])),
 * which the reference runs per utterance in its DataLoader workers.  The arithmetic is torchaudio.functional.resample with its defaults
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99); PARITY WITH TORCHAUDIO IS UNPINNED (it is not part of this build), the
 * definition is the one stated here.  For a ratio (orig, new) divided by its gcd:
 *     base = min(orig, new) * 0.99,  width = ceil(6 * orig / base),  K = 2 * width + orig
 *     t[p][k] = clamp(((k - width) / orig - p / new) * base, -6, 6)                                  p < new, k < K, float64
 *     taps[p][k] = (float)((t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / 12)^2 * base / orig)
 *     out_len = (new * len + orig - 1) / orig                                                        64-bit
 *     out[q * new + p] = sum_k taps[p][k] * xpad[q * orig + k],  xpad[i] = x[i - width] inside [0, len), else 0
 * orig == new is a copy: the table (width 0, K = 1, one tap of 1.0).  A speed factor f is the ratio (int(f * rate), rate).
 *
 *   halo_resample_batch  waveforms [N, L] fp32, lengths [N] int64 (device, clamped to [0, L]; a sample at or past lengths[n] is never
 *                        read) -> out [N, L_out] fp32 and out_lengths [N] int64, ONE launch, no atomics, one summation order (taps
 *                        in ascending k, fmaf), so a row's bits depend on neither the run nor the other rows.  Every element of out
 *                        is written; elements at or past out_lengths[n] are exact zeros.  L_out = max over the R ratios of
 *                        (new * L + orig - 1) / orig (the caller passes it; checked).  Tables:
 *                          ratios   HOST int32 [R][6], R <= HALO_RESAMPLE_MAX_RATIOS: orig, new, width, stride, phase_off, tap_off
 *                          phases   device int32 [n_phases]: at phase_off, [new] first non-zero tap k0 of each phase, then [new] counts
 *                          taps     device fp32 [n_taps]: at tap_off + p * stride, taps[p][k0 .. k0 + count); count <= stride (an odd
 *                                   stride keeps consecutive phases on different LDS banks).  The taps left out are exact zeros, so
 *                                   the packed sum is the dense one.
 *                        The ratio of row n: R == 1: ratios[0]; index != NULL: ratios[index[n]] (device int32 [N], clamped to
 *                        [0, R)); else draw != 0 and
 *                            (r0, ..) = philox4x32_10(ctr = (n, 0, HALO_SPEED_STREAM, step), key = (lo32(seed), hi32(seed)))
 *                            u0 = float32(r0 >> 8) * 2^-24,  index = min(int(u0 * R), R - 1)          the product rounded to float32
 *                        indices (device int32 [N], or NULL) receives the ratio each row took.  A workgroup stages one ratio's packed
 *                        taps and the input span of 1024 outputs in LDS: halo_resample_lds_bytes(ratios, R) (-1: bad descriptors)
 *                        must not exceed 64 KiB, else HALO_ENOTSUP. */
#define HALO_RESAMPLE_MAX_RATIOS 8
#define HALO_SPEED_STREAM 0x53504544u        /* 'SPED': distinct from HALO_SPECMASK_STREAM, HALO_GPT_SAMPLE_STREAM, HALO_MLM_STREAM, dropout */
long halo_resample_lds_bytes(const int *ratios, int R);
int halo_resample_batch(const float *waveforms, const int64_t *lengths, int N, long L, const int *ratios, int R, const int *phases,
                        long n_phases, const float *taps, long n_taps, const int *index, int draw, uint64_t seed, uint32_t step,
                        float *out, long L_out, int64_t *out_lengths, int *indices, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The reference's two further lattices, one workgroup per utterance, forward score and gradient.
 *   halo_star_ctc_fwd     ha/star.py:65-166 star_ctc_forward_score(emissions [T, N, C] log-probabilities, targets [N, S], lengths,
 *                         star_penalty): losses [N] = -log of the 4S+3-state star lattice (stars are evaluated from the C symbols in
 *                         the kernel: the 2C-wide emissions of intersperse_stars :9-49 are never built).  workspace (optional, needed
 *                         for the backward): halo_star_ctc_workspace_bytes(T, N, S) bytes, keeps the alpha lattice.
 *   halo_star_ctc_bwd     d sum_n grad_losses[n] * losses[n] / d emissions (what autograd gives the reference), written to
 *                         grad_log_probs with the strides of log_probs; rows at or past emission_lengths[n] are zero.
 *   halo_transducer_fwd   ha/transducer.py:175-207 transducer_forward_score(joint [N, T, U+1, K] log-probabilities, targets [N, U],
 *                         joint_lengths, target_lengths) -> losses [N]; any T (the reference's scan needs T in (2^(k-1/2), 2^k]).
 *   halo_transducer_bwd   its gradient w.r.t. joint (dense [N, T, U+1, K], zero outside the two symbols of every lattice cell). */
size_t halo_star_ctc_workspace_bytes(int T, int N, int S);
int halo_star_ctc_fwd(const float *log_probs, long stride_t, long stride_n, int T, int N, int C, const int64_t *targets, int S,
                      const int64_t *emission_lengths, const int64_t *target_lengths, float star_penalty, void *workspace,
                      float *losses, halo_stream_t stream);
int halo_star_ctc_bwd(const float *log_probs, long stride_t, long stride_n, int T, int N, int C, const int64_t *targets, int S,
                      const int64_t *emission_lengths, const int64_t *target_lengths, float star_penalty,
                      const void *workspace, const float *losses, const float *grad_losses, float *grad_log_probs,
                      halo_stream_t stream);
size_t halo_transducer_workspace_bytes(int N, int T, int U1);
int halo_transducer_fwd(const float *joint, int N, int T, int U1, int K, const int64_t *targets, const int *joint_lengths,
                        const int *target_lengths, void *workspace, float *losses, halo_stream_t stream);
int halo_transducer_bwd(const float *joint, int N, int T, int U1, int K, const int64_t *targets, const int *joint_lengths,
                        const int *target_lengths, const void *workspace, const float *losses, const float *grad_losses,
                        float *grad_joint, halo_stream_t stream);

/* Beam search with the reference's exact (quirky) semantics, one workgroup per utterance.
 * replaces: ha/beam.py:71-137 (logits) and ha/beam.py:5-68 (probs, log_domain = 0).
 *   em [N,T,V]; seqs [N,beam,T] int64, lens [N,beam] int32, scores [N,beam] f32, ranked best first.
 *   workspace: halo_ctc_beam_workspace_bytes().  Requires beam <= 1+V (reference: topk raises).
 *   Scores are formed with torch.logaddexp's CPU arithmetic reproduced bit for bit (ATen's vector loop on Sleef's expf / log1pf
 *   for whole vector chunks of the candidate array, the scalar loop on glibc's expf / log1pf for the remainder and for the
 *   per-prefix update), because on flat emissions score-tied hypotheses are separated by its last ulp.
 *   halo_set_beam_vector_chunk: 2 * Vectorized<float>::size() of the machine whose reference run is to be reproduced:
 *   32 (AVX-512, default: the fixtures under tests/golden/), 16 (AVX2), 0 (no vector ISA: everything through the scalar loop).
 *   halo_logaddexp_aten: that function on its own, element i of n taking the vector path iff i < n - n % chunk. */
int halo_set_beam_vector_chunk(int elements);
int halo_logaddexp_aten(const float *a, const float *b, float *out, size_t n, halo_stream_t stream);
size_t halo_ctc_beam_workspace_bytes(int N, int T, int V, int beam);
int halo_ctc_beam(const float *em, int N, int T, int V, int beam, int log_domain, int64_t *seqs,
                  int32_t *lens, float *scores, void *workspace, halo_stream_t stream);

/* Row-wise top-k with the order torch.topk(largest=True, sorted=True) produces on CPU, equal keys
 * included (ATen TopKImpl.h: partial_sort when k*64 <= n, else nth_element + sort; libstdc++).
 * replaces: seq_logits.topk(beam_size) ha/beam.py:129 (and beam.py:60).
 *   values [rows,n]; out_values [rows,k] f32; out_indices [rows,k] int64; workspace rows*n*8 bytes. */
int halo_topk_f32(const float *values, int rows, int n, int k, float *out_values, int64_t *out_indices,
                  void *workspace, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GPT forward (scoring) operators.  replaces, in ha/attention.py:
 *   halo_embed_fwd            wte(input_ids) + wpe(pos)                      :222-224
 *   halo_layernorm_fwd        F.layer_norm(x, (C,), weight, bias|NULL, eps)  :29  (also StableEmbedding's norm :61)
 *   halo_attention_causal_fwd F.scaled_dot_product_attention(q,k,v,is_causal=True) on the packed c_attn
 *                             output qkv [B,T,3C] (q|k|v, heads side by side) -> y [B,T,C]  :113-123,90
 *   halo_cross_entropy_fwd    F.cross_entropy(logits, targets, ignore_index, reduction='none')  :231; every target must be
 *                             ignore_index or inside [0, V): the row is read at the target unchecked.  -inf logits are
 *                             fine as long as one logit of the row is finite
 * Linear layers, tanh-GELU and the residual adds are halo_gemm_f32 / halo_gemm_split epilogues.
 * halo_attention_causal_fwd is halo_attention_fwd on the packed qkv rows; head_dim in {16, 32, 64} (GPT-2 small: 64). */
int halo_embed_fwd(const int64_t *ids, const float *wte, const float *wpe, float *x, int n_tokens, int T, int C,
                   int pos0, int vocab, halo_stream_t stream);
int halo_layernorm_fwd(const float *x, const float *weight, const float *bias, float *y, int rows, int C,
                       float eps, halo_stream_t stream);
int halo_attention_causal_fwd(const float *qkv, float *y, int B, int T, int n_head, int C, halo_stream_t stream);
int halo_cross_entropy_fwd(const float *logits, const int64_t *targets, float *loss, int rows, int V, long ld,
                           long ignore_index, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Attention operators shared by the GPT path and the encoder-decoder ASR path (ha/transformer.py).
 *   halo_attention_fwd     F.scaled_dot_product_attention(q, k, v, attn_mask|is_causal)   transformer.py:356, attention.py:90
 *                          q rows [N, Tq], k/v rows [N, Tk] given by row/batch strides (elements); head h occupies
 *                          columns [h*head_dim, (h+1)*head_dim) of a row, so the packed q|k|v output of one fused GEMM
 *                          is consumed in place.  Key j is visible to query i iff j < min(Tk, key_lengths[n]) (the
 *                          ~memory_mask of transformer.py:476) and, when causal, j <= i + Tk - Tq.
 *                          lse (optional) [N, heads, Tq] = log-sum-exp of the scaled scores (saved for the backward);
 *                          entropy (optional) [N, heads, Tq] = -sum_j att*log(att + 1e-8), the monitor of attend()
 *                          transformer.py:413-430 (its mean over all rows is att_entropy).  head_dim in {16, 32, 64}.
 *   halo_rope_table /      rotate_interleaved transformer.py:16-31: cos/sin tables [T, head_dim/2] of t * base^(-2i/head_dim);
 *   halo_rope_interleaved  in-place rotation of the pairs (2i, 2i+1) of every head of x rows (row r sits at position
 *                          t0 + r % T); inverse != 0 rotates back (the backward of the rotation).
 *   halo_kv_cache_store    kv_cache[layer, 0|1, alive, :, t0:t0+S, :] = k|v  transformer.py:318-319,333-334: fp32 rows
 *                          (k at column 0, v at column v_offset of each source row) -> float16 caches [N, heads, cache_len, head_dim]
 *   halo_attention_decode  one query token per (n, head) against the first n_keys cached keys: the T == 1 branch of
 *                          MultiHeadAttention.forward transformer.py:313-356; cos/sin tables (optional) rotate the cached
 *                          keys at positions 0..n_keys-1 (transformer.py:343), q must already be rotated.
 *   halo_logprob_max       log_softmax(dim=-1).max(dim=-1) per row (+ sum p*logp/log 2)  transformer.py:175-179,116
 *   halo_greedy_update     the per-step bookkeeping of Decoder.decode transformer.py:179-192 (alive rows only; the entropy
 *                          increment is the sum over ALL alive rows, as the reference's .sum(dim=(-2,-1)) makes it). */
int halo_attention_fwd(const float *q, long q_row_stride, long q_batch_stride, const float *k, const float *v,
                       long kv_row_stride, long kv_batch_stride, float *y, long y_row_stride, long y_batch_stride,
                       float *lse, float *entropy, int N, int heads, int head_dim, int Tq, int Tk, int causal,
                       const int *key_lengths, halo_stream_t stream);
/* halo_attention_fwd with explicit head strides: q_head_stride / kv_head_stride = head_dim for packed rows, or
 * cache_len * head_dim (with row stride head_dim, batch stride heads * cache_len * head_dim) to read K/V straight from a
 * [N, heads, cache_len, head_dim] fp32 cache -- the `past` / `present` layout of ha/attention.py:64-69,232 (attend_cached).
 * p_drop > 0: inverted dropout on the attention probabilities (the dropout_p of SDPA, ha/transformer.py:356,
 * ha/attention.py:90) from the Philox stream (seed, stream_id, offset [+ *offset_dev]); probability (n, h, i, j) uses element
 *   e = ((((n*heads + h)*Tq + i) * ceil(Tk/64) + j/64) * 64 + 4*(j%16) + (j%64)/16
 * of the stream; halo_attention_bwd must be given the same five values. */
int halo_attention_fwd_strided(const float *q, long q_row_stride, long q_batch_stride, long q_head_stride,
                               const float *k, const float *v, long kv_row_stride, long kv_batch_stride,
                               long kv_head_stride, float *y, long y_row_stride, long y_batch_stride, float *lse,
                               float *entropy, int N, int heads, int head_dim, int Tq, int Tk, int causal,
                               const int *key_lengths, float p_drop, uint64_t seed, uint32_t stream_id,
                               uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
int halo_rope_table(float *cos_table, float *sin_table, int T, int head_dim, float base, halo_stream_t stream);
int halo_rope_interleaved(float *x, long row_stride, int n_rows, int T, int heads, int head_dim, int t0,
                          const float *cos_table, const float *sin_table, int table_rows, int inverse,
                          halo_stream_t stream);
/* halo_rope_interleaved on the packed q | k | v rows of the GPT block forms (csrc/rope_rows.hip): ONE launch rotates in place the q and
 * the k column blocks -- columns [0, 2 * heads * head_dim) of each of n_rows rows, 2 * heads heads of head_dim; v and anything beyond it
 * is never touched.  Row r sits at position t0 + r % T; the tables are halo_rope_table's and must cover t0 + T rows; inverse != 0
 * applies the transpose (sine negated: what the backward applies to dq | dk).  is_bf16 == 0: fp32 rows, the expressions of
 * halo_rope_interleaved; != 0: bf16 rows, upcast, rotated in fp32, rounded to nearest even once.  16-byte accesses only:
 * head_dim % 8 == 0, x and both tables 16-byte aligned, row_stride (elements) a multiple of 16 bytes -- anything else is HALO_EINVAL
 * (there is no slow path). */
int halo_rope_rows(void *x, int is_bf16, long row_stride, long n_rows, int T, int heads, int head_dim, int t0,
                   const float *cos_table, const float *sin_table, int table_rows, int inverse, halo_stream_t stream);
int halo_kv_cache_store(const float *src, long src_row_stride, long v_offset, void *cache_k, void *cache_v, int N,
                        int S, int heads, int head_dim, int cache_len, int t0, halo_stream_t stream);
/* fp32 twin of halo_kv_cache_store: present[layer, 0|1, :, :, t0:t0+S, :] of ha/attention.py:66-67,129 */
int halo_kv_cache_store_f32(const float *src, long src_row_stride, long v_offset, float *cache_k, float *cache_v,
                            int N, int S, int heads, int head_dim, int cache_len, int t0, halo_stream_t stream);
int halo_attention_decode(const float *q, long q_row_stride, const void *cache_k, const void *cache_v, float *y,
                          long y_row_stride, int N, int heads, int head_dim, int cache_len, int n_keys,
                          const int *key_lengths, const float *cos_table, const float *sin_table,
                          halo_stream_t stream);
/* One self-attention decode step in ONE launch: k_new / v_new (rows like q, same row stride) are rounded to float16 and stored
 * at cache position n_keys - 1, q is rotated by that position (when tables are given), the cached keys by theirs, and the
 * token attends to all n_keys positions: halo_kv_cache_store + halo_rope_interleaved + halo_attention_decode fused. */
int halo_attention_decode_step(const float *q, const float *k_new, const float *v_new, long row_stride, void *cache_k,
                               void *cache_v, float *y, long y_row_stride, int N, int heads, int head_dim, int cache_len,
                               int n_keys, const float *cos_table, const float *sin_table, halo_stream_t stream);
int halo_logprob_max(const float *logits, long ld, int rows, int V, float *values, int64_t *indices,
                     float *neg_entropy_bits, halo_stream_t stream);
int halo_greedy_update(const float *values, const int64_t *indices, const float *neg_entropy_bits, int64_t *tokens,
                       long tokens_ld, int t, int plen, int etx, uint8_t *alive, int *output_lengths,
                       float *log_probs, float *sum_entropies, int N, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused launches of one batched greedy decode step (ha/transformer.py:160-195; Block.forward :476-494 with kv caches, T == 1):
 * 5 launches per decoder layer + 2 per token.  M = N utterances is one or a few 16-row MFMA tiles, so these do not go through the
 * tiled GEMM: activations are read as fp32 rows, weights from "decode images" (split-bf16 fragments in MFMA operand order).
 *   halo_decode_image        image of a weight matrix W [n_out][k] (nn.Linear layout); halo_decode_image_bytes() bytes, 16-aligned
 *   halo_decode_linear       out (+)= act(layer_norm?(x) W^T): x [rows][k] fp32; ln_weight != NULL applies F.layer_norm(x, weight, no
 *                            bias, eps) first (k in {512, 768, 1024}); flags: HALO_GEMM_ACCUM (residual add into out) and / or
 *                            HALO_GEMM_GELU_ERF; without LayerNorm k % 512 == 0.  Split-bf16 arithmetic (three MFMAs per product, fp32 accumulate).
 *   halo_decode_attention_pair  both attentions of a step from the packed projection rows a [N][4C] = cross query | self q | k | v:
 *                            cross-attention over the fp16 memory caches [N][heads][S][head_dim] (keys < memory_lengths[n]) into
 *                            y[:, 0:C]; halo_attention_decode_step on the time caches (store at n_keys - 1, rotary) into y[:, C:2C]
 *   halo_decode_memory_caches  the float16 cross-attention caches [layers][2][N][heads][S][head_dim] of every layer (transformer.py:324-334)
 *                            from ONE product: kv rows [N*S], layer l's keys at columns [l*2C, l*2C + C), values at [l*2C + C, (l+1)*2C)
 *   halo_decode_token        halo_logprob_max + halo_greedy_update on logits [N][V], then y_next[n] = wte[tokens[n, t + 1]] (the next
 *                            step's embedding; y_next may be NULL).  alive is [2][N], double-buffered: step t reads plane t & 1 and
 *                            writes the other (several workgroups share the step).  N <= 1024. */
int halo_decode_memory_caches(const float *kv, long row_stride, int layers, void *caches, int N, int S, int heads,
                              int head_dim, halo_stream_t stream);
size_t halo_decode_image_bytes(int n_out, int k);
int halo_decode_image(const float *weight, int n_out, int k, long ld, void *image, halo_stream_t stream);
int halo_decode_linear_supported(int k, int layernorm);
int halo_decode_linear(const float *x, long ldx, int rows, int k, const float *ln_weight, float eps, const void *w_image,
                       int n_out, float *out, long ldo, int flags, halo_stream_t stream);
/* The same launch with the residual stream as a PAIR (main, side), x = main + side -- what lets the two accumulating products of a decoder
 * layer (x += proj(...), x += mix_chan[2](...): ha/transformer.py:476-494) run as TWO K-slices on twice the workgroups with every sum in a
 * fixed order: x_side (LayerNorm variants) is added to the input rows before the statistics; side_out != NULL (no LayerNorm, flags ==
 * HALO_GEMM_ACCUM, k % 256 == 0): slice 0 writes out = (out + side_in) + its half of the product (side_in may be NULL), slice 1 its half
 * alone to side_out [rows][ldo]; the next launch reads out + side_out.  side_out must differ from out and side_in. */
int halo_decode_linear_pair(const float *x, const float *x_side, long ldx, int rows, int k, const float *ln_weight, float eps, const void *w_image,
                            int n_out, float *out, const float *side_in, float *side_out, long ldo, int flags, halo_stream_t stream);
int halo_decode_attention_pair(const float *a, long a_row_stride, int N, int heads, int head_dim, const void *mem_k,
                               const void *mem_v, int S, const int *memory_lengths, void *time_k, void *time_v,
                               int cache_len, int n_keys, const float *cos_table, const float *sin_table, float *y,
                               long y_row_stride, halo_stream_t stream);
int halo_decode_token(const float *logits, long ld, int N, int V, int64_t *tokens, long tokens_ld, int t, int plen, int etx,
                      uint8_t *alive, int *output_lengths, float *log_probs, float *sum_entropies, const float *wte,
                      int vocab, int C, float *y_next, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Beam search of the encoder-decoder ASR model (haloop_amd/transformer.py BeamDecoder) on the fused decode launches.  The
 * reference decodes greedily only (ha/transformer.py:124-199), so the definition is this library's own:
 *
 *   State: per utterance W = beam slots, each empty (log-probability -inf), live, or finished (it has emitted ETX).  Before step 0 slot 0
 *   is live with tokens [STX], log-probability 0 and length 0; the others are empty.  The search runs `capacity` steps t = 0 ..
 *   capacity - 1 and never ends early (no host read).
 *   Candidates of a step: a live slot j with lp_j = log_softmax(logits_j) gives the V candidates (j, k) with log-probability
 *   score_j + lp_j[k] and length len_j + (k != ETX); a finished slot gives the one candidate (j, ETX) with its log-probability and length
 *   unchanged; an empty slot gives none.
 *   Ranking: rank = fmaf(length_bonus, length, log-probability).  The W best are taken in the total order (rank descending, position
 *   j V + k ascending); candidates of rank -inf are never taken, and a slot that takes nothing is empty.  A taken candidate becomes a new
 *   slot, in the order taken, with its parent's tokens plus k; it is finished if its parent was or k == ETX.
 *   Result: the beam after the last step, in that order (hypotheses that never closed keep finished == 0).
 *   beam = 1 with length_bonus = 0 is the greedy decode token for token: the first-index arg-max, the log-probability m - lse summed.
 *
 * Slot n * beam + r is hypothesis r of utterance n.  A step is the 5 launches per layer and the LayerNorm + lm_head product of the greedy
 * step on N * beam rows, with halo_decode_beam_attention in the place of halo_decode_attention_pair, and then halo_decode_beam_select.
 *   halo_decode_beam_attention  halo_decode_attention_pair over slots = N * beam rows a [slots][4C].  Cross-attention reads the memory
 *                            caches [N][heads][S][head_dim] of utterance slot / beam (one per utterance, not per slot) and
 *                            memory_lengths[slot / beam].  Self-attention reads position j < n_keys - 1 from row ancestors[slot][j] of
 *                            the time caches [slots][heads][cache_len][head_dim] (values outside [0, slots) are clamped) and stores
 *                            position n_keys - 1 into the slot's own row; ancestors may be NULL at n_keys == 1.  No slot reads what
 *                            another slot stores in the launch.  The sums run in halo_decode_attention_pair's order: with beam = 1 and
 *                            the identity table the same bits.  head_dim 16 / 32 / 64 / 128, up to 8192 keys, slots <= 65535.
 *   halo_decode_beam_select  one workgroup per utterance on logits [N * beam][ld]: one step of the definition above.  It reads the beam
 *                            (scores_in [N][beam] log-probabilities, lengths_in, finished_in, tokens_in [N][beam][tokens_ld] without STX
 *                            and ETX, ancestors_in [N * beam][ancestors_ld]; at t == 0 none of them is read) and writes the new one to
 *                            the *_out buffers, which must be other buffers (the caller alternates two copies by step parity):
 *                            scores_out (-inf: empty), ranks_out, lengths_out, finished_out, tokens_out, and the next step's table
 *                            ancestors_out[r][0 .. t-1] = ancestors_in[parent][0 .. t-1], ancestors_out[r][t] = the parent's slot (an
 *                            empty slot names itself); then y_next[slot] = wte[token] (ETX for an empty slot; y_next may be NULL).
 *                            beam <= 16, V <= 8192, t < capacity <= tokens_ld, ancestors_ld > t.  The utterance's beam V logits stay in
 *                            LDS when they are 8192 floats or fewer and are re-read by the same operations otherwise; no float atomics,
 *                            every sum has one order: bit-reproducible. */
int halo_decode_beam_attention(const float *a, long a_row_stride, int slots, int beam, int heads, int head_dim, const void *mem_k,
                               const void *mem_v, int S, const int *memory_lengths, void *time_k, void *time_v, int cache_len, int n_keys,
                               const int *ancestors, long ancestors_ld, const float *cos_table, const float *sin_table, float *y,
                               long y_row_stride, halo_stream_t stream);
int halo_decode_beam_select(const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                            const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in,
                            const int *ancestors_in, float *scores_out, float *ranks_out, int *lengths_out, int *finished_out,
                            int *tokens_out, int *ancestors_out, long tokens_ld, long ancestors_ld, const float *wte, int vocab, int C,
                            float *y_next, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Joint CTC/attention beam search (BeamDecoder.decode(..., ctc_log_probs, ctc_weight)): the beam search above with every
 * candidate ranked by a mix of the decoder's score and the CTC prefix score of the extended token sequence.  The library's own definition:
 *
 *   Per utterance n: x[t][k], t < T_n = input_lengths[n], the CTC head's log-probabilities; class 0 the blank; ETX the decoder's end token;
 *   a hypothesis's tokens exclude STX and ETX.  A live slot with prefix g carries r[t][2], t < T_n: the log-mass of the CTC paths over
 *   frames 0 .. t that spell exactly g and end in a non-blank (r[t][0]) or in a blank (r[t][1]).
 *   The empty prefix: r[t][0] = -inf, r[t][1] = x[0][0] + ... + x[t][0], psi = 0.
 *   Candidate scores of g, from g's state alone, with both[t] = logaddexp(r[t][0], r[t][1]):
 *     psi(g, 0) = -inf (the lattice cannot spell a blank); psi(g, ETX) = both[T_n - 1] (the utterance spells exactly g: -ctc_loss(g));
 *     every other k: phi[t] = r[t][1] if k is g's last token, else both[t], and
 *     psi(g, k) = logsumexp({phi[t-1] + x[t][k] : 1 <= t < T_n} U {x[0][k] if g is empty}); an empty sum is -inf.
 *   State of h = g.k, k not in {0, ETX}: q[0][0] = x[0][k] if g is empty, else -inf; q[0][1] = -inf; for t >= 1
 *     q[t][0] = logaddexp(q[t-1][0], phi[t-1]) + x[t][k],  q[t][1] = logaddexp(q[t-1][0], q[t-1][1]) + x[t][0].
 *   Ranking with ctc_weight = c in (0, 1]: a candidate (j, k) of a live slot has rank = (1 - c) * fmaf(length_bonus, length, logp) +
 *   c * psi(g_j, k) (two products and a sum in fp32, each rounded); a finished slot's one candidate (j, ETX) uses its stored psi.  Everything
 *   else is the search above: rank -inf is never taken, ties by position j V + k, slots in the order taken, `capacity` steps.  A taken
 *   candidate's psi becomes its slot's psi, so a finished hypothesis ends with (1 - c) * rank + c * (-ctc_loss).
 *
 * fp32 in every arithmetic mode, no float atomics, every sum in one order.  Frames t >= T_n of x and of the states are never read or
 * written.  S <= 4096, V <= 8192, beam <= 16 (HALO_ENOTSUP above).  log_probs [N][S][V] with strides (batch_stride, frame_stride, 1);
 * states [N * beam][S][2], 8-byte aligned, two copies by step parity like the beam's records.
 *   halo_ctc_prefix_scores   psi_cand[slot][k] for every class of every live slot (as halo_decode_beam_select reads the records: at t == 0
 *                            none is read and slot 0 holds the empty prefix; a slot of length 0 holds the empty prefix, otherwise
 *                            last_tokens[slot] is its last token); rows of empty and finished slots are -inf.  One workgroup per (slot,
 *                            64 classes; 32 when V <= 32); both[] and r[.][1] are built once in LDS; threads are (class, one of 4 (8)
 *                            contiguous frame stretches); a max pass and a sum pass, the stretches combined in order, one log per
 *                            (slot, class).
 *   halo_decode_beam_select_joint  halo_decode_beam_select (the same kernel body) with the rank above: psi_cand [N * beam][psi_ld], psi_in /
 *                            psi_out [N][beam] (two copies; psi_in is not read at t == 0), and parents_out [N][beam] = the parent's slot index
 *                            (-1: empty), last_out [N][beam] = the token taken (ETX for an empty slot).  ctc_weight in [0, 1]; with 0 and
 *                            finite psi every output shared with halo_decode_beam_select has that launch's bits.
 *   halo_ctc_prefix_advance  states_out[slot] for every slot that took a label (parents[slot] >= 0 and last_tokens_new[slot] not ETX), from
 *                            states_in[parent]: g is empty iff lengths_new[slot] == 1, and its last token is last_tokens_prev[parent].
 *                            Finished and empty slots are left alone.  parents == NULL: the empty prefix's state into slot 0 of every
 *                            utterance (before step 0; states_in and the records may be NULL).  One wave per slot: 64 frames' operands
 *                            are loaded at once, the serial chain runs over them lane by lane (its two log-sum-exps on the hardware
 *                            exp2 / log2). */
int halo_ctc_prefix_scores(const float *log_probs, long batch_stride, long frame_stride, int N, int beam, int S, int V,
                           const int *input_lengths, const float *states, const int *last_tokens, const int *lengths, const float *scores,
                           const int *finished, int t, int etx, float *psi_cand, long psi_ld, halo_stream_t stream);
int halo_decode_beam_select_joint(const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                                  float ctc_weight, const float *psi_cand, long psi_ld, const float *psi_in, float *psi_out,
                                  const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in,
                                  const int *ancestors_in, float *scores_out, float *ranks_out, int *lengths_out, int *finished_out,
                                  int *tokens_out, int *ancestors_out, int *parents_out, int *last_out, long tokens_ld, long ancestors_ld,
                                  const float *wte, int vocab, int C, float *y_next, halo_stream_t stream);
int halo_ctc_prefix_advance(const float *log_probs, long batch_stride, long frame_stride, int N, int beam, int S, int V,
                            const int *input_lengths, int etx, const float *states_in, float *states_out, const int *parents,
                            const int *last_tokens_new, const int *lengths_new, const int *last_tokens_prev, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LM shallow fusion inside the attention decoder's beam search (fusion.AttentionFusionDecoder): the search of
 * halo_decode_beam_select / _joint with every candidate also scored by an LSTM language model (rnn.Decoder).  The library's own definition,
 * per utterance, W slots, `capacity` steps, exactly the search above with these additions:
 *
 *   Every slot also carries lm, the LM's log-probability of its tokens, and the LSTM state behind lp = log_softmax(lg + lg_bias) over all
 *   V classes, after the LM consumed start_token and then the slot's tokens.  Before step 0 slot 0 holds lm = 0 and the state after
 *   start_token.
 *   lmc(j, k), the LM score of candidate (j, k): lm_j + lp_j[k] for a label k != ETX; for k == ETX lm_j + lp_j[lm_eos] when lm_eos >= 0
 *   and lm_j when lm_eos < 0 (closing costs nothing); lm_j for a finished slot's one candidate.
 *   rank = fmaf(lm_weight, lmc, base), base the rank of the launches above: fmaf(length_bonus, length, score), or the (1 - c) * . + c * psi
 *   mix when psi_cand is given.  The order, the tie rule (rank descending, position j V + k ascending) and the treatment of -inf / NaN
 *   are unchanged.  A taken candidate's lmc becomes its slot's lm.
 *   A slot that took a label steps the LM from its PARENT's state with that label as input; a finished or empty slot's LM state is never
 *   read again.  lm_weight = 0 gives the tokens, lengths, flags and counts of the launches above, scores and ranks comparing equal.
 *
 *   halo_decode_beam_select_lm  the same kernel body as halo_decode_beam_select / _joint (a further instantiation; psi_cand, psi_in and
 *                            psi_out all NULL: the attention-only rank, ctc_weight ignored).  lg [N * beam][ldlg] the LM's logits of every
 *                            slot without their bias, lg_bias [V] (may be NULL); lm_in / lm_out [N][beam] (two copies; lm_in is not read
 *                            at t == 0; -inf in an empty slot); lm_weight finite; lm_eos in -1 .. V-1.  parents_out / last_out as the
 *                            joint launch writes them.  After the selection the launch gathers the next LM step's cell inputs
 *                            (halo_rnnt_lstm_cell): for a slot r that took a label k from parent p, lm_xh[0][r][:H] = lm_wte[k],
 *                            lm_xh[l][r][H:] = h_in[l][p] and c_out[l][r] = c_in[l][p] for every layer l; for every other slot zeros in
 *                            those places (the x halves of the layers above 0 are the cells' own).  h_in, c_in, c_out
 *                            [lm_layers][N * beam][lm_hidden], lm_xh [lm_layers][N * beam][2 lm_hidden], lm_wte [V][lm_hidden], 16-byte
 *                            aligned, lm_hidden % 4 == 0; the state exists twice by step parity (h_in != lm_xh, c_in != c_out), and
 *                            nothing a workgroup writes is read by another in the launch.  lm_xh == NULL (the last step): no gather.
 *                            Both tables of an utterance (beam V decoder logits, beam V LM logits) stay in LDS when 2 beam V <=
 *                            HALO_DECODE_BEAM_LM_LDS_FLOATS and are both recomputed from L2 by the same operations otherwise: the same
 *                            bits.  fp32 in every arithmetic mode, no float atomics, every sum in one order. */
#define HALO_DECODE_BEAM_LM_LDS_FLOATS 14336
int halo_decode_beam_select_lm(const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                               float ctc_weight, const float *psi_cand, long psi_ld, const float *psi_in, float *psi_out, const float *lg,
                               long ldlg, const float *lg_bias, const float *lm_in, float *lm_out, float lm_weight, int lm_eos,
                               const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in,
                               const int *ancestors_in, float *scores_out, float *ranks_out, int *lengths_out, int *finished_out,
                               int *tokens_out, int *ancestors_out, int *parents_out, int *last_out, long tokens_ld, long ancestors_ld,
                               const float *wte, int vocab, int C, float *y_next, const float *lm_wte, int lm_hidden, int lm_layers,
                               const float *h_in, const float *c_in, float *lm_xh, float *c_out, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused launches of one batched GPT sampling step (haloop_amd/generation.py; the T == 1 case of ha/attention.py:253-321 under a KV
 * cache): 5 launches per layer (LayerNorm + c_attn | cache store + attention | c_proj, accumulate | LayerNorm + c_fc + tanh-GELU |
 * mlp.c_proj, accumulate) and 2 per token (LayerNorm + lm_head | the draw), over the decode images of halo_decode_image.  Every per-step
 * scalar (position, draw counter, alive flags, seed, temperature, top_k, stop token) is read from device memory, so the launch arguments
 * of a step never change and one captured step serves every position.
 *   halo_gpt_decode_linear   out (+)= act(layer_norm?(x) W^T) as halo_decode_linear, with flags HALO_GEMM_ACCUM and / or HALO_GEMM_GELU (the
 *                            tanh form).  With LayerNorm (no bias) k in {512, 768, 1024}; without, k % 256 == 0
 *                            (halo_gpt_decode_linear_supported).  Arithmetic by the math mode: bf16x3 the three-MFMA split product, bf16 the
 *                            activations rounded to bf16 against the hi fragments alone (one MFMA, half the image read); HALO_ENOTSUP in f32.
 *   halo_gpt_decode_attention  one layer's attention of a step from the packed rows qkv [B][>= 3C] = q | k | v: row b's k and v are stored at
 *                            position p = clamp(pos[b], 0, cache_len - 1) of the fp32 cache planes [B][heads][cache_len][64] (the reference's
 *                            `present` layout, ha/attention.py:64-69), the query attends over keys 0 .. p, y [B][C].  pos: device int32 [B];
 *                            the host checks the largest position it will reach before launching.  head_dim 64, cache_len <= 8192.
 *   halo_gpt_sample          the draw and the bookkeeping of a step, one workgroup per row of logits [B][V].  cfg: device int32 [8] =
 *                            { bits of float 1 / temperature, top_k (<= 0: none), stop_token, lo32(seed), hi32(seed), 0, 0, 0 };
 *                            state: device int32 [4][state_ld] = pos | step | length | alive, one word of each per row (a row's words are
 *                            read and written by that row's workgroup alone, so nothing races within the launch; the launches that read
 *                            pos are ordered against this one by the stream).  A row:
 *                              l_v = logits[v] / temperature as fl(logits[v] * (1 / temperature)); with top_k the kept set is
 *                              { v : logits[v] >= the min(top_k, V)-th largest logit } (ties at the threshold stay), else every v;
 *                              e_v = expf(l_v - max l) over the kept set; chunk sums in vocabulary order (chunk = 4 ceil(V / 1024) consecutive
 *                              indices, summed left to right), the chunk sums accumulated left to right: total;
 *                              r = philox4x32_10(ctr = (row, 0, HALO_GPT_SAMPLE_STREAM, step[row]), key = seed)[0], u = (r >> 8) * 2^-24;
 *                              token = the smallest kept v whose cumulative mass (the chunk prefix plus the running sum inside its chunk)
 *                              exceeds u * total; top_k == 1: the arg max, lowest index on ties.
 *                            Then, for an alive row: token == stop_token turns the row dead (the token is not counted), else length += 1;
 *                            a dead row's token is stop_token.  tokens[row][step] = token while step < n_slots; next_ids[row] = token;
 *                            step += 1; pos += 1; x_next[row] = wte[clamp(token)] + wpe[min(pos, n_pos - 1)] when x_next is given (the
 *                            next step's input row).  Same (logits, cfg, state) -> same tokens.
 * HALO_GPT_SAMPLE_STREAM is outside the dropout sites' ids (small integers) and the LoRA sites' (4096 + layer). */
#define HALO_GPT_SAMPLE_STREAM 0x47505453u   /* 'GPTS' */
#define HALO_MLM_STREAM 0x4D4C4D31u          /* 'MLM1': the token-masking draws of halo_mask_tokens / halo_mlm_batch_u16 */
int halo_gpt_decode_linear_supported(int k, int layernorm);
int halo_gpt_decode_linear(const float *x, long ldx, int rows, int k, const float *ln_weight, float eps, const void *w_image,
                           int n_out, float *out, long ldo, int flags, halo_stream_t stream);
int halo_gpt_decode_attention(const float *qkv, long row_stride, int B, int heads, int head_dim, float *cache_k, float *cache_v,
                              int cache_len, const int *pos, float *y, long y_row_stride, halo_stream_t stream);
int halo_gpt_sample(const float *logits, long ld, int B, int V, const int *cfg, int *state, long state_ld, int64_t *tokens,
                    long tokens_ld, int n_slots, int64_t *next_ids, const float *wte, const float *wpe, int n_pos, int C,
                    float *x_next, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Greedy decode of the RNN transducer head (haloop_amd/transducer.py GreedyDecoder; [Graves12] greedy search over the additive joint of
 * ha/recognizer.py:86-127, blank 0) as a launch sequence: per emitted symbol one halo_rnnt_advance, one halo_rnnt_lstm_cell per LSTM
 * layer and one halo_decode_linear (out_layer, on the image of the tied embedding).  Blank frames cost no launch; every launch is finite
 * (no grid barrier, no polling) and none reads a buffer another workgroup of the same launch writes.
 *   halo_rnnt_advance    one workgroup per row n of f [N][T][V] (the transcription logits; strides in floats).  state: device int32
 *                        [5][state_ld] = t | u | here | done | truncated, one word of each per row; a row with done != 0 is skipped.
 *                        With l = g[n, :] + g_bias (g_bias may be NULL) and L = clamp(input_lengths[n], 0, T), the row walks its frames
 *                        from t: lp = log_softmax(f[n, t] + l); k = 0 when here == max_symbols, else argmax lp (lowest index on ties).
 *                        k == 0: scores[n] += lp[0], t += 1, here = 0, next frame -- the sums in frame order.  The first k != 0:
 *                        tokens[n][u] = k, frames[n][u] = t, scores[n] += lp[k], u += 1, here += 1; u == capacity sets done and
 *                        truncated, otherwise x_next[n][0 .. E) = wte[k] (layer 0's next input row).  t == L sets done.  Frames at or
 *                        past L are never read.  *live += 1 for every row not done afterwards (the caller zeroes the word; a fresh
 *                        word per launch needs no reset).  V <= 8192, E % 4 == 0; wte has V rows.
 *   halo_rnnt_lstm_cell  one LSTM layer at one step for `rows` rows: gates = xh [W_ih | W_hh]^T + b_ih + b_hh with xh [rows][2 hidden] =
 *                        x | h_prev (input size == hidden), then c = f c + i g, h = o tanh(c) (nn.LSTM's gate order i, f, g, o) in the same
 *                        launch.  w_image: halo_decode_image of the [4 hidden][2 hidden] matrix whose row 16 j + 4 q + i is row
 *                        q hidden + 4 j + i of [W_ih | W_hh] (one feature tile = the four gates of four units).  The split three-MFMA
 *                        product of halo_decode_linear (2 hidden must pass halo_decode_linear_supported(k, 0)); the biases are indexed in
 *                        nn.LSTM's layout.  c [rows][hidden] is updated in place (each element by one thread); h is written twice: to
 *                        h_next (this layer's h_prev of the next step: the h half of the OTHER copy of its xh rows) and to h_up (the x
 *                        half of the layer above in this step, or out_layer's input).  xh, c, h_next and h_up may not overlap. */
int halo_rnnt_advance(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                      const float *g_bias, const int *input_lengths, int *state, long state_ld, float *scores, int64_t *tokens,
                      int64_t *frames, long tokens_ld, int capacity, int max_symbols, const float *wte, int E, float *x_next, long ldx,
                      int *live, halo_stream_t stream);
int halo_rnnt_lstm_cell(const float *xh, long ldx, int rows, int hidden, const void *w_image, const float *b_ih, const float *b_hh,
                        float *c, float *h_next, long ld_next, float *h_up, long ld_up, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same greedy search carried across calls (haloop_amd/transducer.py GreedyStream): the logits arrive in chunks and
 * a row's search goes on where the previous call left it.  The state is halo_rnnt_advance's plus pos and row_mask, int32 [rows] each.
 * The word t counts the frames of the whole stream (frames[u] is stream-absolute); `done` means "sits out the rest of this call".
 *   halo_rnnt_stream_open     once per call, one workgroup per row of the state (rows >= B take no part): pos = 0; done = 1 for a row
 *                             with n_frames <= 0 or truncated, else 0; row_mask = 0.  A row whose flags (may be NULL) carry bit 1 (begin)
 *                             is reset first: t = u = here = truncated = 0, score 0, its `capacity` slots of tokens / frames -1, h
 *                             (xh[l][n][hidden ..], layers xh_layer_stride floats apart) and c (layers c_layer_stride apart) of every
 *                             layer zero, xh[0][n][0 .. E) = wte[0], row_mask = 1: one masked step of the prediction network gives it g.
 *                             live[0 .. n_live) = 0.
 *   halo_rnnt_advance_stream  halo_rnnt_advance over this call's chunk f [N][T][V]: row n walks the frames [pos[n], clamp(n_frames[n],
 *                             0, T)).  A row that runs out of them sets done and keeps everything else (it waits); u == capacity sets
 *                             done and truncated, which stays until the row begins again.  pos[n] is updated; row_mask[n] = 1 for a row
 *                             that emitted and goes on, else 0 (rows skipped as done included).
 *   halo_rnnt_lstm_cell_rows  halo_rnnt_lstm_cell with row_mask [rows] (NULL: every row): a row with 0 keeps c, gets its h_prev
 *                             (xh[row][hidden ..]) written to h_next, and writes no h_up. */
int halo_rnnt_stream_open(const int *n_frames, const int *flags, int B, int rows, int *state, long state_ld, int *pos, int *row_mask,
                          float *scores, int64_t *tokens, int64_t *frames, long tokens_ld, int capacity, float *xh, long xh_layer_stride,
                          long ldx, float *c, long c_layer_stride, const float *wte, int E, int hidden, int layers, int *live, int n_live,
                          halo_stream_t stream);
int halo_rnnt_advance_stream(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                             const float *g_bias, const int *n_frames, int *state, long state_ld, float *scores, int64_t *tokens,
                             int64_t *frames, long tokens_ld, int capacity, int max_symbols, const float *wte, int E, float *x_next,
                             long ldx, int *live, int *pos, int *row_mask, halo_stream_t stream);
int halo_rnnt_lstm_cell_rows(const float *xh, long ldx, int rows, int hidden, const void *w_image, const float *b_ih, const float *b_hh,
                             float *c, float *h_next, long ld_next, float *h_up, long ld_up, const int *row_mask, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Beam search of the RNN transducer head (haloop_amd/transducer.py BeamDecoder; alignment-length synchronous decoding with exact merging,
 * [Saon20]) as a launch sequence: per alignment step one halo_rnnt_beam_step, one halo_rnnt_lstm_cell per LSTM layer and one
 * halo_decode_linear on all N * beam slots, and one halo_rnnt_beam_keep.  Slot n * beam + r is hypothesis r of row n.  The beam's records
 * (scores, symbols emitted, tokens) and the state (h and c [layers][N * beam][hidden], g [N * beam][ldg]) exist twice; a step reads one
 * copy and writes the other, so no launch reads what another of its workgroups writes.
 *   halo_rnnt_beam_step  one workgroup per row n of f [N][T][V].  Hypothesis j of the beam read (u_in[n][j] >= 0; at step 0 the records
 *                        are not read: the beam is the empty hypothesis with score 0, or nothing when L = clamp(input_lengths[n], 0, T)
 *                        is 0, and the row's finals are reset -- to the empty hypothesis with score 0 when L is 0) stands at frame
 *                        t_j = step - u_j < L; lp_j = log_softmax(f[n, t_j] + g[slot j] + g_bias).  Candidates, in this order: the blank
 *                        extension of every j (score + lp_j[0]; at t_j + 1 == L it is complete and goes to the finals instead), then for
 *                        every j with u_j < capacity the extension by k = 1 .. V - 1.  The extension of j by k that spells the tokens of
 *                        hypothesis s is merged into s's blank extension (logaddexp).  The `beam` best by (score descending, position
 *                        ascending) become the new beam: scores_out, u_out, tokens_out [N][beam][tokens_ld], parent (the slot within the
 *                        row it came from; -1: no hypothesis), last (the new token; 0: a blank extension).  The finals keep the row's
 *                        `beam` best complete hypotheses, unordered: fin_scores (-inf: none), fin_seq (order of completion), fin_lengths
 *                        (-1: none), fin_tokens [N][beam][tokens_ld], fin_n [N] (hypotheses completed so far); a later one displaces
 *                        the worst kept only with a strictly higher score.  The gather: xh [layers][N * beam][2 hidden] of every new slot
 *                        = wte[last] (layer 0's x half) | h_in of its parent (the h halves), c_out = c_in of its parent.  *live += 1 for
 *                        every row whose new beam is not empty.  Frames at or past L are never read.  V <= 8192, beam <= 16, hidden % 4
 *                        == 0; the sums have a fixed order: bit-reproducible.
 *   halo_rnnt_beam_keep  one workgroup per slot: a slot with parent >= 0 and last == 0 takes h, c and g of its parent's slot from the
 *                        copy the step read (h_in, c_in, g_in) into the copy the cells and out_layer wrote (h_out, c_out, g_out). */
int halo_rnnt_beam_step(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                        const float *g_bias, const int *input_lengths, int step, int beam, int capacity, const float *scores_in,
                        const int *u_in, const int *tokens_in, float *scores_out, int *u_out, int *tokens_out, long tokens_ld,
                        int *parent, int *last, float *fin_scores, int *fin_seq, int *fin_lengths, int *fin_tokens, int *fin_n,
                        const float *wte, int hidden, int layers, const float *h_in, const float *c_in, float *xh, float *c_out,
                        int *live, halo_stream_t stream);
int halo_rnnt_beam_keep(int slots, int beam, int V, int hidden, int layers, const int *parent, const int *last, const float *h_in,
                        const float *c_in, const float *g_in, long ldg, float *h_out, float *c_out, float *g_out, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same beam search carried across calls (haloop_amd/transducer.py BeamStream): the logits arrive in chunks, the beam
 * stays in device memory, and after the final call a row's finals are halo_rnnt_beam_step's over the whole utterance, bit for bit.  Every
 * row has four words in stream_state int32 [4][state_ld]: its alignment step, the frames received R, final (no more frames follow) and
 * closed (its search is over, or it never began), and a ring [rows][ring_frames][V] of its latest logit frames, frame t at t % ring_frames.
 * A call is one halo_rnnt_beam_stream_open, then rounds of (halo_rnnt_beam_step_stream, the cells and halo_decode_linear on all rows *
 * beam slots, halo_rnnt_beam_keep) until a round leaves its live word 0.  Records and state exist twice and every round crosses to the
 * other copy for every row; the caller carries the parity across calls.
 *   halo_rnnt_beam_stream_open  one workgroup per row of the state; rows >= B take no part.  live[0 .. n_live) = 0.  A row whose flags
 *                               (may be NULL) carry bit 1 (begin) is reset first: step = R = final = closed = 0, the empty hypothesis with
 *                               score 0 in slot 0 of scores / u (the copy the next step reads), no finals, and h0 / c0 [layers][hidden] and
 *                               g0 [V] (the prediction network after the zero prefix) in slot 0 of h, c [layers][rows * beam][hidden] and
 *                               g.  A row that is closed or final and does not begin is left as it is.  Otherwise the row's first
 *                               clamp(n_frames, 0, S) frames of f [B][S][V] go to the ring at R % ring_frames and R grows; bit 2 (final)
 *                               sets final, and with R == 0 the finals become the empty hypothesis with score 0 and the row is closed.
 *   halo_rnnt_beam_step_stream  halo_rnnt_beam_step with the step, R and the flags read from the row's words.  A row executes its step
 *                               iff it is not closed, its beam is not empty, and it is final (then L = R) or every hypothesis stands
 *                               at a frame t_j with t_j + 1 < R (then no blank extension is complete and no frame >= R is read);
 *                               it then adds 1 to its step, sets closed when a final row's new beam is empty, and *live += 1 iff its
 *                               next step is executable by the same rule.  Every other row does an identity round: records and tokens
 *                               cross to the other copy unchanged, parent[r] = r for a present slot and -1 otherwise, last = 0, the
 *                               gather is from the slot itself, so halo_rnnt_beam_keep carries h, c and g across.  ring_frames >=
 *                               capacity + S + 1 holds every frame a step can read after calls of at most S frames. */
int halo_rnnt_beam_step_stream(const float *ring, int ring_frames, int rows, int V, const float *g, long ldg, const float *g_bias,
                               int *stream_state, long state_ld, int beam, int capacity, const float *scores_in, const int *u_in,
                               const int *tokens_in, float *scores_out, int *u_out, int *tokens_out, long tokens_ld, int *parent,
                               int *last, float *fin_scores, int *fin_seq, int *fin_lengths, int *fin_tokens, int *fin_n,
                               const float *wte, int hidden, int layers, const float *h_in, const float *c_in, float *xh, float *c_out,
                               int *live, halo_stream_t stream);
int halo_rnnt_beam_stream_open(const float *f, long f_row_stride, long f_frame_stride, int B, int S, int V, const int *n_frames,
                               const int *flags, int rows, float *ring, int ring_frames, int *stream_state, long state_ld, int beam,
                               float *scores, int *u, float *fin_scores, int *fin_seq, int *fin_lengths, int *fin_n, const float *h0,
                               const float *c0, const float *g0, float *h, float *c, float *g, long ldg, int hidden, int layers,
                               int *live, int n_live, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The RNN transducer's training loss over the additive joint z[n, t, u, k] = f[n, t, k] + g[n, u, k] (haloop_amd/transducer.py
 * transducer_loss; the quantity of ha/recognizer.py:121-126, rnnt_loss(..., fused_log_softmax=True)) without a tensor of N T U1 V elements:
 * halo_rnnt_joint_fwd, then halo_transducer_fwd / halo_transducer_bwd on lp2 as a joint with K = 2 and targets of ones, then
 * halo_rnnt_joint_bwd.  f [N][T][V] and g [N][U1][V] are fp32 with unit stride along V and an n stride and a row stride in floats (rows
 * may not overlap: a transposed view of time-major rows is fine); targets [N][U1 - 1] (labels outside [0, V) are treated as absent, never
 * indexed); f_lengths / target_lengths [N] int32, clamped to [0, T] / [0, U1 - 1].  Exact fp32 in every math mode.  Limits: 1 <= N <= 65535,
 * T >= 1, 2 <= U1 <= 7679 (the lattice kernels' bound), 1 <= V <= 8192.  Every launch is finite (no grid barrier, no polling) and no
 * workgroup reads what another workgroup of its launch writes.
 *   halo_rnnt_joint_fwd  for every cell t < f_lengths[n], u <= target_lengths[n]: lse[n][t][u] = log sum_k exp(z[k]), computed against the
 *                        cell's own maximum; lp2[n][t][u][0] = z[0] - lse; lp2[n][t][u][1] = z[targets[n][u]] - lse for
 *                        u < target_lengths[n], else 0.  Every other cell of lse [N][T][U1] and lp2 [N][T][U1][2] is written as 0 (a
 *                        finite fill: the lattice's alpha sweep walks those cells, nothing reads them as data).
 *   halo_rnnt_joint_bwd  with (gb, gy) = grad_lp2[n][t][u][0 .. 1] (halo_transducer_bwd's output) and p[k] = exp(z[k] - lse[n][t][u]), the
 *                        gradient at the joint logit is dz[k] = gb [k == 0] + gy [k == targets[n][u]] - (gb + gy) p[k]; it is never stored:
 *                        df[n][t][k] = sum_u dz[k] (in u order) and dg[n][u][k] = sum_t dz[k] (in t order), over the cells inside the
 *                        lengths.  Two launches, each recomputing p; every output element is summed by one thread in a fixed order (no
 *                        atomics: bit-reproducible from run to run).  Rows t >= f_lengths[n] of df and u > target_lengths[n] of dg are
 *                        written as zeros.  df and dg are written through their own strides (same rules as f and g; they may not alias
 *                        f, g, lse or grad_lp2). */
int halo_rnnt_joint_fwd(const float *f, long f_n_stride, long f_t_stride, const float *g, long g_n_stride, long g_u_stride, int N, int T,
                        int U1, int V, const int64_t *targets, const int *f_lengths, const int *target_lengths, float *lse, float *lp2,
                        halo_stream_t stream);
int halo_rnnt_joint_bwd(const float *f, long f_n_stride, long f_t_stride, const float *g, long g_n_stride, long g_u_stride, int N, int T,
                        int U1, int V, const int64_t *targets, const int *f_lengths, const int *target_lengths, const float *lse,
                        const float *grad_lp2, float *df, long df_n_stride, long df_t_stride, float *dg, long dg_n_stride,
                        long dg_u_stride, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Forced alignment: the best path (max-plus, "log 0" = -inf) of the two lattices and its backtrace, one workgroup per utterance
 * (csrc/viterbi.hip).  The reference has no aligner (TemporalClassifier.decode, ha/recognizer.py:48-59, returns greedy
 * alignments only): a capability of this library.  fp32, no atomics (bit-reproducible); every launch is finite (no grid barrier, no
 * polling) and no workgroup reads what another workgroup of its launch writes.  Emissions are read from global memory a few frames
 * ahead of the recursion, never staged whole: T is bounded by the workspace alone.
 *   halo_ctc_viterbi         lp, targets, input_lengths (NULL: T), target_lengths as halo_ctc_fwd takes them (lengths clamped to [0, T] /
 *                            [0, S]); F.ctc_loss's lattice: states 0 .. 2 tl, starts at state 0 or 1, ends at state 2 tl or 2 tl - 1 of
 *                            frame il - 1, the skip s-2 -> s only into a label that differs from the label two states back;
 *                            v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if skip) + lp[t][ext[s]].  Ties: the smallest shift (stay,
 *                            then s-1, then s-2); at the end state 2 tl before 2 tl - 1.  A label outside [0, C) is never indexed (its
 *                            state is unreachable); targets past target_lengths[n] are never read.
 *                            scores [N]: the best path's log-probability, -inf for an infeasible row; alignments [N][T] int64: the label
 *                            of each frame's state (0 = blank), -1 at t >= il and in a whole infeasible row; starts / ends [N][S] int32:
 *                            first / last frame of each target token's label state, -1 for u >= tl and in infeasible rows.  tl = 0: the
 *                            all-blank path; il = 0: score 0 if tl = 0, else infeasible.
 *                            workspace: halo_ctc_viterbi_workspace_bytes(T, N, S) bytes, 2 bits per (t, s) as [N][T][ceil((2S+1)/64)][2]
 *                            uint64 (bit s % 64 of the two words = the shift into s at frame t).  Limits: 1 <= S <= 3839 (2S+1 <= 7679
 *                            states, spread over the workgroup's threads: one wave up to 64 states, else up to 30 states per thread of
 *                            256); HALO_ENOTSUP above.
 *   halo_transducer_viterbi  joint, targets, joint_lengths, target_lengths as halo_transducer_fwd takes them (on halo_rnnt_joint_fwd's lp2:
 *                            K = 2, targets of ones); lengths clamped to [0, T] / [0, U1 - 1]; cells outside them are never read:
 *                            v[t][u] = max(v[t-1][u] + joint[t-1][u][0], v[t][u-1] + joint[t][u-1][y[u-1]]) along the anti-diagonals,
 *                            scores [N] = v[Tn-1][Un] + joint[Tn-1][Un][0].  Tie: the blank predecessor (t-1, u).  frames [N][U1 - 1] int32:
 *                            the frame at which target token u is emitted (GreedyDecoder's `frames`), -1 for u >= Un.  A row with Tn = 0
 *                            (or a -inf score) gets score -inf and frames -1.
 *                            workspace: halo_transducer_viterbi_workspace_bytes(N, T, U1) bytes, 1 bit per cell as
 *                            [N][T + U1 - 1][ceil(U1/64)] uint64 (bit u % 64 of word [t + u][u / 64] set: entered by the label arc).
 *                            Limits: 2 <= U1 <= 7679 as the lattice kernels. */
size_t halo_ctc_viterbi_workspace_bytes(int T, int N, int S);
int halo_ctc_viterbi(const float *lp, long stride_t, long stride_n, int T, int N, int C, const int64_t *targets, long tg_stride, int S,
                     const int64_t *input_lengths, const int64_t *target_lengths, void *workspace, float *scores, int64_t *alignments,
                     int *starts, int *ends, halo_stream_t stream);
size_t halo_transducer_viterbi_workspace_bytes(int N, int T, int U1);
int halo_transducer_viterbi(const float *joint, int N, int T, int U1, int K, const int64_t *targets, const int *joint_lengths,
                            const int *target_lengths, void *workspace, float *scores, int *frames, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Edit distance and the minimum-word-error-rate risk of an n-best list (csrc/edit_distance.hip).  The reference counts
 * word errors on the host through kaldialign (ha/wer.py:28-52) and has no MWER objective ([Prabhavalkar18], [Guo20]): the risk is a
 * capability of this library.  No atomics, no workspace (bit-reproducible); every launch is finite and no workgroup reads what another
 * workgroup of its launch writes.
 *   halo_edit_distance   batched Levenshtein distance with operation counts, one workgroup per pair.  hyp [P][hyp_stride] int64 (tokens
 *                        0 .. Lh - 1 of a row, unit stride), hyp_lengths [P] int32; ref [R][ref_stride] int64, ref_lengths [R] int32;
 *                        P = R * group, pair p is scored against reference p / group (the [N, W, capacity] n-best lists of the beam
 *                        search against their rows' transcripts: group = W).  Lengths above Lh / Lr are clamped to them, a negative
 *                        ref length to 0; tokens at or past a length are never read (padding may hold anything).
 *                        errors [P] int32: the distance; counts [P][3] int32 = (ins, del, sub) in ha/wer.py's sense: ins = hypothesis
 *                        tokens without a reference partner, del = reference tokens without a hypothesis partner, sub = partners that
 *                        differ; ins + del + sub = errors.  hyp_lengths[p] < 0 (an absent hypothesis): errors -1, counts 0.
 *                        Tie rule (the distance is unique, the counts are not): with D[i][j] the distance of the first i hypothesis
 *                        tokens to the first j reference tokens, every cell keeps ONE predecessor among those that give its minimal
 *                        total, taken in the order diagonal (i-1, j-1: match or substitution), deletion (i, j-1), insertion (i-1, j);
 *                        the counts are those of the path these choices lead along from (Lh, Lr) back to (0, 0).  (The counts travel
 *                        forward with the cost, which yields exactly that path's: no back-pointers, no backtrace.)
 *                        Limits: 0 <= Lh, Lr <= HALO_EDIT_DISTANCE_MAX_LEN = 1024 tokens (one wave up to Lr = 64, else up to 4 reference
 *                        columns per thread of 256); HALO_ENOTSUP above, nothing is launched.
 *   halo_nbest_risk_fwd  losses [N][W] fp32 = -log P(hypothesis | x), errors [N][W] int32 (< 0: absent), W <= 16.  Over the present
 *                        hypotheses of a row: p = softmax(-losses) (the maximum taken out before the exponentials),
 *                        risk [N] = sum_w p_w err_w - mean_w err_w (the plain mean as the baseline, [Prabhavalkar18]; it has no gradient);
 *                        a row without a present hypothesis has risk 0.
 *   halo_nbest_risk_bwd  dlosses [N][W] = grad_risk[n] * -p_w (err_w - sum_v p_v err_v); 0 for an absent hypothesis.
 *                        Both: fp32, one thread per row, sums in hypothesis order. */
#define HALO_EDIT_DISTANCE_MAX_LEN 1024
int halo_edit_distance(const int64_t *hyp, long hyp_stride, const int *hyp_lengths, int P, int Lh, const int64_t *ref, long ref_stride,
                       const int *ref_lengths, int R, int Lr, int group, int *errors, int *counts, halo_stream_t stream);
int halo_nbest_risk_fwd(const float *losses, const int *errors, int N, int W, float *risk, halo_stream_t stream);
int halo_nbest_risk_bwd(const float *losses, const int *errors, int N, int W, const float *grad_risk, float *dlosses, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CTC prefix beam search with exact merging ([Hannun14], Graves' prefix search; csrc/ctc_prefix_beam.hip): n-best lists
 * from CTC emissions in the format of the transducer beam search.  The reference's own CTC beam (ha/beam.py, halo_ctc_beam above) never
 * merges hypotheses that spell the same tokens; this search is a capability of this library.  One launch for the whole batch, one
 * workgroup per utterance, the frame loop inside; fp32, no float atomics, every sum in a fixed order (bit-reproducible); the launch is
 * finite and no workgroup reads what another workgroup writes.
 *   halo_ctc_prefix_beam   emissions [T][N][V] fp32 log-probabilities, read in place (stride_t, stride_n in floats, unit class stride;
 *                          they are not normalised here); emission_lengths [N] int64 (NULL: T), L = clamp(., 0, T); frames at or past L
 *                          are never loaded.  Class 0 is the blank.  Per row, with W = beam and cap = capacity:
 *                              beam = [((), pb = 0, pnb = -inf)]     pb / pnb: log-mass of the prefix's alignments ending in blank / in
 *                                                                    its last label
 *                              for t in 0 .. L-1:
 *                                total_j = logaddexp(pb_j, pnb_j)
 *                                candidates, in this order:
 *                                  for j in beam order: stay (y_j, pb' = total_j + e[t][0], pnb' = pnb_j + e[t][last(y_j)], -inf for the
 *                                      empty prefix)
 *                                  for j in beam order, if len(y_j) < cap, for k = 1 .. V-1: extension (y_j + [k], pb' = -inf,
 *                                      pnb' = e[t][k] + (pb_j if k == last(y_j) else total_j))
 *                                an extension that spells the prefix of a stay candidate s is merged into it
 *                                  (pnb'_s = logaddexp(pnb'_s, the extension's pnb')) and dropped.  Equality of prefixes is decided by
 *                                  comparing tokens (a hash only shortlists).  Beam members are distinct, so this is the only merge.
 *                                beam = the W best candidates by (logaddexp(pb', pnb') descending, candidate position ascending: a stay
 *                                  before every extension, then beam order, then k); candidates at -inf are never kept
 *                          Outputs, best first in that order: tokens [N][beam][capacity] int64 (-1 past a hypothesis's length and in absent
 *                          hypotheses), lengths [N][beam] int64 (-1: absent), scores [N][beam] = logaddexp(pb, pnb) (-inf: absent),
 *                          counts [N] int64.  L = 0: the empty hypothesis alone, score 0.  Without pruning a score is the CTC lattice total
 *                          log P(y | x), what halo_ctc_fwd negates; with pruning a lower bound of it.
 *                          Limits: 1 <= beam <= 16, 2 <= V <= 2^26, T >= 1, 1 <= capacity <= T.
 *                          workspace: halo_ctc_prefix_beam_workspace_bytes(N, T, V, beam, capacity) bytes (NULL when that is 0): the
 *                          token rows of the beam, [N][2][beam][capacity] int32, when they do not fit LDS (V > 65536 or
 *                          2 beam capacity > 12288); 0 for an invalid shape. */
size_t halo_ctc_prefix_beam_workspace_bytes(int N, int T, int V, int beam, int capacity);
int halo_ctc_prefix_beam(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int64_t *emission_lengths,
                         int beam, int capacity, void *workspace, int64_t *tokens, int64_t *lengths, float *scores, int64_t *counts,
                         halo_stream_t stream);

/* The same search with the beam carried between launches (haloop_amd/ctc.py PrefixBeamStream, streaming.py): a stream's
 * frames arrive over any number of launches, and after each the n-best list of the frames so far is what halo_ctc_prefix_beam returns
 * on their concatenation, bit for bit (one frame body, the same operations in the same order).
 *   halo_ctc_prefix_beam_advance  row n takes its first clamp(n_frames[n], 0, T) frames of emissions [T][N][V] (NULL: T; strides as
 *                          above, read in place).  flags [N]: the per-stream flags of the streaming launches (bit 0 active, bit 1 begin,
 *                          bit 2 final), of which only begin is read; NULL: no row begins.  A beginning row starts from the empty prefix
 *                          whatever its state held, then takes its frames.  A row with no frames and no begin is left bit-identical:
 *                          its state row and its rows of the four outputs.  Every other row has its state row and its n-best rows
 *                          written, in halo_ctc_prefix_beam's format; a row begun with no frames holds the empty hypothesis, score 0.
 *                          state [N][halo_ctc_prefix_beam_state_bytes(V, beam, capacity)], opaque, the caller's to keep between
 *                          launches of the same V, beam and capacity; a row needs no initialisation before it begins (zeros are an
 *                          empty beam).  A row holds the beam's records (pb, pnb, score, length, last token, the two hashes), the
 *                          member count and the token rows: 512 + 2 beam capacity bytes where the launch works on the token rows in LDS
 *                          (V <= 65536 and 2 beam capacity <= 12288), else 512 + 8 beam capacity (the token rows rounded up to 16 bytes).  capacity is the longest hypothesis
 *                          of the stream, independent of T: 1 <= capacity <= HALO_CTC_PREFIX_BEAM_MAX_CAPACITY (1 MiB + 512 bytes per row
 *                          at beam 16).  Other limits as above; state_bytes is 0 for an invalid shape. */
#define HALO_CTC_PREFIX_BEAM_MAX_CAPACITY 8192
size_t halo_ctc_prefix_beam_state_bytes(int V, int beam, int capacity);
int halo_ctc_prefix_beam_advance(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int *n_frames,
                                 const int *flags, int beam, int capacity, void *state, int64_t *tokens, int64_t *lengths, float *scores,
                                 int64_t *counts, halo_stream_t stream);

/* Contextual biasing ("hotwords") inside both searches (haloop_amd/biasing.py ContextGraph, csrc/ctc_prefix_beam.hip with BIASED set;
 * DESIGN.md 3.3ac): a phrase list compiled on the host into an automaton over token ids; a hypothesis that is spelling a phrase holds a
 * bonus per matched token, gives it back when the match breaks and keeps it when the phrase completes.  Still one launch, no host read.
 *   The automaton.  Phrases are non-empty token sequences over 1 .. V-1, duplicates dropped.  Their trie has the root as state 0, d(s)
 *   the depth of s and final(s) where a phrase ends.  fail(s) is the Aho-Corasick failure link: the state of the longest proper suffix
 *   of s's path that is a trie path.  goto(s, k) is the trie child of s by k if there is one, else the child by k of the first state on
 *   s's failure chain that has one, else the root.  Dictionary (output) links are not followed: a phrase is credited only along the
 *   active path, so a phrase that ends inside a longer match earns nothing by itself.
 *       fa(s)   = the depth of the deepest final proper ancestor of s in the trie, 0 if there is none
 *       held(s) = 0 if final(s), else bonus * (d(s) - fa(s))            what a hypothesis in s loses if its match breaks
 *       gain(s, k) = bonus * (d(s') - fa(s')) - held(s),  s' = goto(s, k)
 *   bonus is one finite number and may be negative.  A hypothesis y_1 .. y_n has state c_0 = 0, c_i = goto(c_{i-1}, y_i) and boost
 *   z_0 = 0, z_i = z_{i-1} + gain(c_{i-1}, y_i), one fp32 addition per token, left to right.
 *   Device form.  ctx_columns [V] int32: 0 for a token in no phrase, else its column 1 .. A.  ctx_next [ctx_states][ctx_width] int32 and
 *   ctx_gain [ctx_states][ctx_width] fp32 with ctx_width = A + 1: entry (s, columns[k]) is goto(s, k) and gain(s, k), gains computed in
 *   float64 and rounded once; column 0 is "any other token": next 0, gain -held(s).  No phrases: one state, one column.  Limits:
 *   1 <= ctx_states <= HALO_CONTEXT_MAX_STATES, ctx_width >= 1, ctx_states * ctx_width < 2^31.  The tables are read, never written; every
 *   column, state and next entry read from memory is clamped into its table before it indexes one.
 *   The search is halo_ctc_prefix_beam's with these changes.  A member carries (c, z) besides pb / pnb; the empty prefix has c = 0,
 *   z = 0.  A stay candidate keeps its member's (c, z) and ranks by logaddexp(pb', pnb') + z.  The extension of j by k has
 *   col = columns[k], c' = next[c_j][col], z' = z_j + gain[c_j][col], pnb' = its CTC mass as above, and ranks by pnb' + z'.  The merge
 *   is unchanged and on CTC mass alone: members that spell the same prefix took the same gains in the same order, so the stay
 *   candidate's (c, z) are the merged extension's.  The W best are taken by (rank descending, candidate position ascending); a candidate
 *   whose CTC mass is -inf is never taken, whatever its boost.  pb / pnb stay CTC masses throughout.
 *   halo_ctc_prefix_beam_biased   halo_ctc_prefix_beam's arguments, workspace rule and outputs, with scores [N][beam] = the rank, CTC
 *                          mass + boost, and boosts [N][beam] fp32 (the boost in that score, 0 where absent: scores - boosts is the CTC
 *                          mass) and states [N][beam] int64 (the automaton state, -1 where absent).  A caller that wants broken
 *                          matches settled at the end of an utterance subtracts held(state) itself.
 *   halo_ctc_prefix_beam_advance_biased  halo_ctc_prefix_beam_advance with the same extra arguments; state
 *                          [N][halo_ctc_prefix_beam_biased_state_bytes(V, beam, capacity)]: halo_ctc_prefix_beam_state_bytes + 128, every
 *                          member's c and z behind the records (zeros are an empty beam here too).  A row with no frames and no begin
 *                          keeps its rows of boosts and states as well.  A stream keeps one automaton from its begin on. */
#define HALO_CONTEXT_MAX_STATES 65535
int halo_ctc_prefix_beam_biased(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int64_t *emission_lengths,
                                int beam, int capacity, void *workspace, int64_t *tokens, int64_t *lengths, float *scores, int64_t *counts,
                                const int *ctx_columns, const int *ctx_next, const float *ctx_gain, int ctx_states, int ctx_width,
                                float *boosts, int64_t *states, halo_stream_t stream);
size_t halo_ctc_prefix_beam_biased_state_bytes(int V, int beam, int capacity);
int halo_ctc_prefix_beam_advance_biased(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int *n_frames,
                                        const int *flags, int beam, int capacity, void *state, int64_t *tokens, int64_t *lengths,
                                        float *scores, int64_t *counts, const int *ctx_columns, const int *ctx_next, const float *ctx_gain,
                                        int ctx_states, int ctx_width, float *boosts, int64_t *states, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CTC prefix beam search with shallow fusion of an LSTM language model (haloop_amd/fusion.py CTCFusionDecoder; csrc/ctc_lm_beam.hip,
 * DESIGN.md 3.3q) as a launch sequence: per frame one halo_ctc_lm_beam_step, one halo_rnnt_lstm_cell per LSTM layer and one
 * halo_decode_linear on all N * beam slots, and one halo_rnnt_beam_keep.  Slot n * beam + r is member r of row n's beam.  The beam's
 * records and the LM state (h and c [layers][N * beam][hidden], g [N * beam][ldg]) exist twice, by frame parity; a step reads one copy
 * and writes the other.
 *   Definition, per row, with e = emissions[:, n] (log-probabilities, class 0 the blank), L = clamp(emission_lengths[n], 0, T),
 *   W = beam, cap = capacity, a = lm_weight, b = insertion_bonus.  A member is (y, pb, pnb, lm, lp, state): pb / pnb the CTC masses of
 *   halo_ctc_prefix_beam, lm the LM's log-probability of y, lp = log_softmax(g + g_bias) over all V classes of the LM after it consumed
 *   the start token and then y, state the LSTM state behind lp.
 *       beam = [((), pb = 0, pnb = -inf, lm = 0, lp and state after one LM step on the start token from the zero state)]
 *       for t in 0 .. L-1:
 *         total_j = logaddexp(pb_j, pnb_j)
 *         candidates, in this order:
 *           for j in beam order: stay (y_j, pb' = total_j + e[t][0], pnb' = pnb_j + e[t][last(y_j)] (-inf for the empty prefix), lm' = lm_j)
 *           for j in beam order, if len(y_j) < cap, for k = 1 .. V-1: extension (y_j + [k], pb' = -inf,
 *               pnb' = e[t][k] + (pb_j if k == last(y_j) else total_j), lm' = lm_j + lp_j[k])
 *         an extension that spells the prefix of a stay candidate s is merged into it: its CTC mass joins pnb'_s (logaddexp), s keeps its
 *           own lm, and the extension is no candidate.  Equality of prefixes is decided by comparing tokens (a hash only shortlists).
 *         beam = the W best candidates by (logaddexp(pb', pnb') + a lm' + b len(y') descending, candidate position ascending: stay j at
 *           j, the extension of j by k at W + j V + k); a candidate whose CTC mass is -inf is never kept.  A kept extension takes one LM
 *           step from its parent's state; a kept stay keeps its parent's lp and state.
 *       result: the beam after frame L-1, best first.  L = 0: the empty hypothesis alone, every score 0.
 *   With a = b = 0 this is halo_ctc_prefix_beam, token for token.
 *   halo_ctc_lm_beam_step  frame `frame` of every row, one workgroup of 256 threads per row.  rec [N][beam][4] fp32 = pb | pnb | lm | the
 *                          ranking value, meta [N][beam][4] int32 = length (-1: no member) | last token (0: the empty prefix) | hash of
 *                          the prefix | hash of the prefix without its last token, tokens [N][beam][tokens_ld] int32; at frame 0 the
 *                          input records are not read.  Outputs: the new beam's records in the order taken, parent (the slot within the
 *                          row it came from; -1: no member) and last (the token appended; 0: a stay), and the gather of
 *                          halo_rnnt_beam_step: xh [layers][N * beam][2 hidden] of every new slot = wte[last] (layer 0's x half) | h_in of
 *                          its parent (the h halves), c_out = c_in of its parent.  A row with frame >= L passes its beam through
 *                          unchanged (parent = own index, last = 0) and loads no emission; frames at or past L, other rows' frames and
 *                          the gaps of a strided view are never loaded.  lp_j[k] = (g[slot j][k] + g_bias[k]) - lse_j with the
 *                          log-sum-exp summed in one fixed order; an extension's ranking value is
 *                          fma(a, lm_j + lp_j[k], pnb') + b (len(y_j) + 1), a stay's fma(a, lm_j, logaddexp(pb', pnb')) + b len(y_j).
 *                          The row's beam * V LM logits are cached in LDS when (beam + 1) V <= 14336 floats and recomputed from L2
 *                          by the same operations otherwise: the same bits.  fp32, no float atomics, bit-reproducible.
 *                          Limits: 2 <= V <= 8192, 1 <= beam <= 16, hidden % 4 == 0, 1 <= capacity <= tokens_ld, 0 <= frame < T. */
int halo_ctc_lm_beam_step(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int *emission_lengths, int frame,
                          int beam, int capacity, float lm_weight, float insertion_bonus, const float *g, long ldg, const float *g_bias,
                          const float *rec_in, const int *meta_in, const int *tokens_in, float *rec_out, int *meta_out, int *tokens_out,
                          long tokens_ld, int *parent, int *last, const float *wte, int hidden, int layers, const float *h_in,
                          const float *c_in, float *xh, float *c_out, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Beam search of the RNN transducer head with shallow fusion of an LSTM language model (haloop_amd/fusion.py TransducerFusionDecoder;
 * csrc/rnnt_lm_beam.hip) as a launch sequence: per alignment step one halo_rnnt_lm_beam_step, then for each of the two
 * networks (the prediction network, Lp layers; the fusion LM, Ll layers) one halo_rnnt_lstm_cell per layer, one halo_decode_linear and
 * one halo_rnnt_beam_keep on all N * beam slots: Lp + Ll + 5 launches.  Slot n * beam + r is hypothesis r of row n.  The beam's records
 * and both states (h and c [layers][N * beam][hidden], logits [N * beam][ld]) exist twice, by step parity; a step reads one copy and
 * writes the other.
 *   Definition, per row, with F = f[n], L = clamp(input_lengths[n], 0, T), W = beam, cap = capacity, a = lm_weight, b =
 *   insertion_bonus.  A member is (y, s, lm, g, pstate, lp, lstate): y the token sequence, s the transducer mass of
 *   halo_rnnt_beam_step, lm the LM's log-probability of y, g the prediction network's logits after the zero prefix and then y, pstate
 *   its state behind g, lp = log_softmax(lg + lg_bias) over all V classes of the fusion LM after it consumed the start token and then
 *   y, lstate the LM's state behind lp.
 *       B = [((), s = 0, lm = 0, g / pstate after one prediction-network step on token 0 from the zero state,
 *             lp / lstate after one LM step on the start token from the zero state)];  finals = []
 *       if L == 0: finals = [((), rank 0, s 0, lm 0)]
 *       for i in 0 .. L + cap - 1, while B is not empty:
 *         t_j = i - len(y_j);  q_j = log_softmax(F[t_j] + g_j)
 *         candidates, in this order:
 *           for j in beam order: blank (y_j, s' = s_j + q_j[0], lm' = lm_j); if t_j + 1 == L it is complete: appended to finals, no
 *               candidate
 *           for j in beam order, if len(y_j) < cap, for k = 1 .. V-1: (y_j + [k], s' = s_j + q_j[k], lm' = lm_j + lp_j[k])
 *         equal token sequences merge into the earliest (masses by logaddexp; the earliest keeps its own lm'), exactly
 *           halo_rnnt_beam_step's merge
 *         rank(candidate) = fma(a, lm', s') + b * len(y')
 *         B = the W best by (rank descending, candidate position ascending: blank of j at j, j extended by k at W + j V + k); a kept
 *           blank keeps its parent's g, pstate, lp, lstate; a kept label takes one step of BOTH networks on k from its parent's states
 *       result: the W best finals by (rank descending, order of completion), kept as halo_rnnt_beam_step keeps its running W best: a
 *         later one displaces the worst kept (lowest rank, the latest among equals) only with a strictly higher rank.
 *   Everything else is halo_rnnt_beam_step's: the log-sum-exp order, hypotheses at the capacity take no label, frames at or past L are
 *   never read, the tie rules.  With a = b = 0 this is halo_rnnt_beam_step, token for token.
 *   halo_rnnt_lm_beam_step  alignment step `step` of every row, one workgroup of 256 threads per row.  rec [N][beam][3] fp32 = s | lm |
 *                           rank, u [N][beam] (symbols emitted; -1: no hypothesis), tokens [N][beam][tokens_ld]; at step 0 the input
 *                           records are not read and the finals are reset.  g [N * beam][ldg] / lg [N * beam][ldlg]: the logits of the
 *                           prediction network / the LM of every slot without their biases (g_bias, lg_bias [V]; may be NULL).  Outputs:
 *                           the new beam's records in the order taken, parent (-1: no hypothesis) and last (0: a blank extension);
 *                           the finals fin_rec [N][beam][3] = rank | s | lm (-inf: none), fin_seq, fin_lengths (-1: none), fin_tokens,
 *                           fin_n as halo_rnnt_beam_step's; the gather of halo_rnnt_beam_step once per network: xh / lm_xh
 *                           [layers][N * beam][2 hidden] of every new slot = wte[last] | h_in of its parent, c_out = c_in of its
 *                           parent, each with its own embedding, hidden size and depth.  *live += 1 for every row whose new beam is not
 *                           empty.  lp_j[k] = (lg[slot j][k] + lg_bias[k]) - lse_j, both log-sum-exps summed in one fixed order.
 *                           LDS rule: the row's beam * V joint logits and beam * V LM logits are both kept in LDS when 2 * beam * V
 *                           <= 14336 floats (56 KiB of dynamic LDS, what a launch gets without the opt-in) and both recomputed from L2
 *                           by the same operations otherwise: the same bits.  fp32, no float atomics, bit-reproducible.
 *                           Limits: 2 <= V <= 8192, 1 <= beam <= 16, hidden % 4 == 0 and lm_hidden % 4 == 0, 1 <= capacity <=
 *                           tokens_ld; both embeddings hold a row for every class. */
int halo_rnnt_lm_beam_step(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                           const float *g_bias, const float *lg, long ldlg, const float *lg_bias, const int *input_lengths, int step,
                           int beam, int capacity, float lm_weight, float insertion_bonus, const float *rec_in, const int *u_in,
                           const int *tokens_in, float *rec_out, int *u_out, int *tokens_out, long tokens_ld, int *parent, int *last,
                           float *fin_rec, int *fin_seq, int *fin_lengths, int *fin_tokens, int *fin_n, const float *wte, int hidden,
                           int layers, const float *h_in, const float *c_in, float *xh, float *c_out, const float *lm_wte, int lm_hidden,
                           int lm_layers, const float *lm_h_in, const float *lm_c_in, float *lm_xh, float *lm_c_out, int *live,
                           halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward operators of the GPT / transformer training step (the autograd graph of ha/attention.py:205-232 as
 * `hal` runs it, ha/attention_loop.py:196-215: loss.backward()).
 *   halo_attention_bwd         gradient of halo_attention_fwd: dq, dk, dv (same row layouts as q, k, v; written, not
 *                              accumulated) from dy, the saved y and lse; delta [N, heads, Tq] is scratch.
 *                              Two sweeps (per query tile, per key tile), no atomics: bitwise reproducible.
 *   halo_layernorm_bwd         dx = dres + d(layer_norm)/dx . dy (dres: the residual-stream gradient, may be NULL),
 *                              dweight, dbias (NULL when the LayerNorm has no bias); workspace per *_workspace_bytes.
 *   halo_gelu_fwd / _bwd       y = gelu(a) keeping the pre-activation; da = dy * gelu'(a); exact != 0 -> erf form
 *   halo_cross_entropy_fwd_lse halo_cross_entropy_fwd that also returns the row log-sum-exp
 *   halo_cross_entropy_bwd     logits <- (softmax(logits) - onehot(target)) * grad[n * grad_stride] in place
 *                              (grad_stride 0: one scalar for all rows; 1: per row); ignored rows -> 0
 *   halo_embed_bwd             dwte[ids] += dx (float atomics; dwte is the tied lm_head gradient buffer),
 *                              dwpe[pos0 + t] (+)= sum_b dx  (either of dwte / dwpe may be NULL) */
int halo_attention_bwd(const float *q, long q_row_stride, long q_batch_stride, const float *k, const float *v,
                       long kv_row_stride, long kv_batch_stride, const float *y, const float *dy, long y_row_stride,
                       long y_batch_stride, const float *lse, float *delta, float *dq, long dq_row_stride,
                       long dq_batch_stride, float *dk, float *dv, long dkv_row_stride, long dkv_batch_stride, int N,
                       int heads, int head_dim, int Tq, int Tk, int causal, const int *key_lengths, float p_drop,
                       uint64_t seed, uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev,
                       halo_stream_t stream);
/* ha/transformer.py:413-430 `attend(q, k, v, mask)` for ANY boolean mask and head dimension (the reference's tests/test_attention.py: head
 * dimension 7, a (T, S) triangle): q [N][heads][T][hd], k / v [N][heads][S][hd] contiguous fp32; mask bytes (non-zero = the key is hidden
 * from the query) addressed as mask[n * stride_n + h * stride_h + t * stride_t + s] (stride 0 = broadcast), NULL = none; y like q;
 * entropy [N][heads][T] = -sum att log(att + 1e-8) (optional).  One wave per query row, exact fp32: the slow, general path; the models run
 * the tiled kernels above through key lengths and the causal flag.  HALO_ENOTSUP when 4 (hd + S) floats exceed the LDS. */
int halo_attention_masked(const float *q, const float *k, const float *v, const unsigned char *mask, long mask_stride_n, long mask_stride_h,
                          long mask_stride_t, float *y, float *entropy, int N, int heads, int T, int S, int head_dim, halo_stream_t stream);
/* halo_attention_fwd_strided (packed rows) / halo_attention_bwd on the matrix-core kernels with row-major bf16 outputs for the Linear
 * layers around the attention (bf16 / bf16x3 modes, head_dim 32 or 64; HALO_ENOTSUP otherwise): the forward writes y in fp32 (the
 * backward's delta needs it) AND as bf16 [rows][ybf_row_stride]; the backward writes dq, dk, dv as bf16 ONLY (one row / batch stride,
 * e.g. the three column blocks of a packed [rows][3C] buffer) -- they are operands of c_attn's two gradient products and nothing else. */
int halo_attention_fwd_bf16(const float *q, long q_row_stride, long q_batch_stride, const float *k, const float *v, long kv_row_stride,
                            long kv_batch_stride, float *y, long y_row_stride, long y_batch_stride, void *y_bf16, long ybf_row_stride,
                            long ybf_batch_stride, float *lse, int N, int heads, int head_dim, int Tq, int Tk, int causal,
                            const int *key_lengths, float p_drop, uint64_t seed, uint32_t stream_id, uint32_t offset,
                            const uint32_t *offset_dev, halo_stream_t stream);
int halo_attention_bwd_bf16(const float *q, long q_row_stride, long q_batch_stride, const float *k, const float *v, long kv_row_stride,
                            long kv_batch_stride, const float *y, const float *dy, long y_row_stride, long y_batch_stride, const float *lse,
                            float *delta, void *dq_bf16, void *dk_bf16, void *dv_bf16, long d_row_stride, long d_batch_stride, int N,
                            int heads, int head_dim, int Tq, int Tk, int causal, const int *key_lengths, float p_drop, uint64_t seed,
                            uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream);
size_t halo_layernorm_bwd_workspace_bytes(int rows, int C);
int halo_layernorm_bwd(const float *dy, const float *x, const float *weight, const float *dres, float *dx,
                       float *dweight, float *dbias, void *workspace, int rows, int C, float eps,
                       halo_stream_t stream);
/* halo_layernorm_bwd that also writes dx as row-major bf16 (dx_bf16 [rows][C]; C % 4 == 0, C <= 2048, 16-byte aligned operands): dx is the
 * output gradient of the Linear below, whose two gradient products read it as bf16 */
int halo_layernorm_bwd_bf16(const float *dy, const float *x, const float *weight, const float *dres, float *dx, void *dx_bf16,
                            float *dweight, float *dbias, void *workspace, int rows, int C, float eps, halo_stream_t stream);
/* ... with the incoming gradient dy as ROW-MAJOR bf16 (round 5: the input-gradient product's bf16 result, halo_gemm_rows); dx_bf16 optional.
 * C % 4 == 0, C <= 2048. */
int halo_layernorm_bwd_b16(const void *dy_bf16, const float *x, const float *weight, const float *dres, float *dx, void *dx_bf16, float *dweight,
                           float *dbias, void *workspace, int rows, int C, float eps, halo_stream_t stream);
int halo_gelu_fwd(const float *a, float *y, size_t n, int exact, halo_stream_t stream);
int halo_gelu_bwd(const float *dy, const float *a, float *da, size_t n, int exact, halo_stream_t stream);
int halo_cross_entropy_fwd_lse(const float *logits, const int64_t *targets, float *loss, float *lse, int rows, int V,
                               long ld, long ignore_index, halo_stream_t stream);
int halo_cross_entropy_bwd(float *logits, const int64_t *targets, const float *lse, const float *grad,
                           long grad_stride, int rows, int V, long ld, long ignore_index, halo_stream_t stream);
int halo_embed_bwd(const int64_t *ids, const float *dx, float *dwte, float *dwpe, int B, int T, int C, int pos0,
                   int vocab, int accumulate_wpe, halo_stream_t stream);
/* The dwte half of halo_embed_bwd without atomics: dwte[v] = the sum, in token order, of the rows dx[n] with ids[n] == v (ids clamped to
 * [0, vocab) as there); every row of dwte [vocab][C] is WRITTEN (rows no token names become 0).  One thread per (v, column) scans the n
 * ids, so the cost is vocab x n id reads: made for the prediction network's small vocabularies and the few thousand tokens of an n-best
 * list (rnn.Decoder.forward_batch_first(..., ordered_grad=True), Transducer.mwer_forward), whose gradients it makes bit-reproducible. */
int halo_embed_bwd_ordered(const int64_t *ids, const float *dx, float *dwte, int n, int C, int vocab, halo_stream_t stream);
/* x[n, :] += p[n % T, :]: tok_emb + pos_emb when both went through StableEmbedding's LayerNorm first (ha/attention.py:30-61,224) */
int halo_add_rows_bcast(float *x, const float *p, int rows, int T, int C, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Convolutional front-end of AudioEncoder, channels-last.  replaces, in ha/conv.py:
 *   halo_im2col_cl    the unfold of nn.Conv1d(input_dim, hidden_dim, 3, stride, padding=1) :29; the conv itself is a
 *                     GEMM of col [N*T', Cin*ks] with weight [Cout, Cin*ks] + bias + HALO_GEMM_GELU_ERF (:46)
 *   halo_dwconv1d_cl  DWConv1d.depthwise (groups = channels) :15-18; .pointwise :19 is a GEMM over the rows
 * x [N, T, C] -> [N, T', C] with T' = (T + 2*pad - ks)/stride + 1; no length masking (the reference has none).  A window wider
 * than the padded input (T + 2*pad < ks) is HALO_EINVAL in all four launches, whatever the stride (nn.Conv1d refuses it too). */
int halo_im2col_cl(const float *x, float *col, int N, int T, int Cin, int ks, int stride, int pad,
                   halo_stream_t stream);
/* gradient of the unfold (the fold): dx [N,T,Cin] from dcol [N*T', Cin*ks]; with it a dense Conv1d whose input is an activation
 * (ha/attention_audio.py:71 conv_subsample) back-propagates as GEMM + halo_col2im_cl */
int halo_col2im_cl(const float *dcol, float *dx, int N, int T, int Cin, int ks, int stride, int pad,
                   halo_stream_t stream);
int halo_dwconv1d_cl(const float *x, const float *weight, const float *bias, float *y, int N, int T, int C, int ks,
                     int stride, int pad, halo_stream_t stream);
/* gradient of halo_dwconv1d_cl: dx [N,T,C] (NULL to skip), dweight [C,ks], dbias [C] (NULL when bias-free); ks <= 8;
 * fixed-order partial sums through the workspace (bitwise reproducible) */
size_t halo_dwconv1d_cl_bwd_workspace_bytes(int C, int ks);
int halo_dwconv1d_cl_bwd(const float *dy, const float *x, const float *weight, float *dx, float *dweight,
                         float *dbias, void *workspace, int N, int T, int C, int ks, int stride, int pad,
                         halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Token-tape batching (the data formats either side of the LM paths).  Integer gathers on
 * HBM-resident tapes, bit-exact.
 *   halo_tape_batch    SymbolTapeNoPad.__getitem__(i)  ha/symbol_tape.py:239-279: out [rows, batch_size] (row-major, same
 *                      element type as the tape: elem_bytes 1/2/4/8), out[t, b] = data[b*(tape_len-1) + i*bptt_len + t] with
 *                      tape_len = ceil(n_tokens / batch_size); positions past the tape get pad_value.  rows = bptt_len, or
 *                      the trailing token count for the last part.
 *   halo_lm_batch_u16  get_batch of ha/attention_loop.py:98-125 on a uint16 tape (np.memmap dtype uint16 :90): x[b, :] =
 *                      data[offsets[b] : offsets[b] + T] as int64, y = x shifted left with a 0 in the last column
 *                      (objective "lm"); objective_cond != 0 keeps only column (#non-zero x) - 2 of y ("cond"). */
int halo_tape_batch(const void *data, int elem_bytes, long n_tokens, int batch_size, int bptt_len, long part_index,
                    int rows, long pad_value, void *out, halo_stream_t stream);
int halo_lm_batch_u16(const uint16_t *data, long n_tokens, const int64_t *offsets, int B, int T, int objective_cond,
                      int64_t *x, int64_t *y, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The masked objectives of the GPT trainer (--objective denoise | cond, ha/attention_loop.py:110-120).
 *
 * Token masking.  replaces: mask_tokens (ha/mlm.py:11-40) and its call in get_batch (ha/attention_loop.py:113-114).  torch's
 * generator cannot be reproduced on the device, so the draws come from the library's counter stream (the policy of the dropout
 * masks).  For the flat position e = b*T + t holding ``token``:
 *     (r0, r1, r2, r3) = philox4x32_10(ctr = (lo32(e), hi32(e), HALO_MLM_STREAM, step), key = (lo32(seed), hi32(seed)))
 *     thr(p)   = min(int(float32(p) * 2^32), 0xFFFFFFFF)
 *     selected = token != endoftext_token and r0 < thr(mlm_probability)
 *     replaced = selected and r1 < thr(0.8)                         -> mask_token
 *     random   = selected and not replaced and r2 < thr(0.5)        -> (uint64(r3) * max_token) >> 32
 *     label    = token where selected, else 0; every other input keeps its token.
 *   halo_mask_tokens    inputs [n] int64 masked in place, labels [n] int64 written.  0 <= p <= 1, 0 < max_token <= 2^32.
 *   halo_mlm_batch_u16  the gather of halo_lm_batch_u16 (x[b, t] = data[offsets[b] + t], 0 past the tape) and the masking in one
 *                       launch: x [B, T] the masked inputs, y [B, T] the labels.  A position past the tape draws like any other.
 *
 * Target rows.  replaces: the work F.cross_entropy(..., ignore_index=0) (ha/attention.py:230-231) and the lm_head spend on rows
 * without a target: the caller runs ln_f, the lm_head and the loss on the compacted rows.  Every shape is set by ``capacity``, none
 * by the count, and no launch uses atomics: the compact order is the ascending row order.
 *   halo_target_rows    targets [M] int64 -> rows [capacity] int32 (the first ``limit`` <= capacity rows with targets[row] != ignore_index,
 *                       ascending; -1 behind them), targets_c [capacity] int64 (their targets; ignore_index behind them), slot [M] int32
 *                       (the inverse map: rows[slot[i]] == i; -1 for a row without a target or past the limit), count [1] int32 (all
 *                       rows with a target, which may exceed limit).  capacity sizes the compact rows (a caller rounds it up to what its
 *                       products need), limit is the number of targets it allowed for.
 *   halo_gather_rows    dst [K, C] fp32: dst[k] = src[rows[k]], a zero row where rows[k] is outside [0, M).  16-byte accesses along C
 *                       when C % 4 == 0.
 *   halo_scatter_rows   dst [M, C] fp32: dst[i] = src[slot[i]] (src [capacity, C]), a zero row where slot[i] is outside [0, capacity):
 *                       every row of dst is written.  dst_bf16 (optional): the same rows as row-major bf16.  count (optional, device):
 *                       when *count > limit every element written is NaN (more targets than the caller allowed for). */
int halo_mask_tokens(int64_t *inputs, int64_t *labels, long n, float mlm_probability, long mask_token, long endoftext_token,
                     long max_token, uint64_t seed, uint32_t step, halo_stream_t stream);
int halo_mlm_batch_u16(const uint16_t *data, long n_tokens, const int64_t *offsets, int B, int T, float mlm_probability,
                       long mask_token, long endoftext_token, long max_token, uint64_t seed, uint32_t step, int64_t *x, int64_t *y,
                       halo_stream_t stream);
int halo_target_rows(const int64_t *targets, int M, long ignore_index, int capacity, int limit, int *rows, int64_t *targets_c,
                     int *slot, int *count, halo_stream_t stream);
int halo_gather_rows(const float *src, const int *rows, int M, int K, int C, float *dst, halo_stream_t stream);
int halo_scatter_rows(const float *src, const int *slot, const int *count, int capacity, int limit, int M, int C, float *dst,
                      void *dst_bf16, halo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step on flat buffers.
 * replaces: clip_grad_norm_ ha/loop.py:184 and torch.optim.AdamW(fused) ha/optim.py:137-139
 *   halo_sumsq: partials[0..HALO_SUMSQ_PARTS) = per-workgroup sums of x^2 (fixed order, so the
 *   norm is bitwise reproducible); halo_clip_coef: norm = sqrt(sum partials[0..count)),
 *   coef[0] = min(1, max_norm / (norm + 1e-6)) as clip_grad_norm_ computes it, coef[1] = 1; when
 *   the norm is not finite both are NaN, and halo_adamw skips the whole update when *grad_scale
 *   is NaN -- the on-device form of the reference's "skip batch" on NaN/Inf loss or gradient norm
 *   (ha/loop.py:167-174,185-189).  coef is a device float[2], norm_out a device float (or NULL).
 *   halo_adamw: torch.optim.AdamW single-tensor arithmetic; grad is multiplied by *grad_scale
 *   (device scalar, may be NULL) before use.  step >= 1 is the 1-based update count.
 * ------------------------------------------------------------------------------------------ */
#define HALO_SUMSQ_PARTS 1024
/* y = alpha*y + beta*x on flat buffers: accumulates micro-batch gradients (loss / accumulate; ha/loop.py:176-181) */
int halo_scale_add(float *y, const float *x, float alpha, float beta, size_t n, halo_stream_t stream);
/* the same with a device guard: when *guard (e.g. this micro-batch's loss) is not finite, x contributes nothing -- the reference
 * skips a micro-batch whose loss is NaN/Inf (ha/loop.py:167-174).  alpha == 0 never reads y (a poisoned sum cannot survive). */
int halo_scale_add_guarded(float *y, const float *x, float alpha, float beta, size_t n, const float *guard,
                           halo_stream_t stream);
/* wire format of the data-parallel gradient all-reduce (optional bf16 buckets, haloop_amd/dp.py): y_bf16[i] = bf16(x[i]);
 * y[i] = float(x_bf16[i]) * scale (scale = 1 / world after an all-reduce SUM) */
int halo_cast_f32_bf16(const float *x, void *y_bf16, size_t n, halo_stream_t stream);
int halo_cast_bf16_f32(const void *x_bf16, float *y, float scale, size_t n, halo_stream_t stream);
int halo_sumsq(const float *x, size_t n, float *partials, halo_stream_t stream);
/* The sharded data-parallel update (ha/attention_loop.py:154 semantics, ZeRO-1 shape; haloop_amd/dp.py): a rank owns a chunk of each
 * reduce-scattered span of the flat buffers.  n <= 8 ranges, each beginning and ending on a multiple of 4 elements.
 *   halo_sumsq_ranges:       partials[0..HALO_SUMSQ_PARTS) of the concatenation of x[begin[k], end[k]) (fixed order).
 *   halo_pack_ranges_bf16:   dst (bf16, contiguous) <- the concatenation of src[begin[k], end[k]) rounded to nearest-even: what a rank
 *                            sends in the all-gather of matrix parameters whose consumers only ever multiply by their bf16 values.
 *   halo_expand_ranges_bf16: the inverse on the gathered buffer.  stage holds `world` records of sum(chunk[k]) bf16 values, rank-major;
 *                            span k of dst begins at begin[k] and consists of `world` chunks of chunk[k] elements; every chunk but
 *                            skip_rank's (the caller's own fp32 master values; -1: none) is overwritten with the gathered values. */
/* Round 5: direct peer exchange for the data-parallel step (csrc/dp_direct.hip; replaces the NCCL collectives
 * DistributedDataParallel issues, ha/attention_loop.py:154,203, with writes over the point-to-point xGMI links).
 *   halo_dx_alloc / open / close / free: an ARENA of device memory peers can write (uncached where the runtime allows) and its 64-byte HIP
 *       IPC handle; a peer maps it with halo_dx_open.  The arena starts zeroed; its first 4096 bytes are flag blocks (64 bytes each).
 *   halo_dx_push:   piece p of src (piece_bytes each, piece_stride_bytes apart; same != 0: src itself for every peer) -> peer p's arena at
 *       dst_offset + rank * piece_bytes, every peer p != rank, one launch.  16-byte granules.
 *   halo_dx_signal: epoch -> word `rank` of the flag block at flag_offset of every peer's arena (system-scope release).
 *   halo_dx_wait:   one workgroup waits until every peer's word of own_flags carries epoch (or later); BOUNDED (5 s): a timeout raises the
 *       status word of halo_set_status_word and returns.
 *   halo_dx_reduce: own [elems] <- scale * (sum in RANK ORDER of own (at position rank) and the inbox pieces p != rank, elems apart).
 * peer_bases: `world` (<= 16) mapped arena pointers, own rank's the local one. */
int halo_dx_alloc(size_t bytes, void **ptr, void *handle64);
int halo_dx_open(const void *handle64, void **ptr);
int halo_dx_close(void *ptr);
int halo_dx_free(void *ptr);
int halo_dx_push(const void *src, size_t piece_bytes, size_t piece_stride_bytes, int same, void *const *peer_bases, size_t dst_offset, int world,
                 int rank, halo_stream_t stream);
int halo_dx_signal(void *const *peer_bases, size_t flag_offset, int world, int rank, uint32_t epoch, halo_stream_t stream);
int halo_dx_wait(const void *own_flags, int world, int rank, uint32_t epoch, halo_stream_t stream);
int halo_dx_reduce(float *own, const float *inbox, size_t elems, int world, int rank, float scale, halo_stream_t stream);

int halo_sumsq_ranges(const float *x, int n, const size_t *begin, const size_t *end, float *partials, halo_stream_t stream);
int halo_pack_ranges_bf16(const float *src, int n, const size_t *begin, const size_t *end, void *dst, halo_stream_t stream);
int halo_expand_ranges_bf16(const void *stage, int n, const size_t *begin, const size_t *chunk, int world, int skip_rank, float *dst,
                            halo_stream_t stream);
int halo_clip_coef(const float *partials, int count, float max_norm, float *coef, float *norm_out,
                   halo_stream_t stream);
/* halo_clip_coef that also advances a device-side update counter (uint32) when the norm is finite: torch's AdamW step count
 * advances only with an applied update (the reference skips optimizer.step() on a non-finite norm, ha/loop.py:185-189).
 * A raised status word (halo_set_status_word) counts as a non-finite norm: the update is skipped on the device. */
int halo_clip_coef_step(const float *partials, int count, float max_norm, float *coef, float *norm_out,
                        uint32_t *applied_steps, halo_stream_t stream);
int halo_adamw(float *p, const float *g, float *m, float *v, size_t n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, const float *grad_scale, halo_stream_t stream);
/* halo_adamw over n_ranges (<= 8) contiguous element ranges [begin[r], end[r]) of the same flat buffers in ONE launch (host
 * arrays; offsets multiples of 4): range r has its own weight_decay[r] and device gradient scale grad_scale[r] (NULL: 1).
 * counter (optional, device): incremented once -- the dropout step counter of halo_counter_inc rides along.
 * A NaN *grad_scale[r] skips range r only (its p, m and v keep their bits; the other ranges are updated).  counter advances by one
 * per launch whether or not any range was applied. */
int halo_adamw_ranges(float *p, const float *g, float *m, float *v, int n_ranges, const size_t *begin, const size_t *end,
                      const float *weight_decay, const float *const *grad_scale, float lr, float beta1, float beta2,
                      float eps, int step, uint32_t *counter, halo_stream_t stream);

/* halo_adamw_ranges with the 1-based update count read from the device (the counter halo_clip_coef_step advances), so that a
 * whole training step -- optimizer included -- has no host-side scalar and replays from one hipGraph. */
/* lr_dev (optional, device float): the learning rate is read from there instead of ``lr`` -- a schedule (the reference applies
 * lr.apply_lr_ every step, ha/loop.py:191) then reaches a captured launch: the caller writes the device scalar between replays. */
int halo_adamw_ranges_dev(float *p, const float *g, float *m, float *v, int n_ranges, const size_t *begin, const size_t *end,
                          const float *weight_decay, const float *const *grad_scale, float lr, const float *lr_dev, float beta1,
                          float beta2, float eps, const uint32_t *step_dev, uint32_t *counter, halo_stream_t stream);

/* halo_adamw over MANY tensors in one launch (what torch.optim.AdamW(fused=True) does for a parameter list, ha/attention_loop.py:
 * 141-147).  tensor_table (device, built once): n_tensors records of halo_adamw_multi_tensor_bytes() bytes each:
 *   { float *p; float *m; float *v; uint64 n; float weight_decay; int32 pad }
 * chunk_table (device, built once): n_chunks pairs { uint32 tensor, uint32 chunk } -- every tensor cut into
 * ceil(n / halo_adamw_multi_chunk()) chunks, one workgroup each.  grads: HOST array of the n_tensors gradient pointers of this
 * step (autograd allocates new ones every backward); they are copied into the kernel arguments, so the caller may reuse the
 * array at once.  n_tensors <= halo_adamw_multi_max_tensors() per call.  lr may change from call to call (LR schedules,
 * ha/optim.py:68-72): the decay factor 1 - lr*weight_decay is formed in the kernel.  Bit-identical to one halo_adamw call per
 * tensor. */
size_t halo_adamw_multi_tensor_bytes(void);
unsigned halo_adamw_multi_chunk(void);
int halo_adamw_multi_max_tensors(void);
int halo_adamw_multi(const void *tensor_table, const void *chunk_table, int n_chunks, const float *const *grads, int n_tensors,
                     float lr, float beta1, float beta2, float eps, int step, const float *grad_scale, halo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HALO_H */
