// ABI bookkeeping: version, error strings, device probe.
#include <string.h>
#include <new>
#include <atomic>
#include "halo_common.h"
#include "halo_internal.h"

static HaloCtx g_default_ctx;
static thread_local HaloCtx *t_ctx = nullptr;
HaloCtx &halo_ctx_cur() { return t_ctx ? *t_ctx : g_default_ctx; }

// per-device facts, indexed by the HIP device ordinal (relaxed atomics: racing host threads write the same value)
namespace {
constexpr int MAX_DEVICES = 64;
std::atomic<int> g_cus[MAX_DEVICES];
int cur_device() {
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAX_DEVICES) ? dev : -1;
}
}  // namespace
int halo_cu_count() {
    const int dev = cur_device();
    if (dev < 0) return -1;
    int n = g_cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : -1;
        g_cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
int halo_lstm_fusion() { return halo_ctx_cur().lstm_fusion; }
// the scratch is cut in two halves so that work forked onto a side stream (slot 1) never shares
// split-K slabs with the main stream (slot 0)
void halo_set_scratch_slot(int slot) { halo_ctx_cur().scratch_slot = slot ? 1 : 0; }
void halo_get_scratch(void **ptr, size_t *bytes) {
    const HaloCtx &c = halo_ctx_cur();
    const size_t half = (c.scratch_bytes / 2) & ~(size_t)255;
    *ptr = c.scratch ? (char *)c.scratch + (size_t)c.scratch_slot * half : nullptr;
    *bytes = c.scratch ? half : 0;
}

// side stream + events for fork/join inside one C-ABI call (created once, on first use, outside capture)
static hipStream_t g_side_stream = nullptr;
static hipEvent_t g_fork_event = nullptr, g_join_event = nullptr;
int halo_side_stream(hipStream_t *side, hipEvent_t *fork_ev, hipEvent_t *join_ev) {
    if (!g_side_stream) {
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);      // lo = least urgent
        if (hipStreamCreateWithPriority(&g_side_stream, hipStreamNonBlocking, lo) != hipSuccess) return HALO_ELAUNCH;
        if (hipEventCreateWithFlags(&g_fork_event, hipEventDisableTiming) != hipSuccess) return HALO_ELAUNCH;
        if (hipEventCreateWithFlags(&g_join_event, hipEventDisableTiming) != hipSuccess) return HALO_ELAUNCH;
    }
    *side = g_side_stream; *fork_ev = g_fork_event; *join_ev = g_join_event;
    return HALO_OK;
}
int halo_math_mode() { return halo_ctx_cur().math_mode; }

// ---- known-size read kernels for calibrating the FETCH_SIZE counter per access width (halo_debug_read; tools/pmc_calibrate.py) ----
namespace {
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
// pattern 0: 16 B per lane, a wave instruction reads 1 KiB contiguous (global_load_dwordx4)
// pattern 1:  4 B per lane, a wave instruction reads 256 B contiguous (global_load_dword)
// pattern 2:  4 B per lane, 16-lane groups read 64 B each in four rows `row_bytes` apart (the recurrences' saved-activation loads)
// pattern 3: 16 B per lane through a buffer resource with sc1 (the recurrences' fragment loads)
template <int PATTERN>
__global__ __launch_bounds__(256) void debug_read_kernel(const char *__restrict__ src, size_t bytes, size_t row_bytes, float *sink) {
    unsigned acc = 0;
    const size_t tid = blockIdx.x * (size_t)256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    if (PATTERN == 0) {
        for (size_t i = tid; i < bytes / 16; i += nthreads) { const u32x4_t v = reinterpret_cast<const u32x4_t *>(src)[i]; acc += v[0] ^ v[1] ^ v[2] ^ v[3]; }
    } else if (PATTERN == 1) {
        for (size_t i = tid; i < bytes / 4; i += nthreads) acc += reinterpret_cast<const unsigned *>(src)[i];
    } else if (PATTERN == 2) {
        // the buffer as [rows][row_bytes]; a wave covers 4 rows x 64 B per instruction and walks along the rows, then to the next 4 rows
        const size_t rows = bytes / row_bytes, segs = row_bytes / 64, wave = tid >> 6, nwaves = nthreads >> 6;
        const int lane = threadIdx.x & 63, r = lane >> 4, c = lane & 15;
        for (size_t u = wave; u < (rows / 4) * segs; u += nwaves) {
            const size_t rb = (u / segs) * 4, sg = u % segs;
            acc += *reinterpret_cast<const unsigned *>(src + (rb + r) * row_bytes + sg * 64 + c * 4);
        }
    } else {
        // 2 GiB windows through a buffer resource
        for (size_t base = 0; base < bytes; base += ((size_t)1 << 30)) {
            const size_t len = bytes - base < ((size_t)1 << 30) ? bytes - base : ((size_t)1 << 30);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(src + base), 0, 0x7fffffff, 0x00020000);
            for (size_t i = tid; i < len / 16; i += nthreads) {
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(i * 16), 0, 16);
                acc += v[0] ^ v[1] ^ v[2] ^ v[3];
            }
        }
    }
    if (acc == 0x9e3779b9u) *sink = 1.f;          // (keeps the loads alive)
}
}  // namespace

extern "C" {

int halo_set_math_mode(int mode) {
    if (mode != HALO_MATH_F32 && mode != HALO_MATH_BF16X3 && mode != HALO_MATH_BF16) return HALO_EINVAL;
    halo_ctx_cur().math_mode = mode;
    return HALO_OK;
}
int halo_get_math_mode(void) { return halo_ctx_cur().math_mode; }

int halo_set_lstm_fusion(int on) {
    halo_ctx_cur().lstm_fusion = on ? 1 : 0;
    return HALO_OK;
}

int halo_set_scratch(void *device_ptr, size_t bytes) {
    if (device_ptr && ((uintptr_t)device_ptr % 16 != 0)) return HALO_EINVAL;
    halo_ctx_cur().scratch = device_ptr;
    halo_ctx_cur().scratch_bytes = device_ptr ? bytes : 0;
    return HALO_OK;
}

halo_ctx *halo_ctx_create(void) { return reinterpret_cast<halo_ctx *>(new (std::nothrow) HaloCtx(halo_ctx_cur())); }
void halo_ctx_destroy(halo_ctx *ctx) {
    HaloCtx *c = reinterpret_cast<HaloCtx *>(ctx);
    if (t_ctx == c) t_ctx = nullptr;
    delete c;
}
int halo_ctx_use(halo_ctx *ctx) {
    t_ctx = reinterpret_cast<HaloCtx *>(ctx);
    return HALO_OK;
}
int halo_set_status_word(uint32_t *device_word) {
    if (device_word && ((uintptr_t)device_word % 4 != 0)) return HALO_EINVAL;
    halo_ctx_cur().status = device_word;
    return HALO_OK;
}

int halo_debug_read(const void *src, size_t bytes, int pattern, size_t row_bytes, float *sink, void *stream) {
    if (!src || !sink || bytes < 65536 || bytes % 16 || pattern < 0 || pattern > 3) return HALO_EINVAL;
    if (pattern == 2 && (row_bytes < 64 || row_bytes % 64 || bytes % (4 * row_bytes))) return HALO_EINVAL;
    const dim3 grid(256 * 8), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (pattern) {
        case 0: hipLaunchKernelGGL(debug_read_kernel<0>, grid, block, 0, st, (const char *)src, bytes, row_bytes, sink); break;
        case 1: hipLaunchKernelGGL(debug_read_kernel<1>, grid, block, 0, st, (const char *)src, bytes, row_bytes, sink); break;
        case 2: hipLaunchKernelGGL(debug_read_kernel<2>, grid, block, 0, st, (const char *)src, bytes, row_bytes, sink); break;
        default: hipLaunchKernelGGL(debug_read_kernel<3>, grid, block, 0, st, (const char *)src, bytes, row_bytes, sink); break;
    }
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_ELAUNCH;
}

int halo_abi_version(void) { return HALO_ABI_VERSION; }

const char *halo_strerror(int code) {
    switch (code) {
        case HALO_OK: return "ok";
        case HALO_EINVAL: return "invalid argument";
        case HALO_ENOTSUP: return "shape not supported by the gfx950 kernels";
        case HALO_ELAUNCH: return "HIP launch failed";
        default: return "unknown halo error";
    }
}

int halo_device_info(int device, char *arch, int arch_len, int *cu_count) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HALO_ELAUNCH;
    if (arch && arch_len > 0) {
        strncpy(arch, prop.gcnArchName, (size_t)arch_len - 1);
        arch[arch_len - 1] = 0;
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    return HALO_OK;
}

}  // extern "C"
