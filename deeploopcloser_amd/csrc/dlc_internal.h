// Internal helpers shared by the HIP translation units behind include/dlc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>

#include "../../include/dlc.h"

struct dlc_host_staging;                           // pinned staging ring + host copy threads (host_staging.hip)

struct dlc_ctx {
    int device;
    char err[512];
    int profiling;
    long long prof_calls;                       // ring entries (product-kernel launches, dlc::profiled) since profiling was enabled
    hipEvent_t ev_start[DLC_PROFILE_RING];
    hipEvent_t ev_stop[DLC_PROFILE_RING];
    void* scratch;                              // caller-owned split-K scratch (dlc_set_scratch), may be null
    size_t scratch_bytes;
    // hipFuncSetAttribute is per DEVICE and a context is bound to one device: which kernels already
    // have their dynamic-LDS limit raised on this context's device (bit = DLC_ATTR_* id)
    unsigned long long func_attr_set;
    void* zero_page;                            // 4 KiB of zeros in device memory (source of masked LDS-DMA pieces)
    dlc_host_staging* staging;                  // created by the first dlc_host_to_device / dlc_device_to_host
    std::mutex* host_lock;                      // serialises the staged transfers, the ring's creation and its teardown
    int host_threads;                           // host copy threads of the staging (0 = min(16, hardware threads))
    unsigned long long* host_flag;              // 64 page-locked bytes: the one word dlc_sdav_similarity_matrix reads back
    hipEvent_t ev_flag;                         // ... and the event behind its copy
    int prune_mode;                             // DLC_PRUNE_* (dlc_set_prune_mode): dlc_cosine_topk's pruned score pass
    int prune_kept;                             // keep mode: the state below belongs to the last pruned call
    const void* prune_id[3];                    // ... its workspace, queries and database
    long long prune_shape[4];                   // ... and q, n, d / 64, kg
};

#include "dlc_hd.h"                             // dlc::fail, the size and row-limit helpers, dlc_f64_key: HIP-free, shared with the host tests

// ids of the kernels that need hipFuncAttributeMaxDynamicSharedMemorySize (bits of dlc_ctx::func_attr_set)
enum {
    DLC_ATTR_GEMM_BASE = 0,      // + tag (0 bf16, 1 f16) * 8 + mode (0..3) * 2 + maskq   -> bits 0..15
    DLC_ATTR_GEMV_BASE = 16,     // + tag * 3 + {QB 1,2,4 -> 0,1,2}                        -> bits 16..21
    DLC_ATTR_DGEMM_BASE = 24,    // + (fp32 ? 4 : 0) + {KN, NK, conv C%8, conv any -> 0..3}  -> bits 24..31
    DLC_ATTR_DMA64_BASE = 32,    // gemm_dma_f64_kernel: + {KN, NK, conv} + (96-column form ? 3 : 0) + (128-row tile ? 6 : 0) -> bits 32..43
    DLC_ATTR_PAIR_TILE = 48,     // pair_score_tile_kernel
    DLC_ATTR_GRAM_I8 = 49,       // gram_i8_kernel
    DLC_ATTR_PAIR_FILTER = 50,   // pair_score_filter_kernel
    DLC_ATTR_SPLIT_F16 = 51,     // gemm_split_f16_kernel
    DLC_ATTR_DS_DMA = 52,        // distinctive_score_dma_kernel
    DLC_ATTR_CONV_SPLIT_F16 = 53,    // gemm_split_f16_kernel<SP_CONV>
    DLC_ATTR_TRACK_BASE = 54,    // track_resident_kernel: + {fp64, fp32, int64 -> 0, 1, 2} * 2 + (8 columns per thread ? 1 : 0)  -> bits 54..59
};

namespace dlc {

void staging_free(dlc_host_staging* s);

#define DLC_HIP_CHECK(ctx, expr)                                                              \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess)                                                                \
            return dlc::fail((ctx), DLC_ERR_HIP, "%s failed: %s (%s:%d)", #expr,              \
                             hipGetErrorString(e__), __FILE__, __LINE__);                     \
    } while (0)

#define DLC_LAUNCH_CHECK(ctx, what)                                                           \
    do {                                                                                      \
        hipError_t e__ = hipGetLastError();                                                   \
        if (e__ != hipSuccess)                                                                \
            return dlc::fail((ctx), DLC_ERR_HIP, "launch of %s failed: %s", (what),           \
                             hipGetErrorString(e__));                                         \
    } while (0)

// bench.py's kernel-only timing (dlc_set_profiling): one ring entry, a hipEvent pair on the stream around the ONE product
// kernel launch() makes (a split-K reduce or a min / max fold over its output is launched outside it).
template <typename F>
inline int profiled(dlc_ctx* ctx, hipStream_t st, F&& launch) {
    if (!ctx->profiling) return launch();
    const int slot = (int)(ctx->prof_calls % DLC_PROFILE_RING);
    DLC_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start[slot], st));
    const int rc = launch();
    if (rc != DLC_OK) return rc;
    DLC_HIP_CHECK(ctx, hipEventRecord(ctx->ev_stop[slot], st));
    ctx->prof_calls++;
    return DLC_OK;
}

// RAII-free device guard: the C ABI is re-entrant per context and each context
// is bound to one device.
struct DeviceGuard {
    int prev;
    bool ok;
    explicit DeviceGuard(int dev) : prev(-1), ok(true) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace dlc

// An entry point's step onto its context's device, behind its argument checks: the guard lives to the end of the
// enclosing function and puts the caller's device back.
#define DLC_ON_DEVICE(ctx)                                                                    \
    dlc::DeviceGuard guard((ctx)->device);                                                    \
    if (!guard.ok) return dlc::fail((ctx), DLC_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device)

#include "entry.h"                              // dlc::overlap, check_workspace, split_plan, capped_blocks: HIP-free too

// ---- device-side vector types ------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) double f64x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

struct dlc_bf16_tag {};
struct dlc_f16_tag {};

__device__ __forceinline__ float dlc_bf16_bits_to_f32(unsigned short h) {
    return __uint_as_float(((unsigned)h) << 16);
}
__device__ __forceinline__ float dlc_f16_bits_to_f32(unsigned short h) {
    _Float16 v = __builtin_bit_cast(_Float16, h);
    return (float)v;
}

// Ordering key of an fp64 score: quantised to 2^-40 (oracle/cosine.py: order_key), so that two rows whose exact
// scores are equal but whose fp64 sums differ in the last bits (the same products in another order) still tie.
// The integer the whole cosine path ranks by (cosine_topk.hip) and the one cosine_rows.hip writes as rows.
constexpr long long KEY64_EMPTY = (long long)0x8000000000000000ull;
__device__ __forceinline__ long long f64_key(double s) {
    const double x = s * 1099511627776.0;                 // 2^40
    if (!(x > -4.0e18)) return KEY64_EMPTY + 1;           // -inf, NaN, absurdly negative: last
    if (x > 4.0e18) return 0x7fffffffffffffffll;
    return __double2ll_rn(x);                             // round half to even, as np.round
}
