// The helpers of dlc_internal.h that need nothing from the HIP runtime, each written once: the translation units behind
// include/dlc.h get them through dlc_internal.h, the host programs of tests/host_sanitize/ through a stand-in for it, so
// a kernel text compiled as C++ runs on the library's own arithmetic.  No HIP header is included here.  Whoever includes
// this file has defined struct dlc_ctx (with its `char err[]`) and declared __double_as_longlong / __longlong_as_double.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

// DLC_HD: callable from host and device.  DLC_DEVICE_INLINE: a device helper, inlined.  Plain inline functions elsewhere.
#if defined(__HIPCC__)
#define DLC_HD __host__ __device__
#define DLC_DEVICE_INLINE __device__ inline __attribute__((always_inline))
#else
#define DLC_HD
#define DLC_DEVICE_INLINE inline
#endif

namespace dlc {

inline int fail(dlc_ctx* ctx, int status, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return status;
}

DLC_HD inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
DLC_HD inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Columns row r of a selection may see, of n: linear in the row, so over a range of rows the largest sits at one end.
DLC_HD inline __attribute__((always_inline)) int64_t row_limit(int64_t r, int64_t n, int64_t limit0, int64_t limit_step) {
    const int64_t l = limit0 + r * limit_step;
    return l < 0 ? 0 : (l > n ? n : l);
}
// The largest row_limit of rows r_first .. r_last: at one end of the range (host entry points size their launches by it).
inline int64_t max_row_limit(int64_t r_first, int64_t r_last, int64_t n, int64_t limit0, int64_t limit_step) {
    const int64_t la = row_limit(r_first, n, limit0, limit_step), lb = row_limit(r_last, n, limit0, limit_step);
    return la > lb ? la : lb;
}

// A scan's column tiles shared out among G slabs so that row_tiles x G comes to about max_wg workgroups.  max_slabs
// bounds G for every smaller col_tiles too (the split's own G is not monotonic in col_tiles): it sizes the workspace.
struct SlabSplit { int64_t G, tiles_per_slab; };
inline int64_t max_slabs(int64_t row_tiles, int64_t col_tiles, int64_t max_wg) {
    const int64_t cap = cdiv(max_wg, row_tiles);
    return col_tiles < cap ? col_tiles : cap;
}
inline SlabSplit split_slabs(int64_t row_tiles, int64_t col_tiles, int64_t max_wg) {
    const int64_t tps = cdiv(col_tiles, max_slabs(row_tiles, col_tiles, max_wg));
    return {cdiv(col_tiles, tps), tps};
}

}  // namespace dlc

// The AREA RESIZE of include/dlc.h (dlc_seqslam_describe_u8, dlc_ldb_describe_u8), written once: one frame gray [H, W]
// -> the thumbnail T [h, w] as bytes at thumb, T(y, x) = floor((2 sum wy wx gray + H W) / (2 H W)), by a workgroup of
// `threads` threads of which this is thread tid.  Cells go to GROUPS of G lanes, G a power of two (dlc_lane_group): a
// group's lanes walk the cell's source rows G apart and group_sum(v, G) -- the caller's butterfly of shuffles, passed in
// because this header names nothing of HIP -- adds their partial sums, integers, so the order is free.  The trip count
// that holds group_sum is the workgroup's, so all lanes of a wave meet in it.  No barrier here: the caller places one
// between this and its first read of thumb.
template <class GroupSum>
DLC_DEVICE_INLINE void dlc_area_resize(const uint8_t* g, int H_, int W_, int h_, int w_, unsigned char* thumb, int tid,
                                       int threads, int G, GroupSum group_sum) {
    const long long H = H_, W = W_, h = h_, w = w_;
    const int cells = h_ * w_, sub = tid & (G - 1), per = threads / G;
    for (int base = 0; base < cells; base += per) {
        const int cell = base + tid / G;
        unsigned acc = 0u;                                     // <= 255 H W < 2^31
        if (cell < cells) {
            const long long y = cell / w_, x = cell % w_;
            // source rows whose interval [i h, (i + 1) h) meets [y H, (y + 1) H): i0 .. i1 - 1 (columns alike)
            const long long i0 = y * H / h, i1 = ((y + 1) * H + h - 1) / h;
            const long long j0 = x * W / w, j1 = ((x + 1) * W + w - 1) / w;
            for (long long i = i0 + sub; i < i1; i += G) {
                const long long lo = i * h > y * H ? i * h : y * H, hi = (i + 1) * h < (y + 1) * H ? (i + 1) * h : (y + 1) * H;
                const unsigned wy = (unsigned)(hi - lo);       // > 0 inside i0 .. i1 - 1, <= h
                unsigned row = 0u;
                for (long long j = j0; j < j1; ++j) {
                    const long long l2 = j * w > x * W ? j * w : x * W, h2 = (j + 1) * w < (x + 1) * W ? (j + 1) * w : (x + 1) * W;
                    row += (unsigned)(h2 - l2) * g[i * W + j];
                }
                acc += wy * row;
            }
        }
        acc = group_sum(acc, G);
        if (cell < cells && sub == 0) {
            const unsigned long long hw = (unsigned long long)(H * W);
            thumb[cell] = (unsigned char)((2ull * acc + hw) / (2ull * hw));
        }
    }
}
// the power of two at or above v, at most 64 (a wave): the lanes per item of the kernels that hand items to lane groups
inline int dlc_lane_group(int64_t v) {
    int g = 1;
    while (g < 64 && g < v) g <<= 1;
    return g;
}

// Order-preserving 64-bit key of a double (atomicMin / atomicMax on unsigned long long): per-frame minima / maxima of
// the CnnVtl descriptor are folded this way by several kernels (cnnvtl.hip, the convolution epilogue of gemm_dma_f64.hip).
// keys[2 f] = key of the minimum of frame f (initially ~0), keys[2 f + 1] = key of its maximum (initially 0).
DLC_DEVICE_INLINE unsigned long long dlc_f64_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
DLC_DEVICE_INLINE double dlc_f64_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}
