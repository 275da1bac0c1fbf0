// Multi-descriptor fusion of score rows: dlc_fuse_rows (include/dlc.h holds the definition -- the normalisations, the
// TREE order of every row sum, the rounding).
//
//   A lane owns four consecutive cells of an aligned group, (x0 + x1) + (x2 + x3); a wave owns an aligned chunk of 256
//   columns and folds its lanes by an xor-butterfly over 1, 2, .. 32 (addition commutes, so every lane ends with the
//   chunk's node of the tree); the chunks' nodes go to LDS, padded with -0.0 to a power of two, and are folded in place,
//   neighbour with neighbour, 4096 at a time and then the blocks of 4096 the same way.  Every aligned power-of-two
//   block of columns is a node of TREE, so the bits do not depend on which of these steps a plan cuts the row at.
//
//   ROW:  one workgroup (four waves) per row and ONE launch: per source the row is swept for its statistic(s) (sum,
//         then squared deviations; or min / max), the re-reads served by L2, and once more -- all sources side by
//         side -- to write.
//   SLAB: workgroups cover (row, slab of 4096 columns = 16 chunks, a node of the tree).  Up to three launches: the slabs'
//         sums (or min / max), the slabs' squared deviations, the write; the partials sit in the workspace and every
//         workgroup of the next launch folds its row's partials by the same tree.  No atomics, no memset.
//   Loads and stores are 16 bytes per lane where the cell's address allows it (an 8-byte element whose group starts in
//   the upper half of its 16 bytes goes as 8 + 16 + 8), element by element at a row's limit.
#include "score_rows.h"
#include "lds_tree.h"

// every product and every sum rounded on its own (hipcc contracts a * b + c into an fma otherwise), as NumPy's are
#pragma clang fp contract(off)

namespace {

constexpr int FR_THREADS = 256, FR_WAVES = 4;
constexpr int FR_CHUNK = 256;                  // columns of a wave: 64 lanes x 4 cells
constexpr int FR_SLAB = 4096;                  // columns of a SLAB workgroup: 16 chunks
constexpr int FR_BLOCK = 4096;                 // tree nodes folded in LDS at a time
constexpr int FR_TOP = 2048;                   // blocks of a row: 2^31 / 256 / 4096
// AUTO (docs/LAB.md 25: ROW against SLAB over rows 16 .. 2048 x n 4096 .. 262144): SLAB wins from two slabs of offered
// columns on while there are fewer rows than two per compute unit -- 256 rows yes, 512 no, at every n measured
constexpr int FR_SLAB_MIN_COLS = 2 * FR_SLAB;
constexpr int FR_SLAB_ROWS_PER_CU = 2;

typedef __attribute__((ext_vector_type(2))) unsigned long long u64x2_t;

struct FrArgs {
    const void* src[DLC_MAX_FUSE];
    long long ld[DLC_MAX_FUSE];
    double w[DLC_MAX_FUSE];
    int dt[DLC_MAX_FUSE];
    int lib[DLC_MAX_FUSE];
    double* out;
    double* pa;                                // SLAB partials [m, rows, slabs]: sums, or minima
    double* pb;                                //                                 squared deviations, or maxima
    long long ld_out, limit0, limit_step, n, rows, slabs, items;
    int m;
};

__device__ __forceinline__ double fr_cvt(int dt, unsigned long long bits) {
    if (dt == DLC_F64) return __longlong_as_double((long long)bits);
    return (double)(long long)bits;                                   // round to nearest even; exact below 2^53
}

// The lane's four cells, row[at .. at + 3], of which the first cnt (0..4) are offered: the others are -0.0 and not read.
__device__ __forceinline__ void fr_load4(int dt, const void* row, long long at, int cnt, double (&x)[4]) {
    x[0] = x[1] = x[2] = x[3] = -0.0;
    if (cnt <= 0) return;
    if (dt == DLC_F32) {
        const float* p = (const float*)row + at;
        if (cnt == 4 && !((uintptr_t)p & 15)) {
            const f32x4_t v = *(const f32x4_t*)p;
            x[0] = (double)v[0]; x[1] = (double)v[1]; x[2] = (double)v[2]; x[3] = (double)v[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) x[k] = (double)p[k];
        }
        return;
    }
    const unsigned long long* p = (const unsigned long long*)row + at;
    if (cnt == 4) {
        unsigned long long b0, b1, b2, b3;
        if (!((uintptr_t)p & 15)) {
            const u64x2_t u = *(const u64x2_t*)p, v = *(const u64x2_t*)(p + 2);
            b0 = u[0]; b1 = u[1]; b2 = v[0]; b3 = v[1];
        } else {
            const u64x2_t u = *(const u64x2_t*)(p + 1);
            b0 = p[0]; b1 = u[0]; b2 = u[1]; b3 = p[3];
        }
        x[0] = fr_cvt(dt, b0); x[1] = fr_cvt(dt, b1); x[2] = fr_cvt(dt, b2); x[3] = fr_cvt(dt, b3);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) x[k] = fr_cvt(dt, p[k]);
    }
}

__device__ __forceinline__ void fr_store4(double* p, int cnt, const double (&y)[4]) {
    if (cnt == 4) {
        double2 u, v;
        if (!((uintptr_t)p & 15)) {
            u.x = y[0]; u.y = y[1]; v.x = y[2]; v.y = y[3];
            *(double2*)p = u;
            *(double2*)(p + 2) = v;
        } else {
            u.x = y[1]; u.y = y[2];
            p[0] = y[0];
            *(double2*)(p + 1) = u;
            p[3] = y[3];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) p[k] = y[k];
    }
}

__device__ __forceinline__ int fr_cells(long long lim, long long col) {
    const long long c = lim - col;
    return c < 0 ? 0 : (c > 4 ? 4 : (int)c);
}

// the chunk's node of the tree from the lanes' four values, in every lane
__device__ __forceinline__ double fr_wave_sum(const double (&v)[4]) {
    double s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s = s + __shfl_xor(s, off);
    return s;
}

// TREE of C >= 1 nodes; fill(base, cnt) puts nodes base .. base + cnt - 1 into node[0 .. cnt)
template <class Fill>
__device__ __forceinline__ double fr_tree(long long C, double* node, double* top, Fill fill) {
    const long long nblk = (C + FR_BLOCK - 1) / FR_BLOCK;
    if (nblk == 1) {
        fill(0, (int)C);
        return dlc_lds_tree<FR_THREADS>(node, (int)C);
    }
    for (long long b = 0; b < nblk; ++b) {
        const long long left = C - b * FR_BLOCK;
        const int cnt = left < FR_BLOCK ? (int)left : FR_BLOCK;
        fill(b * FR_BLOCK, cnt);
        const double v = dlc_lds_tree<FR_THREADS>(node, cnt);
        if (threadIdx.x == 0) top[b] = v;
    }
    return dlc_lds_tree<FR_THREADS>(top, (int)nblk);
}

// the order of the numbers, -0.0 below +0.0 (dlc_f64_key); never called with a NaN
__device__ __forceinline__ bool fr_below(double x, double y) { return dlc_f64_key(x) < dlc_f64_key(y); }

// chunks chunk0 .. chunk0 + chunks - 1 of row `row` of source i: TREE of x (SQ: of (x - mean)^2)
template <bool SQ>
__device__ __forceinline__ double fr_chunk_tree(const FrArgs& a, int i, const void* row, long long chunk0, long long chunks,
                                                long long lim, double mean, double* node, double* top) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int dt = a.dt[i];
    return fr_tree(chunks, node, top, [&](long long base, int cnt) {
        for (int k = w; k < cnt; k += FR_WAVES) {
            const long long col = (chunk0 + base + k) * FR_CHUNK + lane * 4;
            const int c = fr_cells(lim, col);
            double x[4];
            fr_load4(dt, row, col, c, x);
            if (SQ) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double d = x[e] - mean;
                    const double d2 = d * d;
                    x[e] = e < c ? d2 : -0.0;
                }
            }
            const double s = fr_wave_sum(x);
            if (lane == 0) node[k] = s;
        }
    });
}

// A running (least, greatest) pair in the order of the numbers; a NaN among what it took makes both NaN.
struct FrRange {
    bool any = false, nan = false;
    double l = 0.0, h = 0.0;
    __device__ __forceinline__ void take(double vl, double vh) {
        if (vl != vl || vh != vh) { nan = true; return; }
        if (!any) { l = vl; h = vh; any = true; return; }
        if (fr_below(vl, l)) l = vl;
        if (fr_below(h, vh)) h = vh;
    }
};

// the threads' ranges folded over the workgroup -> (lo, hi) in every thread.  mm: 3 * FR_WAVES words.
__device__ __forceinline__ void fr_range_fold(FrRange g, double* mm, double& lo, double& hi) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double qnan = __longlong_as_double(ROWS_NAN_BITS);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ol = __shfl_xor(g.l, off), oh = __shfl_xor(g.h, off);
        const int oany = __shfl_xor((int)g.any, off), onan = __shfl_xor((int)g.nan, off);
        if (onan) g.nan = true;
        if (oany) g.take(ol, oh);
    }
    if (lane == 0) {
        mm[2 * w] = g.nan ? qnan : g.l;
        mm[2 * w + 1] = g.nan ? qnan : g.h;
        mm[2 * FR_WAVES + w] = g.any || g.nan ? 1.0 : 0.0;              // (a wave that took nothing has nothing to say)
    }
    __syncthreads();
    FrRange all;
    for (int v = 0; v < FR_WAVES; ++v)
        if (mm[2 * FR_WAVES + v] != 0.0) all.take(mm[2 * v], mm[2 * v + 1]);
    lo = all.nan ? qnan : all.l;
    hi = all.nan ? qnan : all.h;
    __syncthreads();                                                  // (mm is free again)
}

// least and greatest of columns col0 .. col1 - 1 (< lim) of a row
__device__ __forceinline__ void fr_minmax(int dt, const void* row, long long col0, long long col1, double* mm, double& lo, double& hi) {
    FrRange g;
    for (long long col = col0 + (long long)threadIdx.x * 4; col < col1; col += FR_THREADS * 4) {
        const int c = fr_cells(col1, col);
        double x[4];
        fr_load4(dt, row, col, c, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < c) g.take(x[e], x[e]);
    }
    fr_range_fold(g, mm, lo, hi);
}

// the same over partials p[0 .. cnt) / q[0 .. cnt) (the slabs' minima / maxima; NaN: the slab held one)
__device__ __forceinline__ void fr_minmax_partials(const double* p, const double* q, long long cnt, double* mm, double& lo, double& hi) {
    FrRange g;
    for (long long t = threadIdx.x; t < cnt; t += FR_THREADS) g.take(p[t], q[t]);
    fr_range_fold(g, mm, lo, hi);
}

__device__ __forceinline__ const void* fr_row(const FrArgs& a, int i, long long r) {
    return (const char*)a.src[i] + r * a.ld[i] * (a.dt[i] == DLC_F32 ? 4 : 8);
}

// chunks chunk0 .. chunk0 + chunks - 1 of row r written: every source's cell normalised by st[i] = (mean, sd) or (lo, hi)
template <int NORM>
__device__ __forceinline__ void fr_write(const FrArgs& a, long long r, long long chunk0, long long chunks, long long lim,
                                         const double (*st)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (long long k = w; k < chunks; k += FR_WAVES) {
        const long long col = (chunk0 + k) * FR_CHUNK + lane * 4;
        const int c = fr_cells(lim, col);
        if (c == 0) continue;
        double y[4];
        for (int i = 0; i < a.m; ++i) {
            double x[4];
            fr_load4(a.dt[i], fr_row(a, i, r), col, c, x);
            const double wi = a.w[i];
            const bool lib = a.lib[i] != 0;
            const double s0 = NORM == DLC_FUSE_NONE ? 0.0 : st[i][0], s1 = NORM == DLC_FUSE_NONE ? 0.0 : st[i][1];
            const double range = s1 - s0;                             // (MINMAX)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double u;
                if (NORM == DLC_FUSE_NONE) {
                    u = lib ? -x[e] : x[e];
                } else if (NORM == DLC_FUSE_ZSCORE) {
                    const double d = lib ? s0 - x[e] : x[e] - s0;
                    const double z = d / s1;
                    u = (lim < 2 || s1 == 0.0) ? 0.0 : z;
                } else {
                    const double d = lib ? s1 - x[e] : x[e] - s0;
                    const double z = d / range;
                    u = range == 0.0 ? 0.0 : z;
                }
                const double t = wi * u;
                y[e] = i == 0 ? t : y[e] + t;
            }
        }
        fr_store4(a.out + r * a.ld_out + col, c, y);
    }
}

template <int NORM>
__global__ __launch_bounds__(FR_THREADS) void fuse_row_kernel(const FrArgs a) {
    __shared__ double node[FR_BLOCK];
    __shared__ double top[FR_TOP];
    __shared__ double st[DLC_MAX_FUSE][2];
    __shared__ double mm[3 * FR_WAVES];
    for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const long long lim = dlc::row_limit(r, a.n, a.limit0, a.limit_step);
        if (lim == 0) continue;                                       // (the same in every thread)
        const long long chunks = dlc::cdiv(lim, FR_CHUNK);
        if (NORM != DLC_FUSE_NONE) {
            for (int i = 0; i < a.m; ++i) {
                const void* row = fr_row(a, i, r);
                double s0, s1;
                if (NORM == DLC_FUSE_ZSCORE) {
                    s0 = fr_chunk_tree<false>(a, i, row, 0, chunks, lim, 0.0, node, top) / (double)lim;
                    s1 = __builtin_sqrt(fr_chunk_tree<true>(a, i, row, 0, chunks, lim, s0, node, top) / (double)(lim - 1));
                } else {
                    fr_minmax(a.dt[i], row, 0, lim, mm, s0, s1);
                }
                if (threadIdx.x == 0) { st[i][0] = s0; st[i][1] = s1; }
            }
            __syncthreads();
        }
        fr_write<NORM>(a, r, 0, chunks, lim, st);
        __syncthreads();                                              // st is read before the next row writes it
    }
}

// PHASE 0: the slabs' sums (ZSCORE) or minima and maxima (MINMAX) -> pa, pb.  PHASE 1: ZSCORE's squared deviations -> pb.
// PHASE 2: the write.
template <int NORM, int PHASE>
__global__ __launch_bounds__(FR_THREADS) void fuse_slab_kernel(const FrArgs a) {
    __shared__ double node[FR_BLOCK];
    __shared__ double top[FR_TOP];
    __shared__ double st[DLC_MAX_FUSE][2];
    __shared__ double mm[3 * FR_WAVES];
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long r = item / a.slabs, slab = item % a.slabs;
        const long long lim = dlc::row_limit(r, a.n, a.limit0, a.limit_step);
        const long long col0 = slab * FR_SLAB;
        if (col0 >= lim) continue;                                    // (the same in every thread)
        const long long col1 = lim - col0 < FR_SLAB ? lim : col0 + FR_SLAB;
        const long long chunk0 = slab * (FR_SLAB / FR_CHUNK), chunks = dlc::cdiv(col1 - col0, FR_CHUNK);
        const long long slabs_r = dlc::cdiv(lim, FR_SLAB);            // the row's slabs that hold a cell: those with partials
        if (NORM != DLC_FUSE_NONE) {
            for (int i = 0; i < a.m; ++i) {
                const void* row = fr_row(a, i, r);
                const long long part = ((long long)i * a.rows + r) * a.slabs;
                double s0 = 0.0, s1 = 0.0;
                if (NORM == DLC_FUSE_ZSCORE) {
                    if (PHASE == 0) {
                        s0 = fr_chunk_tree<false>(a, i, row, chunk0, chunks, lim, 0.0, node, top);
                    } else {
                        const double* p = a.pa + part;
                        s0 = fr_tree(slabs_r, node, top, [&](long long base, int cnt) {
                            for (int t = threadIdx.x; t < cnt; t += FR_THREADS) node[t] = p[base + t];
                        }) / (double)lim;
                        if (PHASE == 1) {
                            s1 = fr_chunk_tree<true>(a, i, row, chunk0, chunks, lim, s0, node, top);
                        } else {
                            const double* q = a.pb + part;
                            s1 = __builtin_sqrt(fr_tree(slabs_r, node, top, [&](long long base, int cnt) {
                                for (int t = threadIdx.x; t < cnt; t += FR_THREADS) node[t] = q[base + t];
                            }) / (double)(lim - 1));
                        }
                    }
                } else if (PHASE == 0) {
                    fr_minmax(a.dt[i], row, col0, col1, mm, s0, s1);
                } else {
                    fr_minmax_partials(a.pa + part, a.pb + part, slabs_r, mm, s0, s1);
                }
                if (threadIdx.x == 0) {
                    if (PHASE == 2) { st[i][0] = s0; st[i][1] = s1; }
                    else if (PHASE == 1) a.pb[part + slab] = s1;
                    else if (NORM == DLC_FUSE_ZSCORE) a.pa[part + slab] = s0;
                    else { a.pa[part + slab] = s0; a.pb[part + slab] = s1; }
                }
            }
            __syncthreads();
        }
        if (PHASE == 2) {
            fr_write<NORM>(a, r, chunk0, chunks, lim, st);
            __syncthreads();
        }
    }
}

size_t fr_workspace(int64_t rows, int64_t n, int m) {
    if (rows < 1 || n < 1 || n > 0x7fffffffll || m < 1 || m > DLC_MAX_FUSE) return 0;
    const int64_t slabs = dlc::cdiv(n, FR_SLAB);
    if (rows > ((int64_t)1 << 62) / (2 * 8 * DLC_MAX_FUSE * slabs)) return 0;       // (the byte count fits)
    return dlc::align_up((size_t)(2 * 8) * (size_t)m * (size_t)rows * (size_t)slabs, 256);
}

template <int NORM>
int fr_launch(dlc_ctx* ctx, const FrArgs& a, bool slab, hipStream_t st) {
    const long long items = slab ? a.items : a.rows;
    const unsigned blocks = dlc::capped_blocks(items);
    if (!slab) {
        hipLaunchKernelGGL((fuse_row_kernel<NORM>), dim3(blocks), dim3(FR_THREADS), 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "fuse_row_kernel");
        return DLC_OK;
    }
    if (NORM != DLC_FUSE_NONE) {
        hipLaunchKernelGGL((fuse_slab_kernel<NORM, 0>), dim3(blocks), dim3(FR_THREADS), 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "fuse_slab_kernel (partials)");
    }
    if (NORM == DLC_FUSE_ZSCORE) {
        hipLaunchKernelGGL((fuse_slab_kernel<NORM, 1>), dim3(blocks), dim3(FR_THREADS), 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "fuse_slab_kernel (deviations)");
    }
    hipLaunchKernelGGL((fuse_slab_kernel<NORM, 2>), dim3(blocks), dim3(FR_THREADS), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "fuse_slab_kernel (write)");
    return DLC_OK;
}

}  // namespace

extern "C" size_t dlc_fuse_rows_workspace_bytes(int64_t rows, int64_t n, int m) { return fr_workspace(rows, n, m); }

extern "C" int dlc_fuse_rows(dlc_ctx* ctx, int m, const int* dtypes, const void* const* scores, const int64_t* lds,
                             const double* weights, const int* lower_is_better,
                             int64_t rows, int64_t n, int64_t limit0, int64_t limit_step, int norm, int plan,
                             double* out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (m < 1 || m > DLC_MAX_FUSE) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: m=%d outside 1..%d", m, DLC_MAX_FUSE);
    if (!dtypes || !scores || !lds || !weights || !lower_is_better || !out)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: bad argument");
    if (norm != DLC_FUSE_NONE && norm != DLC_FUSE_ZSCORE && norm != DLC_FUSE_MINMAX)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: unknown norm %d", norm);
    if (plan != DLC_FUSE_PLAN_AUTO && plan != DLC_FUSE_PLAN_ROW && plan != DLC_FUSE_PLAN_SLAB)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: unknown plan %d", plan);
    if (((uintptr_t)out) & 7) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: out must be aligned to 8 bytes");
    if (ld_out < n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: ld_out=%lld < n=%lld", (long long)ld_out, (long long)n);
    FrArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < m; ++i) {
        const int rc = rows_check_matrix(ctx, "fuse_rows", dtypes[i], scores[i], lds[i], n);
        if (rc != DLC_OK) return rc;
        if (!(weights[i] - weights[i] == 0.0)) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "fuse_rows: weights[%d] is not finite", i);
        a.src[i] = scores[i]; a.ld[i] = lds[i]; a.w[i] = weights[i]; a.dt[i] = dtypes[i]; a.lib[i] = lower_is_better[i] != 0;
    }
    // the operand's shape, which the sources share, once: on the first of them
    const ScoreRows s0 = {dtypes[0], scores[0], rows, n, lds[0], limit0, limit_step, 0, 0, 0};
    const int rc = rows_check(ctx, "fuse_rows", s0, nullptr, DLC_ERR_BAD_SHAPE);
    if (rc != DLC_OK) return rc;
    const size_t need = fr_workspace(rows, n, m);
    const bool ws_ok = dlc::workspace_ok(workspace, workspace_bytes, need);
    if (plan == DLC_FUSE_PLAN_SLAB && !ws_ok) return dlc::check_workspace(ctx, "fuse_rows", workspace, workspace_bytes, need);
    // columns any row offers (limits are linear in the row, so the largest sits at an end)
    const int64_t cols = dlc::max_row_limit(0, rows - 1, n, limit0, limit_step);
    if (cols == 0) return DLC_OK;
    DLC_ON_DEVICE(ctx);
    bool slab = plan == DLC_FUSE_PLAN_SLAB;
    if (plan == DLC_FUSE_PLAN_AUTO && ws_ok && cols >= FR_SLAB_MIN_COLS) {
        int cus = 0;
        DLC_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        slab = rows < (int64_t)FR_SLAB_ROWS_PER_CU * cus;
    }
    a.out = out; a.ld_out = ld_out; a.limit0 = limit0; a.limit_step = limit_step; a.n = n; a.rows = rows; a.m = m;
    a.slabs = dlc::cdiv(n, FR_SLAB);                                   // (the workspace's layout: of n, not of cols)
    a.items = slab ? rows * a.slabs : rows;
    a.pa = (double*)workspace;
    a.pb = a.pa ? a.pa + (size_t)m * (size_t)rows * (size_t)a.slabs : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (norm == DLC_FUSE_NONE) return fr_launch<DLC_FUSE_NONE>(ctx, a, slab, st);
    if (norm == DLC_FUSE_ZSCORE) return fr_launch<DLC_FUSE_ZSCORE>(ctx, a, slab, st);
    return fr_launch<DLC_FUSE_MINMAX>(ctx, a, slab, st);
}
