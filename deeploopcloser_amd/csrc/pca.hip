// PCA projection of place descriptors: dlc_pca_project (include/dlc.h holds the definition -- the centred t_d, the
// serial chain within a chunk of DLC_PCA_CHUNK columns of x, the serial sum of the chunks, the scale).
//
//   PARTIAL SUMS (both plans, one kernel): a workgroup of 256 threads owns a tile of RT rows x 256 * CT components; a
//          thread owns the RT x CT outputs of the components c0 + t + 256 * u, each one serial chain in d within a chunk.
//          The centred rows are formed once per (row, d) and staged in LDS in slabs of 128 columns, [d][row of the tile]:
//          every thread reads the same RT values (a broadcast, RT / 2 16-byte reads per d).  The basis streams from
//          memory, thread t next to thread t + 1 along c, eight d in flight per thread.  Rows and components past the
//          edge are clamped to the last valid one (computed twice, stored once): no operand is read outside [rows, D] or
//          [D, M].  (RT, CT) = (2, 1) for rows <= 2, else (8, 1), or (8, 2) under ONE_PASS with rows > 2 and M > 256.
//   ONE_PASS: the workgroup walks every chunk, y = s_0, y = y + s_j, and stores y * scale.  Tiles are numbered row tile
//          first: the workgroups in flight share their basis columns.
//   SPLIT:  a workgroup takes one (tile, chunk) and stores s_j to the workspace [rows][chunks][M]; the finish kernel's
//          thread (row, c) adds its chunks in order and applies the scale.  No atomics.
#include "dlc_internal.h"

// every difference, product and sum rounded on its own (hipcc contracts a * b + c into an fma otherwise)
#pragma clang fp contract(off)

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_SLAB = 128;                   // columns of x of an LDS slab (divides DLC_PCA_CHUNK)
constexpr int PC_FLIGHT = 8;                   // basis rows a thread loads before it sums them
constexpr long long PC_FILL = 256;             // AUTO: ONE_PASS once it has this many workgroups (one per CU)

struct PcArgs {
    const double* x;
    const double* mean;                        // may be null
    const void* basis;
    const double* scale;                       // may be null
    double* out;
    double* part;                              // SPLIT: [rows][chunks][M]
    long long rows, D, ldx, ldb, ld_out, chunks, row_tiles, col_tiles, items;
    int M;
};

template <typename BT, int RT, int CT, bool SPLIT>
__global__ __launch_bounds__(PC_THREADS) void pca_partial_kernel(const PcArgs a) {
    __shared__ double ts[PC_SLAB * RT];        // [column of the slab][row of the tile]
    const int t = threadIdx.x;
    const BT* basis = (const BT*)a.basis;
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long tile = item % (a.row_tiles * a.col_tiles), row0 = (tile % a.row_tiles) * RT;
        const int c0 = (int)(tile / a.row_tiles) * (PC_THREADS * CT);
        const long long j0 = SPLIT ? item / (a.row_tiles * a.col_tiles) : 0, j1 = SPLIT ? j0 + 1 : a.chunks;
        int cc[CT];                            // the thread's components, clamped
#pragma unroll
        for (int u = 0; u < CT; ++u) cc[u] = c0 + t + u * PC_THREADS < a.M ? c0 + t + u * PC_THREADS : a.M - 1;
        double y[RT][CT];
        for (long long j = j0; j < j1; ++j) {
            double s[RT][CT];
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int u = 0; u < CT; ++u) s[r][u] = 0.0;
            const long long d0 = j * DLC_PCA_CHUNK, d1 = a.D - d0 < DLC_PCA_CHUNK ? a.D : d0 + DLC_PCA_CHUNK;
            for (long long ds = d0; ds < d1; ds += PC_SLAB) {
                const int n = d1 - ds < PC_SLAB ? (int)(d1 - ds) : PC_SLAB;
                __syncthreads();               // the last slab has been read
                for (int e = t; e < PC_SLAB * RT; e += PC_THREADS) {
                    const int r = e / PC_SLAB, dd = e % PC_SLAB;
                    if (dd < n) {
                        const long long row = row0 + r < a.rows ? row0 + r : a.rows - 1;
                        const double xv = a.x[row * a.ldx + ds + dd];
                        ts[dd * RT + r] = a.mean ? xv - a.mean[ds + dd] : xv;
                    }
                }
                __syncthreads();
                const BT* bp = basis + ds * a.ldb;
                int dd = 0;
                for (; dd + PC_FLIGHT <= n; dd += PC_FLIGHT) {
                    double bv[PC_FLIGHT][CT];
#pragma unroll
                    for (int f = 0; f < PC_FLIGHT; ++f)
#pragma unroll
                        for (int u = 0; u < CT; ++u) bv[f][u] = (double)bp[(dd + f) * a.ldb + cc[u]];
#pragma unroll
                    for (int f = 0; f < PC_FLIGHT; ++f)
#pragma unroll
                        for (int r = 0; r < RT; ++r) {
                            const double tv = ts[(dd + f) * RT + r];
#pragma unroll
                            for (int u = 0; u < CT; ++u) {
                                const double q = tv * bv[f][u];
                                s[r][u] = s[r][u] + q;
                            }
                        }
                }
                for (; dd < n; ++dd) {
                    double bv[CT];
#pragma unroll
                    for (int u = 0; u < CT; ++u) bv[u] = (double)bp[dd * a.ldb + cc[u]];
#pragma unroll
                    for (int r = 0; r < RT; ++r) {
                        const double tv = ts[dd * RT + r];
#pragma unroll
                        for (int u = 0; u < CT; ++u) {
                            const double q = tv * bv[u];
                            s[r][u] = s[r][u] + q;
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int u = 0; u < CT; ++u) {
                    if (SPLIT) {
                        if (row0 + r < a.rows && c0 + t + u * PC_THREADS < a.M)
                            a.part[((row0 + r) * a.chunks + j) * a.M + cc[u]] = s[r][u];
                    } else {
                        y[r][u] = j == 0 ? s[r][u] : y[r][u] + s[r][u];
                    }
                }
        }
        if (!SPLIT) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int u = 0; u < CT; ++u)
                    if (row0 + r < a.rows && c0 + t + u * PC_THREADS < a.M)
                        a.out[(row0 + r) * a.ld_out + cc[u]] = a.scale ? y[r][u] * a.scale[cc[u]] : y[r][u];
        }
    }
}

// thread (row, c): y = s_0; y = y + s_j in chunk order; out = y * scale
__global__ __launch_bounds__(PC_THREADS) void pca_finish_kernel(const PcArgs a) {
    const long long total = a.rows * a.M;
    for (long long g = (long long)blockIdx.x * PC_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * PC_THREADS) {
        const long long row = g / a.M;
        const int c = (int)(g % a.M);
        const double* p = a.part + row * a.chunks * a.M + c;
        double y = p[0];
        for (long long j = 1; j < a.chunks; ++j) y = y + p[j * a.M];
        a.out[row * a.ld_out + c] = a.scale ? y * a.scale[c] : y;
    }
}

bool pc_shape_ok(int64_t rows, int64_t D, int M) {
    return rows >= 1 && D >= 1 && M >= 1 && M <= DLC_PCA_MAX_COMPONENTS && rows <= 0x7fffffffll && D <= 0x7fffffffll;
}

// the plan a call runs: DLC_PCA_PLAN_ONE_PASS or DLC_PCA_PLAN_SPLIT; -1 for a plan that is unknown or not allowed
int pc_plan(int64_t rows, int64_t D, int M, int plan) {
    const long long tiles = dlc::cdiv(rows, rows <= 2 ? 2 : 8) * dlc::cdiv(M, rows > 2 && M > 256 ? 512 : 256);
    return dlc::split_plan(plan, rows, DLC_PCA_SPLIT_MAX_ROWS, D > DLC_PCA_CHUNK && tiles < PC_FILL);
}

size_t pc_workspace(int64_t rows, int64_t D, int M, int plan) {
    if (!pc_shape_ok(rows, D, M) || pc_plan(rows, D, M, plan) != DLC_PCA_PLAN_SPLIT) return 0;
    return dlc::align_up((size_t)rows * (size_t)dlc::cdiv(D, DLC_PCA_CHUNK) * (size_t)M * 8, 256);
}

template <typename BT>
int pc_launch(dlc_ctx* ctx, PcArgs a, bool split, hipStream_t st) {
    const int rt = a.rows <= 2 ? 2 : 8, ct = (!split && rt == 8 && a.M > PC_THREADS) ? 2 : 1;
    a.row_tiles = dlc::cdiv(a.rows, rt);
    a.col_tiles = dlc::cdiv(a.M, PC_THREADS * ct);
    a.items = a.row_tiles * a.col_tiles * (split ? a.chunks : 1);
    const dim3 grid(dlc::capped_blocks(a.items)), block(PC_THREADS);
    if (split) {
        if (rt == 2) hipLaunchKernelGGL((pca_partial_kernel<BT, 2, 1, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((pca_partial_kernel<BT, 8, 1, true>), grid, block, 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "pca_partial_kernel (split)");
        hipLaunchKernelGGL(pca_finish_kernel, dim3(dlc::capped_blocks(dlc::cdiv(a.rows * a.M, PC_THREADS))), block, 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "pca_finish_kernel");
    } else {
        if (rt == 2) hipLaunchKernelGGL((pca_partial_kernel<BT, 2, 1, false>), grid, block, 0, st, a);
        else if (ct == 1) hipLaunchKernelGGL((pca_partial_kernel<BT, 8, 1, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((pca_partial_kernel<BT, 8, 2, false>), grid, block, 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "pca_partial_kernel (one pass)");
    }
    return DLC_OK;
}

}  // namespace

extern "C" size_t dlc_pca_project_workspace_bytes(int64_t rows, int64_t D, int M, int plan) {
    return pc_workspace(rows, D, M, plan);
}

extern "C" int dlc_pca_project(dlc_ctx* ctx, const double* x, int64_t rows, int64_t D, int64_t ldx, const double* mean,
                               int basis_dtype, const void* basis, int M, int64_t ldb, const double* scale, double* out,
                               int64_t ld_out, int plan, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!x || !basis || !out) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: null pointer");
    if (basis_dtype != DLC_F64 && basis_dtype != DLC_F32)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: basis dtype %d is neither DLC_F64 nor DLC_F32", basis_dtype);
    const size_t be = basis_dtype == DLC_F64 ? 8 : 4;
    if (((((uintptr_t)x) | ((uintptr_t)mean) | ((uintptr_t)scale) | ((uintptr_t)out)) & 7) || (((uintptr_t)basis) & (be - 1)))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: a pointer is not aligned to its element");
    if (rows < 1 || D < 1 || M < 1)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: rows=%lld, D=%lld, M=%d must be >= 1", (long long)rows, (long long)D, M);
    if (ldx < D || ldb < M || ld_out < M)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: ldx=%lld < D=%lld, or ldb=%lld or ld_out=%lld < M=%d", (long long)ldx,
                         (long long)D, (long long)ldb, (long long)ld_out, M);
    if (plan != DLC_PCA_PLAN_AUTO && plan != DLC_PCA_PLAN_ONE_PASS && plan != DLC_PCA_PLAN_SPLIT)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: unknown plan %d", plan);
    if (!pc_shape_ok(rows, D, M))
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "pca_project: M=%d > %d, rows=%lld or D=%lld >= 2^31", M, DLC_PCA_MAX_COMPONENTS,
                         (long long)rows, (long long)D);
    const int run = pc_plan(rows, D, M, plan);
    if (run < 0)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "pca_project: DLC_PCA_PLAN_SPLIT takes at most %d rows, not %lld",
                         DLC_PCA_SPLIT_MAX_ROWS, (long long)rows);
    const size_t out_bytes = (size_t)((rows - 1) * ld_out + M) * 8;
    if (dlc::overlap(out, out_bytes, x, (size_t)((rows - 1) * ldx + D) * 8) || dlc::overlap(out, out_bytes, mean, (size_t)D * 8) ||
        dlc::overlap(out, out_bytes, basis, (size_t)((D - 1) * ldb + M) * be) || dlc::overlap(out, out_bytes, scale, (size_t)M * 8))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pca_project: out overlaps an input");
    const bool split = run == DLC_PCA_PLAN_SPLIT;
    const size_t need = pc_workspace(rows, D, M, run);
    if (split) {
        const int rc = dlc::check_workspace(ctx, "pca_project", workspace, workspace_bytes, need);
        if (rc != DLC_OK) return rc;
    }
    DLC_ON_DEVICE(ctx);
    PcArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.mean = mean; a.basis = basis; a.scale = scale; a.out = out; a.part = split ? (double*)workspace : nullptr;
    a.rows = rows; a.D = D; a.ldx = ldx; a.ldb = ldb; a.ld_out = ld_out; a.chunks = dlc::cdiv(D, DLC_PCA_CHUNK); a.M = M;
    return basis_dtype == DLC_F64 ? pc_launch<double>(ctx, a, split, (hipStream_t)stream)
                                  : pc_launch<float>(ctx, a, split, (hipStream_t)stream);
}
