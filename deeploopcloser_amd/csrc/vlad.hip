// Orderless place descriptors: dlc_vlad_assign, dlc_vlad_encode, dlc_kmeans_step (include/dlc.h holds the definition --
// DIST's serial chain, the lowest-index arg-min, the member sums in row order, the TREE over row blocks, the rounding).
//
//   ASSIGN (the hot path, rows x K x H x 3 fp64 operations): a workgroup of 16 x 16 threads owns RT*16 rows and sweeps the
//          words in tiles of WT*16; a thread owns an RT x WT register tile of (row, word) pairs, each pair one serial
//          chain in h.  x and the centroids stream through LDS in chunks of 32 columns, stored column-major (pitch + 2,
//          so the transposing stores spread over the banks) and read as the thread's RT and WT neighbours; the next
//          chunk is fetched into registers while the current one is summed.  Behind a word
//          tile every thread leaves its rows' best (distance, word) in LDS and the row's thread folds the 16 in ascending
//          word order into its running minimum: strict <, so the lowest index keeps a tie.  (RT, WT) = (8, 1) for K <= 16,
//          (4, 2) for K <= 32, else (4, 4).
//   MEMBER SUMS (VLAD residuals; k-means block sums): the accumulator is indexed by a(p), which is dynamic, so it lives in
//          LDS, [K][TW] with one column h per thread, TW = 256 / 128 / 64 / 32 for K <= 32 / 64 / 128 / 256 (64 KiB): a
//          thread walks its item's rows in order and adds into its own column -- no atomics, no bank conflicts.  The
//          accumulators start at -0.0 and x + (-0.0) = x, which IS "start from the first member's term".
//   INTRA NORM: a workgroup per (frame, word), TREE_h(R * R) folded in LDS, 2048 leaves at a time and two levels above.
//   K-MEANS: assign (distances to the workspace), block sums, per-block counts / inertia / changed, and one finishing
//          launch whose thread (k, h) folds its column of block sums in place, neighbour with neighbour, and divides.
#include "dlc_internal.h"
#include "lds_tree.h"

// every difference, product and sum rounded on its own (hipcc contracts a * b + c into an fma otherwise)
#pragma clang fp contract(off)

namespace {

constexpr int VL_THREADS = 256;
constexpr int VL_HC = 32;                      // columns of an LDS chunk of the assignment
constexpr int VL_WALK = 8;                    // rows of a member sum whose loads are issued together
constexpr int VL_ACC = 8192;                   // doubles of LDS accumulators, [K][TW]
constexpr int VL_TREE = 2048;                  // tree nodes folded in LDS at a time
constexpr int VL_TREE_TOP = 512;               // 2048 * 2048 * 512 = 2^31 leaves
constexpr unsigned long long VL_NAN_BITS = 0x7ff8000000000000ull;

struct VlAssignArgs {
    const double* x;
    const double* c;
    int* assign;
    double* dist;                              // may be null
    long long rows, H, ldx, ldc, row_tiles;
    int K;
};

template <int RT, int WT>
__global__ __launch_bounds__(VL_THREADS) void vlad_assign_kernel(const VlAssignArgs a) {
    constexpr int RB = RT * 16, WB = WT * 16, XS = RB + 2, CS = WB + 2;
    constexpr int XL = RB * VL_HC / VL_THREADS, CL = WB * VL_HC / VL_THREADS;    // a thread's elements of a chunk: whole numbers
    __shared__ double xs[VL_HC * XS];          // [column of the chunk][row of the tile]; behind a word tile: the candidates
    __shared__ double cs[VL_HC * CS];          // [column of the chunk][word of the tile]
    __shared__ int cand_k[16 * XS];            // [word column of the thread grid][row of the tile]
    double* cand_d = xs;                       // the same, in the first 16 * XS words of xs
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double xr[XL], cr[CL];                     // the next chunk, on its way from memory
    for (long long tile = blockIdx.x; tile < a.row_tiles; tile += gridDim.x) {
        const long long row0 = tile * RB;
        double best_d = 0.0;
        int best_k = -1;                       // (of row row0 + t, in the threads t < RB)
        for (int k0 = 0; k0 < a.K; k0 += WB) {
            double d[RT][WT];
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < WT; ++j) d[i][j] = 0.0;
            // the chunk at h0: the thread's XL + CL elements of it from memory into registers (element e = t + i * 256)
            auto fetch = [&](long long h0) {
#pragma unroll
                for (int i = 0; i < XL; ++i) {
                    const int e = t + i * VL_THREADS, r = e / VL_HC, hh = e % VL_HC;
                    const long long row = row0 + r, h = h0 + hh;
                    xr[i] = (row < a.rows && h < a.H) ? a.x[row * a.ldx + h] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < CL; ++i) {
                    const int e = t + i * VL_THREADS, w = e / VL_HC, hh = e % VL_HC;
                    const long long k = k0 + w, h = h0 + hh;
                    cr[i] = (k < a.K && h < a.H) ? a.c[k * a.ldc + h] : 0.0;
                }
            };
            fetch(0);
            for (long long h0 = 0; h0 < a.H; h0 += VL_HC) {
                __syncthreads();               // the last chunk, or the candidates, have been read
#pragma unroll
                for (int i = 0; i < XL; ++i) {
                    const int e = t + i * VL_THREADS;
                    xs[(e % VL_HC) * XS + e / VL_HC] = xr[i];
                }
#pragma unroll
                for (int i = 0; i < CL; ++i) {
                    const int e = t + i * VL_THREADS;
                    cs[(e % VL_HC) * CS + e / VL_HC] = cr[i];
                }
                __syncthreads();
                if (h0 + VL_HC < a.H) fetch(h0 + VL_HC);           // in flight while this chunk is summed
                const int hn = a.H - h0 < VL_HC ? (int)(a.H - h0) : VL_HC;
                for (int hh = 0; hh < hn; ++hh) {
                    double xv[RT], cv[WT];
#pragma unroll
                    for (int i = 0; i < RT; ++i) xv[i] = xs[hh * XS + ty * RT + i];
#pragma unroll
                    for (int j = 0; j < WT; ++j) cv[j] = cs[hh * CS + tx * WT + j];
#pragma unroll
                    for (int i = 0; i < RT; ++i)
#pragma unroll
                        for (int j = 0; j < WT; ++j) {
                            const double u = xv[i] - cv[j];
                            const double q = u * u;
                            d[i][j] = d[i][j] + q;
                        }
                }
            }
            __syncthreads();                   // xs has been read: it takes the candidates
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                double cd = 0.0;
                int ck = -1;
#pragma unroll
                for (int j = 0; j < WT; ++j) {
                    const int k = k0 + tx * WT + j;
                    if (k < a.K && d[i][j] == d[i][j] && (ck < 0 || d[i][j] < cd)) { cd = d[i][j]; ck = k; }
                }
                cand_d[tx * XS + ty * RT + i] = cd;
                cand_k[tx * XS + ty * RT + i] = ck;
            }
            __syncthreads();
            if (t < RB) {
                for (int u = 0; u < 16; ++u) {
                    const int ck = cand_k[u * XS + t];
                    const double cd = cand_d[u * XS + t];
                    if (ck >= 0 && (best_k < 0 || cd < best_d)) { best_d = cd; best_k = ck; }
                }
            }
        }
        if (t < RB && row0 + t < a.rows) {
            a.assign[row0 + t] = best_k;
            if (a.dist) a.dist[row0 + t] = best_k < 0 ? __longlong_as_double((long long)VL_NAN_BITS) : best_d;
        }
    }
}

// Member sums of items (group g of `per` consecutive rows, tile of tw columns): out[g][k][h] = the sum over the group's
// rows with assign == k, in row order, of x - c_k (RESIDUAL) or of x.  A word without a member: +0.0 (RESIDUAL), -0.0.
struct VlSumArgs {
    const double* x;
    const double* c;
    const int* assign;
    double* out;
    long long rows, per, groups, H, ldx, ldc, ld_out, htiles, items;
    int K, tw;
};

template <bool RESIDUAL>
__global__ __launch_bounds__(VL_THREADS) void vlad_member_sum_kernel(const VlSumArgs a) {
    __shared__ double acc[VL_ACC];
    __shared__ int member[256];
    const int t = threadIdx.x, tw = a.tw;      // (the workgroup has tw threads)
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long g = item / a.htiles, h = (item % a.htiles) * tw + t;
        const long long r0 = g * a.per, r1 = a.rows - r0 < a.per ? a.rows : r0 + a.per;
        for (int k = 0; k < a.K; ++k) acc[k * tw + t] = -0.0;
        if (RESIDUAL) {
            for (int k = t; k < a.K; k += tw) member[k] = 0;
            __syncthreads();
            for (long long r = r0 + t; r < r1; r += tw) {
                const int k = a.assign[r];
                if (k >= 0 && k < a.K) member[k] = 1;              // (several threads may write the same 1)
            }
        }
        if (h < a.H) {
            for (long long r = r0; r < r1; r += VL_WALK) {         // VL_WALK rows' loads in flight, added in row order
                int kk[VL_WALK];
                double v[VL_WALK];
#pragma unroll
                for (int u = 0; u < VL_WALK; ++u) {
                    const int k = r + u < r1 ? a.assign[r + u] : -1;
                    kk[u] = (k >= 0 && k < a.K) ? k : -1;          // (the same in every thread)
                }
#pragma unroll
                for (int u = 0; u < VL_WALK; ++u) {
                    v[u] = kk[u] >= 0 ? a.x[(r + u) * a.ldx + h] : 0.0;
                    if (RESIDUAL && kk[u] >= 0) v[u] = v[u] - a.c[kk[u] * a.ldc + h];
                }
#pragma unroll
                for (int u = 0; u < VL_WALK; ++u)
                    if (kk[u] >= 0) acc[kk[u] * tw + t] = acc[kk[u] * tw + t] + v[u];
            }
        }
        __syncthreads();
        if (h < a.H) {
            double* o = a.out + g * a.ld_out + h;
            for (int k = 0; k < a.K; ++k) o[(long long)k * a.H] = (RESIDUAL && !member[k]) ? 0.0 : acc[k * tw + t];
        }
        __syncthreads();                       // member is read before the next item clears it
    }
}

// TREE of C >= 1 leaves leaf(0) .. leaf(C - 1), in every thread of a workgroup of VL_THREADS
template <class Leaf>
__device__ __forceinline__ double vl_tree(long long C, double* node, double* mid, double* top, Leaf leaf) {
    const long long nmid = (C + VL_TREE - 1) / VL_TREE;
    const long long ntop = (nmid + VL_TREE - 1) / VL_TREE;
    for (long long T = 0; T < ntop; ++T) {
        const long long mleft = nmid - T * VL_TREE;
        const int mcnt = mleft < VL_TREE ? (int)mleft : VL_TREE;
        for (int m = 0; m < mcnt; ++m) {
            const long long base = (T * VL_TREE + m) * VL_TREE, left = C - base;
            const int cnt = left < VL_TREE ? (int)left : VL_TREE;
            for (int j = threadIdx.x; j < cnt; j += VL_THREADS) node[j] = leaf(base + j);
            const double v = dlc_lds_tree<VL_THREADS>(node, cnt);
            if (nmid == 1) return v;
            if (threadIdx.x == 0) mid[m] = v;
        }
        const double v = dlc_lds_tree<VL_THREADS>(mid, mcnt);
        if (ntop == 1) return v;
        if (threadIdx.x == 0) top[T] = v;
    }
    return dlc_lds_tree<VL_THREADS>(top, (int)ntop);
}

struct VlNormArgs {
    double* out;
    long long items, H, ld_out;
    int K;
};

__global__ __launch_bounds__(VL_THREADS) void vlad_intra_norm_kernel(const VlNormArgs a) {
    __shared__ double node[VL_TREE];
    __shared__ double mid[VL_TREE];
    __shared__ double top[VL_TREE_TOP];
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        double* row = a.out + (item / a.K) * a.ld_out + (item % a.K) * a.H;
        const double s = vl_tree(a.H, node, mid, top, [&](long long j) { const double r = row[j]; return r * r; });
        const double n = __builtin_sqrt(s);                        // (every read of row is behind a barrier by now)
        for (long long h = threadIdx.x; h < a.H; h += VL_THREADS) {
            const double q = row[h] / n;
            row[h] = n == 0.0 ? 0.0 : q;
        }
    }
}

struct VlStepArgs {
    const double* c_in;
    double* c_out;
    const int* prev;                           // may be null
    const int* assign;
    const double* dist;
    double* S;                                 // [nb][K][H] block sums; folded in place
    double* inert;                             // [nb]
    long long* cnt;                            // [nb][K]
    long long* chg;                            // [nb]
    long long* out_counts;
    double* out_inertia;
    long long* out_changed;
    long long rows, nb, H, ldc, ldc_out;
    int K;
};

// item (b, j): j < K -- the members of word j in block b; j == K -- the block's inertia and changed rows
__global__ __launch_bounds__(VL_THREADS) void kmeans_block_stats_kernel(const VlStepArgs a) {
    const long long items = a.nb * (a.K + 1);
    for (long long it = (long long)blockIdx.x * VL_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * VL_THREADS) {
        const long long b = it / (a.K + 1);
        const int j = (int)(it % (a.K + 1));
        const long long r0 = b * DLC_KMEANS_BLOCK, r1 = a.rows - r0 < DLC_KMEANS_BLOCK ? a.rows : r0 + DLC_KMEANS_BLOCK;
        if (j < a.K) {
            long long n = 0;
            for (long long r = r0; r < r1; ++r) n += a.assign[r] == j;
            a.cnt[b * a.K + j] = n;
        } else {
            double s = 0.0;
            long long ch = 0;
            for (long long r = r0; r < r1; ++r) {
                const int k = a.assign[r];
                if (k >= 0) s = s + a.dist[r];
                ch += a.prev ? (a.prev[r] != k) : 1;
            }
            a.inert[b] = s;
            a.chg[b] = ch;
        }
    }
}

// p[0], p[stride], .. p[(nb - 1) * stride] folded in place by TREE (a missing right neighbour is -0.0: nothing to add)
__device__ __forceinline__ double vl_fold_blocks(double* p, long long nb, long long stride) {
    for (long long s = 1; s < nb; s <<= 1)
        for (long long b = 0; b + s < nb; b += 2 * s) p[b * stride] = p[b * stride] + p[(b + s) * stride];
    return p[0];
}

// thread g < K * H: centre (k, h); the next K threads: the counts; the last one: inertia and changed
__global__ __launch_bounds__(VL_THREADS) void kmeans_finish_kernel(const VlStepArgs a) {
    const long long KH = (long long)a.K * a.H, total = KH + a.K + 1;
    for (long long g = (long long)blockIdx.x * VL_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * VL_THREADS) {
        if (g < KH + a.K) {
            const int k = (int)(g < KH ? g / a.H : g - KH);
            long long n = 0;
            for (long long b = 0; b < a.nb; ++b) n += a.cnt[b * a.K + k];
            if (g >= KH) {
                a.out_counts[k] = n;
            } else {
                const long long h = g % a.H;
                if (n > 0) a.c_out[k * a.ldc_out + h] = vl_fold_blocks(a.S + g, a.nb, KH) / (double)n;
                else a.c_out[k * a.ldc_out + h] = a.c_in[k * a.ldc + h];
            }
        } else {
            long long ch = 0;
            for (long long b = 0; b < a.nb; ++b) ch += a.chg[b];
            *a.out_changed = ch;
            *a.out_inertia = vl_fold_blocks(a.inert, a.nb, 1);
        }
    }
}

int vl_tile_width(int K) {
    int tw = VL_THREADS;
    while ((long long)K * tw > VL_ACC) tw >>= 1;
    return tw;
}

// the operands the three entry points share: rows [rows, ldx] and a codebook [K, ldc] of H columns
int vl_check(dlc_ctx* ctx, const char* who, const double* x, int64_t rows, int64_t H, int64_t ldx, const double* c, int K,
             int64_t ldc) {
    if (!x || !c) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: null pointer", who);
    if ((((uintptr_t)x) | ((uintptr_t)c)) & 7) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: operands must be aligned to 8 bytes", who);
    if (rows < 1 || H < 1 || K < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: rows=%lld, H=%lld, K=%d must be >= 1", who,
                                                       (long long)rows, (long long)H, K);
    if (ldx < H || ldc < H) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ldx=%lld or ldc=%lld < H=%lld", who, (long long)ldx,
                                             (long long)ldc, (long long)H);
    if (K > DLC_VLAD_MAX_WORDS || (int64_t)K * H > 0x7fffffffll || rows > 0x7fffffffll)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: K=%d > %d, K * H >= 2^31 or rows=%lld >= 2^31", who, K, DLC_VLAD_MAX_WORDS,
                         (long long)rows);
    return DLC_OK;
}

int vl_assign_launch(dlc_ctx* ctx, const double* x, long long rows, long long H, long long ldx, const double* c, int K,
                     long long ldc, int* assign, double* dist, hipStream_t st) {
    VlAssignArgs a = {x, c, assign, dist, rows, H, ldx, ldc, 0, K};
    if (K <= 16) {
        a.row_tiles = dlc::cdiv(rows, 128);
        hipLaunchKernelGGL((vlad_assign_kernel<8, 1>), dim3(dlc::capped_blocks(a.row_tiles)), dim3(VL_THREADS), 0, st, a);
    } else if (K <= 32) {
        a.row_tiles = dlc::cdiv(rows, 64);
        hipLaunchKernelGGL((vlad_assign_kernel<4, 2>), dim3(dlc::capped_blocks(a.row_tiles)), dim3(VL_THREADS), 0, st, a);
    } else {
        a.row_tiles = dlc::cdiv(rows, 64);
        hipLaunchKernelGGL((vlad_assign_kernel<4, 4>), dim3(dlc::capped_blocks(a.row_tiles)), dim3(VL_THREADS), 0, st, a);
    }
    DLC_LAUNCH_CHECK(ctx, "vlad_assign_kernel");
    return DLC_OK;
}

size_t vl_encode_workspace(int64_t frames, int P, int64_t H, int K) {
    if (frames < 1 || frames > 0x7fffffffll || P < 1 || P > DLC_VLAD_MAX_PATCHES || H < 1 || K < 1 || K > DLC_VLAD_MAX_WORDS ||
        (int64_t)K * H > 0x7fffffffll)
        return 0;
    return dlc::align_up((size_t)frames * (size_t)P * 4, 256);
}

size_t vl_step_workspace(int64_t rows, int64_t H, int K) {
    if (rows < 1 || rows > 0x7fffffffll || H < 1 || K < 1 || K > DLC_VLAD_MAX_WORDS || (int64_t)K * H > 0x7fffffffll) return 0;
    const size_t nb = (size_t)dlc::cdiv(rows, DLC_KMEANS_BLOCK);
    return dlc::align_up(8 * ((size_t)rows + nb * (size_t)K * (size_t)H + nb * ((size_t)K + 2)), 256);
}

}  // namespace

extern "C" int dlc_vlad_assign(dlc_ctx* ctx, const double* x, int64_t rows, int64_t H, int64_t ldx, const double* centroids,
                               int K, int64_t ldc, int32_t* out_assign, double* out_dist, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    const int rc = vl_check(ctx, "vlad_assign", x, rows, H, ldx, centroids, K, ldc);
    if (rc != DLC_OK) return rc;
    if (!out_assign || (((uintptr_t)out_assign) & 3) || (((uintptr_t)out_dist) & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "vlad_assign: out_assign is null or an output is not aligned to its element");
    DLC_ON_DEVICE(ctx);
    return vl_assign_launch(ctx, x, rows, H, ldx, centroids, K, ldc, out_assign, out_dist, (hipStream_t)stream);
}

extern "C" size_t dlc_vlad_encode_workspace_bytes(int64_t frames, int P, int64_t H, int K) {
    return vl_encode_workspace(frames, P, H, K);
}

extern "C" int dlc_vlad_encode(dlc_ctx* ctx, const double* x, int64_t frames, int P, int64_t H, int64_t ldx,
                               const double* centroids, int K, int64_t ldc, int norm, double* out, int64_t ld_out,
                               int32_t* out_assign, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (P < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "vlad_encode: P=%d must be >= 1", P);
    if (P > DLC_VLAD_MAX_PATCHES) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "vlad_encode: P=%d > %d", P, DLC_VLAD_MAX_PATCHES);
    const int rc = vl_check(ctx, "vlad_encode", x, frames, H, ldx, centroids, K, ldc);
    if (rc != DLC_OK) return rc;
    if (norm != DLC_VLAD_NORM_NONE && norm != DLC_VLAD_NORM_INTRA)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "vlad_encode: unknown norm %d", norm);
    if (!out || (((uintptr_t)out) & 7) || (((uintptr_t)out_assign) & 3))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "vlad_encode: out is null or an output is not aligned to its element");
    if (ld_out < (int64_t)K * H)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "vlad_encode: ld_out=%lld < K * H=%lld", (long long)ld_out, (long long)K * H);
    const int rw = dlc::check_workspace(ctx, "vlad_encode", workspace, workspace_bytes, vl_encode_workspace(frames, P, H, K));
    if (rw != DLC_OK) return rw;
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    int* assign = out_assign ? out_assign : (int*)workspace;
    const long long rows = (long long)frames * P;
    const int ra = vl_assign_launch(ctx, x, rows, H, ldx, centroids, K, ldc, assign, nullptr, st);
    if (ra != DLC_OK) return ra;
    VlSumArgs s = {x, centroids, assign, out, rows, P, frames, H, ldx, ldc, ld_out, 0, 0, K, vl_tile_width(K)};
    s.htiles = dlc::cdiv(H, s.tw);
    s.items = frames * s.htiles;
    hipLaunchKernelGGL((vlad_member_sum_kernel<true>), dim3(dlc::capped_blocks(s.items)), dim3(s.tw), 0, st, s);
    DLC_LAUNCH_CHECK(ctx, "vlad_member_sum_kernel (residuals)");
    if (norm == DLC_VLAD_NORM_INTRA) {
        const VlNormArgs n = {out, (long long)frames * K, H, ld_out, K};
        hipLaunchKernelGGL(vlad_intra_norm_kernel, dim3(dlc::capped_blocks(n.items)), dim3(VL_THREADS), 0, st, n);
        DLC_LAUNCH_CHECK(ctx, "vlad_intra_norm_kernel");
    }
    return DLC_OK;
}

extern "C" size_t dlc_kmeans_step_workspace_bytes(int64_t rows, int64_t H, int K) { return vl_step_workspace(rows, H, K); }

extern "C" int dlc_kmeans_step(dlc_ctx* ctx, const double* x, int64_t rows, int64_t H, int64_t ldx, const double* c_in, int K,
                               int64_t ldc, double* c_out, int64_t ldc_out, const int32_t* prev_assign, int32_t* out_assign,
                               int64_t* out_counts, double* out_inertia, int64_t* out_changed, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    const int rc = vl_check(ctx, "kmeans_step", x, rows, H, ldx, c_in, K, ldc);
    if (rc != DLC_OK) return rc;
    if (!c_out || !out_assign || !out_counts || !out_inertia || !out_changed)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "kmeans_step: null pointer");
    if (((((uintptr_t)c_out) | ((uintptr_t)out_counts) | ((uintptr_t)out_inertia) | ((uintptr_t)out_changed)) & 7) ||
        ((((uintptr_t)out_assign) | ((uintptr_t)prev_assign)) & 3))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "kmeans_step: a pointer is not aligned to its element");
    if (ldc_out < H) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "kmeans_step: ldc_out=%lld < H=%lld", (long long)ldc_out, (long long)H);
    if (dlc::overlap(c_in, (size_t)(((int64_t)K - 1) * ldc + H) * 8, c_out, (size_t)(((int64_t)K - 1) * ldc_out + H) * 8))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "kmeans_step: c_out overlaps c_in");
    if (prev_assign && dlc::overlap(prev_assign, (size_t)rows * 4, out_assign, (size_t)rows * 4))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "kmeans_step: out_assign overlaps prev_assign");
    const int rw = dlc::check_workspace(ctx, "kmeans_step", workspace, workspace_bytes, vl_step_workspace(rows, H, K));
    if (rw != DLC_OK) return rw;
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = dlc::cdiv(rows, DLC_KMEANS_BLOCK), KH = (long long)K * H;
    double* dist = (double*)workspace;
    VlStepArgs a;
    memset(&a, 0, sizeof(a));
    a.c_in = c_in; a.c_out = c_out; a.prev = prev_assign; a.assign = out_assign; a.dist = dist;
    a.S = dist + rows; a.inert = a.S + nb * KH; a.cnt = (long long*)(a.inert + nb); a.chg = a.cnt + nb * K;
    a.out_counts = (long long*)out_counts; a.out_inertia = out_inertia; a.out_changed = (long long*)out_changed;
    a.rows = rows; a.nb = nb; a.H = H; a.ldc = ldc; a.ldc_out = ldc_out; a.K = K;
    const int ra = vl_assign_launch(ctx, x, rows, H, ldx, c_in, K, ldc, out_assign, dist, st);
    if (ra != DLC_OK) return ra;
    VlSumArgs s = {x, c_in, out_assign, a.S, rows, DLC_KMEANS_BLOCK, nb, H, ldx, ldc, KH, 0, 0, K, vl_tile_width(K)};
    s.htiles = dlc::cdiv(H, s.tw);
    s.items = nb * s.htiles;
    hipLaunchKernelGGL((vlad_member_sum_kernel<false>), dim3(dlc::capped_blocks(s.items)), dim3(s.tw), 0, st, s);
    DLC_LAUNCH_CHECK(ctx, "vlad_member_sum_kernel (block sums)");
    hipLaunchKernelGGL(kmeans_block_stats_kernel, dim3(dlc::capped_blocks(dlc::cdiv(nb * (K + 1), VL_THREADS))), dim3(VL_THREADS), 0,
                       st, a);
    DLC_LAUNCH_CHECK(ctx, "kmeans_block_stats_kernel");
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(dlc::capped_blocks(dlc::cdiv(KH + K + 1, VL_THREADS))), dim3(VL_THREADS), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "kmeans_finish_kernel");
    return DLC_OK;
}
