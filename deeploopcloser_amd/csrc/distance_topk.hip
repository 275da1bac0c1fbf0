// k-nearest search by the cnn_vtl distance (DistanceCalculator.calculate_distance, src/cnn_vtl/similarity/
// DistanceCalculator.py:4-12: sum_k popcount(|a_k ^ b_k|) on signed int8), fused: no [Q, N] distance matrix.
//
//   scan   one workgroup per (query tile, super-slab of db rows).  It walks the slab's tiles in row order; each tile is
//          the matrix kernel's form (match_ref.hip: x ^ m(x) and s(x) staged per operand word, three VALU instructions
//          per word pair), then the tile's distances are filtered against a per-query running bound -- the key of the
//          k-th best row the slab has produced so far -- and the few that pass are inserted into a sorted per-query
//          list in LDS (a wave per query, the list in its registers while it inserts).  The slab's list goes to the workspace: [Q][G][k] keys.
//   merge  one workgroup per query: the k smallest keys of its G sorted lists.
//
// Key of a (query, row) pair: (distance << 32) | row.  Ascending keys are the required order (distance ascending,
// ties -> the lower row) and every key is distinct, so the result is the same however the rows were split.  An empty
// slot is ~0.  No floating point anywhere: the result is exact.
#include "distance_tile.h"
#include "topk_list.h"

namespace {

constexpr unsigned long long TK_EMPTY = ~0ull;

size_t tk_lds_bytes(const TkPlan& p, int k) {
    return (size_t)p.qt() * (size_t)(k + p.db() + 1) * 8 + (size_t)p.qt() * 4;
}

template <int NTX, int QR>
__global__ __launch_bounds__(256) void distance_topk_scan_kernel(const int8_t* __restrict__ queries, long long Q,
                                                                 long long ldq, const int8_t* __restrict__ db,
                                                                 long long N, long long ldd, long long D,
                                                                 long long limit0, long long limit_step, int k,
                                                                 long long tiles_per_slab,
                                                                 unsigned long long* __restrict__ part) {
    constexpr int NTY = 256 / NTX, QT = NTY * QR, DB = NTX * 4;
    constexpr int PA = (QT + 63) / 64, PB = DB / 64;     // 16-byte loads per thread and step: 4 threads per row
    __shared__ unsigned As[QT][TK_W + 1], Asg[QT][TK_W + 1];
    __shared__ unsigned Bs[DB][TK_W + 1], Bsg[DB][TK_W + 1];
    extern __shared__ __attribute__((aligned(16))) char tk_smem[];
    unsigned long long* list = (unsigned long long*)tk_smem;     // [QT][k] sorted keys of the slab so far
    unsigned long long* surv = list + (size_t)QT * k;            // [QT][DB] keys of this tile that beat the bound
    unsigned long long* bound = surv + (size_t)QT * DB;          // [QT] key of the k-th in the list, ~0 until it is full
    unsigned* scnt = (unsigned*)(bound + QT);                    // [QT] survivors of this tile

    const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
    const long long q0 = (long long)blockIdx.x * QT;
    const long long G = gridDim.y, g = blockIdx.y;
    for (int i = tid; i < QT * k; i += 256) list[i] = TK_EMPTY;
    if (tid < QT) { bound[tid] = TK_EMPTY; scnt[tid] = 0; }

    const long long lmax = tk_tile_limit<QT>(q0, Q, N, limit0, limit_step);
    long long lq[QR];
#pragma unroll
    for (int r = 0; r < QR; ++r) lq[r] = tk_query_limit(q0 + ty + NTY * r, Q, N, limit0, limit_step);
    const long long slab0 = g * tiles_per_slab * DB;
    const long long slab1 = slab0 + tiles_per_slab * DB < lmax ? slab0 + tiles_per_slab * DB : lmax;

    for (long long j0 = slab0; j0 < slab1; j0 += DB) {
        u32x4_t va[PA], vb[PB];
        auto fetch = [&](long long k0) {
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const int row = (tid >> 2) + 64 * p;
                const long long q = q0 + row;
                va[p] = (row < QT && q < Q) ? tk_load16(queries + q * ldq, k0 + (tid & 3) * 16, D) : u32x4_t{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                const long long j = j0 + (tid >> 2) + 64 * p;
                vb[p] = j < slab1 ? tk_load16(db + j * ldd, k0 + (tid & 3) * 16, D) : u32x4_t{0u, 0u, 0u, 0u};
            }
        };
        int acc[QR][4];
#pragma unroll
        for (int r = 0; r < QR; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0;
        fetch(0);
        for (long long k0 = 0; k0 < D; k0 += TK_CH) {
            const int lw0 = (tid & 3) * 4;
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const int row = (tid >> 2) + 64 * p;
                if (row < QT) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned s = (va[p][w] >> 7) & 0x01010101u;
                        As[row][lw0 + w] = va[p][w] ^ ((s << 8) - s);
                        Asg[row][lw0 + w] = s;
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                const int row = (tid >> 2) + 64 * p;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned s = (vb[p][w] >> 7) & 0x01010101u;
                    Bs[row][lw0 + w] = vb[p][w] ^ ((s << 8) - s);
                    Bsg[row][lw0 + w] = s;
                }
            }
            __syncthreads();
            if (k0 + TK_CH < D) fetch(k0 + TK_CH);
#pragma unroll
            for (int w = 0; w < TK_W; ++w) {
                unsigned a[QR], sa[QR], b[4], sb[4];
#pragma unroll
                for (int r = 0; r < QR; ++r) { a[r] = As[ty + NTY * r][w]; sa[r] = Asg[ty + NTY * r][w]; }
#pragma unroll
                for (int c = 0; c < 4; ++c) { b[c] = Bs[tx + NTX * c][w]; sb[c] = Bsg[tx + NTX * c][w]; }
#pragma unroll
                for (int r = 0; r < QR; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] += __popc((a[r] ^ b[c]) + (sa[r] ^ sb[c]));
            }
            __syncthreads();
        }
        // filter: only keys below the query's running bound can enter its list
#pragma unroll
        for (int r = 0; r < QR; ++r) {
            const int ql = ty + NTY * r;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long j = j0 + tx + NTX * c;
                if (j < lq[r]) {
                    const unsigned long long key = ((unsigned long long)(unsigned)acc[r][c] << 32) | (unsigned long long)j;
                    if (key < bound[ql]) surv[(size_t)ql * DB + atomicAdd(&scnt[ql], 1u)] = key;
                }
            }
        }
        __syncthreads();
        // insertion, one wave per query (queries w, w + 4, ...): the list sits in the wave's registers as E[i] = lane i's e0,
        // E[64 + i] = lane i's e1, and inserting x is E'[i] = E[i] < x ? E[i] : (E[i - 1] < x ? x : E[i - 1]) -- a shift
        // by one lane, no serial chain through LDS.  The next tile's first barrier orders it before the next filter.
        const int lane = tid & 63;
        for (int ql = tid >> 6; ql < QT; ql += 4) {
            const unsigned ns = scnt[ql];
            if (ns == 0) continue;
            unsigned long long* L = list + (size_t)ql * k;
            unsigned long long e0 = lane < k ? L[lane] : TK_EMPTY, e1 = lane + 64 < k ? L[lane + 64] : TK_EMPTY;
            const int kl = (k - 1) & 63;
            unsigned long long kth = k <= 64 ? __shfl(e0, kl) : __shfl(e1, kl);
            for (unsigned s = 0; s < ns; ++s) {
                const unsigned long long x = surv[(size_t)ql * DB + s];
                if (x >= kth) continue;
                unsigned long long p0 = __shfl_up(e0, 1), p1 = __shfl_up(e1, 1);
                const unsigned long long last0 = __shfl(e0, 63);
                if (lane == 0) { p0 = 0; p1 = last0; }
                const bool lo0 = lane == 0 || p0 < x;
                e1 = e1 < x ? e1 : (p1 < x ? x : p1);
                e0 = e0 < x ? e0 : (lo0 ? x : p0);
                kth = k <= 64 ? __shfl(e0, kl) : __shfl(e1, kl);
            }
            if (lane < k) L[lane] = e0;
            if (lane + 64 < k) L[lane + 64] = e1;
            if (lane == 0) { scnt[ql] = 0; bound[ql] = kth; }
        }
    }
    __syncthreads();
    for (int i = tid; i < QT * k; i += 256) {
        const long long q = q0 + i / k;
        if (q < Q) part[((size_t)q * G + g) * k + i % k] = list[i];
    }
}

// One workgroup per query: the k smallest keys of its G sorted lists.
__global__ __launch_bounds__(256) void distance_topk_merge_kernel(const unsigned long long* __restrict__ part, int G, int k,
                                                                  long long* __restrict__ out_dist,
                                                                  long long* __restrict__ out_idx) {
    const long long q = blockIdx.x;
    tl_merge_slabs<TlWord>(part + (size_t)q * G * k, G, k, [&](int i, TlWord m) {
        out_dist[q * k + i] = m.is_empty() ? -1 : (long long)(m.v >> 32);
        out_idx[q * k + i] = m.is_empty() ? -1 : (long long)(m.v & 0xffffffffull);
    });
}

}  // namespace

extern "C" size_t dlc_cnnvtl_distance_topk_workspace_bytes(int64_t Q, int64_t N, int64_t D, int k) {
    if (Q < 1 || N < 1 || D < 1 || k < 1 || k > DLC_MAX_K) return 0;
    const TkPlan p = tk_plan(Q);
    const int64_t slabs = dlc::max_slabs(dlc::cdiv(Q, p.qt()), dlc::cdiv(N, p.db()), TL_MAX_SLABS);
    return dlc::align_up((size_t)Q * (size_t)slabs * (size_t)k * 8, 256);
}

extern "C" int dlc_cnnvtl_distance_topk(dlc_ctx* ctx, const int8_t* queries, int64_t Q, int64_t ldq, const int8_t* db,
                                        int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step, int k,
                                        int64_t* out_dist, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!out_dist || !out_idx || !workspace) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "distance_topk: bad argument");
    if (k < 1 || k > DLC_MAX_K) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "distance_topk: k=%d outside 1..%d", k, DLC_MAX_K);
    if (const int rc = tk_operands_check(ctx, "distance_topk", queries, Q, ldq, db, N, ldd, D, 1ll << 28); rc != DLC_OK)
        return rc;
    if (Q > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "distance_topk: Q too large");
    const size_t need = dlc_cnnvtl_distance_topk_workspace_bytes(Q, N, D, k);
    if (workspace_bytes < need)
        return dlc::fail(ctx, DLC_ERR_WORKSPACE, "distance_topk: workspace %zu < %zu bytes", workspace_bytes, need);
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;

    // rows any query sees (the limit is linear in the query row: its largest value is at one end)
    const int64_t lmax = dlc::max_row_limit(0, Q - 1, N, limit0, limit_step);
    const TkPlan p = tk_plan(Q);
    int64_t G = 0;
    if (lmax > 0) {
        const int64_t qtiles = dlc::cdiv(Q, p.qt());
        const dlc::SlabSplit slabs = dlc::split_slabs(qtiles, dlc::cdiv(lmax, p.db()), TL_MAX_SLABS);
        G = slabs.G;
        const size_t lds = tk_lds_bytes(p, k);
        auto launch = [&](auto kern) -> int {
            DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)qtiles, (unsigned)G), dim3(256), lds, st, queries, (long long)Q,
                               (long long)ldq, db, (long long)N, (long long)ldd, (long long)D, (long long)limit0,
                               (long long)limit_step, k, (long long)slabs.tiles_per_slab, (unsigned long long*)workspace);
            DLC_LAUNCH_CHECK(ctx, "distance_topk_scan_kernel");
            return DLC_OK;
        };
        int rc;
        if (p.ntx == 16) rc = launch(distance_topk_scan_kernel<16, 4>);
        else if (p.qr == 4) rc = launch(distance_topk_scan_kernel<64, 4>);
        else rc = launch(distance_topk_scan_kernel<64, 1>);
        if (rc != DLC_OK) return rc;
    }
    hipLaunchKernelGGL(distance_topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, st,
                       (const unsigned long long*)workspace, (int)G, k, (long long*)out_dist, (long long*)out_idx);
    DLC_LAUNCH_CHECK(ctx, "distance_topk_merge_kernel");
    return DLC_OK;
}
