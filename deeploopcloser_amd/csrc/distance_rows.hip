// Rectangular cnn_vtl distance rows (DistanceCalculator.calculate_distance, src/cnn_vtl/similarity/
// DistanceCalculator.py:4-12: sum_k popcount(|a_k ^ b_k|) on signed int8): out[r][j] for a batch of Q query rows against
// the first lim(r) of N db rows -- what a streaming caller needs to run the sequence search (sequence.hip) on this
// measure without the (N + Q)^2 matrix of everything.
//
// One workgroup per (query tile, db tile) below the largest limit of the call, in the top-k scan's three tile shapes
// (distance_tile.h); where the scan filters a tile's distances into its lists, this kernel stores them.  No split along
// D, so no zeroed output and no atomics: every thread stores its acc[QR][4] once, guarded by j < lim(r) -- everything
// else of `out` keeps its value.  Threads consecutive in tx write consecutive columns (coalesced 8-byte stores).
// Integers throughout: the result is exact and the same for every plan.
#include "distance_tile.h"

namespace {

constexpr int64_t DR_MAX_GRID_X = 1 << 16;     // db tiles beyond it are walked by the same workgroups (grid stride)

template <int NTX, int QR>
__global__ __launch_bounds__(256) void distance_rows_kernel(const int8_t* __restrict__ queries, long long Q, long long ldq,
                                                            const int8_t* __restrict__ db, long long N, long long ldd,
                                                            long long D, long long limit0, long long limit_step,
                                                            long long* __restrict__ out, long long ld_out) {
    constexpr int NTY = 256 / NTX, QT = NTY * QR, DB = NTX * 4;
    constexpr int PA = (QT + 63) / 64, PB = DB / 64;     // 16-byte loads per thread and step: 4 threads per row
    __shared__ unsigned As[QT][TK_W + 1], Asg[QT][TK_W + 1];
    __shared__ unsigned Bs[DB][TK_W + 1], Bsg[DB][TK_W + 1];

    const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
    const long long q0 = (long long)blockIdx.y * QT;
    // rows this tile's queries may see: limits are linear in the query row, so the largest sits at an end
    const long long qlast = (q0 + QT < Q ? q0 + QT : Q) - 1;
    const long long la = dlc::row_limit(q0, N, limit0, limit_step), lb = dlc::row_limit(qlast, N, limit0, limit_step);
    const long long lmax = la > lb ? la : lb;
    long long lq[QR];
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const long long q = q0 + ty + NTY * r;
        lq[r] = q < Q ? dlc::row_limit(q, N, limit0, limit_step) : 0;
    }
    for (long long j0 = (long long)blockIdx.x * DB; j0 < lmax; j0 += (long long)gridDim.x * DB) {
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
                vb[p] = j < lmax ? tk_load16(db + j * ldd, k0 + (tid & 3) * 16, D) : u32x4_t{0u, 0u, 0u, 0u};
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
        // the store addresses are formed here, behind the loop: hoisted above it (they do not depend on it) they would
        // hold 32 registers through it -- 176 instead of 134 in the 64 x 64 shape, a wave per SIMD less
        int sx = tx, sy = ty;
        asm volatile("" : "+v"(sx), "+v"(sy));
#pragma unroll
        for (int r = 0; r < QR; ++r) {
            const long long q = q0 + sy + NTY * r;                 // (lq[r] = 0 where q >= Q: nothing is stored there)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long j = j0 + sx + NTX * c;
                if (j < lq[r]) out[q * ld_out + j] = (long long)acc[r][c];
            }
        }
    }
}

}  // namespace

extern "C" int dlc_cnnvtl_distance_rows(dlc_ctx* ctx, const int8_t* queries, int64_t Q, int64_t ldq, const int8_t* db,
                                        int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step,
                                        int64_t* out, int64_t ld_out, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!queries || !db || !out || Q < 1 || N < 1 || D < 1 || ldq < D || ldd < D)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "distance_rows: bad argument");
    if (ld_out < N) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "distance_rows: ld_out=%lld < N=%lld", (long long)ld_out, (long long)N);
    if ((((uintptr_t)queries) & 15) || (((uintptr_t)db) & 15) || (ldq & 15) || (ldd & 15))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "distance_rows: rows must be 16-byte aligned (bases, ldq, ldd)");
    if (((uintptr_t)out) & 7) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "distance_rows: out must be 8-byte aligned");
    if (D > (1ll << 28)) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "distance_rows: D too large for int32 accumulation");
    if (N > 0xffffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "distance_rows: N must be below 2^32");
    const TkPlan p = tk_plan(Q);
    const int64_t qtiles = dlc::cdiv(Q, p.qt());
    if (qtiles > 65535) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "distance_rows: Q must not exceed 2^20");
    // rows any query sees (the limit is linear in the query row: its largest value is at one end)
    const int64_t lmax = dlc::max_row_limit(0, Q - 1, N, limit0, limit_step);
    if (lmax == 0) return DLC_OK;
    dlc::DeviceGuard guard(ctx->device);
    if (!guard.ok) return dlc::fail(ctx, DLC_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
    const int64_t tiles = dlc::cdiv(lmax, p.db());
    const dim3 grid((unsigned)(tiles < DR_MAX_GRID_X ? tiles : DR_MAX_GRID_X), (unsigned)qtiles);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, queries, (long long)Q, (long long)ldq, db,
                           (long long)N, (long long)ldd, (long long)D, (long long)limit0, (long long)limit_step,
                           (long long*)out, (long long)ld_out);
    };
    if (p.ntx == 16) launch(distance_rows_kernel<16, 4>);
    else if (p.qr == 4) launch(distance_rows_kernel<64, 4>);
    else launch(distance_rows_kernel<64, 1>);
    DLC_LAUNCH_CHECK(ctx, "distance_rows_kernel");
    return DLC_OK;
}
