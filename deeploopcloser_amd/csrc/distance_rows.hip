// Rectangular cnn_vtl distance rows (DistanceCalculator.calculate_distance, src/cnn_vtl/similarity/
// DistanceCalculator.py:4-12: sum_k popcount(|a_k ^ b_k|) on signed int8): out[r][j] for a batch of Q query rows against
// the first lim(r) of N db rows -- what a streaming caller needs to run the sequence search (sequence.hip) on this
// measure without the (N + Q)^2 matrix of everything.
//
// One workgroup per (query tile, db tile) below the largest limit of the call, in the top-k scan's three tile shapes
// (distance_tile.h); where the scan filters a tile's distances into its lists, this kernel stores them.  No split along
// D, so no zeroed output and no atomics: every thread stores its acc[QR][4] once, guarded by j < lim(r) (tk_store_rows).
// Integers throughout: the result is exact and the same for every plan.
#include "distance_tile.h"

namespace {

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
    const long long lmax = tk_tile_limit<QT>(q0, Q, N, limit0, limit_step);
    long long lq[QR];
#pragma unroll
    for (int r = 0; r < QR; ++r) lq[r] = tk_query_limit(q0 + ty + NTY * r, Q, N, limit0, limit_step);
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
        tk_store_rows<NTX>(acc, lq, q0, j0, tx, ty, out, ld_out);
    }
}

}  // namespace

extern "C" int dlc_cnnvtl_distance_rows(dlc_ctx* ctx, const int8_t* queries, int64_t Q, int64_t ldq, const int8_t* db,
                                        int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step,
                                        int64_t* out, int64_t ld_out, void* stream) {
    return tk_rows_call(ctx, "distance_rows", "distance_rows_kernel", 1ll << 28, queries, Q, ldq, db, N, ldd, D, limit0,
                        limit_step, out, ld_out, stream, [](auto s) { return distance_rows_kernel<s.ntx, s.qr>; });
}
