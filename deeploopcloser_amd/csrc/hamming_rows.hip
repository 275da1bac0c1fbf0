// Hamming distance of packed binary descriptors as rows (the comparison of the LDB codes of dlc_ldb_describe_u8, and of
// any bit string): out[r][j] = sum_p popcount(q_r[p] ^ db_j[p]) on bytes, for a batch of Q query rows against the first
// lim(r) of N db rows -- dlc_hamming_rows, the contract of dlc_hamming_rows word for word.
//
// The launch is sad_rows.hip's: one workgroup per (query tile, db tile) below the largest limit of the call, in the three
// tile shapes of distance_tile.h, no split along D, every thread storing its acc[QR][4] once under j < lim(r); one array
// staged per side, rows 20 words apart (16-byte aligned, conflict-free 16-byte reads: the reasoning is in sad_rows.hip)
// and read 16 bytes at a time.  What differs is the inner operation: v_xor and v_bcnt, which takes the accumulate, on
// whole words -- two VALU operations per word pair where v_sad_u8 is one.
// Bytes at and past D read as zero on both sides: popcount(0 ^ 0) = 0.
// Integers throughout (8 * D fits the 32-bit accumulator for D <= 2^24): the result is exact and the same for every plan.
#include "distance_tile.h"

namespace {

constexpr int64_t HR_MAX_GRID_X = 1 << 16;     // db tiles beyond it are walked by the same workgroups (grid stride)
constexpr int HR_PITCH = TK_W + 4;             // words between staged rows: 16-byte aligned, conflict-free 16-byte reads

template <int NTX, int QR>
__global__ __launch_bounds__(256) void hamming_rows_kernel(const uint8_t* __restrict__ queries, long long Q, long long ldq,
                                                       const uint8_t* __restrict__ db, long long N, long long ldd,
                                                       long long D, long long limit0, long long limit_step,
                                                       long long* __restrict__ out, long long ld_out) {
    constexpr int NTY = 256 / NTX, QT = NTY * QR, DB = NTX * 4;
    constexpr int PA = (QT + 63) / 64, PB = DB / 64;     // 16-byte loads per thread and step: 4 threads per row
    __shared__ __attribute__((aligned(16))) unsigned As[QT][HR_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned Bs[DB][HR_PITCH];

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
        unsigned acc[QR][4];
#pragma unroll
        for (int r = 0; r < QR; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0u;
        fetch(0);
        for (long long k0 = 0; k0 < D; k0 += TK_CH) {
            const int lw0 = (tid & 3) * 4;
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const int row = (tid >> 2) + 64 * p;
                if (row < QT) *(u32x4_t*)&As[row][lw0] = va[p];
            }
#pragma unroll
            for (int p = 0; p < PB; ++p) *(u32x4_t*)&Bs[(tid >> 2) + 64 * p][lw0] = vb[p];
            __syncthreads();
            if (k0 + TK_CH < D) fetch(k0 + TK_CH);
#pragma unroll
            for (int w = 0; w < TK_W; w += 4) {
                u32x4_t a[QR], b[4];
#pragma unroll
                for (int r = 0; r < QR; ++r) a[r] = *(const u32x4_t*)&As[ty + NTY * r][w];
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = *(const u32x4_t*)&Bs[tx + NTX * c][w];
#pragma unroll
                for (int r = 0; r < QR; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[r][c] += (unsigned)__popc(a[r][e] ^ b[c][e]);
            }
            __syncthreads();
        }
        // the store addresses are formed behind the loop, as in distance_rows.hip (hoisted they hold registers through it)
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

extern "C" int dlc_hamming_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq, const uint8_t* db,
                               int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step,
                               int64_t* out, int64_t ld_out, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!queries || !db || !out || Q < 1 || N < 1 || D < 1 || ldq < D || ldd < D)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "hamming_rows: bad argument");
    if (ld_out < N) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "hamming_rows: ld_out=%lld < N=%lld", (long long)ld_out, (long long)N);
    if ((((uintptr_t)queries) & 15) || (((uintptr_t)db) & 15) || (ldq & 15) || (ldd & 15))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "hamming_rows: rows must be 16-byte aligned (bases, ldq, ldd)");
    if (((uintptr_t)out) & 7) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "hamming_rows: out must be 8-byte aligned");
    if (D > (1ll << 24)) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "hamming_rows: D too large for 32-bit accumulation (8 * D)");
    if (N > 0xffffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "hamming_rows: N must be below 2^32");
    if (Q > (1ll << 20)) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "hamming_rows: Q must not exceed 2^20");
    const TkPlan p = tk_plan(Q);
    const int64_t qtiles = dlc::cdiv(Q, p.qt());                 // <= 65535 (grid y) for every Q <= 2^20: 16-row tiles end at 2^20 - 16
    // rows any query sees (the limit is linear in the query row: its largest value is at one end)
    const int64_t lmax = dlc::max_row_limit(0, Q - 1, N, limit0, limit_step);
    if (lmax == 0) return DLC_OK;
    dlc::DeviceGuard guard(ctx->device);
    if (!guard.ok) return dlc::fail(ctx, DLC_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
    const int64_t tiles = dlc::cdiv(lmax, p.db());
    const dim3 grid((unsigned)(tiles < HR_MAX_GRID_X ? tiles : HR_MAX_GRID_X), (unsigned)qtiles);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, queries, (long long)Q, (long long)ldq, db,
                           (long long)N, (long long)ldd, (long long)D, (long long)limit0, (long long)limit_step,
                           (long long*)out, (long long)ld_out);
    };
    if (p.ntx == 16) launch(hamming_rows_kernel<16, 4>);
    else if (p.qr == 4) launch(hamming_rows_kernel<64, 4>);
    else launch(hamming_rows_kernel<64, 1>);
    DLC_LAUNCH_CHECK(ctx, "hamming_rows_kernel");
    return DLC_OK;
}
