// Two exact measures on UNSIGNED bytes as rows: out[r][j] = sum over the words of op(q_r, db_j), for a batch of Q query rows
// against the first lim(r) of N db rows -- the contract of dlc_cnnvtl_distance_rows word for word.
//   dlc_sad_u8_rows   SeqSLAM's image difference (Milford & Wyeth, ICRA 2012, III-A: the sum of absolute differences of
//                     two patch-normalised thumbnails), sum_p |q_r[p] - db_j[p]|: v_sad_u8 takes four byte differences
//                     and the accumulate in one VALU instruction on the bytes as they are.
//   dlc_hamming_rows  the Hamming distance of packed binary descriptors (the LDB codes of dlc_ldb_describe_u8, and any
//                     bit string), sum_p popcount(q_r[p] ^ db_j[p]): v_xor and v_bcnt, which takes the accumulate, on
//                     whole words -- two VALU operations per word pair.
//
// One workgroup per (query tile, db tile) below the largest limit of the call, in the three tile shapes of
// distance_tile.h, no split along D, every thread storing its acc[QR][4] once under j < lim(r) (tk_store_rows).  Against
// the cnn_vtl rows (distance_rows.hip) a tile is staged once (no sign-split second array: half the LDS) and a word pair
// costs one or two operations where the popcount distance spends four.  With so few operations per pair the 4-byte LDS
// reads of that kernel would bind (8 ds_read_b32 = 16 LDS cycles per wave against 16 VALU operations = 32 cycles per
// SIMD, and four SIMDs share the LDS), so rows are staged 20 words apart -- 16-byte aligned, and 20 tx mod 64 takes 16
// distinct 4-bank slots over any 16 lanes with distinct tx mod 16, which is what the lane groups of ds_read_b128 are --
// and read and written 16 bytes at a time: 8 reads = 32 LDS cycles per wave for 64 word pairs.
// Bytes at and past D read as zero on both sides: |0 - 0| = 0 and popcount(0 ^ 0) = 0.
// Integers throughout (255 * D and 8 * D fit the 32-bit accumulator for D <= 2^24): the result is exact and the same for
// every plan.
#include "distance_tile.h"

namespace {

constexpr int UR_PITCH = TK_W + 4;             // words between staged rows: 16-byte aligned, conflict-free 16-byte reads

// The word-pair operations: acc plus the measure of the words a and b.
struct SadOp {
    static __device__ __forceinline__ unsigned apply(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }
};
struct HammingOp {
    static __device__ __forceinline__ unsigned apply(unsigned a, unsigned b, unsigned acc) { return acc + (unsigned)__popc(a ^ b); }
};

template <int NTX, int QR, typename Op>
__global__ __launch_bounds__(256) void u8_rows_kernel(const uint8_t* __restrict__ queries, long long Q, long long ldq,
                                                      const uint8_t* __restrict__ db, long long N, long long ldd,
                                                      long long D, long long limit0, long long limit_step,
                                                      long long* __restrict__ out, long long ld_out) {
    constexpr int NTY = 256 / NTX, QT = NTY * QR, DB = NTX * 4;
    constexpr int PA = (QT + 63) / 64, PB = DB / 64;     // 16-byte loads per thread and step: 4 threads per row
    __shared__ __attribute__((aligned(16))) unsigned As[QT][UR_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned Bs[DB][UR_PITCH];

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
                        for (int e = 0; e < 4; ++e) acc[r][c] = Op::apply(a[r][e], b[c][e], acc[r][c]);
            }
            __syncthreads();
        }
        tk_store_rows<NTX>(acc, lq, q0, j0, tx, ty, out, ld_out);
    }
}

}  // namespace

extern "C" int dlc_sad_u8_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq, const uint8_t* db,
                               int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step,
                               int64_t* out, int64_t ld_out, void* stream) {
    return tk_rows_call(ctx, "sad_u8_rows", "u8_rows_kernel<SadOp>", 1ll << 24, queries, Q, ldq, db, N, ldd, D, limit0, limit_step,
                        out, ld_out, stream, [](auto s) { return u8_rows_kernel<s.ntx, s.qr, SadOp>; });
}

extern "C" int dlc_hamming_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq, const uint8_t* db,
                                int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step,
                                int64_t* out, int64_t ld_out, void* stream) {
    return tk_rows_call(ctx, "hamming_rows", "u8_rows_kernel<HammingOp>", 1ll << 24, queries, Q, ldq, db, N, ldd, D, limit0,
                        limit_step, out, ld_out, stream, [](auto s) { return u8_rows_kernel<s.ntx, s.qr, HammingOp>; });
}
