// What the two cnn_vtl distance kernels over (query tile x db tile) share: distance_topk.hip (the fused k-nearest scan)
// and distance_rows.hip (the rectangular distance rows) -- and sad_rows.hip, the same rows for SeqSLAM's sum of absolute
// differences on unsigned bytes.  The tile shapes and the masked 16-byte load.
#pragma once
#include "gemm_internal.h"

namespace {

constexpr int TK_CH = 64;                  // descriptor bytes per step (16 words)
constexpr int TK_W = TK_CH / 4;

// The three tile shapes (NTX threads across db rows, 256 / NTX across queries; QR queries x 4 db rows per thread).
struct TkPlan {
    int ntx, qr;
    int qt() const { return (256 / ntx) * qr; }   // queries per tile
    int db() const { return ntx * 4; }            // db rows per tile
};

// Few queries get a tall tile (every thread's 4 db rows against the same one or four queries: the query operand is an
// LDS broadcast); many get the matrix kernel's 64 x 64.  Ties in padded work go to the larger query tile (fewer passes
// over the db).
inline TkPlan tk_plan(int64_t Q) {
    if (Q <= 4) return {64, 1};
    const int64_t big = dlc::cdiv(Q, 64) * 64, mid = dlc::cdiv(Q, 16) * 16;
    return big <= mid ? TkPlan{16, 4} : TkPlan{64, 4};
}

// 16 bytes of a row at byte k (a multiple of 16) as four words; bytes at and past D read as zero (the row's padding may
// hold anything).  A 16-byte aligned block that holds byte k < D lies inside the row's allocation.
__device__ __forceinline__ u32x4_t tk_load16(const int8_t* row, long long k, long long D) {
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (k < D) {
        v = *(const u32x4_t*)(row + k);
        const long long left = D - k;
        if (left < 16) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const long long lw = left - 4 * w;
                const unsigned mask = lw >= 4 ? 0xffffffffu : (lw <= 0 ? 0u : ((1u << (8 * (int)lw)) - 1u));
                v[w] &= mask;
            }
        }
    }
    return v;
}
// The same block of a row of unsigned bytes (sad_rows.hip): the words are the same, only the operand's type differs.
__device__ __forceinline__ u32x4_t tk_load16(const uint8_t* row, long long k, long long D) {
    return tk_load16((const int8_t*)row, k, D);
}

}  // namespace
