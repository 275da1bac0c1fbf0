// What the byte-row distance kernels share: one workgroup per (query tile, db tile) of int64 rows out[r][j], j < lim(r) --
// distance_rows.hip (the cnn_vtl distance on int8), u8_rows.hip (SeqSLAM's SAD and the Hamming distance on uint8),
// sad_shift_rows.hip (SAD under lateral shifts) and distance_topk.hip (the fused k-nearest scan, which filters a tile's
// distances where the others store them).  Here, each once: the tile shapes, the masked 16-byte load, the row limits of a
// tile, the guarded store, and the host side of a row call (the argument checks and the launch).
// NOT here: the int8 fetch / sign-split stage / accumulate loop, which distance_rows.hip and distance_topk.hip both spell
// out (they differ in the db bound of the fetch, lmax and slab1).  As functions of this header the compiler forms other
// code from it (an accumulating v_bcnt chain in place of v_add3 trees, other register counts); the one form that kept
// every kernel's waves per SIMD ran the 100 000 x 2243 rows 0.3 .. 11 % faster and the one-query top-k scan 2.3 % slower.
#pragma once
#include "gemm_internal.h"

namespace {

constexpr int TK_CH = 64;                  // descriptor bytes per step (16 words)
constexpr int TK_W = TK_CH / 4;
constexpr int64_t TK_MAX_GRID_X = 1 << 16; // db tiles beyond it are walked by the same workgroups (grid stride)

// The three tile shapes (NTX threads across db rows, 256 / NTX across queries; QR queries x 4 db rows per thread).
struct TkPlan {
    int ntx, qr;
    int qt() const { return (256 / ntx) * qr; }   // queries per tile
    int db() const { return ntx * 4; }            // db rows per tile
};
// A shape as a type: what a launch instantiates its kernel by.
template <int NTX, int QR>
struct TkShape { static constexpr int ntx = NTX, qr = QR; };

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
// The same block of a row of unsigned bytes: the words are the same, only the operand's type differs.
__device__ __forceinline__ u32x4_t tk_load16(const uint8_t* row, long long k, long long D) {
    return tk_load16((const int8_t*)row, k, D);
}

// The row limits of a tile, which every kernel forms in front of its tiles' loop as
//     const long long lmax = tk_tile_limit<QT>(q0, Q, N, limit0, limit_step);
//     long long lq[QR];
//     for (int r = 0; r < QR; ++r) lq[r] = tk_query_limit(q0 + ty + NTY * r, Q, N, limit0, limit_step);
// (the loop over r stays in the kernel: inside a function here the compiler no longer sinks the limits of a workgroup
// with nothing to do behind that test, and the four-query kernels come out differently).
// The db rows that any of the QT queries from q0 on may see: limits are linear in the query row, so the largest sits at an end.
template <int QT>
__device__ __forceinline__ long long tk_tile_limit(long long q0, long long Q, long long N, long long limit0,
                                                   long long limit_step) {
    const long long qlast = (q0 + QT < Q ? q0 + QT : Q) - 1;
    const long long la = dlc::row_limit(q0, N, limit0, limit_step), lb = dlc::row_limit(qlast, N, limit0, limit_step);
    return la > lb ? la : lb;
}
// The db rows that query q sees: none where it is past Q, so that nothing is stored or listed for it.
__device__ __forceinline__ long long tk_query_limit(long long q, long long Q, long long N, long long limit0,
                                                    long long limit_step) {
    return q < Q ? dlc::row_limit(q, N, limit0, limit_step) : 0;
}

// tx and ty as the compiler must take them where a tile's loop has ended: the store addresses formed from these are
// formed there.  Hoisted above the loop (they do not depend on it) they would hold 32 registers through it -- 176 instead
// of 134 in the 64 x 64 shape of the cnn_vtl rows, a wave per SIMD less.
__device__ __forceinline__ void tk_behind_loop(int& sx, int& sy) {
    asm volatile("" : "+v"(sx), "+v"(sy));
}

// A thread's acc[QR][4] of the tile at (q0, j0) into out, each cell under j < lim(r): everything else of `out` keeps its
// value.  Threads consecutive in tx write consecutive columns (coalesced 8-byte stores).
template <int NTX, int QR, typename T>
__device__ __forceinline__ void tk_store_rows(const T (&acc)[QR][4], const long long (&lq)[QR], long long q0, long long j0,
                                              int tx, int ty, long long* __restrict__ out, long long ld_out) {
    constexpr int NTY = 256 / NTX;
    int sx = tx, sy = ty;
    tk_behind_loop(sx, sy);
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

// ---- the host side of a row call ------------------------------------------------------------------------------------
// The checks of the byte rows of a call, `who` naming it in the message: D <= d_max is what its 32-bit accumulator holds.
inline int tk_operands_check(dlc_ctx* ctx, const char* who, const void* queries, int64_t Q, int64_t ldq, const void* db,
                             int64_t N, int64_t ldd, int64_t D, int64_t d_max) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!queries || !db || Q < 1 || N < 1 || D < 1 || ldq < D || ldd < D)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: bad argument", who);
    if ((((uintptr_t)queries) & 15) || (((uintptr_t)db) & 15) || (ldq & 15) || (ldd & 15))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: rows must be 16-byte aligned (bases, ldq, ldd)", who);
    if (D > d_max)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: D=%lld too large for 32-bit accumulation (above %lld)", who,
                         (long long)D, (long long)d_max);
    if (N > 0xffffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: N must be below 2^32", who);
    return DLC_OK;
}
// The checks of a row call: its operands, its int64 [Q, ld_out] result, and Q <= 2^20 (the query tiles fit grid y).
inline int tk_rows_check(dlc_ctx* ctx, const char* who, const void* queries, int64_t Q, int64_t ldq, const void* db,
                         int64_t N, int64_t ldd, int64_t D, int64_t d_max, const void* out, int64_t ld_out) {
    const int rc = tk_operands_check(ctx, who, queries, Q, ldq, db, N, ldd, D, d_max);
    if (rc != DLC_OK) return rc;
    if (!out) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: bad argument", who);
    if (ld_out < N) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld_out=%lld < N=%lld", who, (long long)ld_out, (long long)N);
    if (((uintptr_t)out) & 7) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: out must be 8-byte aligned", who);
    if (Q > (1ll << 20)) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: Q must not exceed 2^20", who);
    return DLC_OK;
}

// The grid of a row kernel whose tiles hold db_rows db rows, for the lmax rows that any query sees.
inline dim3 tk_grid(int64_t lmax, int db_rows, unsigned qtiles) {
    const int64_t tiles = dlc::cdiv(lmax, db_rows);
    return dim3((unsigned)(tiles < TK_MAX_GRID_X ? tiles : TK_MAX_GRID_X), qtiles);
}

// The launch of a checked row call: launch(TkShape<NTX, QR>{}, lmax, qtiles) starts `kernel` in the plan's shape on the
// context's device -- nothing where no query sees a row.
template <typename Launch>
int tk_rows_launch(dlc_ctx* ctx, const char* kernel, int64_t Q, int64_t N, int64_t limit0, int64_t limit_step,
                   Launch&& launch) {
    const TkPlan p = tk_plan(Q);
    const unsigned qtiles = (unsigned)dlc::cdiv(Q, p.qt());      // <= 65535 (grid y) for every Q <= 2^20: 16-row tiles end at 2^20 - 16
    // rows any query sees (the limit is linear in the query row: its largest value is at one end)
    const int64_t lmax = dlc::max_row_limit(0, Q - 1, N, limit0, limit_step);
    if (lmax == 0) return DLC_OK;
    DLC_ON_DEVICE(ctx);
    if (p.ntx == 16) launch(TkShape<16, 4>{}, lmax, qtiles);
    else if (p.qr == 4) launch(TkShape<64, 4>{}, lmax, qtiles);
    else launch(TkShape<64, 1>{}, lmax, qtiles);
    DLC_LAUNCH_CHECK(ctx, kernel);
    return DLC_OK;
}

// A whole plain row call (B: the byte type): pick(shape) is the kernel of a shape, all of one signature.
template <typename B, typename Pick>
int tk_rows_call(dlc_ctx* ctx, const char* who, const char* kernel, int64_t d_max, const B* queries, int64_t Q, int64_t ldq,
                 const B* db, int64_t N, int64_t ldd, int64_t D, int64_t limit0, int64_t limit_step, int64_t* out,
                 int64_t ld_out, void* stream, Pick pick) {
    const int rc = tk_rows_check(ctx, who, queries, Q, ldq, db, N, ldd, D, d_max, out, ld_out);
    if (rc != DLC_OK) return rc;
    return tk_rows_launch(ctx, kernel, Q, N, limit0, limit_step, [&](auto shape, int64_t lmax, unsigned qtiles) {
        hipLaunchKernelGGL(pick(shape), tk_grid(lmax, shape.ntx * 4, qtiles), dim3(256), 0, (hipStream_t)stream, queries,
                           (long long)Q, (long long)ldq, db, (long long)N, (long long)ldd, (long long)D, (long long)limit0,
                           (long long)limit_step, (long long*)out, (long long)ld_out);
    });
}

}  // namespace
