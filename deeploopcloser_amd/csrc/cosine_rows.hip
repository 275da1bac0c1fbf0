// Cosine score rows in fp64: out_scores[r][j] = THE score of the cosine path (include/dlc.h: the fp64 sum of the exact
// products in rescore8_f64's order, cosine_topk.hip) of query row r against database row j, and out_keys[r][j] = the
// integer the path ranks by (f64_key: round-half-even(s * 2^40)), for a batch of Q query rows against the first lim(r)
// of N rows -- what a streaming caller needs to run the sequence search (sequence.hip) on the cosine measure, and what
// anyone needs who wants a row that agrees bit for bit with what dlc_cosine_topk* reports.
//
// The order that defines the value fixes only which LANE sums which 16-byte pieces (lane l: pieces l, l + 64, ... in
// ascending order, the eight elements of a piece in ascending order, one fma chain from +0.0) and how the 64 chains are
// combined (the xor 32, 16, ..., 1 butterfly).  So a wave register-tiles: it owns a QT x RT block of (query, row) pairs,
// keeps QT * RT chains per lane, converts QT + RT pieces to fp64 once per 512-element step and issues QT * RT * 8 fmas on
// them.  A lane whose piece lies past d takes zeros: fma(0, 0, acc) = acc, the chain is the shorter chain.  The operands
// come straight from L2 (a wave's 64 pieces of a row are 1 KiB contiguous; the next step's pieces are in flight while
// this step's are multiplied): no LDS, no barrier -- the four waves of a workgroup are independent and a wave whose
// queries' limits all lie below its rows goes on to its next tile.
//
// The butterfly is folded: at xor 32 lanes 0..31 keep pair 2i and lanes 32..63 pair 2i + 1, each sending the other
// one's half across -- lane l then holds exactly what the plain butterfly leaves in lane l for the pair it kept (the
// same two addends; a + b = b + a), with half the values left.  After log2(QT * RT) levels one value per lane is left,
// the remaining levels are the plain butterfly, and the lane stores its pair.  QT * RT * 6 shuffles become QT * RT + 1.
// No workspace, no memset, no atomics: every offered cell is stored once, everything else of the outputs keeps its bits.
#include "dlc_internal.h"

namespace {

constexpr int64_t CR_MAX_GRID_Y = 65535;     // db tiles beyond it are walked by the same workgroups (grid stride)

template <typename Tag> __device__ __forceinline__ double cr_f64(unsigned short h);
template <> __device__ __forceinline__ double cr_f64<dlc_bf16_tag>(unsigned short h) { return (double)dlc_bf16_bits_to_f32(h); }
template <> __device__ __forceinline__ double cr_f64<dlc_f16_tag>(unsigned short h) { return (double)dlc_f16_bits_to_f32(h); }

template <typename Tag>
__device__ __forceinline__ void cr_unpack(const u32x4_t& v, double (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[2 * e] = cr_f64<Tag>((unsigned short)(v[e] & 0xffffu));
        o[2 * e + 1] = cr_f64<Tag>((unsigned short)(v[e] >> 16));
    }
}

// One level of the folded butterfly: the first P values of v -> P / 2, lanes with bit O clear keep the even ones.
template <int P, int O, int PMAX>
__device__ __forceinline__ void cr_fold(double (&v)[PMAX], int lane) {
    const bool hi = (lane & O) != 0;
#pragma unroll
    for (int i = 0; i < P / 2; ++i) {
        const double keep = hi ? v[2 * i + 1] : v[2 * i], send = hi ? v[2 * i] : v[2 * i + 1];
        v[i] = keep + __shfl_xor(send, O);
    }
}

// QT x RT pairs per wave, WQ x WR waves per workgroup (256 threads): the workgroup's tile is QT WQ queries x RT WR rows.
// blockIdx.x walks the query tiles (fastest: the workgroups in flight together share their database rows in L2),
// blockIdx.y the database tiles.
template <typename Tag, int QT, int RT, int WQ, int WR>
__global__ __launch_bounds__(256) void cosine_rows_kernel(const char* __restrict__ Q, long long nq, long long ldq_b,
                                                          const char* __restrict__ DB, long long n, long long lddb_b,
                                                          long long d, long long limit0, long long limit_step,
                                                          double* __restrict__ out_s, long long* __restrict__ out_k,
                                                          long long ld_out) {
    static_assert(WQ * WR == 4 && (QT * RT == 8 || QT * RT == 16), "four waves; 8 or 16 pairs per wave");
    constexpr int P = QT * RT;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long q0 = ((long long)blockIdx.x * WQ + w / WR) * QT;
    if (q0 >= nq) return;                                       // (wave-uniform; the kernel has no barrier)
    // rows this wave's queries may see: limits are linear in the query row, so the largest sits at an end
    const long long qlast = (q0 + QT < nq ? q0 + QT : nq) - 1;
    const long long la = dlc::row_limit(q0, n, limit0, limit_step), lb = dlc::row_limit(qlast, n, limit0, limit_step);
    const long long lmax = la > lb ? la : lb;
    const char* qp[QT];
#pragma unroll
    for (int r = 0; r < QT; ++r)                                 // a query past the batch reads the last one's row: never stored
        qp[r] = Q + (q0 + r < nq ? q0 + r : nq - 1) * ldq_b + lane * 16;

    for (long long j0 = ((long long)blockIdx.y * WR + w % WR) * RT; j0 < lmax; j0 += (long long)gridDim.y * (WR * RT)) {
        const char* rp[RT];
#pragma unroll
        for (int c = 0; c < RT; ++c)                             // a row nobody sees reads the last seen one: never stored
            rp[c] = DB + (j0 + c < lmax ? j0 + c : lmax - 1) * lddb_b + lane * 16;
        double acc[P];
#pragma unroll
        for (int i = 0; i < P; ++i) acc[i] = 0.0;
        u32x4_t qv[QT], rv[RT], qn[QT], rn[RT];
        auto fetch = [&](long long k0, u32x4_t (&a)[QT], u32x4_t (&b)[RT]) {
            const bool ok = k0 + lane * 8 < d;
#pragma unroll
            for (int r = 0; r < QT; ++r) a[r] = ok ? *(const u32x4_t*)(qp[r] + k0 * 2) : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < RT; ++c) b[c] = ok ? *(const u32x4_t*)(rp[c] + k0 * 2) : u32x4_t{0u, 0u, 0u, 0u};
        };
        // one 512-element step on the pieces in (cq, cr) while the next step's pieces arrive in (nq_, nr)
        auto step = [&](long long k0, const u32x4_t (&cq)[QT], const u32x4_t (&cr)[RT], u32x4_t (&nq_)[QT], u32x4_t (&nr)[RT]) {
            if (k0 + 512 < d) fetch(k0 + 512, nq_, nr);
            double qd[QT][8];
#pragma unroll
            for (int r = 0; r < QT; ++r) cr_unpack<Tag>(cq[r], qd[r]);
#pragma unroll
            for (int c = 0; c < RT; ++c) {
                double xd[8];
                cr_unpack<Tag>(cr[c], xd);
#pragma unroll
                for (int r = 0; r < QT; ++r)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[r * RT + c] = fma(qd[r][e], xd[e], acc[r * RT + c]);
            }
        };
        fetch(0, qv, rv);
        for (long long k0 = 0; k0 < d; k0 += 1024) {             // two steps a trip: the two sets of pieces swap roles
            step(k0, qv, rv, qn, rn);
            if (k0 + 512 < d) step(k0 + 512, qn, rn, qv, rv);
        }
        // folded butterfly: level t (xor 32 >> t) puts bit t of the pair's index into the lane's bit 5 - t
        cr_fold<P, 32>(acc, lane);
        cr_fold<P / 2, 16>(acc, lane);
        cr_fold<P / 4, 8>(acc, lane);
        int pair = ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2);
        int rest = 4;
        if constexpr (P == 16) {
            cr_fold<2, 4>(acc, lane);
            pair |= ((lane >> 2) & 1) << 3;
            rest = 2;
        }
        double v = acc[0];
        for (int o = rest; o > 0; o >>= 1) v += __shfl_xor(v, o);
        // the lane with the low bits clear stores its pair (query row pair / RT, db row pair % RT), guarded by j < lim(r)
        const long long q = q0 + pair / RT, j = j0 + pair % RT;
        if ((lane & (2 * rest - 1)) == 0 && q < nq && j < dlc::row_limit(q, n, limit0, limit_step)) {
            if (out_s) out_s[q * ld_out + j] = v;
            if (out_k) out_k[q * ld_out + j] = f64_key(v);
        }
    }
}

}  // namespace

extern "C" int dlc_cosine_score_rows(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq, const void* DB,
                                     int64_t n, int64_t lddb, int64_t d, int64_t limit0, int64_t limit_step,
                                     double* out_scores, int64_t* out_keys, int64_t ld_out, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (dtype != DLC_BF16 && dtype != DLC_F16)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: dtype %d (need DLC_BF16 or DLC_F16)", dtype);
    if (!Q || !DB || q < 1 || n < 1 || d < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: null/empty operand");
    if (!out_scores && !out_keys) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: neither out_scores nor out_keys");
    if ((d % 8) || ldq < d || lddb < d || (ldq % 8) || (lddb % 8))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: d and the row strides (>= d) must be multiples of 8 elements");
    if (((uintptr_t)Q & 15) || ((uintptr_t)DB & 15))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: operands must be 16-byte aligned");
    if (ld_out < n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: ld_out=%lld < n=%lld", (long long)ld_out, (long long)n);
    if (((uintptr_t)out_scores & 7) || ((uintptr_t)out_keys & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cosine_score_rows: outputs must be 8-byte aligned");
    if (q > 0x7fffff00ll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "cosine_score_rows: q too large");
    // rows any query sees (the limit is linear in the query row: its largest value is at one end)
    const int64_t lmax = dlc::max_row_limit(0, q - 1, n, limit0, limit_step);
    if (lmax == 0) return DLC_OK;
    DLC_ON_DEVICE(ctx);
    auto launch = [&](auto kern, int qtile, int rtile) {
        const int64_t tiles = dlc::cdiv(lmax, rtile);
        const dim3 grid((unsigned)dlc::cdiv(q, qtile), (unsigned)(tiles < CR_MAX_GRID_Y ? tiles : CR_MAX_GRID_Y));
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, (const char*)Q, (long long)q, (long long)ldq * 2,
                           (const char*)DB, (long long)n, (long long)lddb * 2, (long long)d, (long long)limit0,
                           (long long)limit_step, out_scores, (long long*)out_keys, (long long)ld_out);
    };
    // a single query has no second query to share a row's conversion with: 1 x 8 pairs per wave, 32 rows per workgroup
    if (dtype == DLC_BF16) {
        if (q == 1) launch(cosine_rows_kernel<dlc_bf16_tag, 1, 8, 1, 4>, 1, 32);
        else launch(cosine_rows_kernel<dlc_bf16_tag, 4, 4, 2, 2>, 8, 8);
    } else {
        if (q == 1) launch(cosine_rows_kernel<dlc_f16_tag, 1, 8, 1, 4>, 1, 32);
        else launch(cosine_rows_kernel<dlc_f16_tag, 4, 4, 2, 2>, 8, 8);
    }
    DLC_LAUNCH_CHECK(ctx, "cosine_rows_kernel");
    return DLC_OK;
}
