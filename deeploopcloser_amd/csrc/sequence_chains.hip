// The matched chain of a candidate of the sequence searches: dlc_sequence_elastic_chains and dlc_sequence_chains
// (include/dlc.h).  The searches answer (score, j) per candidate and keep one scalar of the alignment behind it (the
// span, the slope); here the alignment itself is formed again for the candidates' cells alone -- the L matched columns,
// oldest frame first, and the matrix cells along them.
//
//   elastic   one WAVE, one workgroup, per (output row, slot).  Only a trapezoid can reach (r, j): at level t the columns
//             lo_t .. lo_t + w_t - 1 with lo_t = j - (L-1-t) * d_max and w_t = (L-1-t) * (d_max - d_min) + 1 (at most
//             505 at level 0, one at the last), closed under "predecessor of".  In the trapezoid's own coordinates,
//             b = c - lo_t, the predecessor of b by step d is b + d_max - d of the level before: a level reads at or
//             RIGHT of what it writes, so the wave keeps ONE level of keys in LDS and updates it in place, 64-column
//             chunks from the left to the right (the mirror image of the scan in sequence_elastic.hip, which keeps
//             global columns and goes right to left).  Keys, flip, validity and the wave-level fencing are the scan's
//             (el_level_key, sequence_merge.h).  What the scan does not keep: the chosen step, or "not valid", of every
//             (level, column) -- ONE BYTE per entry, [L][W] with W = w_0 padded to whole chunks, at most 64 x 512 = 32 KB
//             beside the 4 KB of keys, so a workgroup is one wave and four of them share a CU's LDS at the largest
//             shape (a 4-bit table would put two waves into a workgroup at the price of a read-modify-write per entry).
//             A level's matrix row is loaded one level ahead into registers (at most 8 chunks), so the wave waits for
//             memory L times, not once per chunk.  Then every lane walks back from j through the table (the reads are
//             broadcasts), lane t keeps the column of level t, and the wave writes the L columns and cells.
//   lines     one wave per (output row, slot), four to a workgroup, no LDS: lane v forms Z_v in the header's order
//             (newest row first), the lowest best v is found by n_slopes shuffles, lane t writes column and cell of row
//             rho(t).
#include "sequence_merge.h"

namespace {

constexpr int CH_MAX_Q = 8;                // 64-column chunks of the widest level: (64 - 1) * 8 + 1 = 505 columns
constexpr unsigned char CH_NONE = 0xff;    // the step of a cell that is not valid (a step is at most DLC_MAX_STEP)

struct ChArgs {
    const void* M;
    long long rows, row0, n, ld, limit0, limit_step, slots;       // slots = (rows - row0) * k
    const long long* idx;                  // [slots]
    int* chain;                            // [slots][L]
    void* cells;                           // [slots][L] fp64 / int64; may be NULL
    int* slope;                            // [slots]; lines only, may be NULL
    const long long* poison;
    int L, d_min, d_max, V, lower, k, W;
};

// (r, j) of a slot; j = -1 where the slot holds no cell the row offers (never a column to read from)
__device__ __forceinline__ long long ch_cell(const ChArgs& a, long long slot, long long& r) {
    r = a.row0 + slot / a.k;
    const long long j = a.idx[slot];
    const bool poisoned = a.poison && *a.poison != 0;
    const bool cand = !poisoned && r - (a.L - 1) >= 0 && j >= 0 && j < dlc::row_limit(r, a.n, a.limit0, a.limit_step);
    return cand ? j : -1ll;
}

// Lane t < L writes level t of the slot's chain: `col` (-1: not a chain) and the cell M[rho(t)][col].
template <int DT>
__device__ __forceinline__ void ch_write(const ChArgs& a, long long slot, long long r, int t, int col) {
    a.chain[slot * a.L + t] = col;
    if (!a.cells) return;
    const long long rho = r - (a.L - 1) + t;                      // fp64 goes out by its bits: the conversion from fp32 is exact
    ((long long*)a.cells)[slot * a.L + t] = col >= 0 ? (long long)rows_bits<DT>(a.M, rho * a.ld + col)
                                                      : (DT == DLC_I64 ? -1ll : ROWS_NAN_BITS);
}

template <int DT>
__global__ __launch_bounds__(64) void sequence_elastic_chains_kernel(const ChArgs a) {
    constexpr bool IS_INT = DT == DLC_I64;
    extern __shared__ __attribute__((aligned(16))) char ch_smem[];
    unsigned long long* K = (unsigned long long*)ch_smem;         // [W] the level's keys
    unsigned char* T = (unsigned char*)(K + a.W);                 // [L][W] the chosen step of every (level, column)
    const int lane = threadIdx.x, L = a.L, W = a.W, dmin = a.d_min, dmax = a.d_max, dd = dmax - dmin;
    const long long slot = blockIdx.x;
    long long r;
    const long long jl = ch_cell(a, slot, r);
    const int j = (int)jl;                                        // (n < 2^31)
    const unsigned long long flip = a.lower ? ~0ull : 0ull;
    int mine = -1;                                                // lane t: the chain's column at level t

    if (jl >= 0) {
        // level t's chunks of its matrix row, 0 where the trapezoid leaves the row's offer
        auto fetch = [&](int t, unsigned long long (&x)[CH_MAX_Q]) {
            const long long rho = r - (L - 1) + t;
            const long long lim = dlc::row_limit(rho, a.n, a.limit0, a.limit_step);
            const int lo = j - (L - 1 - t) * dmax, wt = (L - 1 - t) * dd + 1;
#pragma unroll
            for (int q = 0; q < CH_MAX_Q; ++q) {
                const int b = q * 64 + lane;
                const long long c = (long long)lo + b;
                x[q] = (q * 64 < wt && b < wt && c >= 0 && c < lim) ? rows_bits<DT>(a.M, rho * a.ld + c) : 0ull;
            }
        };
        unsigned long long cur[CH_MAX_Q], nxt[CH_MAX_Q];
        fetch(0, cur);
        for (int t = 0; t < L; ++t) {
            if (t + 1 < L) fetch(t + 1, nxt);
            const long long lim = dlc::row_limit(r - (L - 1) + t, a.n, a.limit0, a.limit_step);
            const int lo = j - (L - 1 - t) * dmax, wt = (L - 1 - t) * dd + 1;
            unsigned char* Tt = T + (size_t)t * W;
#pragma unroll
            for (int q = 0; q < CH_MAX_Q; ++q) {
                if (q * 64 >= wt) break;                          // (wave-uniform)
                const int b = q * 64 + lane;
                const long long c = (long long)lo + b;
                const bool act = b < wt;                          // b + dd < w_{t-1} <= W then: every read stays inside
                bool ok = act && c >= 0 && c < lim;
                unsigned long long key = 0ull;                    // (the best predecessor's, then the cell's own)
                int step = 0;
                if (t > 0 && act) {
                    bool have = false;
                    for (int d = dmin; d <= dmax; ++d) {          // ascending d, strict compare: the lowest d among equals
                        const int bp = b + dmax - d;
                        const unsigned long long pk = K[bp];
                        if (Tt[bp - W] != CH_NONE && (!have || pk > key)) { have = true; key = pk; step = d; }
                    }
                    ok = ok && have;
                }
                key = el_level_key<IS_INT>(key, flip, cur[q], t, ok);
                if (act) {
                    K[b] = key;
                    Tt[b] = ok ? (unsigned char)step : CH_NONE;
                }
                // Within the chunk all 64 lanes have read before any of them writes (one wave, in lockstep); the next
                // chunk, the next level and the walk back read what other lanes of this wave wrote: keep the order
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int q = 0; q < CH_MAX_Q; ++q) cur[q] = nxt[q];
        }
        if (T[(size_t)(L - 1) * W] != CH_NONE) {                  // E(r, j) is valid: every cell its chain passes is
            int c = j;
            for (int t = L - 1; t >= 0; --t) {
                if (lane == t) mine = c;
                if (t > 0) c -= T[(size_t)t * W + (c - (j - (L - 1 - t) * dmax))];
            }
        }
    }
    if (lane < L) ch_write<DT>(a, slot, r, lane, mine);
}

template <int DT>
__global__ __launch_bounds__(256) void sequence_chains_kernel(const ChArgs a, const SqOffsets offs) {
    constexpr bool IS_INT = DT == DLC_I64;
    const int lane = threadIdx.x & 63, L = a.L;
    const long long slot = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= a.slots) return;                                  // (the kernel has no barrier)
    long long r;
    const long long j = ch_cell(a, slot, r);
    bool ok = j >= 0 && lane < a.V;
    unsigned long long key = 0ull;
    if (ok) {                                                     // lane v: Z_v, newest row first
        const short* o = offs.o + lane * L;
        double facc = 0.0;                                        // (sequence_scan_kernel<DT, false> sums the same way)
        unsigned long long iacc = 0ull;
        for (int s = 0; s < L; ++s) {
            const long long jj = j - o[s];
            const bool in = jj >= 0 && jj < dlc::row_limit(r - s, a.n, a.limit0, a.limit_step);
            ok &= in;
            const unsigned long long bits = in ? rows_bits<DT>(a.M, (r - s) * a.ld + jj)
                                               : (IS_INT ? 0ull : (unsigned long long)ROWS_NAN_BITS);
            if (IS_INT) iacc += bits;
            else facc = s == 0 ? __longlong_as_double((long long)bits) : facc + __longlong_as_double((long long)bits);
        }
        if (!IS_INT) ok = facc == facc;
        key = IS_INT ? (iacc ^ ROWS_SIGN) : dlc_f64_key(facc);
        if (a.lower) key = ~key;
    }
    bool have = false;
    unsigned long long bk = 0ull;
    int bv = -1;
    for (int v = 0; v < a.V; ++v) {                               // ascending v, strict compare: the lowest v among equals
        const unsigned long long kv = (unsigned long long)__shfl((long long)key, v);
        const bool okv = __shfl((int)ok, v) != 0;
        if (okv && (!have || kv > bk)) { have = true; bk = kv; bv = v; }
    }
    if (lane < L) ch_write<DT>(a, slot, r, lane, have ? (int)(j - offs.o[bv * L + (L - 1 - lane)]) : -1);
    if (lane == 0 && a.slope) a.slope[slot] = bv;
}

// What the two entry points check alike (`who` names the caller in the message); DLC_OK: a holds what they fill alike.
int ch_front(dlc_ctx* ctx, const char* who, const ScoreRows& s, int64_t row0, int L, int k, const int64_t* idx, int32_t* out_chain,
             void* out_cells, int32_t* out_slope, const int64_t* poison, ChArgs& a) {
    const int rc = rows_check(ctx, who, s, poison, DLC_ERR_BAD_ARG);
    if (rc != DLC_OK) return rc;
    if (!idx || !out_chain || row0 < 0 || row0 >= s.rows) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: bad argument", who);
    if (L < 1 || L > SQ_MAX_L) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: L=%d outside 1..%d", who, L, SQ_MAX_L);
    if (k < 1 || k > DLC_MAX_K) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: k=%d outside 1..%d", who, k, DLC_MAX_K);
    if ((s.rows - row0) * (int64_t)k > 0x7fffffffll)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: too many candidates for one launch", who);
    rows_fill(a, s);
    a.rows = s.rows; a.row0 = row0; a.slots = (s.rows - row0) * k; a.idx = (const long long*)idx; a.chain = out_chain;
    a.cells = out_cells; a.slope = out_slope; a.poison = (const long long*)poison; a.L = L; a.d_min = 0; a.d_max = 0; a.V = 0;
    a.lower = s.lower; a.k = k; a.W = 0;
    return DLC_OK;
}

}  // namespace

extern "C" int dlc_sequence_elastic_chains(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n,
                                           int64_t ld, int64_t limit0, int64_t limit_step, int L, int d_min, int d_max,
                                           int lower_is_better, int k, const int64_t* idx, int32_t* out_chain, void* out_cells,
                                           const int64_t* poison, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, 0, 0};
    ChArgs a;
    const int bad = ch_front(ctx, "sequence_elastic_chains", s, row0, L, k, idx, out_chain, out_cells, nullptr, poison, a);
    if (bad != DLC_OK) return bad;
    if (d_min < 0 || d_min > d_max || d_max > DLC_MAX_STEP)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_elastic_chains: steps %d..%d: need 0 <= d_min <= d_max <= %d", d_min,
                         d_max, DLC_MAX_STEP);
    DLC_ON_DEVICE(ctx);
    a.d_min = d_min; a.d_max = d_max;
    a.W = ((L - 1) * (d_max - d_min) + 1 + 63) / 64 * 64;         // <= 64 * CH_MAX_Q
    const size_t lds = dlc::align_up((size_t)a.W * 8 + (size_t)L * a.W, 16);   // <= 36 KB
    const dim3 grid((unsigned)a.slots);
    hipStream_t st = (hipStream_t)stream;
    rows_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(sequence_elastic_chains_kernel<dt.value>, grid, dim3(64), lds, st, a);
        return 0;
    });
    DLC_LAUNCH_CHECK(ctx, "sequence_elastic_chains_kernel");
    return DLC_OK;
}

extern "C" int dlc_sequence_chains(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n, int64_t ld,
                                   int64_t limit0, int64_t limit_step, int L, int n_slopes, const int32_t* offsets,
                                   int lower_is_better, int k, const int64_t* idx, int32_t* out_chain, void* out_cells,
                                   int32_t* out_slope, const int64_t* poison, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, 0, 0};
    ChArgs a;
    const int bad = ch_front(ctx, "sequence_chains", s, row0, L, k, idx, out_chain, out_cells, out_slope, poison, a);
    if (bad != DLC_OK) return bad;
    if (!offsets) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_chains: bad argument");
    if (n_slopes < 1 || n_slopes > SQ_MAX_SLOPES)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_chains: n_slopes=%d outside 1..%d", n_slopes, SQ_MAX_SLOPES);
    SqOffsets offs;
    int maxoff = 0;
    const int bad_table = sq_pack_offsets(ctx, "sequence_chains", offsets, n_slopes, L, &offs, &maxoff);
    if (bad_table != DLC_OK) return bad_table;
    DLC_ON_DEVICE(ctx);
    a.V = n_slopes;
    const dim3 grid((unsigned)dlc::cdiv(a.slots, 4));
    hipStream_t st = (hipStream_t)stream;
    rows_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(sequence_chains_kernel<dt.value>, grid, dim3(256), 0, st, a, offs);
        return 0;
    });
    DLC_LAUNCH_CHECK(ctx, "sequence_chains_kernel");
    return DLC_OK;
}
