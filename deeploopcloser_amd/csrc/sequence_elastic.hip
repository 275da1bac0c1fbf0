// Elastic sequence search over a dense score matrix, with the selection fused: dlc_sequence_elastic_topk (include/dlc.h).
// Where dlc_sequence_topk (sequence.hip) sums along straight lines, here every frame of the L-frame chain may step back by
// any d in d_min .. d_max key-frames: a dynamic programme over L levels,
//     A_0(c) = M[r-L+1][c],   A_t(c) = best valid A_{t-1}(c - d) + M[r-L+1+t][c],   E(r, j) = A_{L-1}(j),
// the lowest d among equals, one addition per cell and level (oldest row first).
//
//   scan   one WAVE per (output row, slab of columns); a workgroup is four consecutive rows of one slab, whose matrix
//          rows are nearly the same ones (L1 / L2 serve three of the four).  The wave walks its slab in tiles of ct
//          columns.  Per tile it keeps ONE level of the programme in LDS, (key, span) per column over the tile and a
//          halo of (L-1) * d_max columns on its left, padded to `lead` (whole 64-lane chunks), and updates it IN PLACE
//          level by level: a level reads only columns at or left of the one it writes, so the wave takes the level's
//          64-column chunks from the right to the left and every chunk still finds the previous level to its left.
//          Level t needs ONE matrix row, read coalesced through the caches (nothing at or past that row's limit).  The
//          halo shrinks by d_max per level: at level t only columns from lead - (L-1-t) * d_max on can reach an output
//          column, whole chunks left of that are skipped, and what the rest of that chunk holds is never read by a
//          column that counts.  The last level is not stored: its cells go to seq_out and into the
//          row's sorted list, which stays in the wave's registers for the whole slab (topk_list.h).  No barrier: a wave
//          shares its LDS with nobody.
//   merge  sequence_merge.h, as the linear search: the tag's low word carries the span.
//
// LDS holds keys in the order of merit (larger = better: dlc_f64_key of the fp64 sum or the biased int64 sum, complemented
// when lower is better), so "best" is one unsigned compare for every dtype and order; the span word EL_NONE marks a cell
// that is not valid (out of its row's limit, a NaN, no valid predecessor) -- no per-predecessor limit test.
#include "sequence_merge.h"

namespace {

constexpr int EL_ROWS = 4;                 // output rows per workgroup: one per wave
constexpr int EL_CT = 512, EL_CT_WIDE = 1024, EL_WIDE_HALO = 256;   // columns per tile; the wide tile past this halo
constexpr int EL_CT_MIN = 128, EL_WANT_WG = 256;   // a small call: narrower tiles, down to this, until this many workgroups
constexpr int EL_PAD = DLC_MAX_STEP;       // never-valid columns in front of a wave's level: b - d stays inside it
constexpr unsigned short EL_NONE = 0xffff; // the span of a cell that is not valid ((L-1) * d_max <= 504)

struct ElArgs {
    const void* M;
    long long rows, row0, n, ld, limit0, limit_step, tiles_per_slab, ld_out;
    unsigned long long* part;              // [rows - row0][G][k][2]; NULL: no lists (dense output only)
    void* seq_out;
    const long long* poison;
    int L, d_min, d_max, lower, k, ct, lead;
};

template <int DT>
__global__ __launch_bounds__(256) void sequence_elastic_scan_kernel(const ElArgs a) {
    constexpr bool IS_INT = DT == DLC_I64;
    extern __shared__ __attribute__((aligned(16))) char el_smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int L = a.L, k = a.k, ct = a.ct, lead = a.lead, dmin = a.d_min, dmax = a.d_max;
    const int wcols = EL_PAD + lead + ct;                         // a wave's level: columns b = -EL_PAD .. lead + ct - 1
    unsigned long long* K = (unsigned long long*)el_smem + (size_t)w * wcols + EL_PAD;
    unsigned short* S = (unsigned short*)((unsigned long long*)el_smem + (size_t)EL_ROWS * wcols) + (size_t)w * wcols + EL_PAD;
    const long long r = a.row0 + (long long)blockIdx.x * EL_ROWS + w;
    if (r >= a.rows) return;                                      // (the kernel has no barrier)
    const long long G = gridDim.y, g = blockIdx.y;
    const bool poisoned = a.poison && *a.poison != 0;
    const bool search = !poisoned && r - (L - 1) >= 0;            // else: the row offers nothing
    // columns this row may offer; the dense output wants every column of the matrix
    const long long colend = a.seq_out ? a.n : (search ? dlc::row_limit(r, a.n, a.limit0, a.limit_step) : 0);
    const long long slab0 = g * a.tiles_per_slab * ct;
    const long long slab1 = slab0 + a.tiles_per_slab * ct < colend ? slab0 + a.tiles_per_slab * ct : colend;
    const unsigned long long flip = a.lower ? ~0ull : 0ull;

    if (lane < EL_PAD) { K[-1 - lane] = 0ull; S[-1 - lane] = EL_NONE; }   // (level 0 writes every chunk a later level reads)
    WaveList<TlPair> wl;
    wl.clear();
    for (long long j0 = slab0; j0 < slab1; j0 += ct) {
        const int top = slab1 - j0 < ct ? (int)(slab1 - j0) : ct;   // the tile's columns in use
        if (!search) {
            for (int jl = lane; jl < top; jl += 64)
                sq_store_dense<IS_INT>(a.seq_out, (r - a.row0) * a.ld_out + j0 + jl, false, 0ull);
            continue;
        }
        const int qtop = (lead + top - 1) >> 6;
        for (int t = 0; t < L; ++t) {
            const long long rho = r - (L - 1) + t;
            const long long lim = dlc::row_limit(rho, a.n, a.limit0, a.limit_step);
            const long long base = rho * a.ld;
            const bool last = t == L - 1;
            const int qlow = (lead - (L - 1 - t) * dmax) >> 6;    // the chunk of the first column that can reach an output
            for (int q = qtop; q >= qlow; --q) {
                const int b = q * 64 + lane;
                const long long c = j0 - lead + b;
                const bool in = c >= 0 && c < lim;
                const unsigned long long bits = in ? rows_bits<DT>(a.M, base + c) : 0ull;
                bool ok = in;
                unsigned long long key = 0ull;                    // (the best predecessor's, then the cell's own)
                int span = 0;
                if (t > 0) {
                    ok = false;
                    for (int d = dmin; d <= dmax; ++d) {          // ascending d, strict compare: the lowest d among equals
                        const unsigned long long pk = K[b - d];
                        const int ps = S[b - d];
                        if (ps != EL_NONE && (!ok || pk > key)) { ok = true; key = pk; span = ps + d; }
                    }
                    ok = ok && in;
                }
                // (el_level_key of sequence_merge.h, spelled out: through the function the same arithmetic is scheduled
                // differently and this kernel measured 8-17 % slower, docs/LAB.md 19)
                if (IS_INT) {
                    const unsigned long long sum = t > 0 ? ((key ^ flip) ^ ROWS_SIGN) + bits : bits;
                    key = (sum ^ ROWS_SIGN) ^ flip;
                } else {
                    const double x = __longlong_as_double((long long)bits);
                    const double sum = t > 0 ? dlc_f64_unkey(key ^ flip) + x : x;
                    ok = ok && sum == sum;
                    key = dlc_f64_key(sum) ^ flip;
                }
                if (!last) {
                    K[b] = key;
                    S[b] = ok ? (unsigned short)span : EL_NONE;
                    // Within the chunk all 64 lanes have read before any of them writes (one wave, in lockstep); the
                    // next chunk, and the next level, read what other lanes of this wave wrote: keep the order
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    continue;
                }
                const bool have = ok && c < slab1;                // (b >= lead here: c >= j0)
                if (a.seq_out && c < slab1) sq_store_dense<IS_INT>(a.seq_out, (r - a.row0) * a.ld_out + c, have, key ^ flip);
                if (a.part) {                                     // (the line scan offers the same way: docs/LAB.md 26)
                    const TlPair cand = {key, ((unsigned long long)(~(unsigned)c) << 32) | (unsigned)span};
                    for (unsigned long long todo = __ballot(have && cand.before(wl.kth)); todo; todo &= todo - 1) {
                        const TlPair x = cand.shfl(__ffsll((long long)todo) - 1);
                        if (x.before(wl.kth)) wl.insert(x, k, lane);      // (the k-th may have moved up since the ballot)
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // (the next tile's level 0 overwrites what this one read)
        __builtin_amdgcn_wave_barrier();
    }
    if (a.part) {
        unsigned long long* P = a.part + (((size_t)(r - a.row0) * G + g) * k) * 2;
        wl.store(k, lane, [&](int i, TlPair e) { P[2 * i] = e.key; P[2 * i + 1] = e.tag; });
    }
}

// The scan's shape: the halo padded to whole chunks, and a tile that grows with it (the halo's columns are recomputed
// per tile: a fifth of the chunks at d_max = 8, L = 64).  A call too small to give every CU a workgroup (a streamed
// batch against a short map) halves the tile, not below the padded halo: a wave's serial walk over its tiles is what
// such a call takes.
struct ElPlan { int ct, lead; size_t lds; };
ElPlan el_plan(int L, int d_max, int64_t blocks, int64_t cols) {
    const int halo = (L - 1) * d_max, lead = (halo + 63) / 64 * 64;
    int ct = halo > EL_WIDE_HALO ? EL_CT_WIDE : EL_CT;
    while (ct > EL_CT_MIN && ct / 2 >= lead && blocks * dlc::cdiv(cols, ct) < EL_WANT_WG) ct /= 2;
    return {ct, lead, dlc::align_up((size_t)EL_ROWS * (EL_PAD + lead + ct) * 10, 16)};
}

bool el_sizes_ok(int64_t rows, int64_t n, int L, int d_min, int d_max, int k) {
    return rows >= 1 && n >= 1 && n <= 0x7fffffffll && L >= 1 && L <= EL_MAX_L && d_min >= 0 && d_min <= d_max &&
           d_max <= DLC_MAX_STEP && k >= 1 && k <= DLC_MAX_K;
}

}  // namespace

extern "C" size_t dlc_sequence_elastic_topk_workspace_bytes(int64_t rows, int64_t n, int L, int d_min, int d_max, int k) {
    if (!el_sizes_ok(rows, n, L, d_min, d_max, k)) return 0;
    const int64_t slabs = dlc::max_slabs(dlc::cdiv(rows, EL_ROWS), dlc::cdiv(n, EL_CT_MIN), TL_MAX_SLABS);
    return dlc::align_up((size_t)rows * (size_t)slabs * (size_t)k * 16, 256);
}

extern "C" int dlc_sequence_elastic_topk(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n,
                                         int64_t ld, int64_t limit0, int64_t limit_step, int L, int d_min, int d_max,
                                         int lower_is_better, int k, void* out_scores, int64_t* out_idx, int32_t* out_span,
                                         void* seq_out, int64_t ld_out, const int64_t* poison, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (L < 1 || L > EL_MAX_L) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_elastic_topk: L=%d outside 1..%d", L, EL_MAX_L);
    if (d_min < 0 || d_min > d_max || d_max > DLC_MAX_STEP)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_elastic_topk: steps %d..%d: need 0 <= d_min <= d_max <= %d", d_min, d_max,
                         DLC_MAX_STEP);
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, 0, 0};
    ElArgs a;
    const int rc = sq_front(ctx, "sequence_elastic_topk", s, row0, L, k, out_scores, out_idx, out_span, seq_out, ld_out, poison,
                            workspace, workspace_bytes, dlc_sequence_elastic_topk_workspace_bytes(rows, n, L, d_min, d_max, k), a);
    if (rc != DLC_OK) return rc;
    const int64_t rows_out = rows - row0;
    const int64_t blocks = dlc::cdiv(rows_out, EL_ROWS);
    if (rows_out > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sequence_elastic_topk: too many rows for one launch");
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;

    // columns any output row offers (limits are linear in the row); the dense output covers the matrix's n columns
    const int64_t cols = seq_out ? n : dlc::max_row_limit(row0, rows - 1, n, limit0, limit_step);
    const ElPlan p = el_plan(L, d_max, blocks, cols);
    dlc::SlabSplit slabs = {1, 1};
    if (cols > 0) slabs = dlc::split_slabs(dlc::cdiv(rows, EL_ROWS), dlc::cdiv(cols, p.ct), TL_MAX_SLABS);
    a.tiles_per_slab = slabs.tiles_per_slab; a.d_min = d_min; a.d_max = d_max; a.ct = p.ct; a.lead = p.lead;
    const dim3 grid((unsigned)blocks, (unsigned)slabs.G);
    rows_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(sequence_elastic_scan_kernel<dt.value>, grid, dim3(256), p.lds, st, a);
        return 0;
    });
    DLC_LAUNCH_CHECK(ctx, "sequence_elastic_scan_kernel");
    return sq_launch_merge(ctx, dtype, a, slabs.G, out_scores, out_idx, out_span, st);
}
