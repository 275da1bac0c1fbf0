// Windowed peak top-k over score rows -- distinct-place candidates, the last step of SeqSLAM's matcher (Milford & Wyeth,
// ICRA 2012, III-D: the best trajectory, then the best one outside a window of key-frames around it):
// dlc_peak_topk_rows (include/dlc.h holds the definition).  Pick i is the best offered cell of the row that lies more
// than `suppress` columns from every earlier pick.
//
//   chunks  one workgroup per (row, slab of chunks); a CHUNK is 256 columns, one wave's work: a lane takes four cells 64
//           columns apart, the wave's best offered entry goes into the workspace table [rows][ceil(n / 256)].  This is
//           the only pass over the rows from HBM.  No LDS, no barrier.
//   picks   one workgroup per row, k rounds: the arg-max over the row's table is the pick.  The pick's window
//           [p - suppress, p + suppress] can only have changed the maxima of the chunks it overlaps: a chunk that lies
//           wholly inside it has nothing left (its entry becomes empty without a read), and the at most two chunks the
//           window cuts are formed again from the row, a cell within `suppress` of ANY pick so far counting as absent
//           (waves 0 and 1 take one each).  Every other entry still is the best unsuppressed cell of its chunk.  Work per
//           row: n reads, then k * (n / 256 table entries + at most 512 cells) -- also when suppress >= n.
//
// An entry is topk_list.h's TlPair: a KEY whose unsigned order is the order of merit (the ordered key of the fp64 value,
// or the biased int64, complemented when lower is better) and a TAG (~column << 32: larger = lower column).  (0, 0) is
// the empty slot: below every entry, since a column < 2^31 leaves the tag's top bit set.  Entries of a row are distinct,
// so the result does not depend on the plan.
#include "score_rows.h"
#include "topk_list.h"

namespace {

constexpr int PK_CHUNK = 256;              // columns of a chunk
constexpr int PK_CELLS = PK_CHUNK / 64;    // cells of a lane
constexpr int PK_MAX_WG = 2048;            // workgroups the chunk pass aims at (rows x slabs)

struct PkArgs {
    const void* M;
    unsigned long long* table;             // [rows][nch][2]
    long long rows, n, ld, limit0, limit_step, nch, G, chunks_per_slab, suppress, absent;
    const long long* poison;
    void* out_scores;
    long long* out_idx;
    int lower, has_absent, k;
};

__device__ __forceinline__ TlPair pk_wave_best(TlPair m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const TlPair o = m.shfl_xor(off);
        m = TlPair::pick(o.before(m), o, m);
    }
    return m;
}

// One wave: the best entry of chunk c of the row that starts at element `row`, among its cells below lim.  SUPP: a cell
// within a.suppress of a pick counts as absent -- the picks are picks[0 .. npicks - 1] and `cur` (the round's own, which
// is not in picks[] yet).  Only the picks whose window reaches the chunk are looked at per cell.
template <int DT, bool SUPP>
__device__ __forceinline__ TlPair pk_chunk_best(const PkArgs& a, long long row, long long c, long long lim, int lane,
                                                const int* picks, int npicks, long long cur) {
    const long long j0 = c * PK_CHUNK;
    unsigned long long key[PK_CELLS];
    bool ok[PK_CELLS];
#pragma unroll
    for (int t = 0; t < PK_CELLS; ++t) {                          // (the four loads are in flight together)
        const long long j = j0 + t * 64 + lane;
        key[t] = 0ull;
        ok[t] = j < lim && rows_key<DT>(a.M, row + j, a.has_absent, a.absent, key[t]);
    }
    if (SUPP) {
        // lane i holds picks i and 64 + i; near0 / near1: those whose window reaches [j0, j0 + 255]
        const long long q0 = lane < npicks ? picks[lane] : cur, q1 = lane + 64 < npicks ? picks[lane + 64] : cur;
        auto reaches = [&](long long q) { return q - j0 - (PK_CHUNK - 1) <= a.suppress && j0 - q <= a.suppress; };
        unsigned long long near0 = __ballot(lane <= npicks && reaches(q0));
        unsigned long long near1 = __ballot(lane + 64 <= npicks && reaches(q1));
        auto drop = [&](long long q) {
#pragma unroll
            for (int t = 0; t < PK_CELLS; ++t) {
                const long long d = j0 + t * 64 + lane - q;
                ok[t] = ok[t] && (d < 0 ? -d : d) > a.suppress;
            }
        };
        for (; near0; near0 &= near0 - 1) drop(__shfl(q0, __ffsll((long long)near0) - 1));
        for (; near1; near1 &= near1 - 1) drop(__shfl(q1, __ffsll((long long)near1) - 1));
    }
    TlPair best = TlPair::empty();
#pragma unroll
    for (int t = 0; t < PK_CELLS; ++t) {
        const unsigned long long kk = a.lower ? ~key[t] : key[t];
        const TlPair e = {kk, (unsigned long long)(~(unsigned)(j0 + t * 64 + lane)) << 32};
        best = TlPair::pick(ok[t] && e.before(best), e, best);
    }
    return pk_wave_best(best);
}

template <int DT>
__global__ __launch_bounds__(256) void peak_chunks_kernel(const PkArgs a) {
    if (a.poison && *a.poison != 0) return;                       // (the pick pass answers (NaN, -1) without the table)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long items = a.rows * a.G;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long r = item / a.G, g = item % a.G;
        const long long lim = dlc::row_limit(r, a.n, a.limit0, a.limit_step);
        const long long nchr = dlc::cdiv(lim, PK_CHUNK);
        const long long c1 = (g + 1) * a.chunks_per_slab < nchr ? (g + 1) * a.chunks_per_slab : nchr;
        unsigned long long* T = a.table + r * a.nch * 2;
        for (long long c = g * a.chunks_per_slab + w; c < c1; c += 4) {
            const TlPair b = pk_chunk_best<DT, false>(a, r * a.ld, c, lim, lane, nullptr, 0, 0);
            if (lane == 0) { T[2 * c] = b.key; T[2 * c + 1] = b.tag; }
        }
    }
}

template <int DT>
__global__ __launch_bounds__(256) void peak_picks_kernel(const PkArgs a) {
    constexpr bool IS_INT = DT == DLC_I64;
    __shared__ int picks[DLC_MAX_K];
    __shared__ TlPair wbest[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, k = a.k;
    const bool poisoned = a.poison && *a.poison != 0;
    auto emit = [&](long long slot, TlPair m) {
        const bool none = m.is_empty();
        const unsigned long long k2 = a.lower ? ~m.key : m.key;
        if (IS_INT) ((long long*)a.out_scores)[slot] = none ? -1ll : (long long)(k2 ^ ROWS_SIGN);
        else ((double*)a.out_scores)[slot] = none ? (a.lower ? INFINITY : -INFINITY) : dlc_f64_unkey(k2);
        a.out_idx[slot] = none ? -1ll : (long long)(~(unsigned)(m.tag >> 32));
    };
    // (the trip counts are the workgroup's: every wave meets every barrier)
    for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        if (poisoned) {
            for (int t = tid; t < k; t += 256) {
                ((double*)a.out_scores)[r * k + t] = __longlong_as_double(ROWS_NAN_BITS);
                a.out_idx[r * k + t] = -1;
            }
            continue;
        }
        const long long lim = dlc::row_limit(r, a.n, a.limit0, a.limit_step);
        const long long nchr = dlc::cdiv(lim, PK_CHUNK);
        unsigned long long* T = a.table + r * a.nch * 2;
        int i = 0;
        for (; i < k; ++i) {
            TlPair m = TlPair::empty();
            for (long long c = tid; c < nchr; c += 256) {
                const TlPair v = {T[2 * c], T[2 * c + 1]};
                m = TlPair::pick(v.before(m), v, m);
            }
            m = pk_wave_best(m);
            if (lane == 0) wbest[w] = m;
            __syncthreads();
            m = wbest[0];
#pragma unroll
            for (int ww = 1; ww < 4; ++ww) m = TlPair::pick(wbest[ww].before(m), wbest[ww], m);
            if (m.is_empty()) break;                              // nothing is left: the same in every thread
            const long long p = (long long)(~(unsigned)(m.tag >> 32));
            if (tid == 0) { emit(r * k + i, m); picks[i] = (int)p; }
            // the pick's window, clipped to the row (suppress may be INT64_MAX: no p - suppress, no p + suppress before the test)
            const long long lo = a.suppress >= p ? 0 : p - a.suppress;
            const long long hi = a.suppress >= lim - 1 - p ? lim - 1 : p + a.suppress;
            const long long c_lo = lo / PK_CHUNK, c_hi = hi / PK_CHUNK;
            const long long end_hi = (c_hi + 1) * PK_CHUNK < lim ? (c_hi + 1) * PK_CHUNK : lim;
            const bool cut_lo = lo > c_lo * PK_CHUNK, cut_hi = hi < end_hi - 1;      // cells of the chunk outside the window
            const bool again_lo = cut_lo || (c_lo == c_hi && cut_hi), again_hi = c_hi != c_lo && cut_hi;
            if (w == 0 && again_lo) {
                const TlPair b = pk_chunk_best<DT, true>(a, r * a.ld, c_lo, lim, lane, picks, i, p);
                if (lane == 0) { T[2 * c_lo] = b.key; T[2 * c_lo + 1] = b.tag; }
            }
            if (w == 1 && again_hi) {
                const TlPair b = pk_chunk_best<DT, true>(a, r * a.ld, c_hi, lim, lane, picks, i, p);
                if (lane == 0) { T[2 * c_hi] = b.key; T[2 * c_hi + 1] = b.tag; }
            }
            for (long long c = c_lo + tid; c <= c_hi; c += 256)
                if (!(c == c_lo && again_lo) && !(c == c_hi && again_hi)) { T[2 * c] = 0ull; T[2 * c + 1] = 0ull; }
            __syncthreads();                                      // the table and picks[i] are written, wbest is read
        }
        for (int t = i + tid; t < k; t += 256) emit(r * k + t, TlPair::empty());
        __syncthreads();                                          // (a round left early: wbest is read)
    }
}

template <int DT>
int pk_launch(dlc_ctx* ctx, const PkArgs& a, unsigned chunk_blocks, unsigned pick_blocks, hipStream_t st) {
    if (chunk_blocks) {
        hipLaunchKernelGGL(peak_chunks_kernel<DT>, dim3(chunk_blocks), dim3(256), 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "peak_chunks_kernel");
    }
    hipLaunchKernelGGL(peak_picks_kernel<DT>, dim3(pick_blocks), dim3(256), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "peak_picks_kernel");
    return DLC_OK;
}

}  // namespace

extern "C" size_t dlc_peak_topk_rows_workspace_bytes(int64_t rows, int64_t n, int k) {
    if (rows < 1 || n < 1 || n > 0x7fffffffll || k < 1 || k > DLC_MAX_K) return 0;
    const int64_t nch = dlc::cdiv(n, PK_CHUNK);
    if (rows > (0x7fffffffffffffffll / 16 - 256) / nch) return 0;
    return dlc::align_up((size_t)rows * (size_t)nch * 16, 256);
}

extern "C" int dlc_peak_topk_rows(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t n, int64_t ld,
                                  int64_t limit0, int64_t limit_step, int lower_is_better, int64_t suppress,
                                  int has_absent, int64_t absent, int k, void* out_scores, int64_t* out_idx,
                                  const int64_t* poison, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!out_scores || !out_idx || (((uintptr_t)out_scores) & 7) || (((uintptr_t)out_idx) & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "peak_topk_rows: the outputs must be set and aligned to their element");
    if (suppress < 0) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "peak_topk_rows: suppress=%lld is negative", (long long)suppress);
    if (k < 1 || k > DLC_MAX_K) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "peak_topk_rows: k=%d outside 1..%d", k, DLC_MAX_K);
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, has_absent != 0, absent};
    int rc = rows_check(ctx, "peak_topk_rows", s, poison, DLC_ERR_BAD_SHAPE);
    if (rc == DLC_OK)
        rc = rows_check_workspace(ctx, "peak_topk_rows", workspace, workspace_bytes, dlc_peak_topk_rows_workspace_bytes(rows, n, k));
    if (rc != DLC_OK) return rc;
    PkArgs a;
    rows_fill(a, s);
    a.table = (unsigned long long*)workspace; a.rows = rows; a.nch = dlc::cdiv(n, PK_CHUNK); a.suppress = suppress;
    a.absent = absent; a.poison = (const long long*)poison; a.out_scores = out_scores; a.out_idx = (long long*)out_idx;
    a.lower = s.lower; a.has_absent = s.has_absent; a.k = k;
    // columns any row offers (limits are linear in the row, so the largest sits at an end); none: the pick pass alone
    // writes the empty lists
    const int64_t cols = dlc::max_row_limit(0, rows - 1, n, limit0, limit_step);
    dlc::SlabSplit slabs = {1, 1};
    if (cols > 0) slabs = dlc::split_slabs(rows, dlc::cdiv(cols, PK_CHUNK), PK_MAX_WG);
    a.G = slabs.G; a.chunks_per_slab = slabs.tiles_per_slab;
    const int64_t items = rows * a.G;                             // (<= rows * nch: the workspace's size was formed)
    const unsigned chunk_blocks = cols > 0 ? dlc::capped_blocks(items) : 0u;
    const unsigned pick_blocks = dlc::capped_blocks(rows);
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    return rows_dispatch(dtype, [&](auto dt) { return pk_launch<dt.value>(ctx, a, chunk_blocks, pick_blocks, st); });
}
