// Ground-truth evaluation over score rows: dlc_pr_cell_counts and dlc_positive_rank_rows (include/dlc.h holds the
// definitions).  Both read a score matrix next to a truth mask of bytes once and count; every result is an integer, so
// nothing depends on the grid, the batching or the plan.
//
//   counts  the cell-level protocol.  A workgroup keeps the T threshold keys and a 2 x (T + 1) u32 histogram in LDS and
//           grid-strides over (row, chunk of 2048 columns) items: a lane takes eight cells 256 columns apart (coalesced
//           loads of the scores and of the mask bytes), finds each cell's bin by a binary search of the keys and adds one
//           to histogram[class][bin].  Real matrices put nearly every negative cell into a few bins, where same-address
//           LDS adds serialise: before the add a wave combines -- twice -- the lanes that share the first pending lane's
//           (class, bin) into one add of their number (ev_add).  A workgroup owns one row of u64 partials in the
//           workspace; it moves its histogram there at the end, and every EV_FLUSH_ITEMS items (2^31 cells) in between,
//           long before a u32 bin can wrap.  A second launch sums the partials into the outputs: no atomics on global
//           memory, no memset.
//   ranks   the retrieval protocol.  The best offered positive cell p of a row and the number of positives, then the
//           number of offered cells that beat p.  Rows short enough for one workgroup each (every row, once there are
//           2048 of them) take both passes in ONE launch, the second pass out of the cache; fewer, longer rows are cut
//           into slabs: best per slab, beat count per slab against the row's best, and a finish per row (three launches).
//
// A cell is topk_list.h's TlPair, as in peak_rows.hip: a KEY whose unsigned order is the order of merit (the ordered key
// of the fp64 value, or the biased int64, complemented when lower is better) and a TAG (~column << 32: larger = lower
// column).  a.before(b) is "a beats b".
#include "score_rows.h"
#include "topk_list.h"

namespace {

constexpr int EV_CELLS = 8;                       // cells of a lane per item
constexpr int EV_CHUNK = 256 * EV_CELLS;          // columns of an item of the count pass
constexpr int EV_MAX_T = 4096;
constexpr long long EV_BINS = 1ll << 21;          // the count pass: workgroups x (T + 1) stays below this (32 MiB of partials) ...
constexpr int EV_MIN_WG = 256, EV_MAX_WG = 2048;  // ... between these numbers of workgroups, ...
constexpr int EV_CELLS_PER_BIN = 16;              // ... and a workgroup has this many cells per bin it flushes, or there are fewer of them
constexpr long long EV_FLUSH_ITEMS = (1ll << 31) / EV_CHUNK;       // items between two flushes of the u32 histogram
constexpr int RK_TILE = 1024;                     // columns a slab of the rank pass is a multiple of
constexpr int RK_MAX_WG = 2048;                   // workgroups the slab passes aim at (rows x slabs)

struct EvMatrix {
    const void* M;
    const unsigned char* truth;
    long long rows, n, ld, ldt, limit0, limit_step, absent;
    int lower, has_absent;
};

// ---- counts ---------------------------------------------------------------------------------------------------------------
struct PrArgs {
    EvMatrix m;
    const void* thresholds;
    unsigned long long* part;                     // [workgroups][2][T + 1]
    long long nch, items;
    int T;
};

// hist[code] += 1 from every lane with code >= 0.  Two rounds of: the lanes whose code equals the first pending lane's
// become one add of their number.  What is left after that is spread over the bins and goes lane by lane.
__device__ __forceinline__ void ev_add(unsigned* hist, int code, int lane) {
    unsigned long long rest = __ballot(code >= 0);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (!rest) break;                                             // (the same in every lane)
        const int lead = __ffsll((long long)rest) - 1;
        const int c = __shfl(code, lead);
        const unsigned long long same = __ballot(code == c);
        if (lane == lead) atomicAdd(&hist[c], (unsigned)__popcll(same));
        rest &= ~same;
        if (code == c) code = -1;
    }
    if (code >= 0) atomicAdd(&hist[code], 1u);
}

template <int DT>
__global__ __launch_bounds__(256) void pr_count_kernel(const PrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ev_lds[];
    const int tid = threadIdx.x, lane = tid & 63, T = a.T, nb = 2 * (T + 1);
    unsigned long long* keys = ev_lds;                                // [T]
    unsigned* hist = (unsigned*)(ev_lds + T);                         // [2][T + 1]: negatives, then positives
    for (int i = tid; i < T; i += 256)
        keys[i] = DT == DLC_I64 ? (unsigned long long)((const long long*)a.thresholds)[i] ^ ROWS_SIGN
                                : dlc_f64_key(((const double*)a.thresholds)[i]);
    for (int i = tid; i < nb; i += 256) hist[i] = 0u;
    __syncthreads();
    int top = 1;                                                      // the largest power of two <= T
    while (top * 2 <= T) top *= 2;
    unsigned long long* P = a.part + (size_t)blockIdx.x * nb;         // this workgroup's partials: written here first, then added to
    bool first = true;
    auto flush = [&]() {
        __syncthreads();
        for (int i = tid; i < nb; i += 256) {
            const unsigned long long v = hist[i];
            P[i] = first ? v : P[i] + v;
            hist[i] = 0u;
        }
        first = false;
        __syncthreads();
    };
    long long since = 0;
    // (the trip counts are the workgroup's: every wave meets every barrier)
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long r = item / a.nch, j0 = (item % a.nch) * EV_CHUNK;
        const long long lim = dlc::row_limit(r, a.m.n, a.m.limit0, a.m.limit_step);
        if (j0 < lim) {
            unsigned long long x[EV_CELLS];
            int cls[EV_CELLS];                                        // -1: not offered, 0: negative, 1: positive
#pragma unroll
            for (int u = 0; u < EV_CELLS; ++u) {                      // (the loads are in flight together)
                const long long j = j0 + u * 256 + tid;
                x[u] = 0ull;
                cls[u] = -1;
                if (j < lim) {
                    const bool ok = rows_key<DT>(a.m.M, r * a.m.ld + j, a.m.has_absent, a.m.absent, x[u]);
                    const int pos = a.m.truth[r * a.m.ldt + j] != 0;
                    cls[u] = ok ? pos : -1;
                }
            }
            // b = #{i : t_i <= x} (t_i < x when lower is better); t <= T keeps b in 0..T whatever the keys hold.  The
            // eight searches go step by step together: eight independent LDS reads in flight, not one dependent chain
            int b[EV_CELLS];
#pragma unroll
            for (int u = 0; u < EV_CELLS; ++u) b[u] = 0;
            for (int s = top; s > 0; s >>= 1) {
#pragma unroll
                for (int u = 0; u < EV_CELLS; ++u) {
                    const int t = b[u] + s;
                    const unsigned long long k = keys[(t < T ? t : T) - 1];
                    if (t <= T && (a.m.lower ? k < x[u] : k <= x[u])) b[u] = t;
                }
            }
#pragma unroll
            for (int u = 0; u < EV_CELLS; ++u) ev_add(hist, cls[u] < 0 ? -1 : cls[u] * (T + 1) + b[u], lane);
        }
        if (++since == EV_FLUSH_ITEMS) { flush(); since = 0; }
    }
    flush();
}

__global__ __launch_bounds__(256) void pr_reduce_kernel(const unsigned long long* __restrict__ part, int G, int T,
                                                        long long* __restrict__ out_pos, long long* __restrict__ out_neg) {
    const int nb = 2 * (T + 1), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    unsigned long long s = 0ull;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * nb + i];
    if (i <= T) out_neg[i] = (long long)s;
    else out_pos[i - (T + 1)] = (long long)s;
}

// Workgroups of the count pass for `items` items at T thresholds: every one of them writes 2 (T + 1) partials that the
// second launch reads, which a small matrix must not pay more for than for itself.
inline int64_t pr_workgroups(int64_t items, int T) {
    int64_t cap = EV_BINS / (T + 1);
    cap = cap < EV_MIN_WG ? EV_MIN_WG : (cap > EV_MAX_WG ? EV_MAX_WG : cap);
    const int64_t worth = dlc::cdiv(items, dlc::cdiv((int64_t)EV_CELLS_PER_BIN * (T + 1), EV_CHUNK));
    return worth < cap ? worth : cap;
}

// ---- ranks ----------------------------------------------------------------------------------------------------------------
struct RkArgs {
    EvMatrix m;
    unsigned long long* ws;                       // [rows][G][4]: key, tag, positives, cells that beat the row's best
    long long G, cols_per_slab;
    long long *out_rank, *out_idx, *out_npos;
};

__device__ __forceinline__ TlPair rk_entry(const EvMatrix& m, unsigned long long key, long long j) {
    return {m.lower ? ~key : key, (unsigned long long)(~(unsigned)j) << 32};
}

__device__ __forceinline__ TlPair rk_wg_best(TlPair m, TlPair* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const TlPair o = m.shfl_xor(off);
        m = TlPair::pick(o.before(m), o, m);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    m = sh[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = TlPair::pick(sh[w].before(m), sh[w], m);
    __syncthreads();                                                  // (sh may be written again)
    return m;
}

__device__ __forceinline__ unsigned long long rk_wg_sum(unsigned long long v, unsigned long long* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return v;
}

// This thread's share of columns c0 .. c1 - 1 of row r: the best offered positive cell and the number of them.
template <int DT>
__device__ __forceinline__ void rk_scan_best(const EvMatrix& m, long long r, long long c0, long long c1, TlPair& best,
                                             unsigned long long& npos) {
    best = TlPair::empty();
    npos = 0ull;
    for (long long j0 = c0 + threadIdx.x; j0 < c1; j0 += 4 * 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long j = j0 + u * 256;
            unsigned long long key = 0ull;
            const bool pos = j < c1 && rows_key<DT>(m.M, r * m.ld + j, m.has_absent, m.absent, key) && m.truth[r * m.ldt + j] != 0;
            const TlPair e = rk_entry(m, key, j);
            best = TlPair::pick(pos && e.before(best), e, best);
            npos += pos ? 1ull : 0ull;
        }
    }
}

// This thread's share of columns c0 .. c1 - 1 of row r: the offered cells that beat p.
template <int DT>
__device__ __forceinline__ unsigned long long rk_scan_beat(const EvMatrix& m, long long r, long long c0, long long c1, TlPair p) {
    unsigned long long cnt = 0ull;
    for (long long j0 = c0 + threadIdx.x; j0 < c1; j0 += 4 * 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long j = j0 + u * 256;
            unsigned long long key = 0ull;
            const bool ok = j < c1 && rows_key<DT>(m.M, r * m.ld + j, m.has_absent, m.absent, key);
            cnt += ok && rk_entry(m, key, j).before(p) ? 1ull : 0ull;
        }
    }
    return cnt;
}

__device__ __forceinline__ void rk_emit(const RkArgs& a, long long r, TlPair best, unsigned long long npos, unsigned long long beat) {
    const bool none = best.is_empty();
    a.out_idx[r] = none ? -1ll : (long long)(~(unsigned)(best.tag >> 32));
    a.out_rank[r] = none ? -1ll : (long long)beat;
    a.out_npos[r] = (long long)npos;
}

// One workgroup per row, both passes.
template <int DT>
__global__ __launch_bounds__(256) void rank_rows_kernel(const RkArgs a) {
    __shared__ TlPair shb[4];
    __shared__ unsigned long long shs[4];
    for (long long r = blockIdx.x; r < a.m.rows; r += gridDim.x) {
        const long long lim = dlc::row_limit(r, a.m.n, a.m.limit0, a.m.limit_step);
        TlPair best;
        unsigned long long npos;
        rk_scan_best<DT>(a.m, r, 0, lim, best, npos);
        best = rk_wg_best(best, shb);
        npos = rk_wg_sum(npos, shs);
        unsigned long long beat = 0ull;
        if (!best.is_empty()) beat = rk_wg_sum(rk_scan_beat<DT>(a.m, r, 0, lim, best), shs);     // (the same in every thread)
        if (threadIdx.x == 0) rk_emit(a, r, best, npos, beat);
    }
}

// The slab passes: item = (row, slab g), the slab's columns [g * cols_per_slab, (g + 1) * cols_per_slab) below lim(r).
__device__ __forceinline__ void rk_slab(const RkArgs& a, long long item, long long& r, long long& g, long long& c0, long long& c1) {
    r = item / a.G;
    g = item % a.G;
    const long long lim = dlc::row_limit(r, a.m.n, a.m.limit0, a.m.limit_step);
    c0 = g * a.cols_per_slab;
    c1 = c0 + a.cols_per_slab < lim ? c0 + a.cols_per_slab : lim;
}

// The best of a row's slab entries and the sum of word `word` of them.
__device__ __forceinline__ TlPair rk_row_best(const RkArgs& a, long long r, TlPair* shb) {
    TlPair best = TlPair::empty();
    for (long long g = threadIdx.x; g < a.G; g += 256) {
        const TlPair v = {a.ws[(r * a.G + g) * 4], a.ws[(r * a.G + g) * 4 + 1]};
        best = TlPair::pick(v.before(best), v, best);
    }
    return rk_wg_best(best, shb);
}
__device__ __forceinline__ unsigned long long rk_row_sum(const RkArgs& a, long long r, int word, unsigned long long* shs) {
    unsigned long long s = 0ull;
    for (long long g = threadIdx.x; g < a.G; g += 256) s += a.ws[(r * a.G + g) * 4 + word];
    return rk_wg_sum(s, shs);
}

template <int DT>
__global__ __launch_bounds__(256) void rank_best_kernel(const RkArgs a) {
    __shared__ TlPair shb[4];
    __shared__ unsigned long long shs[4];
    for (long long item = blockIdx.x; item < a.m.rows * a.G; item += gridDim.x) {
        long long r, g, c0, c1;
        rk_slab(a, item, r, g, c0, c1);
        TlPair best;
        unsigned long long npos;
        rk_scan_best<DT>(a.m, r, c0, c1, best, npos);
        best = rk_wg_best(best, shb);
        npos = rk_wg_sum(npos, shs);
        if (threadIdx.x == 0) {
            unsigned long long* e = a.ws + item * 4;
            e[0] = best.key; e[1] = best.tag; e[2] = npos;
        }
    }
}

template <int DT>
__global__ __launch_bounds__(256) void rank_beat_kernel(const RkArgs a) {
    __shared__ TlPair shb[4];
    __shared__ unsigned long long shs[4];
    for (long long item = blockIdx.x; item < a.m.rows * a.G; item += gridDim.x) {
        long long r, g, c0, c1;
        rk_slab(a, item, r, g, c0, c1);
        const TlPair best = rk_row_best(a, r, shb);
        unsigned long long beat = 0ull;
        if (!best.is_empty()) beat = rk_wg_sum(rk_scan_beat<DT>(a.m, r, c0, c1, best), shs);     // (the same in every thread)
        if (threadIdx.x == 0) a.ws[item * 4 + 3] = beat;
    }
}

__global__ __launch_bounds__(256) void rank_finish_kernel(const RkArgs a) {
    __shared__ TlPair shb[4];
    __shared__ unsigned long long shs[4];
    for (long long r = blockIdx.x; r < a.m.rows; r += gridDim.x) {
        const TlPair best = rk_row_best(a, r, shb);
        const unsigned long long npos = rk_row_sum(a, r, 2, shs), beat = rk_row_sum(a, r, 3, shs);
        if (threadIdx.x == 0) rk_emit(a, r, best, npos, beat);
    }
}

template <int DT>
int rk_launch(dlc_ctx* ctx, const RkArgs& a, hipStream_t st) {
    const int64_t items = a.m.rows * a.G;
    const unsigned row_blocks = dlc::capped_blocks(a.m.rows);
    if (a.G == 1) {
        hipLaunchKernelGGL(rank_rows_kernel<DT>, dim3(row_blocks), dim3(256), 0, st, a);
        DLC_LAUNCH_CHECK(ctx, "rank_rows_kernel");
        return DLC_OK;
    }
    const unsigned blocks = dlc::capped_blocks(items);
    hipLaunchKernelGGL(rank_best_kernel<DT>, dim3(blocks), dim3(256), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "rank_best_kernel");
    hipLaunchKernelGGL(rank_beat_kernel<DT>, dim3(blocks), dim3(256), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "rank_beat_kernel");
    hipLaunchKernelGGL(rank_finish_kernel, dim3(row_blocks), dim3(256), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "rank_finish_kernel");
    return DLC_OK;
}

// The checks the two entry points share; DLC_OK: m is filled in.
int ev_matrix(dlc_ctx* ctx, const char* who, const ScoreRows& s, const uint8_t* truth, int64_t ld_truth, EvMatrix& m) {
    if (!truth) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: bad argument", who);
    if (ld_truth < s.n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld_truth=%lld < n=%lld", who, (long long)ld_truth, (long long)s.n);
    const int rc = rows_check(ctx, who, s, nullptr, DLC_ERR_BAD_SHAPE);
    if (rc != DLC_OK) return rc;
    rows_fill(m, s);
    m.truth = truth; m.rows = s.rows; m.ldt = ld_truth; m.absent = s.absent; m.lower = s.lower; m.has_absent = s.has_absent;
    return DLC_OK;
}

}  // namespace

extern "C" size_t dlc_pr_cell_counts_workspace_bytes(int64_t rows, int64_t n, int n_thresholds) {
    if (rows < 1 || n < 1 || n > 0x7fffffffll || n_thresholds < 1 || n_thresholds > EV_MAX_T) return 0;
    const int64_t nch = dlc::cdiv(n, EV_CHUNK);
    if (rows > (1ll << 62) / nch) return 0;
    return dlc::align_up((size_t)pr_workgroups(rows * nch, n_thresholds) * 2 * (size_t)(n_thresholds + 1) * 8, 256);
}

extern "C" int dlc_pr_cell_counts(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t n, int64_t ld,
                                  int64_t limit0, int64_t limit_step, int lower_is_better, int has_absent, int64_t absent,
                                  const uint8_t* truth, int64_t ld_truth, const void* thresholds, int n_thresholds,
                                  int64_t* out_pos, int64_t* out_neg, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    PrArgs a;
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, has_absent != 0, absent};
    const int rc = ev_matrix(ctx, "pr_cell_counts", s, truth, ld_truth, a.m);
    if (rc != DLC_OK) return rc;
    if (!thresholds || !out_pos || !out_neg) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pr_cell_counts: bad argument");
    if (n_thresholds < 1 || n_thresholds > EV_MAX_T)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pr_cell_counts: n_thresholds=%d outside 1..%d", n_thresholds, EV_MAX_T);
    if ((((uintptr_t)thresholds) & 7) || (((uintptr_t)out_pos) & 7) || (((uintptr_t)out_neg) & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "pr_cell_counts: thresholds and the outputs must be aligned to their element");
    const int wrc = rows_check_workspace(ctx, "pr_cell_counts", workspace, workspace_bytes,
                                 dlc_pr_cell_counts_workspace_bytes(rows, n, n_thresholds));
    if (wrc != DLC_OK) return wrc;
    const int T = n_thresholds;
    a.thresholds = thresholds; a.part = (unsigned long long*)workspace; a.T = T;
    // columns any row offers (limits are linear in the row, so the largest sits at an end); none: the sum of no partials
    const int64_t cols = dlc::max_row_limit(0, rows - 1, n, limit0, limit_step);
    a.nch = dlc::cdiv(cols, EV_CHUNK);
    a.items = rows * a.nch;                                           // (<= the items the workspace was sized by)
    const int64_t G = pr_workgroups(a.items, T);
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    if (G > 0) {
        const size_t lds = (size_t)T * 8 + 2 * (size_t)(T + 1) * 4;   // 65 544 bytes at T = 4096
        auto launch = [&](auto kern) -> int {
            if (lds > 64 * 1024)
                DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(256), lds, st, a);
            DLC_LAUNCH_CHECK(ctx, "pr_count_kernel");
            return DLC_OK;
        };
        const int lrc = rows_dispatch(dtype, [&](auto dt) { return launch(pr_count_kernel<dt.value>); });
        if (lrc != DLC_OK) return lrc;
    }
    hipLaunchKernelGGL(pr_reduce_kernel, dim3((unsigned)dlc::cdiv(2 * (T + 1), 256)), dim3(256), 0, st,
                       (const unsigned long long*)workspace, (int)G, T, (long long*)out_pos, (long long*)out_neg);
    DLC_LAUNCH_CHECK(ctx, "pr_reduce_kernel");
    return DLC_OK;
}

extern "C" size_t dlc_positive_rank_rows_workspace_bytes(int64_t rows, int64_t n) {
    if (rows < 1 || n < 1 || n > 0x7fffffffll) return 0;
    const int64_t G = dlc::max_slabs(rows, dlc::cdiv(n, RK_TILE), RK_MAX_WG);
    if (rows > (1ll << 56) / G) return 0;
    return dlc::align_up((size_t)rows * (size_t)G * 32, 256);
}

extern "C" int dlc_positive_rank_rows(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t n, int64_t ld,
                                      int64_t limit0, int64_t limit_step, int lower_is_better, int has_absent, int64_t absent,
                                      const uint8_t* truth, int64_t ld_truth, int64_t* out_rank, int64_t* out_idx,
                                      int64_t* out_npos, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    RkArgs a;
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, has_absent != 0, absent};
    const int rc = ev_matrix(ctx, "positive_rank_rows", s, truth, ld_truth, a.m);
    if (rc != DLC_OK) return rc;
    if (!out_rank || !out_idx || !out_npos) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "positive_rank_rows: bad argument");
    if ((((uintptr_t)out_rank) & 7) || (((uintptr_t)out_idx) & 7) || (((uintptr_t)out_npos) & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "positive_rank_rows: the outputs must be aligned to their element");
    const int wrc = rows_check_workspace(ctx, "positive_rank_rows", workspace, workspace_bytes,
                                 dlc_positive_rank_rows_workspace_bytes(rows, n));
    if (wrc != DLC_OK) return wrc;
    a.ws = (unsigned long long*)workspace; a.out_rank = (long long*)out_rank; a.out_idx = (long long*)out_idx;
    a.out_npos = (long long*)out_npos;
    const int64_t cols = dlc::max_row_limit(0, rows - 1, n, limit0, limit_step);
    dlc::SlabSplit slabs = {1, 1};                                    // nothing offered: the one-launch form writes (-1, -1, 0)
    if (cols > 0) slabs = dlc::split_slabs(rows, dlc::cdiv(cols, RK_TILE), RK_MAX_WG);
    a.G = slabs.G; a.cols_per_slab = slabs.tiles_per_slab * RK_TILE;  // (G <= the slabs the workspace was sized by)
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    return rows_dispatch(dtype, [&](auto dt) { return rk_launch<dt.value>(ctx, a, st); });
}
