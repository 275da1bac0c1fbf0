// Place tracking over score rows -- a max-plus (Viterbi) filter whose states are the n key-frames and "no loop":
// dlc_track_rows and dlc_track_backtrace (include/dlc.h holds the definition).  Row r's state V_r(c) is one maximum
// over exact values -- the moves V_{r-1}(c - d), the jump from the previous row's best G_{r-1}, the no-loop state
// U_{r-1}, the origin -- and one addition of the cell; the rows depend on each other through V and through (G, g), a
// reduction over the whole row.  Two plans give the same bits:
//
//   RESIDENT  one workgroup of up to 1024 threads runs every row of the call in one launch.  V_{r-1} and V_r live in
//             two LDS buffers of n words (n <= DLC_TRACK_RESIDENT_MAX: 128 KiB), thread t owns columns t, t + T, ...
//             (at most 8), the cells of the next rows -- 8 cells per thread -- are in registers or on their way while a
//             row is worked out, the (value, column) reduction is a wave butterfly, one LDS slot per wave and ONE
//             barrier per row that waits for LDS alone (slots and V buffers alternate with the row's parity, so the
//             barrier that publishes row r also frees row r - 1).
//   ROWS      one launch per row, any n: workgroup b takes columns [b * tile, (b + 1) * tile) and reads V_{r-1} (its
//             tile and the d_max columns left of it) from the workspace; every workgroup first reduces the previous
//             row's per-workgroup (value, column) partials -- at most 1024, in a fixed order -- then writes its tile, its
//             back-pointers and its own partial.  No atomics; V alternates between two workspace buffers; a last
//             launch reduces the last row's partials and writes V and head back.
//
// "Best" is a total order (the merit key, then the lower column), so neither reduction's shape shows in the result.
#include <cmath>

#include "score_rows.h"

namespace {

constexpr long long TR_I64_ABSENT = (long long)0x8000000000000000ull;   // INT64_MIN: the absent mark of int64 state
constexpr int TR_THREADS = 1024;                                        // RESIDENT: the most threads of the workgroup
constexpr int TR_CPT = DLC_TRACK_RESIDENT_MAX / TR_THREADS;             // ... and the most columns of a thread
constexpr int TR_ROW_THREADS = 256;                                     // ROWS: threads of a workgroup
constexpr int TR_MAX_WG = 1024;                                         // ... and the most workgroups (partials) of a row
constexpr int TR_AUTO_RESIDENT_MAX = 3072;                              // AUTO: the RESIDENT plan up to this n (tr_plan)

struct TrArgs {
    const void* M;
    long long rows, n, ld, limit0, limit_step;
    int d_min, d_max, lower, null_on;
    long long jump, gate, null_score;          // fp64 bits, or the int64
    long long* V;                              // state, as bits
    long long* head;                           // rows seen, U, G, g
    long long *out_place, *out_g, *out_G, *out_U;
    signed char *out_backU, *out_back;
    long long ld_back;
    long long* dense;
    long long ld_dense;
    // ROWS
    long long* W[2];                           // V of the even / odd rows of the call
    unsigned long long* part;                  // [2][nwg][2]: (merit key, column or -1) of a workgroup, by the row's parity
    long long* ustate;                         // [2]: U by the row's parity
    long long nwg, tile;
};

template <int DT>
__device__ __forceinline__ long long tr_absent() { return DT == DLC_I64 ? TR_I64_ABSENT : ROWS_NAN_BITS; }

template <int DT>
__device__ __forceinline__ bool tr_present(long long b) {
    if (DT == DLC_I64) return b != TR_I64_ABSENT;
    const double v = __longlong_as_double(b);
    return v == v;
}

// The key whose unsigned order is the order of merit (larger = better) of a present value.
template <int DT>
__device__ __forceinline__ unsigned long long tr_mk(long long b, int lower) {
    const unsigned long long k = DT == DLC_I64 ? (unsigned long long)b ^ ROWS_SIGN : dlc_f64_key(__longlong_as_double(b));
    return lower ? ~k : k;
}
template <int DT>
__device__ __forceinline__ long long tr_unmk(unsigned long long mk, int lower) {
    const unsigned long long k = lower ? ~mk : mk;
    return DT == DLC_I64 ? (long long)(k ^ ROWS_SIGN) : __double_as_longlong(dlc_f64_unkey(k));
}

// predecessor + cell: the one addition (wrapping for int64); a NaN sum is the absent mark
template <int DT>
__device__ __forceinline__ long long tr_add(long long p, long long x) {
    if (DT == DLC_I64) return (long long)((unsigned long long)p + (unsigned long long)x);
    const double s = __longlong_as_double(p) + __longlong_as_double(x);
    return s == s ? __double_as_longlong(s) : ROWS_NAN_BITS;
}
// v worsened by the penalty p: v - p, v + p when lower is better
template <int DT>
__device__ __forceinline__ long long tr_worsen(long long v, long long p, int lower) {
    if (DT == DLC_I64)
        return (long long)(lower ? (unsigned long long)v + (unsigned long long)p : (unsigned long long)v - (unsigned long long)p);
    const double a = __longlong_as_double(v), b = __longlong_as_double(p);
    return __double_as_longlong(lower ? a + b : a - b);
}

struct TrCand { int have; unsigned long long mk; long long bits; };

template <int DT>
__device__ __forceinline__ TrCand tr_cand(bool have, long long bits, int lower) { return {have ? 1 : 0, tr_mk<DT>(bits, lower), bits}; }

// What a row's cells share: the three candidates that do not depend on the column, and the row's own no-loop state.
struct TrRow { TrCand jump, null, origin; long long U; int backU; };

template <int DT>
__device__ __forceinline__ TrRow tr_row(const TrArgs& a, long long U, long long G, bool first) {
    TrRow s;
    const bool hg = tr_present<DT>(G), hu = a.null_on && tr_present<DT>(U);
    s.jump = tr_cand<DT>(hg, tr_worsen<DT>(G, a.jump, a.lower), a.lower);
    s.null = tr_cand<DT>(hu, tr_worsen<DT>(U, a.gate, a.lower), a.lower);
    s.origin = tr_cand<DT>(first, 0ll, a.lower);
    TrCand q = tr_cand<DT>(hu, U, a.lower);                            // stay
    int code = hu ? 0 : DLC_TRACK_ABSENT;
    const TrCand leave = tr_cand<DT>(hg, tr_worsen<DT>(G, a.gate, a.lower), a.lower);
    if (leave.have && (!q.have || leave.mk > q.mk)) { q = leave; code = DLC_TRACK_JUMP; }
    if (s.origin.have && (!q.have || s.origin.mk > q.mk)) { q = s.origin; code = DLC_TRACK_ORIGIN; }
    s.U = tr_absent<DT>();
    s.backU = DLC_TRACK_ABSENT;
    if (a.null_on && q.have) {
        const long long u = tr_add<DT>(q.bits, a.null_score);
        if (tr_present<DT>(u)) { s.U = u; s.backU = code; }
    }
    return s;
}

// The cell rule for column c, offered, with the cell x: prev(j) = V_{r-1}(j) as bits, asked for 0 <= j <= c only.
template <int DT, class Prev>
__device__ __forceinline__ void tr_cell(const TrArgs& a, const TrRow& s, long long c, long long x, Prev prev, long long& v, int& code) {
    int have = 0, cd = DLC_TRACK_ABSENT;
    unsigned long long mk = 0ull;
    long long bits = 0ll;
    for (int d0 = a.d_min; d0 <= a.d_max && d0 <= c; d0 += 3) {       // lowest d first, strict compare; three reads in flight
        long long p[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) p[t] = prev(d0 + t <= c ? c - (d0 + t) : c);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const unsigned long long k = tr_mk<DT>(p[t], a.lower);
            if (d0 + t <= a.d_max && d0 + t <= c && tr_present<DT>(p[t]) && (!have || k > mk)) { have = 1; mk = k; bits = p[t]; cd = d0 + t; }
        }
    }
    if (s.jump.have && (!have || s.jump.mk > mk)) { have = 1; mk = s.jump.mk; bits = s.jump.bits; cd = DLC_TRACK_JUMP; }
    if (s.null.have && (!have || s.null.mk > mk)) { have = 1; mk = s.null.mk; bits = s.null.bits; cd = DLC_TRACK_FROM_NULL; }
    if (s.origin.have && (!have || s.origin.mk > mk)) { have = 1; mk = s.origin.mk; bits = s.origin.bits; cd = DLC_TRACK_ORIGIN; }
    v = tr_absent<DT>();
    code = DLC_TRACK_ABSENT;
    if (have) {
        const long long sum = tr_add<DT>(bits, x);
        if (tr_present<DT>(sum)) { v = sum; code = cd; }
    }
}

// The cell of row r, column c < lim as bits, and whether it is offered (a float NaN is not).
template <int DT>
__device__ __forceinline__ bool tr_load(const TrArgs& a, long long r, long long c, long long& x) {
    x = (long long)rows_bits<DT>(a.M, r * a.ld + c);
    return tr_present<DT>(x) || DT == DLC_I64;
}

// (merit key, column): the best present V of a set of columns; col = -1: none.
struct TrBest {
    unsigned long long mk;
    long long col;
    __device__ __forceinline__ void take(unsigned long long k, long long c) {
        if (c >= 0 && (col < 0 || k > mk || (k == mk && c < col))) { mk = k; col = c; }
    }
};

__device__ __forceinline__ TrBest tr_wave_best(TrBest b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) b.take(__shfl_xor(b.mk, off), __shfl_xor(b.col, off));
    return b;
}

// One row's outputs that wait for its reduction: G, g and the filtered place.
template <int DT>
__device__ __forceinline__ void tr_emit(const TrArgs& a, long long r, TrBest best, long long U, long long& G) {
    G = best.col >= 0 ? tr_unmk<DT>(best.mk, a.lower) : tr_absent<DT>();
    a.out_G[r] = G;
    if (a.out_g) a.out_g[r] = best.col;
    a.out_place[r] = best.col >= 0 && (!tr_present<DT>(U) || best.mk > tr_mk<DT>(U, a.lower)) ? best.col : -1ll;
}

// The workgroup's LDS writes are complete and visible to it; global loads and stores stay in flight across the barrier
// (the next rows' cells are on their way, the back-pointers need not have landed).
__device__ __forceinline__ void tr_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// CPT: the columns of a thread.  The cells of the next PF = 8 / CPT rows are in registers or on their way: a row costs
// a barrier and a few LDS round trips, far less than one trip to memory, so one row ahead would not hide it.
template <int DT, int CPT>
__global__ __launch_bounds__(TR_THREADS) void track_resident_kernel(const TrArgs a) {
    constexpr int PF = TR_CPT / CPT;
    extern __shared__ long long tr_lds[];                             // V of the odd rows, then of the even rows: 2 n words
    __shared__ TrBest slots[2][TR_THREADS / 64];
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = T >> 6;
    const long long n = a.n;
    bool first = a.head[0] == 0;
    long long U = first ? tr_absent<DT>() : a.head[1], G = first ? tr_absent<DT>() : a.head[2], g = first ? -1ll : a.head[3];
    for (long long c = tid; c < n; c += T) tr_lds[c] = first ? tr_absent<DT>() : a.V[c];   // row -1 is an odd row
    long long xq[PF][CPT];
    // row r's cells of this thread as bits, the absent mark at or past the row's limit (and past the call's rows);
    // nothing waits for them here
    auto load_row = [&](long long r, long long (&x)[CPT]) {
        const long long lim = r < a.rows ? dlc::row_limit(r, n, a.limit0, a.limit_step) : 0;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const long long c = tid + (long long)i * T;
            x[i] = c < lim ? (long long)rows_bits<DT>(a.M, r * a.ld + c) : tr_absent<DT>();
        }
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) load_row(k, xq[k]);
    tr_lds_barrier();
    for (long long r0 = 0; r0 < a.rows; r0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const long long r = r0 + k;
            if (r >= a.rows) break;
            const long long* prev = tr_lds + ((r & 1) ? n : 0);     // even rows read the odd buffer (the first n words)
            long long* cur = tr_lds + ((r & 1) ? 0 : n);
            const long long lim = dlc::row_limit(r, n, a.limit0, a.limit_step);
            long long x[CPT];
#pragma unroll
            for (int i = 0; i < CPT; ++i) x[i] = xq[k][i];
            load_row(r + PF, xq[k]);
            const TrRow s = tr_row<DT>(a, U, G, first);
            TrBest best = {0ull, -1ll};
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const long long c = tid + (long long)i * T;
                if (c < n) {
                    long long v = tr_absent<DT>();
                    int code = DLC_TRACK_ABSENT;
                    if (c < lim && (DT == DLC_I64 || tr_present<DT>(x[i])))
                        tr_cell<DT>(a, s, c, x[i], [&](long long j) { return prev[j]; }, v, code);
                    cur[c] = v;
                    if (a.out_back) a.out_back[r * a.ld_back + c] = (signed char)code;
                    if (a.dense) a.dense[r * a.ld_dense + c] = v;
                    if (code != DLC_TRACK_ABSENT) best.take(tr_mk<DT>(v, a.lower), c);
                }
            }
            best = tr_wave_best(best);
            if (lane == 0) slots[r & 1][w] = best;
            tr_lds_barrier();                                         // row r's V and slots are written; row r - 1's are free
            // every wave folds the (at most 16) slots in four steps, lane l starting from slot l & 15
            best = {0ull, -1ll};
            if ((lane & 15) < nw) best = slots[r & 1][lane & 15];
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) best.take(__shfl_xor(best.mk, off), __shfl_xor(best.col, off));
            U = s.U;
            first = false;
            g = best.col;
            if (tid == 0) {
                a.out_U[r] = U;
                a.out_backU[r] = (signed char)s.backU;
                tr_emit<DT>(a, r, best, U, G);
            } else {
                G = best.col >= 0 ? tr_unmk<DT>(best.mk, a.lower) : tr_absent<DT>();
            }
        }
    }
    const long long* last = tr_lds + (((a.rows - 1) & 1) ? 0 : n);
    for (long long c = tid; c < n; c += T) a.V[c] = last[c];
    if (tid == 0) { a.head[0] += a.rows; a.head[1] = U; a.head[2] = G; a.head[3] = g; }
}

// The workgroup's 256 threads' bests folded into every thread's (LDS slots; the caller's barrier discipline: one call per
// kernel, or a barrier between two).
__device__ __forceinline__ TrBest tr_block_best(TrBest b, TrBest* slots) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    b = tr_wave_best(b);
    if (lane == 0) slots[w] = b;
    __syncthreads();
    b = slots[0];
#pragma unroll
    for (int ww = 1; ww < TR_ROW_THREADS / 64; ++ww) b.take(slots[ww].mk, slots[ww].col);
    return b;
}

// The previous row's partials (parity p), reduced by the whole workgroup.
__device__ __forceinline__ TrBest tr_reduce_parts(const TrArgs& a, int p, TrBest* slots) {
    TrBest b = {0ull, -1ll};
    const unsigned long long* part = a.part + (long long)p * a.nwg * 2;
    for (long long i = threadIdx.x; i < a.nwg; i += TR_ROW_THREADS) b.take(part[2 * i], (long long)part[2 * i + 1]);
    return tr_block_best(b, slots);
}

template <int DT>
__global__ __launch_bounds__(TR_ROW_THREADS) void track_row_kernel(const TrArgs a, const long long r) {
    __shared__ TrBest slots_prev[TR_ROW_THREADS / 64], slots_own[TR_ROW_THREADS / 64];
    const int tid = threadIdx.x;
    const long long n = a.n;
    const bool first = r == 0 && a.head[0] == 0;
    long long U, G;
    if (r == 0) {
        U = first ? tr_absent<DT>() : a.head[1];
        G = first ? tr_absent<DT>() : a.head[2];
    } else {
        const TrBest pb = tr_reduce_parts(a, (int)((r - 1) & 1), slots_prev);
        U = a.ustate[(r - 1) & 1];
        if (blockIdx.x == 0 && tid == 0) tr_emit<DT>(a, r - 1, pb, U, G);
        else G = pb.col >= 0 ? tr_unmk<DT>(pb.mk, a.lower) : tr_absent<DT>();
    }
    const TrRow s = tr_row<DT>(a, U, G, first);
    if (blockIdx.x == 0 && tid == 0) {
        a.out_U[r] = s.U;
        a.out_backU[r] = (signed char)s.backU;
        a.ustate[r & 1] = s.U;
    }
    const long long* prev = r == 0 ? a.V : a.W[(r - 1) & 1];          // (a fresh state: no predecessor is present, V is not read)
    long long* cur = a.W[r & 1];
    const long long lim = dlc::row_limit(r, n, a.limit0, a.limit_step);
    const long long c0 = (long long)blockIdx.x * a.tile, c1 = c0 + a.tile < n ? c0 + a.tile : n;
    TrBest best = {0ull, -1ll};
    for (long long c = c0 + tid; c < c1; c += TR_ROW_THREADS) {
        long long v = tr_absent<DT>(), x = 0ll;
        int code = DLC_TRACK_ABSENT;
        if (c < lim && tr_load<DT>(a, r, c, x))
            tr_cell<DT>(a, s, c, x, [&](long long j) { return first ? tr_absent<DT>() : prev[j]; }, v, code);
        cur[c] = v;
        if (a.out_back) a.out_back[r * a.ld_back + c] = (signed char)code;
        if (a.dense) a.dense[r * a.ld_dense + c] = v;
        if (code != DLC_TRACK_ABSENT) best.take(tr_mk<DT>(v, a.lower), c);
    }
    best = tr_block_best(best, slots_own);
    if (tid == 0) {
        unsigned long long* part = a.part + ((r & 1) * a.nwg + blockIdx.x) * 2;
        part[0] = best.mk;
        part[1] = (unsigned long long)best.col;
    }
}

// After the last row: its G, g and place, head, and V out of the workspace.
template <int DT>
__global__ __launch_bounds__(TR_ROW_THREADS) void track_finish_kernel(const TrArgs a) {
    __shared__ TrBest slots[TR_ROW_THREADS / 64];
    const long long r = a.rows - 1;
    const long long* last = a.W[r & 1];
    for (long long c = (long long)blockIdx.x * TR_ROW_THREADS + threadIdx.x; c < a.n; c += (long long)gridDim.x * TR_ROW_THREADS)
        a.V[c] = last[c];
    if (blockIdx.x == 0) {
        const TrBest pb = tr_reduce_parts(a, (int)(r & 1), slots);
        if (threadIdx.x == 0) {
            const long long U = a.ustate[r & 1];
            long long G;
            tr_emit<DT>(a, r, pb, U, G);
            a.head[0] += a.rows; a.head[1] = U; a.head[2] = G; a.head[3] = pb.col;
        }
    }
}

// One wave walks the pointers from the last row to row 0; lane i keeps row lo + i of the current 64 rows: its no-loop
// pointer, the g of the row before it and, at the end, its state.
__global__ __launch_bounds__(64) void track_backtrace_kernel(long long rows, long long n, const signed char* back, long long ld_back,
                                                             const signed char* backU, const long long* g,
                                                             const long long* place_last, long long end, long long* path) {
    const int lane = threadIdx.x;
    long long s = end == DLC_TRACK_END_FILTERED ? *place_last : end;
    bool dead = s < -1 || s >= n;
    for (long long hi = rows; hi > 0; hi -= 64) {
        const long long lo = hi > 64 ? hi - 64 : 0, row = lo + lane;
        const int bu = row < hi ? (int)backU[row] : DLC_TRACK_ABSENT;
        const long long gp = row < hi && row > 0 ? g[row - 1] : -1ll;
        long long mine = DLC_TRACK_NO_PATH;
        for (long long r = hi - 1; r >= lo; --r) {                    // (s and dead are the same in every lane)
            if (dead) break;
            const int j = (int)(r - lo);
            const int code = s >= 0 ? (int)back[r * ld_back + s] : __shfl(bu, j);
            const long long gprev = __shfl(gp, j);
            if (code == DLC_TRACK_ABSENT) { dead = true; break; }     // not a state of this row
            if (lane == j) mine = s;
            if (code == DLC_TRACK_ORIGIN) dead = r > 0;               // the first row ever seen
            else if (code == DLC_TRACK_JUMP) s = gprev;
            else if (code == DLC_TRACK_FROM_NULL) s = s >= 0 ? -1ll : -2ll;
            else if (code >= 0) s = s >= 0 ? s - code : (code == 0 ? -1ll : -2ll);
            else s = -2ll;
            if (r > 0 && (s < -1 || s >= n)) dead = true;             // (pointers that are not this call's: nothing is read)
        }
        if (row < hi) path[row] = mine;
    }
}

struct TrPlan { int plan; long long nwg, tile; size_t v_bytes, part_bytes, total; };

// AUTO (docs/LAB.md 27): a row of the RESIDENT plan costs about 2.5 us (the barrier, the two reductions, the row's shared
// candidates) + 1.1 us per 1024 columns, a row of the ROWS plan one launch, 6.6 us at every n measured; 3072 is the
// largest measured n at which RESIDENT is the faster (5.9 against 6.6 us), at 4096 it is the slower (7.0 against 6.7).
inline TrPlan tr_plan(int64_t rows, int64_t n, int plan) {
    TrPlan p = {plan, 0, 0, 0, 0, 256};
    if (plan == DLC_TRACK_AUTO) p.plan = n <= TR_AUTO_RESIDENT_MAX ? DLC_TRACK_RESIDENT : DLC_TRACK_ROWS;
    if (p.plan == DLC_TRACK_ROWS) {
        const long long cpt = dlc::cdiv(n, (int64_t)TR_ROW_THREADS * TR_MAX_WG);
        p.tile = cpt * TR_ROW_THREADS;
        p.nwg = dlc::cdiv(n, p.tile);
        p.v_bytes = dlc::align_up((size_t)n * 8, 256);
        p.part_bytes = dlc::align_up((size_t)p.nwg * 2 * 2 * 8, 256);
        p.total = 2 * p.v_bytes + p.part_bytes + 256;
    }
    return p;
}

inline bool tr_is_int53(double v) { return v == std::floor(v) && std::fabs(v) <= 9007199254740992.0; }

inline long long tr_bits(int dtype, double v) {
    if (dtype == DLC_I64) return (long long)v;
    long long b;
    memcpy(&b, &v, 8);
    return b;
}

template <int DT>
int tr_launch(dlc_ctx* ctx, const TrArgs& a, const TrPlan& p, hipStream_t st) {
    if (p.plan == DLC_TRACK_RESIDENT) {
        const size_t lds = (size_t)a.n * 16;
        long long threads = dlc::cdiv(a.n, 64) * 64;
        if (threads > TR_THREADS) threads = TR_THREADS;
        const long long cpt = dlc::cdiv(a.n, threads);
        auto launch = [&](auto kern, int slot) -> int {               // (only the two widest forms pass 48 KiB of LDS)
            const int bit = DLC_ATTR_TRACK_BASE + (DT == DLC_F64 ? 0 : DT == DLC_F32 ? 1 : 2) * 2 + slot;
            if (lds > 48 * 1024 && !(ctx->func_attr_set & (1ull << bit))) {
                DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       DLC_TRACK_RESIDENT_MAX * 16));
                ctx->func_attr_set |= 1ull << bit;
            }
            hipLaunchKernelGGL(kern, dim3(1), dim3((unsigned)threads), lds, st, a);
            DLC_LAUNCH_CHECK(ctx, "track_resident_kernel");
            return DLC_OK;
        };
        if (cpt <= 1) return launch(track_resident_kernel<DT, 1>, 0);
        if (cpt <= 2) return launch(track_resident_kernel<DT, 2>, 0);
        if (cpt <= 4) return launch(track_resident_kernel<DT, 4>, 0);
        return launch(track_resident_kernel<DT, 8>, 1);
    }
    for (long long r = 0; r < a.rows; ++r) {
        hipLaunchKernelGGL(track_row_kernel<DT>, dim3((unsigned)a.nwg), dim3(TR_ROW_THREADS), 0, st, a, r);
        DLC_LAUNCH_CHECK(ctx, "track_row_kernel");
    }
    const long long copy_wg = dlc::cdiv(a.n, (int64_t)TR_ROW_THREADS * 4);
    hipLaunchKernelGGL(track_finish_kernel<DT>, dim3((unsigned)(copy_wg < TR_MAX_WG ? copy_wg : TR_MAX_WG)), dim3(TR_ROW_THREADS), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "track_finish_kernel");
    return DLC_OK;
}

}  // namespace

extern "C" size_t dlc_track_rows_workspace_bytes(int64_t rows, int64_t n, int plan) {
    if (rows < 1 || n < 1 || n > 0x7fffffffll || plan < DLC_TRACK_AUTO || plan > DLC_TRACK_ROWS) return 0;
    if (plan == DLC_TRACK_RESIDENT && n > DLC_TRACK_RESIDENT_MAX) return 0;
    return tr_plan(rows, n, plan).total;
}

extern "C" int dlc_track_rows(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t n, int64_t ld, int64_t limit0,
                              int64_t limit_step, int d_min, int d_max, int lower_is_better, double jump, double gate,
                              double null_score, int plan, void* V, int64_t* head, int64_t* out_place, int64_t* out_g, void* out_G,
                              void* out_U, int8_t* out_backU, int8_t* out_back, int64_t ld_back, void* dense, int64_t ld_dense,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    const char* who = "track_rows";
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, 0, 0};
    int rc = rows_check(ctx, who, s, nullptr, DLC_ERR_BAD_SHAPE);
    if (rc != DLC_OK) return rc;
    if (d_min < 0 || d_min > d_max || d_max > DLC_MAX_STEP)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: steps %d..%d outside 0 <= d_min <= d_max <= %d", who, d_min, d_max, DLC_MAX_STEP);
    if (!std::isfinite(jump) || !std::isfinite(gate) || jump < 0 || gate < 0)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: jump and gate must be finite and not negative", who);
    const bool null_on = !std::isnan(null_score);
    if (dtype == DLC_I64 && (!tr_is_int53(jump) || !tr_is_int53(gate) || (null_on && !tr_is_int53(null_score))))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: with DLC_I64 jump, gate and null_score are integers of magnitude <= 2^53", who);
    if (plan < DLC_TRACK_AUTO || plan > DLC_TRACK_ROWS)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: plan=%d is none of DLC_TRACK_AUTO, _RESIDENT, _ROWS", who, plan);
    const void* words[] = {V, head, out_place, out_G, out_U, out_g, dense};
    for (int i = 0; i < 7; ++i)
        if ((i < 5 && !words[i]) || (((uintptr_t)words[i]) & 7))
            return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: V, head, out_place, out_G and out_U must be set, and every 8-byte output aligned", who);
    if (!out_backU) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: out_backU must be set", who);
    if (out_back && ld_back < n)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld_back=%lld < n=%lld", who, (long long)ld_back, (long long)n);
    if (dense && ld_dense < n)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld_dense=%lld < n=%lld", who, (long long)ld_dense, (long long)n);
    if (plan == DLC_TRACK_RESIDENT && n > DLC_TRACK_RESIDENT_MAX)
        return dlc::fail(ctx, DLC_ERR_UNSUPPORTED, "%s: the RESIDENT plan takes n <= %d, n=%lld", who, DLC_TRACK_RESIDENT_MAX, (long long)n);
    const TrPlan p = tr_plan(rows, n, plan);
    if (p.plan == DLC_TRACK_ROWS) {
        rc = rows_check_workspace(ctx, who, workspace, workspace_bytes, p.total);
        if (rc != DLC_OK) return rc;
    }
    TrArgs a;
    rows_fill(a, s);
    a.rows = rows; a.d_min = d_min; a.d_max = d_max; a.lower = s.lower; a.null_on = null_on;
    a.jump = tr_bits(dtype, jump); a.gate = tr_bits(dtype, gate); a.null_score = null_on ? tr_bits(dtype, null_score) : 0;
    a.V = (long long*)V; a.head = (long long*)head; a.out_place = (long long*)out_place; a.out_g = (long long*)out_g;
    a.out_G = (long long*)out_G; a.out_U = (long long*)out_U; a.out_backU = (signed char*)out_backU;
    a.out_back = (signed char*)out_back; a.ld_back = ld_back; a.dense = (long long*)dense; a.ld_dense = ld_dense;
    a.W[0] = a.W[1] = nullptr; a.part = nullptr; a.ustate = nullptr; a.nwg = p.nwg; a.tile = p.tile;
    if (p.plan == DLC_TRACK_ROWS) {
        char* w = (char*)workspace;
        a.W[0] = (long long*)w; a.W[1] = (long long*)(w + p.v_bytes);
        a.part = (unsigned long long*)(w + 2 * p.v_bytes);
        a.ustate = (long long*)(w + 2 * p.v_bytes + p.part_bytes);
    }
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    return rows_dispatch(dtype, [&](auto dt) { return tr_launch<dt.value>(ctx, a, p, st); });
}

extern "C" int dlc_track_backtrace(dlc_ctx* ctx, int64_t rows, int64_t n, const int8_t* out_back, int64_t ld_back,
                                   const int8_t* out_backU, const int64_t* g, const int64_t* place_last, int64_t end,
                                   int64_t* out_path, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    const char* who = "track_backtrace";
    if (rows < 1 || n < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: bad argument", who);
    if (n > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: n must be below 2^31", who);
    if (!out_back || !out_backU || !g || !out_path || (((uintptr_t)g) & 7) || (((uintptr_t)out_path) & 7) || (((uintptr_t)place_last) & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: the pointers must be set and aligned to their element", who);
    if (ld_back < n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld_back=%lld < n=%lld", who, (long long)ld_back, (long long)n);
    if (end == DLC_TRACK_END_FILTERED ? !place_last : (end < -1 || end >= n))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: end=%lld is no column, -1 or DLC_TRACK_END_FILTERED with place_last", who,
                         (long long)end);
    DLC_ON_DEVICE(ctx);
    hipLaunchKernelGGL(track_backtrace_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)rows, (long long)n,
                       (const signed char*)out_back, (long long)ld_back, (const signed char*)out_backU, (const long long*)g,
                       (const long long*)place_last, (long long)end, (long long*)out_path);
    DLC_LAUNCH_CHECK(ctx, "track_backtrace_kernel");
    return DLC_OK;
}
