// Sequence-consistent loop search (the trajectory search of SeqSLAM, Milford & Wyeth, ICRA 2012) over a dense score
// matrix, with the selection fused: dlc_sequence_topk (include/dlc.h).  The score of cell (r, j) along slope v is the sum
// of L frame scores on a line through it, M[r - s][j - off[v][s]], s = 0 .. L-1, added in that order; the cell's score is
// the best valid slope's, and a row's answer its k best cells.
//
//   scan   one workgroup per (block of rb output rows, slab of columns).  It walks the slab in tiles of ct columns; per
//          tile the (rb + L - 1) x (ct + max offset) window of the matrix is staged ONCE in LDS as fp64 / int64 (elements
//          outside the matrix or past their row's limit as NaN, so that a float sum through one is not valid without a
//          test per element), and every slope of every cell is formed from it: the rows come from HBM (rb + L - 1) / rb
//          times, not L x slopes times.  A wave owns rows w, w + 4, ... of the block and takes 64 columns at a time; a
//          cell that beats the row's k-th best so far is inserted into the row's sorted list, which sits in the wave's
//          registers while the wave is on that row (lane i holds entries i and 64 + i; an insertion is a shift by one
//          lane) and in LDS in between.  The slab's lists go to the workspace: [row][slab][k] entries.
//          Tables whose window does not fit in LDS (offsets of thousands of columns) read the matrix through the caches
//          instead: same arithmetic, same order.
//   merge  one workgroup per output row: the k best of its slabs' sorted lists.
//
// An entry is two words: a KEY whose unsigned order is the order of merit (larger = better: the ordered key of the fp64
// sum, or the biased int64 sum, complemented when lower is better) and a TAG (~column << 32 | slope; larger = lower
// column).  Entries of a row are distinct (the column is in them), so the result does not depend on the plan.  (0, 0) is
// the empty slot: below every entry, since a column < 2^31 leaves the tag's top bit set.
#include "sequence_merge.h"

namespace {

constexpr int SQ_SLAB_UNIT = 256;          // columns a slab is counted in
constexpr int SQ_MAX_RB = 32;              // output rows per workgroup, at most
constexpr size_t SQ_LDS_SMALL = 64 * 1024, SQ_LDS_LARGE = 150 * 1024;

struct SqArgs {
    const void* M;
    long long rows, row0, n, ld, limit0, limit_step, tiles_per_slab, ld_out;
    unsigned long long* part;              // [rows - row0][G][k][2]; NULL: no lists (dense output only)
    void* seq_out;
    const long long* poison;
    int L, V, maxoff, lower, k, rb, ct, wc;
};

template <int DT, bool STAGED>
__global__ __launch_bounds__(256) void sequence_scan_kernel(const SqArgs a, const SqOffsets offs) {
    constexpr bool IS_INT = DT == DLC_I64;
    extern __shared__ __attribute__((aligned(16))) char sq_smem[];
    const int L = a.L, rb = a.rb, k = a.k, wc = a.wc, ct = a.ct, maxoff = a.maxoff;
    const int wr = rb + L - 1;                                    // window rows: global rows rbase - (L-1) .. rbase + rb - 1
    unsigned long long* win = (unsigned long long*)sq_smem;       // [wr][wc], STAGED only
    unsigned long long* lkey = win + (STAGED ? (size_t)wr * wc : 0);   // [rb][k] the slab's lists so far
    unsigned long long* ltag = lkey + (a.part ? (size_t)rb * k : 0);
    int* lims = (int*)(ltag + (a.part ? (size_t)rb * k : 0));     // [wr] columns each window row offers (0: no such row)
    int* dtab = lims + wr;                                        // [V][L] window steps s * wc + off[v][s], STAGED only

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long rbase = a.row0 + (long long)blockIdx.x * rb;
    const long long G = gridDim.y, g = blockIdx.y;
    const bool poisoned = a.poison && *a.poison != 0;

    for (int i = tid; i < wr; i += 256) {
        const long long gr = rbase - (L - 1) + i;
        lims[i] = (gr < 0 || gr >= a.rows) ? 0 : (int)dlc::row_limit(gr, a.n, a.limit0, a.limit_step);
    }
    if (STAGED)
        for (int i = tid; i < a.V * L; i += 256) dtab[i] = (i % L) * wc + (int)offs.o[i];
    if (a.part)
        for (int lr = w; lr < rb; lr += 4)
            for (int i = lane; i < k; i += 64) { lkey[lr * k + i] = 0ull; ltag[lr * k + i] = 0ull; }
    // columns this block's rows may offer: limits are linear in the row, so the largest sits at an end.  The dense output
    // wants every column of the matrix (what is not offered is written as such).
    const long long rlast = (rbase + rb < a.rows ? rbase + rb : a.rows) - 1;
    const long long la = dlc::row_limit(rbase, a.n, a.limit0, a.limit_step), lb = dlc::row_limit(rlast, a.n, a.limit0, a.limit_step);
    const long long colend = (a.seq_out || poisoned) ? (a.seq_out ? a.n : 0) : (la > lb ? la : lb);
    const long long slab0 = g * a.tiles_per_slab * SQ_SLAB_UNIT;
    const long long slab1 = slab0 + a.tiles_per_slab * SQ_SLAB_UNIT < colend ? slab0 + a.tiles_per_slab * SQ_SLAB_UNIT : colend;
    __syncthreads();

    for (long long j0 = slab0; j0 < slab1; j0 += ct) {
        if (STAGED) {
            __syncthreads();                                      // the previous tile's reads are done
            for (int wrow = w; wrow < wr; wrow += 4) {
                const long long lim = lims[wrow];
                const long long base = (rbase - (L - 1) + wrow) * a.ld;
                for (int cc = lane; cc < wc; cc += 64) {
                    const long long c = j0 - maxoff + cc;
                    unsigned long long bits = IS_INT ? 0ull : (unsigned long long)ROWS_NAN_BITS;
                    if (c >= 0 && c < lim) bits = rows_bits<DT>(a.M, base + c);
                    win[(size_t)wrow * wc + cc] = bits;
                }
            }
            __syncthreads();
        }
        for (int lr = w; lr < rb; lr += 4) {
            const long long r = rbase + lr;
            if (r >= a.rows) break;
            WaveList<TlPair> wl;
            wl.clear();
            // lane s holds what element s of a line needs (read back with v_readlane: no memory access per element)
            const int lv = (STAGED && IS_INT && lane < L) ? lims[lr + L - 1 - lane] : 0;
            if (a.part) wl.load(k, lane, [&](int i) { return TlPair{lkey[lr * k + i], ltag[lr * k + i]}; });
            for (int ch = 0; ch < ct && j0 + ch < slab1; ch += 64) {
                const int jl = ch + lane;
                const long long j = j0 + jl;
                const bool active = j < slab1 && !poisoned;
                bool have = false;
                unsigned long long bk = 0ull;
                int bv = 0;
                for (int v = 0; v < a.V; ++v) {
                    const short* o = offs.o + v * L;
                    bool ok = true;
                    unsigned long long key;
                    if (STAGED && !IS_INT) {
                        const int dl = lane < L ? dtab[v * L + lane] : 0;
                        const unsigned long long* p = win + (size_t)(lr + L - 1) * wc + jl + maxoff;
                        auto el = [&](int t) { return __longlong_as_double((long long)p[-__builtin_amdgcn_readlane(dl, t)]); };
                        double acc = __longlong_as_double((long long)p[0]);
                        int s = 1;
                        for (; s + 4 <= L; s += 4) {              // four loads in flight, the additions in order
                            const double x0 = el(s), x1 = el(s + 1), x2 = el(s + 2), x3 = el(s + 3);
                            acc += x0; acc += x1; acc += x2; acc += x3;
                        }
                        for (; s < L; ++s) acc += el(s);
                        ok = acc == acc;
                        key = dlc_f64_key(acc);
                    } else if (STAGED) {
                        const int dl = lane < L ? dtab[v * L + lane] : 0;
                        const unsigned long long* p = win + (size_t)(lr + L - 1) * wc + jl + maxoff;
                        auto el = [&](int t) {
                            const int d = __builtin_amdgcn_readlane(dl, t);
                            const int jj = (int)j - (d - t * wc);
                            ok &= jj >= 0 && jj < __builtin_amdgcn_readlane(lv, t);
                            return p[-d];
                        };
                        unsigned long long acc = 0ull;
                        int s = 0;
                        for (; s + 4 <= L; s += 4) acc += (el(s) + el(s + 1)) + (el(s + 2) + el(s + 3));
                        for (; s < L; ++s) acc += el(s);
                        key = acc ^ ROWS_SIGN;
                    } else {
                        double facc = 0.0;                        // (sequence_chains_kernel sums the same way)
                        unsigned long long iacc = 0ull;
                        for (int s = 0; s < L; ++s) {
                            const long long jj = j - o[s];
                            const bool in = active && jj >= 0 && jj < lims[lr + L - 1 - s];
                            ok &= in;
                            const unsigned long long bits = in ? rows_bits<DT>(a.M, (r - s) * a.ld + jj)
                                                               : (IS_INT ? 0ull : (unsigned long long)ROWS_NAN_BITS);
                            if (IS_INT) iacc += bits;
                            else facc = s == 0 ? __longlong_as_double((long long)bits) : facc + __longlong_as_double((long long)bits);
                        }
                        if (!IS_INT) ok = facc == facc;
                        key = IS_INT ? (iacc ^ ROWS_SIGN) : dlc_f64_key(facc);
                    }
                    if (a.lower) key = ~key;
                    if (ok && (!have || key > bk)) { have = true; bk = key; bv = v; }
                }
                have = have && active;
                if (a.seq_out && j < slab1) {                      // (sq_store_dense, spelled out: docs/LAB.md 26)
                    const unsigned long long k2 = a.lower ? ~bk : bk;
                    const long long at = (r - a.row0) * a.ld_out + j;
                    if (IS_INT) ((long long*)a.seq_out)[at] = have ? (long long)(k2 ^ ROWS_SIGN) : -1ll;
                    else ((double*)a.seq_out)[at] = have ? dlc_f64_unkey(k2) : __longlong_as_double(ROWS_NAN_BITS);
                }
                if (a.part) {                                     // (the elastic scan offers the same way: docs/LAB.md 26)
                    const TlPair cand = {bk, ((unsigned long long)(~(unsigned)j) << 32) | (unsigned)bv};
                    for (unsigned long long todo = __ballot(have && cand.before(wl.kth)); todo; todo &= todo - 1) {
                        const TlPair x = cand.shfl(__ffsll((long long)todo) - 1);
                        if (x.before(wl.kth)) wl.insert(x, k, lane);      // (the k-th may have moved up since the ballot)
                    }
                }
            }
            if (a.part) wl.store(k, lane, [&](int i, TlPair e) { lkey[lr * k + i] = e.key; ltag[lr * k + i] = e.tag; });
        }
    }
    if (a.part)                                                   // (a wave writes the rows it owns: no barrier)
        for (int lr = w; lr < rb; lr += 4) {
            const long long r = rbase + lr;
            if (r >= a.rows) break;
            unsigned long long* P = a.part + (((size_t)(r - a.row0) * G + g) * k) * 2;
            for (int i = lane; i < k; i += 64) { P[2 * i] = lkey[lr * k + i]; P[2 * i + 1] = ltag[lr * k + i]; }
        }
}

// The scan's shape for a table: rows per block, columns per tile, staged or not, LDS bytes.
struct SqPlan { int rb, ct, staged; size_t lds; };
SqPlan sq_plan(int64_t rows_out, int L, int n_slopes, int maxoff, int k, bool lists, int rb_cap) {
    const size_t per_list = lists ? (size_t)k * 16 : 0, tab = (size_t)n_slopes * L * 4;
    const int want = rows_out < 8 ? (int)rows_out : 8;            // fewer rows per block than this: try a narrower tile
    const size_t budgets[2] = {SQ_LDS_SMALL, SQ_LDS_LARGE};
    const int cts[3] = {256, 128, 64};
    for (size_t budget : budgets)
        for (int ct : cts) {
            const size_t wc = (size_t)ct + maxoff, fixed = (size_t)(L - 1) * (wc * 8 + 4) + tab, per = wc * 8 + 4 + per_list;
            if (budget < fixed + per * want) continue;
            int64_t rb = (int64_t)((budget - fixed) / per);
            if (rb > rb_cap) rb = rb_cap;
            if (rb > rows_out) rb = rows_out;
            if (rb >= 4) rb &= ~(int64_t)3;                       // whole rounds of the four waves
            return {(int)rb, ct, 1, dlc::align_up(fixed + per * (size_t)rb, 16)};
        }
    int64_t rb = (int64_t)((SQ_LDS_SMALL - (size_t)(L - 1) * 4) / (per_list + 4));
    if (rb > rb_cap) rb = rb_cap;
    if (rb > rows_out) rb = rows_out;
    return {(int)rb, 256, 0, dlc::align_up((size_t)(L - 1) * 4 + (per_list + 4) * (size_t)rb, 16)};
}

}  // namespace

extern "C" size_t dlc_sequence_topk_workspace_bytes(int64_t rows, int64_t n, int L, int n_slopes, int k) {
    if (rows < 1 || n < 1 || n > 0x7fffffffll || L < 1 || L > SQ_MAX_L || n_slopes < 1 || n_slopes > SQ_MAX_SLOPES || k < 1 ||
        k > DLC_MAX_K)
        return 0;
    const int64_t slabs = dlc::max_slabs(dlc::cdiv(rows, SQ_MAX_RB), dlc::cdiv(n, SQ_SLAB_UNIT), TL_MAX_SLABS);
    return dlc::align_up((size_t)rows * (size_t)slabs * (size_t)k * 16, 256);
}

extern "C" int dlc_sequence_topk(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n, int64_t ld,
                                 int64_t limit0, int64_t limit_step, int L, int n_slopes, const int32_t* offsets,
                                 int lower_is_better, int k, void* out_scores, int64_t* out_idx, int32_t* out_slope,
                                 void* seq_out, int64_t ld_out, const int64_t* poison, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!offsets) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_topk: bad argument");
    if (L < 1 || L > SQ_MAX_L) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_topk: L=%d outside 1..%d", L, SQ_MAX_L);
    if (n_slopes < 1 || n_slopes > SQ_MAX_SLOPES)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sequence_topk: n_slopes=%d outside 1..%d", n_slopes, SQ_MAX_SLOPES);
    SqOffsets offs;
    int maxoff = 0;
    int rc = sq_pack_offsets(ctx, "sequence_topk", offsets, n_slopes, L, &offs, &maxoff);
    if (rc != DLC_OK) return rc;
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, lower_is_better != 0, 0, 0};
    SqArgs a;
    rc = sq_front(ctx, "sequence_topk", s, row0, L, k, out_scores, out_idx, out_slope, seq_out, ld_out, poison, workspace,
                  workspace_bytes, dlc_sequence_topk_workspace_bytes(rows, n, L, n_slopes, k), a);
    if (rc != DLC_OK) return rc;
    const int64_t rows_out = rows - row0;
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;

    // columns any output row offers (limits are linear in the row); the dense output covers the matrix's n columns
    const int64_t cols = seq_out ? n : dlc::max_row_limit(row0, rows - 1, n, limit0, limit_step);
    dlc::SlabSplit slabs = {1, 1};
    if (cols > 0) slabs = dlc::split_slabs(dlc::cdiv(rows, SQ_MAX_RB), dlc::cdiv(cols, SQ_SLAB_UNIT), TL_MAX_SLABS);
    // a few rows (a streamed batch): smaller row blocks, down to a row per wave, until the chip has a workgroup per CU --
    // the window's extra rows then come from L2, and a wave's serial chain of additions is what the call takes
    int rb_cap = SQ_MAX_RB;
    while (rb_cap > 4 && dlc::cdiv(rows_out, rb_cap) * slabs.G < 256) rb_cap /= 2;
    const SqPlan p = sq_plan(rows_out, L, n_slopes, maxoff, a.k, a.part != nullptr, rb_cap);
    a.tiles_per_slab = slabs.tiles_per_slab; a.V = n_slopes; a.maxoff = maxoff; a.rb = p.rb; a.ct = p.ct; a.wc = p.ct + maxoff;
    const int64_t blocks = dlc::cdiv(rows_out, p.rb);
    if (blocks > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sequence_topk: too many rows for one launch");
    auto launch = [&](auto kern) -> int {
        DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)slabs.G), dim3(256), p.lds, st, a, offs);
        DLC_LAUNCH_CHECK(ctx, "sequence_scan_kernel");
        return DLC_OK;
    };
    if (p.staged) rc = rows_dispatch(dtype, [&](auto dt) { return launch(sequence_scan_kernel<dt.value, true>); });
    else rc = rows_dispatch(dtype, [&](auto dt) { return launch(sequence_scan_kernel<dt.value, false>); });
    if (rc != DLC_OK) return rc;
    return sq_launch_merge(ctx, dtype, a, slabs.G, out_scores, out_idx, out_slope, st);
}
