// SeqSLAM's local contrast normalisation of score rows (Milford & Wyeth, ICRA 2012, III-B): dlc_contrast_rows
// (include/dlc.h holds the definition -- the window, the order of every addition, the rounding).
//
//   one WAVE per (row, slab of 256 columns); a workgroup is four such waves on neighbouring slabs.  The wave stages its
//   slab and a halo on each side ONCE in LDS, converted to fp64, what lies outside [0, lim(r)) as -0.0: x + -0.0 = x for
//   every x, so a sum that runs over a clipped window's missing elements still "starts from x_a".  A lane owns four
//   consecutive cells and reads their 4 + 2 RB window elements into registers in one go (RB: the radius the kernel is
//   compiled for, 5, 16 or 32, the smallest that holds the call's) -- (4 + 2 RB) / 4 LDS reads per cell instead of
//   2 (2 RB + 1), which leaves the fp64 additions, the two divisions and the square root as what the kernel takes.
//   Each cell's window is then summed on its own, left to right, twice (sum, squared deviations), with every index a
//   constant.  A wave all of whose windows are whole and as wide as RB runs the sums without a test per element; any
//   other wave (a row's ends, a radius between two RBs) selects the identity (-0.0 / +0.0) for what is not in the window.
//   The four results of a lane go back through LDS so that the wave's stores are coalesced: 16 bytes per lane from the
//   first 16-byte aligned cell on, 8 bytes for the cell before it and at the row's limit.  Only offered cells are written.
#include "score_rows.h"

// every product and every sum rounded on its own (hipcc contracts a * b + c into an fma otherwise), as NumPy's are
#pragma clang fp contract(off)

namespace {

constexpr int CR_CELLS = 4;                    // consecutive cells of a lane
constexpr int CR_SLAB = 64 * CR_CELLS;         // columns of a wave
constexpr int CR_WAVES = 4;
constexpr int CR_MAX_RADIUS = 32;

struct CrArgs {
    const void* M;
    double* out;
    long long ld, ld_out, limit0, limit_step, items, slabs;
    long long n;
    int radius;
};

// The four cells of a lane from their 4 + 2 RB window elements x (x[c + t]: cell c's element t, its own at t = RB).
// tlo[c] .. thi[c]: the elements of cell c's window, looked at only when !WHOLE.
template <int RB, bool WHOLE>
__device__ __forceinline__ void cr_cells(const double (&x)[CR_CELLS + 2 * RB], const int (&tlo)[CR_CELLS], const int (&thi)[CR_CELLS],
                                         double (&y)[CR_CELLS]) {
#pragma unroll
    for (int c = 0; c < CR_CELLS; ++c) {
        auto in = [&](int t) { return WHOLE || (t >= tlo[c] && t <= thi[c]); };
        double s = in(0) ? x[c] : -0.0;
#pragma unroll
        for (int t = 1; t <= 2 * RB; ++t) s = s + (in(t) ? x[c + t] : -0.0);
        const int cnt = WHOLE ? 2 * RB + 1 : thi[c] - tlo[c] + 1;
        const double mean = s / (double)cnt;
        double q = 0.0;                                           // (a square is never -0.0: 0.0 + the first one is the first one)
#pragma unroll
        for (int t = 0; t <= 2 * RB; ++t) {
            const double d = x[c + t] - mean;
            const double d2 = d * d;
            q = q + (in(t) ? d2 : 0.0);
        }
        const double sd = __builtin_sqrt(q / (double)(cnt - 1));
        const double z = (x[c + RB] - mean) / sd;
        y[c] = (cnt < 2 || sd == 0.0) ? 0.0 : z;
    }
}

template <int DT, int RB>
__global__ __launch_bounds__(64 * CR_WAVES) void contrast_rows_kernel(const CrArgs a) {
    constexpr int HELD = CR_CELLS + 2 * RB, SEGW = CR_SLAB + 2 * RB;
    __shared__ __attribute__((aligned(16))) double seg[CR_WAVES][SEGW];      // columns slab0 - RB .. slab0 + 255 + RB
    __shared__ __attribute__((aligned(16))) double res[CR_WAVES][CR_SLAB];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (the trip count is the workgroup's: every wave meets every barrier)
    for (long long base = (long long)blockIdx.x * CR_WAVES; base < a.items; base += (long long)gridDim.x * CR_WAVES) {
        const long long item = base + w;
        const bool live = item < a.items;
        const long long r = live ? item / a.slabs : 0;
        const long long slab0 = live ? (item % a.slabs) * CR_SLAB : 0;
        const long long lim = live ? dlc::row_limit(r, a.n, a.limit0, a.limit_step) : 0;
        const bool work = slab0 < lim;                                     // the same in every lane of the wave
        __syncthreads();                                                   // the previous item's reads are done
        if (work) {
            const long long row = r * a.ld;
            for (int cc = lane; cc < SEGW; cc += 64) {
                const long long col = slab0 - RB + cc;
                double v = -0.0;
                if (col >= 0 && col < lim) v = rows_f64<DT>(a.M, row + col);
                seg[w][cc] = v;
            }
        }
        __syncthreads();
        if (work) {
            double x[HELD], y[CR_CELLS];
#pragma unroll
            for (int i = 0; i < HELD; ++i) x[i] = seg[w][lane * CR_CELLS + i];
            // columns to the left of the slab and to the right of its first cell, as far as a window can reach
            const int left = (int)(slab0 < CR_MAX_RADIUS ? slab0 : CR_MAX_RADIUS);
            const int right = (int)(lim - 1 - slab0 < CR_SLAB + CR_MAX_RADIUS ? lim - 1 - slab0 : CR_SLAB + CR_MAX_RADIUS);
            if (a.radius == RB && left >= RB && right >= CR_SLAB - 1 + RB) {
                const int none[CR_CELLS] = {0, 0, 0, 0};
                cr_cells<RB, true>(x, none, none, y);
            } else {
                int tlo[CR_CELLS], thi[CR_CELLS];
#pragma unroll
                for (int c = 0; c < CR_CELLS; ++c) {
                    const int jl = left + lane * CR_CELLS + c, jr = right - lane * CR_CELLS - c;     // min(., j), min(., lim - 1 - j)
                    tlo[c] = RB - (a.radius < jl ? a.radius : jl);
                    thi[c] = RB + (a.radius < jr ? a.radius : jr);
                }
                cr_cells<RB, false>(x, tlo, thi, y);
            }
#pragma unroll
            for (int c = 0; c < CR_CELLS; ++c) res[w][lane * CR_CELLS + c] = y[c];
        }
        __syncthreads();
        if (work) {
            double* o = a.out + r * a.ld_out + slab0;
            const int offered = (int)(lim - slab0 < CR_SLAB ? lim - slab0 : CR_SLAB);
            const int odd = (int)(((uintptr_t)o >> 3) & 1);                // cell 0 sits in the upper half of its 16 bytes
            if (odd && lane == 0) o[0] = res[w][0];
#pragma unroll
            for (int i = 0; i < CR_CELLS / 2; ++i) {
                const int e = odd + 2 * (lane + 64 * i);
                if (e + 1 < offered) {
                    double2 v;
                    v.x = res[w][e];
                    v.y = res[w][e + 1];
                    *(double2*)(o + e) = v;
                } else if (e < offered) {
                    o[e] = res[w][e];
                }
            }
        }
    }
}

template <int DT>
int cr_launch(dlc_ctx* ctx, const CrArgs& a, unsigned blocks, hipStream_t st) {
    if (a.radius <= 5) hipLaunchKernelGGL((contrast_rows_kernel<DT, 5>), dim3(blocks), dim3(64 * CR_WAVES), 0, st, a);
    else if (a.radius <= 16) hipLaunchKernelGGL((contrast_rows_kernel<DT, 16>), dim3(blocks), dim3(64 * CR_WAVES), 0, st, a);
    else hipLaunchKernelGGL((contrast_rows_kernel<DT, 32>), dim3(blocks), dim3(64 * CR_WAVES), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "contrast_rows_kernel");
    return DLC_OK;
}

}  // namespace

extern "C" int dlc_contrast_rows(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t n, int64_t ld,
                                 int64_t limit0, int64_t limit_step, int radius,
                                 double* out, int64_t ld_out, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!out || (((uintptr_t)out) & 7)) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "contrast_rows: out must be set and aligned to 8 bytes");
    if (radius < 1 || radius > CR_MAX_RADIUS)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "contrast_rows: radius=%d outside 1..%d", radius, CR_MAX_RADIUS);
    if (ld_out < n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "contrast_rows: ld_out=%lld < n=%lld", (long long)ld_out, (long long)n);
    const ScoreRows s = {dtype, scores, rows, n, ld, limit0, limit_step, 0, 0, 0};
    const int rc = rows_check(ctx, "contrast_rows", s, nullptr, DLC_ERR_BAD_SHAPE);
    if (rc != DLC_OK) return rc;
    // columns any row offers (limits are linear in the row, so the largest sits at an end)
    const int64_t cols = dlc::max_row_limit(0, rows - 1, n, limit0, limit_step);
    if (cols == 0) return DLC_OK;
    CrArgs a;
    rows_fill(a, s);
    a.out = out; a.ld_out = ld_out;
    a.slabs = dlc::cdiv(cols, CR_SLAB);
    if (rows > 0x7fffffffffffffffll / a.slabs) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "contrast_rows: rows * n too large");
    a.items = rows * a.slabs; a.radius = radius;
    const int64_t want = dlc::cdiv(a.items, CR_WAVES);
    const unsigned blocks = dlc::capped_blocks(want);
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    return rows_dispatch(dtype, [&](auto dt) { return cr_launch<dt.value>(ctx, a, blocks, st); });
}
