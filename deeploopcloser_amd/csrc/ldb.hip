// A binary global place descriptor: the LDB code ("Local Difference Binary", Yang & Cheng, ISMAR 2012) of the whole
// down-sampled frame, as ABLE-M takes it (Arroyo et al., IROS 2015) -- dlc_ldb_describe_u8 (include/dlc.h holds the
// definition: the area resize, the grid levels, the quadrant sums S, DX, DY of a cell, the order of the bits).
//
//   one workgroup per frame, the thumbnail T [h, w] held in LDS as bytes, as seqslam_describe_kernel has it.
//     resize:     dlc_area_resize (dlc_hd.h), the one seqslam.hip calls.
//     quadrants:  a level of g x g cells is a grid of 2g x 2g quadrants; all levels' quadrants (4 sum g^2 <= 696 items) go
//                 to GROUPS of G lanes, G a power of two chosen by the host so that no lane idles, in at most LDB_PASSES
//                 passes.  The sums stay in registers until every lane has read T, then take its place in LDS: the
//                 thumbnail may fill the 64 KiB a workgroup gets without asking.
//     cells:      S, DX, DY of every cell from its four quadrants, one thread per cell.
//     bits:       lane l of a wave evaluates bit 64 i + l of the row and one ballot is 8 finished bytes, each stored by
//                 one lane: a byte of the row has exactly one writer.  A bit index is decoded in closed form -- the level
//                 by comparing with the levels' first bits, the pair (a, b) of the level by the triangular root.
//   Every trip count that holds a shuffle or a ballot is the workgroup's, so all lanes of a wave meet in it.
// Integers throughout: a function of the pixels alone, the same for every launch plan.
// This text also runs on the host (tests/host_sanitize/ldb): it includes nothing but dlc_internal.h and dlc_hd.h.
#include "dlc_internal.h"

namespace {

constexpr int LDB_THREADS = 256;
constexpr int LDB_MAX_CELLS = 65536;               // of the thumbnail
constexpr int64_t LDB_MAX_PIXELS = 1ll << 23;
constexpr int LDB_MAX_LEVELS = 4, LDB_MIN_GRID = 2, LDB_MAX_GRID = 8;
constexpr int LDB_MAX_QUADS = 4 * (25 + 36 + 49 + 64);      // of the four largest grids: 696
constexpr int LDB_PASSES = 3;                      // 256 / G groups a pass take every quadrant in at most this many (see the host)
constexpr int LDB_WORK_BYTES = LDB_MAX_QUADS * 4 + (LDB_MAX_QUADS / 4) * 3 * 4;     // quadrant sums, then (S, DX, DY) per cell
constexpr int LDB_NONE = 0x7fffffff;               // first bit / first quadrant of a level that is not there

struct LdbArgs {
    const uint8_t* gray;
    uint8_t* out;
    long long ld_out;
    int H, W, h, w;
    int g_resize, g_quad;                          // lanes per thumbnail cell, lanes per quadrant (powers of two, <= 64)
    int bits, row_bytes, quads;
    int grid[LDB_MAX_LEVELS];                      // g of a level
    int bit0[LDB_MAX_LEVELS];                      // its first bit (LDB_NONE past n_levels)
    int quad0[LDB_MAX_LEVELS];                     // its first quadrant, = 4 x its first cell (LDB_NONE past n_levels)
};

// sum over the G lanes of a group (G a power of two: the lanes lane ^ m, m < G, are the group)
__device__ __forceinline__ unsigned ldb_group_sum(unsigned v, int G) {
    for (int m = G >> 1; m; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}

// the level that holds item t, of the levels' first items (ascending, LDB_NONE where there is no level)
__device__ __forceinline__ int ldb_level(const int* first, int t) {
    return (int)(t >= first[1]) + (int)(t >= first[2]) + (int)(t >= first[3]);
}

__global__ __launch_bounds__(LDB_THREADS) void ldb_describe_kernel(const LdbArgs a) {
#if defined(__HIPCC__)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];            // max(h w, LDB_WORK_BYTES) bytes
#else
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDB_MAX_CELLS];      // (the host has no dynamic LDS)
#endif
    unsigned char* thumb = lds;                                    // T [h, w] ...
    unsigned* quad = (unsigned*)lds;                               // ... then, in its place, the quadrant sums
    int* cell = (int*)(lds + LDB_MAX_QUADS * 4);                   // ... and (S, DX, DY) of every cell
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* g = a.gray + (long long)blockIdx.x * a.H * a.W;

    dlc_area_resize(g, a.H, a.W, a.h, a.w, thumb, tid, LDB_THREADS, a.g_resize, [](unsigned v, int G) { return ldb_group_sum(v, G); });
    __syncthreads();

    // ---- quadrant sums: quadrant e of level lv is block (e / 2g, e % 2g) of the 2g x 2g grid of (h / 2g) x (w / 2g) pixels
    {
        const int G = a.g_quad, sub = tid & (G - 1), per = LDB_THREADS / G;
        unsigned keep[LDB_PASSES];
#pragma unroll
        for (int p = 0; p < LDB_PASSES; ++p) {
            const int item = p * per + tid / G;
            unsigned s = 0u;                                       // <= 255 h w / 16
            if (item < a.quads) {
                const int lv = ldb_level(a.quad0, item), e = item - a.quad0[lv], g2 = 2 * a.grid[lv];
                const int qh = a.h / g2, qw = a.w / g2, y0 = (e / g2) * qh, x0 = (e % g2) * qw;
                for (int i = sub; i < qh * qw; i += G) s += thumb[(y0 + i / qw) * a.w + x0 + i % qw];
            }
            keep[p] = ldb_group_sum(s, G);
        }
        __syncthreads();                                           // T has been read: its bytes are free
#pragma unroll
        for (int p = 0; p < LDB_PASSES; ++p) {
            const int item = p * per + tid / G;
            if (item < a.quads && sub == 0) quad[item] = keep[p];
        }
    }
    __syncthreads();

    // ---- cells: S = Q00 + Q01 + Q10 + Q11, DX = right - left, DY = bottom - top --------------------------------------------
    for (int c = tid; 4 * c < a.quads; c += LDB_THREADS) {
        const int lv = ldb_level(a.quad0, 4 * c), gg = a.grid[lv], g2 = 2 * gg, k = c - a.quad0[lv] / 4;
        const unsigned* q = quad + a.quad0[lv] + 2 * (k / gg) * g2 + 2 * (k % gg);
        const int q00 = (int)q[0], q01 = (int)q[1], q10 = (int)q[g2], q11 = (int)q[g2 + 1];
        cell[3 * c] = q00 + q01 + q10 + q11;
        cell[3 * c + 1] = (q01 + q11) - (q00 + q10);
        cell[3 * c + 2] = (q10 + q11) - (q00 + q01);
    }
    __syncthreads();

    // ---- bits: 3 per pair (a, b), a < b, of a level's cells; a ascending, then b ascending ---------------------------------
    uint8_t* o = a.out + (long long)blockIdx.x * a.ld_out;
    for (int i = wave; 8 * i < a.row_bytes; i += LDB_THREADS / 64) {
        const int t = 64 * i + lane;
        bool bit = false;
        if (t < a.bits) {
            const int lv = ldb_level(a.bit0, t), u = t - a.bit0[lv], pair = u / 3, comp = u - 3 * pair;
            const int n = a.grid[lv] * a.grid[lv];
            // counted from the last pair, row a = n - 2 - k holds the k + 1 pairs r = k (k + 1) / 2 .. : k is the
            // triangular root of r, floor((sqrt(8 r + 1) - 1) / 2) -- and right whatever the root's last bit does
            const int r = n * (n - 1) / 2 - 1 - pair;
            int k = (int)((__builtin_sqrtf((float)(8 * r + 1)) - 1.0f) * 0.5f);
            k -= (int)(k * (k + 1) / 2 > r);
            k += (int)((k + 1) * (k + 2) / 2 <= r);
            const int ca = n - 2 - k, cb = n - 1 - (r - k * (k + 1) / 2);
            const int* v = cell + 3 * (a.quad0[lv] / 4) + comp;
            bit = v[3 * ca] > v[3 * cb];
        }
        const unsigned long long word = __ballot(bit);
        if (lane < 8) o[8 * i + lane] = (uint8_t)(word >> (8 * lane));
    }
}

// bits of a level list, 0 for one that is not 1 to 4 grids, strictly ascending, each 2 .. 8
int64_t ldb_bits(const int* levels, int n_levels) {
    if (!levels || n_levels < 1 || n_levels > LDB_MAX_LEVELS) return 0;
    int64_t bits = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t n = (int64_t)levels[l] * levels[l];
        if (levels[l] < LDB_MIN_GRID || levels[l] > LDB_MAX_GRID || (l && levels[l] <= levels[l - 1])) return 0;
        bits += 3 * (n * (n - 1) / 2);
    }
    return bits;
}

}  // namespace

extern "C" int64_t dlc_ldb_row_bytes(const int* levels, int n_levels) {
    return 16 * dlc::cdiv(ldb_bits(levels, n_levels), 128);
}

extern "C" int dlc_ldb_describe_u8(dlc_ctx* ctx, const uint8_t* gray, int64_t frames, int H, int W, int h, int w,
                                   const int* levels, int n_levels, uint8_t* out, int64_t ld_out, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!gray || !out || !levels || frames < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "ldb_describe: bad argument");
    const int64_t bits = ldb_bits(levels, n_levels);
    if (!bits)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "ldb_describe: levels must be 1 to %d grids, strictly ascending, each %d..%d",
                         LDB_MAX_LEVELS, LDB_MIN_GRID, LDB_MAX_GRID);
    if (h < 1 || w < 1 || h > H || w > W)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "ldb_describe: thumbnail %d x %d outside 1 x 1 .. %d x %d", h, w, H, W);
    if ((int64_t)h * w > LDB_MAX_CELLS)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "ldb_describe: thumbnail %d x %d has more than %d cells", h, w, LDB_MAX_CELLS);
    if ((int64_t)H * W >= LDB_MAX_PIXELS)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "ldb_describe: frames of %d x %d pixels, 2^23 or more", H, W);
    for (int l = 0; l < n_levels; ++l)
        if (h % (2 * levels[l]) || w % (2 * levels[l]))
            return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "ldb_describe: 2 x %d does not divide the thumbnail %d x %d", levels[l], h, w);
    const int64_t row_bytes = 16 * dlc::cdiv(bits, 128);
    if (ld_out < row_bytes)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "ldb_describe: ld_out=%lld < row bytes=%lld", (long long)ld_out, (long long)row_bytes);
    if (frames > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "ldb_describe: frames must be below 2^31");
    DLC_ON_DEVICE(ctx);
    LdbArgs a;
    a.gray = gray; a.out = out; a.ld_out = ld_out;
    a.H = H; a.W = W; a.h = h; a.w = w;
    a.bits = (int)bits; a.row_bytes = (int)row_bytes;
    int bit0 = 0, quad0 = 0;
    for (int l = 0; l < LDB_MAX_LEVELS; ++l) {
        const int gg = l < n_levels ? levels[l] : 0, n = gg * gg;
        a.grid[l] = gg;
        a.bit0[l] = l < n_levels ? bit0 : LDB_NONE;
        a.quad0[l] = l < n_levels ? quad0 : LDB_NONE;
        bit0 += 3 * (n * (n - 1) / 2);
        quad0 += 4 * n;
    }
    a.quads = quad0;
    a.g_resize = dlc_lane_group(dlc::cdiv(LDB_THREADS, (int64_t)h * w));
    a.g_quad = dlc_lane_group(dlc::cdiv(LDB_THREADS, quad0));
    // (passes: fewer than 256 quadrants give G < 2 * 256 / quads, so 256 / G groups take them in two; more give G = 1 and
    // at most 696 / 256 -> LDB_PASSES)
    const size_t cells = (size_t)h * w;
    const size_t lds = dlc::align_up(cells > (size_t)LDB_WORK_BYTES ? cells : (size_t)LDB_WORK_BYTES, 16);
    hipLaunchKernelGGL(ldb_describe_kernel, dim3((unsigned)frames), dim3(LDB_THREADS), lds, (hipStream_t)stream, a);
    DLC_LAUNCH_CHECK(ctx, "ldb_describe_kernel");
    return DLC_OK;
}
