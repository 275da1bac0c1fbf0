// SeqSLAM's image descriptor (Milford & Wyeth, ICRA 2012, III-A): a grey frame down-sampled to a thumbnail and
// patch-normalised -- dlc_seqslam_describe_u8 (include/dlc.h holds the definition: the integer area resize, the tiles,
// the three fp64 operations of a cell).
//
//   one workgroup per frame, the thumbnail T [h, w] held in LDS as bytes (h * w <= 65536: at most the 64 KiB a workgroup
//   gets without asking).  Both phases hand their items (a thumbnail cell, then a tile) to GROUPS of G lanes, G a power
//   of two chosen by the host so that no lane idles where there is work: a group's lanes walk the item's elements G
//   apart and their partial sums meet in a butterfly of shuffles.  The sums are integers, so the order is free.
//     resize:     cell (y, x) sums wy * wx * gray over its footprint of source pixels; G = 1 for any ordinary ratio
//                 (2048 cells of 35 pixels at 192 x 240 -> 32 x 64), larger only when the thumbnail has fewer cells than
//                 the workgroup has lanes.
//     normalise:  tile (y0, x0) sums T and T * T over its c cells, then each lane writes its cells' bytes;
//                 G = the power of two at or above patch^2, at most a wave.
//   Every trip count that holds a shuffle is the workgroup's, so all lanes of a wave meet in it.
#include "dlc_internal.h"

// (strength * u) * v: the product rounded once, no fma with what surrounds it
#pragma clang fp contract(off)

namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_MAX_CELLS = 65536;
constexpr int64_t SD_MAX_PIXELS = 1ll << 23;

struct SdArgs {
    const uint8_t* gray;
    uint8_t* out;
    long long ld_out;
    int H, W, h, w, patch, strength;
    int g_resize, g_tile;                          // lanes per thumbnail cell, lanes per tile (powers of two, <= 64)
};

// sum over the G lanes of a group (G a power of two: the lanes lane ^ m, m < G, are the group)
__device__ __forceinline__ unsigned sd_group_sum(unsigned v, int G) {
    for (int m = G >> 1; m; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}

__global__ __launch_bounds__(SD_THREADS) void seqslam_describe_kernel(const SdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char thumb[];          // T [h, w]
    const int tid = threadIdx.x;
    const uint8_t* g = a.gray + (long long)blockIdx.x * a.H * a.W;

    // ---- area resize: T(y, x) = floor((2 sum wy wx gray + H W) / (2 H W)) (dlc_hd.h) ------------------------------------
    dlc_area_resize(g, a.H, a.W, a.h, a.w, thumb, tid, SD_THREADS, a.g_resize, [](unsigned v, int G) { return sd_group_sum(v, G); });
    __syncthreads();

    // ---- patch normalisation: 128 + strength (T - mean) / sample std, tile by tile ---------------------------------------
    {
        const int G = a.g_tile, sub = tid & (G - 1), per = SD_THREADS / G;
        const int ty_n = (a.h + a.patch - 1) / a.patch, tx_n = (a.w + a.patch - 1) / a.patch, tiles = ty_n * tx_n;
        uint8_t* o = a.out + (long long)blockIdx.x * a.ld_out;
        for (int base = 0; base < tiles; base += per) {
            const int tile = base + tid / G;
            const bool live = tile < tiles;
            const int y0 = live ? (tile / tx_n) * a.patch : 0, x0 = live ? (tile % tx_n) * a.patch : 0;
            const int th = a.h - y0 < a.patch ? a.h - y0 : a.patch, tw = a.w - x0 < a.patch ? a.w - x0 : a.patch;
            const int c = live ? th * tw : 0;                      // <= 4096
            unsigned s = 0u, t = 0u;                               // <= 255 c, <= 255^2 c < 2^29
            for (int e = sub; e < c; e += G) {
                const unsigned v = thumb[(y0 + e / tw) * a.w + x0 + e % tw];
                s += v;
                t += v * v;
            }
            s = sd_group_sum(s, G);
            t = sd_group_sum(t, G);
            const long long qv = (long long)c * (long long)t - (long long)s * (long long)s;      // c^2 x the variance's numerator
            const bool flat = c < 2 || qv == 0;
            const double v = flat ? 0.0 : __builtin_sqrt((double)(c - 1) / ((double)c * (double)qv));
            for (int e = sub; e < c; e += G) {
                const int at = (y0 + e / tw) * a.w + x0 + e % tw;
                int b = 128;
                if (!flat) {
                    const double u = (double)(c * (int)thumb[at] - (int)s);
                    const double z = __builtin_rint(((double)a.strength * u) * v);
                    const double r = 128.0 + z;                    // |z| <= 127 * 64: exact
                    b = r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r);
                }
                o[at] = (uint8_t)b;
            }
        }
    }
}

}  // namespace

extern "C" int dlc_seqslam_describe_u8(dlc_ctx* ctx, const uint8_t* gray, int64_t frames, int H, int W, int h, int w,
                                       int patch, int strength, uint8_t* out, int64_t ld_out, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!gray || !out || frames < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "seqslam_describe: bad argument");
    if (patch < 1 || patch > 64) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "seqslam_describe: patch=%d outside 1..64", patch);
    if (strength < 1 || strength > 127)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "seqslam_describe: strength=%d outside 1..127", strength);
    if (h < 1 || w < 1 || h > H || w > W)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "seqslam_describe: thumbnail %d x %d outside 1 x 1 .. %d x %d", h, w, H, W);
    if ((int64_t)h * w > SD_MAX_CELLS)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "seqslam_describe: thumbnail %d x %d has more than %d cells", h, w, SD_MAX_CELLS);
    if ((int64_t)H * W >= SD_MAX_PIXELS)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "seqslam_describe: frames of %d x %d pixels, 2^23 or more", H, W);
    if (ld_out < (int64_t)h * w)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "seqslam_describe: ld_out=%lld < h * w=%d", (long long)ld_out, h * w);
    if (frames > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "seqslam_describe: frames must be below 2^31");
    DLC_ON_DEVICE(ctx);
    SdArgs a;
    a.gray = gray; a.out = out; a.ld_out = ld_out;
    a.H = H; a.W = W; a.h = h; a.w = w; a.patch = patch; a.strength = strength;
    a.g_resize = dlc_lane_group(dlc::cdiv(SD_THREADS, (int64_t)h * w));
    a.g_tile = dlc_lane_group((int64_t)patch * patch);
    const size_t lds = dlc::align_up((size_t)h * w, 16);
    hipLaunchKernelGGL(seqslam_describe_kernel, dim3((unsigned)frames), dim3(SD_THREADS), lds, (hipStream_t)stream, a);
    DLC_LAUNCH_CHECK(ctx, "seqslam_describe_kernel");
    return DLC_OK;
}
