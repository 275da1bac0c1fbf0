// Geometric verification of loop candidates over patch key-points: dlc_verify_pairs (include/dlc.h holds the definition --
// DIST's serial chain, the lowest-index arg-mins of rows and columns, the cross-check, the exhaustive integer hypotheses).
//
//   TABLES (the hot path, pairs x P x P x H x 3 fp64 operations): a workgroup is ONE wave of 8 x 8 threads and owns a
//          CT*8 x CT*8 tile of one pair's (p, j) cells; a thread owns a CT x CT register tile, each cell one serial chain
//          in h.  The query's and the candidate's patch rows stream through LDS in chunks of 128 / CT columns (16 + 16
//          doubles a thread, whatever CT: the fewer cells a wave sums per column, the more columns it needs in flight to
//          cover a chunk's round trip to memory), stored column-major (pitch + 2, so the transposing stores spread over
//          the banks) and read as the thread's CT + CT neighbours; the next chunk is fetched into registers while the
//          current one is summed -- vlad_assign_kernel's shape, with the "codebook" of a pair reached through cand.
//          The grid is pairs x cell tiles.  A chain cannot be cut, so the most a call can spread is one cell per
//          thread: CT = 4 (a 32 x 32 tile: the 30 patches of a frame in one wave, 48 fp64 operations per 8 LDS values)
//          when that still gives every CU its waves, else CT = 2, else CT = 1 -- one streamed frame with k = 5 is 80
//          waves on 80 CUs instead of 5.  Any tiling gives the same bits.
//   RESOLVE: a workgroup of 256 threads per pair.  The table goes to LDS (pitch 65); thread p folds row p and thread
//          64 + j column j, strict < in ascending index; the cross-check, the presence of the points and the compaction of
//          M (a thread's slot = the kept matches below it); the hypotheses dealt out idx = t, t + 256, ..; (count, idx)
//          folded in LDS, more inliers first, then the lower idx; the winner's mask.  int64 throughout, no atomics.
#include "dlc_internal.h"

// every difference, product and sum rounded on its own (hipcc contracts a * b + c into an fma otherwise)
#pragma clang fp contract(off)

namespace {

constexpr int VF_WAVE = 64;                    // threads of a table workgroup: 8 x 8
constexpr int VF_CHUNK = 128;                  // columns of an LDS chunk x cells a thread owns along a side
constexpr int VF_AHEAD = 8;                    // columns x cells a side whose LDS values a thread reads ahead of its chains
constexpr int VF_THREADS = 256;                // threads of a resolve workgroup
constexpr int VF_PITCH = DLC_VERIFY_MAX_PATCHES + 1;       // of the table in LDS: odd, so a row scan and a column scan spread over the banks
constexpr long long VF_SPREAD = 512;           // workgroups a coarser tile must still give (two waves per CU)
constexpr int VF_MAX_COORD = 8191;

struct VfTableArgs {
    const double* q;
    const double* d;
    const long long* cand;
    double* table;                             // [pairs][P][P]
    long long ldq, ldd, H, N, ld_cand, items;
    int k, P, tiles;                           // tiles: of a side of the table
};

template <int CT>
__global__ __launch_bounds__(VF_WAVE) void verify_table_kernel(const VfTableArgs a) {
    constexpr int TB = CT * 8, XS = TB + 2, VF_HC = VF_CHUNK / CT;
    constexpr int XL = TB * VF_HC / VF_WAVE;   // a thread's elements of a chunk, per side: 16
    constexpr int AHEAD = CT == 4 ? 1 : VF_AHEAD / CT;     // (CT = 4 has no registers left for it: two waves a SIMD hide the reads)
    __shared__ double xs[VF_HC * XS];          // [column of the chunk][query patch of the tile]
    __shared__ double cs[VF_HC * XS];          // [column of the chunk][candidate patch of the tile]
    const int t = threadIdx.x, tx = t & 7, ty = t >> 3;
    double xr[XL], cr[XL];                     // the next chunk, on its way from memory
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long pair = item / (a.tiles * a.tiles);
        const int tile = (int)(item % (a.tiles * a.tiles));
        const long long c = a.cand[(pair / a.k) * a.ld_cand + pair % a.k];
        if (c < 0 || c >= a.N) continue;       // (the same in every thread) the pair's slot keeps its bits
        const int p0 = (tile / a.tiles) * TB, j0 = (tile % a.tiles) * TB;
        const double* xq = a.q + (pair / a.k) * a.P * a.ldq;
        const double* xd = a.d + c * a.P * a.ldd;
        double d[CT][CT];
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int j = 0; j < CT; ++j) d[i][j] = 0.0;
        // the chunk at h0: the thread's XL + XL elements of it from memory into registers (element e = t + i * 64)
        auto fetch = [&](long long h0) {
#pragma unroll
            for (int i = 0; i < XL; ++i) {
                const int e = t + i * VF_WAVE, r = e / VF_HC, hh = e % VF_HC;
                const long long h = h0 + hh;
                xr[i] = (p0 + r < a.P && h < a.H) ? xq[(long long)(p0 + r) * a.ldq + h] : 0.0;
                cr[i] = (j0 + r < a.P && h < a.H) ? xd[(long long)(j0 + r) * a.ldd + h] : 0.0;
            }
        };
        fetch(0);
        for (long long h0 = 0; h0 < a.H; h0 += VF_HC) {
            __syncthreads();                   // the last chunk has been read
#pragma unroll
            for (int i = 0; i < XL; ++i) {
                const int e = t + i * VF_WAVE;
                xs[(e % VF_HC) * XS + e / VF_HC] = xr[i];
                cs[(e % VF_HC) * XS + e / VF_HC] = cr[i];
            }
            __syncthreads();
            if (h0 + VF_HC < a.H) fetch(h0 + VF_HC);               // in flight while this chunk is summed
            const int hn = a.H - h0 < VF_HC ? (int)(a.H - h0) : VF_HC;
            auto column = [&](int hh) {
                double xv[CT], cv[CT];
#pragma unroll
                for (int i = 0; i < CT; ++i) xv[i] = xs[hh * XS + ty * CT + i];
#pragma unroll
                for (int j = 0; j < CT; ++j) cv[j] = cs[hh * XS + tx * CT + j];
#pragma unroll
                for (int i = 0; i < CT; ++i)
#pragma unroll
                    for (int j = 0; j < CT; ++j) {
                        const double u = xv[i] - cv[j];
                        const double q = u * u;
                        d[i][j] = d[i][j] + q;
                    }
            };
            if (AHEAD > 1 && hn == VF_HC) {    // a whole chunk: AHEAD columns' LDS reads are issued ahead of their sums
#pragma unroll AHEAD
                for (int hh = 0; hh < VF_HC; ++hh) column(hh);
            } else {
                for (int hh = 0; hh < hn; ++hh) column(hh);
            }
        }
        double* out = a.table + pair * a.P * a.P;
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const int p = p0 + ty * CT + i, jj = j0 + tx * CT + j;
                if (p < a.P && jj < a.P) out[p * a.P + jj] = d[i][j];
            }
    }
}

struct VfResolveArgs {
    const double* table;
    const int* q_pts;
    const int* db_pts;
    const long long* cand;
    int* out_inliers;
    int* out_matches;
    int* out_hyp;                              // may be null
    unsigned long long* out_mask;              // may be null
    int* out_match;                            // may be null
    long long N, ld_cand, pairs;
    int k, P, model, tol, S, mutual;
};

__device__ __forceinline__ bool vf_present(int x, int y) { return x >= 0 && x <= VF_MAX_COORD && y >= 0 && y <= VF_MAX_COORD; }

// A hypothesis, fixed by the matches at the compacted slots s (and t): what every inlier test of it shares.
struct VfHyp {
    long long asx, asy, bsx, bsy, ux, uy, vx, vy, bound;
};

// SIMILARITY (s, t): false if the hypothesis is not valid
__device__ __forceinline__ bool vf_similarity(VfHyp& h, const int* ax, const int* ay, const int* bx, const int* by, int s, int t,
                                               long long tol, long long S) {
    h.asx = ax[s]; h.asy = ay[s]; h.bsx = bx[s]; h.bsy = by[s];
    h.ux = ax[t] - h.asx; h.uy = ay[t] - h.asy; h.vx = bx[t] - h.bsx; h.vy = by[t] - h.bsy;
    const long long uu = h.ux * h.ux + h.uy * h.uy, vv = h.vx * h.vx + h.vy * h.vy;
    h.bound = tol * tol * uu;
    if (uu <= 0 || vv <= 0) return false;
    return S <= 0 || (256 * vv <= S * S * uu && 256 * uu <= S * S * vv);
}

__device__ __forceinline__ bool vf_similarity_inlier(const VfHyp& h, int ax, int ay, int bx, int by) {
    const long long dax = ax - h.asx, day = ay - h.asy, dbx = bx - h.bsx, dby = by - h.bsy;
    const long long re = (dbx * h.ux - dby * h.uy) - (h.vx * dax - h.vy * day);
    const long long im = (dbx * h.uy + dby * h.ux) - (h.vx * day + h.vy * dax);
    return re * re + im * im <= h.bound;
}

// TRANSLATION s: (vx, vy) is the shift b_s - a_s
__device__ __forceinline__ void vf_translation(VfHyp& h, const int* ax, const int* ay, const int* bx, const int* by, int s,
                                                long long tol) {
    h.vx = (long long)bx[s] - ax[s];
    h.vy = (long long)by[s] - ay[s];
    h.bound = tol * tol;
}

__device__ __forceinline__ bool vf_translation_inlier(const VfHyp& h, int ax, int ay, int bx, int by) {
    const long long ex = ((long long)bx - ax) - h.vx, ey = ((long long)by - ay) - h.vy;
    return ex * ex + ey * ey <= h.bound;
}

// idx-th pair (s, t), s < t < n, in ascending lexicographic order
__device__ __forceinline__ void vf_decode(int idx, int n, int& s, int& t) {
    s = 0;
    while (idx >= n - 1 - s) { idx -= n - 1 - s; ++s; }
    t = s + 1 + idx;
}

__global__ __launch_bounds__(VF_THREADS) void verify_resolve_kernel(const VfResolveArgs a) {
    __shared__ double D[DLC_VERIFY_MAX_PATCHES * VF_PITCH];
    __shared__ int row_min[DLC_VERIFY_MAX_PATCHES], col_min[DLC_VERIFY_MAX_PATCHES], keep[DLC_VERIFY_MAX_PATCHES];
    __shared__ int Mi[DLC_VERIFY_MAX_PATCHES], ax[DLC_VERIFY_MAX_PATCHES], ay[DLC_VERIFY_MAX_PATCHES];
    __shared__ int bx[DLC_VERIFY_MAX_PATCHES], by[DLC_VERIFY_MAX_PATCHES], inl[DLC_VERIFY_MAX_PATCHES];
    __shared__ int red_cnt[VF_THREADS], red_idx[VF_THREADS];
    const int t = threadIdx.x, P = a.P;
    const bool similarity = a.model == DLC_VERIFY_SIMILARITY;
    for (long long pair = blockIdx.x; pair < a.pairs; pair += gridDim.x) {
        const long long r = pair / a.k, c = a.cand[r * a.ld_cand + pair % a.k];
        if (c < 0 || c >= a.N) {               // (the same in every thread) no such key-frame
            if (t < P && a.out_match) a.out_match[pair * P + t] = -1;
            if (t == 0) {
                a.out_inliers[pair] = 0;
                a.out_matches[pair] = 0;
                if (a.out_hyp) { a.out_hyp[2 * pair] = -1; a.out_hyp[2 * pair + 1] = -1; }
                if (a.out_mask) a.out_mask[pair] = 0;
            }
            continue;
        }
        const double* table = a.table + pair * P * P;
        for (int e = t; e < P * P; e += VF_THREADS) D[(e / P) * VF_PITCH + e % P] = table[e];
        __syncthreads();
        // 1. thread p: m(p) along row p; thread 64 + j: r(j) down column j
        if (t < 2 * DLC_VERIFY_MAX_PATCHES && (t & (DLC_VERIFY_MAX_PATCHES - 1)) < P) {
            const int own = t & (DLC_VERIFY_MAX_PATCHES - 1);
            const bool row = t < DLC_VERIFY_MAX_PATCHES;
            double bd = 0.0;
            int best = -1;
            for (int o = 0; o < P; ++o) {
                const double v = row ? D[own * VF_PITCH + o] : D[o * VF_PITCH + own];
                if (v == v && (best < 0 || v < bd)) { bd = v; best = o; }
            }
            (row ? row_min : col_min)[own] = best;
        }
        __syncthreads();
        // 2. the cross-check and the points' presence
        int m = -1, pax = 0, pay = 0, pbx = 0, pby = 0;
        if (t < P) {
            m = row_min[t];
            bool ok = m >= 0 && (!a.mutual || col_min[m] == t);
            if (ok) {
                pax = a.q_pts[(r * P + t) * 2]; pay = a.q_pts[(r * P + t) * 2 + 1];
                pbx = a.db_pts[(c * P + m) * 2]; pby = a.db_pts[(c * P + m) * 2 + 1];
                ok = vf_present(pax, pay) && vf_present(pbx, pby);
            }
            keep[t] = ok;
            if (a.out_match) a.out_match[pair * P + t] = ok ? m : -1;
        }
        __syncthreads();
        // 3. M in ascending p: a kept match's slot is the number of kept matches below it
        if (t < P && keep[t]) {
            int slot = 0;
            for (int o = 0; o < t; ++o) slot += keep[o];
            Mi[slot] = t; ax[slot] = pax; ay[slot] = pay; bx[slot] = pbx; by[slot] = pby;
        }
        int n = 0;
        for (int o = 0; o < P; ++o) n += keep[o];
        __syncthreads();
        // 4. the hypotheses, idx = t, t + 256, ..: a thread meets its own in ascending order, so strict > keeps the first
        const int hyps = similarity ? n * (n - 1) / 2 : n;
        int best_cnt = 0, best_idx = 0x7fffffff;
        for (int idx = t; idx < hyps; idx += VF_THREADS) {
            VfHyp h;
            int cnt = 0;
            if (similarity) {
                int s, u;
                vf_decode(idx, n, s, u);
                if (!vf_similarity(h, ax, ay, bx, by, s, u, a.tol, a.S)) continue;
                for (int i = 0; i < n; ++i) cnt += vf_similarity_inlier(h, ax[i], ay[i], bx[i], by[i]);
            } else {
                vf_translation(h, ax, ay, bx, by, idx, a.tol);
                for (int i = 0; i < n; ++i) cnt += vf_translation_inlier(h, ax[i], ay[i], bx[i], by[i]);
            }
            if (cnt > best_cnt) { best_cnt = cnt; best_idx = idx; }
        }
        // 5. the largest count, the lowest idx among equals
        red_cnt[t] = best_cnt;
        red_idx[t] = best_idx;
        __syncthreads();
        for (int s = VF_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) {
                const int oc = red_cnt[t + s], oi = red_idx[t + s];
                if (oc > red_cnt[t] || (oc == red_cnt[t] && oi < red_idx[t])) { red_cnt[t] = oc; red_idx[t] = oi; }
            }
            __syncthreads();
        }
        // 6. the winner's mask and the outputs
        const int win_cnt = red_cnt[0], win_idx = red_idx[0];
        int hs = -1, ht = -1;
        if (win_cnt > 0) {
            VfHyp h;
            if (similarity) {
                vf_decode(win_idx, n, hs, ht);
                (void)vf_similarity(h, ax, ay, bx, by, hs, ht, a.tol, a.S);
                if (t < n) inl[t] = vf_similarity_inlier(h, ax[t], ay[t], bx[t], by[t]);
            } else {
                hs = win_idx;
                vf_translation(h, ax, ay, bx, by, hs, a.tol);
                if (t < n) inl[t] = vf_translation_inlier(h, ax[t], ay[t], bx[t], by[t]);
            }
        }
        __syncthreads();
        if (t == 0) {
            unsigned long long mask = 0;
            if (win_cnt > 0)
                for (int i = 0; i < n; ++i)
                    if (inl[i]) mask |= 1ull << Mi[i];
            a.out_inliers[pair] = win_cnt;
            a.out_matches[pair] = n;
            if (a.out_hyp) {
                a.out_hyp[2 * pair] = hs >= 0 ? Mi[hs] : -1;
                a.out_hyp[2 * pair + 1] = ht >= 0 ? Mi[ht] : -1;
            }
            if (a.out_mask) a.out_mask[pair] = mask;
        }
        __syncthreads();                       // the LDS is read before the next pair fills it
    }
}

size_t vf_workspace(int64_t Q, int k, int P) {
    if (Q < 1 || k < 1 || k > DLC_MAX_K || P < 1 || P > DLC_VERIFY_MAX_PATCHES || Q > 0x7fffffffll / DLC_MAX_K) return 0;
    return dlc::align_up((size_t)Q * (size_t)k * (size_t)P * (size_t)P * 8, 256);
}

// the cells a thread owns along a side: the coarsest tile that still spreads the call over the chip
int vf_cells(long long pairs, int P) {
    for (int ct = 4; ct > 1; ct >>= 1) {
        const long long tiles = dlc::cdiv(P, ct * 8);
        if (pairs * tiles * tiles >= VF_SPREAD) return ct;
    }
    return 1;
}

}  // namespace

extern "C" size_t dlc_verify_pairs_workspace_bytes(int64_t Q, int k, int P) { return vf_workspace(Q, k, P); }

extern "C" int dlc_verify_pairs(dlc_ctx* ctx, const double* q_desc, int64_t ldq, const int32_t* q_pts, int64_t Q,
                                const double* db_desc, int64_t ldd, const int32_t* db_pts, int64_t N, int P, int64_t H,
                                const int64_t* cand, int64_t ld_cand, int k, int model, int tol, int max_scale_x16, int mutual,
                                int32_t* out_inliers, int32_t* out_matches, int32_t* out_hyp, uint64_t* out_mask,
                                int32_t* out_match, double* out_dist, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!q_desc || !q_pts || !db_desc || !db_pts || !cand || !out_inliers || !out_matches)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: null pointer");
    if ((((uintptr_t)q_desc) | ((uintptr_t)db_desc) | ((uintptr_t)cand) | ((uintptr_t)out_mask) | ((uintptr_t)out_dist)) & 7)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: descriptors, cand, out_mask and out_dist must be aligned to 8 bytes");
    if ((((uintptr_t)q_pts) | ((uintptr_t)db_pts) | ((uintptr_t)out_inliers) | ((uintptr_t)out_matches) | ((uintptr_t)out_hyp) |
         ((uintptr_t)out_match)) & 3)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: points and int32 outputs must be aligned to 4 bytes");
    if (Q < 1 || N < 1 || P < 1 || H < 1 || k < 1 || k > DLC_MAX_K)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: Q=%lld, N=%lld, P=%d, H=%lld must be >= 1 and k=%d in 1..%d",
                         (long long)Q, (long long)N, P, (long long)H, k, DLC_MAX_K);
    if (ldq < H || ldd < H || ld_cand < k)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: ldq=%lld or ldd=%lld < H=%lld, or ld_cand=%lld < k=%d", (long long)ldq,
                         (long long)ldd, (long long)H, (long long)ld_cand, k);
    if (model != DLC_VERIFY_SIMILARITY && model != DLC_VERIFY_TRANSLATION)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: unknown model %d", model);
    if (tol < 0 || tol > 255 || (max_scale_x16 != 0 && (max_scale_x16 < 16 || max_scale_x16 > 256)) || (mutual != 0 && mutual != 1))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "verify_pairs: tol=%d outside 0..255, max_scale_x16=%d neither 0 nor in 16..256, or "
                         "mutual=%d neither 0 nor 1", tol, max_scale_x16, mutual);
    if (P > DLC_VERIFY_MAX_PATCHES || Q > 0x7fffffffll / DLC_MAX_K || N > 0x7fffffffll)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "verify_pairs: P=%d > %d, Q=%lld > 2^31 / %d or N=%lld >= 2^31", P,
                         DLC_VERIFY_MAX_PATCHES, (long long)Q, DLC_MAX_K, (long long)N);
    const int rw = dlc::check_workspace(ctx, "verify_pairs", workspace, workspace_bytes, vf_workspace(Q, k, P));
    if (rw != DLC_OK) return rw;
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    const long long pairs = (long long)Q * k;
    double* table = out_dist ? out_dist : (double*)workspace;
    VfTableArgs ta = {q_desc, db_desc, (const long long*)cand, table, ldq, ldd, H, N, ld_cand, 0, k, P, 0};
    const int ct = vf_cells(pairs, P);
    ta.tiles = (int)dlc::cdiv(P, ct * 8);
    ta.items = pairs * ta.tiles * ta.tiles;
    if (ct == 4) hipLaunchKernelGGL((verify_table_kernel<4>), dim3(dlc::capped_blocks(ta.items)), dim3(VF_WAVE), 0, st, ta);
    else if (ct == 2) hipLaunchKernelGGL((verify_table_kernel<2>), dim3(dlc::capped_blocks(ta.items)), dim3(VF_WAVE), 0, st, ta);
    else hipLaunchKernelGGL((verify_table_kernel<1>), dim3(dlc::capped_blocks(ta.items)), dim3(VF_WAVE), 0, st, ta);
    DLC_LAUNCH_CHECK(ctx, "verify_table_kernel");
    const VfResolveArgs ra = {table, q_pts, db_pts, (const long long*)cand, out_inliers, out_matches, out_hyp,
                              (unsigned long long*)out_mask, out_match, N, ld_cand, pairs, k, P, model, tol, max_scale_x16, mutual};
    hipLaunchKernelGGL(verify_resolve_kernel, dim3(dlc::capped_blocks(pairs)), dim3(VF_THREADS), 0, st, ra);
    DLC_LAUNCH_CHECK(ctx, "verify_resolve_kernel");
    return DLC_OK;
}
