// SeqSLAM's image difference with lateral-shift tolerance (the best of +-S thumbnail columns, as Milford's low-resolution
// work and SMART compare): dlc_sad_u8_shift_rows.  For a thumbnail of h rows and w columns and every shift -S <= s <= S
//     sad_s(q, d) = sum over y < h, over x with 0 <= x < w and 0 <= x + s < w, of |q[y][x] - d[y][x + s]|
//     v_s = floor(sad_s * w / (w - |s|)),   out = min_s v_s,   shift = the first s of the minimum in 0, -1, +1, -2, +2, ...
// as int64 rows with the contract of dlc_sad_u8_rows (u8_rows.hip) word for word, plus the int8 shift of every cell.
//
// The launch is the plain rows' -- one workgroup per (query tile, db tile) below the largest limit of the call, the thread
// layouts of distance_tile.h (NTX threads across db rows, 256 / NTX across queries, QR queries per thread), grid stride
// past 65 536 db tiles, no split along D, every thread storing its cells once under j < lim(r) -- with CB db rows per
// thread instead of 4: all 2 ST + 1 sums of a pair are accumulated in one pass over the staged bytes, in registers, and
// QR * CB * (2 ST + 1) accumulators have to fit (68 .. 80 at every instantiation).  ST is 1, 2, 4 or 8, the next one at or
// above the call's S; the surplus shifts are accumulated and dropped in the epilogue.
//
// STAGING is by image-row segment, not by the flat 64-byte step of the plain kernel (a shifted window must not run from
// one image row into the next): a step is the columns [c0, c0 + 64) of one image row y -- 16 words of every query of the
// tile, and the columns [c0 - 16, c0 + 80) of every db row, 24 words.  A chunk is 16 columns (4 query words, one
// ds_read_b128); it reads the 12 db words from 16 columns to its left on (three ds_read_b128).  Shift s = 4a + b
// (0 <= b < 4, a = floor(s / 4)) of query word x is word x + a of the db row at byte alignment b:
// __builtin_amdgcn_alignbyte of two neighbouring staged words, so three aligned copies of a db word serve every shift,
// and they are shared by the QR queries of the thread.  v_sad_u8 stays the inner operation: one per (pair, shift, word).
//
// EDGES.  A cell with x + s outside [0, w) contributes nothing: BOTH operands are masked there (a zero halo on the db
// side alone would leave |q - 0|), so what the halo holds changes nothing.  Only the words within 8 columns of an edge
// need a mask.  On the fast path (w a multiple of 16: the segments are 16-byte blocks of the rows, loaded as such and
// prefetched through registers) the left edge is the chunk at column 0 and the right edge the chunk that ends at w, and
// their masks are compile-time constants: words that are masked out entirely cost nothing, the others two v_and.
// Every other width takes the generic path: the same steps staged byte by byte (columns at and past w as zero), run-time
// masks (wave-uniform) on the first chunk of a row and on the chunks within 8 columns of w.  Bytes at and past D = h w
// of a row are never read on either path.
//
// EPILOGUE, exact 64-bit integers.  n_s = sad_s * w < 2^48 (sad_s <= 255 * 2^24, w <= 2^16), d_s = w - |s| <= 2^16.
// floor is monotone, so out = floor(min_s n_s / d_s): the smallest fraction is found by cross-multiplication
// (n_s * d_t < 2^64), divided once (a real 64-bit division), and the shift is the first s in the stated order with
// floor(n_s / d_s) = out, i.e. n_s < (out + 1) * d_s ((out + 1) * d_s <= n_s + d_s < 2^49).
#include "distance_tile.h"

namespace {

constexpr int SS_SEG = 64;                     // columns of an image row per step
constexpr int SS_HALO = 16;                    // db columns staged on either side of them
constexpr int SS_AW = SS_SEG / 4, SS_BW = (SS_SEG + 2 * SS_HALO) / 4;   // words staged per query / db row and step
constexpr int SS_AP = SS_AW + 4, SS_BP = SS_BW + 4;   // pitches: 16-byte aligned; 20 tx and 28 tx mod 64 take 16 distinct
                                                      // 4-bank slots over any 16 lanes with distinct tx mod 16
constexpr int SS_DB_BLOCKS = SS_BW / 4;        // 16-byte blocks per db row and step

// bytes 0 .. hi-1 of a word (hi <= 0: none, hi >= 4: all)
__device__ __forceinline__ unsigned ss_bytes_below(int hi) {
    return hi >= 4 ? 0xffffffffu : (hi <= 0 ? 0u : ((1u << (8 * hi)) - 1u));
}

enum { SS_INNER = 0, SS_LEFT = 1, SS_RIGHT = 2, SS_BOTH = 3, SS_RUNTIME = 4 };

// One chunk: query words a[r][0..3] (columns c .. c + 15 of the image row) against the 12 staged db words e[0..11] of
// each of the thread's db rows (columns c - 16 .. c + 31).  MODE says which masks apply: none, the compile-time ones of a
// chunk that starts at column 0 and / or ends at column w, or the run-time ones for column c with rem = w - c columns left.
template <int MODE, int QR, int CB, int ST, int NTX>
__device__ __forceinline__ void ss_chunk(unsigned (&acc)[QR][CB][2 * ST + 1], const u32x4_t (&a)[QR],
                                         const unsigned (*Bs)[SS_BP], int tx, int t, int c, int rem) {
    constexpr int A = (ST + 3) / 4;            // whole-word offsets reach -A .. A
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) {
        unsigned e[12];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const u32x4_t b = *(const u32x4_t*)&Bs[tx + NTX * cc][4 * t + 4 * v];
#pragma unroll
            for (int i = 0; i < 4; ++i) e[4 * v + i] = b[i];
        }
#pragma unroll
        for (int p = 4 - A; p <= 7 + A; ++p) {             // db word p: columns c - 16 + 4 p ..
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (p == 7 + A && b > 0) continue;         // (no shift reaches past word 7 + A)
                const unsigned d = b == 0 ? e[p] : __builtin_amdgcn_alignbyte(e[p + 1], e[p], (unsigned)b);
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int s = 4 * (p - 4 - x) + b;     // this copy is query word x's operand at shift s
                    if (s < -ST || s > ST) continue;
                    unsigned m = 0xffffffffu;
                    if (MODE != SS_INNER) {
                        // byte i of the word is column c + 4 x + i: kept when 0 <= that + s, that < w and that + s < w
                        const int left = (MODE == SS_LEFT || MODE == SS_BOTH) ? 0 : (MODE == SS_RUNTIME ? c : 1 << 20);
                        const int right = (MODE == SS_RIGHT || MODE == SS_BOTH) ? 16 : (MODE == SS_RUNTIME ? rem : 1 << 20);
                        const int lo = -(left + 4 * x + s);
                        const int hi = right - 4 * x - (s > 0 ? s : 0);
                        m = ss_bytes_below(hi) & ~ss_bytes_below(lo);
                        if (MODE != SS_RUNTIME && m == 0u) continue;
                    }
#pragma unroll
                    for (int r = 0; r < QR; ++r)
                        acc[r][cc][s + ST] = __builtin_amdgcn_sad_u8(a[r][x] & m, d & m, acc[r][cc][s + ST]);
                }
            }
        }
    }
}

template <int NTX, int QR, int CB, int ST, bool FAST>
__global__ __launch_bounds__(256) void sad_shift_rows_kernel(const uint8_t* __restrict__ queries, long long Q, long long ldq,
                                                             const uint8_t* __restrict__ db, long long N, long long ldd,
                                                             int h, int w, int S, long long limit0, long long limit_step,
                                                             long long* __restrict__ out, long long ld_out,
                                                             signed char* __restrict__ shift_out, long long ld_shift) {
    constexpr int NTY = 256 / NTX, QT = NTY * QR, DB = NTX * CB, NS = 2 * ST + 1;
    constexpr int PA = (QT * 4 + 255) / 256, PB = (DB * SS_DB_BLOCKS + 255) / 256;   // 16-byte loads per thread and step
    __shared__ __attribute__((aligned(16))) unsigned As[QT][SS_AP];
    __shared__ __attribute__((aligned(16))) unsigned Bs[DB][SS_BP];

    const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
    const long long q0 = (long long)blockIdx.y * QT;
    const long long lmax = tk_tile_limit<QT>(q0, Q, N, limit0, limit_step);
    long long lq[QR];
#pragma unroll
    for (int r = 0; r < QR; ++r) lq[r] = tk_query_limit(q0 + ty + NTY * r, Q, N, limit0, limit_step);
    const int spr = (w + SS_SEG - 1) / SS_SEG, steps = h * spr;      // segments per image row; steps of a tile
    for (long long j0 = (long long)blockIdx.x * DB; j0 < lmax; j0 += (long long)gridDim.x * DB) {
        unsigned acc[QR][CB][NS];
#pragma unroll
        for (int r = 0; r < QR; ++r)
#pragma unroll
            for (int cc = 0; cc < CB; ++cc)
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[r][cc][s] = 0u;
        u32x4_t va[PA], vb[PB];
        // fast path: the 16-byte blocks of segment (y, c0) into registers (w, c0 multiples of 16: aligned, inside the row)
        auto fetch = [&](int y, int c0) {
            const long long base = (long long)y * w;
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const int i = tid + 256 * p, row = i >> 2, col = c0 + 16 * (i & 3);
                const long long q = q0 + row;
                va[p] = (row < QT && q < Q && col < w) ? *(const u32x4_t*)(queries + q * ldq + base + col)
                                                      : u32x4_t{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                const int i = tid + 256 * p, row = i / SS_DB_BLOCKS, col = c0 - SS_HALO + 16 * (i % SS_DB_BLOCKS);
                const long long j = j0 + row;
                vb[p] = (row < DB && j < lmax && col >= 0 && col < w) ? *(const u32x4_t*)(db + j * ldd + base + col)
                                                                     : u32x4_t{0u, 0u, 0u, 0u};
            }
        };
        // generic path: the same segment word by word, each word from up to four byte loads (columns outside [0, w): 0)
        auto stage_bytes = [&](int y, int c0) {
            const long long base = (long long)y * w;
#pragma unroll 1
            for (int i = tid; i < QT * SS_AW; i += 256) {
                const int row = i / SS_AW, wd = i % SS_AW, col = c0 + 4 * wd;
                const long long q = q0 + row;
                unsigned v = 0u;
                if (q < Q) {
                    const uint8_t* src = queries + q * ldq + base;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (col + b < w) v |= (unsigned)src[col + b] << (8 * b);
                }
                As[row][wd] = v;
            }
#pragma unroll 1
            for (int i = tid; i < DB * SS_BW; i += 256) {
                const int row = i / SS_BW, wd = i % SS_BW, col = c0 - SS_HALO + 4 * wd;
                const long long j = j0 + row;
                unsigned v = 0u;
                if (j < lmax) {
                    const uint8_t* src = db + j * ldd + base;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (col + b >= 0 && col + b < w) v |= (unsigned)src[col + b] << (8 * b);
                }
                Bs[row][wd] = v;
            }
        };
        if (FAST) fetch(0, 0);
        int y = 0, c0 = 0;
        for (int k = 0; k < steps; ++k) {
            int yn = y, cn = c0 + SS_SEG;                    // the next segment
            if (cn >= w) { cn = 0; ++yn; }
            if (FAST) {
#pragma unroll
                for (int p = 0; p < PA; ++p) {
                    const int i = tid + 256 * p;
                    if (i < QT * 4) *(u32x4_t*)&As[i >> 2][4 * (i & 3)] = va[p];
                }
#pragma unroll
                for (int p = 0; p < PB; ++p) {
                    const int i = tid + 256 * p;
                    if (i < DB * SS_DB_BLOCKS) *(u32x4_t*)&Bs[i / SS_DB_BLOCKS][4 * (i % SS_DB_BLOCKS)] = vb[p];
                }
                __syncthreads();
                if (k + 1 < steps) fetch(yn, cn);
            } else {
                stage_bytes(y, c0);
                __syncthreads();
            }
            const int seg = w - c0 < SS_SEG ? w - c0 : SS_SEG;
            const int chunks = (seg + 15) / 16;
#pragma unroll 1
            for (int t = 0; t < chunks; ++t) {
                const int c = c0 + 16 * t, rem = w - c;
                u32x4_t a[QR];
#pragma unroll
                for (int r = 0; r < QR; ++r) a[r] = *(const u32x4_t*)&As[ty + NTY * r][4 * t];
                if (FAST) {
                    const bool left = c == 0, right = rem == 16;
                    if (left && right) ss_chunk<SS_BOTH, QR, CB, ST, NTX>(acc, a, Bs, tx, t, c, rem);
                    else if (left) ss_chunk<SS_LEFT, QR, CB, ST, NTX>(acc, a, Bs, tx, t, c, rem);
                    else if (right) ss_chunk<SS_RIGHT, QR, CB, ST, NTX>(acc, a, Bs, tx, t, c, rem);
                    else ss_chunk<SS_INNER, QR, CB, ST, NTX>(acc, a, Bs, tx, t, c, rem);
                } else {
                    // inner: all 16 columns below w and 8 more to their right, 16 or more to their left
                    if (c > 0 && rem >= 24) ss_chunk<SS_INNER, QR, CB, ST, NTX>(acc, a, Bs, tx, t, c, rem);
                    else ss_chunk<SS_RUNTIME, QR, CB, ST, NTX>(acc, a, Bs, tx, t, c, rem);
                }
            }
            __syncthreads();
            y = yn;
            c0 = cn;
        }
        int sx = tx, sy = ty;
        tk_behind_loop(sx, sy);
#pragma unroll
        for (int r = 0; r < QR; ++r) {
            const long long q = q0 + sy + NTY * r;                 // (lq[r] = 0 where q >= Q: nothing is stored there)
#pragma unroll
            for (int cc = 0; cc < CB; ++cc) {
                const long long j = j0 + sx + NTX * cc;
                if (j < lq[r]) {
                    const unsigned long long uw = (unsigned long long)w;
                    unsigned long long nb = acc[r][cc][ST] * uw, dbest = uw;      // the smallest fraction n / d so far
#pragma unroll
                    for (int k = 1; k <= ST; ++k) {
                        if (k <= S) {
                            const unsigned long long d = uw - (unsigned long long)k;
#pragma unroll
                            for (int sg = -1; sg <= 1; sg += 2) {
                                const unsigned long long n = acc[r][cc][ST + sg * k] * uw;
                                if (n * dbest < nb * d) { nb = n; dbest = d; }
                            }
                        }
                    }
                    const unsigned long long v = nb / dbest;
                    int sh = 0;
                    // the stated order backwards, so that the first shift of the minimum is the last one assigned
#pragma unroll
                    for (int k = ST; k >= 1; --k) {
                        if (k <= S) {
                            const unsigned long long bound = (v + 1ull) * (uw - (unsigned long long)k);
                            if (acc[r][cc][ST + k] * uw < bound) sh = k;
                            if (acc[r][cc][ST - k] * uw < bound) sh = -k;
                        }
                    }
                    if (acc[r][cc][ST] * uw < (v + 1ull) * uw) sh = 0;
                    out[q * ld_out + j] = (long long)v;
                    if (shift_out) shift_out[q * ld_shift + j] = (signed char)sh;
                }
            }
        }
    }
}

struct SsArgs {
    const uint8_t *queries, *db;
    long long Q, ldq, N, ldd, limit0, limit_step, ld_out, ld_shift;
    int h, w, S;
    long long* out;
    signed char* shift_out;
    dim3 grid;
    hipStream_t stream;
};

template <int NTX, int QR, int CB, int ST>
void ss_launch(const SsArgs& a, bool fast) {
    if (fast)
        hipLaunchKernelGGL((sad_shift_rows_kernel<NTX, QR, CB, ST, true>), a.grid, dim3(256), 0, a.stream, a.queries, a.Q,
                           a.ldq, a.db, a.N, a.ldd, a.h, a.w, a.S, a.limit0, a.limit_step, a.out, a.ld_out, a.shift_out,
                           a.ld_shift);
    else
        hipLaunchKernelGGL((sad_shift_rows_kernel<NTX, QR, CB, ST, false>), a.grid, dim3(256), 0, a.stream, a.queries, a.Q,
                           a.ldq, a.db, a.N, a.ldd, a.h, a.w, a.S, a.limit0, a.limit_step, a.out, a.ld_out, a.shift_out,
                           a.ld_shift);
}

// db rows per thread: QR * CB * (2 ST + 1) accumulators stay in registers
constexpr int ss_cb(int qr, int st) { return qr == 1 ? 4 : (st == 8 ? 1 : (st == 4 ? 2 : 4)); }
// the instantiation that serves max_shift S (0 is served by 1: the plain sum is its shift 0)
inline int ss_st(int S) { return S <= 1 ? 1 : (S <= 2 ? 2 : (S <= 4 ? 4 : 8)); }

template <int NTX, int QR>
void ss_launch_plan(SsArgs& a, int st, int64_t lmax, unsigned qtiles, bool fast) {
    auto grid_for = [&](int cb) { a.grid = tk_grid(lmax, NTX * cb, qtiles); };
    if (st == 1) { grid_for(ss_cb(QR, 1)); ss_launch<NTX, QR, ss_cb(QR, 1), 1>(a, fast); }
    else if (st == 2) { grid_for(ss_cb(QR, 2)); ss_launch<NTX, QR, ss_cb(QR, 2), 2>(a, fast); }
    else if (st == 4) { grid_for(ss_cb(QR, 4)); ss_launch<NTX, QR, ss_cb(QR, 4), 4>(a, fast); }
    else { grid_for(ss_cb(QR, 8)); ss_launch<NTX, QR, ss_cb(QR, 8), 8>(a, fast); }
}

}  // namespace

extern "C" int dlc_sad_u8_shift_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq, const uint8_t* db,
                                     int64_t N, int64_t ldd, int h, int w, int max_shift, int64_t limit0,
                                     int64_t limit_step, int64_t* out, int64_t ld_out, int8_t* shift_out,
                                     int64_t ld_shift, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (h < 1 || w < 1 || max_shift < 0) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sad_u8_shift_rows: bad argument");
    if (max_shift > DLC_MAX_SHIFT || max_shift >= w)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sad_u8_shift_rows: max_shift=%d outside 0..min(%d, w - 1 = %d)", max_shift,
                         DLC_MAX_SHIFT, w - 1);
    if (w > 65536) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sad_u8_shift_rows: w=%d exceeds 65536", w);
    if (shift_out && ld_shift < N)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sad_u8_shift_rows: ld_shift=%lld < N=%lld", (long long)ld_shift, (long long)N);
    // the rest as a plain row call of D = h * w bytes (255 * h * w fits the 32-bit accumulator for h * w <= 2^24)
    if (const int rc = tk_rows_check(ctx, "sad_u8_shift_rows", queries, Q, ldq, db, N, ldd, (int64_t)h * w, 1ll << 24, out, ld_out);
        rc != DLC_OK)
        return rc;
    SsArgs a{queries, db, (long long)Q, (long long)ldq, (long long)N, (long long)ldd, (long long)limit0,
             (long long)limit_step, (long long)ld_out, (long long)ld_shift, h, w, max_shift, (long long*)out,
             (signed char*)shift_out, dim3(), (hipStream_t)stream};
    const bool fast = w % 16 == 0;                               // image rows are 16-byte blocks of the descriptor rows
    const int st = ss_st(max_shift);
    return tk_rows_launch(ctx, "sad_shift_rows_kernel", Q, N, limit0, limit_step, [&](auto s, int64_t lmax, unsigned qtiles) {
        ss_launch_plan<s.ntx, s.qr>(a, st, lmax, qtiles, fast);
    });
}
