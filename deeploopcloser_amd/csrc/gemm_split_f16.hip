// SDAV.transform in a TOLERANCE mode on the 16-bit MFMA (dlc_sdav_encode_split; SDAV.py:126-163,293-302;
// TensorflowWrapper.py:57-78: five times sigmoid(h . W + b)).  The fp64 encoder (gemm_dma_f64.hip) stays the parity mode
// and the default; this one trades bit parity for the matrix cores' 16-bit rate under north_star's own tolerance
// ("descriptor L2 within 1e-4"): measured relative L2 <= 2.1e-5 with the reference's N(0,1) weights, 2e-7 with 1/sqrt(fan_in)
// weights (tests/test_gpu_parity.py; the NumPy emulation that chose the form: scripts/emul_split_encoder.py).
//
// Arithmetic.  Every operand is TWO fp16 pieces of a power-of-two multiple of its value,
//   h 2^11 = h1 + h2 + O(2^-22 h 2^11),   W 2^s = W1 + W2 + O(2^-22 W 2^s)   (s: the layer's largest |W| 2^s lands in [2048, 4096)),
// and a layer is THREE fp16 MFMA products into one fp32 accumulator, z 2^(11+s) = h1.W1 + h1.W2 + h2.W1 (the dropped h2.W2 is
// 2^-22 of a term).  fp16 pieces carry 11 significant bits each where bf16 pieces carry 8: the bf16 split needs SIX products
// (three pieces per operand) to come under 1e-4 with N(0,1) weights -- three bf16 products leave 2.7e-4 (same emulation) --
// at the same MFMA rate per product.  The products of two fp16 values are exact in fp32; what is left is the fp32
// accumulation over K = 2500 (1.7e-5 of the descriptor norm through five saturating layers) and the fp32 sigmoid.
//
// Kernel.  The three products of a k-slice share ONE set of operands (r04 ran them as one plain GEMM over K' = 3 K: six
// operand tiles staged and six sets of fragments read per 64-deep k-tile, where four are distinct -- DMA issue and LDS
// fragment reads were worth 17 % of the kernel each, docs/LAB.md 10.2).  Per 32-deep k-slice (one MFMA of K) the four
// tiles W1, W2 (256 weight columns), h1, h2 (256 activation rows) are staged once (64 KiB by LDS-DMA), each wave reads its
// fragments of the four once (W1, W2: 8 x 16 B per lane; h1, h2: 4 x 16 B) and issues 96 MFMAs from registers:
//   P1 = h1 . W1,  P2 = h2 . W1,  P3 = h1 . W2       (8 x 4 tiles of 16 x 16 each, v_mfma_f32_16x16x32_f16)
// with ONE workgroup barrier per slice (r04: four per 64 MFMAs), behind P1: by then every wave holds all four fragment
// sets of the slice (W1, h1 were read during P3 of the slice before, h2 and W2 between P1's MFMAs) and the slice's LDS is
// dead.  The LDS is a ring of 2 1/2 slices, all 160 KiB: two slots for (W2, h2) pairs, three for (W1, h1) pairs.  Behind the
// barrier of slice s the loaders issue (W2, h2) of slice s + 2 -- wanted one period later -- and then (W1, h1) of slice
// s + 3, which has TWO periods to land: the wait in front of a barrier leaves the youngest (W1, h1) pair in flight, so the
// L2 -> LDS stream never drains (with two whole-slice stages every refill had to be issued behind one barrier and land in
// front of the next: 64 KiB take ~2900 cycles round trip on a CU, the slice's MFMAs 3072 -- the period was their sum's
// better part, 3900 cycles; in-kernel stamps, docs/LAB.md 11.3).
//
// Operand format ("K32-major", private to this file -- both operands are written by kernels here): element (row r, k) of a
// piece lives at byte ((k / 32) * rows_pad + r) * 64 + (k % 32) * 2, so that the 256 rows x 32 k of one tile and slice are
// ONE contiguous 16 KiB block: sixteen LDS-DMA wave-instructions of 1 KiB, every one a fully coalesced read (a row-major
// operand would hand each of them sixteen half lines).  The LDS image is that block with the four 16-byte slots of a row
// XOR-ed by 2 * bit 3 of the row (on the DMA's per-lane source offset; the destination is lane-linear), which makes the
// fragment reads -- lane (i, kq) takes slot kq of row i of a 16-row block, ds_read_b128 -- conflict-free in each of the
// instruction's four 16-lane groups.
// Roles: MFMA A operand = 256 weight columns; the weight panel's rows are PERMUTED inside every 64 (column 16 g + 4 t + r
// sits at row 16 t + 4 g + r) so that sixteen consecutive panel rows are one A fragment whose accumulators are, per lane,
// sixteen CONSECUTIVE output columns.  B operand = 256 activation rows (a lane holds ONE row m).  The epilogue therefore
// holds, per lane, runs of sixteen consecutive outputs of one row: bias + sigmoid in fp32 (one fma, v_exp_f32, v_rcp_f32 per
// element), then either the next layer's two fp16 pieces (32 bytes each, K32-major; lanes l and l + 32 trade halves so that a
// store instruction writes one whole slice: 1 KiB in a piece) or, for the last layer, fp64 values that leave through LDS a
// row at a time.  The activations never exist as fp64 between the layers.
// Both operands are re-read (neither is a once-only stream).  Tile order: the tiles in "super-rows" of four activation row
// tiles, column by column inside a super-row, cut into EIGHT CONTIGUOUS RANGES, one per XCD (workgroup ids go round-robin
// to the XCDs; an XCD starts its ids in order, one workgroup per CU): the 32 tiles an XCD runs at a time are 4 rows x 8
// columns of tiles -- 12 operand panels out of that XCD's L2 -- and every XCD gets its 1 / 8 of the tiles to within one.
// (r04 .. the first r05 form dealt whole blocks of 6 x 5 tiles to the XCDs: 1250 tiles = 42 blocks = SIX rounds on two of
// the XCDs where 1250 / 256 = 4.9 fit in five -- a sixth of the kernel's time, found through the in-kernel stamps: the k
// loop accounted for 140 of a tile's 186 us.)
//
// The same k loop serves CnnVtl's tolerance mode (dlc_cnnvtl_encode_split) through a third epilogue, MODE SP_CONV: the
// second half of this file.
#include "gemm_internal.h"
#include "lds_dma.h"

namespace dlc_gemm {
namespace {

constexpr int SP_BM = 256;                     // weight columns per tile (MFMA A operand)
constexpr int SP_BN = 256;                     // activation rows per tile (MFMA B operand)
constexpr int SP_THREADS = 512;
constexpr int SP_KS = 32;                      // k per slice: one v_mfma_f32_16x16x32_f16
constexpr int SP_ROWB = SP_KS * 2;             // 64 bytes of a row per slice
constexpr int SP_OP = 256 * SP_ROWB;           // one operand tile of one slice: 16 KiB, contiguous in memory and in LDS
constexpr int SP_PAIR_B = 2 * SP_OP;           // a slot: one weight tile + one activation tile of a slice, 32 KiB
constexpr int SP_RING_B = 0;                   // (W2, h2) slots 0, 1
constexpr int SP_RING_A = 2 * SP_PAIR_B;       // (W1, h1) slots 0, 1, 2
constexpr int SP_LDS = 5 * SP_PAIR_B;          // 160 KiB: all of a CU's LDS
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
constexpr int SP_X_SHIFT = 11;                 // activations are carried as h * 2^11
constexpr int SP_SUPER = 4;                    // activation row tiles per super-row of the tile order

struct SplitArgs {
    const char* W[2];           // weight pieces, K32-major: [K/32][Np rows (permuted inside 64s)][32] fp16 (rows >= N, k >= K: zeros)
    const char* X[2];           // activation pieces, K32-major: [slices][Mp rows][32] fp16
    long long wslice_b, xslice_b;   // bytes from one k-slice to the next: Np * 64, Mp * 64
    long long M;                // activation rows
    int N;                      // output columns
    int ns;                     // k-slices of 32
    const double* bias;         // [N] or null
    const float* wscale;        // device: 2^s of this layer's weights
    char* O[2];                 // next layer's pieces, K32-major with oslice_b per slice (null for the last layer) ...
    long long oslice_b;
    double* C;                  // ... whose output is fp64 [M, ldc]
    long long ldc;
    long long tiles_m;          // activation row tiles
    int tiles_n;                // weight column tiles
    long long per_xcd, extra;   // tiles per XCD: per_xcd (+ 1 for the first `extra` XCDs), in the order of the file header
};

// The operands reach LDS by dma_run4_if (lds_dma.h): four pieces (a 4 KiB run) in one statement, SKIPPED by a wave whose
// `on` is 0.  The jump is inside the statement, so that the compiler sees straight-line code (a C-level `if` around the
// statement -- basic blocks inside the k loop -- cost the register allocator its footing at 252 of 256 registers: spills).

// s_waitcnt vmcnt(N0) for a wave whose `sel` is 0, vmcnt(N1) otherwise -- the choice inside the statement (as in dma_run4_if)
template <int N0, int N1>
__device__ __forceinline__ void sp_wait_vmcnt_by(unsigned sel) {
    asm volatile(
        "s_cmp_eq_u32 %0, 0\n\t"
        "s_cbranch_scc1 .Lsp_w0_%=\n\t"
        "s_waitcnt vmcnt(%2)\n\t"
        "s_branch .Lsp_w1_%=\n"
        ".Lsp_w0_%=:\n\t"
        "s_waitcnt vmcnt(%1)\n"
        ".Lsp_w1_%=:"
        :
        : "s"(sel), "n"(N0), "n"(N1)
        : "memory", "scc");
}
// SplitArgs + what the convolution epilogue of the CnnVtl tolerance mode needs (O, C, ldc, oslice_b are unused there)
struct ConvSplitArgs : SplitArgs {
    float* Cf;                  // [M, N] fp32: the layer's NHWC output
    const float* xinv;          // [frames] 2^-sx of each frame's activation exponent
    unsigned rows_per_frame;    // oh * ow: row m belongs to frame m / rows_per_frame
    int relu;
    unsigned long long* keys;   // [frames, 2] ordered keys the outputs' per-frame min / max are folded into, or null
    int* status;                // bit 1 <- a non-finite output (only with keys)
};
constexpr int SP_HIDDEN = 0, SP_FINAL = 1, SP_CONV = 2;
template <int MODE> struct SpArgsOf { typedef SplitArgs type; };
template <> struct SpArgsOf<SP_CONV> { typedef ConvSplitArgs type; };

// MODE SP_HIDDEN: hidden SDAV layer (sigmoid, the next layer's pieces); SP_FINAL: last SDAV layer (sigmoid, fp64 out);
// SP_CONV: a convolution layer of the CnnVtl tolerance mode (per-frame descale, bias, ReLU / none, fp32 [M, N] = NHWC out).
// The k loop is the same statement for all three.
template <int MODE>
__global__ __launch_bounds__(SP_THREADS, 2) void gemm_split_f16_kernel(typename SpArgsOf<MODE>::type p) {
    constexpr bool FINAL = MODE == SP_FINAL;
    constexpr bool CONV = MODE == SP_CONV;
    extern __shared__ __attribute__((aligned(16))) char smem_sp[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2;   // weight-column half (128 columns)
    const int wc = wid & 3;    // activation-row block (64 rows)
    // workgroup -> tile: ids go round-robin to the 8 XCDs; XCD x walks its own contiguous range of the tile order
    long long tile_m;
    int tile_n;
    {
        const long long id = blockIdx.x;
        const long long x = id & 7, l = id >> 3;
        if (l >= p.per_xcd + (x < p.extra ? 1 : 0)) return;
        const long long t = x * p.per_xcd + (x < p.extra ? x : p.extra) + l;
        const long long full = (p.tiles_m / SP_SUPER) * SP_SUPER * p.tiles_n;       // tiles in whole super-rows
        if (t < full) {
            const long long w = t % ((long long)SP_SUPER * p.tiles_n);
            tile_m = t / ((long long)SP_SUPER * p.tiles_n) * SP_SUPER + w % SP_SUPER;
            tile_n = (int)(w / SP_SUPER);
        } else {
            const long long rr = p.tiles_m % SP_SUPER, w = t - full;
            tile_m = p.tiles_m / SP_SUPER * SP_SUPER + w % rr;
            tile_n = (int)(w / rr);
        }
    }
    const unsigned lds_base = (unsigned)(unsigned long long)(lptr_t)smem_sp;

    // ---- DMA roles.  A piece costs its wave ~100 cycles of issue, 64 pieces a slice: all eight waves carry eight each, the
    // two waves of a SIMD (w and w + 4) in ANTIPHASE.  Waves 0-3 ("early") stage the (W2, h2) pairs -- wanted within one
    // period -- right behind the barrier, between P2's first MFMAs; waves 4-7 ("late") stage the (W1, h1) pairs, which have
    // two periods, between P3's: while one wave of a SIMD is inside its DMA statements (no matrix instruction for hundreds
    // of cycles) the matrix pipe has the other's.  Wave w stages half (w & 1) of the weight tile (w & 2 == 0) or of the
    // activation tile of its class: eight pieces a slice.
    const unsigned late = __builtin_amdgcn_readfirstlane(wid >> 2);            // 0: (W2, h2) loader, 1: (W1, h1) loader
    const unsigned early = late ^ 1u;
    const int lw = wid & 3;
    unsigned voff;                                          // this lane's 16 B inside a piece
    {
        const int row = lane >> 2, slot = lane & 3;         // a piece = 16 rows x 4 slots; LDS slot s of row r holds source slot s ^ 2 * bit3(r)
        voff = (unsigned)(row * SP_ROWB + ((slot ^ (((row >> 3) & 1) << 1)) << 4));
    }
    const long long slice_b = lw < 2 ? p.wslice_b : p.xslice_b;
    const long long tile_off = (lw < 2 ? (long long)tile_n * SP_BM * SP_ROWB : tile_m * SP_BN * SP_ROWB) + (lw & 1) * (SP_OP / 2);
    const int piece_sel = late ? 0 : 1;                     // late waves stage the first pieces (W1 / h1), early ones the second
    const char* src = uniform_ptr((lw < 2 ? p.W[piece_sel] : p.X[piece_sel]) + tile_off);
    const unsigned lds_mine = lds_base + (late ? (unsigned)SP_RING_A : (unsigned)SP_RING_B) + (unsigned)(lw >> 1) * SP_OP +
                              (unsigned)(lw & 1) * (SP_OP / 2);                // inside slot 0 of this wave's ring
    const int ns = p.ns;

    // ---- fragment read addresses: lane (i, kq) -> row i, slot kq ^ 2 * bit3(i) of a 16-row block
    const int i = lane & 15;
    const int kq = lane >> 4;
    typedef const __attribute__((address_space(3))) u32x4_t* lds_u4p;
    const lcptr_t lbase = (lcptr_t)(lptr_t)smem_sp;
    const unsigned rd_l = (unsigned)(i * SP_ROWB + ((kq ^ (((i >> 3) & 1) << 1)) << 4));
    const unsigned rdW = rd_l + (unsigned)wr * (SP_OP / 2);                      // weight fragment T at + T KiB inside a slot
    const unsigned rdH = rd_l + (unsigned)SP_OP + (unsigned)wc * (SP_OP / 4);    // activation fragment c at + c KiB
    unsigned sb = 0;          // byte offset of the (W2, h2) slot of the current slice: s % 2
    unsigned sa_next = SP_PAIR_B;   // ... of the (W1, h1) slot of slice s + 1: (s + 1) % 3
    unsigned sa_free = 0;           // ... of slice s's own (W1, h1) slot, refilled with slice s + 3: s % 3

    f32x4_t acc[8][4];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[t][c] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    u32x4_t fW1[8], fW2[8], fhA[4], fhB[4];

#define SP_READ_W(DST, BASE) _Pragma("unroll") for (int tt = 0; tt < 8; ++tt) DST[tt] = *(lds_u4p)(lbase + (BASE) + rdW + tt * 1024)
#define SP_READ_H(DST, BASE) _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = *(lds_u4p)(lbase + (BASE) + rdH + c * 1024)
    // MFMAs E0 .. E0 + NE - 1 of one product, in the order e -> (tile e / 4, row block e % 4)
#define SP_MFMA(FA, FB, E0, NE)                                                                                  \
    do {                                                                                                         \
        _Pragma("unroll") for (int e = (E0); e < (E0) + (NE); ++e)                                               \
            acc[e >> 2][e & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(                                         \
                __builtin_bit_cast(f16x8_t, FA[e >> 2]), __builtin_bit_cast(f16x8_t, FB[e & 3]), acc[e >> 2][e & 3], 0, 0, 0); \
    } while (0)
    // "N times one MFMA, then one LDS read" for the scheduler: the fragment reads ride in the issue slots an MFMA leaves
    // (it holds the SIMD's vector issue for 8 of its 16 cycles), not in a block of their own with the matrix pipe idle
#define SP_PAIR(N) _Pragma("unroll") for (int z_ = 0; z_ < (N); ++z_) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#define SP_ONLY_MFMA(N) __builtin_amdgcn_sched_group_barrier(0x008, (N), 0)
    // pieces 4 Q .. 4 Q + 3 (Q = 0, 1) of slice S2's pair into the slot at byte SLOT of this wave's ring, issued by the
    // waves whose ON is set (past the end: clamped -- the redundant DMA lands in a dead slot and keeps the vmcnt
    // bookkeeping uniform); the other waves jump over the statement
#define SP_ISSUE4(ON, SLOT, S2, Q)                                                                               \
    do {                                                                                                         \
        const int ss_ = (S2) < ns ? (S2) : ns - 1;                                                               \
        dma_run4_if(ON, voff, src + (long long)ss_ * slice_b + (Q) * 4096, lds_mine + (SLOT) + (Q) * 4096);      \
    } while (0)

    // One slice, entered with W1 and HCUR = h1 of it in registers; leaves W1 and HNXT = h1 of the next.
#define SP_STEP(S, HCUR, HNXT)                                                                                   \
    do {                                                                                                         \
        SP_READ_H(HNXT, SP_RING_B + sb);                           /* h2 (s) */                                   \
        SP_READ_W(fW2, SP_RING_B + sb);                            /* W2 (s) */                                   \
        SP_MFMA(fW1, HCUR, 0, 32);                                 /* P1 = h1 . W1, the twelve reads between */   \
        SP_PAIR(12); SP_ONLY_MFMA(20);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        sp_wait_vmcnt_by<0, 8>(late);                              /* early: (W2, h2) of s + 1 landed; late: all but its youngest (W1, h1) pair */ \
        DLC_WAIT_LGKM0();                                          /* this wave's reads of slice s are done */     \
        wg_barrier();                                              /* slice s is dead; slice s + 1 is visible */  \
        SP_ISSUE4(early, sb, (S) + 2, 0);                          /* (W2, h2) of s + 2: wanted in one period */  \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_MFMA(fW1, HNXT, 0, 4);                                  /* P2 = h2 . W1 */                            \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_ISSUE4(early, sb, (S) + 2, 1);                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_MFMA(fW1, HNXT, 4, 28);                                                                               \
        SP_READ_H(HNXT, SP_RING_A + sa_next);                      /* h1, W1 (s + 1) */                           \
        SP_READ_W(fW1, SP_RING_A + sa_next);                                                                     \
        SP_MFMA(fW2, HCUR, 0, 12);                                 /* P3 = h1 . W2 */                            \
        SP_ONLY_MFMA(28); SP_PAIR(12);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_ISSUE4(late, sa_free, (S) + 3, 0);                      /* (W1, h1) of s + 3: two periods to land */  \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_MFMA(fW2, HCUR, 12, 4);                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_ISSUE4(late, sa_free, (S) + 3, 1);                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        SP_MFMA(fW2, HCUR, 16, 16);                                                                              \
        sb ^= SP_PAIR_B;                                                                                         \
        sa_free = sa_next;                                                                                       \
        sa_next = sa_next == 2 * SP_PAIR_B ? 0u : sa_next + SP_PAIR_B;                                           \
    } while (0)

    // this thread's bias of the tile (threads 0 .. 255), folded for the epilogue's one fma (see there); fetched here, a
    // register across the k loop, because behind the loop its miss was 2 000 cycles that every wave of the tile waited for
    float bias_l = 0.0f;
    if (tid < SP_BM) {
        const int n = tile_n * SP_BM + tid;
        if constexpr (CONV) bias_l = (float)((p.bias && n < p.N) ? p.bias[n] : 0.0);
        else bias_l = (float)(-1.4426950408889634 * ((p.bias && n < p.N) ? p.bias[n] : 0.0) - (FINAL ? 0.0 : (double)SP_X_SHIFT));
    }
    // ---- prologue: early waves issue (W2, h2) of slices 0, 1; late waves (W1, h1) of slices 0, 1, 2; slice 0 landed and
    // visible; W1, h1 (0) read
    SP_ISSUE4(early, 0, 0, 0); SP_ISSUE4(early, 0, 0, 1);
    SP_ISSUE4(early, SP_PAIR_B, 1, 0); SP_ISSUE4(early, SP_PAIR_B, 1, 1);
    SP_ISSUE4(late, 0, 0, 0); SP_ISSUE4(late, 0, 0, 1);
    SP_ISSUE4(late, SP_PAIR_B, 1, 0); SP_ISSUE4(late, SP_PAIR_B, 1, 1);
    SP_ISSUE4(late, 2 * SP_PAIR_B, 2, 0); SP_ISSUE4(late, 2 * SP_PAIR_B, 2, 1);
    sp_wait_vmcnt_by<8, 16>(late);                             // slice 0 landed (this wave's share)
    wg_barrier();
    SP_READ_W(fW1, SP_RING_A + 0);
    SP_READ_H(fhA, SP_RING_A + 0);
    for (int s = 0; s < ns; s += 2) {
        SP_STEP(s, fhA, fhB);
        if (s + 1 < ns) SP_STEP(s + 1, fhB, fhA);
    }
    DLC_WAIT_VMCNT(0);   // the clamped tail DMAs must not outlive the workgroup's LDS
    DLC_WAIT_LGKM0();
#undef SP_STEP
#undef SP_ISSUE4
#undef SP_PAIR
#undef SP_ONLY_MFMA
#undef SP_READ_W
#undef SP_READ_H
#undef SP_MFMA

    // ---- epilogue.  C/D layout: column = lane & 15 -> activation row, row = 4 * (lane >> 4) + reg -> weight column; with
    // the permuted panel rows, acc[th * 4 + tt][c][r] is output (m, n0 + 4 tt + r): sixteen consecutive columns per (c, th).
    const int lg = lane >> 4;
    // sigmoid(z) = 1 / (1 + 2^(-z log2 e)), z = acc * inv + b with inv = 1 / (2^11 * the weights' scale), a power of two.
    // The constants are folded into the ONE fma in front of v_exp_f32: zl = acc * (-inv log2 e) + (-b log2 e); a hidden
    // layer wants h * 2^11 = 1 / (2^-11 + 2^(zl - 11)), so its -11 rides in the staged bias too.  The reciprocal is
    // v_rcp_f32 (1 ulp): `1.0f / x` and __frcp_rn are the IEEE division here -- ten instructions per element, 1280 per lane
    // and tile, a third of the epilogue (the tolerance of this mode is 2^-15 of the descriptors, not the last bit).
    const float ninv = -1.4426950408889634f / ((float)(1 << SP_X_SHIFT) * p.wscale[0]);
    const float one = FINAL ? 1.0f : 1.0f / (float)(1 << SP_X_SHIFT);
    // the tile's 256 biases through LDS (the ring is dead): ONE global load per thread; a lane's sixteen then come as four
    // 16-byte LDS reads (read straight from memory they were 32 dependent 8-byte loads per lane: a tenth of a tile's time)
    {
        wg_barrier();                                          // every wave is past its last fragment read
        float* bl = (float*)smem_sp;
        if (tid < SP_BM) bl[tid] = bias_l;
        __syncthreads();
    }
    constexpr int SP_TP = 68;                                 // floats per row of a wave's 64 x 64 block: 16 rows of float4 writes / a row of float2 reads each sweep the 64 banks once
    float* tl = (float*)(smem_sp + 4096) + wid * 64 * SP_TP;  // (behind the biases; 8 waves x 17 KiB)
    // SP_CONV: this lane's running min / max of its row of each c (over both column halves), and "saw a non-finite value"
    float rmn[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, rmx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
#pragma unroll
    for (int th = 0; th < 2; ++th) {
        const int n0 = tile_n * SP_BM + wr * 128 + th * 64 + 16 * lg;
        const bool whole = tile_n * SP_BM + wr * 128 + th * 64 + 64 <= p.N;      // all 64 columns of this wave's half exist
        float bv[16];
        {
            const float4* b4 = (const float4*)((const float*)smem_sp + wr * 128 + th * 64 + 16 * lg);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = b4[j];
                bv[4 * j] = v.x; bv[4 * j + 1] = v.y; bv[4 * j + 2] = v.z; bv[4 * j + 3] = v.w;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long m = tile_m * SP_BN + wc * 64 + c * 16 + i;
            float hv[16];
            if constexpr (CONV) {
                // y = acc 2^-(sx + sw) + b with sx the exponent of row m's FRAME (both factors powers of two: exact), ReLU
                // (cnn_vtl.py:33-93) or none, fp32 [M, N]: the NHWC output.  A NaN stays a NaN (v < 0 is false for it).
                // Rows past M store nothing and fold nothing.
                const long long m0 = tile_m * SP_BN + wc * 64 + c * 16;         // the wave's 16 rows of this c (wave-uniform)
                if (m0 >= p.M) continue;
                const bool valid = m < p.M;
                const float xi = p.xinv[(unsigned)(valid ? m : p.M - 1) / p.rows_per_frame];
                const float wi = 1.0f / p.wscale[0];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = fmaf(acc[th * 4 + tt][c][r] * xi, wi, bv[4 * tt + r]);
                        v = (p.relu && v < 0.0f) ? 0.0f : v;
                        hv[4 * tt + r] = v;
                        if (valid && (whole || n0 + 4 * tt + r < p.N)) {
                            rmn[c] = fminf(rmn[c], v);
                            rmx[c] = fmaxf(rmx[c], v);
                            bad |= !(fabsf(v) <= 3.402823466e38f);
                        }
                    }
                if (valid) {
                    float* dst = p.Cf + m * p.N + n0;
                    if (whole && (p.N & 3) == 0) {
#pragma unroll
                        for (int j = 0; j < 16; j += 4) *(float4*)(dst + j) = make_float4(hv[j], hv[j + 1], hv[j + 2], hv[j + 3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            if (n0 + j < p.N) dst[j] = hv[j];
                    }
                }
                continue;
            }
            if (m >= p.M) continue;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float zl = fmaf(acc[th * 4 + tt][c][r], ninv, bv[4 * tt + r]);
                    hv[4 * tt + r] = __builtin_amdgcn_rcpf(one + __builtin_amdgcn_exp2f(zl));   // sigmoid (TensorflowWrapper.py:77-78) [* 2^11]
                }
            if constexpr (FINAL) {
                // into the wave's LDS block, row (c, i), columns 16 lg .. + 15: the stores below want whole rows
                float* row = tl + (c * 16 + i) * SP_TP + 16 * lg;
#pragma unroll
                for (int j = 0; j < 16; j += 4) *(float4*)(row + j) = make_float4(hv[j], hv[j + 1], hv[j + 2], hv[j + 3]);
            } else {
                // the next layer's two pieces of h * 2^11; columns past N are zeros there (its weights' k rows past N too)
                unsigned w1[8], w2[8];
                if (!whole) {                                  // (wave-uniform: only the last column tile has such columns)
#pragma unroll
                    for (int j = 0; j < 16; ++j) hv[j] = n0 + j < p.N ? hv[j] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 16; j += 2) {
                    const f32x2_t v = {hv[j], hv[j + 1]};
                    const f16x2_t a = __builtin_convertvector(v, f16x2_t);                 // v_cvt_pk_f16_f32
                    const f16x2_t b = __builtin_convertvector(v - __builtin_convertvector(a, f32x2_t), f16x2_t);
                    w1[j >> 1] = __builtin_bit_cast(unsigned, a);
                    w2[j >> 1] = __builtin_bit_cast(unsigned, b);
                }
                // K32-major: columns n0 .. n0 + 15 are half of row m's 64 bytes in slice n0 / 32 -- the wave's 64 columns are two
                // slices, lanes 0-31 hold the first one's.  Stored as they lie, an instruction wrote 16 of every row's 64 bytes
                // in each slice; v_permlane32_swap trades the second 16 bytes of the lower lanes for the first 16 of the upper
                // ones, and every instruction writes ONE slice: sixteen rows x 64 bytes = 1 KiB in a piece.
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const u32x2_t s1 = __builtin_amdgcn_permlane32_swap(w1[e], w1[4 + e], false, false);
                    const u32x2_t s2 = __builtin_amdgcn_permlane32_swap(w2[e], w2[4 + e], false, false);
                    w1[e] = s1[0]; w1[4 + e] = s1[1];
                    w2[e] = s2[0]; w2[4 + e] = s2[1];
                }
                const int nb = tile_n * SP_BM + wr * 128 + th * 64;                      // the wave's 64 columns: slices nb / 32, + 1
                const long long o = (long long)(nb >> 5) * p.oslice_b + m * SP_ROWB + (lg & 1) * 32 + (lg >> 1) * 16;
                char* o1 = p.O[0] + o;
                char* o2 = p.O[1] + o;
                *(uint4*)o1 = make_uint4(w1[0], w1[1], w1[2], w1[3]);
                *(uint4*)(o1 + p.oslice_b) = make_uint4(w1[4], w1[5], w1[6], w1[7]);
                *(uint4*)o2 = make_uint4(w2[0], w2[1], w2[2], w2[3]);
                *(uint4*)(o2 + p.oslice_b) = make_uint4(w2[4], w2[5], w2[6], w2[7]);
            }
        }
        if constexpr (FINAL) {
            // fp64 out, a ROW at a time: the wave's 64 rows x 64 columns come back from LDS with 32 lanes on one row's 512
            // bytes, two rows per store instruction.  (Stored from the accumulators' layout every lane wrote 16 bytes of a
            // different cache line: 64 lines per instruction, 0.14 ms of this layer's 0.99.)
            DLC_WAIT_LGKM0();
            __builtin_amdgcn_wave_barrier();
            const int nb = tile_n * SP_BM + wr * 128 + th * 64, cj = 2 * (lane & 31);
            const bool pairs = (p.ldc & 1) == 0 && ((unsigned long long)p.C & 15) == 0;
#pragma unroll 4
            for (int it = 0; it < 32; ++it) {
                const int r = 2 * it + (lane >> 5);
                const long long m = tile_m * SP_BN + wc * 64 + r;
                const float2 v = *(const float2*)(tl + r * SP_TP + cj);
                if (m >= p.M) continue;
                double* dst = p.C + m * p.ldc + nb + cj;
                if (pairs && nb + cj + 2 <= p.N) *(double2*)dst = make_double2((double)v.x, (double)v.y);
                else {
                    if (nb + cj < p.N) dst[0] = (double)v.x;
                    if (nb + cj + 1 < p.N) dst[1] = (double)v.y;
                }
            }
            DLC_WAIT_LGKM0();                                      // the next half's rows overwrite the block
            __builtin_amdgcn_wave_barrier();
        }
    }
    if constexpr (CONV) {
        // per-frame min / max of the outputs into the ordered fp64 keys (dlc_f64_key; cnn_vtl.py:110-112 takes them over the
        // whole descriptor of a frame).  Wave-uniform tests: the wave's 64 rows in ONE frame -> one reduction and one pair
        // of atomics; otherwise per block of 16 rows, and a block that spans frames leaves a pair per row.
        if (p.keys) {
            if (bad) atomicOr(p.status, 2);
            const long long w0 = tile_m * SP_BN + wc * 64;
            if (w0 < p.M) {
                const long long wl = w0 + 63 < p.M ? w0 + 63 : p.M - 1;
                const unsigned fw = (unsigned)w0 / p.rows_per_frame;
                if (fw == (unsigned)wl / p.rows_per_frame) {
                    float mn = fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
                    float mx = fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
                    if (lane == 0 && mn <= mx) {
                        atomicMin(&p.keys[2 * (size_t)fw], dlc_f64_key((double)mn));
                        atomicMax(&p.keys[2 * (size_t)fw + 1], dlc_f64_key((double)mx));
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const long long m0 = w0 + c * 16, m = m0 + i;
                        if (m0 >= p.M) continue;
                        float mn = rmn[c], mx = rmx[c];
                        mn = fminf(mn, __shfl_xor(mn, 32)); mx = fmaxf(mx, __shfl_xor(mx, 32));     // the four lanes of a row
                        mn = fminf(mn, __shfl_xor(mn, 16)); mx = fmaxf(mx, __shfl_xor(mx, 16));
                        const long long ml = m0 + 15 < p.M ? m0 + 15 : p.M - 1;
                        const unsigned f0 = (unsigned)m0 / p.rows_per_frame;
                        if (f0 == (unsigned)ml / p.rows_per_frame) {
#pragma unroll
                            for (int o = 8; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
                            if (lane == 0 && mn <= mx) {
                                atomicMin(&p.keys[2 * (size_t)f0], dlc_f64_key((double)mn));
                                atomicMax(&p.keys[2 * (size_t)f0 + 1], dlc_f64_key((double)mx));
                            }
                        } else if (lg == 0 && m < p.M && mn <= mx) {
                            const unsigned f = (unsigned)m / p.rows_per_frame;
                            atomicMin(&p.keys[2 * (size_t)f], dlc_f64_key((double)mn));
                            atomicMax(&p.keys[2 * (size_t)f + 1], dlc_f64_key((double)mx));
                        }
                    }
                }
            }
        }
    }
}

// ---- operand preparation --------------------------------------------------------------------------------------------

// largest |w| of a weight matrix -> bits of a non-negative double (they order like the values)
__global__ __launch_bounds__(256) void sp_absmax_kernel(const double* __restrict__ w, long long n, unsigned long long* out) {
    double m = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) m = fmax(m, fabs(w[e]));
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(m));     // (a NaN never wins: fmax drops it)
}
// 2^s with the layer's largest |W| 2^s in [2048, 4096) (1 for a zero matrix), as the float the GEMM's epilogue divides by
__global__ void sp_scale_kernel(const unsigned long long* amax, float* wscale) {
    if (threadIdx.x != 0) return;
    const double m = __longlong_as_double((long long)*amax);
    int e = 0;
    if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);                   // m = f 2^e, f in [0.5, 1)
    int s = (m > 0.0 && m < INFINITY) ? 12 - e : 0;                     // m 2^s = f 2^12 in [2048, 4096)
    s = s > 100 ? 100 : (s < -100 ? -100 : s);
    *wscale = (float)ldexp(1.0, s);
}
// panel row of weight column n: inside every 64 columns, column 16 g + 4 t + r sits at row 16 t + 4 g + r (the kernel's header)
__device__ __forceinline__ long long sp_panel_row(long long n) {
    const int c = (int)(n & 63);
    return (n & ~63ll) | (long long)((((c >> 2) & 3) << 4) | ((c >> 4) << 2) | (c & 3));
}
// W [K, N] fp64 -> its two fp16 pieces, K32-major [kp / 32][Np rows][32] (k contiguous inside a row's 64 bytes), zeros past
// K / N: 64 x 64 tiles through LDS
__global__ __launch_bounds__(256) void sp_split_weights_kernel(const double* __restrict__ w, long long K, long long N, const float* wscale,
                                                               unsigned short* __restrict__ p1, unsigned short* __restrict__ p2,
                                                               long long np) {
    __shared__ float t1[64][65], t2[64][65];
    const long long n0 = (long long)blockIdx.x * 64, k0 = (long long)blockIdx.y * 64;
    const double sc = (double)wscale[0];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int kk = ty; kk < 64; kk += 4) {
        const long long k = k0 + kk, n = n0 + tx;
        const double v = (k < K && n < N) ? w[k * N + n] * sc : 0.0;
        const _Float16 a = (_Float16)v;
        const _Float16 b = (_Float16)(v - (double)a);
        t1[kk][tx] = (float)a;
        t2[kk][tx] = (float)b;
    }
    __syncthreads();
    for (int nn = ty; nn < 64; nn += 4) {
        const long long k = k0 + tx;
        const long long o = ((k >> 5) * np + sp_panel_row(n0 + nn)) * SP_KS + (k & 31);
        p1[o] = __builtin_bit_cast(unsigned short, (_Float16)t1[tx][nn]);
        p2[o] = __builtin_bit_cast(unsigned short, (_Float16)t2[tx][nn]);
    }
}
// x [rows, K] fp64 -> the two fp16 pieces of x 2^11, K32-major [kp / 32][mp rows][32], zeros past K (rows past `rows` are
// never read into a stored output and stay unwritten).  645 MB in 170 us for 1063 frames = 3.8 TB/s, the rate of a device copy
// on this chip; two other forms were measured and dropped: eight consecutive k per thread (64 cache lines per load instruction:
// 258 us) and 32 rows x 256 k per workgroup turned through LDS (whole-KiB stores, 256-byte reads: 211 us).
__global__ __launch_bounds__(256) void sp_split_rows_kernel(const double* __restrict__ x, long long rows, long long K, long long kp,
                                                            unsigned short* __restrict__ p1, unsigned short* __restrict__ p2,
                                                            long long mp) {
    const long long total = rows * kp;
    const double sc = (double)(1 << SP_X_SHIFT);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / kp, k = e - r * kp;
        const double v = k < K ? x[r * K + k] * sc : 0.0;
        const _Float16 a = (_Float16)v;
        const long long o = ((k >> 5) * mp + r) * SP_KS + (k & 31);
        p1[o] = __builtin_bit_cast(unsigned short, a);
        p2[o] = __builtin_bit_cast(unsigned short, (_Float16)(v - (double)a));
    }
}

struct PanelLayout {
    size_t scale, amax, p1, p2, total;          // byte offsets inside one layer's panel block
    long long np, kp;
};
PanelLayout panel_layout(int64_t K, int64_t N) {
    PanelLayout L;
    L.np = (long long)dlc::align_up((size_t)N, (size_t)SP_BM);
    L.kp = (long long)dlc::align_up((size_t)K, 64);           // (whole 64 x 64 tiles of the preparation kernel; the GEMM walks align(K, 32))
    L.scale = 0; L.amax = 8;
    L.p1 = 256;
    L.p2 = L.p1 + dlc::align_up((size_t)L.np * L.kp * 2, 256);
    L.total = L.p2 + dlc::align_up((size_t)L.np * L.kp * 2, 256);
    return L;
}

}  // namespace

size_t split_panels_bytes(int n_layers, const int64_t* dims) {
    size_t t = 0;
    for (int l = 0; l < n_layers; ++l) t += panel_layout(dims[l], dims[l + 1]).total;
    return t;
}

int split_prepare(dlc_ctx* ctx, int n_layers, const int64_t* dims, const double* const* W, char* panels, hipStream_t st) {
    size_t off = 0;
    for (int l = 0; l < n_layers; ++l) {
        const PanelLayout L = panel_layout(dims[l], dims[l + 1]);
        char* base = panels + off;
        DLC_HIP_CHECK(ctx, hipMemsetAsync(base, 0, 256, st));
        const long long n = dims[l] * dims[l + 1];
        hipLaunchKernelGGL(sp_absmax_kernel, dim3(1024), dim3(256), 0, st, W[l], n, (unsigned long long*)(base + L.amax));
        hipLaunchKernelGGL(sp_scale_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)(base + L.amax), (float*)(base + L.scale));
        hipLaunchKernelGGL(sp_split_weights_kernel, dim3((unsigned)(L.np / 64), (unsigned)(L.kp / 64)), dim3(256), 0, st, W[l],
                           (long long)dims[l], (long long)dims[l + 1], (const float*)(base + L.scale), (unsigned short*)(base + L.p1),
                           (unsigned short*)(base + L.p2), L.np);
        DLC_LAUNCH_CHECK(ctx, "sp_split_weights_kernel");
        off += L.total;
    }
    return DLC_OK;
}

// the k-slices an activation piece holds for a layer input of width K: whole 256-column output tiles of the layer before
static long long split_slices(int64_t K) { return (long long)dlc::align_up((size_t)K, (size_t)SP_BM) / SP_KS; }
// ... and its rows: whole 256-row tiles (the GEMM stages full tiles; rows past the last are never stored)
static long long split_rows_pad(int64_t rows) { return (long long)dlc::align_up((size_t)rows, (size_t)SP_BN); }

size_t split_encode_workspace_bytes(int64_t rows, const int64_t* dims, int n_layers) {
    long long smax = 0;
    for (int l = 0; l < n_layers; ++l) smax = split_slices(dims[l]) > smax ? split_slices(dims[l]) : smax;
    return 4 * dlc::align_up((size_t)split_rows_pad(rows) * (size_t)smax * SP_ROWB, 256);          // two ping-pong buffers of two pieces
}

int split_encode(dlc_ctx* ctx, int64_t rows, int n_layers, const int64_t* dims, const double* x, const char* panels,
                 const double* const* b, double* out, char* ws, hipStream_t st) {
    long long smax = 0;
    for (int l = 0; l < n_layers; ++l) smax = split_slices(dims[l]) > smax ? split_slices(dims[l]) : smax;
    const long long mp = split_rows_pad(rows);
    const size_t piece = dlc::align_up((size_t)mp * (size_t)smax * SP_ROWB, 256);
    char* buf[2][2] = {{ws, ws + piece}, {ws + 2 * piece, ws + 3 * piece}};
    {
        const long long kp = (long long)dlc::align_up((size_t)dims[0], (size_t)SP_KS);
        long long blocks = dlc::cdiv(rows * kp, (int64_t)256);
        if (blocks > 256 * 32) blocks = 256 * 32;
        hipLaunchKernelGGL(sp_split_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, (long long)rows, (long long)dims[0], kp,
                           (unsigned short*)buf[0][0], (unsigned short*)buf[0][1], mp);
        DLC_LAUNCH_CHECK(ctx, "sp_split_rows_kernel");
    }
    if (!(ctx->func_attr_set & (1ull << DLC_ATTR_SPLIT_F16))) {
        DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)gemm_split_f16_kernel<SP_HIDDEN>, hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS));
        DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)gemm_split_f16_kernel<SP_FINAL>, hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS));
        ctx->func_attr_set |= 1ull << DLC_ATTR_SPLIT_F16;
    }
    size_t off = 0;
    for (int l = 0; l < n_layers; ++l) {
        const PanelLayout L = panel_layout(dims[l], dims[l + 1]);
        const char* base = panels + off;
        SplitArgs a;
        a.W[0] = base + L.p1; a.W[1] = base + L.p2; a.wslice_b = L.np * SP_ROWB;
        a.X[0] = buf[l & 1][0]; a.X[1] = buf[l & 1][1]; a.xslice_b = mp * SP_ROWB;
        a.M = rows; a.N = (int)dims[l + 1]; a.ns = (int)dlc::cdiv(dims[l], (int64_t)SP_KS);
        a.bias = b ? b[l] : nullptr;
        a.wscale = (const float*)(base + L.scale);
        const bool fin = l == n_layers - 1;
        a.O[0] = fin ? nullptr : buf[(l + 1) & 1][0]; a.O[1] = fin ? nullptr : buf[(l + 1) & 1][1];
        a.oslice_b = fin ? 0 : mp * SP_ROWB;
        a.C = fin ? out : nullptr; a.ldc = dims[l + 1];
        a.tiles_m = dlc::cdiv(rows, (int64_t)SP_BN);
        a.tiles_n = (int)(L.np / SP_BM);
        const long long tiles = a.tiles_m * a.tiles_n;
        a.per_xcd = tiles / 8; a.extra = tiles % 8;
        const long long nwg = (a.per_xcd + (a.extra ? 1 : 0)) * 8;
        if (nwg > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sdav_encode_split: too many tiles");
        const int rc = dlc::profiled(ctx, st, [&]() -> int {
            if (fin) hipLaunchKernelGGL(gemm_split_f16_kernel<SP_FINAL>, dim3((unsigned)nwg), dim3(SP_THREADS), SP_LDS, st, a);
            else hipLaunchKernelGGL(gemm_split_f16_kernel<SP_HIDDEN>, dim3((unsigned)nwg), dim3(SP_THREADS), SP_LDS, st, a);
            DLC_LAUNCH_CHECK(ctx, "gemm_split_f16_kernel");
            return DLC_OK;
        });
        if (rc != DLC_OK) return rc;
        off += L.total;
    }
    return DLC_OK;
}

}  // namespace dlc_gemm

extern "C" size_t dlc_sdav_split_panels_bytes(int n_layers, const int64_t* dims) {
    if (!dims || n_layers < 1) return 0;
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return 0;
    return dlc_gemm::split_panels_bytes(n_layers, dims);
}

extern "C" int dlc_sdav_split_prepare(dlc_ctx* ctx, int n_layers, const int64_t* dims, const double* const* W, void* panels,
                                      size_t panels_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!dims || !W || !panels || n_layers < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sdav_split_prepare: null/empty argument");
    const size_t need = dlc_sdav_split_panels_bytes(n_layers, dims);
    if (need == 0) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sdav_split_prepare: bad dims");
    if (panels_bytes < need) return dlc::fail(ctx, DLC_ERR_WORKSPACE, "sdav_split_prepare: panels %zu < %zu bytes", panels_bytes, need);
    if ((uintptr_t)panels & 255) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sdav_split_prepare: panels must be 256-byte aligned");
    for (int l = 0; l < n_layers; ++l)
        if (!W[l]) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sdav_split_prepare: W[%d] is null", l);
    DLC_ON_DEVICE(ctx);
    return dlc_gemm::split_prepare(ctx, n_layers, dims, W, (char*)panels, (hipStream_t)stream);
}

extern "C" size_t dlc_sdav_encode_split_workspace_bytes(int64_t rows, const int64_t* dims, int n_layers) {
    if (rows < 1 || !dims || n_layers < 1) return 0;
    return dlc_gemm::split_encode_workspace_bytes(rows, dims, n_layers);
}

extern "C" int dlc_sdav_encode_split(dlc_ctx* ctx, int64_t rows, int n_layers, const int64_t* dims, const double* x,
                                     const void* panels, const double* const* b, double* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!dims || !x || !panels || !out || rows < 1 || n_layers < 1)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sdav_encode_split: null/empty argument");
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sdav_encode_split: dims[%d] = %lld", l, (long long)dims[l]);
    if (rows * 4096 > 0x7fffffffll * 64) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "sdav_encode_split: too many rows");
    const size_t need = dlc_sdav_encode_split_workspace_bytes(rows, dims, n_layers);
    if (!workspace || workspace_bytes < need)
        return dlc::fail(ctx, DLC_ERR_WORKSPACE, "sdav_encode_split: workspace %zu < %zu bytes", workspace_bytes, need);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)panels & 255))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "sdav_encode_split: workspace and panels must be 256-byte aligned");
    DLC_ON_DEVICE(ctx);
    return dlc_gemm::split_encode(ctx, rows, n_layers, dims, x, (const char*)panels, b, out, (char*)workspace, (hipStream_t)stream);
}

// ======================================================================================================================
// CnnVtl in the same TOLERANCE mode (dlc_cnnvtl_encode_split; cnn_vtl.py:28-128): every convolution y = act(conv(x, W) + b)
// is the split GEMM above over the convolution's im2col rows.  What differs from the SDAV chain:
//   * activations are not in [0, 1] (ReLU, pixels 0 .. 255 fed unscaled: create_distance_matrix.py:23,27), so the activation
//     exponent is ONE POWER OF TWO PER FRAME AND LAYER, from that frame's own max |x| of the layer's input: x 2^sx, the
//     frame's largest scaled magnitude in [1024, 2048) (sx = 0 for an all-zero frame).  Per frame, not per chunk: a
//     frame's descriptor does not depend on the batch it is encoded in;
//   * the activation operand is written by cs_im2col_split_kernel: im2col and split in one pass over the fp32 NHWC
//     input, zero padding and the zero k-tail written as zeros, straight into the K32-major pieces;
//   * the epilogue (MODE SP_CONV) descales per row's frame, adds the bias, applies ReLU / none in fp32 and stores fp32 NHWC;
//     max-pool runs on those fp32 values; the features that reach the quantiser are the fp32 layer outputs, promoted to
//     fp64 for the reference's formula (cnn_vtl.py:108-128) -- the per-frame min / max folded by the same epilogue into
//     the ordered keys the fp64 mode folds (dlc_f64_key; a tile may span several frames).
// Non-finite values (in the input or produced on the way: a frame whose max |x| is inf / NaN, an output that is) set
// bits of a device status word instead of travelling on as bytes: 1 = a layer input, 2 = a layer output.
namespace dlc_gemm {
namespace {

constexpr int CS_GEOM = 11;     // ints per layer of the geometry array: kh kw cin cout stride pad_top pad_left oh ow act pool
struct CsGeom { int kh, kw, cin, cout, stride, pt, pl, oh, ow, act, pool; };
CsGeom cs_geom(const int32_t* g, int l) {
    const int32_t* q = g + (size_t)l * CS_GEOM;
    return CsGeom{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10]};
}
bool cs_geom_ok(const CsGeom& g) {
    return g.kh >= 1 && g.kw >= 1 && g.cin >= 1 && g.cout >= 1 && g.stride >= 1 && g.pt >= 0 && g.pl >= 0 && g.oh >= 1 && g.ow >= 1 &&
           (g.act == DLC_ACT_NONE || g.act == DLC_ACT_RELU) && (g.pool == 0 || (g.pool == 1 && g.oh >= 3 && g.ow >= 3)) &&
           (long long)g.kh * g.kw * g.cin <= (1 << 24) && g.cout <= (1 << 20);
}

// frames [n, h, w, c] (uint8 / fp32 / fp64) -> fp32 [n, h/s, w/s, s*s*c], space-to-depth with block s (s = 1: a plain
// conversion; the index map of dlc_space_to_depth_nhwc_f64)
template <typename T>
__global__ __launch_bounds__(256) void cs_input_kernel(const T* __restrict__ x, long long n, int h, int w, int c, int s,
                                                       float* __restrict__ y) {
    const int oh = h / s, ow = w / s, sc = s * c, oc = s * sc;
    const long long total = n * oh * ow * oc;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int k = (int)(e % oc);
        long long t = e / oc;
        const int ox = (int)(t % ow);
        t /= ow;
        const int oy = (int)(t % oh);
        const long long img = t / oh;
        const int dy = k / sc, rem = k - dy * sc;
        y[e] = (float)x[((img * h + (long long)oy * s + dy) * w + (long long)ox * s) * c + rem];
    }
}

// per-frame max |x| as the bits of a non-negative float (they order like the values; inf and every NaN sort on top)
__global__ __launch_bounds__(256) void cs_frame_absmax_kernel(const float* __restrict__ x, long long per, unsigned* __restrict__ amax) {
    const float* p = x + (long long)blockIdx.y * per;
    unsigned m = 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const unsigned b = __float_as_uint(p[e]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned q = (unsigned)__shfl_xor((int)m, o); m = q > m ? q : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&amax[blockIdx.y], m);
}
// 2^sx per frame with max |x| 2^sx in [1024, 2048) (sx = 0 for a zero frame, |sx| <= 100), and 2^-sx
__global__ void cs_frame_scale_kernel(const unsigned* __restrict__ amax, long long n, float* __restrict__ xscale,
                                      float* __restrict__ xinv, int* status) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const unsigned b = amax[f];
    int s = 0;
    if (b >= 0x7f800000u) atomicOr(status, 1);
    else if (b) {
        int e;
        (void)frexpf(__uint_as_float(b), &e);                       // m = f 2^e, f in [0.5, 1): m 2^(11 - e) in [1024, 2048)
        s = 11 - e;
        s = s > 100 ? 100 : (s < -100 ? -100 : s);
    }
    xscale[f] = ldexpf(1.0f, s);
    xinv[f] = ldexpf(1.0f, -s);
}

struct Im2colArgs {
    const float* x;             // [n, h, w, c] fp32
    const float* xscale;        // [n] 2^sx
    long long M, mp;            // rows n * oh * ow, and the pieces' padded row count
    int h, w, c, kh, kw, stride, pt, pl, oh, ow;
    int K, ns;                  // kh * kw * c, slices of 32
    unsigned short *p1, *p2;
};
// im2col + split: a workgroup writes 64 rows x every slice (4 KiB contiguous per slice and piece); thread (row, q) the 8
// consecutive k of slot q -- with c % 8 == 0 eight channels of one tap, two 16-byte loads; otherwise element by element
__global__ __launch_bounds__(256) void cs_im2col_split_kernel(Im2colArgs a) {
    const long long m = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
    if (m >= a.M) return;
    const int q = threadIdx.x & 3;
    const int ox = (int)(m % a.ow);
    const long long t = m / a.ow;
    const int oy = (int)(t % a.oh);
    const long long img = t / a.oh;
    const float sc = a.xscale[img];
    const int iy0 = oy * a.stride - a.pt, ix0 = ox * a.stride - a.pl;
    const float* xi = a.x + img * a.h * a.w * a.c;
    const bool vec = (a.c & 7) == 0;
    for (int sl = 0; sl < a.ns; ++sl) {
        const int k0 = sl * 32 + q * 8;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.0f;
        if (vec) {
            if (k0 < a.K) {
                const int tap = k0 / a.c, ch = k0 - tap * a.c;
                const int ky = tap / a.kw, kx = tap - ky * a.kw;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) {
                    const float4* s4 = (const float4*)(xi + ((long long)iy * a.w + ix) * a.c + ch);
                    const float4 u0 = s4[0], u1 = s4[1];
                    v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                if (k < a.K) {
                    const int tap = k / a.c, ch = k - tap * a.c;
                    const int ky = tap / a.kw, kx = tap - ky * a.kw;
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) v[j] = xi[((long long)iy * a.w + ix) * a.c + ch];
                }
            }
        }
        unsigned w1[4], w2[4];
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const f32x2_t s2 = {v[j] * sc, v[j + 1] * sc};
            const f16x2_t h1 = __builtin_convertvector(s2, f16x2_t);
            const f16x2_t h2 = __builtin_convertvector(s2 - __builtin_convertvector(h1, f32x2_t), f16x2_t);
            w1[j >> 1] = __builtin_bit_cast(unsigned, h1);
            w2[j >> 1] = __builtin_bit_cast(unsigned, h2);
        }
        const long long o = ((long long)sl * a.mp + m) * SP_KS + q * 8;
        *(uint4*)(a.p1 + o) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
        *(uint4*)(a.p2 + o) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
    }
}

// tf.layers.max_pooling2d(3x3, stride 2, VALID) on NHWC fp32 (cnn_vtl.py:42-45,58-61)
__global__ __launch_bounds__(256) void cs_maxpool_kernel(const float* __restrict__ x, long long n, int h, int w, int c, int oh, int ow,
                                                         float* __restrict__ y) {
    const long long total = n * oh * ow * c;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % c);
        long long t = e / c;
        const int ox = (int)(t % ow);
        t /= ow;
        const int oy = (int)(t % oh);
        const long long img = t / oh;
        const float* p = x + ((img * h + 2 * oy) * w + 2 * ox) * c + ch;
        float m = p[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float v = p[((long long)dy * w + dx) * c];
                m = (v > m || v != v) ? v : m;                          // a NaN is kept
            }
        y[e] = m;
    }
}

__global__ void cs_keys_init_kernel(unsigned long long* __restrict__ keys, long long n) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < n) { keys[r * 2] = ~0ull; keys[r * 2 + 1] = 0ull; }
}

constexpr int CS_MAX_LAYERS = 8;
struct FSegs {
    const float* ptr[CS_MAX_LAYERS];
    long long size[CS_MAX_LAYERS];
    long long start[CS_MAX_LAYERS + 1];
    int n;
};
// out[r, j] = int8(trunc((d[r, cols[j]] - min_r) * (255 / (max_r - min_r)))), wrap mod 256 -- cnn_vtl.py:108-128 in fp64 on
// the promoted fp32 features, operation for operation what quant_gather_kernel (cnnvtl.hip) does
__global__ __launch_bounds__(256) void cs_quant_gather_kernel(FSegs s, const long long* __restrict__ cols, long long n_cols,
                                                              const unsigned long long* __restrict__ keys, int8_t* __restrict__ out) {
    const long long r = blockIdx.y;
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_cols) return;
    const long long col = cols[j];
    if (col < 0 || col >= s.start[s.n]) { out[r * n_cols + j] = 0; return; }
    int g = 0;
    while (g + 1 < s.n && col >= s.start[g + 1]) ++g;
    const double v = (double)s.ptr[g][r * s.size[g] + (col - s.start[g])];
    const double mn = dlc_f64_unkey(keys[r * 2]), mx = dlc_f64_unkey(keys[r * 2 + 1]);
    const double scaled = (v - mn) * (255.0 / (mx - mn));
    long long t = 0;
    if (scaled == scaled && fabs(scaled) < 9.0e18) t = (long long)scaled;
    out[r * n_cols + j] = (int8_t)(unsigned char)(t & 0xff);
}

size_t a256(size_t v) { return dlc::align_up(v, 256); }

// the workspace of n frames whose first layer reads [h, w, c]: offsets of its parts
struct ConvWs {
    size_t in0, out[CS_MAX_LAYERS], pool[CS_MAX_LAYERS], piece[2], amax, xscale, xinv, keys, status, total;
    int ih[CS_MAX_LAYERS], iw[CS_MAX_LAYERS], ic[CS_MAX_LAYERS];      // each layer's input
};
bool conv_ws(int64_t n, int h, int w, int c, int n_layers, const int32_t* geom, ConvWs* W) {
    size_t off = 0, pmax = 0;
    W->in0 = off; off += a256((size_t)n * h * w * c * 4);
    for (int l = 0; l < n_layers; ++l) {
        const CsGeom g = cs_geom(geom, l);
        if (!cs_geom_ok(g) || g.cin != c) return false;
        W->ih[l] = h; W->iw[l] = w; W->ic[l] = c;
        const long long M = (long long)n * g.oh * g.ow;
        if (M > 0x7fffffffll * 64 / 4096) return false;
        W->out[l] = off; off += a256((size_t)M * g.cout * 4);
        const size_t pb = (size_t)split_rows_pad(M) * (size_t)dlc::cdiv((int64_t)g.kh * g.kw * g.cin, SP_KS) * SP_ROWB;
        pmax = pb > pmax ? pb : pmax;
        h = g.oh; w = g.ow; c = g.cout;
        W->pool[l] = off;
        if (g.pool) {
            h = (h - 3) / 2 + 1; w = (w - 3) / 2 + 1;
            off += a256((size_t)n * h * w * c * 4);
        }
    }
    W->piece[0] = off; off += a256(pmax);
    W->piece[1] = off; off += a256(pmax);
    W->amax = off; off += a256((size_t)n * 4);
    W->xscale = off; off += a256((size_t)n * 4);
    W->xinv = off; off += a256((size_t)n * 4);
    W->keys = off; off += a256((size_t)n * 16);
    W->status = off; off += 256;
    W->total = off;
    return true;
}

unsigned cs_blocks(long long total) {
    long long b = dlc::cdiv(total, (int64_t)256);
    return (unsigned)(b > 256 * 32 ? 256 * 32 : (b < 1 ? 1 : b));
}
// slices of a frame for the per-frame reductions: a handful of frames still fills the chip
unsigned cs_slices(int64_t n, long long per) {
    long long s = dlc::cdiv(per, (int64_t)(256 * 16)), cap = dlc::cdiv((int64_t)4096, n);
    s = s > cap ? cap : s;
    return (unsigned)(s < 1 ? 1 : s);
}

size_t conv_panels_offset(int n_layers, const int32_t* geom, int upto) {
    size_t t = 0;
    for (int l = 0; l < upto && l < n_layers; ++l) {
        const CsGeom g = cs_geom(geom, l);
        t += panel_layout((int64_t)g.kh * g.kw * g.cin, g.cout).total;
    }
    return t;
}

// layers a .. b on n frames; `x` = layer a's fp32 input [n, ih[a], iw[a], ic[a]].  feats[l - a] (may be null, entries too):
// where layer l's output goes instead of the workspace.  keys (may be null): per-frame min / max of every output folded in.
int conv_run_layers(dlc_ctx* ctx, int64_t n, const ConvWs& W, int n_layers, const int32_t* geom, int a, int b, const float* x,
                    const char* panels, const double* const* bias, float* const* feats, const float** outs, char* ws,
                    unsigned long long* keys, int* status, hipStream_t st) {
    if (!(ctx->func_attr_set & (1ull << DLC_ATTR_CONV_SPLIT_F16))) {
        DLC_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)gemm_split_f16_kernel<SP_CONV>, hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS));
        ctx->func_attr_set |= 1ull << DLC_ATTR_CONV_SPLIT_F16;
    }
    unsigned* amax = (unsigned*)(ws + W.amax);
    float* xscale = (float*)(ws + W.xscale);
    float* xinv = (float*)(ws + W.xinv);
    const float* h = x;
    for (int l = a; l <= b; ++l) {
        const CsGeom g = cs_geom(geom, l);
        const int ih = W.ih[l], iw = W.iw[l], ic = W.ic[l];
        const long long per_in = (long long)ih * iw * ic, rpf = (long long)g.oh * g.ow, M = n * rpf;
        const int K = g.kh * g.kw * g.cin, ns = (int)dlc::cdiv((int64_t)K, SP_KS);
        const long long mp = split_rows_pad(M);
        // this layer's exponent per frame
        DLC_HIP_CHECK(ctx, hipMemsetAsync(amax, 0, (size_t)n * 4, st));
        hipLaunchKernelGGL(cs_frame_absmax_kernel, dim3(cs_slices(n, per_in), (unsigned)n), dim3(256), 0, st, h, per_in, amax);
        hipLaunchKernelGGL(cs_frame_scale_kernel, dim3((unsigned)dlc::cdiv(n, (int64_t)256)), dim3(256), 0, st, (const unsigned*)amax,
                           (long long)n, xscale, xinv, status);
        Im2colArgs ia;
        ia.x = h; ia.xscale = xscale; ia.M = M; ia.mp = mp;
        ia.h = ih; ia.w = iw; ia.c = ic; ia.kh = g.kh; ia.kw = g.kw; ia.stride = g.stride; ia.pt = g.pt; ia.pl = g.pl; ia.oh = g.oh; ia.ow = g.ow;
        ia.K = K; ia.ns = ns;
        ia.p1 = (unsigned short*)(ws + W.piece[0]); ia.p2 = (unsigned short*)(ws + W.piece[1]);
        hipLaunchKernelGGL(cs_im2col_split_kernel, dim3((unsigned)dlc::cdiv(M, (int64_t)64)), dim3(256), 0, st, ia);
        DLC_LAUNCH_CHECK(ctx, "cs_im2col_split_kernel");
        float* out = (feats && feats[l - a]) ? feats[l - a] : (float*)(ws + W.out[l]);
        const PanelLayout L = panel_layout(K, g.cout);
        const char* base = panels + conv_panels_offset(n_layers, geom, l);
        ConvSplitArgs p;
        p.W[0] = base + L.p1; p.W[1] = base + L.p2; p.wslice_b = L.np * SP_ROWB;
        p.X[0] = ws + W.piece[0]; p.X[1] = ws + W.piece[1]; p.xslice_b = mp * SP_ROWB;
        p.M = M; p.N = g.cout; p.ns = ns;
        p.bias = bias ? bias[l] : nullptr;
        p.wscale = (const float*)(base + L.scale);
        p.O[0] = p.O[1] = nullptr; p.oslice_b = 0; p.C = nullptr; p.ldc = g.cout;
        p.tiles_m = dlc::cdiv(M, (int64_t)SP_BN);
        p.tiles_n = (int)(L.np / SP_BM);
        const long long tiles = p.tiles_m * p.tiles_n;
        p.per_xcd = tiles / 8; p.extra = tiles % 8;
        p.Cf = out; p.xinv = xinv; p.rows_per_frame = (unsigned)rpf; p.relu = g.act == DLC_ACT_RELU;
        p.keys = keys; p.status = status;
        const long long nwg = (p.per_xcd + (p.extra ? 1 : 0)) * 8;
        if (nwg > 0x7fffffffll) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "cnnvtl_encode_split: too many tiles");
        const int rc = dlc::profiled(ctx, st, [&]() -> int {
            hipLaunchKernelGGL(gemm_split_f16_kernel<SP_CONV>, dim3((unsigned)nwg), dim3(SP_THREADS), SP_LDS, st, p);
            DLC_LAUNCH_CHECK(ctx, "gemm_split_f16_kernel<SP_CONV>");
            return DLC_OK;
        });
        if (rc != DLC_OK) return rc;
        if (outs) outs[l] = out;
        h = out;
        if (g.pool && l < b) {
            const int ph = (g.oh - 3) / 2 + 1, pw = (g.ow - 3) / 2 + 1;
            float* y = (float*)(ws + W.pool[l]);
            hipLaunchKernelGGL(cs_maxpool_kernel, dim3(cs_blocks(n * ph * pw * g.cout)), dim3(256), 0, st, (const float*)out, (long long)n,
                               g.oh, g.ow, g.cout, ph, pw, y);
            h = y;
        }
        DLC_LAUNCH_CHECK(ctx, "cnnvtl split layer");
    }
    return DLC_OK;
}

int conv_check_common(dlc_ctx* ctx, const char* who, int64_t n, int n_layers, const int32_t* geom, const void* panels, const void* ws) {
    if (!geom || !panels || n < 1 || n_layers < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: null/empty argument", who);
    if (n_layers > CS_MAX_LAYERS) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: at most %d layers", who, CS_MAX_LAYERS);
    if (n > 65535) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: more than 65535 frames per call", who);
    if (((uintptr_t)ws & 255) || ((uintptr_t)panels & 255)) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: workspace and panels must be 256-byte aligned", who);
    return DLC_OK;
}

}  // namespace
}  // namespace dlc_gemm

extern "C" size_t dlc_cnnvtl_split_panels_bytes(int n_layers, const int32_t* geom) {
    if (!geom || n_layers < 1 || n_layers > dlc_gemm::CS_MAX_LAYERS) return 0;
    for (int l = 0; l < n_layers; ++l)
        if (!dlc_gemm::cs_geom_ok(dlc_gemm::cs_geom(geom, l))) return 0;
    return dlc_gemm::conv_panels_offset(n_layers, geom, n_layers);
}

extern "C" int dlc_cnnvtl_split_prepare(dlc_ctx* ctx, int n_layers, const int32_t* geom, const double* const* W, void* panels,
                                        size_t panels_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!geom || !W || !panels || n_layers < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cnnvtl_split_prepare: null/empty argument");
    const size_t need = dlc_cnnvtl_split_panels_bytes(n_layers, geom);
    if (need == 0) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "cnnvtl_split_prepare: bad geometry");
    if (panels_bytes < need) return dlc::fail(ctx, DLC_ERR_WORKSPACE, "cnnvtl_split_prepare: panels %zu < %zu bytes", panels_bytes, need);
    if ((uintptr_t)panels & 255) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cnnvtl_split_prepare: panels must be 256-byte aligned");
    for (int l = 0; l < n_layers; ++l)
        if (!W[l]) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cnnvtl_split_prepare: W[%d] is null", l);
    DLC_ON_DEVICE(ctx);
    for (int l = 0; l < n_layers; ++l) {
        const dlc_gemm::CsGeom g = dlc_gemm::cs_geom(geom, l);
        const int64_t dims[2] = {(int64_t)g.kh * g.kw * g.cin, g.cout};
        const int rc = dlc_gemm::split_prepare(ctx, 1, dims, W + l, (char*)panels + dlc_gemm::conv_panels_offset(n_layers, geom, l),
                                               (hipStream_t)stream);
        if (rc != DLC_OK) return rc;
    }
    return DLC_OK;
}

extern "C" size_t dlc_cnnvtl_encode_split_workspace_bytes(int64_t n, int h, int w, int c, int n_layers, const int32_t* geom) {
    if (n < 1 || n > 65535 || h < 1 || w < 1 || c < 1 || !geom || n_layers < 1 || n_layers > dlc_gemm::CS_MAX_LAYERS) return 0;
    dlc_gemm::ConvWs W;
    return dlc_gemm::conv_ws(n, h, w, c, n_layers, geom, &W) ? W.total : 0;
}

extern "C" int dlc_cnnvtl_encode_split(dlc_ctx* ctx, int dtype, const void* x, int64_t n, int h, int w, int c, int s2d, int n_layers,
                                       const int32_t* geom, const void* panels, const double* const* b, const int64_t* cols,
                                       int64_t n_cols, int8_t* out, float* const* feats, int32_t* status, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    int rc = dlc_gemm::conv_check_common(ctx, "cnnvtl_encode_split", n, n_layers, geom, panels, workspace);
    if (rc != DLC_OK) return rc;
    if (!x || !cols || !out || !status || n_cols < 1 || h < 1 || w < 1 || c < 1 || s2d < 1 || h % s2d || w % s2d)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cnnvtl_encode_split: bad argument");
    if (dtype != DLC_F64 && dtype != DLC_F32 && dtype != DLC_U8)
        return dlc::fail(ctx, DLC_ERR_UNSUPPORTED, "cnnvtl_encode_split: frames must be DLC_F64, DLC_F32 or DLC_U8");
    const int h0 = h / s2d, w0 = w / s2d, c0 = c * s2d * s2d;
    dlc_gemm::ConvWs W;
    if (!dlc_gemm::conv_ws(n, h0, w0, c0, n_layers, geom, &W)) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "cnnvtl_encode_split: bad geometry");
    if (!workspace || workspace_bytes < W.total)
        return dlc::fail(ctx, DLC_ERR_WORKSPACE, "cnnvtl_encode_split: workspace %zu < %zu bytes", workspace_bytes, W.total);
    DLC_ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* in0 = (float*)(ws + W.in0);
    const unsigned blocks = dlc_gemm::cs_blocks((long long)n * h * w * c);
    if (dtype == DLC_F64) hipLaunchKernelGGL(dlc_gemm::cs_input_kernel<double>, dim3(blocks), dim3(256), 0, st, (const double*)x, (long long)n, h, w, c, s2d, in0);
    else if (dtype == DLC_F32) hipLaunchKernelGGL(dlc_gemm::cs_input_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)x, (long long)n, h, w, c, s2d, in0);
    else hipLaunchKernelGGL(dlc_gemm::cs_input_kernel<unsigned char>, dim3(blocks), dim3(256), 0, st, (const unsigned char*)x, (long long)n, h, w, c, s2d, in0);
    DLC_LAUNCH_CHECK(ctx, "cs_input_kernel");
    unsigned long long* keys = (unsigned long long*)(ws + W.keys);
    hipLaunchKernelGGL(dlc_gemm::cs_keys_init_kernel, dim3((unsigned)dlc::cdiv(n, (int64_t)256)), dim3(256), 0, st, keys, (long long)n);
    const float* outs[dlc_gemm::CS_MAX_LAYERS];
    rc = dlc_gemm::conv_run_layers(ctx, n, W, n_layers, geom, 0, n_layers - 1, in0, (const char*)panels, b, feats, outs, ws, keys,
                                   (int*)status, st);
    if (rc != DLC_OK) return rc;
    dlc_gemm::FSegs s;
    s.n = n_layers;
    s.start[0] = 0;
    for (int l = 0; l < n_layers; ++l) {
        const dlc_gemm::CsGeom g = dlc_gemm::cs_geom(geom, l);
        s.ptr[l] = outs[l];
        s.size[l] = (long long)g.oh * g.ow * g.cout;
        s.start[l + 1] = s.start[l] + s.size[l];
    }
    hipLaunchKernelGGL(dlc_gemm::cs_quant_gather_kernel, dim3((unsigned)dlc::cdiv(n_cols, (int64_t)256), (unsigned)n), dim3(256), 0, st, s,
                       (const long long*)cols, (long long)n_cols, (const unsigned long long*)keys, out);
    DLC_LAUNCH_CHECK(ctx, "cs_quant_gather_kernel");
    return DLC_OK;
}

extern "C" int dlc_cnnvtl_layers_split(dlc_ctx* ctx, const float* x, int64_t n, int h, int w, int c, int n_layers, const int32_t* geom,
                                       int layer_a, int layer_b, const void* panels, const double* const* b, float* const* feats,
                                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    int rc = dlc_gemm::conv_check_common(ctx, "cnnvtl_layers_split", n, n_layers, geom, panels, workspace);
    if (rc != DLC_OK) return rc;
    if (!x || !feats || !status || layer_a < 0 || layer_b < layer_a || layer_b >= n_layers || h < 1 || w < 1 || c < 1)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cnnvtl_layers_split: bad argument");
    dlc_gemm::ConvWs W;
    if (!dlc_gemm::conv_ws(n, h, w, c, n_layers, geom, &W)) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "cnnvtl_layers_split: bad geometry");
    if (!workspace || workspace_bytes < W.total)
        return dlc::fail(ctx, DLC_ERR_WORKSPACE, "cnnvtl_layers_split: workspace %zu < %zu bytes", workspace_bytes, W.total);
    for (int l = layer_a; l <= layer_b; ++l)
        if (!feats[l - layer_a]) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "cnnvtl_layers_split: feats[%d] is null", l - layer_a);
    DLC_ON_DEVICE(ctx);
    return dlc_gemm::conv_run_layers(ctx, n, W, n_layers, geom, layer_a, layer_b, x, (const char*)panels, b, feats, nullptr,
                                     (char*)workspace, nullptr, (int*)status, (hipStream_t)stream);
}
