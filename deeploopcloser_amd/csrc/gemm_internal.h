// Shared between the dense-GEMM translation units (gemm_dense.hip, gemm_dma_f64.hip).
#pragma once
#include "dlc_internal.h"

namespace dlc_gemm {

// Implicit im2col (tf.layers.conv2d on NHWC, src/cnn_vtl/network/cnn_vtl.py:33-93): row m of the
// A operand is output pixel (img, oy, ox), column k is (ky, kx, c) with c fastest; A then points
// at the NHWC input and lda is unused.
struct ConvGeom {
    int H, W, C, KW, stride, pad_t, pad_l, OH, OW;
    // optional: [images, 2] ordered keys (dlc_f64_key) into which the minimum / maximum of every image's outputs is
    // folded (cnn_vtl.py:110-112 takes them over the whole descriptor of a frame; dlc_cnnvtl_frame_minmax_init)
    unsigned long long* mm_keys;
};

// Triangular skip of a launch (the Gram blocks of the SDAV similarity, match_ref.hip): rows / columns are
// patches of frames of `p` patches, row r is global patch row0 + r, column c global patch col0 + c; only
// (row frame < column frame) entries are ever read, so a tile that holds none is not computed.  p = 0: off.
struct TriSkip {
    int p;
    long long row0, col0;
};

constexpr int ACT_AXPY = 16;        // internal activation: C += alpha * (A . B), no bias (the SGD step of a weight gradient)

// One dense fp64 / fp32 GEMM call: C = act(A . B + bias), B stored [K,N] (DLC_B_KN) or [N,K] (DLC_B_NK).
struct GemmCall {
    int dtype, blayout, act;                    // DLC_F64 / DLC_F32, DLC_B_*, DLC_ACT_* or ACT_AXPY
    int64_t M, N, K;                            // K: the reduction length as A has it
    const void* A; int64_t lda;
    const void* B; int64_t ldb;
    const void* bias;
    void* C; int64_t ldc;
    hipStream_t st;
    // Kb (0 = K): B's reduction length when A is zero-padded past it (SDAV's 1681 input columns copied into rows of 1696):
    // the LDS-DMA kernel walks K and reads B's missing k-rows as zeros, the register-staged kernel walks Kb
    int64_t Kb = 0;
    double alpha = 0.0;                         // ACT_AXPY
    const ConvGeom* cv = nullptr;               // implicit im2col (A is the NHWC input, lda unused)
    const TriSkip* tri = nullptr;
    bool dma_first = false;                     // the LDS-DMA one-pass forms even where the register-staged kernel would split K
    int64_t kb() const { return Kb > 0 && Kb < K ? Kb : K; }
};

// One launch of the LDS-DMA kernel (gemm_dma_f64.hip): rows row0 .. row0 + M - 1 of the call.
struct DmaLaunch {
    int tm, tn;                                 // tile: 256 / 128 / 64 rows x 128 / 96 columns
    int br, bc;                                 // block of br x bc tiles
    int64_t row0, M;
    int64_t kchunk;                             // > 0: split-K in chunks of kchunk into the context's scratch
    int64_t nwg;                                // workgroups (0: no tile holds a wanted entry of the triangle, nothing to launch)
};

// How a call runs (plan_gemm, gemm_dense.hip, describes the routes): every launch parameter, fixed before any launch.
enum GemmRoute { ROUTE_DMA_SPLITK, ROUTE_DMA, ROUTE_DMA_TWO_PART, ROUTE_STAGED_SPLITK, ROUTE_STAGED };
struct GemmPlan {
    int route;
    int chunks;                                 // split-K: K chunks, summed by the reduce (1 = one pass)
    DmaLaunch dma[2];                           // ROUTE_DMA*: its launches (two for ROUTE_DMA_TWO_PART)
    int64_t kchunk, nwg;                        // ROUTE_STAGED*: K per chunk (>= K in one pass), workgroups, ...
    int br, bc;                                 // ... in blocks of br x bc tiles
};

// The call, planned and launched.  DLC_OK; 1 for an ACT_AXPY call the LDS-DMA kernel does not take (nothing is launched);
// < 0 = error.  The wrappers below fill the call in.
int gemm(dlc_ctx* ctx, const GemmCall& c);
// The LDS-DMA planning and launcher (gemm_dma_f64.hip): false when the kernel does not take the launch.
bool plan_dma_launch(const dlc_ctx* ctx, const GemmCall& c, int tm, int64_t row0, int64_t M, int64_t kchunk, DmaLaunch* l);
bool plan_dma_forms(const dlc_ctx* ctx, const GemmCall& c, GemmPlan* p);
int launch_dma(dlc_ctx* ctx, const GemmCall& c, const DmaLaunch& l);

// act(A . B + bias) with its arguments checked (dlc_gemm_bias_act)
int gemm_bias_act(dlc_ctx* ctx, int dtype, int blayout, int act, int64_t M, int64_t N, int64_t K, const void* A,
                  int64_t lda, const void* B, int64_t ldb, const void* bias, void* C, int64_t ldc, hipStream_t st);
// A zero-padded by the caller to lda = Kpad columns (columns K .. Kpad-1 are zeros), B [K,N]: act(A[:, :K] . B + bias),
// the LDS-DMA forms (which walk Kpad) ahead of the register-staged kernel (on the first K columns)
int gemm_bias_act_padded_f64(dlc_ctx* ctx, int act, int64_t M, int64_t N, int64_t K, int64_t Kpad, const double* A,
                             const double* B, int64_t ldb, const double* bias, double* C, int64_t ldc, hipStream_t st);
// C += alpha * (A . B) in the epilogue of the LDS-DMA kernel (the SGD step of a weight gradient: W -= lr * dW without dW
// ever reaching memory -- SDAV.py:223-226).  DLC_OK, or 1 when the kernel does not take the shape (nothing launched).
int gemm_axpy_dma_f64(dlc_ctx* ctx, int blayout, double alpha, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda,
                      const double* B, int64_t ldb, double* C, int64_t ldc, hipStream_t st);
// Gram block of the SDAV similarity (match_ref.hip): C = A . B^T in fp64 (B stored [N,K], or its transpose stored
// [K,N]), tiles that hold no (row frame < column frame) entry skipped (their part of C stays unwritten, never read).
int gram_upper_f64(dlc_ctx* ctx, int blayout, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda,
                   const double* B, int64_t ldb, double* C, int64_t ldc, int patches, int64_t row0, int64_t col0,
                   hipStream_t st);

// The SDAV similarity's arg-min filter (gram_i8.hip): descriptors as three signed fixed-point digits of their offset from
// the column's centre, their exact integer products, and the bound of what the rounding misses.
constexpr int DLC_SIM_KEYS = 8;        // words of a call's `keys` (gram_i8.hip: sim_filter_prepare)
size_t sim_filter_panel_bytes(int64_t rows, int64_t H);
size_t sim_range_words(int64_t H);
int sim_frames_per_unit(int64_t P);
int64_t sim_col_rows(int64_t N, int64_t P);
int64_t sim_col_frames(int64_t N, int64_t P);
int64_t sim_argmin_pitch(int64_t N, int64_t P);
bool sim_filter_fits(int64_t N, int64_t P, int64_t H);
int sim_filter_prepare(dlc_ctx* ctx, const double* desc, int64_t N, int64_t P, int64_t H, const double* score,
                       unsigned long long* keys, double* cc, unsigned long long* ws_range, char* X, int* nbp, double* nu2,
                       double* proj, unsigned long long* rowhash, void* prog, const unsigned long long* range, hipStream_t st);
size_t sim_pairwise_program_bytes(int64_t H);
int sim_row_sums(dlc_ctx* ctx, const double* desc, int64_t rows, int64_t H, const double* score, double* nrm2, double* proj,
                 unsigned long long* rowhash, void* prog, unsigned long long* prog_len, hipStream_t st);
// the streaming form: a resident append-only panel quantised over a fixed range (match_ref.hip: dlc_sdav_stream_*)
int sim_stream_init(dlc_ctx* ctx, unsigned long long* keys, double* cc, void* prog, int64_t H, double lo, double hi,
                    const double* centre, hipStream_t st);
int sim_stream_quantise(dlc_ctx* ctx, const double* desc, int64_t rows_total, int64_t H, const double* score,
                        unsigned long long* keys, const double* cc, char* X, double* nu2, double* proj,
                        unsigned long long* rowhash, int64_t g_first, int64_t g_count, int64_t P, int* nbp, hipStream_t st);
size_t sim_stream_panel_bytes(int64_t rows, int64_t H);
int64_t gram_strip_frames(int64_t f_first, int64_t f_last, int64_t P);
int gram_argmin_i8_strip(dlc_ctx* ctx, int64_t f_first, int64_t f_last, int64_t P, int64_t H, const char* X, int64_t zrow,
                         const int* nbp, const unsigned long long* keys, unsigned char* abi, unsigned* acand, int64_t rp,
                         int64_t* fj_base_out, hipStream_t st, bool launch = true);
int gram_argmin_i8(dlc_ctx* ctx, int64_t N, int64_t P, int64_t H, const char* X, const int* nbp,
                   const unsigned long long* keys, unsigned char* abi, unsigned* acand, void* blocks, hipStream_t st);
size_t gram_blocks_bytes(int64_t N, int64_t P);

// How far apart two d2 = |v_b|^2 - 2 v_a . v_b of the filter (units of 2^-15, gram_i8.hip's header) must be before their
// order is the order of the true distances: twice the bound of one d2's error, + 1e-8 for the fp64 roundings of v and of
// |v|^2, rounded up, + 2.  keys[3]: the ordered key of the largest row sum of |v|.
__device__ __forceinline__ long long dlc_sim_window(const unsigned long long* __restrict__ keys, int H) {
    const double sv = dlc_f64_unkey(keys[3]);
    const double ed = 0x1p-23 * sv + (double)H * (0x1p-24 + 0x1p-33 + 0x1p-46) + 1.004 * 0x1p-15 + 0x1p-16;
    return (long long)ceil((2.0 * ed + 1e-8) * 32768.0) + 2;
}

}  // namespace dlc_gemm

namespace dlc_cnn {
// Folds min / max of x[img, per_img] (fp64, contiguous) into keys[img, 2] (cnnvtl.hip).
int fold_minmax_f64(dlc_ctx* ctx, const double* x, int64_t n_img, int64_t per_img, unsigned long long* keys, hipStream_t st);
}
