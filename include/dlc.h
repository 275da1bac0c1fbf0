/*
 * dlc.h -- C ABI of the MI355X-native loop-closure descriptor-and-match engine.
 *
 * This is the drop-in boundary for ONE path of nschejtman/deepLoopCloser:
 *     encode (SDAV / DA / CnnVtl forward) -> all-vs-all similarity / distance
 *     -> top-k match.
 * The reference has no FFI of its own (it is pure Python on TensorFlow-1 and
 * NumPy); each entry point below names the reference interface (file:line,
 * relative to the reference repo) whose arithmetic it replaces.  The Python
 * classes in deeploopcloser_amd/ keep the reference's names and signatures and
 * bind these symbols through ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) owned by the caller unless the
 *     parameter is documented as host; nothing is allocated or freed here,
 *     callers pass a workspace whose size the *_workspace_bytes() functions
 *     give;
 *   - every call is asynchronous on the caller's hipStream_t (`stream`,
 *     passed as void*; NULL = the null stream) and never synchronises -- with ONE
 *     exception, stated at dlc_sdav_similarity_matrix (an 8-byte flag read, which
 *     DLC_SIM_NO_HOST_SYNC rules out) -- and dlc_profile_gemm_ms, which waits by design;
 *   - matrices are row-major with explicit leading dimensions in ELEMENTS;
 *   - return value: DLC_OK (0) or a negative dlc_status; dlc_last_error()
 *     returns a human-readable message for the last failure on that context.
 *   - a context is bound to one device; use one context per GPU / rank, and one host thread per context at a time
 *     (the profiling ring, the staging ring and the similarity call's flag word live in it).
 */
#ifndef DLC_H_
#define DLC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Raised when a prototype, a struct or the meaning of an existing argument value changes.  A new bit in a `flags`
 * argument (zero keeps the old behaviour) and a larger *_workspace_bytes() answer (callers ask, never compute) change
 * neither: DLC_SELECT_NO_HINTS, DLC_SELECT_SERIAL and the hint array of dlc_cosine_topk_workspace_bytes came in at 20. */
#define DLC_ABI_VERSION 20

typedef struct dlc_ctx dlc_ctx;

typedef enum dlc_status {
    DLC_OK = 0,
    DLC_ERR_BAD_ARG = -1,      /* null pointer, negative size, unknown enum     */
    DLC_ERR_BAD_SHAPE = -2,    /* shape the kernels cannot take (see each call) */
    DLC_ERR_UNSUPPORTED = -3,  /* dtype / mode not implemented                  */
    DLC_ERR_HIP = -4,          /* a HIP runtime call failed                     */
    DLC_ERR_WORKSPACE = -5     /* workspace too small                           */
} dlc_status;

typedef enum dlc_dtype {
    DLC_BF16 = 0,
    DLC_F16 = 1,
    DLC_F32 = 2,
    DLC_F64 = 3,
    DLC_I8 = 4,
    DLC_U8 = 5,                /* 8-bit pixels as cv2.imread returns them (dlc_cnnvtl_encode_split) */
    DLC_I64 = 6                /* int64 score / distance matrices (dlc_sequence_topk)               */
} dlc_dtype;

typedef enum dlc_act {
    DLC_ACT_NONE = 0,
    DLC_ACT_SIGMOID = 1,       /* tf.nn.sigmoid, TensorflowWrapper.py:77-78 */
    DLC_ACT_RELU = 2           /* tf.nn.relu,    cnn_vtl.py:37             */
} dlc_act;

typedef enum dlc_blayout {
    DLC_B_KN = 0,              /* B stored [K,N] (weights, HWIO conv kernels) */
    DLC_B_NK = 1               /* B stored [N,K] (C = A . B^T)                */
} dlc_blayout;

/* ---- context --------------------------------------------------------- */
int dlc_abi_version(void);
int dlc_create(int device, dlc_ctx** out);
int dlc_destroy(dlc_ctx* ctx);
const char* dlc_last_error(const dlc_ctx* ctx);      /* host string, never NULL */
const char* dlc_status_string(int status);

/* ---- encode: dense layers -------------------------------------------- */
/*
 * C[M,N] = act(A[M,K] . B + bias[N]).
 * Replaces TensorWrapper.matmul/.add/.sigmoid (src/utils/TensorflowWrapper.py:57-78)
 * as used by SDAV._define_model (src/sdav/network/SDAV.py:129-157), DA's
 * sigmoid(x @ W + b) (src/sdav/network/DenoisingAutoencoderVariant.py:119) and,
 * with DLC_ACT_RELU/NONE on an im2col matrix, tf.layers.conv2d
 * (src/cnn_vtl/network/cnn_vtl.py:33-93).
 * dtype: DLC_F64 (the reference's arithmetic; v_mfma_f64_16x16x4_f64) or
 * DLC_F32 (v_mfma_f32_16x16x4_f32).  bias may be NULL.  Any M,N,K >= 1.
 * Operands: A is M rows of pitch lda >= K; B is K rows of pitch ldb >= N (DLC_B_KN) or N rows of pitch
 * ldb >= K (DLC_B_NK); C is M rows of pitch ldc >= N; pitches in elements.  Any such pitch is accepted, and the
 * bases and pitches need only the alignment of an element.  What lies between a row's end and the next row (and
 * around the operands) is never read into a result -- it may hold NaNs -- and never written.  Even lda / ldb, even
 * K (and N for DLC_B_KN) and 16-byte-aligned bases of A and B only select a faster route (the LDS-DMA kernel) for
 * DLC_F64; in one pass every route sums k in the same order and returns the same bits
 * (tests/test_gpu_gemm_f64_operands.py).
 */
int dlc_gemm_bias_act(dlc_ctx* ctx, int dtype, int blayout, int act,
                      int64_t M, int64_t N, int64_t K,
                      const void* A, int64_t lda, const void* B, int64_t ldb,
                      const void* bias, void* C, int64_t ldc, void* stream);

/*
 * Elementwise C[M,N] = act(A[M,N] + bias[N]) in fp64 / fp32: TensorWrapper.add
 * and .sigmoid (src/utils/TensorflowWrapper.py:69-71,77-78) when they are not
 * fused behind a matmul.  bias may be NULL.  In place (C == A) is allowed.
 */
int dlc_bias_act(dlc_ctx* ctx, int dtype, int act, int64_t M, int64_t N,
                 const void* A, int64_t lda, const void* bias, void* C, int64_t ldc, void* stream);

/*
 * SDAV.transform (src/sdav/network/SDAV.py:293-302): the n_layers-deep chain
 * h_l = sigmoid(h_{l-1} . W_l + b_l) on x[rows = B*P, dims[0]], corruption
 * level 0 (mask == 1, TensorflowWrapper.py:148-156, skipped).  W / b are HOST
 * arrays of n_layers DEVICE pointers, W_l is [dims[l], dims[l+1]] row-major,
 * b_l is [dims[l+1]] (may be NULL); dims is a HOST array of n_layers+1 widths.
 * out is the FLAT [rows, dims[n_layers]] array the reference returns (:163).
 * Workspace: dlc_sdav_encode_workspace_bytes(rows, dims, n_layers, dtype).
 */
size_t dlc_sdav_encode_workspace_bytes(int64_t rows, const int64_t* dims, int n_layers, int dtype);
int dlc_sdav_encode(dlc_ctx* ctx, int dtype, int64_t rows, int n_layers, const int64_t* dims,
                    const void* x, const void* const* W, const void* const* b,
                    void* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * SDAV.transform in a TOLERANCE mode on the 16-bit matrix cores (opt-in; dlc_sdav_encode in DLC_F64 stays the parity mode):
 * the same chain h_l = sigmoid(h_{l-1} . W_l + b_l) (src/sdav/network/SDAV.py:126-163,293-302;
 * src/utils/TensorflowWrapper.py:57-78) with every operand carried as two fp16 pieces of a power-of-two multiple of its
 * value and a layer computed as three v_mfma_f32_16x16x32_f16 products into fp32 accumulators (csrc/gemm_split_f16.hip),
 * bias + sigmoid in fp32, the activations handed from layer to layer as fp16 pieces.  Accuracy (measured against the fp64
 * oracle, tests/test_gpu_parity.py): descriptor relative L2 <= 2.1e-5 with the reference's N(0,1) initialiser, 2e-7 with
 * 1/sqrt(fan_in) weights -- inside north_star's "descriptor L2 within 1e-4"; NOT bit parity.  x must lie in [-16, 16]
 * (the reference feeds pixel / 255): larger values overflow fp16 and come out as NaN.
 *   dlc_sdav_split_prepare   once per set of weights: W_l (DEVICE fp64 [dims[l], dims[l+1]] row-major; W a HOST array of
 *                            DEVICE pointers) -> `panels` (DEVICE, dlc_sdav_split_panels_bytes(), 256-byte aligned): per
 *                            layer the two fp16 pieces of W_l 2^s, transposed and zero-padded, and 2^s;
 *   dlc_sdav_encode_split    x [rows, dims[0]] fp64 -> out [rows, dims[n_layers]] fp64 (the FLAT array of SDAV.py:163);
 *                            b: HOST array of n_layers DEVICE pointers (fp64 [dims[l+1]], entries or b itself may be NULL).
 * Both are stream-ordered.  Workspace: dlc_sdav_encode_split_workspace_bytes (256-byte aligned).
 */
size_t dlc_sdav_split_panels_bytes(int n_layers, const int64_t* dims);
int dlc_sdav_split_prepare(dlc_ctx* ctx, int n_layers, const int64_t* dims, const double* const* W, void* panels,
                           size_t panels_bytes, void* stream);
size_t dlc_sdav_encode_split_workspace_bytes(int64_t rows, const int64_t* dims, int n_layers);
int dlc_sdav_encode_split(dlc_ctx* ctx, int64_t rows, int n_layers, const int64_t* dims, const double* x,
                          const void* panels, const double* const* b, double* out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- SDAV training step (the surface train.py drives: SDAV.fit / fit_dataset) ----------------- */
/*
 * One `sess.run(train_steps[layer])` (src/sdav/network/SDAV.py:223-226,257-263): forward of
 * layers 0..layer with masking noise (:126-159; masks[l] is the [P, dims[l]] 0/1 mask of
 * TensorflowWrapper.py:148-156, shared by the frames of the batch), tied-weight decoder of
 * `layer`, loss cd + sparse_penalty*cs + consecutive_penalty*cc (:171-186), gradients with
 * respect to every variable the loss reaches (W_0..W_layer, b_enc_0..b_enc_layer, b_dec of
 * `layer`) and plain gradient descent with `learning_rate`, in place.  fp64.
 * x is [batch*P, dims[0]] (batch >= 2 frames); W / b_enc / masks are HOST arrays of DEVICE
 * pointers (entries 0..layer used); loss_out (DEVICE, 4 doubles, may be NULL) receives
 * {loss, cd, cs, cc} evaluated BEFORE the update.
 */
size_t dlc_sdav_train_workspace_bytes(int64_t batch, int64_t patches, const int64_t* dims, int n_layers, int layer);
int dlc_sdav_train_step(dlc_ctx* ctx, int layer, int64_t batch, int64_t patches, int n_layers, const int64_t* dims,
                        const double* x, const double* const* masks, double* const* W, double* const* b_enc,
                        double* b_dec, double sparse_level, double sparse_penalty, double consecutive_penalty,
                        double learning_rate, double* loss_out, void* workspace, size_t workspace_bytes,
                        void* stream);

/*
 * tw.random_mask / TensorWrapper.corrupt's mask (src/utils/TensorflowWrapper.py:34-38,148-156): n_zeros zeros among n
 * ones in random order -- every placement equally likely, the count exact (the reference rounds P*K*level and shuffles).
 * The draw is a function of (seed, counter): a caller steps the counter once per mask.  mask: DEVICE fp64 [n].
 */
int dlc_random_mask_f64(dlc_ctx* ctx, double* mask, int64_t n, int64_t n_zeros, uint64_t seed, uint64_t counter,
                        void* stream);

/* ---- DA training step (the surface train-sdav.py drives: SDA.fit, one DA layer at a time) ------ */
/*
 * The DA's static salt-and-pepper corruption (src/sdav/network/DenoisingAutoencoderVariant.py:182-202): `zeros` gets
 * EXACTLY n_zeros zeros among n ones, every placement equally likely (the draw of dlc_random_mask_f64 for the same
 * (seed, counter); the reference's count is int(n * corruption_level), a truncation), and `ones` gets 1 where `zeros` is 0
 * and an independent fair bit is set (salt), 0 everywhere else -- so ones <= 1 - zeros.  The bits are a function of
 * (seed, counter), from a key stream apart from the zeros' keys.  zeros, ones: DEVICE fp64 [n], distinct; n <= 2^26.
 */
int dlc_salt_pepper_mask_f64(dlc_ctx* ctx, double* zeros, double* ones, int64_t n, int64_t n_zeros, uint64_t seed,
                             uint64_t counter, void* stream);
/*
 * x~ = zeros * x + ones (DenoisingAutoencoderVariant.py:201-202), elementwise over x [rows, cols] (pitch cols) and the
 * two masks of the same shape, into out [rows, ldo] (ldo >= cols; columns cols .. ldo - 1 written as zeros; nothing
 * outside out[0 .. rows*ldo - 1] is written).  Give dlc_da_train_step an even ldo: cols + (cols & 1).
 * out may be x itself where ldo == cols (in place); out == x at another pitch is DLC_ERR_BAD_ARG, and out must not
 * overlap x in any other way, nor the masks.
 */
int dlc_da_corrupt_f64(dlc_ctx* ctx, const double* x, const double* zeros, const double* ones, int64_t rows, int64_t cols,
                       double* out, int64_t ldo, void* stream);
/*
 * One `sess.run(self.train_step)` of a DA (DenoisingAutoencoderVariant.py:103-148,201-202,231): h = sigmoid(x~ W + b_enc),
 * y = sigmoid(h W^T + b_dec) (tied decoder), loss cd + sparse_penalty*cs + consecutive_penalty*cc with
 * cd = mean over rows of softmax_cross_entropy(labels = x, logits = y) (the clean batch as labels),
 * cs = mean over the batch*patches rows of ||h - sparse_level||_1 (h is 2-D here: the denominator is batch*patches, not
 * the batch*N of dlc_sdav_train_step's layer 0), cc = mean over frames of ||H_t - H_t+1||_F; plain gradient descent
 * with `learning_rate` on W, b_enc, b_dec, in place.  fp64.  The same kernels as dlc_sdav_train_step's layer 0, with x~
 * taken from the caller instead of drawn per step.
 * x [batch*patches, in_units] (pitch in_units), x_tilde [batch*patches, in_units + (in_units & 1)] (dlc_da_corrupt_f64's
 * output, pad columns zero), W [in_units, hidden_units], b_enc [hidden_units], b_dec [in_units]: DEVICE.  batch >= 2.
 * loss_out (DEVICE, 4 doubles, may be NULL) receives {loss, cd, cs, cc} evaluated BEFORE the update.  Stream-ordered,
 * no synchronisation.
 */
size_t dlc_da_train_workspace_bytes(int64_t batch, int64_t patches, int64_t in_units, int64_t hidden_units);
int dlc_da_train_step(dlc_ctx* ctx, int64_t batch, int64_t patches, int64_t in_units, int64_t hidden_units, const double* x,
                      const double* x_tilde, double* W, double* b_enc, double* b_dec, double sparse_level,
                      double sparse_penalty, double consecutive_penalty, double learning_rate, double* loss_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- encode: SDAV patch front-end after key-point detection -------------------------------- */
/*
 * cv2.imread(path, IMREAD_GRAYSCALE) of a colour frame (src/sdav/input/CvInputParser.py:32):
 * OpenCV's fixed-point BT.601, (R*4899 + G*9617 + B*1868 + 8192) >> 14, on interleaved uint8 RGB.
 */
int dlc_rgb_to_gray_u8(dlc_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, uint8_t* gray, void* stream);
/*
 * CvInputParser.parse after get_top_n_key_points (CvInputParser.py:19-28, 49-123): for each of
 * the P key-points of each frame a patch_size x patch_size window centred on it, shifted to
 * stay inside the image (:74-86), flattened row-major and divided by 255.0.  gray is uint8
 * [frames, H, W]; key_points int32 [frames, P, 2] holds (round(kp.pt[0]), round(kp.pt[1])) --
 * as in the reference the first coordinate walks image dimension 0 (:111-119).  out is
 * [frames, P, patch_size^2] in out_dtype (DLC_F64 or DLC_F32).  SURF itself (:36-46) is
 * non-free OpenCV-contrib code and is not part of this library: key-points are an input.
 */
int dlc_extract_patches(dlc_ctx* ctx, const uint8_t* gray, int64_t frames, int H, int W,
                        const int32_t* key_points, int P, int patch_size, int out_dtype, void* out,
                        void* stream);

/*
 * Key-point detector for the patch front-end.  NOT the reference's: it takes the n strongest SURF
 * key-points (CvInputParser.py:36-46), and SURF is non-free OpenCV-contrib code that is neither
 * available nor re-implemented.  This is a Harris corner detector in exact integer arithmetic
 * (so the result is a function of the pixels alone): Sobel 3x3 gradients, structure tensor over
 * the 5x5 window, response 16*det - trace^2 (k = 1/16) for pixels >= 3 from the border, 3x3
 * non-maximum suppression, the n largest responses per frame (ties: lower row-major index).
 * gray uint8 [frames, H, W]; points int32 [frames, n, 2] = (x = column, y = row) as
 * cv2.KeyPoint.pt, (-1, -1) past the frame's count; responses int64 [frames, n]; counts int32
 * [frames].  Feed `points` to dlc_extract_patches as they are: like the reference it then uses
 * pt[0] along image dimension 0 (CvInputParser.py:111-119).
 */
size_t dlc_harris_keypoints_workspace_bytes(int64_t frames, int H, int W);
int dlc_harris_keypoints_u8(dlc_ctx* ctx, const uint8_t* gray, int64_t frames, int H, int W, int n,
                            int32_t* points, int64_t* responses, int32_t* counts, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- encode: SeqSLAM's image descriptor (not in the reference; needs no weights) ------------ */
/*
 * SeqSLAM's descriptor of a frame (Milford & Wyeth, ICRA 2012, III-A): the grey frame down-sampled to a thumbnail and
 * patch-normalised; two descriptors are compared by their sum of absolute differences (dlc_sad_u8_rows), and the
 * difference rows feed dlc_contrast_rows / dlc_sequence_topk / dlc_peak_topk_rows, the rest of the method.
 * INPUT.  gray is uint8 [frames, H, W] (what dlc_rgb_to_gray_u8 writes).  The result is exact: a function of the pixels
 * alone, the same for every launch plan.
 * AREA RESIZE to T [h, w], integers only.  Source row i covers [i h, (i + 1) h) and thumbnail row y covers
 * [y H, (y + 1) H) of a common axis of h H units:
 *     wy(y, i) = max(0, min((i + 1) h, (y + 1) H) - max(i h, y H))         (these sum to H over i; wx(x, j) alike with w, W)
 *     T(y, x)  = floor((2 * sum_{i, j} wy(y, i) wx(x, j) gray[i][j] + H W) / (2 H W))
 * -- the area-weighted mean, rounded half up.  h == H and w == W is the identity.
 * PATCH NORMALISATION over the tiles [y0, min(y0 + patch, h)) x [x0, min(x0 + patch, w)), y0 and x0 multiples of patch
 * (tiles at the lower and right edge are clipped).  Per tile of c cells: s = sum T, t = sum T * T, Qv = c t - s s, all
 * exact integers.  If c < 2 or Qv == 0 every cell of the tile is 128.  Otherwise, per cell, in fp64 with division and
 * sqrt the IEEE correctly rounded ones and no fma contraction:
 *     u   = (double)(c T - s)
 *     v   = sqrt((double)(c - 1) / ((double)c * (double)Qv))             (one multiply, one divide, one sqrt)
 *     z   = rint(((double)strength * u) * v)                             (the first product is exact, the second rounded
 *                                                                         once; rint rounds to nearest even)
 *     out = clamp(128 + z, 0, 255)
 * -- that is 128 + strength * (T - mean) / sample std (MATLAB's std, as OpenSeqSLAM normalises) with every input an exact
 * integer: no summation order is involved.  (OpenSeqSLAM's own byte format, 127 + round(z), is not this one.)
 * OUTPUT.  out is uint8 [frames, ld_out], ld_out >= h * w: the thumbnail row-major in the first h * w bytes of a row.
 * Bytes h * w .. ld_out-1 KEEP THEIR VALUE.  out must not overlap gray.  A row pitch that is a multiple of 16 on a
 * 16-byte aligned base is what dlc_sad_u8_rows takes.
 * Limits: frames >= 1, 1 <= h <= H, 1 <= w <= W, h * w <= 65536, H * W < 2^23, 1 <= patch <= 64, 1 <= strength <= 127.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, frames < 1, patch or strength outside its range or ld_out < h * w;
 * DLC_ERR_BAD_SHAPE for h, w, H, W outside the limits.  Nothing is written then.
 * No workspace; one launch on `stream` (one workgroup per frame, the thumbnail in LDS); never synchronises.
 */
int dlc_seqslam_describe_u8(dlc_ctx* ctx, const uint8_t* gray, int64_t frames, int H, int W, int h, int w,
                            int patch, int strength, uint8_t* out, int64_t ld_out, void* stream);

/* ---- encode: a binary global descriptor, LDB over the thumbnail (not in the reference; needs no weights) ------------ */
/*
 * The global LDB code of a frame ("Local Difference Binary", Yang & Cheng, ISMAR 2012, taken over the whole down-sampled
 * frame as ABLE-M does, Arroyo et al., IROS 2015): a few hundred bits, each the comparison of two grid cells of a
 * thumbnail by their mean or by one of their two gradients.  Two codes are compared by their Hamming distance
 * (dlc_hamming_rows), and the rows feed dlc_contrast_rows / dlc_sequence_topk / dlc_peak_topk_rows as the SAD rows do.
 * Every bit is unchanged by a gain and an offset of the image (a T + b, a > 0, compares as T does).  Integers only: a
 * function of the pixels alone, the same for every launch plan.
 * THUMBNAIL.  gray is uint8 [frames, H, W].  T [h, w] is the AREA RESIZE of dlc_seqslam_describe_u8 above, the same
 * formula, with no patch normalisation.  h == H and w == W is the identity.
 * LEVELS.  levels[0 .. n_levels-1]: 1 to 4 grid sizes g, strictly ascending, each 2 <= g <= 8; 2 g must divide both h
 * and w.  Level g cuts T into g x g cells of (h / g) x (w / g) pixels, row-major index c = cy * g + cx.  The four
 * quadrants of a cell are (top | bottom) x (left | right), a half being exactly h / 2g rows or w / 2g columns.  Per cell,
 * with the sums Q00, Q01, Q10, Q11 of T over the four quadrants (first index: 0 top, 1 bottom; second: 0 left, 1 right):
 *     S  = Q00 + Q01 + Q10 + Q11
 *     DX = (Q01 + Q11) - (Q00 + Q10)            (right minus left)
 *     DY = (Q10 + Q11) - (Q00 + Q01)            (bottom minus top)
 * All cells of a level have the same area, so sums are compared, not means.  With h * w <= 65536 every value fits int32.
 * BITS, t counting from 0.  Levels go in the order given; within a level the pairs (a, b) of cells with a < b go a
 * ascending, then b ascending; each pair gives three bits in the order S_a > S_b, DX_a > DX_b, DY_a > DY_b.  The
 * comparisons are strict: a tie is 0.
 *     bits(levels) = 3 * sum over the levels of g^2 (g^2 - 1) / 2        ((2,3,4): 486; (2,4,8): 6426; (8): 6048;
 *                                                                         (5,6,7,8): 12366)
 * Bit t is bit t & 7, least significant first, of byte t >> 3 of the frame's row.
 *     row_bytes = 16 * ceil(bits / 128)                                  (what the row-bytes call below returns)
 * The bits from `bits` to 8 * row_bytes - 1 are written as 0.
 * WORKED EXAMPLE.  T is 4 x 4 (identity resize), levels (2):
 *     1 2 5 5          cell   S   DX   DY
 *     3 4 5 5           0    10    2    4
 *     9 7 0 8           1    20    0    0
 *     9 7 8 0           2    32   -4    0
 *                       3    16    0    0
 * 6 pairs, 18 bits: pair (0,1) 0 1 1, (0,2) 0 1 1, (0,3) 0 1 1, (1,2) 0 1 0, (1,3) 1 0 0, (2,3) 1 0 0.  The row is
 * B6 95 00 followed by 13 zero bytes.
 * OUTPUT.  out is uint8 [frames, ld_out], ld_out >= row_bytes.  Bytes row_bytes .. ld_out-1 of a row KEEP THEIR VALUE.
 * out must not overlap gray.  A row pitch that is a multiple of 16 on a 16-byte aligned base is what dlc_hamming_rows
 * takes.
 * Limits, those of dlc_seqslam_describe_u8: frames >= 1, 1 <= h <= H, 1 <= w <= W, h * w <= 65536, H * W < 2^23.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, frames < 1, a bad level list (n_levels outside 1..4, a g outside 2..8, not
 * strictly ascending) or ld_out < row_bytes; DLC_ERR_BAD_SHAPE for h, w, H, W outside the limits, or a 2 g that does not
 * divide h or w.  Nothing is written then.
 * No workspace; one launch on `stream` (one workgroup per frame, the thumbnail in LDS); never synchronises.
 * The row-bytes call is host arithmetic: 0 for a bad level list.
 */
int64_t dlc_ldb_row_bytes(const int* levels, int n_levels);
int dlc_ldb_describe_u8(dlc_ctx* ctx, const uint8_t* gray, int64_t frames, int H, int W, int h, int w,
                        const int* levels, int n_levels, uint8_t* out, int64_t ld_out, void* stream);

/* ---- encode: sign-random-projection hashes, a float descriptor -> a Hamming code (not in the reference) -------------- */
/*
 * The bridge from the deep descriptors (searched by cosine, 8 KB a key-frame at 4096 bf16 columns) to the binary path
 * (dlc_hamming_rows and everything behind its rows, 128 bytes a key-frame at 1024 bits): bit t of a row is the sign of its
 * product with hyperplane t.  For random hyperplanes P(a bit differs) = angle / pi (Charikar, STOC 2002; on ConvNet place
 * descriptors: Suenderhauf et al., IROS 2015).  The product is formed on INT8 operands, so every sum is an exact integer
 * whatever the order, the tiling or the split: a code is bit for bit a function of the row and the model.
 * QUANTISE (dlc_lsh_quantize_i8).  x is [rows, ldx] of DLC_F64, DLC_F32 or DLC_BF16 (ldx in elements) using its first D
 * columns; mean fp64 [D] or NULL; q int8 [rows, ldq].  All arithmetic is fp64, every operation rounded on its own.  The
 * conversion of x to double is exact.  For row r:  t_d = (double)x[r][d] - mean[d], or (double)x[r][d] when mean is NULL;
 * m = max_d |t_d|.  If m == 0, or any t_d is a NaN or an infinity, the row is written as D zeros.  Otherwise s = 127.0 / m
 * and q[r][d] = (int8) rint(t_d * s), ties to even, which lies in -127 .. 127 (t_d == 0 gives 0, and where 127.0 / m
 * overflows the rounded product is clamped to +-127).  Only q[r][0 .. D-1] is written: bytes D .. ldq-1 KEEP THEIR VALUE.
 * A row's bytes depend on that row and mean alone.  q must not overlap x or mean.  1 <= rows < 2^31, 1 <= D <=
 * DLC_LSH_MAX_D, ldx >= D, ldq >= D.  One launch (a workgroup per row), no workspace.
 * WORKED EXAMPLE.  x = (0.5, -1, 0.25, 0), no mean: m = 1, s = 127, products 63.5, -127, 31.75, 0 -> (64, -127, 32, 0);
 * 63.5 ties to the even 64.
 * HASH (dlc_lsh_hash_i8).  q is int8 [rows, ldq] and planes int8 [bits, ldp], both using their first D columns; ARBITRARY
 * int8 in both (-128 included), not only +-1: learned hyperplanes fit the same call.
 *     S(r, t) = sum over d < D of q[r][d] * planes[t][d]          exact in int32: 128 * 128 * DLC_LSH_MAX_D < 2^31
 * Bit t of row r is 1 iff S(r, t) > 0; a tie is 0.  Bit t is bit t & 7, least significant first, of byte t >> 3 of the row.
 *     row_bytes = 16 * ceil(bits / 128)                           (dlc_lsh_row_bytes; 0 for bits outside 1 .. MAX_BITS)
 * The bits from `bits` to 8 * row_bytes - 1 are written as 0; bytes row_bytes .. ld_out-1 of a row KEEP THEIR VALUE -- the
 * contract of dlc_ldb_describe_u8, so dlc_hamming_rows takes the rows as they are and out may be rows of a key-frame
 * store.  Both q and planes are 16-byte aligned with ldq and ldp multiples of 16 and >= D.  Bytes D .. ld-1 of either may
 * hold anything and change nothing (the K tail is masked; no byte past D of a row is read).  out must not overlap q or
 * planes.  1 <= rows < 2^31, 1 <= D <= DLC_LSH_MAX_D, 1 <= bits <= DLC_LSH_MAX_BITS, ld_out >= row_bytes.
 * WORKED EXAMPLE.  q = (3, -2, 0, 1) against planes (1, 1, 1, 1), (-1, 1, 1, -1), (1, 1, -1, -1), (1, -1, 1, 1): the sums
 * are 2, -6, 0, 6, the bits 1 0 0 1, the row 09 followed by 15 zero bytes.
 * PLANS.  DLC_LSH_PLAN_ONE_PASS: a workgroup owns a (row tile, bit tile) and walks all of D on the int8 matrix cores; no
 * workspace, one launch.  DLC_LSH_PLAN_SPLIT (rows <= DLC_LSH_SPLIT_MAX_ROWS): a workgroup takes one DLC_LSH_CHUNK-byte
 * piece of D for a tile and stores its int32 sums to the workspace [chunks][rows][8 * row_bytes] with plain stores (no
 * atomics, no memset); a finish kernel adds a bit's chunks, takes the sign and packs: two launches, and the planes of one
 * streamed frame are read by chunks x as many workgroups.  DLC_LSH_PLAN_AUTO: SPLIT iff rows <= DLC_LSH_SPLIT_MAX_ROWS and
 * D > DLC_LSH_CHUNK (there is a second chunk to give away), else ONE_PASS.  The result does not depend on the plan: that
 * is integer arithmetic, not a tolerance.
 * dlc_lsh_hash_workspace_bytes(rows, D, bits, plan) is host arithmetic: the bytes the plan (AUTO: the plan it chooses)
 * needs -- 0 under ONE_PASS, at least rows * chunks * bits * 4 under SPLIT -- and 0 for refused shapes.
 * Errors: DLC_ERR_BAD_ARG for a null pointer (x, q, planes, out), a misaligned one, rows / D / bits < 1, a pitch below D
 * (or, of the hash, not a multiple of 16), ld_out < row_bytes, an unknown dtype or plan, or an output overlapping an
 * input; DLC_ERR_BAD_SHAPE for D > DLC_LSH_MAX_D, bits > DLC_LSH_MAX_BITS, rows >= 2^31 or SPLIT with more than
 * DLC_LSH_SPLIT_MAX_ROWS rows; DLC_ERR_WORKSPACE for a workspace (SPLIT) that is missing, too small or not 16-byte aligned.
 * Nothing is written then.  All launches on `stream`, none synchronises; memory and the workspace are the caller's.
 */
#define DLC_LSH_MAX_BITS 8192
#define DLC_LSH_MAX_D 131071          /* 128 * 128 * D < 2^31: the int32 sum cannot overflow */
#define DLC_LSH_CHUNK 8192            /* bytes of D per split piece */
#define DLC_LSH_SPLIT_MAX_ROWS 64
enum { DLC_LSH_PLAN_AUTO = 0, DLC_LSH_PLAN_ONE_PASS = 1, DLC_LSH_PLAN_SPLIT = 2 };
int dlc_lsh_quantize_i8(dlc_ctx* ctx, int x_dtype /* DLC_F64 | DLC_F32 | DLC_BF16 */, const void* x, int64_t rows, int64_t D,
                        int64_t ldx, const double* mean /* [D], may be NULL */, int8_t* q, int64_t ldq, void* stream);
int64_t dlc_lsh_row_bytes(int bits);
size_t dlc_lsh_hash_workspace_bytes(int64_t rows, int64_t D, int bits, int plan);
int dlc_lsh_hash_i8(dlc_ctx* ctx, const int8_t* q, int64_t rows, int64_t D, int64_t ldq,
                    const int8_t* planes /* [bits, ldp] */, int bits, int64_t ldp,
                    uint8_t* out, int64_t ld_out, int plan, void* workspace, size_t workspace_bytes, void* stream);

/* ---- encode: CnnVtl pieces (src/cnn_vtl/network/cnn_vtl.py:28-133) ------ */
/*
 * im2col for tf.layers.conv2d on NHWC fp64 (cnn_vtl.py:33-93): x[n,h,w,c] ->
 * cols[n*oh*ow, kh*kw*c] with column order (kh,kw,c) == HWIO kernel reshaped
 * to [kh*kw*c, cout].  pad_top/pad_left are TF's SAME pads (0 for VALID).
 * src_dtype DLC_F64 or DLC_I8 is not needed: the reference feeds uint8 pixels
 * as fp64 (create_distance_matrix.py:23,27); x here is fp64.
 */
int dlc_im2col_nhwc_f64(dlc_ctx* ctx, const double* x, int64_t n, int h, int w, int c,
                        int kh, int kw, int stride, int pad_top, int pad_left, int oh, int ow,
                        double* cols, void* stream);
/*
 * tf.layers.conv2d (NHWC fp64, HWIO kernel reshaped [kh*kw*c, cout]) + bias + activation as an
 * IMPLICIT GEMM: the A-tile loader of the fp64 MFMA GEMM gathers input pixels directly, the
 * im2col matrix is never written.  With c %% 16 == 0 (conv2..conv5 of cnn_vtl.py:49-93, conv1 over its
 * space-to-depth input) and at least 16 output tiles of 256 x 128 the operands reach LDS by DMA -- 16 channels
 * of one kernel tap per K tile, padding served as zeros by out-of-range buffer offsets; smaller launches and
 * c %% 8 == 0 fetch 8 channels per 64-byte load into registers; other channel counts (c = 3) are gathered element
 * by element.  Every form sums in the same k order: out is [n, oh, ow, cout], bit-identical between them and to
 * dlc_im2col_nhwc_f64 + dlc_gemm_bias_act, whatever the batch a frame is part of.
 */
int dlc_conv2d_nhwc_f64(dlc_ctx* ctx, const double* x, int64_t n, int h, int w, int c,
                        const double* kernel, const double* bias, int kh, int kw, int cout,
                        int stride, int pad_top, int pad_left, int oh, int ow, int act,
                        double* out, void* stream);
/*
 * Space-to-depth with block s on NHWC fp64: y[n, h/s, w/s, (dy*s + dx)*c + ch] = x[n, y*s + dy, x*s + dx, ch]
 * (h, w multiples of s).  A stride-s VALID convolution with a k x k kernel over x is the stride-1 VALID convolution
 * with the ceil(k/s) x ceil(k/s) kernel W'[ky', kx', (dy*s + dx)*c + ch, :] = W[ky'*s + dy, kx'*s + dx, ch, :] (zero
 * where the index reaches k) over y: same products, and the channel count becomes s*s*c.  cnn_vtl's conv1
 * (11x11, stride 4, 3 channels; cnn_vtl.py:33-40) turns into a 3x3 convolution over 48 channels, which the implicit
 * GEMM gathers 8 / 16 channels at a time instead of element by element.
 */
int dlc_space_to_depth_nhwc_f64(dlc_ctx* ctx, const double* x, int64_t n, int h, int w, int c, int s,
                                double* y, void* stream);
/* tf.layers.max_pooling2d(3x3, stride 2, VALID) on NHWC fp64 (cnn_vtl.py:42-45,58-61). */
int dlc_maxpool3x3s2_nhwc_f64(dlc_ctx* ctx, const double* x, int64_t n, int h, int w, int c,
                              double* y, void* stream);
/*
 * cnn_vtl.py:106-128: the descriptor d[n, width] is the concatenation, per
 * frame, of the n_segs flattened conv outputs (segs[g] is [n, seg_sizes[g]]
 * fp64, contiguous; HOST arrays of DEVICE pointers / sizes, at most 8).  Per row:
 * min/max over all segments, (d-min)*(255/(max-min)), cast to int8 (truncate
 * toward zero, wrap modulo 256), and gather of the n_cols selected columns
 * (`cols`: DEVICE int64 indices into the concatenated row -- the boolean mask of
 * :118-128 as a sorted list).  minmax is a [n,2] fp64 DEVICE scratch the call
 * fills (min,max per row); out is [n, n_cols] int8.  n <= 65535 per call.
 * Outside what the reference defines:
 *   - a column index outside [0, width) writes byte 0;
 *   - min and max are taken over the row's non-NaN cells (fmin / fmax);
 *   - a cell whose scaled value is NaN or beyond +-9e18 writes byte 0: a constant row (255/0), a row holding an
 *     infinity and a row whose spread overflows the scale are all zeros, and so is a NaN cell.
 */
int dlc_minmax_quant_gather_i8(dlc_ctx* ctx, const double* const* segs, const int64_t* seg_sizes, int n_segs,
                               int64_t n, const int64_t* cols, int64_t n_cols, double* minmax,
                               int8_t* out, void* stream);
/*
 * The same with the per-frame minimum / maximum gathered WHILE the layers are computed instead of in a pass over
 * their outputs (4.9 GB at 1063 frames of 192x240):
 *   dlc_cnnvtl_frame_minmax_init   keys[n, 2] (DEVICE, 64-bit ordered keys) <- "no element seen yet";
 *   dlc_conv2d_nhwc_f64_stats      dlc_conv2d_nhwc_f64 that also folds min / max of out[f, :, :, :] into keys[f]
 *                                  (frame_keys may be NULL: plain convolution).  Large launches fold in the GEMM's
 *                                  epilogue (wave reduction + atomicMin / atomicMax on the keys), small ones in a pass
 *                                  over their own output;
 *   dlc_quant_gather_i8            decodes the keys into minmax[n, 2] (fp64 DEVICE scratch, as above) and quantises /
 *                                  gathers exactly as dlc_minmax_quant_gather_i8 does.
 * min / max are order-independent, so the descriptors are bit-identical to the one-call form.
 */
int dlc_cnnvtl_frame_minmax_init(dlc_ctx* ctx, uint64_t* keys, int64_t n, void* stream);
int dlc_conv2d_nhwc_f64_stats(dlc_ctx* ctx, const double* x, int64_t n, int h, int w, int c,
                              const double* kernel, const double* bias, int kh, int kw, int cout,
                              int stride, int pad_top, int pad_left, int oh, int ow, int act,
                              double* out, uint64_t* frame_keys, void* stream);
int dlc_quant_gather_i8(dlc_ctx* ctx, const double* const* segs, const int64_t* seg_sizes, int n_segs,
                        int64_t n, const int64_t* cols, int64_t n_cols, const uint64_t* keys, double* minmax,
                        int8_t* out, void* stream);

/*
 * CnnVtl.transform in the same TOLERANCE mode on the 16-bit matrix cores (opt-in; the fp64 calls above stay the parity mode
 * and the default): conv1..conv5 of src/cnn_vtl/network/cnn_vtl.py:33-93 with every operand carried as two fp16 pieces of a
 * power-of-two multiple of its value and each convolution computed as three v_mfma_f32_16x16x32_f16 products per 32-deep
 * k-slice into fp32 accumulators (csrc/gemm_split_f16.hip), bias and ReLU in fp32, fp32 activations between the layers,
 * max-pool on the fp32 values.  Weights carry one exponent per layer; activations ONE EXPONENT PER FRAME AND LAYER, from
 * that frame's own max |x| of the layer's input (pixels are fed as 0..255 -- create_distance_matrix.py:23,27 -- and ReLU
 * outputs are unbounded), so a frame's descriptor is bit-identical whatever batch it is encoded in.  The quantisation is
 * the reference's fp64 formula on the promoted fp32 features (cnn_vtl.py:108-128: per-frame min / max, (d - min) * (255 /
 * (max - min)), truncation, wrap modulo 256, column gather).
 * What a caller may rely on: every layer within the derived elementwise bound of
 * tests/conv_precision_bounds.py; end to end, measured on an MI355X against the fp64 oracle with seeded 1/sqrt(fan_in)
 * weights (tests/test_gpu_cnn_vtl_f16x2.py): features within 5e-7 of the frame's range, scaled values within 2.9e-4 of a
 * quantisation step (CPU emulation, scripts/emul_cnn_split.py: 2.0e-4), i.e. bytes that equal the fp64 mode's except where
 * the fp64 scaled value lies within the tests' window of 1.6e-3 steps of an integer, where they may differ by one step
 * (1 of 6 714 gathered bytes did; 0.0012 %% of all bytes over 1063 frames).  NOT byte parity, and no guarantee that a
 * nearest-neighbour list built on the bytes equals the fp64 mode's.  Zero-class hazard: about 47 %% of a frame's features are exact ReLU zeros sharing
 * ONE scaled value (0 - min) * 255 / (max - min); a frame for which that value lies within the mode's error of an integer can
 * have close to half of its bytes move by one step at once (a few frames in 10 000).
 * Accepted input: finite values (no [-16, 16] restriction: the per-frame exponent absorbs the range; fp64 frames are
 * rounded to fp32 first, uint8 pixels are exact).  A non-finite value in a layer's input sets bit 0 of *status, one in a
 * layer's output bit 1 (DEVICE int32 the caller zeroes; calls OR into it): the bytes of such a call are undefined.
 *   geom   HOST int32 [n_layers][11]: kh, kw, cin, cout, stride, pad_top, pad_left, oh, ow, act (DLC_ACT_NONE / _RELU),
 *          pool (1: tf.layers.max_pooling2d 3x3 / 2 VALID behind the layer); at most 8 layers;
 *   dlc_cnnvtl_split_prepare   once per set of weights: W[l] DEVICE fp64 [kh*kw*cin, cout] (the HWIO kernel; W a HOST array)
 *                              -> panels (DEVICE, dlc_cnnvtl_split_panels_bytes(), 256-byte aligned);
 *   dlc_cnnvtl_encode_split    frames x [n, h, w, c] (DEVICE; dtype DLC_F64, DLC_F32 or DLC_U8), n <= 65535, -> out int8
 *                              [n, n_cols] (cols as in dlc_minmax_quant_gather_i8, indices into the concatenated layer
 *                              outputs).  s2d > 1: layer 0's geometry describes the stride-1 convolution over the
 *                              space-to-depth(s2d) input [h / s2d, w / s2d, s2d * s2d * c] (dlc_space_to_depth_nhwc_f64) and
 *                              the frames are rearranged on the way in.  b: HOST array of DEVICE fp64 biases (entries or
 *                              b itself may be NULL).  feats (may be NULL, entries too): DEVICE fp32 [n, oh, ow, cout] per
 *                              layer that receives the layer's pre-quantisation output.
 *                              Workspace: dlc_cnnvtl_encode_split_workspace_bytes(n, h / s2d, w / s2d, s2d * s2d * c, ...);
 *   dlc_cnnvtl_layers_split    debug / test entry: layers layer_a .. layer_b on x = layer_a's fp32 input (the [h, w, c] given
 *                              are LAYER 0's input, the workspace is the encode call's); feats[l - layer_a] receives layer l.
 *                              Its *status reports layer INPUTS only (bit 0): the output flag (bit 1) rides on the per-frame
 *                              min / max fold, which only dlc_cnnvtl_encode_split runs -- a caller of this entry that needs
 *                              to know looks at the returned outputs.
 * All are stream-ordered.
 */
size_t dlc_cnnvtl_split_panels_bytes(int n_layers, const int32_t* geom);
int dlc_cnnvtl_split_prepare(dlc_ctx* ctx, int n_layers, const int32_t* geom, const double* const* W, void* panels,
                             size_t panels_bytes, void* stream);
size_t dlc_cnnvtl_encode_split_workspace_bytes(int64_t n, int h, int w, int c, int n_layers, const int32_t* geom);
int dlc_cnnvtl_encode_split(dlc_ctx* ctx, int dtype, const void* x, int64_t n, int h, int w, int c, int s2d, int n_layers,
                            const int32_t* geom, const void* panels, const double* const* b, const int64_t* cols,
                            int64_t n_cols, int8_t* out, float* const* feats, int32_t* status, void* workspace,
                            size_t workspace_bytes, void* stream);
int dlc_cnnvtl_layers_split(dlc_ctx* ctx, const float* x, int64_t n, int h, int w, int c, int n_layers, const int32_t* geom,
                            int layer_a, int layer_b, const void* panels, const double* const* b, float* const* feats,
                            int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- match: reference semantics --------------------------------------- */
/*
 * Distinctive score of a descriptor dataset viewed as [rows, H] fp64:
 * SimilarityCalculator._average_response + _distinctive_score
 * (src/sdav/similarity/SimilarityCalculator.py:20-27): column mean (rows
 * summed in order, as np.average does), then exp(-(avg-mu)^2 / (2 sigma^2)).
 * The reference recomputes this for every pair (:13-14); it is hoisted here.
 * range (DEVICE, dlc_sdav_range_words(H) = 3 + 2 H x uint64, may be NULL): the pass sees every element once and can leave
 * what the similarity's filter form needs to know about THIS dataset -- every column's minimum and maximum (ordered
 * keys) and a NaN / infinity flag; hand it to dlc_sdav_similarity_matrix called on the same descriptors and that call
 * skips its own pass over them.
 */
size_t dlc_sdav_range_words(int64_t H);
int dlc_sdav_distinctive_score(dlc_ctx* ctx, const double* dataset, int64_t rows, int64_t H,
                               double mu, double sigma, double* score, uint64_t* range, void* stream);
/*
 * All-vs-all SDAV similarity: SimilarityCalculator.similarity_score
 * (src/sdav/similarity/SimilarityCalculator.py:12-49) for every frame pair
 * i<j (score(h_i, h_j)), mirrored, diagonal = -1
 * (src/sdav/create_similarity_matrix.py:29-38).  desc is [N,P,H] fp64, P <= 64;
 * score [H] comes from dlc_sdav_distinctive_score.  out_f64 [N,N] receives the
 * float scores (+inf where a matched pair is identical); out_i64 (may be NULL)
 * the reference's int64 matrix (truncation toward zero, non-finite -> INT64_MIN).
 * What the reference takes from the patch-to-patch distances is the arg-min only (np.argmin of
 * np.linalg.norm, :30-37).  For P <= 32 and H <= 32768 it is decided by exact integer products of
 * 24-bit fixed-point values of the descriptors' offsets from their COLUMN's centre (a per-column offset
 * changes no distance; int8 MFMA on three signed digits, csrc/gram_i8.hip), whose error bound says
 * which candidates it cannot separate; those are evaluated directly in fp64, and where that is
 * still a tie to 1e-11, as np.linalg.norm forms them (NumPy's pairwise summation order).  Other
 * shapes, a dataset with a NaN or an infinity in it, a dataset on which a sample of 256 (patch, frame)
 * cells says the bound would leave more than an eighth of the arg-mins undecided (distances far below
 * the largest column range: the direct evaluations would cost more than the fp64 form), or
 * DLC_SIM_FORCE_F64 in `flags` take the fp64 Gram matrix (|a|^2 + |b|^2 - 2 a.b) -- the same matrix.
 * flags:
 *   DLC_SIM_FORCE_F64     the fp64 Gram form whatever the shape (same matrix; checker / experiments);
 *   DLC_SIM_NO_HOST_SYNC  the filter form reads ONE 8-byte flag back to the host (did the range pass
 *                         meet a NaN / infinity, did the sample say "undecidable"? -- it then has to
 *                         take the fp64 form): the only
 *                         blocking read of this library's stream-ordered calls (the host waits for that
 *                         copy alone, with the filter form's kernels already enqueued behind it: the call
 *                         returns when the quantisation pass is done).  With this flag the
 *                         call never synchronises (and can be captured in a hipGraph) and takes no
 *                         sample (undecided arg-mins are evaluated directly however many there are:
 *                         correct, possibly slow); on a dataset with a NaN / infinity the matrix then
 *                         comes back as NaN / INT64_MIN and stats[1] = 1, and the caller repeats the
 *                         call with DLC_SIM_FORCE_F64.
 * chunk_bytes: upper bound of one fp64 Gram block in the workspace (0 = 8 GiB; the filter form keeps no
 * product block at all: its product kernel emits the arg-mins); pass the same value to the
 * workspace-size function.
 * range (DEVICE, may be NULL): what dlc_sdav_distinctive_score left for the SAME desc (pointer, N*P rows, H):
 * the filter form then does not read the descriptors a second time to find their extremes.
 * stats (DEVICE, 2 int64, may be NULL): [0] arg-mins the integer bound could not decide (evaluated
 * directly in fp64), [1] why the filter form did not take the call: 0 it did, bit 0 the dataset held a
 * NaN / infinity, bit 1 the sample's verdict (both: the fp64 form ran, [0] = 0).  direct_pairs (DEVICE, [N,N]
 * bytes, may be NULL): 1 at [i, j], i < j, when at least one arg-min of that frame pair was evaluated
 * directly (the pairs a checker wants to look at first), 0 elsewhere.
 * The workspace holds the quantised descriptors and the product kernel's verdicts (filter form: 0.91 GB
 * at the reference's 1063 frames) or the descriptors' fp64 transpose and the fp64 Gram blocks (8.7 GB
 * there, below 9.5 GB + N*P*H*8 bytes for any N).
 */
#define DLC_SIM_FORCE_F64 1
#define DLC_SIM_NO_HOST_SYNC 2
size_t dlc_sdav_similarity_workspace_bytes(int64_t N, int64_t P, int64_t H, int flags, int64_t chunk_bytes);
int dlc_sdav_similarity_matrix(dlc_ctx* ctx, const double* desc, int64_t N, int64_t P, int64_t H,
                               const double* score, double a, double b,
                               double* out_f64, int64_t* out_i64, int flags, int64_t chunk_bytes,
                               const uint64_t* range, int64_t* stats, uint8_t* direct_pairs,
                               void* workspace, size_t workspace_bytes, void* stream);
/*
 * The same similarity for ONE NEW FRAME against a resident, growing set of older frames -- the shape the reference's
 * loop (src/sdav/create_similarity_matrix.py:34-38) takes when a robot adds a frame: row[j] = similarity_score(h_j, h_f)
 * (SimilarityCalculator.py:12-49) for every older frame j < f, equal to entry [j, f] of dlc_sdav_similarity_matrix bit for
 * bit (same arg-min rule, same terms, same summation order).  P <= 32, H <= 32768.
 * The caller keeps the descriptors desc[capacity, P, H] (fp64, frames in arrival order) and an opaque `state` of
 * dlc_sdav_stream_state_bytes() bytes (256-byte aligned) holding what the filter needs of every resident frame: the
 * 24-bit fixed-point panel, |v|^2, projections on `score`, content hashes.  The fixed-point range is FIXED at init, so
 * appending never re-quantises older frames: every value x of column k must satisfy lo <= x - col_centre[k] <= hi
 * (col_centre: DEVICE, H doubles, or NULL for zeros -- SDAV descriptors are sigmoid outputs: NULL, 0, 1; low-contrast
 * descriptors, whose columns each stay close to their own mean, want that mean here and a narrow [lo, hi]: the filter's
 * error window is a fixed fraction of (hi - lo)^2).
 *   dlc_sdav_stream_init    once (and again after growing: init + append of everything);
 *   dlc_sdav_stream_append  frames [n_old, n_total) of desc have arrived: quantise them (`score` = the distinctive
 *                           score the rows are projected on; it must stay the same for the life of the state);
 *   dlc_sdav_stream_query   row_out[0 .. f-1] for the resident frame f (normally the newest).  stats (DEVICE, 2 int64,
 *                           may be NULL): [0] arg-mins evaluated directly, [1] 1 when some appended value lay outside
 *                           that range or was not finite -- the error bound does not hold then and row_out is NaN.
 * All three are stream-ordered and never synchronise.  A query reads the panel once (245 MB at 1063 frames).
 */
size_t dlc_sdav_stream_state_bytes(int64_t capacity, int64_t P, int64_t H);
int dlc_sdav_stream_init(dlc_ctx* ctx, void* state, size_t state_bytes, int64_t capacity, int64_t P, int64_t H,
                         double lo, double hi, const double* col_centre, void* stream);
int dlc_sdav_stream_append(dlc_ctx* ctx, void* state, size_t state_bytes, int64_t capacity, int64_t P, int64_t H,
                           const double* desc, int64_t n_old, int64_t n_total, const double* score, void* stream);
int dlc_sdav_stream_query(dlc_ctx* ctx, void* state, size_t state_bytes, int64_t capacity, int64_t P, int64_t H,
                          const double* desc, int64_t f, const double* score, double a, double b, double* row_out,
                          int64_t* stats, void* stream);
/*
 * The same for n_queries consecutive resident frames f_first .. f_first + n_queries - 1 in one set of launches (a batch
 * of frames that arrived together: each still sees only the frames older than itself): row q of rows_out [n_queries,
 * ld_rows] receives entries 0 .. f_first + q - 1 (the rest of the row is left alone; ld_rows >= f_first + n_queries - 1),
 * each equal to what dlc_sdav_stream_query writes for that frame, bit for bit.  stats[0]: the direct evaluations of the whole
 * batch.  workspace: dlc_sdav_stream_query_batch_workspace_bytes, 256-byte aligned.
 * Fewer than 8 frames: two query frames per pass over the panel.  8 and more: the batch is a STRIP of the all-vs-all
 * call -- its frames are the columns, every older patch of the resident panel a row, of ONE launch of the int8 product
 * kernel dlc_sdav_similarity_matrix runs (the panel holds the patches in that kernel's operand order; |v|^2 is kept in its
 * column layout), whose undecided cells are then resolved as that call resolves them.  The workspace holds the queries'
 * nearest-patch verdicts and, for such batches, the strip's verdict arrays.
 */
size_t dlc_sdav_stream_query_batch_workspace_bytes(int64_t capacity, int64_t P, int64_t n_queries);
int dlc_sdav_stream_query_batch(dlc_ctx* ctx, void* state, size_t state_bytes, int64_t capacity, int64_t P, int64_t H,
                                const double* desc, int64_t f_first, int64_t n_queries, const double* score, double a,
                                double b, double* rows_out, int64_t ld_rows, int64_t* stats, void* workspace,
                                size_t workspace_bytes, void* stream);
/*
 * The strip form of dlc_sdav_stream_query_batch (n_queries >= 8) in its two halves, for callers that overlap batches on
 * two streams (create_similarity_matrix.py:34-38, one arriving batch behind the other):
 *   stage 1  the int8 product kernel of the strip (columns: the batch's frames; rows: every older patch of the panel) into
 *            the workspace's verdict arrays -- on the stream the NEXT batch's stage 1 will follow on;
 *   stage 2  resolution of the undecided cells + the scores into rows_out -- behind stage 1 of the SAME (f_first, n_queries,
 *            workspace), on any stream ordered behind it; the batch's dlc_topk_rows_f64 follows it there.
 * Stage 1 + stage 2 write exactly what the one call writes.  What may run BESIDE what: dlc_sdav_stream_append of the next
 * batch beside this batch's stage 1 (it rewrites the panel group the two batches share with the same bytes, and only adds
 * rows whose verdicts this strip never reads; the error bound it may raise only sends more cells to the direct evaluation:
 * the rows do not change, stats[0] can), and this batch's stage 2 beside the next batch's stage 1 given a workspace of its
 * own per batch in flight.  DLC_ERR_UNSUPPORTED for fewer than 8 frames (no strip: use the one call).
 */
int dlc_sdav_stream_query_batch_staged(dlc_ctx* ctx, void* state, size_t state_bytes, int64_t capacity, int64_t P, int64_t H,
                                       const double* desc, int64_t f_first, int64_t n_queries, const double* score, double a,
                                       double b, double* rows_out, int64_t ld_rows, int64_t* stats, void* workspace,
                                       size_t workspace_bytes, int stage, void* stream);
/*
 * The k best entries of every row of an fp64 score matrix scores [rows, ld] -- the loop-closure candidates of a batch of
 * streamed frames (rows of dlc_sdav_stream_query): row r offers its first min(ld, limit0 + r * limit_step) entries (none
 * when that is <= 0); order: score descending, ties -> the lower index (the older frame); a NaN is never taken.
 * out_scores / out_idx [rows, k]: (-inf, -1) where a row offers fewer than k.  1 <= k <= DLC_MAX_K.
 * poison (device, may be NULL): one int64 read on the device -- non-zero (stats[1] of a dlc_sdav_stream_* whose range was
 * violated: every row of it is NaN) turns every slot into (NaN, -1), so that a caller who only looks at the lists sees
 * "these scores mean nothing" rather than "no candidates".
 */
int dlc_topk_rows_f64(dlc_ctx* ctx, const double* scores, int64_t rows, int64_t ld, int64_t limit0, int64_t limit_step,
                      int k, double* out_scores, int64_t* out_idx, const int64_t* poison, void* stream);
/*
 * All-vs-all cnn_vtl distance: DistanceCalculator.calculate_distance
 * (src/cnn_vtl/similarity/DistanceCalculator.py:4-12) = sum_k popcount(|a_k ^ b_k|)
 * on signed int8, for the full N x N loop incl. the diagonal
 * (src/cnn_vtl/create_distance_matrix.py:30-36).  desc [N, D] int8 (row stride ldd).
 */
int dlc_cnnvtl_distance_matrix(dlc_ctx* ctx, const int8_t* desc, int64_t N, int64_t D, int64_t ldd,
                               int64_t* out, void* stream);
/*
 * k nearest db rows by the same distance, fused (no [Q, N] matrix is formed): for every query row r of queries [Q, D]
 * (row stride ldq), the k rows with the smallest distance among the first L_r = min(N, limit0 + r * limit_step) rows of
 * db [N, D] (row stride ldd); none when L_r <= 0.  limit_step = 0, limit0 = N: a plain k-nearest search; limit_step = 1:
 * a batch of streamed frames, row r sees one frame more than row r - 1 (the convention of dlc_topk_rows_f64).
 * Order: distance ascending, ties -> the lower db row (the older frame).  out_dist / out_idx [Q, k] (int64, row-major):
 * (-1, -1) in the slots past min(k, L_r).  Integers throughout: the result is exact and does not depend on the plan.
 * Rows: both bases 16-byte aligned, ldq and ldd multiples of 16 bytes (>= D); bytes D .. ld-1 of a row may hold
 * anything and change nothing.  queries may be rows of db itself (both are only read); the outputs and the workspace
 * must not overlap the operands or each other.  1 <= k <= DLC_MAX_K, D <= 2^28 (int32 sums), N < 2^32.
 * Workspace: dlc_cnnvtl_distance_topk_workspace_bytes(Q, N, D, k) bytes (0 = bad arguments: k outside 1..DLC_MAX_K
 * or an empty operand), 256-byte aligned.  Two launches on `stream`.
 */
size_t dlc_cnnvtl_distance_topk_workspace_bytes(int64_t Q, int64_t N, int64_t D, int k);
int dlc_cnnvtl_distance_topk(dlc_ctx* ctx, const int8_t* queries, int64_t Q, int64_t ldq,
                             const int8_t* db, int64_t N, int64_t ldd, int64_t D,
                             int64_t limit0, int64_t limit_step, int k,
                             int64_t* out_dist, int64_t* out_idx,
                             void* workspace, size_t workspace_bytes, void* stream);
/*
 * The same distance as rows: out[r * ld_out + j] = sum_k popcount(|q_r[k] ^ db_j[k]|) of query row r of queries [Q, D]
 * (row stride ldq) against row j of db [N, D] (row stride ldd), written for 0 <= j < lim(r) with
 * lim(r) = clamp(limit0 + r * limit_step, 0, N) -- the limit convention of dlc_cnnvtl_distance_topk, dlc_topk_rows_f64
 * and dlc_sequence_topk; any limit_step, negative included.  limit_step = 0, limit0 = N: the full [Q, N] block;
 * limit_step = 1: a batch of streamed frames, each seeing one frame more than the one before.
 * EVERY OTHER WORD OF out KEEPS ITS VALUE: the cells at or past lim(r) and the columns N .. ld_out-1 (what
 * dlc_sdav_stream_query_batch promises for its rows: a caller's context buffer, or its "not offered" fill, survives
 * the call).  When every lim(r) is 0 nothing is launched and the call returns DLC_OK.
 * out is int64 [Q, ld_out], ld_out >= N: the type dlc_sequence_topk(DLC_I64) and dlc_cnnvtl_distance_matrix use.
 * Rows as in dlc_cnnvtl_distance_topk: both bases 16-byte aligned, ldq and ldd multiples of 16 bytes (>= D); bytes
 * D .. ld-1 of a row may hold anything and change nothing; queries may be rows of db itself (both are only read); out
 * must not overlap the operands.  D <= 2^28 (int32 sums), N < 2^32, Q <= 2^20.
 * No workspace; one launch on `stream` (one workgroup per query tile x db tile below the largest lim(r), the tile
 * shapes of the top-k scan, plain 8-byte stores: no memset, no atomics); never synchronises.  Integers throughout: the
 * result is exact and does not depend on the plan, nor on how the queries are batched.
 */
int dlc_cnnvtl_distance_rows(dlc_ctx* ctx, const int8_t* queries, int64_t Q, int64_t ldq,
                             const int8_t* db, int64_t N, int64_t ldd, int64_t D,
                             int64_t limit0, int64_t limit_step,
                             int64_t* out, int64_t ld_out, void* stream);

/*
 * SeqSLAM's image difference as rows: out[r * ld_out + j] = sum_{p < D} |q_r[p] - db_j[p]| on UNSIGNED bytes (the sum
 * of absolute differences of two dlc_seqslam_describe_u8 descriptors; Milford & Wyeth, ICRA 2012, III-A), of query row r
 * of queries [Q, D] (row stride ldq) against row j of db [N, D] (row stride ldd).  The contract is
 * dlc_cnnvtl_distance_rows' word for word: written for 0 <= j < lim(r) = clamp(limit0 + r * limit_step, 0, N), any
 * limit_step, negative included (limit_step = 0, limit0 = N: the full [Q, N] block -- the difference matrix is this call
 * with queries = db); EVERY OTHER WORD OF out KEEPS ITS VALUE, the cells at or past lim(r) and the columns
 * N .. ld_out-1; when every lim(r) is 0 nothing is launched and the call returns DLC_OK.
 * out is int64 [Q, ld_out], ld_out >= N.  Both bases 16-byte aligned, ldq and ldd multiples of 16 bytes (>= D); bytes
 * D .. ld-1 of a row may hold anything and change nothing; queries may be rows of db itself (both are only read); out
 * must not overlap the operands.  D <= 2^24 (255 * D fits the 32-bit accumulator), N < 2^32, Q <= 2^20.
 * No workspace; one launch on `stream` (the tiles of dlc_cnnvtl_distance_rows, v_sad_u8 on the staged words, plain
 * 8-byte stores: no memset, no atomics); never synchronises.  Integers throughout: the result is exact and does not
 * depend on the plan, nor on how the queries are batched.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, Q, N or D < 1, ldq or ldd < D, ld_out < N or a misaligned base or pitch;
 * DLC_ERR_BAD_SHAPE for D > 2^24, N >= 2^32 or Q > 2^20 (checked as stated: Q = 2^20 is taken).  Nothing is written then.
 */
int dlc_sad_u8_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq,
                    const uint8_t* db, int64_t N, int64_t ldd, int64_t D,
                    int64_t limit0, int64_t limit_step,
                    int64_t* out, int64_t ld_out, void* stream);

/*
 * The same difference with tolerance to a lateral shift of the revisit: the best of the +-S thumbnail columns (the
 * remedy of the SeqSLAM family -- Milford's low-resolution work; SMART, Pepperell, Corke & Milford 2014 -- for a place
 * revisited half a lane to the side, which displaces the thumbnail by a few columns and spoils the cell-by-cell SAD).
 * DEFINITION.  A descriptor is a thumbnail of h rows and w columns, uint8, row-major, D = h * w.  For -S <= s <= S
 * (S = max_shift):
 *     sad_s(q, d) = sum over y < h, over x with 0 <= x < w and 0 <= x + s < w, of |q[y][x] - d[y][x + s]|
 *     v_s         = floor(sad_s * w / (w - |s|))          (int64; the overlap is w - |s| columns in every row)
 *     out         = min over s of v_s
 *     shift       = the s of the minimum; ties go to the first in the order 0, -1, +1, -2, +2, ..., -S, +S
 * A query column is compared with the key-frame column s to its right: when the query's content is the key-frame's
 * moved 8 columns to the left, shift = +8.  The rescaling by w / (w - |s|) keeps every shift on the scale of the plain
 * SAD, so thresholds keep their meaning.  S = 0 is dlc_sad_u8_rows bit for bit, with shift = 0 everywhere.  Only
 * horizontal whole-column shifts.
 * CONTRACT.  dlc_sad_u8_rows' word for word, with D = h * w: out[r * ld_out + j] is written for 0 <= j < lim(r) =
 * clamp(limit0 + r * limit_step, 0, N), any limit_step; EVERY OTHER WORD OF out KEEPS ITS VALUE; when every lim(r) is 0
 * nothing is launched and the call returns DLC_OK.  Both bases 16-byte aligned, ldq and ldd multiples of 16 bytes
 * (>= h * w); bytes h * w .. ld-1 of a row may hold anything and change nothing; queries may be rows of db; the outputs
 * must not overlap the operands or each other.  shift_out may be null; when given it is int8 [Q, ld_shift],
 * ld_shift >= N, written in exactly the cells in which out is written, and EVERY OTHER BYTE OF IT KEEPS ITS VALUE.
 * Ranges: 0 <= S <= DLC_MAX_SHIFT, S < w, w <= 65536, h * w <= 2^24 (so sad_s * w < 2^48), N < 2^32, Q <= 2^20.
 * No workspace; one launch on `stream` (the tiles of dlc_sad_u8_rows with fewer db rows per thread, all 2 S + 1 sums
 * of a pair accumulated in one pass over the staged bytes, plain stores: no memset, no atomics); never synchronises.
 * Every w >= 1 is served; w a multiple of 16 takes the fast path (16-byte loads, compile-time edge masks).  Integers
 * throughout, the rescaling an exact 64-bit division: the result is exact and does not depend on the plan, nor on how
 * the queries are batched.
 * Errors: DLC_ERR_BAD_ARG for what dlc_sad_u8_rows refuses (a null pointer, Q or N < 1, ldq or ldd < h * w, ld_out < N,
 * a misaligned base or pitch), h < 1, w < 1, max_shift < 0, or ld_shift < N with a non-null shift_out;
 * DLC_ERR_BAD_SHAPE for max_shift > DLC_MAX_SHIFT, max_shift >= w, w > 65536, h * w > 2^24, N >= 2^32 or Q > 2^20.
 * Nothing is written then.
 */
#define DLC_MAX_SHIFT 8
int dlc_sad_u8_shift_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq,
                          const uint8_t* db, int64_t N, int64_t ldd, int h, int w, int max_shift,
                          int64_t limit0, int64_t limit_step,
                          int64_t* out, int64_t ld_out, int8_t* shift_out, int64_t ld_shift, void* stream);

/*
 * Hamming distance of packed binary descriptors as rows: out[r * ld_out + j] = sum_{p < D} popcount(q_r[p] ^ db_j[p]) on
 * bytes (the number of differing bits of two dlc_ldb_describe_u8 codes, D = their row_bytes; any bit strings are taken),
 * of query row r of queries [Q, D] (row stride ldq) against row j of db [N, D] (row stride ldd).  (Not
 * dlc_cnnvtl_distance_rows, which is popcount(|a ^ b|) of SIGNED bytes.)  The contract is dlc_sad_u8_rows' word for word:
 * written for 0 <= j < lim(r) = clamp(limit0 + r * limit_step, 0, N), any limit_step, negative included (limit_step = 0,
 * limit0 = N: the full [Q, N] block -- the Hamming matrix is this call with queries = db); EVERY OTHER WORD OF out KEEPS
 * ITS VALUE, the cells at or past lim(r) and the columns N .. ld_out-1; when every lim(r) is 0 nothing is launched and the
 * call returns DLC_OK.
 * out is int64 [Q, ld_out], ld_out >= N.  Both bases 16-byte aligned, ldq and ldd multiples of 16 bytes (>= D); bytes
 * D .. ld-1 of a row may hold anything and change nothing; queries may be rows of db itself (both are only read); out
 * must not overlap the operands.  D <= 2^24 (8 * D fits the 32-bit accumulator), N < 2^32, Q <= 2^20.
 * No workspace; one launch on `stream` (the tiles of dlc_sad_u8_rows, xor and bit count on the staged words, plain 8-byte
 * stores: no memset, no atomics); never synchronises.  Integers throughout: the result is exact and does not depend on
 * the plan, nor on how the queries are batched.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, Q, N or D < 1, ldq or ldd < D, ld_out < N or a misaligned base or pitch;
 * DLC_ERR_BAD_SHAPE for D > 2^24, N >= 2^32 or Q > 2^20 (checked as stated: Q = 2^20 is taken).  Nothing is written then.
 */
int dlc_hamming_rows(dlc_ctx* ctx, const uint8_t* queries, int64_t Q, int64_t ldq,
                     const uint8_t* db, int64_t N, int64_t ldd, int64_t D,
                     int64_t limit0, int64_t limit_step,
                     int64_t* out, int64_t ld_out, void* stream);

/* ---- match: sequence-consistent search over a score matrix (not in the reference) ----------- */
/*
 * The trajectory search of SeqSLAM (Milford & Wyeth, ICRA 2012) over a dense score matrix -- rows of
 * dlc_sdav_stream_query_batch, dlc_sdav_similarity_matrix (fp64 or int64), dlc_cnnvtl_distance_matrix or
 * dlc_cnnvtl_distance_rows (a streamed batch's rows behind the L - 1 rows before it) -- with the selection fused:
 * "does the match of query frame r with key-frame j hold over the last L frames?".
 * INPUT.  M = scores [rows, ld], n <= ld columns in use, dtype DLC_F64, DLC_F32 or DLC_I64.  Row r offers its first
 * lim(r) = clamp(limit0 + r * limit_step, 0, n) entries (the convention of dlc_topk_rows_f64 and
 * dlc_cnnvtl_distance_topk).  offsets: a HOST table [n_slopes, L] of int32, off[v][0] = 0, non-decreasing in s,
 * 0 <= off <= 32767 (anything else: DLC_ERR_BAD_ARG); it is read during the call and may be freed on return.
 * SEQUENCE SCORE of cell (r, j) along slope v:
 *     Z_v(r, j) = M[r][j - off[v][0]] + M[r-1][j - off[v][1]] + ... + M[r-L+1][j - off[v][L-1]],
 * added left to right in that order, in fp64 for DLC_F64 / DLC_F32 (the conversion is exact) and in int64 (wrapping)
 * for DLC_I64: the sums are reproducible bit for bit, and exact on integers.  Z_v(r, j) is VALID when r - (L-1) >= 0,
 * j < lim(r) and every element read satisfies 0 <= j - off[v][s] < lim(r - s); a NaN sum (a NaN element, +inf + -inf)
 * is not valid.
 * CELL SCORE.  S(r, j) = the best valid Z_v -- the maximum, or the minimum when lower_is_better is set; the winning
 * slope is the lowest v that attains it; a cell with no valid slope is not offered.  fp64 values are compared as
 * dlc_topk_rows_f64 compares them (the order of the numbers, -0.0 below +0.0).
 * OUTPUT for rows row0 <= r < rows (rows below row0 are context only: how a streamed batch sees the L - 1 rows before
 * it): the k best offered cells of the row, best first, ties -> the lower j.  out_scores [rows - row0, k] fp64 (int64
 * for DLC_I64), out_idx int64, out_slope int32 (may be NULL); the slots past the offered count hold index -1, slope -1
 * and the score -inf (+inf if lower_is_better) / -1 for DLC_I64.  seq_out [rows - row0, ld_out] (may be NULL; same type
 * as out_scores; ld_out >= n) receives S itself in its first n columns, NaN / -1 where a cell is not offered.  At least
 * one of (out_scores + out_idx) and seq_out must be given; without the lists k, workspace and out_slope are not used.
 * poison (device, may be NULL; DLC_ERR_BAD_ARG with DLC_I64): the word of dlc_topk_rows_f64 -- non-zero turns every
 * fp64 slot into (NaN, -1, slope -1) and seq_out into NaN.
 * Limits: 1 <= L <= 64, 1 <= n_slopes <= 16, 1 <= k <= DLC_MAX_K, any rows, 0 <= row0 < rows, n < 2^31.
 * With L = 1 and one slope the lists equal dlc_topk_rows_f64 on the same rows bit for bit.
 * Two launches on `stream` (a scan over (row block x column slab) that keeps per-row running lists, then a merge; no
 * [rows, n] intermediate unless seq_out asks for it); never synchronises.  Workspace:
 * dlc_sequence_topk_workspace_bytes(rows, n, L, n_slopes, k) bytes (0 = bad arguments), 256-byte aligned.  The outputs
 * and the workspace must not overlap the matrix or each other.
 */
size_t dlc_sequence_topk_workspace_bytes(int64_t rows, int64_t n, int L, int n_slopes, int k);
int dlc_sequence_topk(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n, int64_t ld,
                      int64_t limit0, int64_t limit_step, int L, int n_slopes, const int32_t* offsets,
                      int lower_is_better, int k, void* out_scores, int64_t* out_idx, int32_t* out_slope,
                      void* seq_out, int64_t ld_out, const int64_t* poison, void* workspace, size_t workspace_bytes,
                      void* stream);

/*
 * The ELASTIC sequence search: dlc_sequence_topk's question with a chain in place of a straight line.  A revisit whose
 * speed changes inside the L frames -- a stop at a junction, a slow corner before a fast straight, key-frames inserted
 * at an uneven rate -- lies on none of the lines of an offset table; here every frame of the chain may step back by any
 * d_min <= d <= d_max key-frames from the frame after it (dynamic time warping with bounded steps, by dynamic
 * programming).  Arguments as dlc_sequence_topk (dtype, M = scores [rows, ld] with n columns in use, row0, lim(r) =
 * clamp(limit0 + r * limit_step, 0, n), lower_is_better, k, the outputs, poison, workspace, stream); d_min, d_max take the
 * place of the offset table and out_span that of out_slope.
 * DEFINITION -- the recursion itself.  For an output row r with r - (L-1) >= 0 let rho(t) = r - (L-1) + t, t = 0 .. L-1
 * (the chain's rows, oldest first):
 *     A_0(c) = M[rho(0)][c]                         valid iff 0 <= c < lim(rho(0)) and the element is not NaN
 *     A_t(c) = P_t(c) + M[rho(t)][c],  t = 1 .. L-1   one addition: fp64 for DLC_F64 / DLC_F32 (the conversion is exact),
 *                                                   wrapping int64 for DLC_I64
 *     P_t(c) = the best VALID A_{t-1}(c - d) over d = d_min .. d_max, the LOWEST d among equals
 *              A_t(c) is valid iff P_t(c) exists, 0 <= c < lim(rho(t)) and the sum is not NaN
 *     E(r, j)    = A_{L-1}(j)                       (so j < lim(r) is implied)
 *     span(r, j) = j - (the column the chosen chain started in at t = 0),   0 <= span <= (L-1) * d_max.
 * "Best" is dlc_sequence_topk's: the maximum, or the minimum when lower_is_better is set, in the order of the numbers with
 * -0.0 below +0.0.  A cell that is not valid is not offered; a row with r - (L-1) < 0 offers nothing.
 * OUTPUT for rows row0 <= r < rows (rows below row0 are context only): the k best offered cells of the row by E, best
 * first, ties -> the lower j.  out_scores [rows - row0, k] fp64 (int64 for DLC_I64), out_idx int64, out_span int32 (may be
 * NULL); the slots past the offered count hold index -1, span -1 and the score -inf (+inf if lower_is_better) / -1 for
 * DLC_I64.  seq_out [rows - row0, ld_out] (may be NULL; same type as out_scores; ld_out >= n) receives E in its first n
 * columns, NaN / -1 where a cell is not offered; columns n .. ld_out - 1 keep their bits.  At least one of (out_scores +
 * out_idx) and seq_out must be given; without the lists k, workspace and out_span are not used.  poison: as
 * dlc_sequence_topk (non-zero: every fp64 slot (NaN, -1, span -1), seq_out NaN; DLC_ERR_BAD_ARG with DLC_I64).
 * Nothing at or past a row's limit, and no column n .. ld - 1, is read.
 * CONSEQUENCES.  IEEE addition is monotone (x <= y implies x + m <= y + m when neither sum is NaN), so whenever no
 * partial sum is NaN -- always for finite data; for DLC_I64 while nothing wraps -- E(r, j) is the best PATH SUM over all
 * paths j = j_0 >= j_1 >= ... >= j_{L-1} with j_s - j_{s+1} in [d_min, d_max] and column j_s < lim(r - s) of row r - s,
 * added OLDEST row first: ((M[r-L+1][j_{L-1}] + M[r-L+2][j_{L-2}]) + ...) + M[r][j_0].  With opposite infinities inside a
 * window the recursion decides (a chain whose partial sum is NaN ends there; another may go on).  Every sum is formed in
 * one fixed order, integer rows stay exact, and a cell is a function of the L rows behind it alone: the result does not
 * depend on how rows are batched or on the launch plan.
 *   - With L = 1 the lists equal dlc_topk_rows_f64's on the same rows bit for bit (every span is 0).
 *   - With d_min = d_max = d on DLC_I64, scores and indices equal dlc_sequence_topk's with the one slope off[s] = s * d,
 *     and every span is (L-1) * d: integer sums do not depend on the order.
 *   - For fp64 the same holds whenever the sums are exact: this search adds the OLDEST row first, dlc_sequence_topk the
 *     newest first, and inexact sums may differ in the last place.
 * Limits: 1 <= L <= 64, 0 <= d_min <= d_max <= DLC_MAX_STEP, 1 <= k <= DLC_MAX_K, any rows, 0 <= row0 < rows, n < 2^31.
 * Errors: DLC_ERR_BAD_ARG (a limit above, a missing pointer, ld < n, ld_out < n), DLC_ERR_BAD_SHAPE (more rows than one
 * launch takes), DLC_ERR_WORKSPACE (NULL, not 16-byte aligned, or too small); nothing is written then.
 * Two launches on `stream` (a scan, one wave per output row and column slab that carries the L levels over a column tile
 * and its halo of (L-1) * d_max columns, then dlc_sequence_topk's merge); never synchronises.  Workspace:
 * dlc_sequence_elastic_topk_workspace_bytes(rows, n, L, d_min, d_max, k) bytes (0 = bad arguments).  The outputs and the
 * workspace must not overlap the matrix or each other.
 */
#define DLC_MAX_STEP 8
size_t dlc_sequence_elastic_topk_workspace_bytes(int64_t rows, int64_t n, int L, int d_min, int d_max, int k);
int dlc_sequence_elastic_topk(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n, int64_t ld,
                              int64_t limit0, int64_t limit_step, int L, int d_min, int d_max,
                              int lower_is_better, int k, void* out_scores, int64_t* out_idx, int32_t* out_span,
                              void* seq_out, int64_t ld_out, const int64_t* poison, void* workspace, size_t workspace_bytes,
                              void* stream);

/*
 * The CHAIN of a candidate: the alignment behind a score of dlc_sequence_elastic_topk or dlc_sequence_topk -- for each of
 * the L frames of the chain the key-frame it was matched to, and the matrix cells along it.  The searches keep one
 * scalar of it (the span, the slope); a pose graph wants the L frame-to-key-frame pairs, a gate the weakest frame's score.
 * Arguments as the searches' (dtype, M = scores [rows, ld] with n columns in use, row0, lim(r), L, the steps or the HOST
 * offset table, lower_is_better, poison, stream).  idx [rows - row0, k] (device int64) holds the candidates' end columns
 * j: the out_idx of either search or of dlc_peak_topk_rows over its seq_out, -1 for an empty slot.  The alignment is
 * formed again for those cells alone, by the recursion / the sums defined above, so the same call serves the fused lists
 * and picks from the dense scores (which carry neither slope nor span).
 * OUTPUT.  out_chain int32 [rows - row0, k, L]: the matched columns, OLDEST frame first -- chain[t] is the column in row
 * rho(t) = r - (L-1) + t, chain[L-1] = j.  out_cells [rows - row0, k, L] (may be NULL): cells[t] = M[rho(t)][chain[t]],
 * fp64 for DLC_F64 / DLC_F32 (the conversion is exact), int64 for DLC_I64.
 * ELASTIC (dlc_sequence_elastic_chains), for E(r, j) valid: chain[t-1] = chain[t] - d*, d* the step P_t(chain[t]) chose
 * (the best valid A_{t-1}(c - d), the lowest d among equals, in the order of merit above, -0.0 below +0.0).  Hence
 *   - chain[0] == j - span(r, j); every step chain[t] - chain[t-1] lies in [d_min, d_max]; every chain[t] < lim(rho(t));
 *   - ((cells[0] + cells[1]) + ...) + cells[L-1] equals E(r, j) bit for bit (wrapping for DLC_I64);
 *   - a chain depends on the L rows behind its cell alone: not on the batching, row0 or the launch plan;
 *   - with L = 1 the chain is [j].
 * LINES (dlc_sequence_chains), for S(r, j) offered: v* is dlc_sequence_topk's winning slope (the lowest v attaining the
 * best valid Z_v), chain[t] = j - off[v*][L-1-t], and out_slope [rows - row0, k] (may be NULL) receives v*.  Summed
 * newest first, as Z_v is defined -- cells[L-1] + cells[L-2] + ... + cells[0] -- the cells give S(r, j) bit for bit.
 * NOT A CHAIN: an idx of -1 (any value outside -1 .. n-1 is taken as -1 and never read from), idx >= lim(r), a cell that
 * is not valid (r - (L-1) < 0 included) or a non-zero poison word give chain = -1 in all L places, slope -1 and cells
 * NaN (-1 for DLC_I64).
 * Nothing at or past a row's limit, and no column n .. ld - 1, is read.
 * Limits: the searches' own -- 1 <= L <= 64, 0 <= d_min <= d_max <= DLC_MAX_STEP, 1 <= n_slopes <= 16 and the table as
 * dlc_sequence_topk takes it, 1 <= k <= DLC_MAX_K, 0 <= row0 < rows, n < 2^31; (rows - row0) * k < 2^31.
 * Errors: DLC_ERR_BAD_ARG (a limit above, a missing pointer, ld < n, poison with DLC_I64), DLC_ERR_BAD_SHAPE (more
 * candidates than one launch takes); nothing is written then.
 * Each entry point is ONE launch on `stream` (elastic: one wave per candidate runs the forward recursion over the
 * trapezoid of columns that can reach (r, j) -- at level t the columns j - (L-1-t) * d_max .. j - (L-1-t) * d_min, at most
 * 505 -- keeping the chosen step of every (level, column) in LDS, then walks back); no workspace; never synchronises.
 * The outputs must not overlap the matrix, idx or each other.
 */
int dlc_sequence_elastic_chains(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n, int64_t ld,
                                int64_t limit0, int64_t limit_step, int L, int d_min, int d_max,
                                int lower_is_better, int k, const int64_t* idx, int32_t* out_chain, void* out_cells,
                                const int64_t* poison, void* stream);
int dlc_sequence_chains(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t row0, int64_t n, int64_t ld,
                        int64_t limit0, int64_t limit_step, int L, int n_slopes, const int32_t* offsets,
                        int lower_is_better, int k, const int64_t* idx, int32_t* out_chain, void* out_cells,
                        int32_t* out_slope, const int64_t* poison, void* stream);

/*
 * SeqSLAM's local contrast normalisation of score rows (Milford & Wyeth, ICRA 2012, III-B): every cell against its
 * neighbourhood within its own row, (x - local mean) / local std, before dlc_sequence_topk sums along lines -- a stretch
 * of key-frames that resembles everything goes flat, a true revisit stands out from its neighbours.
 * INPUT.  M = scores [rows, ld], n <= ld columns in use, dtype DLC_F64, DLC_F32 or DLC_I64.  Row r offers its first
 * lim(r) = clamp(limit0 + r * limit_step, 0, n) entries (the convention of dlc_cnnvtl_distance_rows and
 * dlc_sequence_topk; any limit_step, negative included).  radius: 1..32 (SeqSLAM's R_window = 10 is radius 5).
 * For a cell (r, j) with j < lim(r): a = max(0, j - radius), b = min(lim(r), j + radius + 1), cnt = b - a and
 * x_c = (double) M[r][c] (exact from fp32; from int64 rounded to nearest even, exact below 2^53).  All arithmetic is
 * fp64, every operation rounded on its own (no fma contraction), division and sqrt the IEEE correctly rounded ones:
 *     s    = x_a;  s = s + x_{a+1};  ...  s = s + x_{b-1}          (left to right; starts FROM x_a, not from 0)
 *     mean = s / (double)cnt
 *     q    = (x_a - mean) * (x_a - mean);  q = q + (x_c - mean) * (x_c - mean) for c = a+1 .. b-1 (left to right)
 *     sd   = sqrt(q / (double)(cnt - 1))                           (the sample standard deviation, as MATLAB's std)
 *     out[r][j] = 0.0 if cnt < 2 or sd == 0.0, else (x_j - mean) / sd
 * Each cell's window is summed on its own (no running sum across cells), so a row's result depends on that row and its
 * limit alone: not on the tiling, the batching or the plan.  An infinity or a NaN in the window yields what IEEE
 * arithmetic gives, NaN (a cell dlc_sequence_topk does not offer).  sd > 0 keeps the order of merit within a
 * neighbourhood: lower_is_better passes through unchanged.
 * OUTPUT.  out is fp64 [rows, ld_out], ld_out >= n.  EVERY OTHER WORD OF out KEEPS ITS VALUE: the cells at or past
 * lim(r) and the columns n .. ld_out-1.  No element at or past lim(r) of its row is read.  out must not overlap scores.
 * When every lim(r) is 0 nothing is launched and the call returns DLC_OK.
 * scores rows need only their element's alignment (8 bytes, 4 for DLC_F32) and any ld; out 8 bytes.  No workspace; one
 * launch on `stream` (no memset, no atomics); never synchronises.  Any rows >= 1, 1 <= n < 2^31.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, an unknown dtype, rows < 1, n < 1, radius outside 1..32, ld < n or
 * ld_out < n; DLC_ERR_BAD_SHAPE for n >= 2^31.  Nothing is written then.
 */
int dlc_contrast_rows(dlc_ctx* ctx, int dtype, const void* scores, int64_t rows, int64_t n, int64_t ld,
                      int64_t limit0, int64_t limit_step, int radius,
                      double* out, int64_t ld_out, void* stream);

/*
 * Multi-descriptor fusion of score rows: m row sets that compare the same frames with the same key-frames -- cosine scores
 * (dlc_cosine_score_rows), cnn_vtl distances (dlc_cnnvtl_distance_rows), SADs (dlc_sad_u8_rows), SDAV similarities --
 * each normalised within its own row, weighted and summed into ONE fp64, higher-is-better row that everything behind
 * the rows takes (dlc_contrast_rows, dlc_sequence_topk, dlc_peak_topk_rows, dlc_pr_cell_counts).  The sum of per-query
 * standardised similarities of several descriptors (Schubert et al.; Hausler et al., Multi-Process Fusion): a
 * hand-crafted descriptor and a deep one fail in different places.
 * INPUT.  m sources S_0 .. S_{m-1}, 1 <= m <= DLC_MAX_FUSE, described by five HOST arrays of length m: S_i = scores[i] is
 * a device matrix [rows, lds[i]] of dtype dtypes[i] (DLC_F64, DLC_F32 or DLC_I64), all sources using their first n
 * columns; weights[i] is any finite double; lower_is_better[i] != 0 says that S_i is a distance.  Row r offers its first
 * lim(r) = clamp(limit0 + r * limit_step, 0, n) cells (the convention of dlc_contrast_rows; any limit_step, negative
 * included).  x_j = (double) S_i[r][j] (exact from fp32; from int64 rounded to nearest even, exact below 2^53).
 * ARITHMETIC.  All of it is fp64, every operation rounded on its own (no fma contraction), division and sqrt the IEEE
 * correctly rounded ones.
 * THE SUM OF A ROW, TREE(v_0 .. v_{c-1}).  P is the smallest power of two >= c and v_j = -0.0 for c <= j < P;
 *     T(lo, 1) = v_lo;   T(lo, len) = T(lo, len / 2) + T(lo + len / 2, len / 2);   TREE = T(0, P).
 * x + (-0.0) = x for every x, so padding to any larger power of two gives the same bits, and every aligned power-of-two
 * block of columns is a node of the tree whatever n, the tiling or the plan: the sum is parallel, and a row's result
 * depends on that row and its limit alone.  (A left-to-right sum gives other bits.)
 * PER SOURCE i AND ROW r with c = lim(r) >= 1, u:
 *   DLC_FUSE_NONE:    u_j = x_j, or -x_j if lower_is_better[i].
 *   DLC_FUSE_ZSCORE:  mean = TREE(x) / (double)c;  d_j = x_j - mean;  sd = sqrt(TREE(d_j * d_j) / (double)(c - 1)) (the
 *                     sample standard deviation, as dlc_contrast_rows uses);  u_j = 0.0 if c < 2 or sd == 0.0, else
 *                     d_j / sd, or (mean - x_j) / sd if lower_is_better[i].  A NaN or an infinity among the offered
 *                     cells gives what IEEE arithmetic gives: a NaN row, which no search offers.
 *   DLC_FUSE_MINMAX:  lo, hi = the least and the greatest offered cell in the order of the numbers, -0.0 below +0.0;
 *                     if any offered cell is NaN every u_j is NaN;  range = hi - lo;  u_j = 0.0 if range == 0.0, else
 *                     (x_j - lo) / range, or (hi - x_j) / range if lower_is_better[i].
 * OUTPUT.  t_i = weights[i] * u_j and out[r][j] = ((t_0 + t_1) + ...) + t_{m-1}, starting FROM t_0, not from 0.  The
 * fused row is always higher-is-better.  out is fp64 [rows, ld_out], ld_out >= n.  Only offered cells are written:
 * EVERY OTHER WORD OF out KEEPS ITS VALUE, the cells at or past lim(r) and the columns n .. ld_out-1.  No source cell at
 * or past its row's limit, and no column n .. ld-1, is read.  When every lim(r) is 0 nothing is launched and the call
 * returns DLC_OK.  out must not overlap a source; sources may alias each other.
 * CONSEQUENCES.  m = 1, DLC_FUSE_NONE, weight 1.0 is an exact conversion copy.  The result does not depend on the plan,
 * the batching of rows or any ld (NaN payloads aside).  With DLC_FUSE_ZSCORE, a source swapped for its negation together
 * with its lower_is_better flag leaves the bits unchanged.
 * PLANS.  DLC_FUSE_PLAN_ROW: one workgroup per row, one launch, no workspace (it is ignored): the row is swept for its
 * statistic(s) and once more to write, the re-reads served by L2.  DLC_FUSE_PLAN_SLAB, for few long rows (a streaming
 * batch against >= 10^5 key-frames): workgroups cover (row, slab of 4096 columns); at most three launches -- the slabs'
 * sums or min / max, the slabs' squared deviations, the write -- with the slab partials in the workspace, folded by
 * every workgroup of the next launch with the same tree; no atomics, no memset.  It needs
 * dlc_fuse_rows_workspace_bytes(rows, n, m) bytes, 16-byte aligned.  DLC_FUSE_PLAN_AUTO picks SLAB when the workspace
 * suffices, some row offers >= 8192 columns and rows < 2 x the device's compute units (docs/LAB.md 25: the measurement
 * behind the rule), else ROW.  A forced plan works at every shape.  Loads and stores are 16 bytes per lane where the
 * addresses allow; sources need only their element's alignment (8 bytes, 4 for DLC_F32), out 8 bytes.  Every launch is on
 * `stream`; the call never synchronises.  Any rows >= 1, 1 <= n < 2^31.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, m outside 1..DLC_MAX_FUSE, an unknown dtype, norm or plan, a non-finite
 * weight, rows < 1, n < 1, lds[i] < n, ld_out < n or a pointer not aligned to its element; DLC_ERR_BAD_SHAPE for
 * n >= 2^31; DLC_ERR_WORKSPACE for DLC_FUSE_PLAN_SLAB with a workspace that is missing, too small or not 16-byte
 * aligned.  Nothing is written then.  dlc_fuse_rows_workspace_bytes returns 0 for rows < 1, n < 1, n >= 2^31 or m
 * outside 1..DLC_MAX_FUSE.
 */
#define DLC_MAX_FUSE 8
enum { DLC_FUSE_NONE = 0, DLC_FUSE_ZSCORE = 1, DLC_FUSE_MINMAX = 2 };
enum { DLC_FUSE_PLAN_AUTO = 0, DLC_FUSE_PLAN_ROW = 1, DLC_FUSE_PLAN_SLAB = 2 };
size_t dlc_fuse_rows_workspace_bytes(int64_t rows, int64_t n, int m);
int dlc_fuse_rows(dlc_ctx* ctx, int m, const int* dtypes, const void* const* scores, const int64_t* lds,
                  const double* weights, const int* lower_is_better,
                  int64_t rows, int64_t n, int64_t limit0, int64_t limit_step, int norm, int plan,
                  double* out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Distinct-place candidates: the windowed peak top-k of score rows -- the last step of SeqSLAM's matcher (Milford &
 * Wyeth, ICRA 2012, III-D: the best trajectory, then the best one outside a window of key-frames around it).  A revisit
 * of key-frame j scores almost as well against j - 1, j + 1, ...: a plain top-k fills up with the neighbours of one peak.
 * Here a pick keeps every cell within `suppress` columns of it out of the later picks, so k picks are k places.
 * INPUT.  M = scores [rows, ld], n <= ld columns in use, dtype DLC_F64, DLC_F32 or DLC_I64 -- rows of
 * dlc_sdav_stream_query_batch, dlc_cnnvtl_distance_rows, dlc_cosine_score_rows, or dlc_sequence_topk's seq_out.
 * OFFERED CELLS.  Row r offers the cells j < lim(r) = clamp(limit0 + r * limit_step, 0, n) (the convention of
 * dlc_topk_rows_f64 and dlc_sequence_topk; any limit_step, negative included) that are present: for DLC_F64 / DLC_F32 a
 * NaN is never offered (+inf and -inf are ordinary values); for DLC_I64 a cell equal to `absent` is not offered when
 * has_absent != 0 (how the -1 of dlc_sequence_topk's int64 seq_out is passed).  has_absent != 0 with a float dtype is
 * DLC_ERR_BAD_ARG.
 * ORDER OF MERIT.  Exactly dlc_topk_rows_f64's and dlc_sequence_topk's: the order of the numbers, -0.0 below +0.0,
 * descending, or ascending with lower_is_better; ties -> the lower j.
 * PICKS.  p_1 is the best offered cell; p_i is the best offered cell with |j - p_m| > suppress for every m < i; the
 * picking stops after k picks or when no cell is left.  suppress >= 0, any value up to INT64_MAX; 1 <= k <= DLC_MAX_K;
 * n < 2^31; any rows >= 1; ld >= n; rows need only their element's alignment (8 bytes, 4 for DLC_F32).
 * OUTPUT.  out_scores [rows, k]: fp64 for DLC_F64 / DLC_F32 (the conversion is exact), int64 for DLC_I64; out_idx
 * [rows, k] int64; best first.  Empty slots hold (-inf, or +inf if lower_is_better, -1) in fp64 and (-1, -1) for DLC_I64.
 * poison (device, may be NULL; DLC_ERR_BAD_ARG with DLC_I64): the word of dlc_topk_rows_f64 -- non-zero turns every
 * slot into (NaN, -1).
 * READS.  No cell at or past lim(r), and no column n .. ld-1, is read or has any influence.
 * CONSEQUENCES.  With suppress = 0 the lists equal dlc_topk_rows_f64 on the same fp64 rows, bit for bit.  With k = 2,
 * lower_is_better and suppress = R_window / 2, slots 0 and 1 are OpenSeqSLAM's min_value and min_value_2nd (their
 * quotient is its uniqueness ratio).  A row's result depends on that row and its limit alone: not on the batching or
 * the plan.
 * Errors: DLC_ERR_BAD_ARG for a null pointer, an unknown dtype, rows < 1, n < 1, ld < n, suppress < 0, k outside
 * 1..DLC_MAX_K, has_absent with a float dtype, poison with DLC_I64 or a misaligned pointer; DLC_ERR_BAD_SHAPE for
 * n >= 2^31; DLC_ERR_WORKSPACE for a workspace that is missing, too small or not 16-byte aligned.  Nothing is written
 * then.  When every lim(r) is 0 the outputs are the empty fill and the call returns DLC_OK.
 * Workspace: dlc_peak_topk_rows_workspace_bytes(rows, n, k) bytes (0 = bad arguments): 16 bytes per 256 columns of
 * every row.  The outputs and the workspace must not overlap the matrix or each other.
 * At most two launches on `stream` (the best offered cell of every 256-column chunk into the workspace -- the one pass
 * over the rows -- then one workgroup per row: k rounds of "best chunk", each of which forms again only the chunks the
 * pick's window cuts); no atomics, no memset; never synchronises.
 */
size_t dlc_peak_topk_rows_workspace_bytes(int64_t rows, int64_t n, int k);
int dlc_peak_topk_rows(dlc_ctx* ctx, int dtype /* DLC_F64 | DLC_F32 | DLC_I64 */, const void* scores,
                       int64_t rows, int64_t n, int64_t ld, int64_t limit0, int64_t limit_step,
                       int lower_is_better, int64_t suppress, int has_absent, int64_t absent, int k,
                       void* out_scores, int64_t* out_idx, const int64_t* poison,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * PLACE TRACKING: a belief carried from frame to frame, with a state for "this frame closes no loop" -- the max-plus
 * (Viterbi) form of a filter over places.  The searches above ask whether a match holds over the last L frames; this
 * recursion runs over the whole traversal, gives an estimate per frame as the frames arrive and, by its back-pointers,
 * the best labelling of every frame so far: a key-frame or "nowhere".
 * Operand as the other score-row entry points take it: M = scores [rows, ld], n columns in use, DLC_F64, DLC_F32 or
 * DLC_I64, lim(r) = clamp(limit0 + r * limit_step, 0, n) for the call's row r.  Arithmetic is fp64 for float rows (the
 * conversion is exact) and wrapping int64 for DLC_I64.  "Best" is the order of merit of the searches: the order of the
 * numbers, -0.0 below +0.0, the minimum instead of the maximum with lower_is_better.  A penalty p WORSENS a value v:
 * v - p, or v + p with lower_is_better -- one operation, done once per row.
 * Parameters: 0 <= d_min <= d_max <= DLC_MAX_STEP; jump >= 0, gate >= 0, finite; null_score, NaN = there is no no-loop
 * state.  For DLC_I64 all three are integers of magnitude <= 2^53 and are used as int64.
 * STATE after row r: V_r(c) for 0 <= c < n, each absent or a number; U_r, the no-loop state, absent or a number; G_r, the
 * best present V_r(c), and g_r, the lowest c attaining it (-1 if none).  Before the first row ever seen everything is
 * absent, and an ORIGIN O = 0 is available to that first row only.
 * DEFINITION.  CELL RULE: for c < lim(r) with x = M[r][c] not NaN the predecessor P is the best present candidate of
 *     1. move, d = d_min .. d_max, lowest d first:  V_{r-1}(c - d)
 *     2. jump:                                      G_{r-1} worsened by jump
 *     3. from no-loop:                              U_{r-1} worsened by gate
 *     4. origin, first row only:                    0
 * the EARLIER in this list among equals.  V_r(c) = P + x, present iff P exists and the sum is not NaN; every other cell of
 * the row is absent.  back_r(c) records the choice: d for a move, DLC_TRACK_JUMP (the predecessor is column g_{r-1}),
 * DLC_TRACK_FROM_NULL, DLC_TRACK_ORIGIN; DLC_TRACK_ABSENT for an absent cell.
 * NO-LOOP STATE, when there is one: U_r = Q + null_score, Q the best present candidate of
 *     1. stay:    U_{r-1}                           (code 0)
 *     2. leave:   G_{r-1} worsened by gate          (DLC_TRACK_JUMP)
 *     3. origin, first row only: 0                  (DLC_TRACK_ORIGIN)
 * the earlier among equals; present iff Q exists and the sum is not NaN, else absent with the code DLC_TRACK_ABSENT.
 * The FILTERED PLACE of row r is g_r if G_r is present and strictly better than U_r, or if U_r is absent; otherwise -1.
 * CONSEQUENCE.  While nothing is NaN and nothing wraps, V_r(c) and U_r are the best sums over ALL labellings of rows
 * 0 .. r (a column below its row's limit, or nowhere, per row) that end in that state, of the cells of the places and
 * null_score per nowhere, worsened per transition by 0 for a step within [d_min, d_max], by jump to any other place
 * and by gate between a place and nowhere (IEEE addition is monotone; verified by enumeration of every labelling,
 * tests/test_track_cpu.py).  Each cell is one maximum over exact values and one addition in a fixed place, so the result
 * is exact on integer rows, reproducible on fp64 rows, and does not depend on how the rows are batched or on the plan.
 * STATE IN MEMORY, owned by the caller and transparent: V [n], fp64 (int64 for DLC_I64), absent = NaN (INT64_MIN: an int64
 * sum that wraps to exactly INT64_MIN reads as absent); head, four 8-byte device words: the rows seen, U, G, g.  head with
 * rows seen = 0 (an all-zero head) is the fresh state, and V is not read then.  V holds V of the row before the call's
 * first on entry and of its last row on return.  n may grow between calls: the new entries of V hold the absent mark.
 * OUTPUT per row of the call: out_place int64; out_g int64 (may be NULL: g_r, what dlc_track_backtrace follows through a
 * jump); out_G, out_U (typed and marked as V); out_backU int8.  Optional: out_back int8 [rows, ld_back] (ld_back >= n),
 * back_r(c) in its first n columns -- cells not offered or absent hold DLC_TRACK_ABSENT -- columns n .. keep their bits;
 * dense [rows, ld_dense] (typed as V, ld_dense >= n) receives V_r, absent cells the mark, columns n .. keep their bits.
 * Nothing at or past a row's limit, and no column n .. ld - 1, is read.  Never synchronises.
 * PLANS, identical bits: DLC_TRACK_RESIDENT -- ONE launch, one workgroup of up to 1024 threads that keeps V_{r-1} and V_r
 * in LDS and runs every row of the call, for n <= DLC_TRACK_RESIDENT_MAX (DLC_ERR_UNSUPPORTED above it); DLC_TRACK_ROWS --
 * one launch per row over column tiles and one more at the end, any n, V alternating in the workspace, no atomics;
 * DLC_TRACK_AUTO -- RESIDENT for n <= 3072, where it is the faster, ROWS above (docs/LAB.md 27).
 * Workspace: dlc_track_rows_workspace_bytes(rows, n, plan) bytes (0 = bad arguments), 16-byte aligned; the RESIDENT
 * plan reads none of it (workspace may be NULL then).
 * Errors: DLC_ERR_BAD_ARG (a parameter outside the ranges above, a missing or misaligned pointer, ld < n, ld_back < n,
 * ld_dense < n), DLC_ERR_BAD_SHAPE (n >= 2^31), DLC_ERR_UNSUPPORTED, DLC_ERR_WORKSPACE; nothing is written then.
 *
 * dlc_track_backtrace: the labelling behind a state.  out_back [rows, ld_back], out_backU [rows] and g [rows] are
 * dlc_track_rows' outputs for rows 0 .. rows - 1 of a traversal (several calls' outputs one after the other).  end: the
 * state of the last row to start from -- a column, -1 for nowhere, or DLC_TRACK_END_FILTERED: the device word
 * *place_last, the last row's out_place (place_last may be NULL otherwise).  out_path [rows] int64 receives every row's
 * state on the way back to row 0, a column or -1; from a row whose state is absent on, DLC_TRACK_NO_PATH.  Started from
 * the better of G and U of the last row, the path is a best labelling of the whole traversal.  ONE launch of one wave;
 * never synchronises.
 */
#define DLC_TRACK_AUTO 0
#define DLC_TRACK_RESIDENT 1
#define DLC_TRACK_ROWS 2
#define DLC_TRACK_RESIDENT_MAX 8192       /* two LDS buffers of n 8-byte words: 128 KiB of the 160 KiB a workgroup may declare */
#define DLC_TRACK_JUMP (-1)
#define DLC_TRACK_FROM_NULL (-2)
#define DLC_TRACK_ORIGIN (-3)
#define DLC_TRACK_ABSENT (-128)
#define DLC_TRACK_END_FILTERED (-2)
#define DLC_TRACK_NO_PATH (-2)
size_t dlc_track_rows_workspace_bytes(int64_t rows, int64_t n, int plan);
int dlc_track_rows(dlc_ctx* ctx, int dtype /* DLC_F64 | DLC_F32 | DLC_I64 */, const void* scores, int64_t rows, int64_t n,
                   int64_t ld, int64_t limit0, int64_t limit_step, int d_min, int d_max, int lower_is_better, double jump,
                   double gate, double null_score, int plan, void* V, int64_t* head, int64_t* out_place, int64_t* out_g,
                   void* out_G, void* out_U, int8_t* out_backU, int8_t* out_back, int64_t ld_back, void* dense,
                   int64_t ld_dense, void* workspace, size_t workspace_bytes, void* stream);
int dlc_track_backtrace(dlc_ctx* ctx, int64_t rows, int64_t n, const int8_t* out_back, int64_t ld_back,
                        const int8_t* out_backU, const int64_t* g, const int64_t* place_last, int64_t end,
                        int64_t* out_path, void* stream);

/*
 * Ground-truth evaluation of score rows: the last stage of the pipeline.  Given the rows a detector ranks by and a mask
 * of the cells that are true matches, dlc_pr_cell_counts counts the decisions behind a precision-recall curve and
 * dlc_positive_rank_rows the ranks behind recall@K.  Everything is integer counting: every result is exact and does not
 * depend on the grid, the batching or the plan.
 * INPUT (both calls).  M = scores [rows, ld], n <= ld columns in use, dtype DLC_F64, DLC_F32 or DLC_I64, exactly as
 * dlc_peak_topk_rows takes them.  truth [rows, ld_truth] bytes, ld_truth >= n, any alignment: a non-zero byte marks the
 * cell (r, j) as a true match, a POSITIVE; every other cell is a NEGATIVE.
 * OFFERED CELLS.  Row r offers the cells j < lim(r) = clamp(limit0 + r * limit_step, 0, n) (any limit_step, negative
 * included) that are present: for DLC_F64 / DLC_F32 a NaN is never offered (+inf and -inf are ordinary values); for
 * DLC_I64 a cell equal to `absent` is not offered when has_absent != 0.  has_absent != 0 with a float dtype is
 * DLC_ERR_BAD_ARG.
 * ORDER.  The order of the numbers, -0.0 below +0.0: for the float dtypes the unsigned order of the ordered key of the
 * fp64 value (an fp32 cell converts exactly), for DLC_I64 the order of the integers.  The ORDER OF MERIT is that order
 * descending, or ascending with lower_is_better; ties -> the lower j.
 * READS.  No cell at or past lim(r) and no column n .. ld-1 (n .. ld_truth-1), of the scores or of the truth, is read or
 * has any influence.  Rows of scores need only their element's alignment (8 bytes, 4 for DLC_F32).  Any rows >= 1,
 * 1 <= n < 2^31.  The outputs and the workspace must not overlap the inputs or each other.  Neither call synchronises.
 *
 * dlc_pr_cell_counts -- the cell-level protocol: every offered cell is a decision.
 * thresholds: n_thresholds = T values t_0 .. t_{T-1} on the DEVICE, 1 <= T <= 4096, fp64 for the float dtypes and int64
 * for DLC_I64, ASCENDING in the order of the numbers (for either sense of lower_is_better).  The BIN of an offered cell x is
 *     b(x) = #{i : t_i <= x}           (with lower_is_better: b(x) = #{i : t_i < x}),
 * comparisons in the order above, so that a detector run at threshold t_i reports exactly the cells
 *     x >= t_i  <=>  b(x) > i          (with lower_is_better: x <= t_i  <=>  b(x) <= i).
 * OUTPUT.  out_pos [T + 1], out_neg [T + 1] int64: the number of offered positive / negative cells in each bin.  Both are
 * fully written (the caller need not clear them); when every lim(r) is 0 they are all zero and the call returns DLC_OK.
 * The true positives at t_i are the sum of out_pos over the bins above i (with lower_is_better: up to i), the false
 * positives the same sum of out_neg.  A bin index lies in 0 .. T whatever the table holds: one that is not ascending, or
 * holds a NaN, gives unspecified counts (each offered cell still counted once) and no stray access.
 * Workspace: dlc_pr_cell_counts_workspace_bytes(rows, n, T) bytes (0 = bad arguments): 16 (T + 1) bytes per workgroup of
 * the count pass, at most 32 MiB.  Two launches on `stream`: the one pass over the matrix -- a workgroup keeps the
 * threshold keys and a u32 histogram in LDS (8 T + 8 (T + 1) bytes) and moves it into its own u64 partials before any
 * bin can reach 2^32 -- and the sum of the partials; no atomics on global memory, no memset.
 *
 * dlc_positive_rank_rows -- the retrieval protocol: where does a row's best true match stand in its ranking?  Per row:
 *     out_idx[r]  = p, the best offered positive cell in the order of merit (ties -> the lower column),
 *     out_rank[r] = the number of offered cells that BEAT p: better by merit, or equal and at a lower column,
 *     out_npos[r] = the number of offered positive cells;
 * a row without an offered positive gets (-1, -1, 0) (rank, idx, npos).  All three are int64 [rows].
 * CONSEQUENCE.  out_rank[r] is the slot at which dlc_topk_rows_f64 and dlc_peak_topk_rows(suppress = 0) list column
 * out_idx[r]: recall@K is the share of rows with 0 <= rank < K among those with npos > 0.
 * Workspace: dlc_positive_rank_rows_workspace_bytes(rows, n) bytes (0 = bad arguments): 32 bytes per row and slab.  One
 * launch when a workgroup takes a whole row (always from 2048 rows on: the second pass over the row comes out of the
 * cache), else three (per slab the best positive, per slab the cells that beat the row's best, per row the sums); no
 * atomics, no memset.
 *
 * Errors (both): DLC_ERR_BAD_ARG for a null pointer, an unknown dtype, rows < 1, n < 1, ld < n, ld_truth < n, has_absent
 * with a float dtype, n_thresholds outside 1..4096 or a misaligned pointer; DLC_ERR_BAD_SHAPE for n >= 2^31;
 * DLC_ERR_WORKSPACE for a workspace that is missing, too small or not 16-byte aligned.  Nothing is written then.
 */
size_t dlc_pr_cell_counts_workspace_bytes(int64_t rows, int64_t n, int n_thresholds);
int dlc_pr_cell_counts(dlc_ctx* ctx, int dtype /* DLC_F64 | DLC_F32 | DLC_I64 */, const void* scores,
                       int64_t rows, int64_t n, int64_t ld, int64_t limit0, int64_t limit_step,
                       int lower_is_better, int has_absent, int64_t absent,
                       const uint8_t* truth, int64_t ld_truth, const void* thresholds, int n_thresholds,
                       int64_t* out_pos, int64_t* out_neg,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t dlc_positive_rank_rows_workspace_bytes(int64_t rows, int64_t n);
int dlc_positive_rank_rows(dlc_ctx* ctx, int dtype /* DLC_F64 | DLC_F32 | DLC_I64 */, const void* scores,
                           int64_t rows, int64_t n, int64_t ld, int64_t limit0, int64_t limit_step,
                           int lower_is_better, int has_absent, int64_t absent,
                           const uint8_t* truth, int64_t ld_truth,
                           int64_t* out_rank, int64_t* out_idx, int64_t* out_npos,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * Orderless place descriptors: a k-means codebook of patch descriptors and VLAD pooling (Jegou et al., CVPR 2010; the
 * pooling of NetVLAD).  A frame's P patch descriptors come in key-point response order, which a viewpoint change
 * permutes; their concatenation then compares unrelated patches.  VLAD describes the frame by the per-word sums of
 * residuals x - c_k instead: a fixed-length row [K * H] that does not depend on the order of the patches and goes into
 * dlc_l2_normalize_rows and the cosine top-k as it is.
 * INPUT.  x is fp64 [rows, ldx] and the codebook fp64 [K, ldc], both using their first H columns; no other column of
 * either is ever read.  1 <= K <= DLC_VLAD_MAX_WORDS, 1 <= H, K * H < 2^31, 1 <= P <= DLC_VLAD_MAX_PATCHES, 1 <= rows,
 * frames < 2^31, ld >= H, ld_out >= K * H.
 * ARITHMETIC.  All of it is fp64, every operation rounded on its own (no fma contraction), division and sqrt the IEEE
 * correctly rounded ones.  TREE is the parallel sum defined at dlc_fuse_rows (pad with -0.0 to a power of two, add
 * halves recursively).
 * DIST(x, c):  d = +0.0;  for h = 0 .. H-1 ascending:  t = x_h - c_h;  q = t * t;  d = d + q.  One serial chain in h: any
 * tiling of (row, word) pairs gives the same bits, and the sum is never split along H or formed from a Gram product.
 * ASSIGNMENT.  a(x) = the lowest k whose DIST(x, c_k) is not NaN and is <= every other non-NaN distance (+inf can win);
 * -1 if every distance is NaN.  A copy of a centroid at a higher index is never taken.  dlc_vlad_assign writes
 * out_assign[n] = a(x_n) and, if out_dist is given, out_dist[n] = DIST(x_n, c_a(n)) (a quiet NaN for a(n) = -1).
 * VLAD of frame f (rows f * P .. f * P + P - 1).  R_k[h] = the sum of x_ph - c_kh over the patches p with a(p) = k, in
 * ascending p, starting FROM the first member's term, not from 0; +0.0 for a word without a member; patches with
 * a = -1 belong to no word.  DLC_VLAD_NORM_NONE: out[f][k * H + h] = R_k[h].  DLC_VLAD_NORM_INTRA: n_k =
 * sqrt(TREE_h(R_k[h] * R_k[h])); the word's H outputs are +0.0 if n_k == 0.0, else R_k[h] / n_k (NaN and inf give what
 * IEEE gives).  The global L2 normalisation is dlc_l2_normalize_rows' when the row is stored.  Only out[f][0 .. K*H-1]
 * is written; columns K * H .. ld_out-1 keep their bits.  A frame's row depends on its P rows and the codebook alone:
 * not on the batch, ldx, ldc or ld_out.  out_assign (optional) receives a() of all frames * P rows.  out must not overlap
 * x or the codebook.  dlc_vlad_encode always needs dlc_vlad_encode_workspace_bytes(frames, P, H, K) bytes.
 * ONE LLOYD STEP (dlc_kmeans_step) over rows x[0 .. rows-1] with codebook c_in.  a(n) as above, written to out_assign.
 * Rows are cut into blocks of DLC_KMEANS_BLOCK consecutive rows.  S_{b,k}[h] = the sum of x_nh over the members of k in
 * block b in ascending n, starting from the first member's value; -0.0 for a block without a member of k.
 * S_k[h] = TREE_b(S_{b,k}[h]).  out_counts[k] = the number of members.  c_out_k[h] = S_k[h] / (double)count_k if
 * count_k > 0, else c_in_k[h]: an empty word keeps its centre.  *out_inertia = TREE over the blocks of the block's sum
 * s = +0.0; s = s + DIST(x_n, c_in_a(n)) over its rows with a(n) >= 0 in ascending n.  *out_changed = the number of rows
 * with a(n) != prev_assign[n]; rows if prev_assign is NULL.  The step is a function of the rows in their order and of
 * c_in: no plan, no grid, no atomics.  c_out must not overlap c_in, out_assign must not overlap prev_assign.
 * LAUNCHES.  All on `stream`, none synchronises; memory and workspaces (16-byte aligned) are the caller's.  assign: 1;
 * encode: assign, residual sums, (INTRA) the norm; k-means step: assign, block sums, block statistics, finish.
 * Errors: DLC_ERR_BAD_ARG for a null or misaligned pointer, rows / frames / H / K / P < 1, ld < H, ld_out < K * H, an
 * unknown norm or an overlap named above; DLC_ERR_BAD_SHAPE for K > DLC_VLAD_MAX_WORDS, P > DLC_VLAD_MAX_PATCHES,
 * K * H >= 2^31, rows or frames >= 2^31; DLC_ERR_WORKSPACE for a workspace that is missing, too small or not 16-byte
 * aligned.  Nothing is written then.  The *_workspace_bytes functions return 0 for refused shapes.
 */
#define DLC_VLAD_MAX_WORDS 256
#define DLC_VLAD_MAX_PATCHES 1024
#define DLC_KMEANS_BLOCK 1024
enum { DLC_VLAD_NORM_NONE = 0, DLC_VLAD_NORM_INTRA = 1 };
int dlc_vlad_assign(dlc_ctx* ctx, const double* x, int64_t rows, int64_t H, int64_t ldx,
                    const double* centroids, int K, int64_t ldc,
                    int32_t* out_assign, double* out_dist /* may be NULL */, void* stream);
size_t dlc_vlad_encode_workspace_bytes(int64_t frames, int P, int64_t H, int K);
int dlc_vlad_encode(dlc_ctx* ctx, const double* x, int64_t frames, int P, int64_t H, int64_t ldx,
                    const double* centroids, int K, int64_t ldc, int norm,
                    double* out, int64_t ld_out, int32_t* out_assign /* [frames * P], may be NULL */,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t dlc_kmeans_step_workspace_bytes(int64_t rows, int64_t H, int K);
int dlc_kmeans_step(dlc_ctx* ctx, const double* x, int64_t rows, int64_t H, int64_t ldx,
                    const double* c_in, int K, int64_t ldc, double* c_out, int64_t ldc_out,
                    const int32_t* prev_assign /* may be NULL */, int32_t* out_assign,
                    int64_t* out_counts /* [K] */, double* out_inertia /* device, 1 */,
                    int64_t* out_changed /* device, 1 */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Compact place descriptors: the PCA projection (and whitening) of a pooled row -- out = ((x - mean) . basis) * scale
 * (Jegou & Chum, ECCV 2012).  A VLAD row of the reference's SDAV is 40 000 wide and the concatenation 75 000; the
 * projection takes either to the <= 4096 columns the cosine top-k stores.  The sum order is STATED, and chosen so that
 * it can be cut along D: a frame projected alone while streaming has the bits it had in the batch that built the
 * database.
 * INPUT.  x is fp64 [rows, ldx] using its first D columns; mean fp64 [D] or NULL; basis [D, ldb] in DLC_F64 or DLC_F32,
 * component c in column c, using its first M columns; scale fp64 [M] or NULL.  No column of x past D and no column of
 * basis past M is ever read.  1 <= rows, D < 2^31, 1 <= M <= DLC_PCA_MAX_COMPONENTS, ldx >= D, ldb >= M, ld_out >= M.
 * ARITHMETIC.  All of it is fp64, every operation rounded on its own (no fma contraction).  For row r and component c:
 * b_d = (double)basis[d][c] (exact for fp32);  t_d = x[r][d] - mean[d], or x[r][d] when mean is NULL.  Chunk j covers
 * d = DLC_PCA_CHUNK * j .. min(D, DLC_PCA_CHUNK * (j + 1)) - 1.  Within a chunk  s_j = +0.0;  for d ascending:
 * q = t_d * b_d;  s_j = s_j + q.  Then  y = s_0;  for j = 1, 2, .. ascending:  y = y + s_j.  out[r][c] = y * scale[c],
 * or y when scale is NULL.  NaN and inf give what IEEE gives.  Only out[r][0 .. M-1] is written; columns M .. ld_out-1
 * keep their bits.  A row's bits depend on that row, mean, basis and scale alone: not on rows, the pitches, the plan or
 * the workspace.  out must not overlap x, mean, basis or scale.
 * PLANS.  DLC_PCA_PLAN_ONE_PASS: a workgroup owns a (row tile, column tile), walks every chunk itself and keeps s and
 * y per output; no workspace.  DLC_PCA_PLAN_SPLIT (rows <= DLC_PCA_SPLIT_MAX_ROWS): a workgroup takes one chunk of a
 * tile and stores every s_j to the workspace [rows][chunks][M]; a finish kernel forms y in chunk order and applies
 * scale -- a frame's gigabyte of basis is streamed by the whole chip.  DLC_PCA_PLAN_AUTO: SPLIT if rows <=
 * DLC_PCA_SPLIT_MAX_ROWS, D > DLC_PCA_CHUNK and ONE_PASS would launch fewer than 256 workgroups (ceil(rows / RT) *
 * ceil(M / CW) with RT = 2 for rows <= 2, else 8, and CW = 512 for rows > 2 and M > 256, else 256); otherwise ONE_PASS.  No atomics;
 * t_d is formed once per (row, d); the basis is read along c.
 * LAUNCHES.  All on `stream`, none synchronises; memory and the workspace (16-byte aligned) are the caller's.
 * ONE_PASS: 1; SPLIT: partial sums, finish.  dlc_pca_project_workspace_bytes(rows, D, M, plan) is host arithmetic: the
 * bytes the plan (AUTO: the plan it chooses) needs -- 0 under ONE_PASS, at least rows * chunks * M * 8 under SPLIT --
 * and 0 for refused shapes.
 * Errors: DLC_ERR_BAD_ARG for a null (x, basis, out) or misaligned pointer, rows / D / M < 1, ldx < D, ldb < M,
 * ld_out < M, an unknown dtype or plan, or out overlapping an input; DLC_ERR_BAD_SHAPE for M > DLC_PCA_MAX_COMPONENTS,
 * rows or D >= 2^31, or SPLIT with more than DLC_PCA_SPLIT_MAX_ROWS rows; DLC_ERR_WORKSPACE for a workspace (SPLIT)
 * that is missing, too small or not 16-byte aligned.  Nothing is written then.
 * The training mean needs no entry point of its own: dlc_kmeans_step with K = 1 is a defined column mean.
 */
#define DLC_PCA_CHUNK 1024
#define DLC_PCA_MAX_COMPONENTS 8192
#define DLC_PCA_SPLIT_MAX_ROWS 64
enum { DLC_PCA_PLAN_AUTO = 0, DLC_PCA_PLAN_ONE_PASS = 1, DLC_PCA_PLAN_SPLIT = 2 };
size_t dlc_pca_project_workspace_bytes(int64_t rows, int64_t D, int M, int plan);
int dlc_pca_project(dlc_ctx* ctx, const double* x, int64_t rows, int64_t D, int64_t ldx,
                    const double* mean /* [D], may be NULL */,
                    int basis_dtype /* DLC_F64 | DLC_F32 */, const void* basis /* [D, ldb], component c in column c */,
                    int M, int64_t ldb, const double* scale /* [M], may be NULL */,
                    double* out, int64_t ld_out, int plan, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Geometric verification of loop candidates over patch key-points: the last stage of a loop closer.  Every detector
 * above reports a candidate on appearance alone; two frames that look alike but are different places (perceptual
 * aliasing) pass all of them.  This stage matches the P patches of the query frame to those of the candidate, fits a
 * 2-D transform to the matched key-points and counts the matches that agree with it.  The matching uses DIST of
 * dlc_vlad_assign; the geometry is an EXHAUSTIVE search in integer arithmetic -- no random sampling, no floating
 * point -- so the result is a function of the inputs alone, whatever the launch plan or the batching.
 * A PAIR is (query frame r, candidate key-frame c = cand[r * ld_cand + s]), 0 <= r < Q, 0 <= s < k.  INPUT.  The P patch
 * descriptors of each frame, fp64, H columns: frame f's patch p is row f * P + p of its matrix (q_desc [Q * P, ldq],
 * db_desc [N * P, ldd]; no column past H is ever read); the P key-points of each frame, int32 (x, y) (q_pts [Q, P, 2],
 * db_pts [N, P, 2]).  1 <= P <= DLC_VERIFY_MAX_PATCHES, 1 <= H, 1 <= k <= DLC_MAX_K, 1 <= Q <= 2^31 / DLC_MAX_K,
 * 1 <= N < 2^31, ld >= H, ld_cand >= k.
 * POINT VALIDITY.  A point is PRESENT iff 0 <= x <= 8191 and 0 <= y <= 8191 (every intermediate below stays under
 * 2^57).  (-1, -1), what dlc_harris_keypoints_u8 writes past a frame's point count, is absent.
 * PATCH MATCHING.  D[p][j] = DIST(q_p, d_j) exactly as defined at dlc_vlad_assign: d = +0.0; for h ascending:
 * t = x_h - c_h; q = t * t; d = d + q -- no fma, never split along H, never formed from a Gram product.  DIST is
 * symmetric bit for bit, so one P x P table serves both directions.  m(p) = the lowest j whose D[p][j] is not NaN and is
 * <= every other non-NaN entry of row p (+inf can win); -1 if the whole row is NaN.  r(j) = the same rule down column
 * j, taking the lowest p.  mutual = 1: match p is kept iff m(p) >= 0 and r(m(p)) == p (the cross-check); mutual = 0:
 * iff m(p) >= 0.  A kept match is dropped if either of its two points is absent.  The surviving set is M; a_p is the
 * query's point p and b_p the candidate's point m(p).  The arg-mins never depend on the points.
 * DLC_VERIFY_SIMILARITY: rotation + uniform scale + translation, orientation-preserving, fixed by two matches.  The
 * hypotheses are the pairs (s, t), s < t, both in M, in ascending lexicographic order.  u = a_t - a_s, v = b_t - b_s.
 * The hypothesis is VALID iff |u|^2 > 0 and |v|^2 > 0 and, when max_scale_x16 = S > 0 (16 <= S <= 256),
 * 256 |v|^2 <= S^2 |u|^2 and 256 |u|^2 <= S^2 |v|^2: the scale lies within [16 / S, S / 16].  For i in M, da = a_i - a_s,
 * db = b_i - b_s, all int64:
 *     re = (db.x * u.x - db.y * u.y) - (v.x * da.x - v.y * da.y)
 *     im = (db.x * u.y + db.y * u.x) - (v.x * da.y + v.y * da.x)
 *     inlier(i)  <=>  re * re + im * im <= tol * tol * (u.x * u.x + u.y * u.y)
 * which is |b_i - (b_s + (v / u)(a_i - a_s))| <= tol in complex numbers, multiplied through by |u|.  The count of a
 * hypothesis is its number of inliers (s and t always count).  The result is the valid hypothesis with the largest
 * count, the first in order among equals; with no valid hypothesis: inliers 0, hypothesis (-1, -1), mask 0.
 * DLC_VERIFY_TRANSLATION: one-match hypotheses s in M, ascending.  e = (b_i - a_i) - (b_s - a_s); inlier(i) iff
 * e.x^2 + e.y^2 <= tol^2.  The same selection; the hypothesis is (s, -1).  0 <= tol <= 255.
 * OUTPUTS per pair, [Q, k]-shaped with row pitch k (pair r * k + s): out_inliers int32; out_matches int32 = |M|;
 * out_hyp int32 x 2 (optional); out_mask uint64 (optional): bit p is set iff match p is an inlier of the winning
 * hypothesis; out_match int32 [P] (optional): m(p) for p in M, else -1; out_dist fp64 [P, P] (optional): the table D.
 * A pair whose candidate id is < 0 or >= N writes inliers 0, matches 0, hyp (-1, -1), mask 0 and match -1 and leaves
 * its out_dist slot untouched.  A pair's result depends on that pair's 2 P descriptors and 2 P points alone: not on Q,
 * k, the pitches or which other pairs are in the call.
 * LAUNCHES.  Two on `stream` (the tables; the resolution), none synchronises; memory and the workspace (16-byte
 * aligned) are the caller's.  The call always needs dlc_verify_pairs_workspace_bytes(Q, k, P) bytes: the tables live
 * there unless out_dist is given.  Nothing but the stated outputs and the workspace is written.
 * Errors: DLC_ERR_BAD_ARG for a null (descriptors, points, cand, out_inliers, out_matches) or misaligned pointer,
 * Q / N / P / H < 1, k outside 1..DLC_MAX_K, ld < H, ld_cand < k, an unknown model, tol outside 0..255, max_scale_x16
 * neither 0 nor in 16..256, mutual neither 0 nor 1; DLC_ERR_BAD_SHAPE for P > DLC_VERIFY_MAX_PATCHES,
 * Q > 2^31 / DLC_MAX_K or N >= 2^31; DLC_ERR_WORKSPACE for a workspace that is missing, too small or not 16-byte
 * aligned.  Nothing is written then.  dlc_verify_pairs_workspace_bytes returns 0 for refused shapes.
 */
#define DLC_VERIFY_MAX_PATCHES 64
enum { DLC_VERIFY_SIMILARITY = 0, DLC_VERIFY_TRANSLATION = 1 };
size_t dlc_verify_pairs_workspace_bytes(int64_t Q, int k, int P);
int dlc_verify_pairs(dlc_ctx* ctx, const double* q_desc, int64_t ldq /* doubles between patch rows, >= H */,
                     const int32_t* q_pts /* [Q, P, 2] */, int64_t Q,
                     const double* db_desc, int64_t ldd, const int32_t* db_pts /* [N, P, 2] */, int64_t N,
                     int P, int64_t H, const int64_t* cand, int64_t ld_cand, int k,
                     int model, int tol, int max_scale_x16, int mutual,
                     int32_t* out_inliers, int32_t* out_matches, int32_t* out_hyp /* may be NULL */,
                     uint64_t* out_mask /* may be NULL */, int32_t* out_match /* may be NULL */,
                     double* out_dist /* may be NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- match: cosine similarity + top-k (BASELINE.json north_star; not in the reference) */
/*
 * Row L2-normalisation (optional mean-centring first) of src[n,d] (DLC_F32 or
 * DLC_F64, row stride lds) into the stored descriptor format dst[n, ldd]
 * (DLC_BF16 or DLC_F16), columns d..ldd-1 zero-filled.  ldd must be a multiple
 * of 64 (the GEMM's K step).
 * Each element is (x - mean) * (1 / norm) evaluated in fp64 and rounded fp64 ->
 * fp32 -> the stored type, both to nearest even; a row's bits depend on the
 * row, d, ldd, the types and the alignment of its operands, never on the other
 * rows of the call.  A row of zeros (or, centred, of one repeated value whose
 * mean is exact) is stored as zeros; a row holding a NaN or an infinity is
 * stored with at least one NaN.
 * ALIGNMENT.  dst must be 4-byte aligned (outputs are stored in pairs;
 * DLC_ERR_BAD_SHAPE otherwise); src needs its type's alignment only.  The
 * one-pass forms additionally want src 16-byte aligned, lds a multiple of 16
 * bytes and dst 8-byte aligned -- any other call is served by the multi-pass
 * kernel, same values up to the summation order.
 * RANGE.  Sums of squares are formed in fp64 without scaling: every fp32 source
 * is in range; an fp64 source must keep |x - mean| within [1e-154, 1e154] (or
 * zero) -- beyond it the squares under- or overflow and the row is not
 * normalised.
 */
int dlc_l2_normalize_rows(dlc_ctx* ctx, int src_dtype, const void* src, int64_t n, int64_t d, int64_t lds,
                          int center, int dst_dtype, void* dst, int64_t ldd, void* stream);
/*
 * Top-k cosine match of q query rows against n database rows of width d
 * (both stored in `dtype` = DLC_BF16 / DLC_F16; row strides ldq / lddb in elements, d a multiple of
 * 64, rows 16-byte aligned).
 *
 * NORMS.  tau_scale = NULL states that every query and database row is what dlc_l2_normalize_rows
 * wrote (norm <= 1.005): the certificate's tau below is derived for |q| |x| <= 1.01.  Rows from anywhere
 * else (descriptors stored by another tool, a saved shard, un-normalised vectors) need
 * tau_scale = the [q] floats of dlc_cosine_tau_scale(Q, the database's largest row norm from
 * dlc_max_row_norm): query i then certifies with tau * tau_scale[i] -- the score pass's error is linear in
 * |q| |x| -- and the result is the exact fp64 top-k for operands of ANY norm (elements finite,
 * |q| |x| < 2^21 so that the ordering key below does not saturate).  A scale of +inf (a non-finite norm)
 * certifies nothing: that query is decided by the exhaustive pass.  Every call of the staged / sharded
 * forms below takes the same array; all shards must use the bound of the WHOLE database (the maximum
 * over the shards' dlc_max_row_norm).
 *
 * THE SCORE of a (query, row) pair is one number, whatever call, plan, shard or batch computes it:
 * the fp64 sum of the exact products of the stored elements (bf16 / fp16 products are exact in
 * fp64; the additions follow one fixed order that depends on d only).  THE ORDER of every result is
 * score descending on the key round(score * 2^40), ties -> lower global row index: the order of
 * oracle/cosine.py.  out_scores_f64[q,k] (may be NULL) receives the fp64 scores, out_scores[q,k]
 * the same values rounded once to fp32, out_idx[q,k] the rows (int64, row_offset added -- the
 * shard's first global row).  Slots past min(k,n) get -inf / -1.  1 <= k <= DLC_MAX_K.
 *
 * How the rows are found.  The score pass (bf16/fp16 MFMA, fp32 accumulate; a v_dot2 bandwidth
 * kernel for <= 4 queries) only chooses CANDIDATES: it keeps the maximum of every 8 database rows
 * (and, for databases of <= 16384 rows, the fp32 score matrix itself in the workspace).  The
 * selection takes the kg = dlc_cosine_groups_per_query(k) = k + 4 groups with the largest maxima
 * (under the small-database plan the k + 4 best rows of those groups), re-scores them in fp64,
 * ranks them, and CERTIFIES the result: every row left behind has an fp32 score <= B (the best
 * group / row not taken), fp32 scores err by at most tau = dlc_cosine_score_error_bound(...)
 * against the fp64 score, so the result is the exact top-k when the k-th fp64 score > B + tau.
 * Queries that fail the test (crowded scores: more near-ties at the k-th place than the slack
 * holds) go through an exhaustive pass in the same call: every group whose maximum is >= (k-th
 * score found) - tau is re-scored in fp64 against a running top-k.  out_status[q] (int32, may be
 * NULL): 0 = certified at once, 2 = resolved by the exhaustive pass.  Either way the result is the
 * top-k of the fp64 scores; the pass costs time only (in the degenerate case of a database of
 * near-identical rows it is an fp64 brute force for that query).
 * Plans (picked from the shape; the workspace size reflects them): one score pass for databases of
 * >= 256 tiles of 256 rows; split-K partial score tiles + a reducing pass (chunks summed in fp64)
 * for few rows with long descriptors; for <= 32 queries with long rows the re-score is spread over
 * one workgroup per selected group and merged; against <= 16384 rows (k <= 35; with <= 4 queries: up to
 * 32 MB of database, beyond that the bandwidth kernel streams it) one selection launch
 * sums the partial scores, picks the candidate ROWS, re-scores and certifies (and runs the exhaustive
 * pass of its own uncertified queries).  Results are identical across plans.
 */
#define DLC_MAX_K 128
size_t dlc_cosine_topk_workspace_bytes(int64_t q, int64_t n, int64_t d, int k);
/*
 * The pruned score pass (dlc_cosine_topk only).  The selection reads the group maxima and the half-tile hints (below)
 * of the kt = min(kg, half tiles) half tiles of 128 rows with the largest maxima only, so on the one-pass MFMA plan the
 * score pass of dlc_cosine_topk does not store the rest: per query it keeps a running lower bound of the kt-th largest
 * half-tile maximum and writes a half tile's 16 group maxima and its hint only where the half tile's maximum reaches
 * the bound.  The half-tile maxima themselves are always written.  The state -- per query 64 uint32 score keys
 * bkt[64][q] (class major: the largest half-tile key seen in class `half tile % 64`, 0 = none) and one uint32 threshold thr[q] --
 * sits BEHIND the workspace: dlc_cosine_topk_prune_bytes(q, n, d, k) is that room (0 where the plan does not prune), and
 * a call prunes when its workspace holds dlc_cosine_topk_workspace_bytes + dlc_cosine_topk_prune_bytes bytes; with less
 * it writes everything, as every other entry point does.  ABI: callers ask both functions, never compute the sizes;
 * no array of the workspace moved.  The state is cleared on the stream before the score pass of every pruned call.
 *   It prunes when   the plan writes the hints (one pass, not the <= 16384-row plan, more than 4 queries), kg = k + 4 <= 64,
 *                    the re-score is not spread over several workgroups per query, and the shard has at most 24576 half
 *                    tiles (3.1 M rows: beyond that the selection consumes the half-tile maxima in place).
 *   Why it is safe   Every value bkt[b][q] ever holds is 0 or the key of a half tile of class b of this call, and classes
 *                    are disjoint, so the kt-th largest of ANY snapshot of bkt[*][q] -- at any time, under any
 *                    interleaving, with stale or lost updates -- is at most the call's true kt-th largest half-tile key.
 *                    thr[q] only ever holds such a value rounded down to its top 20 bits (0 while fewer than kt classes are filled).  The selection
 *                    takes half tiles at or above the true kt-th key only (ties by index), and such a half tile passes
 *                    `key >= thr` whatever value of thr its workgroup saw: everything the selection reads was written.
 *   The exhaustive   pass behind a pruned call computes thr_final, the kt-th largest of the final bkt[*][q] (a function of
 *   pass             the half-tile maxima alone, >= every threshold the score pass went by), skips a half tile whose
 *                    maximum is below its bound, goes by the group maxima where key(half-tile maximum) >= thr_final
 *                    (they were written) and takes all 16 groups of any other half tile.  More groups, the same
 *                    result: the exact top-k by (fp64 key descending, row ascending) over rows that include every row
 *                    that can belong to it.
 * Scores, rows and status are bit for bit those of the unpruned call.  dlc_set_prune_mode (one setting per context):
 *   DLC_PRUNE_ON    the default.
 *   DLC_PRUNE_OFF   dlc_cosine_topk writes everything, exactly as before the pruned pass existed.
 *   DLC_PRUNE_KEEP  for tests: the state is cleared only on the first of a run of calls with the same workspace, Q, DB
 *                   and shape, and every call leaves thr = thr_final behind.  A repeated call then starts from its own
 *                   final threshold and writes exactly what pruning can never drop -- the extreme of the protocol,
 *                   deterministic at any size.  The caller must not change the contents of Q or DB inside such a run.
 *                   Setting any mode ends the run.
 */
#define DLC_PRUNE_ON 0
#define DLC_PRUNE_OFF 1
#define DLC_PRUNE_KEEP 2
size_t dlc_cosine_topk_prune_bytes(int64_t q, int64_t n, int64_t d, int k);
int dlc_set_prune_mode(dlc_ctx* ctx, int mode);
int dlc_cosine_topk(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                    const void* DB, int64_t n, int64_t lddb, int64_t d, int k, int64_t row_offset,
                    float* out_scores, double* out_scores_f64, int64_t* out_idx, int32_t* out_status,
                    const float* tau_scale, void* workspace, size_t workspace_bytes, void* stream);
/*
 * The two reductions behind tau_scale (rows as the match takes them: 16-byte aligned, d and the stride multiples of 8).
 *   dlc_max_row_norm      *max_norm (ONE device float the caller zeroed before the first call) = max(*max_norm, the
 *                         largest L2 norm of rows [n, d], fp32, rounded up; +inf when an element is not finite).
 *                         Call it once per shard at load time and again for appended rows; sharded: all-reduce(MAX).
 *   dlc_cosine_tau_scale  tau_scale[i] = max(1, |Q_i| * R / 1.01), R = *db_max_norm (a device float; NULL = 1.005: the
 *                         database is dlc_l2_normalize_rows' output and only the queries are foreign).
 * Both never under-report: the norm is an fp32 sum of squares (one chain per lane of a wave) times 1.001, which covers the
 * chain's rounding for rows of up to 2^20 elements (d <= 1048576: the worst row loses 1e-3 of its sum of squares there);
 * longer rows are outside the guarantee, and so are rows whose elements are so small (|x| < 1.1e-19) that their squares
 * are not normal fp32 numbers.  Neither over-reports by more than 1 %, by the same count: a lane's chain of d / 64 fp32
 * fmas and the butterfly can also err UPWARDS by 1e-3 of the sum of squares at 2^20 elements (5e-4 of the norm); with the
 * 1.001, the roundings of the square root and the products, the scale's 1.000001 and its rounded 1 / 1.01 the factor stays
 * below 1.002.  The padding ld > d is never read.
 */
int dlc_max_row_norm(dlc_ctx* ctx, int dtype, const void* rows, int64_t n, int64_t ld, int64_t d, float* max_norm,
                     void* stream);
int dlc_cosine_tau_scale(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq, int64_t d,
                         const float* db_max_norm, float* tau_scale, void* stream);
/*
 * The same match with an age limit per query (the streaming loop-closure query, SURVEY 8f-4, for a batch of frames that
 * were appended to the database together): query i only sees rows 0 .. min(n, limit0 + i) - 1 (local rows, before
 * row_offset); a query that sees nothing gets (-inf, -1) and status 0.  One score pass over the n rows serves the whole
 * batch -- its group maxima remain upper bounds of what a query may see, which is all the selection and the certificate
 * need; rows a query may not see are never re-scored.  Same workspace, plans, ordering rule and status values as
 * dlc_cosine_topk; the lists equal dlc_cosine_topk with k + q - 1 candidates followed by dlc_topk_keep_older.
 */
int dlc_cosine_topk_older(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                          const void* DB, int64_t n, int64_t lddb, int64_t d, int k, int64_t row_offset, int64_t limit0,
                          float* out_scores, double* out_scores_f64, int64_t* out_idx, int32_t* out_status,
                          const float* tau_scale, void* workspace, size_t workspace_bytes, void* stream);
/*
 * tau of the plan dlc_cosine_topk takes for this shape: |fp32 score of the score pass - fp64 score|
 * <= tau for rows of norm <= 1.005 (times tau_scale[i] for any other operands, see NORMS above).  (s MFMA / v_dot2 accumulation steps of at most 2^-23 *
 * (|accumulator| + sum |products|) each, partial sums <= |q| |x| <= 1.01: tau = 2^-23 * 1.01 *
 * (s + 2) + 2^-38; s = 2 * (K tiles of 64 per split-K chunk).  4096-d one pass: 1.6e-5.)
 * A caller that merges shards of different shapes certifies with the largest of their taus:
 * dlc_cosine_score_error_bound_any_plan(d) is the largest tau ANY plan has for descriptors of width d (the unsplit
 * MFMA pass, or the bandwidth kernel's chain for very short rows) -- the same number on every rank whatever its shard's
 * size or plan, which is what a sharded merge must certify with.
 */
double dlc_cosine_score_error_bound(int64_t q, int64_t n, int64_t d, int k);
double dlc_cosine_score_error_bound_any_plan(int64_t d);
/*
 * The two stages of dlc_cosine_topk as separate calls, for callers that pipeline batches
 * over two streams (stage 2 of batch i overlapping stage 1 of batch i+1, each batch with its
 * own workspace):
 *   dlc_cosine_score_groups  -- the score pass; fills the workspace, reads Q and DB;
 *   dlc_cosine_select_topk   -- selection, fp64 re-score, final top-k, certificate, exhaustive
 *                               pass; reads the workspace (and consumes it), Q and DB.
 * Same operand rules, same workspace size (dlc_cosine_topk_workspace_bytes), same results.
 * flags: DLC_SELECT_COOP selects a small-footprint kernel (256 threads, < 96 VGPRs, a few KiB
 * of LDS) whose workgroups can share a CU with a running score GEMM.  DLC_SELECT_NO_HINTS makes the
 * selection ignore the score pass's half-tile hints (below) and re-score every selected group whole: the
 * same results bit for bit, more rows gathered -- it is there so that tests can hold the two against each other.
 * DLC_SELECT_SERIAL (dlc_cosine_select_topk and dlc_cosine_select_groups) does the same for the filtered selection
 * (below): the 512-thread kernels extract the best half tiles one at a time and rank every key, as the general path
 * does -- the same results bit for bit, group_max's bound column included.
 */
#define DLC_SELECT_COOP 1
#define DLC_SELECT_NO_HINTS 2
#define DLC_SELECT_SERIAL 4
int dlc_cosine_score_groups(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                            const void* DB, int64_t n, int64_t lddb, int64_t d, int k,
                            void* workspace, size_t workspace_bytes, void* stream);
int dlc_cosine_select_topk(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                           const void* DB, int64_t n, int64_t lddb, int64_t d, int k, int64_t row_offset,
                           float* out_scores, double* out_scores_f64, int64_t* out_idx, int32_t* out_status,
                           const float* tau_scale, void* workspace, size_t workspace_bytes, int flags, void* stream);
/*
 * Stage 2 split once more, for a database sharded over several GPUs.  Each shard would
 * otherwise re-score its own kg = dlc_cosine_groups_per_query(k) best groups per query, whatever
 * the shard size; exchanging the groups' MAXIMA first lets every shard skip the groups that
 * cannot be among the kg best of the whole database:
 *   dlc_cosine_select_groups -- from the workspace: group_ids [q,kg] (int32 shard-local group
 *                               index, -1 = none) and group_max [q,kg+1] (fp32): the groups'
 *                               maxima in rank order and, in column kg, the largest maximum among
 *                               the shard's groups that are NOT listed (-inf: none);
 *   (caller: all-gather group_max over the `parts` shards -> all_group_max [parts,q,kg+1])
 *   dlc_cosine_rescore_topk  -- drops every own group with >= kg strictly larger maxima in
 *                               all_group_max (parts = 0: no filter), re-scores the rest in fp64
 *                               and writes the shard's part of the top-k (fp64 scores + rows) and,
 *                               to out_bound[q] (may be NULL), the largest fp32 score a row outside
 *                               the surviving groups of ALL shards can have -- the same value on
 *                               every shard;
 *   (caller: all-gather the parts; dlc_topk_merge_strided with bound = out_bound and tau = the
 *    largest dlc_cosine_score_error_bound of the shards: out_status[q] = 0 certified / 1 not)
 *   dlc_cosine_exhaustive_topk -- for the queries with status[q] == 1 (others are skipped on the
 *                               device): lower[q * lower_stride] = the k-th merged fp64 score (-inf:
 *                               fewer than k rows found); every group of THIS shard whose maximum
 *                               (still in the workspace of the score pass) is >= lower - tau is
 *                               re-scored in fp64; the shard's exact top-k over those rows REPLACES
 *                               out_*[q] and status[q] becomes 2.  Merging these per-shard lists
 *                               (taking, per query, the new list where status == 2) gives the exact
 *                               global top-k.  dlc_cosine_topk / dlc_cosine_select_topk run it
 *                               themselves; a sharded caller runs it when any status is 1.
 *
 * What each stage hands out, exactly (tests/shard_protocol_oracle.py restates it on the host; tests/
 * test_gpu_shard_protocol.py holds the library to it).  tau_shard = dlc_cosine_score_error_bound of the shard's
 * shape, tau_any = dlc_cosine_score_error_bound_any_plan(d), both times tau_scale[q] where the caller supplies one:
 *   group_ids / group_max  The min(kg, groups of the shard) groups with the largest fp32 maxima, ordered by (maximum
 *                          descending, group index ascending) -- among groups of equal maxima the lower index is
 *                          listed first, and is the one listed at all where the list ends inside a tie; each group
 *                          once; the -1 / -inf padding only at the end.  group_max[e] is within tau_shard of the
 *                          fp64 maximum of group e's rows (rows past n do not count), no unlisted row of the shard
 *                          scores above group_max[kg] + tau_shard in fp64, group_max[kg] <= every listed maximum,
 *                          and it is -inf exactly when every group of the shard is listed.
 *   the filter             "Strictly larger" is the comparison of the fp32 values (equal maxima never drop one
 *                          another; -inf entries count for nothing), over the kg listed columns of all `parts`
 *                          shards, the shard's own included.  parts = 0 keeps every listed group.
 *   the part               The k best rows of the surviving groups by (f64 key descending, row ascending), their fp64
 *                          scores THE scores; (-inf, -1) past the rows found -- all of it where no group survives.
 *                          The group list is only read.
 *   out_bound              max(column kg of every shard, every listed maximum the filter drops on any shard), -inf
 *                          when there is neither: a function of all_group_max alone, so bit-equal on every shard.
 *                          (parts = 0: the shard's own column kg.)  No row outside the surviving groups of all shards
 *                          scores above out_bound + tau_any in fp64.
 *   the merge              Orders the parts' entries by (f64 key descending, global row ascending), whatever order the
 *                          parts were gathered in; entries with idx < 0 are empty.  out_status[q] = 0 when bound[q]
 *                          is -inf (nothing was left behind -- also when fewer than k rows exist at all) or when k rows
 *                          were found and the k-th fp64 score > (double)bound[q] + tau * (double)tau_scale[q]; 1
 *                          otherwise.  A query with status 0 holds the exact global top-k already.
 *   the half-tile hints    (inside dlc_cosine_topk / dlc_cosine_select_topk only; the sharded stages never read them.)  On the
 *                          one-pass MFMA plan -- no split-K, not the <= 16384-row plan, more than 4 queries -- the score pass
 *                          also writes, per (query, half tile of 128 rows), 8 bytes into the workspace behind the half-tile
 *                          maxima: for G*, the lowest group holding the half tile's maximum, the lowest row a* of G* that
 *                          attains it and r2, the largest fp32 score of G*'s other seven rows (rows past n are copies of
 *                          row n - 1, so r2 may equal the maximum there).  The 512-thread selection, looking at the whole
 *                          database (not DLC_SELECT_COOP, not dlc_cosine_topk_older), takes ONE candidate, row a*, from a
 *                          selected group that is its half tile's G* and has (double)r2 < u_k - 2 tau, u_k = the k-th
 *                          largest group maximum (strict: never with tau = +inf, a NaN, or fewer than k groups), and r2
 *                          counts as left behind; every other selected group hands in its 8 rows.  Nothing observable
 *                          changes: k groups have a maximum >= u_k and the row attaining it is re-scored either way,
 *                          so the k-th fp64 score s_k >= u_k - tau; a skipped row has an fp32 score <= r2 < u_k - 2 tau,
 *                          hence an fp64 score < u_k - tau <= s_k -- it is never in the top-k, never ties with its k-th
 *                          score, cannot fail the certificate (s_k > r2 + tau) and does not move the `lower` the
 *                          exhaustive round starts from.  Scores, rows and status are those of DLC_SELECT_NO_HINTS.
 *   the filtered selection (the 512-thread kernels, up to 8192 half tiles per shard; integer keys only: the ordering key of
 *                          an fp32 maximum, then the lower index.)  The kt = min(kg, half tiles) best half tiles: every lane
 *                          holds up to 16 keys, T = the largest over the 8 waves of the kt-th largest LANE MAXIMUM of a wave
 *                          (0 where a wave has fewer than kt lanes with a key).  kt lanes hold kt distinct half tiles, so at
 *                          least kt keys are >= T, i.e. T <= the kt-th largest key.  Behind the pruned score pass T is also
 *                          raised to the kt-th largest of the query's 64 class maxima, a lower bound of the kt-th largest key
 *                          by the pruned pass's own argument (distinct classes hold distinct half tiles).  Only the keys >= max(T, 1) are ranked.
 *                          A key that is not ranked is < T <= the kt-th largest: it is neither selected nor tied with a
 *                          selected key.  The (kt+1)-th largest key overall -- what column kg and the certificate bound the
 *                          rest by -- is the larger of the (kt+1)-th ranked key and the best key not ranked.  More ranked
 *                          keys than the kernel has room for (16 kg; a database of identical rows): the general one-by-one
 *                          extraction runs instead.  The kg groups inside them, the same way: T2 = the smallest, over
 *                          the kt selected half tiles, of the largest group key of a half tile; kt distinct groups have
 *                          a key >= T2, so where kt >= the number of groups to keep only the keys >= T2 are ranked and the
 *                          best other key joins the rest (T2 = 0, every key ranked, otherwise).  The final top-k ranks the
 *                          rows that were re-scored, without the empty slots of the rows that were not.  Lists, order,
 *                          status and bounds are those of DLC_SELECT_SERIAL.
 *   the exhaustive round   Touches the queries with status 1 only: their lists are replaced and their status becomes
 *                          2; every other query's status, scores and rows are left as they are.  lower_stride = 0
 *                          reads one number for every query.  tau must be >= 0 (NaN is refused), lower_stride >= 0.
 * Refusals write nothing: dlc_cosine_rescore_topk with parts < 0 or parts > 0 and no all_group_max
 * (DLC_ERR_BAD_ARG); dlc_topk_merge_strided with parts < 1, a part stride below q * k, tau < 0 or NaN
 * (DLC_ERR_BAD_ARG) or parts * k > 2048 (DLC_ERR_BAD_SHAPE).
 */
int dlc_cosine_groups_per_query(int k);
int dlc_cosine_select_groups(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                             const void* DB, int64_t n, int64_t lddb, int64_t d, int k,
                             void* workspace, size_t workspace_bytes,
                             int32_t* group_ids, float* group_max, int flags, void* stream);
int dlc_cosine_rescore_topk(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                            const void* DB, int64_t n, int64_t lddb, int64_t d, int k, int64_t row_offset,
                            const int32_t* group_ids, const float* group_max,
                            const float* all_group_max, int parts,
                            double* out_scores_f64, int64_t* out_idx, float* out_bound, const float* tau_scale,
                            int flags, void* stream);
int dlc_cosine_exhaustive_topk(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                               const void* DB, int64_t n, int64_t lddb, int64_t d, int k, int64_t row_offset,
                               const double* lower, int64_t lower_stride, double tau, const float* tau_scale,
                               int32_t* status, float* out_scores, double* out_scores_f64, int64_t* out_idx,
                               void* workspace, size_t workspace_bytes, void* stream);
/*
 * Streaming loop-closure queries: a batch of B new frames is matched in one dlc_cosine_topk call with
 * kk = k + B - 1 candidates per frame; frame b may only see key-frames older than limit0 + b.  Row b of the best-first
 * lists scores / idx [rows, kk] keeps its first k entries with 0 <= id < limit0 + b (order kept); the rest of its k
 * slots are (-inf, -1).  kk, k <= DLC_MAX_K.
 */
int dlc_topk_keep_older(dlc_ctx* ctx, const float* scores, const int64_t* idx, int64_t rows, int kk,
                        int64_t limit0, int k, float* out_scores, int64_t* out_idx, void* stream);
/*
 * Merge `parts` per-shard results ([parts, q, k] fp64 scores + int64 rows, as an all-gather leaves
 * them; idx < 0 = empty slot) into the global top-k with the same ordering rule (fp64 key, then the
 * lower row).  out_scores (fp32) / out_scores_f64 may be NULL, not both.
 */
int dlc_topk_merge(dlc_ctx* ctx, const double* scores_f64, const int64_t* idx, int parts, int64_t q, int k,
                   float* out_scores, double* out_scores_f64, int64_t* out_idx, void* stream);
/* Same with explicit distances (in elements) between consecutive parts, for results that were
 * gathered as one packed buffer per shard, and with the certificate of the sharded protocol above:
 * bound [q] (may be NULL: nothing left behind), tau and tau_scale [q] (may be NULL: 1) -> out_status[q] (may be
 * NULL).  parts * k <= 2048. */
int dlc_topk_merge_strided(dlc_ctx* ctx, const double* scores_f64, int64_t score_part_stride,
                           const int64_t* idx, int64_t idx_part_stride, int parts, int64_t q, int k,
                           const float* bound, double tau, const float* tau_scale,
                           float* out_scores, double* out_scores_f64, int64_t* out_idx, int32_t* out_status,
                           void* stream);
/*
 * Dense score block S[q, n] (fp32) = Q . DB^T for the all-vs-all cosine
 * matrix of config 2 (small N); same operand rules as dlc_cosine_topk.
 * Few rows with long descriptors (config 2: 1063 x 75 000) are scored split-K: the partial
 * score tiles go through a caller-provided workspace of dlc_cosine_scores_workspace_bytes()
 * bytes (0 when the shape is scored in one pass; workspace may then be NULL), 256-byte aligned,
 * and are summed in chunk order (deterministic).  dlc_cosine_topk does the same inside its own
 * workspace.
 */
size_t dlc_cosine_scores_workspace_bytes(int64_t q, int64_t n, int64_t d);
int dlc_cosine_scores(dlc_ctx* ctx, int dtype, const void* Q, int64_t q, int64_t ldq,
                      const void* DB, int64_t n, int64_t lddb, int64_t d,
                      float* S, int64_t lds, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The cosine path's score as rows (cosine_rows.hip): out_scores[r * ld_out + j] = THE score of query row r and
 * database row j -- the ONE number of the cosine path, the fp64 sum of the exact products in the order of rescore8_f64
 * (cosine_topk.hip): lane l of a wave takes the 16-byte pieces l, l + 64, ... of the two rows in ascending order, one
 * fp64 fma chain over each piece's eight elements in ascending order, from +0.0 (a lane with no piece contributes +0.0);
 * the 64 chains are combined by the xor 32, 16, ..., 1 butterfly.  It is a function of (query row, database row, d)
 * alone -- not of the tile shape, the limits or the other queries of the call -- and it is, bit for bit, what
 * dlc_cosine_topk* write to out_scores_f64 for that pair.  out_keys[r * ld_out + j] = the integer the whole cosine path
 * ranks by: round-half-even(score * 2^40), clamped (NaN, -inf and anything below -4e18 -> INT64_MIN + 1; above 4e18 ->
 * INT64_MAX).  Either output may be NULL, not both.  int64 key rows are what dlc_sequence_topk(DLC_I64) takes: sums of
 * keys are exact and free of summation order, and its ranking (value, then the lower column) is then the cosine path's
 * own rule.
 * Row r is written for 0 <= j < lim(r), lim(r) = clamp(limit0 + r * limit_step, 0, n) -- the limit convention of
 * dlc_cnnvtl_distance_rows, dlc_topk_rows_f64 and dlc_sequence_topk; any limit_step, negative included.
 * EVERY OTHER WORD OF THE OUTPUTS KEEPS ITS BITS: the cells at or past lim(r) and the columns n .. ld_out-1.  When
 * every lim(r) is 0 nothing is launched and the call returns DLC_OK.
 * Operands as in dlc_cosine_topk -- rows as stored, bases 16-byte aligned -- except that d need only be a multiple of 8
 * (and the strides, >= d); Q may be rows of DB (both are only read); the outputs (8-byte aligned, ld_out >= n) must
 * not overlap the operands.  Any argument error is DLC_ERR_BAD_ARG and leaves the outputs untouched.
 * No workspace, no memset, no atomics; one launch on `stream` (a wave per 4 x 4 block of pairs, 1 x 8 for a single
 * query; the operands come straight from L2); never synchronises.
 */
int dlc_cosine_score_rows(dlc_ctx* ctx, int dtype /* DLC_BF16 | DLC_F16 */,
                          const void* Q, int64_t q, int64_t ldq,
                          const void* DB, int64_t n, int64_t lddb, int64_t d,
                          int64_t limit0, int64_t limit_step,
                          double* out_scores, int64_t* out_keys, int64_t ld_out, void* stream);

/* ---- host arrays in, host arrays out (the reference's NumPy contract) ----------- */
/*
 * The reference's callers hand over and receive PAGEABLE host arrays (SDAV.transform: ndarray in, ndarray out,
 * src/sdav/network/SDAV.py:293-302; CnnVtl.transform, src/cnn_vtl/network/cnn_vtl.py:130-133).  These two calls move
 * such an array through the context's pinned staging ring (8 pieces of 16 MiB, created on first use): host threads
 * copy a piece between the caller's memory and a page-locked buffer while the DMA engine moves the piece before it.
 *   dlc_host_to_device  returns when src_host has been consumed (the caller may overwrite it); the last pieces' DMAs
 *                       are still in flight on `stream` -- work that reads dst_device must be ordered behind it there;
 *   dlc_device_to_host  reads src_device in `stream` order and returns when dst_host is complete (BLOCKING: a host
 *                       array cannot be handed back earlier).
 * Give them their own streams (with events to the compute stream) and a batch's upload, its kernels and the download
 * of the batch before overlap: deeploopcloser_amd/engine.py run_chunked() is that pipeline.
 * dlc_set_host_threads: host copy threads (0 = min(16, hardware threads): one GPU's share of the host).
 * One staged transfer per context at a time (calls from several threads serialise).
 */
int dlc_host_to_device(dlc_ctx* ctx, void* dst_device, const void* src_host, size_t bytes, void* stream);
int dlc_device_to_host(dlc_ctx* ctx, void* dst_host, const void* src_device, size_t bytes, void* stream);
int dlc_set_host_threads(dlc_ctx* ctx, int threads);

/* ---- split-K scratch of the dense GEMMs ------------------------------------- */
/*
 * Latency mode (a single frame: SDAV layers with M = 30 rows, conv3-5 with M = 130 output
 * pixels) leaves a 128x128-tiled GEMM with a handful of workgroups walking a long K.  When
 * the caller lends the context a scratch buffer, dlc_gemm_bias_act / dlc_conv2d_nhwc_f64 /
 * dlc_sdav_encode cut K into chunks for such shapes (partial tiles in the scratch, summed in
 * chunk order by a second kernel that applies bias + activation): deterministic, results
 * equal to the one-pass kernel up to the summation order.  The buffer stays caller-owned
 * (device memory, 256-byte aligned, >= a few MiB to be useful; NULL / 0 turns the mode off)
 * and must outlive every call that may use it; calls sharing one context's scratch must be
 * stream-ordered with respect to each other.
 */
int dlc_set_scratch(dlc_ctx* ctx, void* scratch, size_t bytes);

/* ---- introspection used by bench.py (kernel-only timing with HIP events) -- */
/*
 * With profiling enabled every launch of a product kernel records a hipEvent pair around it on
 * its stream, one entry of a ring of DLC_PROFILE_RING slots: the MFMA score GEMM of dlc_cosine_topk /
 * dlc_cosine_score_groups, the dense fp64 / fp32 GEMM kernels (dlc_gemm_bias_act, dlc_conv2d_nhwc_f64,
 * dlc_sdav_encode(_split), dlc_sdav_train_step) and the int8 / fp64 Gram kernels of
 * dlc_sdav_similarity_matrix.  A split-K reduce or min / max fold is not timed; a GEMM run as two
 * launches records two entries.  dlc_profile_gemm_ms() waits for the recorded events and writes the
 * durations (milliseconds, oldest first) of the last min(entries, capacity, DLC_PROFILE_RING) entries
 * to the HOST array out_ms; it returns how many it wrote (negative dlc_status on error).  Enabling
 * resets the ring.
 */
#define DLC_PROFILE_RING 256
int dlc_set_profiling(dlc_ctx* ctx, int enabled);
int dlc_profile_gemm_ms(dlc_ctx* ctx, float* out_ms, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* DLC_H_ */
