// Sign-random-projection hashes: a float descriptor row -> an int8 row (dlc_lsh_quantize_i8) -> the sign of its integer
// products with `bits` int8 hyperplanes, packed (dlc_lsh_hash_i8).  include/dlc.h holds the definitions.
//
//   quantise:  one workgroup per row, two passes over it: the largest |t_d| and "a NaN or an infinity was seen", then
//              the bytes.  fp64, one rounding per operation (a product and a difference are never contracted: there is
//              nothing to contract them with).
//   hash:      v_mfma_i32_16x16x64_i8 through the builtin, accumulators the compiler's.  The descriptors are the A
//              operand and the planes the B operand, both read from global memory straight into the fragment: lane l
//              holds bytes 16 (l / 16) .. + 15 of the 64-byte k-step of row l % 16 (A) or plane l % 16 (B) -- the same k
//              map on both sides, and an integer sum takes any order.  The result has the plane on the lane (col = lane
//              & 15) and the row in (lane >> 4, register): ONE ballot of acc[reg] > 0 is the 16-bit words of four rows,
//              so the pack needs no LDS.  A wave owns MT x NT tiles of 16 x 16 and a workgroup WR x WC waves.
//              The K tail is masked on the A side alone (0 . anything = 0) and no byte past D is read on either side;
//              rows past `rows` and planes past `bits` are clamped to the last one, never stored / written as 0.
//   split:     the same body over one DLC_LSH_CHUNK piece of D, int32 sums stored (plain stores) at [chunk][row][bit];
//              the finish adds a bit's chunks, one lane per bit, and a ballot is 8 finished bytes.
// Integers throughout: the code is a function of the row and the planes alone, whatever the plan.
#include "dlc_internal.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int v4i;

constexpr int LSH_Q_THREADS = 256;
constexpr int LSH_FILL = 256;                      // workgroups that fill the chip: below it the smaller tile is taken

struct LshQuantArgs {
    const void* x;
    const double* mean;
    int8_t* q;
    long long D, ldx, ldq;
};

template <typename T> __device__ __forceinline__ double lsh_load(const void* x, long long i);
template <> __device__ __forceinline__ double lsh_load<double>(const void* x, long long i) { return ((const double*)x)[i]; }
template <> __device__ __forceinline__ double lsh_load<float>(const void* x, long long i) { return (double)((const float*)x)[i]; }
template <> __device__ __forceinline__ double lsh_load<dlc_bf16_tag>(const void* x, long long i) {
    return (double)dlc_bf16_bits_to_f32(((const unsigned short*)x)[i]);
}

template <typename T>
__global__ __launch_bounds__(LSH_Q_THREADS) void lsh_quantize_kernel(const LshQuantArgs a) {
    __shared__ double s_max[LSH_Q_THREADS / 64];
    __shared__ int s_bad[LSH_Q_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = blockIdx.x, x0 = r * a.ldx;
    double m = 0.0;
    int bad = 0;
    for (long long d = tid; d < a.D; d += LSH_Q_THREADS) {
        const double v = lsh_load<T>(a.x, x0 + d);
        const double t = __builtin_fabs(a.mean ? v - a.mean[d] : v);
        bad |= (int)!(t <= 1.7976931348623157e308);            // NaN or inf
        m = t > m ? t : m;
    }
    for (int o = 32; o; o >>= 1) {
        const double other = __shfl_xor(m, o);
        m = other > m ? other : m;
        bad |= __shfl_xor(bad, o);
    }
    if (lane == 0) { s_max[wave] = m; s_bad[wave] = bad; }
    __syncthreads();
    for (int w = 0; w < LSH_Q_THREADS / 64; ++w) {
        m = s_max[w] > m ? s_max[w] : m;
        bad |= s_bad[w];
    }
    const bool zero = bad || m == 0.0;
    const double s = zero ? 0.0 : 127.0 / m;
    int8_t* q = a.q + r * a.ldq;
    for (long long d = tid; d < a.D; d += LSH_Q_THREADS) {
        int o = 0;
        if (!zero) {
            const double v = lsh_load<T>(a.x, x0 + d);
            const double t = a.mean ? v - a.mean[d] : v;
            double p = __builtin_rint(t * s);                  // ties to even
            p = p > 127.0 ? 127.0 : (p < -127.0 ? -127.0 : p); // (only where 127 / m overflowed)
            o = t == 0.0 ? 0 : (int)p;
        }
        q[d] = (int8_t)o;
    }
}

struct LshArgs {
    const int8_t* q;
    const int8_t* planes;
    uint8_t* out;
    int* part;                                     // split: int32 [chunks][rows][bits128]
    long long rows, D, ldq, ldp, ld_out;
    int bits, bits128, chunks;                     // bits128 = 8 * row_bytes
};

// the first n (1..15) bytes at p, the rest 0: byte loads, so that nothing past them is read
__device__ __forceinline__ v4i lsh_load_tail(const int8_t* p, int n) {
    v4i v = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned w = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4 * j + b < n) w |= (unsigned)(uint8_t)p[4 * j + b] << (8 * b);
        v[j] = (int)w;
    }
    return v;
}

template <int WR, int WC, int MT, int NT, bool SPLIT>
__global__ __launch_bounds__(64 * WR * WC) void lsh_hash_kernel(const LshArgs a) {
    constexpr int ROWS = 16 * MT * WR, BITS = 16 * NT * WC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave / WC, wc = wave % WC;
    const int lr = lane & 15, lk = 16 * (lane >> 4);
    const long long row0 = (long long)blockIdx.x * ROWS + 16 * MT * wr;
    const int bit0 = blockIdx.y * BITS + 16 * NT * wc;
    const long long k_begin = SPLIT ? (long long)blockIdx.z * DLC_LSH_CHUNK : 0;
    const long long k_end = SPLIT ? (k_begin + DLC_LSH_CHUNK < a.D ? k_begin + DLC_LSH_CHUNK : a.D) : a.D;

    const int8_t* pa[MT];
    const int8_t* pb[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        long long r = row0 + 16 * m + lr;
        r = r < a.rows ? r : a.rows - 1;
        pa[m] = a.q + r * a.ldq + lk;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        int t = bit0 + 16 * n + lr;
        t = t < a.bits ? t : a.bits - 1;
        pb[n] = a.planes + (long long)t * a.ldp + lk;
    }
    v4i acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = v4i{0, 0, 0, 0};

    long long k = k_begin;
    for (; k + 64 <= k_end; k += 64) {
        v4i fa[MT], fb[NT];
#pragma unroll
        for (int m = 0; m < MT; ++m) fa[m] = *(const v4i*)(pa[m] + k);
#pragma unroll
        for (int n = 0; n < NT; ++n) fb[n] = *(const v4i*)(pb[n] + k);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
    if (k < k_end) {                                           // the last, partial k-step: this lane has `left` bytes of it
        const long long left = k_end - (k + lk);
        v4i fa[MT], fb[NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            fa[m] = left >= 16 ? *(const v4i*)(pa[m] + k) : (left > 0 ? lsh_load_tail(pa[m] + k, (int)left) : v4i{0, 0, 0, 0});
#pragma unroll
        for (int n = 0; n < NT; ++n)
            fb[n] = left >= 16 ? *(const v4i*)(pb[n] + k) : (left > 0 ? lsh_load_tail(pb[n] + k, (int)left) : v4i{0, 0, 0, 0});
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }

    // acc[m][n][reg] is S(row0 + 16 m + 4 (lane >> 4) + reg, bit0 + 16 n + (lane & 15))
    if (SPLIT) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long r = row0 + 16 * m + 4 * (lane >> 4) + reg;
                if (r < a.rows) {
                    int* p = a.part + ((long long)blockIdx.z * a.rows + r) * a.bits128 + bit0 + lr;
#pragma unroll
                    for (int n = 0; n < NT; ++n) p[16 * n] = acc[m][n][reg];
                }
            }
    } else {
        // one ballot is the 16-bit words of rows 4 g + reg, g = 0..3; lane 2 NT g + b (< 8 NT) stores byte b of row 4 g + reg
        const int g = (lane / (2 * NT)) & 3, b = lane % (2 * NT);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                unsigned long long w = 0ull;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const unsigned long long word = __ballot(acc[m][n][reg] > 0 && bit0 + 16 * n + lr < a.bits);
                    w |= ((word >> (16 * g)) & 0xffffull) << (16 * n);
                }
                const long long r = row0 + 16 * m + 4 * g + reg;
                if (lane < 8 * NT && r < a.rows) a.out[r * a.ld_out + (bit0 >> 3) + b] = (uint8_t)(w >> (8 * b));
            }
    }
}

// split: bit t of row r from its chunks' sums, one lane per bit, a wave per 64 bits of a row
__global__ __launch_bounds__(256) void lsh_finish_kernel(const LshArgs a) {
    const int lane = threadIdx.x & 63;
    const long long words = a.bits128 / 64, item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.rows * words) return;                        // (a whole wave: the ballot below is met by all its lanes)
    const long long r = item / words;
    const int t = (int)(item % words) * 64 + lane;
    int s = 0;
    for (int c = 0; c < a.chunks; ++c) s += a.part[((long long)c * a.rows + r) * a.bits128 + t];
    const unsigned long long word = __ballot(s > 0 && t < a.bits);
    if (lane < 8) a.out[r * a.ld_out + (t >> 6 << 3) + lane] = (uint8_t)(word >> (8 * lane));
}

int64_t lsh_row_bytes(int bits) { return bits < 1 || bits > DLC_LSH_MAX_BITS ? 0 : 16 * dlc::cdiv(bits, 128); }

bool lsh_shape_ok(int64_t rows, int64_t D, int bits) {
    return rows >= 1 && rows <= 0x7fffffffll && D >= 1 && D <= DLC_LSH_MAX_D && bits >= 1 && bits <= DLC_LSH_MAX_BITS;
}

// the plan a call runs, -1 for an unknown one or a SPLIT with too many rows
int lsh_plan(int64_t rows, int64_t D, int plan) { return dlc::split_plan(plan, rows, DLC_LSH_SPLIT_MAX_ROWS, D > DLC_LSH_CHUNK); }

size_t lsh_workspace(int64_t rows, int64_t D, int bits, int plan) {
    if (!lsh_shape_ok(rows, D, bits) || lsh_plan(rows, D, plan) != DLC_LSH_PLAN_SPLIT) return 0;
    return dlc::align_up((size_t)rows * (size_t)dlc::cdiv(D, DLC_LSH_CHUNK) * (size_t)lsh_row_bytes(bits) * 8 * 4, 256);
}

template <int WR, int WC, int MT, int NT>
int lsh_launch_tile(dlc_ctx* ctx, const LshArgs& a, bool split, hipStream_t st) {
    const dim3 grid((unsigned)dlc::cdiv(a.rows, 16 * MT * WR), (unsigned)(a.bits128 / (16 * NT * WC)), split ? (unsigned)a.chunks : 1u);
    if (split) hipLaunchKernelGGL((lsh_hash_kernel<WR, WC, MT, NT, true>), grid, dim3(64 * WR * WC), 0, st, a);
    else hipLaunchKernelGGL((lsh_hash_kernel<WR, WC, MT, NT, false>), grid, dim3(64 * WR * WC), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "lsh_hash_kernel");
    return DLC_OK;
}

// tiles (rows x bits of a workgroup): 16 x 64 up to 16 rows; 64 x 64 up to 64 rows, and beyond while 128 x 128 would not
// fill the chip; else 128 x 128
int lsh_launch(dlc_ctx* ctx, const LshArgs& a, bool split, hipStream_t st) {
    int rc;
    if (a.rows <= 16) rc = lsh_launch_tile<1, 4, 1, 1>(ctx, a, split, st);
    else if (a.rows <= 64 || dlc::cdiv(a.rows, 128) * (a.bits128 / 128) < LSH_FILL) rc = lsh_launch_tile<2, 2, 2, 2>(ctx, a, split, st);
    else rc = lsh_launch_tile<2, 2, 4, 4>(ctx, a, split, st);
    if (rc != DLC_OK || !split) return rc;
    const long long waves = a.rows * (a.bits128 / 64);
    hipLaunchKernelGGL(lsh_finish_kernel, dim3((unsigned)dlc::cdiv(waves, 4)), dim3(256), 0, st, a);
    DLC_LAUNCH_CHECK(ctx, "lsh_finish_kernel");
    return DLC_OK;
}

}  // namespace

extern "C" int64_t dlc_lsh_row_bytes(int bits) { return lsh_row_bytes(bits); }

extern "C" size_t dlc_lsh_hash_workspace_bytes(int64_t rows, int64_t D, int bits, int plan) {
    return lsh_workspace(rows, D, bits, plan);
}

extern "C" int dlc_lsh_quantize_i8(dlc_ctx* ctx, int x_dtype, const void* x, int64_t rows, int64_t D, int64_t ldx,
                                   const double* mean, int8_t* q, int64_t ldq, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!x || !q) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_quantize: null pointer");
    if (x_dtype != DLC_F64 && x_dtype != DLC_F32 && x_dtype != DLC_BF16)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_quantize: dtype %d is none of DLC_F64, DLC_F32, DLC_BF16", x_dtype);
    const size_t xe = x_dtype == DLC_F64 ? 8 : (x_dtype == DLC_F32 ? 4 : 2);
    if ((((uintptr_t)x) & (xe - 1)) || (((uintptr_t)mean) & 7))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_quantize: a pointer is not aligned to its element");
    if (rows < 1 || D < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_quantize: rows=%lld, D=%lld must be >= 1", (long long)rows, (long long)D);
    if (ldx < D || ldq < D)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_quantize: ldx=%lld or ldq=%lld < D=%lld", (long long)ldx, (long long)ldq, (long long)D);
    if (D > DLC_LSH_MAX_D || rows > 0x7fffffffll)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "lsh_quantize: D=%lld > %d or rows=%lld >= 2^31", (long long)D, DLC_LSH_MAX_D, (long long)rows);
    const size_t q_bytes = (size_t)((rows - 1) * ldq + D);
    if (dlc::overlap(q, q_bytes, x, (size_t)((rows - 1) * ldx + D) * xe) || dlc::overlap(q, q_bytes, mean, (size_t)D * 8))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_quantize: q overlaps an input");
    DLC_ON_DEVICE(ctx);
    LshQuantArgs a;
    a.x = x; a.mean = mean; a.q = q; a.D = D; a.ldx = ldx; a.ldq = ldq;
    const dim3 grid((unsigned)rows), block(LSH_Q_THREADS);
    if (x_dtype == DLC_F64) hipLaunchKernelGGL(lsh_quantize_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
    else if (x_dtype == DLC_F32) hipLaunchKernelGGL(lsh_quantize_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(lsh_quantize_kernel<dlc_bf16_tag>, grid, block, 0, (hipStream_t)stream, a);
    DLC_LAUNCH_CHECK(ctx, "lsh_quantize_kernel");
    return DLC_OK;
}

extern "C" int dlc_lsh_hash_i8(dlc_ctx* ctx, const int8_t* q, int64_t rows, int64_t D, int64_t ldq, const int8_t* planes,
                               int bits, int64_t ldp, uint8_t* out, int64_t ld_out, int plan, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!ctx) return DLC_ERR_BAD_ARG;
    if (!q || !planes || !out) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: null pointer");
    if ((((uintptr_t)q) | ((uintptr_t)planes)) & 15)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: q and planes must be 16-byte aligned");
    if (rows < 1 || D < 1 || bits < 1)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: rows=%lld, D=%lld, bits=%d must be >= 1", (long long)rows, (long long)D, bits);
    if (ldq < D || ldp < D || (ldq & 15) || (ldp & 15))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: ldq=%lld and ldp=%lld must be multiples of 16 and >= D=%lld", (long long)ldq,
                         (long long)ldp, (long long)D);
    if (plan != DLC_LSH_PLAN_AUTO && plan != DLC_LSH_PLAN_ONE_PASS && plan != DLC_LSH_PLAN_SPLIT)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: unknown plan %d", plan);
    if (!lsh_shape_ok(rows, D, bits))
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "lsh_hash: D=%lld > %d, bits=%d > %d or rows=%lld >= 2^31", (long long)D, DLC_LSH_MAX_D,
                         bits, DLC_LSH_MAX_BITS, (long long)rows);
    const int64_t row_bytes = lsh_row_bytes(bits);
    if (ld_out < row_bytes)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: ld_out=%lld < row bytes=%lld", (long long)ld_out, (long long)row_bytes);
    const int run = lsh_plan(rows, D, plan);
    if (run < 0)
        return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "lsh_hash: DLC_LSH_PLAN_SPLIT takes at most %d rows, not %lld", DLC_LSH_SPLIT_MAX_ROWS,
                         (long long)rows);
    const size_t out_bytes = (size_t)((rows - 1) * ld_out + row_bytes);
    if (dlc::overlap(out, out_bytes, q, (size_t)((rows - 1) * ldq + D)) ||
        dlc::overlap(out, out_bytes, planes, (size_t)((int64_t)(bits - 1) * ldp + D)))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "lsh_hash: out overlaps an input");
    const bool split = run == DLC_LSH_PLAN_SPLIT;
    const size_t need = lsh_workspace(rows, D, bits, run);
    if (split) {
        const int rc = dlc::check_workspace(ctx, "lsh_hash", workspace, workspace_bytes, need);
        if (rc != DLC_OK) return rc;
    }
    DLC_ON_DEVICE(ctx);
    LshArgs a;
    a.q = q; a.planes = planes; a.out = out; a.part = split ? (int*)workspace : nullptr;
    a.rows = rows; a.D = D; a.ldq = ldq; a.ldp = ldp; a.ld_out = ld_out;
    a.bits = bits; a.bits128 = (int)(8 * row_bytes); a.chunks = (int)dlc::cdiv(D, DLC_LSH_CHUNK);
    return lsh_launch(ctx, a, split, (hipStream_t)stream);
}
