// What the two sequence searches and their chains share (sequence.hip, sequence_elastic.hip, sequence_chains.hip): the
// entry's words, the offset table as the kernels take it, one level's addition of the elastic recursion, and the merge of a
// row's per-slab lists into its k best, decoded.  An entry is (KEY, TAG) as sequence.hip describes it; the tag's low word
// is the winning slope there and the chain's span in the elastic search.
#pragma once
#include "topk_list.h"

namespace {

constexpr unsigned long long SQ_SIGN = 0x8000000000000000ull;
constexpr long long SQ_NAN_BITS = 0x7ff8000000000000ll;
constexpr int SQ_MAX_L = 64, SQ_MAX_SLOPES = 16;
constexpr int EL_MAX_L = 64;

struct SqOffsets { short o[SQ_MAX_SLOPES * SQ_MAX_L]; };          // [slope][L], by value (2 KB of the kernel's arguments)

// The host table [n_slopes, L] checked and packed: rows start at 0, never decrease, stay within 0..32767.
inline int sq_pack_offsets(dlc_ctx* ctx, const char* who, const int32_t* offsets, int n_slopes, int L, SqOffsets* offs,
                           int* maxoff) {
    memset(offs, 0, sizeof(*offs));
    *maxoff = 0;
    for (int v = 0; v < n_slopes; ++v)
        for (int s = 0; s < L; ++s) {
            const int32_t o = offsets[(size_t)v * L + s];
            if (o < 0 || o > 32767 || (s == 0 && o != 0) || (s > 0 && o < offsets[(size_t)v * L + s - 1]))
                return dlc::fail(ctx, DLC_ERR_BAD_ARG,
                                 "%s: offsets[%d][%d]=%d (rows start at 0, never decrease, stay within 0..32767)", who, v, s,
                                 (int)o);
            offs->o[v * L + s] = (short)o;
            if (o > *maxoff) *maxoff = o;
        }
    return DLC_OK;
}

template <int DT>
__device__ __forceinline__ unsigned long long sq_load_bits(const void* M, long long at) {
    if (DT == DLC_F64) return (unsigned long long)__double_as_longlong(((const double*)M)[at]);
    if (DT == DLC_F32) return (unsigned long long)__double_as_longlong((double)((const float*)M)[at]);
    return (unsigned long long)((const long long*)M)[at];
}

// One level of the elastic recursion for one cell: the best predecessor's key (not read at the first level, t = 0) and
// the cell's element -> the cell's own key, in the order of merit (`flip` complements it when lower is better).  A NaN sum
// clears ok.  (sequence_elastic_scan_kernel spells the same lines out in its loop: docs/LAB.md 19.)
template <bool IS_INT>
__device__ __forceinline__ unsigned long long el_level_key(unsigned long long key, unsigned long long flip,
                                                           unsigned long long bits, int t, bool& ok) {
    if (IS_INT) {
        const unsigned long long sum = t > 0 ? ((key ^ flip) ^ SQ_SIGN) + bits : bits;
        key = (sum ^ SQ_SIGN) ^ flip;
    } else {
        const double x = __longlong_as_double((long long)bits);
        const double sum = t > 0 ? dlc_f64_unkey(key ^ flip) + x : x;
        ok = ok && sum == sum;
        key = dlc_f64_key(sum) ^ flip;
    }
    return key;
}

// One workgroup per output row: the k best of its G sorted lists, decoded.
template <bool IS_INT>
__global__ __launch_bounds__(256) void sequence_merge_kernel(const unsigned long long* __restrict__ part, int G, int k, int lower,
                                                             void* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                             int* __restrict__ out_slope, const long long* __restrict__ poison) {
    const long long q = blockIdx.x;
    if (poison && *poison != 0) {
        for (int t = threadIdx.x; t < k; t += 256) {
            ((double*)out_scores)[q * k + t] = __longlong_as_double(SQ_NAN_BITS);
            out_idx[q * k + t] = -1;
            if (out_slope) out_slope[q * k + t] = -1;
        }
        return;
    }
    tl_merge_slabs<TlPair>(part + (size_t)q * G * k * 2, G, k, [&](int i, TlPair m) {
        const bool none = m.is_empty();
        const unsigned long long k2 = lower ? ~m.key : m.key;
        if (IS_INT) ((long long*)out_scores)[q * k + i] = none ? -1ll : (long long)(k2 ^ SQ_SIGN);
        else ((double*)out_scores)[q * k + i] = none ? (lower ? INFINITY : -INFINITY) : dlc_f64_unkey(k2);
        out_idx[q * k + i] = none ? -1ll : (long long)(~(unsigned)(m.tag >> 32));
        if (out_slope) out_slope[q * k + i] = none ? -1 : (int)(m.tag & 0xffffffffull);
    });
}

}  // namespace
