// What the two sequence searches share (sequence.hip, sequence_elastic.hip): the entry's words and the merge of a row's
// per-slab lists into its k best, decoded.  An entry is (KEY, TAG) as sequence.hip describes it; the tag's low word is the
// winning slope there and the chain's span in the elastic search.
#pragma once
#include "topk_list.h"

namespace {

constexpr unsigned long long SQ_SIGN = 0x8000000000000000ull;
constexpr long long SQ_NAN_BITS = 0x7ff8000000000000ll;

template <int DT>
__device__ __forceinline__ unsigned long long sq_load_bits(const void* M, long long at) {
    if (DT == DLC_F64) return (unsigned long long)__double_as_longlong(((const double*)M)[at]);
    if (DT == DLC_F32) return (unsigned long long)__double_as_longlong((double)((const float*)M)[at]);
    return (unsigned long long)((const long long*)M)[at];
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
