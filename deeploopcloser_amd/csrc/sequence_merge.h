// What the two sequence searches and their chains share (sequence.hip, sequence_elastic.hip, sequence_chains.hip): the
// entry's words, the offset table as the kernels take it, one level's addition of the elastic recursion, and the merge of a
// row's per-slab lists into its k best, decoded, and the host front of the two searches.  An entry is (KEY, TAG) as sequence.hip describes it; the tag's low word
// is the winning slope there and the chain's span in the elastic search.
#pragma once
#include "score_rows.h"
#include "topk_list.h"

namespace {

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

// Cell `at` of the dense output: the score behind key k2 (in the order of the numbers), -1 / NaN where there is none.
// (sequence_scan_kernel spells the same two lines out: docs/LAB.md 26.)
template <bool IS_INT>
__device__ __forceinline__ void sq_store_dense(void* seq_out, long long at, bool have, unsigned long long k2) {
    if (IS_INT) ((long long*)seq_out)[at] = have ? (long long)(k2 ^ ROWS_SIGN) : -1ll;
    else ((double*)seq_out)[at] = have ? dlc_f64_unkey(k2) : __longlong_as_double(ROWS_NAN_BITS);
}

// One level of the elastic recursion for one cell: the best predecessor's key (not read at the first level, t = 0) and
// the cell's element -> the cell's own key, in the order of merit (`flip` complements it when lower is better).  A NaN sum
// clears ok.  (sequence_elastic_scan_kernel spells the same lines out in its loop: docs/LAB.md 19.)
template <bool IS_INT>
__device__ __forceinline__ unsigned long long el_level_key(unsigned long long key, unsigned long long flip,
                                                           unsigned long long bits, int t, bool& ok) {
    if (IS_INT) {
        const unsigned long long sum = t > 0 ? ((key ^ flip) ^ ROWS_SIGN) + bits : bits;
        key = (sum ^ ROWS_SIGN) ^ flip;
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
            ((double*)out_scores)[q * k + t] = __longlong_as_double(ROWS_NAN_BITS);
            out_idx[q * k + t] = -1;
            if (out_slope) out_slope[q * k + t] = -1;
        }
        return;
    }
    tl_merge_slabs<TlPair>(part + (size_t)q * G * k * 2, G, k, [&](int i, TlPair m) {
        const bool none = m.is_empty();
        const unsigned long long k2 = lower ? ~m.key : m.key;
        if (IS_INT) ((long long*)out_scores)[q * k + i] = none ? -1ll : (long long)(k2 ^ ROWS_SIGN);
        else ((double*)out_scores)[q * k + i] = none ? (lower ? INFINITY : -INFINITY) : dlc_f64_unkey(k2);
        out_idx[q * k + i] = none ? -1ll : (long long)(~(unsigned)(m.tag >> 32));
        if (out_slope) out_slope[q * k + i] = none ? -1 : (int)(m.tag & 0xffffffffull);
    });
}

// The host front of the two searches: the checks they share, the workspace (`need` bytes, looked at when there are lists)
// and the fields their argument structs share.  who: the caller's name in the messages.
template <class Args>
int sq_front(dlc_ctx* ctx, const char* who, const ScoreRows& s, int64_t row0, int L, int k, void* out_scores, int64_t* out_idx,
             int32_t* out_tag, void* seq_out, int64_t ld_out, const int64_t* poison, void* workspace, size_t workspace_bytes,
             size_t need, Args& a) {
    int rc = rows_check(ctx, who, s, poison, DLC_ERR_BAD_ARG);
    if (rc != DLC_OK) return rc;
    if (row0 < 0 || row0 >= s.rows) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: row0=%lld outside the rows", who, (long long)row0);
    const bool lists = out_scores != nullptr || out_idx != nullptr || out_tag != nullptr;
    if (lists && (!out_scores || !out_idx)) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: out_scores and out_idx come together", who);
    if (!lists && !seq_out) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: no output given", who);
    if (seq_out && ld_out < s.n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld_out < n", who);
    if (lists && (k < 1 || k > DLC_MAX_K)) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: k=%d outside 1..%d", who, k, DLC_MAX_K);
    if (lists && (rc = rows_check_workspace(ctx, who, workspace, workspace_bytes, need)) != DLC_OK) return rc;
    rows_fill(a, s);
    a.rows = s.rows; a.row0 = row0; a.ld_out = ld_out; a.part = lists ? (unsigned long long*)workspace : nullptr;
    a.seq_out = seq_out; a.poison = (const long long*)poison; a.L = L; a.lower = s.lower; a.k = lists ? k : 1;
    return DLC_OK;
}

// The merge behind a scan that kept lists (a.part): G slabs per row -> the k best, decoded.
template <class Args>
int sq_launch_merge(dlc_ctx* ctx, int dtype, const Args& a, int64_t G, void* out_scores, int64_t* out_idx, int32_t* out_tag,
                    hipStream_t st) {
    if (!a.part) return DLC_OK;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)(a.rows - a.row0)), dim3(256), 0, st, (const unsigned long long*)a.part, (int)G,
                           a.k, a.lower, out_scores, (long long*)out_idx, (int*)out_tag, a.poison);
    };
    if (dtype == DLC_I64) launch(sequence_merge_kernel<true>);
    else launch(sequence_merge_kernel<false>);
    DLC_LAUNCH_CHECK(ctx, "sequence_merge_kernel");
    return DLC_OK;
}

}  // namespace
