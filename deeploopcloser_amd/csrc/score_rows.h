// The operand the score-row entry points share (the sequence searches and their chains, peak_rows.hip, evaluate.hip,
// contrast_rows.hip, fuse_rows.hip): a dense score matrix [rows, >= n] of DLC_F64, DLC_F32 or DLC_I64 with leading
// dimension ld, whose row r offers its first clamp(limit0 + r * limit_step, 0, n) cells (dlc::row_limit); an int64 matrix
// may name an `absent` value, a float one comes with a `poison` word.  Here: a cell as bits, as fp64 and as an ordered
// key; the operand's checks; the workspace check; the dtype as a compile-time constant.
#pragma once
#include <type_traits>

#include "dlc_internal.h"

namespace {

constexpr unsigned long long ROWS_SIGN = 0x8000000000000000ull;   // int64 -> a word whose unsigned order is the signed one
constexpr long long ROWS_NAN_BITS = 0x7ff8000000000000ll;         // the quiet NaN "not offered" is written as

// The cell at `at` as the 64 bits of its fp64 value (the conversion from fp32 is exact), or of the int64.
template <int DT>
__device__ __forceinline__ unsigned long long rows_bits(const void* M, long long at) {
    if (DT == DLC_F64) return (unsigned long long)__double_as_longlong(((const double*)M)[at]);
    if (DT == DLC_F32) return (unsigned long long)__double_as_longlong((double)((const float*)M)[at]);
    return (unsigned long long)((const long long*)M)[at];
}

template <int DT>
__device__ __forceinline__ double rows_f64(const void* M, long long at) {
    if (DT == DLC_F64) return ((const double*)M)[at];
    if (DT == DLC_F32) return (double)((const float*)M)[at];
    return (double)((const long long*)M)[at];                     // round to nearest even; exact below 2^53
}

// The key of the cell at `at` in the order of the numbers; false: the cell is not offered (a NaN, the absent value).
template <int DT>
__device__ __forceinline__ bool rows_key(const void* M, long long at, int has_absent, long long absent, unsigned long long& key) {
    if (DT == DLC_I64) {
        const long long v = ((const long long*)M)[at];
        key = (unsigned long long)v ^ ROWS_SIGN;
        return !(has_absent && v == absent);
    }
    const double v = DT == DLC_F64 ? ((const double*)M)[at] : (double)((const float*)M)[at];
    key = dlc_f64_key(v);
    return v == v;
}

// The operand as an entry point receives it; the kernels' argument structs are filled from it.
struct ScoreRows {
    int dtype;
    const void* M;
    int64_t rows, n, ld, limit0, limit_step;
    int lower, has_absent;
    int64_t absent;
};

// The fields every argument struct spells the same way.
template <class Args>
inline void rows_fill(Args& a, const ScoreRows& s) {
    a.M = s.M; a.n = s.n; a.ld = s.ld; a.limit0 = s.limit0; a.limit_step = s.limit_step;
}

// One matrix of an operand: its dtype, its pointer (set, aligned to its element), its rows at least n apart.
inline int rows_check_matrix(dlc_ctx* ctx, const char* who, int dtype, const void* M, int64_t ld, int64_t n) {
    if (dtype != DLC_F64 && dtype != DLC_F32 && dtype != DLC_I64)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: dtype must be DLC_F64, DLC_F32 or DLC_I64", who);
    if (!M || (((uintptr_t)M) & (dtype == DLC_F32 ? 3 : 7)))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: scores must be set and aligned to their element", who);
    if (ld < n) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: ld=%lld < n=%lld", who, (long long)ld, (long long)n);
    return DLC_OK;
}

// The operand's checks.  Everything answers DLC_ERR_BAD_ARG but n >= 2^31, the last one, which answers `too_wide`:
// DLC_ERR_BAD_ARG from the sequence family, DLC_ERR_BAD_SHAPE from the others (include/dlc.h).
inline int rows_check(dlc_ctx* ctx, const char* who, const ScoreRows& s, const void* poison, int too_wide) {
    if (s.rows < 1 || s.n < 1) return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: bad argument", who);
    const int rc = rows_check_matrix(ctx, who, s.dtype, s.M, s.ld, s.n);
    if (rc != DLC_OK) return rc;
    if (s.has_absent && s.dtype != DLC_I64)
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: an absent value is for DLC_I64; a float row marks absence with NaN", who);
    if (poison && (s.dtype == DLC_I64 || (((uintptr_t)poison) & 7)))
        return dlc::fail(ctx, DLC_ERR_BAD_ARG, "%s: the poison word marks fp64 outputs (DLC_I64 has none) and is aligned to 8 bytes", who);
    if (s.n > 0x7fffffffll) return dlc::fail(ctx, too_wide, "%s: n must be below 2^31", who);
    return DLC_OK;
}

// `need` bytes of 16-byte aligned workspace; need = 0 is the caller's "the sizes do not fit" (its _workspace_bytes).
inline int rows_check_workspace(dlc_ctx* ctx, const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    if (need == 0) return dlc::fail(ctx, DLC_ERR_BAD_SHAPE, "%s: rows * n too large", who);
    if (!dlc::workspace_ok(workspace, workspace_bytes, need))
        return dlc::fail(ctx, DLC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (or not 16-byte aligned)", who,
                         workspace ? workspace_bytes : (size_t)0, need);
    return DLC_OK;
}

// f(dt) with the dtype as a compile-time constant, dt.value; a dtype rows_check has passed.
template <class F>
inline auto rows_dispatch(int dtype, F&& f) {
    if (dtype == DLC_F64) return f(std::integral_constant<int, DLC_F64>{});
    if (dtype == DLC_F32) return f(std::integral_constant<int, DLC_F32>{});
    return f(std::integral_constant<int, DLC_I64>{});
}

}  // namespace
