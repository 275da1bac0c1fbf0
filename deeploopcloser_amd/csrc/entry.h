// The rules of the C boundary that the entry points share, each written once: do an output and an input share a byte,
// is the workspace there, which of ONE_PASS / SPLIT a plan word runs, how many workgroups a launch of `items` items gets.
// (The device guard, DLC_ON_DEVICE, sits in dlc_internal.h beside DLC_LAUNCH_CHECK.)  Host code over dlc::fail,
// dlc::align_up and dlc::cdiv (dlc_hd.h) alone: no HIP name, so the host programs of tests/host_sanitize/ compile it as it
// is.  Whoever includes this file has included dlc_internal.h, or the stand-in for it.
#pragma once

static_assert(DLC_PCA_PLAN_AUTO == DLC_LSH_PLAN_AUTO && DLC_PCA_PLAN_ONE_PASS == DLC_LSH_PLAN_ONE_PASS &&
                  DLC_PCA_PLAN_SPLIT == DLC_LSH_PLAN_SPLIT,
              "dlc::split_plan speaks of one set of plan codes");

// more items than this: a workgroup takes several, one after the other
constexpr long long DLC_MAX_BLOCKS = 1 << 20;

namespace dlc {

// [p, p + bytes) and [q, q + bytes2) share a byte; a null q (an operand that was left out) shares none
inline bool overlap(const void* p, size_t bytes, const void* q, size_t bytes2) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return q && a < b + bytes2 && b < a + bytes;
}

// `need` bytes of workspace on a 16-byte boundary; need = 0 is the caller's "the sizes do not fit" (its _workspace_bytes)
inline bool workspace_ok(const void* workspace, size_t workspace_bytes, size_t need) {
    return need != 0 && workspace && workspace_bytes >= need && !(((uintptr_t)workspace) & 15);
}
inline int check_workspace(dlc_ctx* ctx, const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    if (workspace_ok(workspace, workspace_bytes, need)) return DLC_OK;
    return fail(ctx, DLC_ERR_WORKSPACE, "%s: needs %zu bytes of 16-byte aligned workspace", who, need);
}

// The plan a call runs, DLC_*_PLAN_ONE_PASS or DLC_*_PLAN_SPLIT: SPLIT takes at most max_rows rows, AUTO splits where
// it may and the caller's auto_split says it pays.  -1: a plan word that is unknown, or a SPLIT of too many rows.
inline int split_plan(int plan, int64_t rows, int64_t max_rows, bool auto_split) {
    if (plan == DLC_PCA_PLAN_ONE_PASS) return plan;
    if (plan == DLC_PCA_PLAN_SPLIT) return rows <= max_rows ? plan : -1;
    if (plan != DLC_PCA_PLAN_AUTO) return -1;
    return rows <= max_rows && auto_split ? DLC_PCA_PLAN_SPLIT : DLC_PCA_PLAN_ONE_PASS;
}

// the workgroups of a launch whose kernel walks `items` items with a grid stride
inline unsigned capped_blocks(long long items) { return (unsigned)(items < DLC_MAX_BLOCKS ? items : DLC_MAX_BLOCKS); }

}  // namespace dlc
