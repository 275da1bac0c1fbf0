// Stand-in for csrc/dlc_internal.h + the HIP runtime, for contrast_rows.hip compiled as host C++ (driver.cpp): a launch
// runs the kernel thread by thread.  __syncthreads() is nothing; instead every workgroup runs THREE times, all threads one
// after the other each time -- a wave's LDS rows are complete after the first pass (staging), its results after the second,
// and the third stores them; what the earlier passes stored to the offered cells is overwritten.  This holds while a
// workgroup takes one item per wave (grids of up to 2^20 workgroups: every shape of the driver).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <functional>
#define DLC_OK 0
#define DLC_ERR_BAD_ARG -1
#define DLC_ERR_BAD_SHAPE -2
#define DLC_ERR_HIP -4
#define DLC_ERR_WORKSPACE -5
enum { DLC_F32 = 2, DLC_F64 = 3, DLC_I64 = 6 };
struct dlc_ctx { int device; };
typedef void* hipStream_t;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct double2 { double x, y; } __attribute__((aligned(16)));
inline dim3 threadIdx, blockIdx, gridDim;
#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
inline void __syncthreads() {}
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
// what csrc/score_rows.h names beside the loader the kernel uses
inline long long __double_as_longlong(double v) { long long d; memcpy(&d, &v, 8); return d; }
inline unsigned long long dlc_f64_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
template <typename K, typename A> void emu_launch(K kern, dim3 grid, dim3 block, const A& a) {
    gridDim = grid;
    for (unsigned b = 0; b < grid.x; ++b)
        for (int pass = 0; pass < 3; ++pass)
            for (unsigned t = 0; t < block.x; ++t) { blockIdx = dim3(b); threadIdx = dim3(t); kern(a); }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, st, a) emu_launch(kern, grid, block, a)
#define DLC_LAUNCH_CHECK(ctx, what)
namespace dlc {
inline int fail(dlc_ctx*, int status, const char*, ...) { return status; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t row_limit(int64_t r, int64_t n, int64_t limit0, int64_t limit_step) {
    const int64_t l = limit0 + r * limit_step;
    return l < 0 ? 0 : (l > n ? n : l);
}
inline int64_t max_row_limit(int64_t r_first, int64_t r_last, int64_t n, int64_t limit0, int64_t limit_step) {
    const int64_t la = row_limit(r_first, n, limit0, limit_step), lb = row_limit(r_last, n, limit0, limit_step);
    return la > lb ? la : lb;
}
struct DeviceGuard { bool ok = true; explicit DeviceGuard(int) {} };
}
