// Stand-in for csrc/dlc_internal.h + the HIP runtime, for fuse_rows.hip compiled as host C++ (driver.cpp).  The kernels
// synchronise (barriers between the sweeps and the LDS folds, shuffles inside a wave), so a launch runs every workgroup
// with ONE HOST THREAD PER GPU THREAD: __syncthreads() is a std::barrier over the workgroup, __shfl_xor an exchange
// through a table between two barriers of the wave; workgroups run one after the other.  "Device" memory is host memory,
// __shared__ a static: AddressSanitizer + UBSan see every access the kernel text makes.  Test infrastructure only.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <barrier>
#include <thread>
#include <vector>
#include <memory>
#define DLC_OK 0
#define DLC_ERR_BAD_ARG -1
#define DLC_ERR_BAD_SHAPE -2
#define DLC_ERR_HIP -4
#define DLC_ERR_WORKSPACE -5
#define DLC_MAX_FUSE 8
enum { DLC_FUSE_NONE = 0, DLC_FUSE_ZSCORE = 1, DLC_FUSE_MINMAX = 2 };
enum { DLC_FUSE_PLAN_AUTO = 0, DLC_FUSE_PLAN_ROW = 1, DLC_FUSE_PLAN_SLAB = 2 };
enum { DLC_F32 = 2, DLC_F64 = 3, DLC_I64 = 6 };
struct dlc_ctx { int device; };
typedef void* hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
constexpr int hipDeviceAttributeMultiprocessorCount = 0;
inline int hipDeviceGetAttribute(int* v, int, int) { *v = 256; return 0; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct double2 { double x, y; } __attribute__((aligned(16)));
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
inline thread_local dim3 threadIdx, blockIdx;
inline dim3 gridDim;
#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
inline std::barrier<>* g_block;
inline std::barrier<>* g_wave[4];
inline double g_slot[256];
inline void __syncthreads() { g_block->arrive_and_wait(); }
template <class T> inline T __shfl_xor(T v, int off) {
    static_assert(sizeof(T) <= 8, "");
    const int t = threadIdx.x, w = t >> 6;
    double d = 0; memcpy(&d, &v, sizeof(T));
    g_slot[t] = d; g_wave[w]->arrive_and_wait();
    double o = g_slot[(t & ~63) | ((t & 63) ^ off)];
    g_wave[w]->arrive_and_wait();
    T r; memcpy(&r, &o, sizeof(T)); return r;
}
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
inline long long __double_as_longlong(double v) { long long d; memcpy(&d, &v, 8); return d; }
inline unsigned long long dlc_f64_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
template <typename K, typename A> void emu_launch(K kern, dim3 grid, dim3 block, const A& a) {
    gridDim = grid;
    std::barrier<> blk(block.x), w0(64), w1(64), w2(64), w3(64);
    g_block = &blk; g_wave[0] = &w0; g_wave[1] = &w1; g_wave[2] = &w2; g_wave[3] = &w3;
    // a block's threads run the grid-stride loop together; blocks one after the other
    for (unsigned b = 0; b < grid.x; ++b) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block.x; ++t) th.emplace_back([&, t, b] { blockIdx = dim3(b); threadIdx = dim3(t); kern(a); });
        for (auto& x : th) x.join();
    }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, st, a) emu_launch(kern, grid, block, a)
#define DLC_LAUNCH_CHECK(ctx, what)
#define DLC_HIP_CHECK(ctx, expr) (void)(expr)
namespace dlc {
inline int fail(dlc_ctx*, int status, const char* f, ...) { return status; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
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
