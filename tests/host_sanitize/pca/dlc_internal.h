// Stand-in for csrc/dlc_internal.h + the HIP runtime, for pca.hip compiled as host C++ (driver.cpp).  The partial-sum
// kernel synchronises (barriers around the LDS slab of centred rows), so a launch runs every workgroup with
// ONE HOST THREAD PER GPU THREAD: __syncthreads() is a std::barrier over the workgroup; workgroups run one after the
// other.  "Device" memory is host memory, __shared__ a static: AddressSanitizer + UBSan see every access the kernel text
// makes.  Test infrastructure only.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <barrier>
#include <thread>
#include <vector>
#define DLC_OK 0
#define DLC_ERR_BAD_ARG -1
#define DLC_ERR_BAD_SHAPE -2
#define DLC_ERR_HIP -4
#define DLC_ERR_WORKSPACE -5
#define DLC_F32 2
#define DLC_F64 3
#define DLC_PCA_CHUNK 1024
#define DLC_PCA_MAX_COMPONENTS 8192
#define DLC_PCA_SPLIT_MAX_ROWS 64
enum { DLC_PCA_PLAN_AUTO = 0, DLC_PCA_PLAN_ONE_PASS = 1, DLC_PCA_PLAN_SPLIT = 2 };
struct dlc_ctx { int device; };
typedef void* hipStream_t;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
inline thread_local dim3 threadIdx, blockIdx;
inline dim3 gridDim;
#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
inline std::barrier<>* g_block;
inline void __syncthreads() { g_block->arrive_and_wait(); }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
template <typename K, typename A> void emu_launch(K kern, dim3 grid, dim3 block, const A& a) {
    gridDim = grid;
    std::barrier<> blk(block.x);
    g_block = &blk;
    // a block's threads run the grid-stride loop together; blocks one after the other
    for (unsigned b = 0; b < grid.x; ++b) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block.x; ++t) th.emplace_back([&, t, b] { blockIdx = dim3(b); threadIdx = dim3(t); kern(a); });
        for (auto& x : th) x.join();
    }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, st, a) emu_launch(kern, grid, block, a)
#define DLC_LAUNCH_CHECK(ctx, what)
namespace dlc {
inline int fail(dlc_ctx*, int status, const char*, ...) { return status; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct DeviceGuard { bool ok = true; explicit DeviceGuard(int) {} };
}
