// Stand-in for csrc/dlc_internal.h + the HIP runtime, for a kernel text of csrc/ compiled as host C++ (contrast/, fuse/,
// vlad/, pca/ driver.cpp; tests/host_kernel.py builds them).  Constants and prototypes are the library's own
// (include/dlc.h), and so are dlc::fail, the size and row-limit helpers and dlc_f64_key (csrc/dlc_hd.h): nothing of
// either is written again here.  A launch runs the kernel with ONE HOST THREAD PER GPU THREAD: __syncthreads() is a
// std::barrier over the workgroup, __shfl_xor an exchange through the wave's slots between two barriers of the wave.
// __shared__ is a static, so workgroups run one after the other: the threads start once per launch and walk the grid
// together, a block barrier between two workgroups.  "Device" memory is host memory: AddressSanitizer + UBSan see every
// access the kernel text makes.  Test infrastructure only.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <barrier>
#include <deque>
#include <thread>
#include <vector>

#include "../../include/dlc.h"

struct dlc_ctx { int device; char err[512]; };             // what dlc::fail formats into
typedef void* hipStream_t;
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
constexpr int hipDeviceAttributeMultiprocessorCount = 0;
inline hipError_t hipDeviceGetAttribute(int* v, int, int) { *v = 256; return hipSuccess; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct double2 { double x, y; } __attribute__((aligned(16)));
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
inline long long __double_as_longlong(double v) { long long d; memcpy(&d, &v, 8); return d; }

#include "dlc_hd.h"

namespace dlc {
struct DeviceGuard { bool ok = true; explicit DeviceGuard(int) {} };
}
#define DLC_ON_DEVICE(ctx)                                                                                         \
    dlc::DeviceGuard guard((ctx)->device);                                                                         \
    if (!guard.ok) return dlc::fail((ctx), DLC_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device)
#define DLC_LAUNCH_CHECK(ctx, what)
#define DLC_HIP_CHECK(ctx, expr)                                                                                   \
    do {                                                                                                           \
        if ((expr) != hipSuccess) return dlc::fail((ctx), DLC_ERR_HIP, "%s failed (%s:%d)", #expr, __FILE__, __LINE__); \
    } while (0)

#include "entry.h"

// ---- the launcher ------------------------------------------------------------------------------------------------------
namespace emu {
struct Wave {
    std::barrier<> bar;
    unsigned lanes;
    unsigned long long slot[64];
    explicit Wave(unsigned n) : bar(n), lanes(n) {}
};
inline std::barrier<>* block;                              // of the launch that is running
inline std::deque<Wave>* waves;
}  // namespace emu
inline thread_local dim3 threadIdx, blockIdx;
inline dim3 gridDim;
inline void __syncthreads() { emu::block->arrive_and_wait(); }
template <class T> inline T __shfl_xor(T v, int off) {
    static_assert(sizeof(T) <= 8, "");
    emu::Wave& w = (*emu::waves)[threadIdx.x >> 6];
    const unsigned lane = threadIdx.x & 63, from = lane ^ (unsigned)off;
    memcpy(&w.slot[lane], &v, sizeof(T));
    w.bar.arrive_and_wait();
    T r;
    memcpy(&r, &w.slot[from < w.lanes ? from : lane], sizeof(T));
    w.bar.arrive_and_wait();
    return r;
}
template <typename K, typename A> void emu_launch(K kern, dim3 grid, dim3 block, const A& a) {
    std::barrier<> blk(block.x);
    std::deque<emu::Wave> waves;                           // one per 64 threads of block.x, the last one may be short
    for (unsigned t = 0; t < block.x; t += 64) waves.emplace_back(block.x - t < 64 ? block.x - t : 64u);
    emu::block = &blk; emu::waves = &waves; gridDim = grid;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
        th.emplace_back([&, t] {
            threadIdx = dim3(t);
            for (unsigned b = 0; b < grid.x; ++b) {
                blockIdx = dim3(b);
                kern(a);
                blk.arrive_and_wait();                     // the statics of __shared__ are the next workgroup's from here
            }
        });
    for (auto& x : th) x.join();
}
#define hipLaunchKernelGGL(kern, grid, block, lds, st, a) emu_launch(kern, grid, block, a)
