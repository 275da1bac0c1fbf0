// The TREE of include/dlc.h over values that sit in LDS, by a workgroup of THREADS threads (fuse_rows.hip: a row's chunk
// nodes; vlad.hip: a word's squared residuals).  Every aligned power-of-two block of a[] is a node of the tree, so
// callers that cut a long row into blocks of a power of two and fold the blocks' values the same way get the same bits.
#pragma once

// a[0 .. cnt) (written, not yet synchronised), padded with -0.0 to a power of two and folded neighbour with neighbour;
// the root, in every thread.  All threads of the workgroup call it; a[] is free again when it returns.
template <int THREADS>
__device__ __forceinline__ double dlc_lds_tree(double* a, int cnt) {
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int t = cnt + (int)threadIdx.x; t < P; t += THREADS) a[t] = -0.0;
    __syncthreads();
    for (int s = 1; s < P; s <<= 1) {
        for (int t = threadIdx.x; t < P / (2 * s); t += THREADS) a[2 * s * t] = a[2 * s * t] + a[2 * s * t + s];
        __syncthreads();
    }
    const double v = a[0];
    __syncthreads();                                                  // (a is free again)
    return v;
}
