// The sorted list of a row's k <= 128 best entries in a wave's registers (sequence.hip; the distance scan keeps its own
// open-coded copy: docs/LAB.md 15) and the merge of a row's per-slab lists (distance_topk.hip, sequence.hip).
// An entry type E has empty() (every entry ranks before it), a.before(b), a.same(b), is_empty(), the wave shuffles per
// word, load_packed(p, i) (entry i of a slab's list in the workspace) and pick(c, a, b) = c ? a : b chosen word by word:
// entries travel by value, since a select between two entries as objects is one between addresses and costs scratch.
#pragma once
#include "dlc_internal.h"

namespace {

constexpr int TL_MAX_SLABS = 1024;         // lists a merge takes per row (its head[]): the cap on a scan's slabs per row tile

// One word, the smaller the better; ~0 is the empty slot.  (Merged only: it has no shfl / shfl_up.)
struct TlWord {
    unsigned long long v;
    static __device__ __forceinline__ TlWord empty() { return {~0ull}; }
    __device__ __forceinline__ bool before(TlWord o) const { return v < o.v; }
    __device__ __forceinline__ bool same(TlWord o) const { return v == o.v; }
    __device__ __forceinline__ bool is_empty() const { return v == ~0ull; }
    static __device__ __forceinline__ TlWord pick(bool c, TlWord a, TlWord b) { return {c ? a.v : b.v}; }
    __device__ __forceinline__ TlWord shfl_xor(int o) const { return {__shfl_xor(v, o)}; }
    static __device__ __forceinline__ TlWord load_packed(const unsigned long long* p, size_t i) { return {p[i]}; }
};

// (key, tag), the larger the better: by key, then by tag.  (0, 0) is the empty slot; an entry's tag is never 0.
struct TlPair {
    unsigned long long key, tag;
    static __device__ __forceinline__ TlPair empty() { return {0ull, 0ull}; }
    __device__ __forceinline__ bool before(TlPair o) const { return key > o.key || (key == o.key && tag > o.tag); }
    __device__ __forceinline__ bool same(TlPair o) const { return key == o.key && tag == o.tag; }
    __device__ __forceinline__ bool is_empty() const { return tag == 0ull; }
    static __device__ __forceinline__ TlPair pick(bool c, TlPair a, TlPair b) { return {c ? a.key : b.key, c ? a.tag : b.tag}; }
    __device__ __forceinline__ TlPair shfl(int lane) const { return {__shfl(key, lane), __shfl(tag, lane)}; }
    __device__ __forceinline__ TlPair shfl_up(int d) const { return {__shfl_up(key, d), __shfl_up(tag, d)}; }
    __device__ __forceinline__ TlPair shfl_xor(int o) const { return {__shfl_xor(key, o), __shfl_xor(tag, o)}; }
    static __device__ __forceinline__ TlPair load_packed(const unsigned long long* p, size_t i) { return {p[2 * i], p[2 * i + 1]}; }
};

// A list in a wave's registers while the wave inserts into it: E[i] = lane i's e0, E[64 + i] = lane i's e1, best first.
// Inserting x is E'[i] = E[i] before x ? E[i] : (E[i - 1] before x ? x : E[i - 1]) -- a shift by one lane, no serial chain
// through LDS.  kth is the list's last entry, in every lane: only an x before it changes the list.
template <class E>
struct WaveList {
    E e0, e1, kth;

    __device__ __forceinline__ void clear() { e0 = e1 = kth = E::empty(); }
    __device__ __forceinline__ void refresh(int k) { kth = k <= 64 ? e0.shfl((k - 1) & 63) : e1.shfl((k - 1) & 63); }
    template <class Get>
    __device__ __forceinline__ void load(int k, int lane, Get get) {          // get(i): entry i of the list where it is kept
        clear();
        if (lane < k) e0 = get(lane);
        if (lane + 64 < k) e1 = get(lane + 64);
        refresh(k);
    }
    __device__ __forceinline__ void insert(E x, int k, int lane) {          // (all three shuffles issued before any is used)
        const E p0 = e0.shfl_up(1);
        E p1 = e1.shfl_up(1);
        const E last0 = e0.shfl(63);
        if (lane == 0) p1 = last0;                                        // lane 0: e0's last entry wraps into e1
        if (!e1.before(x)) e1 = E::pick(p1.before(x), x, p1);
        if (!e0.before(x)) e0 = E::pick(lane == 0 || p0.before(x), x, p0);
        refresh(k);
    }
    template <class Put>
    __device__ __forceinline__ void store(int k, int lane, Put put) const {   // put(i, entry)
        if (lane < k) put(lane, e0);
        if (lane + 64 < k) put(lane + 64, e1);
    }
};

// One workgroup of 256 threads per row: k rounds of "best head of the row's G sorted lists" P[G][k] (packed entries),
// emit(i, entry) on thread 0 (the empty entry once the lists are exhausted).  A row's entries are distinct: one thread advances.
template <class E, class Emit>
__device__ __forceinline__ void tl_merge_slabs(const unsigned long long* __restrict__ P, int G, int k, Emit emit) {
    __shared__ int head[TL_MAX_SLABS];
    __shared__ E wbest[4];
    const int tid = threadIdx.x;
    for (int g = tid; g < G; g += 256) head[g] = 0;
    __syncthreads();
    int bg;
    auto local_best = [&]() {                             // of this thread's lists g = tid, tid + 256, ...; bg: whose head it is
        E b = E::empty();
        bg = -1;
        for (int g = tid; g < G; g += 256) {
            const int h = head[g];
            if (h < k) {
                const E v = E::load_packed(P, (size_t)g * k + h);
                if (v.before(b)) { b = v; bg = g; }
            }
        }
        return b;
    };
    E best = local_best();
    for (int i = 0; i < k; ++i) {
        E m = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const E o = m.shfl_xor(off);
            m = E::pick(o.before(m), o, m);
        }
        if ((tid & 63) == 0) wbest[tid >> 6] = m;
        __syncthreads();
        m = wbest[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = E::pick(wbest[w].before(m), wbest[w], m);
        __syncthreads();
        if (tid == 0) emit(i, m);
        if (!m.is_empty() && best.same(m)) {
            ++head[bg];
            best = local_best();
        }
    }
}

}  // namespace
