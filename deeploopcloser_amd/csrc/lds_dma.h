// LDS-DMA primitives (global_load_lds_dwordx4, buffer_load_dwordx4 ... offen lds) and the waits that go with them, for
// the kernels that feed LDS by DMA: gemm_dma_f64.hip, cosine_topk.hip, gemm_split_f16.hip, gram_i8.hip, match_ref.hip.
// Device code only (dlc_internal.h does not include it: contrast_rows.hip is also compiled as host C++).
//
// THE PROTOCOL.  A piece is one wave-instruction: lane l's 16 bytes go to LDS at M0 + its `offset:` + 16 * l, 1 KiB per piece.
//  1. Inline asm, so that hipcc does not COUNT the piece in vmcnt: a load it counts makes it wait for vmcnt(0) in front
//     of every LDS read, which serialises a ring.  What hipcc does not count it does not wait for either -- see 6.
//  2. M0 carries the wave-uniform LDS destination and belongs to the compiler, which does not preserve it around a
//     statement.  M0 is therefore written in the SAME statement that uses it, in one of two ways:
//       save / restore -- s_mov_b32 keep, m0 ... s_mov_b32 m0, keep around the pieces (`keep`: an early-clobber "=&s"
//         output, written before the inputs are read).  Every form here but one.
//       clobber -- "m0" in the clobber list and no save (dma1_s_m0clobber).  hipcc answers with a -Winline-asm warning
//         that it may not honour the clobber, so the BUILD checks what the claim rests on: check_m0.py disassembles the
//         one kernel that uses the form (gram_i8_kernel) and fails if any instruction but the pieces' own
//         `s_mov_b32 m0, ...` (each followed by s_nop + global_load_lds) names M0.  A second kernel that wants this form
//         needs the same check.
//  3. s_nop 0 between a write of M0 (s_mov_b32 / s_add_u32) and the DMA that reads it: one wait state, which hipcc pads
//     in its own code and never inside a string.
//  4. s_nop 4 OPENS the statement: an SGPR that a VALU instruction (v_readfirstlane) has just written must be five wait
//     states old before a global_* / buffer_* reads it as base or descriptor, and hipcc pads nothing between its
//     readfirstlane and the string.  (The s_mov_b32 m0, lds of the same register is an SALU read and needs none.)
//     The pad may be omitted ONLY where the base or descriptor is provably not the result of a VALU write within five
//     wait states of the first DMA -- it comes from scalar arithmetic or a kernel argument, or enough instructions lie
//     between.  The source cannot promise that (hipcc decides whether a readfirstlane survives), so a form without the
//     pad states the precondition where it is defined and is re-checked in the kernel's assembly when its caller changes.
//  5. "scc" in the clobber list is for the instructions inside that write SCC: the s_add_u32 that steps M0 from piece to
//     piece, the s_cmp of the in-statement skip.
//  6. Completion is counted by hand: vmcnt counts a wave's pieces in issue order, so the wave waits with its OWN
//     DLC_WAIT_VMCNT(N) (N = pieces it may leave in flight), then the workgroup meets at wg_barrier(), the raw
//     s_barrier, and only behind it anybody reads the data.  Not __syncthreads() with a piece in flight: its fence
//     waits for what hipcc counts, which neither completes a piece nor promises to leave one in flight.  (The loop of
//     match_ref.hip keeps its __syncthreads() behind its own wait; hipcc emits a bare s_barrier for it there.)
//     A kernel ends with DLC_WAIT_VMCNT(0): no piece may outlive the workgroup's LDS.
//  7. Swizzles are applied on the SOURCE side: the LDS destination of a piece is lane-linear (M0 + 16 * lane, fixed by
//     the instruction), so a bank swizzle is a permutation of which 16 bytes each lane FETCHES.
// glds16 below is the other, COUNTED form (the builtin): for a load hipcc should wait for by itself.
#pragma once

namespace {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;          // (unsigned)(unsigned long long)(lptr_t)smem: the LDS byte address
typedef __attribute__((address_space(3))) const char* lcptr_t;

// "s" operands must BE in SGPRs: hipcc does not move a value it keeps in VGPRs there by itself (a diagnostic build
// failed to assemble that way), so the wave-uniform bases go through readfirstlane -- a no-op on a value that is
// already scalar.
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return (const char*)(((unsigned long long)hi << 32) | lo);       // (unsigned halves: the builtin returns int)
}

// The counted form: one 16-byte LDS-DMA load per lane through the builtin, which hipcc tracks in vmcnt like any load.
__device__ __forceinline__ void glds16(const char* g, char* l) {
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}

// ---- the save / restore statements: 1, 2 or 4 pieces, 1 KiB apart in LDS, in three addressing forms ----------------
#define DLC_DMA_PAD "s_nop 4\n\t"
#define DLC_DMA_NOPAD ""
#define DLC_DMA_HEAD "s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[lds]\n\ts_nop 0\n\t"
#define DLC_DMA_STEP(I) "s_add_u32 m0, %[lds], " #I "\n\ts_nop 0\n\t"
#define DLC_DMA_TAIL "s_mov_b32 m0, %[keep]"
// piece J by addressing form; POLICY: a cache-policy suffix such as " nt", or ""
#define DLC_DMA_PIECE_V(J, POLICY) "global_load_lds_dwordx4 %[o" #J "], off" POLICY "\n\t"                 // 64-bit address per lane
#define DLC_DMA_PIECE_S(J, POLICY) "global_load_lds_dwordx4 %[o" #J "], %[base]" POLICY "\n\t"             // SGPR base + 32-bit lane offset
#define DLC_DMA_PIECE_B(J, POLICY) "buffer_load_dwordx4 %[o" #J "], %[base], 0 offen lds" POLICY "\n\t"    // buffer descriptor + lane offset
#define DLC_DMA_SEQ1(PAD, P, POLICY) PAD DLC_DMA_HEAD P(0, POLICY) DLC_DMA_TAIL
#define DLC_DMA_SEQ2(PAD, P, POLICY) PAD DLC_DMA_HEAD P(0, POLICY) DLC_DMA_STEP(0x400) P(1, POLICY) DLC_DMA_TAIL
#define DLC_DMA_SEQ4(PAD, P, POLICY) \
    PAD DLC_DMA_HEAD P(0, POLICY) DLC_DMA_STEP(0x400) P(1, POLICY) DLC_DMA_STEP(0x800) P(2, POLICY) DLC_DMA_STEP(0xc00) P(3, POLICY) DLC_DMA_TAIL
#define DLC_DMA_SRC1 [o0] "v"(src[0])
#define DLC_DMA_SRC2 DLC_DMA_SRC1, [o1] "v"(src[1])
#define DLC_DMA_SRC4 DLC_DMA_SRC2, [o2] "v"(src[2]), [o3] "v"(src[3])
#define DLC_DMA_BASE() [base] "s"(base),       // (function-like: handed on by name, expanded in the statement)
#define DLC_DMA_NOBASE()
// One statement of N pieces.  It CAPTURES, by name, variables of the function it is expanded in: src[N] (the pieces'
// addresses or offsets), lds, keep (an uninitialised unsigned) and, where BASE is DLC_DMA_BASE, base; DLC_DMA_BODY also
// uses that function's template parameter N.
#define DLC_DMA_STMT(N, PAD, P, POLICY, BASE) \
    asm volatile(DLC_DMA_SEQ##N(PAD, P, POLICY) : [keep] "=&s"(keep) : DLC_DMA_SRC##N, BASE() [lds] "s"(lds) : "memory", "scc")
#define DLC_DMA_BODY(PAD, P, POLICY, BASE)                                       \
    static_assert(N == 1 || N == 2 || N == 4, "1, 2 or 4 pieces");               \
    unsigned keep;                                                               \
    if constexpr (N == 4) DLC_DMA_STMT(4, PAD, P, POLICY, BASE);                 \
    else if constexpr (N == 2) DLC_DMA_STMT(2, PAD, P, POLICY, BASE);            \
    else DLC_DMA_STMT(1, PAD, P, POLICY, BASE)

// src[j]: each lane's 64-bit source address of piece j
template <int N>
__device__ __forceinline__ void dma_v(const char* const (&src)[N], unsigned lds) {
    DLC_DMA_BODY(DLC_DMA_PAD, DLC_DMA_PIECE_V, "", DLC_DMA_NOBASE);
}
// The same with a wave-uniform 64-bit base in SGPRs and 32-bit per-lane byte offsets src[j].  NAME: dma_s, or a second
// instance of it under a cache policy (the cosine score kernel's database stream).
#define DLC_DMA_S_FORM(NAME, POLICY)                                                                        \
    template <int N>                                                                                        \
    __device__ __forceinline__ void NAME(const unsigned (&src)[N], const char* base, unsigned lds) {        \
        DLC_DMA_BODY(DLC_DMA_PAD, DLC_DMA_PIECE_S, POLICY, DLC_DMA_BASE);                                   \
    }
DLC_DMA_S_FORM(dma_s, "")
// One piece of that form WITHOUT the opening pad (rule 4).  PRECONDITION: `base` is not the result of a VALU write
// (v_readfirstlane) within five wait states of the DMA.  Its one caller, distinctive_score_dma_kernel, relies on hipcc
// folding uniform_ptr's readfirstlane away (the address is built from kernel arguments and blockIdx: scalar already);
// after a change to that caller or to the compiler, look at the kernel's assembly for what writes the base register.
// ("scc" is declared like in the other forms although this sequence writes no SCC: it changes no emitted instruction.)
__device__ __forceinline__ void dma1_s_nopad(unsigned off, const char* base, unsigned lds) {
    const unsigned src[1] = {off};
    unsigned keep;
    DLC_DMA_STMT(1, DLC_DMA_NOPAD, DLC_DMA_PIECE_S, "", DLC_DMA_BASE);
}

// Buffer addressing: a wave-uniform raw-buffer descriptor + per-lane 32-bit offsets src[j]; an offset at or past
// num_records (DMA_OOB) fetches nothing and its LDS slot receives zeros (gemm_dma_f64.hip uses that, and says more).
typedef __attribute__((ext_vector_type(4))) unsigned rsrc_t;
constexpr unsigned DMA_OOB = 0xfffffff0u;       // >= num_records of every descriptor built here
constexpr unsigned DMA_NUM_RECORDS = 0x80000000u;
__device__ __forceinline__ rsrc_t make_rsrc(const char* base) {
    const unsigned long long a = (unsigned long long)base;
    rsrc_t r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);       // stride 0: raw buffer
    r[2] = DMA_NUM_RECORDS;
    r[3] = 0x00020000u;                         // gfx9 raw-buffer word (32-bit data format)
    return r;
}
template <int N>
__device__ __forceinline__ void dma_b(const unsigned (&src)[N], rsrc_t base, unsigned lds) {
    DLC_DMA_BODY(DLC_DMA_PAD, DLC_DMA_PIECE_B, "", DLC_DMA_BASE);
}

// ---- two sequences of their own ------------------------------------------------------------------------------------
// A 4 KiB RUN in one statement, SKIPPED by a wave whose `on` is 0.  The instruction's immediate offset is added to the
// global address AND to the LDS address (M0 + offset + 16 * lane), and a run is laid out alike on both sides: one
// address register and one M0 value serve every piece of it.  The jump is inside the statement, so that the compiler
// sees straight-line code (gemm_split_f16.hip says what a C-level `if` cost there).
__device__ __forceinline__ void dma_run4_if(unsigned on, unsigned voff, const char* sbase, unsigned lds0) {
    unsigned keep;
    asm volatile(
        "s_cmp_eq_u32 %4, 0\n\t"
        "s_cbranch_scc1 .Lsp_skip_%=\n\t"
        "s_nop 4\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
        "s_mov_b32 m0, %0\n"
        ".Lsp_skip_%=:"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds0), "s"(on)
        : "memory", "scc");
}
// One piece in the CLOBBER form of rule 2 (three instructions, not five), and without the opening pad (rule 4).  Only for
// a kernel that check_m0.py checks.  PRECONDITION: `src` is not the result of a VALU write (v_readfirstlane) within
// five wait states of the DMA.  gram_i8_kernel sets its bases up once, far in front of the first piece; after a change
// to it or to the compiler, look at the kernel's assembly for what writes the base registers.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma1_s_m0clobber(unsigned voff, const char* src, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(src), "s"(lds) : "memory", "m0");
}
#pragma clang diagnostic pop

// ---- completion (rule 6) -------------------------------------------------------------------------------------------
#define DLC_WAIT_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(n) : "memory")
#define DLC_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
__device__ __forceinline__ void wg_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace
