// The hand-written gfx950 device primitives every kernel of libldn_hip.so shares: LDS-DMA issue, counted waits, the LDS barrier, the
// wave-uniform pointer, the bf16 hi / lo split and the vector typedefs.  ONE definition each: a new inline-asm primitive goes here, once
// (DESIGN.md 4).  Everything is __device__ __forceinline__, so a kernel's code is what it was when it carried its own copy.
// Tuning / ablation switches stay in the file that owns them, in a wrapper of a few lines around the primitive; this header knows none.
// Not here, because they are different operations and not further spellings of these: ldn_conv_image.hip's glds16 (the builtin form of the
// 16-byte LDS-DMA, which the compiler DOES count) and its block_sync (a barrier that also waits for vmcnt).
#pragma once
#include <hip/hip_runtime.h>

namespace ldn {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- LDS-DMA.  Inline asm: the compiler neither counts these loads nor waits for them (cdna_hip_programming.md 5.7) -- every wait is
// one of the explicit wait_vm forms below.  Each global_load_lds instruction adds ONE to the wave's vmcnt, whatever its width.  M0 (the
// LDS base of the instruction) is saved and restored around every issue: the compiler keeps values of its own there.

// 16 bytes per lane: LDS destination = lds_base + lane * 16, source = gsrc (per lane).  lds_base must be wave-uniform AND in a scalar
// register (a caller that holds it in a VGPR applies readfirstlane itself).  One vmcnt.
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_base) : "memory");
}
// L2 prefetch: 4 bytes per lane through the same path into a scratch word at lds_base + lane * 4 -- no VGPR result to keep alive, one
// vmcnt like every other DMA instruction.  What it buys is the LINE in the XCD's L2 ahead of the 16-byte DMA that fetches it for real.
__device__ __forceinline__ void dma4_touch(const void* gsrc, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_base) : "memory");
}
// NF (1..4) consecutive 1 KB pieces with ONE M0 set-up: piece f = sbase (wave-uniform, scalar registers: uniform_ptr) + vo[f] (per-lane
// byte offset) + f * 1024 -> LDS lds_base (wave-uniform, scalar) + f * 1024 + lane * 16.  The instruction offset of
// global_load_lds_dwordx4 moves the LDS destination as well as the global source (measured: tools/experiments/dma_offset.hip), so a
// caller whose pieces are NOT 1 KB apart in memory biases vo[f] with (3 - f) * 1024 against sbase - 3072.  NF vmcnt.
template <int NF> __device__ __forceinline__ void dma16_pieces(const unsigned (&vo)[4], const void* sbase, unsigned lds_base) {
    static_assert(NF >= 1 && NF <= 4, "1..4 pieces per M0 set-up");
    unsigned keep;
    if constexpr (NF == 1)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(vo[0]), "s"(sbase), "s"(lds_base) : "memory");
    else if constexpr (NF == 2)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\tglobal_load_lds_dwordx4 %2, %3 offset:1024\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(vo[0]), "v"(vo[1]), "s"(sbase), "s"(lds_base) : "memory");
    else if constexpr (NF == 3)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4\n\tglobal_load_lds_dwordx4 %2, %4 offset:1024\n\t"
                     "global_load_lds_dwordx4 %3, %4 offset:2048\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(vo[0]), "v"(vo[1]), "v"(vo[2]), "s"(sbase), "s"(lds_base) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\tglobal_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                     "global_load_lds_dwordx4 %3, %5 offset:2048\n\tglobal_load_lds_dwordx4 %4, %5 offset:3072\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(vo[0]), "v"(vo[1]), "v"(vo[2]), "v"(vo[3]), "s"(sbase), "s"(lds_base) : "memory");
}

// ---- waits.  vmcnt counts this WAVE's outstanding vector-memory instructions (LDS-DMA, and every global load the compiler issued:
// it returns in order, so "at most N outstanding" means "all but the youngest N have landed").  None of these is a barrier, and none
// waits for LDS traffic (lgkmcnt).

// at most N vector-memory instructions of this wave still in flight (compile-time N, 0..63: the counter has six bits)
template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt has six bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// The same with a run-time, wave-uniform count: exact for 0 <= n <= MAX_EXACT, and OTHER for every other n.  The two parameters ARE the
// caller's clamping rule; each caller names its own next to its instantiation.  OTHER < n over-waits (always safe), OTHER > n would
// under-wait: an instantiation with OTHER > MAX_EXACT says that its counts never exceed OTHER.  A literal switch of immediates (a jump
// table), because s_waitcnt takes no register operand.
template <int MAX_EXACT, int OTHER> __device__ __forceinline__ void wait_vm_rt(int n) {
    static_assert(MAX_EXACT >= 0 && MAX_EXACT <= 62 && OTHER >= 0 && OTHER <= 63, "vmcnt has six bits");
#define LDN_WV(N) case (N <= MAX_EXACT ? N : -1 - N): if constexpr (N <= MAX_EXACT && N != OTHER) { wait_vm<N>(); break; } else goto other;
    switch (n) {
        LDN_WV(0) LDN_WV(1) LDN_WV(2) LDN_WV(3) LDN_WV(4) LDN_WV(5) LDN_WV(6) LDN_WV(7) LDN_WV(8) LDN_WV(9) LDN_WV(10) LDN_WV(11) LDN_WV(12)
        LDN_WV(13) LDN_WV(14) LDN_WV(15) LDN_WV(16) LDN_WV(17) LDN_WV(18) LDN_WV(19) LDN_WV(20) LDN_WV(21) LDN_WV(22) LDN_WV(23) LDN_WV(24)
        LDN_WV(25) LDN_WV(26) LDN_WV(27) LDN_WV(28) LDN_WV(29) LDN_WV(30) LDN_WV(31) LDN_WV(32) LDN_WV(33) LDN_WV(34) LDN_WV(35) LDN_WV(36)
        LDN_WV(37) LDN_WV(38) LDN_WV(39) LDN_WV(40) LDN_WV(41) LDN_WV(42) LDN_WV(43) LDN_WV(44) LDN_WV(45) LDN_WV(46) LDN_WV(47) LDN_WV(48)
        LDN_WV(49) LDN_WV(50) LDN_WV(51) LDN_WV(52) LDN_WV(53) LDN_WV(54) LDN_WV(55) LDN_WV(56) LDN_WV(57) LDN_WV(58) LDN_WV(59) LDN_WV(60)
        LDN_WV(61) LDN_WV(62)
        default: other: wait_vm<OTHER>(); break;
    }
#undef LDN_WV
}
// this wave's LDS traffic (ds_read / ds_write, scalar loads) retired; no barrier, no vmcnt
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// LDS traffic of this wave retired, then the workgroup barrier, then a compiler fence.  Does NOT wait for vmcnt: an LDS-DMA in flight
// stays in flight across it (the point of the counted waits) -- a wave publishes landed DMA data with wait_vm BEFORE this barrier.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- addresses
// byte offset of an LDS pointer inside the workgroup's allocation (what M0 and the ds_ instructions of inline asm take)
__device__ __forceinline__ unsigned lds_off(const void* ptr) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)ptr;
}
// a 64-bit pointer that IS wave-uniform, moved into scalar registers (two readfirstlane): the "s" operands of the DMA forms above, and
// scalar loads through it.  The caller guarantees uniformity; a divergent pointer silently becomes its first active lane's.
template <typename T> __device__ __forceinline__ T uniform_ptr(T v) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return reinterpret_cast<T>(((unsigned long long)hi << 32) | lo);
}

// ---- the bf16x3 operand split: hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even
__device__ __forceinline__ void split2(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}
// eight consecutive elements (two fp32 quads) -> one MFMA operand of 8 hi and one of 8 lo.  V = how the quads are passed: by value unless
// the caller says otherwise.  ldn_conv_image.hip says split8<const f32x4&>, the form its kernels have always been compiled from: hipcc
// schedules the two forms differently around the call (docs/lab_notebook.md), and moving the definition here was not to change any kernel.
template <typename V> __device__ __forceinline__ void split8(const V a, const V b, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = e < 4 ? a[e] : b[e - 4];
        const __bf16 hb = (__bf16)v;
        hi[e] = hb;
        lo[e] = (__bf16)(v - (float)hb);
    }
}

// ---- cross-lane
// sum over the 16 lanes of a DPP row (inline asm: hipcc 7.2 merges neighbouring update_dpp calls, see dpp_swap_pair); fixed order
__device__ __forceinline__ float row16_sum(float v) {
    float t;
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1"
                 : "=&v"(t) : "v"(v));
    return t;
}

}  // namespace ldn
