// lds_dma.h -- device helpers shared by the kernels that stream 64-channel tiles HBM/L2 -> LDS by LDS-DMA and read their MFMA
// fragments back through hand-counted inline asm (conv_nt_bf16.hip, output_softmax_bf16.hip).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void glds16(const __bf16* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const SL_GLOBAL void*)gsrc, (SL_LDS void*)lds_wave_base, 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS fragment reads the compiler does not track (it answers every LDS dependency in these kernels with lgkmcnt(0),
// because the LDS-DMA loads leave a "flat access pending" mark): the hand-counted wait below releases the registers.
template <int OFF>
__device__ __forceinline__ void ds_read128(bf16x8& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <int I, int N, int STRIDE>
struct DsReadRun {
    static __device__ __forceinline__ void go(bf16x8 (&f)[N], unsigned addr) {
        ds_read128<I * STRIDE>(f[I], addr);
        DsReadRun<I + 1, N, STRIDE>::go(f, addr);
    }
};
template <int N, int STRIDE>
struct DsReadRun<N, N, STRIDE> {
    static __device__ __forceinline__ void go(bf16x8 (&)[N], unsigned) {}
};
// s_waitcnt lgkmcnt(CNT) that the MFMAs consuming these fragments cannot be hoisted above
template <int CNT>
__device__ __forceinline__ void wait_frags(bf16x8 (&a)[4], bf16x8 (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
                 : "n"(CNT));
}
template <int CNT>
__device__ __forceinline__ void wait_frags(bf16x8 (&a)[4], bf16x8 (&b)[8]) {
    asm volatile("s_waitcnt lgkmcnt(%12)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                   "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7])
                 : "n"(CNT));
}
template <int CNT>
__device__ __forceinline__ void wait_frags(bf16x8 (&a)[4], bf16x8 (&b)[2]) {
    asm volatile("s_waitcnt lgkmcnt(%6)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1])
                 : "n"(CNT));
}
__device__ __forceinline__ float bf16_lo(unsigned int u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned int u) { return __uint_as_float(u & 0xFFFF0000u); }

}  // namespace
