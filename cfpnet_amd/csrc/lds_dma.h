// LDS-DMA (`global_load_lds_dwordx4`): 16 bytes per lane straight from global memory into LDS, lane l of the wave at lds_wave_base + 16 l,
// and the 16 zero bytes a lane reads instead when its source lies outside the tensor.
#pragma once
#include "common.h"

// one per translation unit (internal linkage)
static __device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};

using gptr_t = const __attribute__((address_space(1))) void*;
using lptr_t = __attribute__((address_space(3))) void*;

__device__ __forceinline__ void glds16(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)lds_wave_base, 16, 0, 0);
}

// counted wait: all but this wave's N youngest vector-memory operations (they complete in order) have landed
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ... before a stage of a STAGES-deep pipeline with LPS operations per stage is consumed: `ahead` (<= STAGES - 2) younger stages may stay in flight
template <int STAGES, int LPS> __device__ __forceinline__ void wait_stage(int ahead) {
  if (ahead >= 2) wait_vmcnt<(STAGES > 3 ? 2 : 1) * LPS>();
  else if (ahead == 1) wait_vmcnt<LPS>();
  else wait_vmcnt<0>();
}
