// The two hand-written statements of the matrix-core kernels (mlp_ro.hpp, wgrad_rows.hip): global memory -> LDS by
// LDS-DMA, and the MFMA that updates its accumulator in place.
#pragma once
#include "trs_common.hpp"

namespace trs {

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}

// one 1 KB piece (16 bytes per lane) from global memory (uniform ``src`` + this lane's ``voff``) straight into LDS at the
// wave-uniform address ``lds_dst``.  M0 belongs to the compiler: saved and restored inside the statement.
__device__ __forceinline__ void lds_dma1(const char* src, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(dst), "s"(src) : "memory");
}

// the same as a buffer operation (offsets past the end read nothing)
__device__ __forceinline__ void lds_dma1_buf(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(dst), "s"(rs) : "memory");
}

// acc += A B (16x16x32 bf16: Acc = 4 floats, Frag = 8 bf16), accumulator pinned to the accumulation registers (AG) or
// the vector registers and updated in place.  Written as an asm statement because with 49 tiles per wave hipcc
// otherwise gives the result a different register from the addend and moves 196 values back every iteration (3.7
// register moves per MFMA).  The compiler still tracks the operands (it waits for the LDS reads that feed A and B); what
// it cannot know is that the statement is an MFMA: the accumulators are read only after the loop, behind explicit wait
// states.
template <bool AG = true, typename Acc, typename Frag>
__device__ __forceinline__ void mfma_inplace(Acc& acc, const Frag& A, const Frag& B) {
  if constexpr (AG) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(A), "v"(B));
  else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(A), "v"(B));
}

}  // namespace trs
