// Device helpers the kernel files share: the 16-byte vector types, the hand-counted LDS-DMA, its
// waits, and the swizzled read of the [row][RB-byte] tile images the DMA fills.
//
// The LDS-DMA contract.  glds16 / glds4 issue global_load_lds from inline asm, so the instruction is
// invisible to hipcc's waitcnt pass.  With the builtin, hipcc cannot tell a pending DMA from the LDS
// the next ds_reads touch (a destination addressed at run time may alias anything) and drains every
// DMA (s_waitcnt vmcnt(0)) before them -- which would serialise a prefetch with the k-loop it is meant
// to overlap.  So the caller counts its DMAs by hand: dma_wait_barrier<N> waits until at most N of
// this wave's are outstanding, and whoever reads the destination waits for it explicitly.  The
// destination goes through M0, which the asm saves and restores: hipcc does not know it changed
// (cdna_hip_programming.md 5.7, the M0-saving LDS-DMA recipe).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace spi {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// One 1-KiB piece: lane l's 16 bytes from `src` to dst + 16 l.
__device__ __forceinline__ void glds16(const void* src, const char* dst) {
  const lds_ptr_t lp = (lds_ptr_t)(const_cast<char*>(dst));
  const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lp);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(m0v)
               : "memory");
}

// The 4-byte form, a 256-byte piece: lane l's 4 bytes to dst + 4 l.
__device__ __forceinline__ void glds4(const void* src, const char* dst) {
  const lds_ptr_t lp = (lds_ptr_t)(const_cast<char*>(dst));
  const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lp);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(m0v)
               : "memory");
}

// Wait for this wave's LDS-DMA down to N outstanding, then barrier.  One asm statement with a
// memory clobber, so no LDS access moves across it (no __syncthreads(): its vmcnt(0) would drain
// the prefetch).
template <int N>
__device__ __forceinline__ void dma_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// The same for this wave's own LDS accesses.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Chunk c of image row `row`: rows of RB bytes, global chunk c at 16-byte slot c ^ (row & (RB / 16 - 1))
// (the XOR swizzle was applied on the DMA's source address).
template <int RB>
__device__ __forceinline__ u32x4 rd_chunk(const char* img, int row, int c) {
  constexpr int CPR = RB / 16;  // 16-byte chunks per image row
  return *reinterpret_cast<const u32x4*>(img + row * RB + ((c ^ (row & (CPR - 1))) << 4));
}

// f(integral_constant<int, T>) for T in [T, N): a loop whose index is a compile-time constant.
template <int T, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (T < N) {
    f(std::integral_constant<int, T>{});
    static_for<T + 1, N>(f);
  }
}

}  // namespace
}  // namespace spi
