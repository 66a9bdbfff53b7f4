// Diagnostic builds of gemm.hip (tools/build_variant.sh ... -DSPI_...): the macros the kernel body
// is written with, the device arrays the stamping builds fill and their extern "C" readers.  In the
// real build every macro is empty or the plain operation; the real kernel has none of this.
// Included by gemm.hip alone.
#pragma once
#include <hip/hip_runtime.h>

namespace spi {
namespace {

// -DSPI_GEMM_STAMPS: per-block s_memtime phase totals.
#ifdef SPI_GEMM_STAMPS
__device__ unsigned long long g_gemm_stamps[65536 * 8];
#define SPI_STAMP(v)                                                                         \
  do {                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");               \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  } while (0)
#else
#define SPI_STAMP(v) \
  do {               \
  } while (0)
#endif
// -DSPI_GEMM_TIMELINE: four s_memrealtime stamps per workgroup (entry, k-loop start, k-loop end,
// exit; 100 MHz) and the hardware ids (HW_ID: CU / SE; XCC_ID), so tools/gemm_timeline.py can split
// a launch into dispatch skew, prologue, loop and epilogue and see how workgroups pack onto CUs.
#ifdef SPI_GEMM_TIMELINE
__device__ unsigned long long g_gemm_timeline[65536 * 8];
// launches made by a thread inside spi_debug_gemm_timeline_enable(1) .. (0) carry KArgs::tl = 1
// (Model::profile_op on the repeated op), so other streams' launches never stamp
int& tl_thread() {
  static thread_local int on = 0;
  return on;
}
#define SPI_RT(v)                                                                  \
  do {                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                             \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                             \
  } while (0)
#else
#define SPI_RT(v) \
  do {            \
  } while (0)
#endif

// -DSPI_DIAG_NO_DMA issues no LDS-DMA (the tiles hold stale bytes), -DSPI_DIAG_NO_MFMA reads the
// fragments but issues no MFMA; timed against the real kernel (tools/ab_gemm.py) they split a launch
// into data movement and matrix work.  Outputs of both are meaningless.
#ifdef SPI_DIAG_NO_DMA
#define SPI_DMA(src, dst, sz, off, aux) \
  do {                                  \
    (void)(src);                        \
    (void)(dst);                        \
  } while (0)
#else
#define SPI_DMA(src, dst, sz, off, aux) __builtin_amdgcn_global_load_lds(src, dst, sz, off, aux)
#endif
// -DSPI_DIAG_L2A: every A-operand DMA reads from the first 64 KiB of A (same instruction count and
// addressing work, almost no L2-miss traffic); timed against the real kernel it separates
// memory-side traffic from the rest.
// -DSPI_DIAG_NO_DMA_A / _W: drop only the A-operand (incl. halo) or only the weight DMAs.
#ifdef SPI_DIAG_NO_DMA_A
#define SPI_DMA_A(src, dst, sz, off, aux) \
  do {                                    \
    (void)(src);                          \
    (void)(dst);                          \
  } while (0)
#else
#define SPI_DMA_A SPI_DMA
#endif
#ifdef SPI_DIAG_NO_DMA_W
#define SPI_DMA_W(src, dst, sz, off, aux) \
  do {                                    \
    (void)(src);                          \
    (void)(dst);                          \
  } while (0)
#else
#define SPI_DMA_W SPI_DMA
#endif
#ifdef SPI_DIAG_L2A
#define SPI_A_SRC(ptr_) \
  (reinterpret_cast<const char*>(a.p.A) + ((reinterpret_cast<const char*>(ptr_) - reinterpret_cast<const char*>(a.p.A)) & 0xFFF0))
#else
#define SPI_A_SRC(ptr_) (ptr_)
#endif

}  // namespace
}  // namespace spi

#ifdef SPI_GEMM_STAMPS
extern "C" int spi_debug_gemm_stamps(unsigned long long* host, size_t n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(spi::g_gemm_stamps), n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
#ifdef SPI_GEMM_TIMELINE
extern "C" int spi_debug_gemm_timeline(unsigned long long* host, size_t n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(spi::g_gemm_timeline), n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
extern "C" void spi_debug_gemm_timeline_enable(int on, hipStream_t) { spi::tl_thread() = on; }
extern "C" int spi_debug_gemm_timeline_clear(void) {
  static unsigned long long zeros[65536 * 8];
  return hipMemcpyToSymbol(HIP_SYMBOL(spi::g_gemm_timeline), zeros, sizeof(zeros)) == hipSuccess ? 0 : 1;
}
#endif
