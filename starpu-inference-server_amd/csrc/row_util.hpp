// Stateless helpers the HBM-bound kernel files (pool.hip, layernorm.hip, elementwise.hip, bert_pool.hip)
// share.  aligned() is plain C++ for the host-only translation units; the rest needs the HIP language.
#pragma once
#include <cstdint>

namespace spi {

// p is a multiple of `bytes` (a power of two).
inline bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace spi

#ifdef __HIP__
#include <algorithm>

#include "lds_dma.hpp"  // half4, half8

namespace spi {
namespace {

inline int grid_for(size_t n, int block = 256, int cap = 8192) {
  return (int)std::max<size_t>(1, std::min<size_t>((n + block - 1) / block, cap));
}

// f(T{}) with the compute type a launcher's f16 flag names, so that a launcher holds one launch per
// kernel: with_type(f16, [&](auto t) { using T = decltype(t); SPI_LAUNCH((kernel<T>), ...); }).
template <typename F>
inline void with_type(bool f16, F&& f) {
  if (f16)
    f(_Float16{});
  else
    f(float{});
}

template <typename T>
__device__ __forceinline__ T cvt(float v) { return static_cast<T>(v); }

__device__ __forceinline__ float wave_sum(float v) {  // xor butterfly: one order, every lane the total
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 4 fp32 values -> the i-th group of 4 T at p: one 8-byte (fp16) or 16-byte (fp32) store; p aligned to that.
template <typename T>
__device__ __forceinline__ void store4(T* p, const float (&v)[4], int i = 0) {
  if constexpr (sizeof(T) == 2)
    reinterpret_cast<half4*>(p)[i] = half4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  else
    reinterpret_cast<float4*>(p)[i] = float4{v[0], v[1], v[2], v[3]};
}

// 8 fp32 values -> T at p: one (fp16) or two (fp32) 16-byte stores; p 16-byte aligned.
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<half8*>(p) = half8{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                                         (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
  } else {
    reinterpret_cast<float4*>(p)[0] = float4{v[0], v[1], v[2], v[3]};
    reinterpret_cast<float4*>(p)[1] = float4{v[4], v[5], v[6], v[7]};
  }
}

}  // namespace
}  // namespace spi
#endif
