// Elementwise and gather kernels around the MFMA contractions (gfx950): layout ingest, ViT
// patchify / assembly, row gather, the toy affine.  The pools are in pool.hip, the LayerNorm family
// and the BERT embedding in layernorm.hip.  16-byte loads / stores where the layout allows (G13).
#include "ln_fold.hpp"
#include "row_util.hpp"
#include "spi_kernels.hpp"

#include <stdexcept>
#include <string>

namespace spi {
namespace {

// Element (b, c, h, w) of an image of kind SRC ([B][C][H][W] fp32 / bytes, or [B][H][W][C] bytes),
// as the fp32 value that enters the network: an 8-bit pixel under the input transform
// (spi_kernels.hpp).  Byte loads: no alignment is assumed.
template <int SRC>
__device__ __forceinline__ float src_pixel(const void* __restrict__ x, const InputXf& xf, size_t b, int c, int C,
                                           size_t hw, size_t HW) {
  if constexpr (SRC == kSrcF32Nchw)
    return static_cast<const float*>(x)[(b * C + c) * HW + hw];
  else if constexpr (SRC == kSrcU8Nchw)
    return input_xf_apply(static_cast<const unsigned char*>(x)[(b * C + c) * HW + hw], xf, c);
  else
    return input_xf_apply(static_cast<const unsigned char*>(x)[(b * HW + hw) * C + c], xf, c);
}

// Image (NCHW fp32, or 8-bit pixels NCHW / NHWC) -> NHWC (T) with channel padding; one thread per pixel.
template <typename T, int SRC>
__global__ void ingest_kernel(const void* __restrict__ x, T* __restrict__ y, int B,
                              int C, int H, int W, int cpad, InputXf xf) {
  const size_t npix = (size_t)B * H * W;
  const size_t HW = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, hw = i - b * HW;
    T* dst = y + i * cpad;
    for (int c = 0; c < cpad; ++c)
      dst[c] = c < C ? cvt<T>(src_pixel<SRC>(x, xf, b, c, C, hw, HW)) : cvt<T>(0.f);
  }
}

// ViT patchify: row (b, ph, pw), column c*ps*ps + kh*ps + kw (conv weight flatten order).
template <typename T, int SRC>
__global__ void patchify_kernel(const void* __restrict__ x, T* __restrict__ y, int B,
                                int C, int H, int W, int ps, InputXf xf) {
  const int GH = H / ps, GW = W / ps;
  const int K = C * ps * ps;
  const size_t n = (size_t)B * GH * GW * K;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const size_t row = i / K;
    const int pw = (int)(row % GW);
    const int ph = (int)((row / GW) % GH);
    const int b = (int)(row / ((size_t)GW * GH));
    const int c = k / (ps * ps);
    const int kh = (k / ps) % ps, kw = k % ps;
    y[i] = cvt<T>(src_pixel<SRC>(x, xf, (size_t)b, c, C, (size_t)(ph * ps + kh) * W + pw * ps + kw, (size_t)H * W));
  }
}

// The vector forms' thread mapping: thread t holds the 8 consecutive kw from 8 seg of one (patch row,
// c, kh), so consecutive threads write consecutive 8-value chunks of y.  h, w0: the chunk's first
// pixel in image b; out: its offset in y.  32-bit index math (host-checked).
struct PatchChunk {
  int b, c, h, w0;
  size_t out;
};
__device__ __forceinline__ PatchChunk patch_chunk(int t, int C, int ps, int GH, int GW) {
  const int segs = ps >> 3;
  const int seg = t % segs;
  int r = t / segs;
  const int kh = r % ps;
  r /= ps;
  const int c = r % C;
  const int row = r / C;  // (b, ph, pw)
  const int pw = row % GW, ph = (row / GW) % GH, b = row / (GW * GH);
  return PatchChunk{b, c, ph * ps + kh, pw * ps + seg * 8, (size_t)row * (C * ps * ps) + (c * ps + kh) * ps + seg * 8};
}

// Vector form (round 6; ps % 8 == 0, W % 4 == 0, 16-byte aligned x / y): two 16-byte loads, one
// 16-byte (fp16) or two (fp32) stores per thread.
template <typename T>
__global__ __launch_bounds__(256) void patchify_vec_kernel(const float* __restrict__ x, T* __restrict__ y, int C,
                                                           int H, int W, int ps, int GH, int GW, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const PatchChunk p = patch_chunk(t, C, ps, GH, GW);
  const float4* src = reinterpret_cast<const float4*>(x + ((size_t)(p.b * C + p.c) * H + p.h) * W + p.w0);
  const float4 v0 = src[0], v1 = src[1];
  const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  store8(y + p.out, v);
}

// The vector form on 8-bit pixels (ps % 8 == 0, 16-byte aligned y; C = 3): the same thread mapping
// and 16-byte stores -- the stores are 2 or 4 times the bytes of the loads, so they are what the
// vector form is for.  WIDE (NCHW only; the host checks x % 8 == 0 and W % 8 == 0, which make every
// (b, c, row, pw ps + 8 seg) offset a multiple of 8): the 8 pixels as one 8-byte load.  Otherwise 8
// byte loads, 1 (NCHW) or 3 (NHWC) bytes apart, at any alignment.
template <typename T, int SRC, bool WIDE>
__global__ __launch_bounds__(256) void patchify_vec_u8_kernel(const unsigned char* __restrict__ x, T* __restrict__ y,
                                                              int H, int W, int ps, int GH, int GW, int n,
                                                              InputXf xf) {
  static_assert(SRC != kSrcF32Nchw && (!WIDE || SRC == kSrcU8Nchw), "8-bit sources; the wide load is NCHW's");
  constexpr int C = 3;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const PatchChunk p = patch_chunk(t, C, ps, GH, GW);
  unsigned char px[8];
  if constexpr (WIDE) {
    const uint2 raw = *reinterpret_cast<const uint2*>(x + ((size_t)(p.b * C + p.c) * H + p.h) * W + p.w0);
#pragma unroll
    for (int q = 0; q < 8; ++q) px[q] = (unsigned char)((q < 4 ? raw.x : raw.y) >> (8 * (q & 3)));
  } else {
    const unsigned char* src = SRC == kSrcU8Nhwc ? x + (((size_t)p.b * H + p.h) * W + p.w0) * C + p.c
                                                 : x + ((size_t)(p.b * C + p.c) * H + p.h) * W + p.w0;
#pragma unroll
    for (int q = 0; q < 8; ++q) px[q] = src[q * (SRC == kSrcU8Nhwc ? C : 1)];
  }
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = input_xf_apply(px[q], xf, p.c);
  store8(y + p.out, v);
}

__global__ void vit_assemble_kernel(const float* __restrict__ patches,
                                    const float* __restrict__ cls,
                                    const float* __restrict__ pos, float* __restrict__ x,
                                    int B, int P, int D) {
  const size_t n = (size_t)B * (P + 1) * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const size_t r = i / D;
    const int t = (int)(r % (P + 1));
    const int b = (int)(r / (P + 1));
    const float v = t == 0 ? cls[c] : patches[((size_t)b * P + (t - 1)) * D + c];
    x[i] = v + pos[(size_t)t * D + c];
  }
}

// ViT stream assembly into the two-plane residual stream (GemmDesc::res_planes) plus the rows'
// per-64-column chunk statistics (ln_fold.hpp) that the first layer's folded QKV GEMM reads: one
// thread per 8 columns of a row, 8 consecutive threads = one 64-column chunk (D % 64 == 0, so a
// chunk never straddles rows or 8-lane groups); 16-byte loads and stores.
__global__ __launch_bounds__(256) void vit_assemble_planes_kernel(const float* __restrict__ patches,
                                                                  const float* __restrict__ cls,
                                                                  const float* __restrict__ pos,
                                                                  _Float16* __restrict__ xh, size_t plane,
                                                                  float* __restrict__ stats, int B, int P, int D) {
  const int groups = D >> 3;
  const size_t n = (size_t)B * (P + 1) * groups;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  // every lane of an 8-lane group takes part in the chunk shuffles: past the end, repeat the last
  // group (n is a multiple of 8) and store nothing
  const size_t gi = gid < n ? gid : n - 1;
  const size_t r = gi / groups;
  const int c0 = (int)(gi - r * groups) * 8;
  const int t = (int)(r % (P + 1)), b = (int)(r / (P + 1));
  const float* src = t == 0 ? cls + c0 : patches + ((size_t)b * P + (t - 1)) * D + c0;
  const float* pp = pos + (size_t)t * D + c0;
  const float4 s0 = reinterpret_cast<const float4*>(src)[0], s1 = reinterpret_cast<const float4*>(src)[1];
  const float4 p0 = reinterpret_cast<const float4*>(pp)[0], p1 = reinterpret_cast<const float4*>(pp)[1];
  const float y[8] = {s0.x + p0.x, s0.y + p0.y, s0.z + p0.z, s0.w + p0.w,
                      s1.x + p1.x, s1.y + p1.y, s1.z + p1.z, s1.w + p1.w};
  float mean, m2;
  ln_chunk_stats(y, mean, m2);
  if (gid >= n) return;
  half8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hi[e] = static_cast<_Float16>(y[e]);
    lo[e] = static_cast<_Float16>(y[e] - static_cast<float>(hi[e]));
  }
  _Float16* xr = xh + r * D + c0;
  *reinterpret_cast<half8*>(xr) = hi;
  *reinterpret_cast<half8*>(xr + plane) = lo;
  if (stats && (c0 & 63) == 0) reinterpret_cast<float2*>(stats)[r * (D >> 6) + (c0 >> 6)] = float2{mean, m2};
}

template <typename T>
__global__ void gather_rows_kernel(const float* __restrict__ x, T* __restrict__ y, int rows,
                                   int stride_rows, int D) {
  const size_t n = (size_t)rows * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / D, c = i - r * D;
    y[i] = cvt<T>(x[r * stride_rows * D + c]);
  }
}

__global__ void affine_kernel(const float* x, float* y, size_t n, float scale, float shift) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    y[i] = x[i] * scale + shift;
}

void check_src(const char* op, int src, int C) {
  if (src < kSrcF32Nchw || src > kSrcU8Nhwc) throw std::invalid_argument(std::string(op) + ": unknown source kind");
  if (src != kSrcF32Nchw && C != 3) throw std::invalid_argument(std::string(op) + ": 8-bit images have 3 channels");
}

template <int SRC>
void ingest_src(const void* x, void* y, int B, int C, int H, int W, int cpad, bool f16, const InputXf& xf,
                hipStream_t s) {
  const size_t n = (size_t)B * H * W;
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((ingest_kernel<T, SRC>), dim3(grid_for(n)), dim3(256), 0, s, x, (T*)y, B, C, H, W, cpad, xf);
  });
}

template <int SRC>
void patchify_scalar(const void* x, void* y, int B, int C, int H, int W, int ps, bool f16, const InputXf& xf,
                     hipStream_t s) {
  const size_t n = (size_t)B * C * H * W;
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((patchify_kernel<T, SRC>), dim3(grid_for(n)), dim3(256), 0, s, x, (T*)y, B, C, H, W, ps, xf);
  });
}

template <int SRC, bool WIDE>
void patchify_vec_u8(const void* x, void* y, int H, int W, int ps, int GH, int GW, int nt, bool f16,
                     const InputXf& xf, hipStream_t s) {
  const unsigned char* xb = static_cast<const unsigned char*>(x);
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((patchify_vec_u8_kernel<T, SRC, WIDE>), dim3((nt + 255) / 256), dim3(256), 0, s, xb, (T*)y, H, W, ps,
               GH, GW, nt, xf);
  });
}

}  // namespace

void ingest_nchw(const void* x, void* y, int B, int C, int H, int W, int cpad, bool f16,
                 hipStream_t s, int src, const InputXf& xf) {
  check_src("ingest_nchw", src, C);
  if (src == kSrcU8Nchw)
    ingest_src<kSrcU8Nchw>(x, y, B, C, H, W, cpad, f16, xf, s);
  else if (src == kSrcU8Nhwc)
    ingest_src<kSrcU8Nhwc>(x, y, B, C, H, W, cpad, f16, xf, s);
  else
    ingest_src<kSrcF32Nchw>(x, y, B, C, H, W, cpad, f16, xf, s);
}

void patchify(const void* xv, void* y, int B, int C, int H, int W, int ps, bool f16,
              hipStream_t s, int src, const InputXf& xf) {
  check_src("patchify", src, C);
  const size_t n = (size_t)B * C * H * W;
  const int GH = H / ps, GW = W / ps;
  const int nt = B * GH * GW * C * ps * (ps / 8);
  if (src != kSrcF32Nchw) {
    // 8-bit pixels: the vector form whenever the stores allow it; its loads are one 8-byte vector
    // per thread only for an NCHW image whose base and row pitch are multiples of 8 bytes
    if (ps % 8 == 0 && n < (size_t)INT32_MAX && aligned(y, 16)) {
      const bool wide = src == kSrcU8Nchw && W % 8 == 0 && aligned(xv, 8);
      if (wide)
        patchify_vec_u8<kSrcU8Nchw, true>(xv, y, H, W, ps, GH, GW, nt, f16, xf, s);
      else if (src == kSrcU8Nchw)
        patchify_vec_u8<kSrcU8Nchw, false>(xv, y, H, W, ps, GH, GW, nt, f16, xf, s);
      else
        patchify_vec_u8<kSrcU8Nhwc, false>(xv, y, H, W, ps, GH, GW, nt, f16, xf, s);
    } else if (src == kSrcU8Nchw) {
      patchify_scalar<kSrcU8Nchw>(xv, y, B, C, H, W, ps, f16, xf, s);
    } else {
      patchify_scalar<kSrcU8Nhwc>(xv, y, B, C, H, W, ps, f16, xf, s);
    }
    return;
  }
  const float* x = static_cast<const float*>(xv);
  if (ps % 8 == 0 && W % 4 == 0 && n / 8 < (size_t)INT32_MAX && n < (size_t)INT32_MAX && aligned(x, 16) &&
      aligned(y, 16)) {
    with_type(f16, [&](auto t) {
      using T = decltype(t);
      SPI_LAUNCH((patchify_vec_kernel<T>), dim3((nt + 255) / 256), dim3(256), 0, s, x, (T*)y, C, H, W, ps, GH, GW, nt);
    });
    return;
  }
  patchify_scalar<kSrcF32Nchw>(xv, y, B, C, H, W, ps, f16, xf, s);
}

void vit_assemble(const float* patches, const float* cls, const float* pos, float* x, int B,
                  int P, int D, hipStream_t s) {
  const size_t n = (size_t)B * (P + 1) * D;
  SPI_LAUNCH(vit_assemble_kernel, dim3(grid_for(n)), dim3(256), 0, s, patches, cls,
                     pos, x, B, P, D);
}

void vit_assemble_planes(const float* patches, const float* cls, const float* pos, _Float16* xh, size_t plane,
                         float* stats, int B, int P, int D, hipStream_t s) {
  if (D % 64 || plane % 8) throw std::invalid_argument("vit_assemble_planes: D % 64 == 0, plane % 8 == 0");
  const size_t n = (size_t)B * (P + 1) * (D / 8);
  SPI_LAUNCH(vit_assemble_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, patches, cls, pos, xh,
             plane, stats, B, P, D);
}

void gather_rows(const float* x, void* y, int rows, int stride_rows, int D, bool f16,
                 hipStream_t s) {
  const size_t n = (size_t)rows * D;
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((gather_rows_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s, x, (T*)y, rows, stride_rows, D);
  });
}

void affine(const float* x, float* y, size_t n, float scale, float shift, hipStream_t s) {
  SPI_LAUNCH(affine_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, y, n, scale, shift);
}

}  // namespace spi
