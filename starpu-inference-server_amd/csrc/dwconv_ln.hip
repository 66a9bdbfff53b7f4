// The ConvNeXt kernels (gfx950): depthwise 7x7 conv + bias + LayerNorm over channels in one pass over an
// NHWC map, and the two row kernels beside it -- LayerNorm of rows of any C % 32 == 0 (optionally behind a
// mean over a map's rows) and LayerNorm into the space-to-depth rows of a 2x2 / stride 2 conv -- and Swin's
// patch merging row kernel s2d_ln (gather the four pixels, then LayerNorm over 4 C).  Swin v2 adds ln_rows_add
// (the residual-post-norm: res + LN(x)) and s2d_rows (the merge's gather alone; its LayerNorm follows the Linear).
//
// dwconv7_ln.  Every channel is its own 49-tap filter: no contraction across channels, nothing for the
// MFMA, 49 FMAs per output on the VALU and the map read once.  A workgroup of 256 threads owns a TH x TW
// pixel tile and all C channels of it, because the LayerNorm behind the conv needs them:
//   for each slab of kDwSlabChunks 16-byte channel chunks (8 fp16 or 4 fp32 channels each)
//     stage the (TH + 6) x (TW + 6) halo of the slab into LDS, 16-byte loads, zeros for the padding ring
//     each lane takes one chunk of a run of R output pixels along W: per filter row it reads R + 6 chunks
//     from LDS and slides the 7-wide window over them in registers (one LDS read feeds up to 7 taps), the
//     row's 7 weight vectors coming from the tap-major [49][C] weights; fp32 accumulators, started at the bias
//     the results go to an fp32 row image [TH TW][C] in LDS
//   then one wave per pixel normalises its row of the image: two-pass fp32 statistics (mean, then centred
//   squares), gain and bias, one rounding at the store.
// The un-normalised conv result never leaves the workgroup.  No atomics, no split: a launch's bits are fixed.
#include <stdexcept>
#include <string>

#include "convnext_pack.hpp"
#include "row_util.hpp"
#include "spi_kernels.hpp"
#include "swin_pack.hpp"

namespace spi {
namespace {

template <typename T>
struct DwChunk;  // one 16-byte channel chunk
template <>
struct DwChunk<_Float16> {
  static constexpr int N = 8;
  using V = half8;
};
template <>
struct DwChunk<float> {
  static constexpr int N = 4;
  using V = floatx4;
};

// The halo image: [halo pixel][kDwPixelStride chunks], a slab's chunks of one pixel contiguous.
// Bank rule: a 16-byte LDS read is served 16 lanes at a time -- 16 lanes x 4 banks are the 64 banks -- so it
// is conflict-free when the 16 lanes of each such group touch 16 different 16-byte bank groups,
// (byte address / 16) % 16.  Lane l of the conv phase takes chunk l % kDwSlabChunks of run l / kDwSlabChunks,
// and a run's next neighbour starts R pixels on.  With 16 chunks per slab and a pixel stride of 16 chunks
// (256 bytes, one line of all 64 banks) a group of 16 lanes is one run reading one whole line, at whatever
// pixel of the window: no padding chunk is needed, and the staging stores (chunk-fastest too) are the same
// lines.  A slab of 8 or 4 chunks would need a stride of 10 or 5 chunks by the same rule (dw_reads_disjoint).
constexpr int kDwSlabChunks = 16;
constexpr int kDwPixelStride = 16;  // (dw_reads_disjoint: convnext_pack.hpp)
static_assert(dw_reads_disjoint(kDwSlabChunks, kDwPixelStride, 4) && dw_reads_disjoint(kDwSlabChunks, kDwPixelStride, 2) &&
                  dw_reads_disjoint(kDwSlabChunks, kDwPixelStride, 1),
              "a 16-lane group of the window reads must cover 16 distinct 16-byte bank groups");
static_assert(dw_reads_disjoint(8, 10, 4) && dw_reads_disjoint(4, 5, 4) && !dw_reads_disjoint(8, 8, 4),
              "the rule's arithmetic for narrower slabs");

// LayerNorm of one fp32 row of C values (C % 4 == 0) a wave holds in LDS or registers through `at(c)`, which
// returns the float4 at column c: two-pass statistics, then `put(c, o)` with the four normalised values.
template <typename At, typename Put>
__device__ __forceinline__ void ln_row_c(int C, int lane, const float* __restrict__ g, const float* __restrict__ b,
                                         float eps, At&& at, Put&& put) {
  float s = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const float4 v = at(c);
    s += (v.x + v.y) + (v.z + v.w);
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const float4 v = at(c);
    const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
    q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  for (int c = lane * 4; c < C; c += 256) {
    const float4 v = at(c), gg = *reinterpret_cast<const float4*>(g + c), bb = *reinterpret_cast<const float4*>(b + c);
    const float o[4] = {(v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y,
                        (v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w};
    put(c, o);
  }
}

// TH x TW: the pixel tile; R: a lane's run of output pixels along W (TW % R == 0); CMAX: the largest C the
// instance's row image holds.  x [B][H][W][C], w [49][C], y [B H W][C], all of T; bias, gamma, beta fp32 [C].
template <typename T, int TH, int TW, int R, int CMAX>
__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, T* __restrict__ y, int H,
                                                         int W, int C, float eps) {
  using V = typename DwChunk<T>::V;
  constexpr int CH = DwChunk<T>::N, NCH = kDwSlabChunks, PS = kDwPixelStride;
  constexpr int HH = TH + 6, HW = TW + 6, RUNS = TH * (TW / R);
  static_assert(TW % R == 0 && 256 % NCH == 0, "runs tile the row; 16-lane groups do not straddle runs");
  static_assert(sizeof(V) * HH * HW * PS + sizeof(float) * TH * TW * CMAX <= 80 * 1024, "two workgroups per CU");
  __shared__ V halo[HH * HW * PS];
  __shared__ __attribute__((aligned(16))) float rows[TH * TW * CMAX];
  const int tid = threadIdx.x;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  int t = blockIdx.x;
  const int x0 = (t % tiles_x) * TW;
  t /= tiles_x;
  const int y0 = (t % tiles_y) * TH;
  const int b = t / tiles_y;
  const int nchunks = C / CH;
  const T* xb = x + (size_t)b * H * W * C;
  // every condition around a barrier depends on the slab or the kernel's arguments only: wave-uniform
  for (int c0 = 0; c0 < nchunks; c0 += NCH) {
    if (c0) __syncthreads();  // the previous slab's window reads are done
    for (int i = tid; i < HH * HW * NCH; i += 256) {
      const int cq = i % NCH, px = i / NCH;
      const int gy = y0 - 3 + px / HW, gx = x0 - 3 + px % HW, c = c0 + cq;
      V v = {};
      if (gy >= 0 && gy < H && gx >= 0 && gx < W && c < nchunks)
        v = *reinterpret_cast<const V*>(xb + ((size_t)gy * W + gx) * C + c * CH);
      halo[px * PS + cq] = v;
    }
    __syncthreads();
    for (int i = tid; i < NCH * RUNS; i += 256) {
      const int cq = i % NCH, run = i / NCH, c = c0 + cq;
      if (c >= nchunks) continue;  // the last slab's missing chunks
      const int ry = run / (TW / R), rx = (run % (TW / R)) * R;
      float acc[R][CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        const float bv = bias[c * CH + e];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][e] = bv;
      }
#pragma unroll 1
      for (int ky = 0; ky < 7; ++ky) {
        V win[R + 6], wv[7];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) wv[kx] = *reinterpret_cast<const V*>(w + (size_t)(ky * 7 + kx) * C + c * CH);
#pragma unroll
        for (int j = 0; j < R + 6; ++j) win[j] = halo[((ry + ky) * HW + rx + j) * PS + cq];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < CH; ++e) acc[r][e] += static_cast<float>(win[r + kx][e]) * static_cast<float>(wv[kx][e]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float* dst = rows + (size_t)((ry * TW + rx + r) * C + c * CH);
#pragma unroll
        for (int e = 0; e < CH; e += 4)
          *reinterpret_cast<float4*>(dst + e) = float4{acc[r][e], acc[r][e + 1], acc[r][e + 2], acc[r][e + 3]};
      }
    }
  }
  __syncthreads();
  // one wave per pixel of the tile; a pixel past the map's edge is skipped by its whole wave, and no
  // barrier follows
  const int lane = tid & 63;
  for (int p = tid >> 6; p < TH * TW; p += 4) {
    const int gy = y0 + p / TW, gx = x0 + p % TW;
    if (gy >= H || gx >= W) continue;
    const float* row = rows + (size_t)p * C;
    T* dst = y + (((size_t)b * H + gy) * W + gx) * C;
    ln_row_c(
        C, lane, gamma, beta, eps, [&](int c) { return *reinterpret_cast<const float4*>(row + c); },
        [&](int c, const float(&o)[4]) { store4(dst + c, o); });
  }
}

template <typename TI>
__device__ __forceinline__ float4 load4(const TI* p) {
  if constexpr (sizeof(TI) == 2) {
    const half4 h = *reinterpret_cast<const half4*>(p);
    return float4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  } else {
    return *reinterpret_cast<const float4*>(p);
  }
}

// One wave per output row, the row in registers (C <= 1536: six float4 per lane).  Input row `row` is
// x[row][C], or with pool_hw > 0 the mean of the pool_hw rows x[row pool_hw ..][C] (summed in row order,
// then divided).  W == 0: y[row][C].  W > 0 (space to depth, pool_hw == 0): row = (b, h, w) of an H x W
// map, written to columns ((h & 1) 2 + (w & 1)) C .. of row (b, h / 2, w / 2) of y [.][4 C].
template <typename T, typename TI>
__global__ __launch_bounds__(256) void ln_rows_c_kernel(const TI* __restrict__ x, T* __restrict__ y,
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        int rows, int C, int pool_hw, int H, int W, float eps) {
  constexpr int NV = kDwconvMaxC / 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TI* xr = x + (size_t)row * (pool_hw > 0 ? pool_hw : 1) * C;
  float4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (lane + 64 * j) * 4;
    v[j] = float4{0.f, 0.f, 0.f, 0.f};
    if (c >= C) continue;
    if (pool_hw <= 0) {
      v[j] = load4(xr + c);
    } else {
      float4 a = load4(xr + c);
      for (int p = 1; p < pool_hw; ++p) {
        const float4 u = load4(xr + (size_t)p * C + c);
        a = float4{a.x + u.x, a.y + u.y, a.z + u.z, a.w + u.w};
      }
      const float n = (float)pool_hw;
      v[j] = float4{a.x / n, a.y / n, a.z / n, a.w / n};
    }
  }
  size_t off = (size_t)row * C;
  if (W > 0) {
    const int wx = row % W, hy = (row / W) % H, img = row / (W * H);
    off = (((size_t)img * (H / 2) + hy / 2) * (W / 2) + wx / 2) * 4 * C + (size_t)((hy & 1) * 2 + (wx & 1)) * C;
  }
  T* dst = y + off;
  ln_row_c(
      C, lane, g, b, eps,
      [&](int c) {  // c = (lane + 64 j) 4: the select chain keeps v in registers (no indexed copy in scratch)
        float4 r = v[0];
#pragma unroll
        for (int j = 1; j < NV; ++j)
          if (c >= 256 * j) r = v[j];
        return r;
      },
      [&](int c, const float(&o)[4]) { store4(dst + c, o); });
}

// Swin's patch merging in front of its Linear: one wave per output row (b, i, j) of y [B (H/2) (W/2)][4 C].
// The row is gathered from its four pixels into registers -- pixel (2 i + dy, 2 j + dx) at columns
// (dx 2 + dy) C .., torchvision's cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]) -- and then
// normalised over all 4 C columns (two-pass fp32 statistics, gain and bias of 4 C).  4 C <= 2048: eight float4
// per lane.  C % 32 == 0, so a float4 never straddles two pixels.
template <typename T>
__global__ __launch_bounds__(256) void s2d_ln_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                     const float* __restrict__ g, const float* __restrict__ b, int rows,
                                                     int H, int W, int C, float eps) {
  constexpr int NV = kS2dMaxRow / 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int W2 = W / 2, H2 = H / 2;
  const int j2 = row % W2, i2 = (row / W2) % H2, img = row / (W2 * H2);
  const T* x00 = x + (((size_t)img * H + 2 * i2) * W + 2 * j2) * C;
  float4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (lane + 64 * j) * 4;
    v[j] = float4{0.f, 0.f, 0.f, 0.f};
    if (c >= 4 * C) continue;
    const int q = c / C;  // dx 2 + dy
    v[j] = load4(x00 + ((size_t)(q & 1) * W + (q >> 1)) * C + (c - q * C));
  }
  T* dst = y + (size_t)row * 4 * C;
  ln_row_c(
      4 * C, lane, g, b, eps,
      [&](int c) {
        float4 r = v[0];
#pragma unroll
        for (int j = 1; j < NV; ++j)
          if (c >= 256 * j) r = v[j];
        return r;
      },
      [&](int c, const float(&o)[4]) { store4(dst + c, o); });
}

// Swin v2's residual-post-norm: y[row] = res[row] + LN(x[row]) gamma + beta, one wave per row, the row of x in
// registers as in ln_rows_c_kernel.  y may be res (the residual stream updated in place): a lane reads the four
// addends of a float4 and then stores the same four columns, and no other lane touches them -- hence no
// __restrict__ on the two.
template <typename T>
__global__ __launch_bounds__(256) void ln_rows_add_kernel(const T* __restrict__ x, const T* res, T* y,
                                                          const float* __restrict__ g, const float* __restrict__ b,
                                                          int rows, int C, float eps) {
  constexpr int NV = kDwconvMaxC / 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* xr = x + (size_t)row * C;
  float4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (lane + 64 * j) * 4;
    v[j] = c < C ? load4(xr + c) : float4{0.f, 0.f, 0.f, 0.f};
  }
  const T* rr = res + (size_t)row * C;
  T* dst = y + (size_t)row * C;
  ln_row_c(
      C, lane, g, b, eps,
      [&](int c) {
        float4 r = v[0];
#pragma unroll
        for (int j = 1; j < NV; ++j)
          if (c >= 256 * j) r = v[j];
        return r;
      },
      [&](int c, const float(&o)[4]) {
        const float4 a = load4(rr + c);
        const float sum[4] = {a.x + o[0], a.y + o[1], a.z + o[2], a.w + o[3]};
        store4(dst + c, sum);
      });
}

// Swin v2's patch merging gathers before its Linear and normalises behind it: s2d_ln's gather alone, a copy in
// 16-byte chunks.  Thread (row, chunk) of y [B (H/2) (W/2)][4 C]: the chunk's column c lies in pixel
// q = c / C = dx 2 + dy of the row's 2x2 block (C % 32 == 0: a chunk never straddles two pixels).
template <typename T>
__global__ __launch_bounds__(256) void s2d_rows_kernel(const T* __restrict__ x, T* __restrict__ y, size_t chunks, int H,
                                                       int W, int C) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const int cpr = 4 * C / EPC;  // chunks per output row
  const size_t row = i / cpr;
  const int c = (int)(i % cpr) * EPC, q = c / C;
  const int W2 = W / 2, H2 = H / 2;
  const int j2 = (int)(row % W2), i2 = (int)((row / W2) % H2);
  const size_t img = row / ((size_t)W2 * H2);
  const T* src = x + ((img * H + 2 * i2 + (q & 1)) * W + 2 * j2 + (q >> 1)) * C + (c - q * C);
  *reinterpret_cast<uint4*>(y + row * 4 * C + c) = *reinterpret_cast<const uint4*>(src);
}

void check_rows(const char* what, const void* x, const void* y, const float* g, const float* b, int C) {
  if (!dwconv7_supported(C)) throw std::invalid_argument(std::string(what) + ": C must be a multiple of 32 from 32 to 1536");
  if (!aligned(x, 16) || !aligned(y, 16) || !aligned(g, 16) || !aligned(b, 16))
    throw std::invalid_argument(std::string(what) + ": 16-byte aligned x, y, gamma and beta");
}

template <typename T, int TH, int TW, int R, int CMAX>
void launch_dwconv(const void* x, const void* w, const float* bias, const float* g, const float* b, void* y, int B,
                   int H, int W, int C, float eps, hipStream_t s) {
  const long long tiles = (long long)B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
  if (tiles > 0x7fffffffLL) throw std::invalid_argument("dwconv7_ln: too many pixel tiles for one grid");
  SPI_LAUNCH((dwconv7_ln_kernel<T, TH, TW, R, CMAX>), dim3((unsigned)tiles), dim3(256), 0, s, static_cast<const T*>(x),
             static_cast<const T*>(w), bias, g, b, static_cast<T*>(y), H, W, C, eps);
}

}  // namespace

// The tile by C: the fp32 row image of TH TW pixels x C channels and the halo of a 16-chunk slab fit 80 KiB
// (two workgroups per CU), so the tile shrinks as C grows and the run with it, to keep lanes busy:
// C <= 96: 8 x 8, runs of 4; <= 256: 4 x 8, runs of 4; <= 768: 4 x 4, runs of 2; <= 1536: 2 x 4, single pixels.
void dwconv7_ln(const void* x, const void* w, const float* bias, const float* gamma, const float* beta, void* y, int B,
                int H, int W, int C, float eps, bool f16, hipStream_t s) {
  check_rows("dwconv7_ln", x, y, gamma, beta, C);
  if (B < 1 || H < 1 || W < 1) throw std::invalid_argument("dwconv7_ln: B, H and W must be positive");
  if (!aligned(w, 16) || !aligned(bias, 16)) throw std::invalid_argument("dwconv7_ln: 16-byte aligned weights and bias");
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    if (C <= 96)
      launch_dwconv<T, 8, 8, 4, 96>(x, w, bias, gamma, beta, y, B, H, W, C, eps, s);
    else if (C <= 256)
      launch_dwconv<T, 4, 8, 4, 256>(x, w, bias, gamma, beta, y, B, H, W, C, eps, s);
    else if (C <= 768)
      launch_dwconv<T, 4, 4, 2, 768>(x, w, bias, gamma, beta, y, B, H, W, C, eps, s);
    else
      launch_dwconv<T, 2, 4, 1, 1536>(x, w, bias, gamma, beta, y, B, H, W, C, eps, s);
  });
}

void ln_rows(const void* x, bool x_f32, void* y, const float* gamma, const float* beta, int rows, int C, int pool_hw,
             float eps, bool f16, hipStream_t s) {
  check_rows("ln_rows", x, y, gamma, beta, C);
  if (rows < 1 || pool_hw < 0) throw std::invalid_argument("ln_rows: rows >= 1, pool_hw >= 0");
  const dim3 grid((rows + 3) / 4);
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    if (x_f32)
      SPI_LAUNCH((ln_rows_c_kernel<T, float>), grid, dim3(256), 0, s, static_cast<const float*>(x), static_cast<T*>(y),
                 gamma, beta, rows, C, pool_hw, 0, 0, eps);
    else
      SPI_LAUNCH((ln_rows_c_kernel<T, T>), grid, dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y), gamma,
                 beta, rows, C, pool_hw, 0, 0, eps);
  });
}

void ln_space_to_depth(const void* x, void* y, const float* gamma, const float* beta, int B, int H, int W, int C,
                       float eps, bool f16, hipStream_t s) {
  check_rows("ln_space_to_depth", x, y, gamma, beta, C);
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2) throw std::invalid_argument("ln_space_to_depth: B >= 1, even H and W");
  if ((long long)B * H * W > 0x7fffffffLL) throw std::invalid_argument("ln_space_to_depth: too many pixels");
  const int rows = B * H * W;
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((ln_rows_c_kernel<T, T>), dim3((rows + 3) / 4), dim3(256), 0, s, static_cast<const T*>(x),
               static_cast<T*>(y), gamma, beta, rows, C, 0, H, W, eps);
  });
}

void s2d_ln(const void* x, void* y, const float* gamma, const float* beta, int B, int H, int W, int C, float eps,
            bool f16, hipStream_t s) {
  if (!s2d_ln_supported(C)) throw std::invalid_argument("s2d_ln: C must be a multiple of 32 with 4 C at most 2048");
  if (!aligned(x, 16) || !aligned(y, 16) || !aligned(gamma, 16) || !aligned(beta, 16))
    throw std::invalid_argument("s2d_ln: 16-byte aligned x, y, gamma and beta");
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2) throw std::invalid_argument("s2d_ln: B >= 1, even H and W");
  if ((long long)B * H * W > 0x7fffffffLL) throw std::invalid_argument("s2d_ln: too many pixels");
  const int rows = B * (H / 2) * (W / 2);
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((s2d_ln_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y),
               gamma, beta, rows, H, W, C, eps);
  });
}

void ln_rows_add(const void* x, const void* res, void* y, const float* gamma, const float* beta, int rows, int C,
                 float eps, bool f16, hipStream_t s) {
  check_rows("ln_rows_add", x, y, gamma, beta, C);
  if (!res || !aligned(res, 16)) throw std::invalid_argument("ln_rows_add: a 16-byte aligned res");
  if (rows < 1) throw std::invalid_argument("ln_rows_add: rows >= 1");
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((ln_rows_add_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, static_cast<const T*>(x),
               static_cast<const T*>(res), static_cast<T*>(y), gamma, beta, rows, C, eps);
  });
}

void s2d_rows(const void* x, void* y, int B, int H, int W, int C, bool f16, hipStream_t s) {
  if (!s2d_ln_supported(C)) throw std::invalid_argument("s2d_rows: C must be a multiple of 32 with 4 C at most 2048");
  if (!aligned(x, 16) || !aligned(y, 16)) throw std::invalid_argument("s2d_rows: 16-byte aligned x and y");
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2) throw std::invalid_argument("s2d_rows: B >= 1, even H and W");
  if ((long long)B * H * W > 0x7fffffffLL) throw std::invalid_argument("s2d_rows: too many pixels");
  const size_t chunks = (size_t)B * H * W * C / (f16 ? 8 : 4);
  if ((chunks + 255) / 256 > 0x7fffffffULL) throw std::invalid_argument("s2d_rows: too many 16-byte chunks for one grid");
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((s2d_rows_kernel<T>), dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, static_cast<const T*>(x),
               static_cast<T*>(y), chunks, H, W, C);
  });
}

}  // namespace spi
