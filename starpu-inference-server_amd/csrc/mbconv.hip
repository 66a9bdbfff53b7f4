// The MBConv kernels of the EfficientNet replicas (gfx950): the depthwise k x k conv + bias + SiLU with the
// squeeze-and-excitation pool sums (dwconv_act), the SE gate of one image (se_gate) and the per-(image, channel)
// scaling of the expanded map (scale_channels).  Launch order in a block: dwconv_act -> se_gate -> scale_channels
// -> the project GEMM.
//
// dwconv_act.  Every channel is its own k x k filter: nothing for the MFMA, k k FMAs per output on the VALU, the
// map read once.  Unlike dwconv7_ln nothing couples the channels, so the grid is (pixel tile, channel slab, image):
//   a workgroup of 256 threads owns a TH x 8 tile of output pixels (16 x 8 at stride 1, 8 x 8 at stride 2) of one
//   slab of kMbSlabChunks 16-byte channel chunks (64 fp16 or 32 fp32 channels);
//   it stages the slab's ((TH - 1) s + k) x (7 s + k) halo in LDS, 16-byte loads, zeros for the padding ring, for
//   pixels past the map and for the chunks a last, partial slab does not have;
//   lane l takes chunk l % 8 of run l / 8, a run being R = 4 / s output pixels along W: per filter row it reads
//   the (R - 1) s + k halo chunks its outputs touch (stride 1: the k-wide window slides over them in registers;
//   stride 2: every column read is used) and the row's k weight vectors from the tap-major [k k][C] weights; fp32
//   accumulators, started at the bias; SiLU in fp32; one rounding at the 16-byte store.
// Pool sums: a lane adds its run's fp32 activations (before the rounding), the 32 runs of a chunk meet in LDS --
// the halo's bytes, free by then -- and one thread per channel adds them in run order into part[b][tile][c].
// se_gate adds the tiles in index order.  No atomics, no split: a launch's bits are fixed.
#include <stdexcept>
#include <string>

#include "convnext_pack.hpp"
#include "device_math.hpp"
#include "mbconv_pack.hpp"
#include "row_util.hpp"
#include "spi_kernels.hpp"

namespace spi {
namespace {

template <typename T>
struct MbChunk;  // one 16-byte channel chunk
template <>
struct MbChunk<_Float16> {
  static constexpr int N = 8;
  using V = half8;
};
template <>
struct MbChunk<float> {
  static constexpr int N = 4;
  using V = floatx4;
};

// The halo image: [halo pixel][kMbPixelStride chunks], of which a slab fills the first kMbSlabChunks.  Lanes are
// chunk-fastest, so the 16 lanes one LDS pass serves are two neighbouring runs of one tile row (TW / R is even),
// kMbRunSpan = R s = 4 halo pixels apart at either stride: with 10 chunks per pixel the second run starts
// 40 = 8 (mod 16) bank groups on, and the two runs' 8 chunks cover all 16 (DESIGN.md 3.1.9's rule).
constexpr int kMbSlabChunks = 8, kMbPixelStride = 10, kMbRunSpan = 4, kMbRuns = 32;
static_assert(dw_reads_disjoint(kMbSlabChunks, kMbPixelStride, kMbRunSpan),
              "a 16-lane group of the window reads must cover 16 distinct 16-byte bank groups");
static_assert(!dw_reads_disjoint(kMbSlabChunks, kMbSlabChunks, kMbRunSpan), "... which an unpadded pixel stride would not");

// x [B][H][W][C], w [K K][C], y [B][OH][OW][C], all of T; bias fp32 [C]; part null or fp32 [B][tiles][C].
// Grid (tiles, slabs, B).  Every condition around a barrier is a kernel argument.
template <typename T, int K, int S>
__global__ __launch_bounds__(256) void dwconv_act_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                         const float* __restrict__ bias, T* __restrict__ y,
                                                         float* __restrict__ part, int H, int W, int OH, int OW, int C,
                                                         int act) {
  using V = typename MbChunk<T>::V;
  constexpr int CH = MbChunk<T>::N, NCH = kMbSlabChunks, PS = kMbPixelStride;
  constexpr int R = kMbRunSpan / S, TW = kDwTileW, TH = S == 1 ? 16 : 8, RPR = TW / R, PAD = K / 2;
  constexpr int HH = (TH - 1) * S + K, HW = (TW - 1) * S + K, WIN = (R - 1) * S + K;
  static_assert(TH * RPR == kMbRuns && NCH * kMbRuns == 256, "one (chunk, run) per thread");
  static_assert(RPR % 2 == 0, "the two runs of a 16-lane group lie in one tile row");
  static_assert(sizeof(V) * HH * HW * PS <= 64 * 1024 && sizeof(float) * kMbRuns * NCH * CH <= sizeof(V) * HH * HW * PS,
                "two workgroups per CU; the pool scratch fits the halo's bytes");
  __shared__ V halo[HH * HW * PS];
  const int tid = threadIdx.x, cq = tid % NCH, run = tid / NCH;
  const int tiles_x = (OW + TW - 1) / TW, tile = blockIdx.x;
  const int ox0 = (tile % tiles_x) * TW, oy0 = (tile / tiles_x) * TH;
  const int c0 = blockIdx.y * NCH, b = blockIdx.z, nchunks = C / CH;
  const T* xb = x + (size_t)b * H * W * C;
  const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
  for (int i = tid; i < HH * HW * NCH; i += 256) {
    const int q = i % NCH, px = i / NCH;
    const int gy = iy0 + px / HW, gx = ix0 + px % HW, c = c0 + q;
    V v = {};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W && c < nchunks)
      v = *reinterpret_cast<const V*>(xb + ((size_t)gy * W + gx) * C + c * CH);
    halo[px * PS + q] = v;
  }
  __syncthreads();
  const int c = c0 + cq, ry = run / RPR, rx = (run % RPR) * R;
  float psum[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) psum[e] = 0.f;
  if (c < nchunks) {  // (a last slab's missing chunks: no barrier inside)
    float acc[R][CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const float bv = bias[c * CH + e];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r][e] = bv;
    }
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
      V win[WIN], wv[K];
#pragma unroll
      for (int kx = 0; kx < K; ++kx) wv[kx] = *reinterpret_cast<const V*>(w + (size_t)(ky * K + kx) * C + c * CH);
#pragma unroll
      for (int j = 0; j < WIN; ++j) win[j] = halo[((ry * S + ky) * HW + rx * S + j) * PS + cq];
#pragma unroll
      for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int e = 0; e < CH; ++e) acc[r][e] += static_cast<float>(win[r * S + kx][e]) * static_cast<float>(wv[kx][e]);
    }
    const int oy = oy0 + ry;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int ox = ox0 + rx + r;
      if (oy >= OH || ox >= OW) continue;
      float o[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        o[e] = act == (int)Act::Silu ? silu(acc[r][e]) : acc[r][e];
        psum[e] += o[e];
      }
      T* dst = y + (((size_t)b * OH + oy) * OW + ox) * C + c * CH;
      if constexpr (CH == 8)
        store8(dst, o);
      else
        store4(dst, o);
    }
  }
  if (!part) return;
  __syncthreads();  // every window read is done: the halo's bytes become the pool scratch [run][NCH CH]
  float* red = reinterpret_cast<float*>(halo);
#pragma unroll
  for (int e = 0; e < CH; ++e) red[run * (NCH * CH) + cq * CH + e] = psum[e];
  __syncthreads();
  if (tid < NCH * CH) {
    float s = 0.f;
    for (int q = 0; q < kMbRuns; ++q) s += red[q * (NCH * CH) + tid];
    const int ch = c0 * CH + tid;
    if (ch < C) part[((size_t)b * gridDim.x + tile) * C + ch] = s;
  }
}

// One workgroup per image, everything fp32: mean[c] = sum over the tiles of part (index order) / hw;
// h[j] = SiLU(W1[j] . mean + b1[j]), one wave per j; gate[c] = sigmoid(W2[c] . h + b2[c]), one thread per c.
// The tile sum keeps four loads in flight and adds them in index order.  A wave's 64 channels own 64 consecutive
// rows of W2, one contiguous block: the wave copies it into LDS in slices of kSeSlice columns with coalesced loads
// (a thread walking its own row from memory touches 64 cache lines per load) and each lane then walks its row of
// the slice, kSeSlice + 1 floats apart: conflict-free.  The barriers' trip counts depend on C and sq only.
constexpr int kSeSlice = 32;
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ part, int tiles, int hw,
                                                      const float* __restrict__ W1, const float* __restrict__ b1,
                                                      const float* __restrict__ W2, const float* __restrict__ b2,
                                                      float* __restrict__ gate, int C, int sq) {
  __shared__ float mean[kMbMaxC];
  __shared__ float h[kSeMaxSq];
  __shared__ float w2t[4 * 64 * (kSeSlice + 1)];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const float* pb = part + (size_t)b * tiles * C;
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    int t = 0;
    for (; t + 4 <= tiles; t += 4) {
      const float v0 = pb[(size_t)t * C + c], v1 = pb[(size_t)(t + 1) * C + c], v2 = pb[(size_t)(t + 2) * C + c],
                  v3 = pb[(size_t)(t + 3) * C + c];
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
    for (; t < tiles; ++t) s += pb[(size_t)t * C + c];
    mean[c] = s / (float)hw;
  }
  __syncthreads();
  for (int j = tid >> 6; j < sq; j += 4) {  // wave-uniform trip count, no barrier inside
    const float* wr = W1 + (size_t)j * C;
    float acc[8] = {};  // eight loads in flight: one chain would wait out every load's latency
    for (int c = lane; c < C; c += 512) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = c + 64 * u < C ? wr[c + 64 * u] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c + 64 * u < C) acc[u] += v[u] * mean[c + 64 * u];
    }
    float a = wave_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))) + b1[j];
    if (lane == 0) h[j] = a / (1.f + expf(-a));
  }
  __syncthreads();
  float* tile = w2t + (tid >> 6) * (64 * (kSeSlice + 1));
  for (int cb = 0; cb < C; cb += 256) {
    const int c0 = cb + (tid >> 6) * 64, nrow = min(64, C - c0);  // nrow <= 0: a wave past the last channels
    float a = 0.f;
    for (int j0 = 0; j0 < sq; j0 += kSeSlice) {
      const int nj = min(kSeSlice, sq - j0);
      if (j0 || cb) __syncthreads();  // the previous slice's reads are done
      for (int i0 = lane; i0 < nrow * nj; i0 += 512) {  // eight loads in flight, then their stores
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 64 * u;
          v[u] = i < nrow * nj ? W2[(size_t)(c0 + i / nj) * sq + j0 + i % nj] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 64 * u;
          if (i < nrow * nj) tile[(i / nj) * (kSeSlice + 1) + i % nj] = v[u];
        }
      }
      __syncthreads();
      if (lane < nrow)
        for (int jj = 0; jj < nj; ++jj) a += tile[lane * (kSeSlice + 1) + jj] * h[j0 + jj];
    }
    if (lane < nrow) {
      a += b2[c0 + lane];
      gate[(size_t)b * C + c0 + lane] = 1.f / (1.f + expf(-a));
    }
  }
}

// Thread per 16-byte chunk of x [B][HW][C]: y = x * gate[b][c], the product in fp32, one rounding.  y may be x:
// a thread reads its chunk before it stores the same chunk, and no other thread touches it.
template <typename T>
__global__ __launch_bounds__(256) void scale_channels_kernel(const T* x, const float* __restrict__ gate, T* y,
                                                             size_t chunks, size_t chunks_per_image, int C) {
  using V = typename MbChunk<T>::V;
  constexpr int CH = MbChunk<T>::N;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const int c = (int)(i % (size_t)(C / CH)) * CH;
  const float* g = gate + (i / chunks_per_image) * C + c;
  const V v = reinterpret_cast<const V*>(x)[i];
  float o[CH];
#pragma unroll
  for (int e = 0; e < CH; e += 4) {
    const float4 gg = *reinterpret_cast<const float4*>(g + e);
    o[e] = static_cast<float>(v[e]) * gg.x;
    o[e + 1] = static_cast<float>(v[e + 1]) * gg.y;
    o[e + 2] = static_cast<float>(v[e + 2]) * gg.z;
    o[e + 3] = static_cast<float>(v[e + 3]) * gg.w;
  }
  if constexpr (CH == 8)
    store8(y + i * CH, o);
  else
    store4(y + i * CH, o);
}

template <typename T, int K, int S>
void launch_dwconv_act(const void* x, const void* w, const float* bias, void* y, float* part, int B, int H, int W,
                       int C, int act, hipStream_t s) {
  const int OH = dwconv_out(H, K, S), OW = dwconv_out(W, K, S);
  const int slabs = (C / MbChunk<T>::N + kMbSlabChunks - 1) / kMbSlabChunks;
  SPI_LAUNCH((dwconv_act_kernel<T, K, S>), dim3((unsigned)dwconv_tiles(H, W, K, S), slabs, B), dim3(256), 0, s,
             static_cast<const T*>(x), static_cast<const T*>(w), bias, static_cast<T*>(y), part, H, W, OH, OW, C, act);
}

}  // namespace

void dwconv_act(const void* x, const void* w, const float* bias, void* y, float* pool_part, int B, int H, int W, int C,
                int k, int stride, int act, bool f16, hipStream_t s) {
  if (!dwconv_supported(C, k, stride))
    throw std::invalid_argument("dwconv_act: C a multiple of 8 from 8 to 4608, k 3 or 5, stride 1 or 2");
  if (act != (int)Act::None && act != (int)Act::Silu) throw std::invalid_argument("dwconv_act: act 0 (none) or 3 (silu)");
  if (B < 1 || B > 65535 || H < 1 || W < 1) throw std::invalid_argument("dwconv_act: 1 <= B <= 65535, H and W positive");
  const long long tiles = (long long)((dwconv_out(H, k, stride) + dwconv_tile_h(stride) - 1) / dwconv_tile_h(stride)) *
                          ((dwconv_out(W, k, stride) + kDwTileW - 1) / kDwTileW);
  if (tiles > 0x7fffffffLL) throw std::invalid_argument("dwconv_act: too many pixel tiles for one grid");
  if (!aligned(x, 16) || !aligned(w, 16) || !aligned(bias, 16) || !aligned(y, 16) || !aligned(pool_part, 4))
    throw std::invalid_argument("dwconv_act: 16-byte aligned x, w_packed, bias and y");
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    if (k == 3 && stride == 1)
      launch_dwconv_act<T, 3, 1>(x, w, bias, y, pool_part, B, H, W, C, act, s);
    else if (k == 3)
      launch_dwconv_act<T, 3, 2>(x, w, bias, y, pool_part, B, H, W, C, act, s);
    else if (stride == 1)
      launch_dwconv_act<T, 5, 1>(x, w, bias, y, pool_part, B, H, W, C, act, s);
    else
      launch_dwconv_act<T, 5, 2>(x, w, bias, y, pool_part, B, H, W, C, act, s);
  });
}

void se_gate(const float* part, int tiles, int hw, const float* W1, const float* b1, const float* W2, const float* b2,
             float* gate, int B, int C, int sq, hipStream_t s) {
  if (!se_supported(C, sq)) throw std::invalid_argument("se_gate: C a multiple of 8 from 8 to 4608, 1 <= sq <= 256");
  if (B < 1 || tiles < 1 || hw < 1) throw std::invalid_argument("se_gate: B, tiles and hw must be positive");
  if (!aligned(part, 4) || !aligned(W1, 4) || !aligned(b1, 4) || !aligned(W2, 4) || !aligned(b2, 4) || !aligned(gate, 4))
    throw std::invalid_argument("se_gate: 4-byte aligned fp32 operands");
  SPI_LAUNCH(se_gate_kernel, dim3(B), dim3(256), 0, s, part, tiles, hw, W1, b1, W2, b2, gate, C, sq);
}

void scale_channels(const void* x, const float* gate, void* y, int B, int HW, int C, bool f16, hipStream_t s) {
  if (!mbconv_channels_ok(C)) throw std::invalid_argument("scale_channels: C a multiple of 8 from 8 to 4608");
  if (B < 1 || HW < 1) throw std::invalid_argument("scale_channels: B and HW must be positive");
  if (!aligned(x, 16) || !aligned(y, 16) || !aligned(gate, 16))
    throw std::invalid_argument("scale_channels: 16-byte aligned x, gate and y");
  const size_t per_image = (size_t)HW * C / (f16 ? 8 : 4), chunks = per_image * B;
  if ((chunks + 255) / 256 > 0x7fffffffULL) throw std::invalid_argument("scale_channels: too many 16-byte chunks for one grid");
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((scale_channels_kernel<T>), dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s,
               static_cast<const T*>(x), gate, static_cast<T*>(y), chunks, per_image, C);
  });
}

}  // namespace spi
