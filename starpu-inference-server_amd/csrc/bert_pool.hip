// BERT sentence outputs (gfx950): the pooler (dense + tanh on the class-token rows) and the masked
// mean over the sequence.  Both are fp32 in every precision mode, small (under 10 MFLOP, 2.4 MB of
// weights / 3 MB of rows at bert-base bs8) and deterministic: every sum has a fixed order and no
// floating-point atomic, so two runs give the same bits.
#include "row_util.hpp"
#include "spi_kernels.hpp"

#include <stdexcept>
#include <string>

namespace spi {
namespace {

// Four consecutive floats: one 16-byte load where the caller established alignment, else four.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* p) {
  if constexpr (VEC) return *reinterpret_cast<const float4*>(p);
  return float4{p[0], p[1], p[2], p[3]};
}

// Pooler: one wave per output column n.  Lane l holds the float4 groups k4 = l, l + 64, ... of the
// weight row (a coalesced 1 KiB per load instruction) and one accumulator per batch row, kPoolRows
// rows per pass over the weight row; the lanes meet in the butterfly and lane 0 stores.
// NK > 0: D = NK * 256 (BERT-base 768, BERT-large 1024), every lane holds NK groups and all of a pass's
// loads are issued before the first FMA -- the kernel is one memory round trip per wave, so the trips
// are what it costs.  NK = 0: any D, a loop over the groups.  The sums and their order are the same.
// The kernel is the dense layer y = act(h W^T + bias) over N output columns (bert_dense_rows): the pooler
// is N = D with TANH, the sequence-classification head N = labels without.
constexpr int kPoolRows = 8;

__device__ __forceinline__ float dot4(float4 x, float4 w, float acc) {
  return fmaf(x.w, w.w, fmaf(x.z, w.z, fmaf(x.y, w.y, fmaf(x.x, w.x, acc))));
}

template <bool VEC, int NK, bool TANH>
__global__ __launch_bounds__(256) void bert_pooler_kernel(const float* __restrict__ h, size_t ld,
                                                          const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ y,
                                                          int B, int D, int N) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;  // the whole wave
  const float* wr = W + (size_t)n * D;
  const int D4 = D >> 2;
  const float bn = bias[n];
  for (int b0 = 0; b0 < B; b0 += kPoolRows) {
    float acc[kPoolRows] = {};
    if constexpr (NK > 0) {
      float4 w[NK], x[kPoolRows][NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) w[j] = load4<VEC>(wr + 4 * (lane + 64 * j));
#pragma unroll
      for (int i = 0; i < kPoolRows; ++i)
#pragma unroll
        for (int j = 0; j < NK; ++j)
          x[i][j] = b0 + i < B ? load4<VEC>(h + (size_t)(b0 + i) * ld + 4 * (lane + 64 * j)) : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < kPoolRows; ++i)
#pragma unroll
        for (int j = 0; j < NK; ++j) acc[i] = dot4(x[i][j], w[j], acc[i]);
    } else {
      for (int k4 = lane; k4 < D4; k4 += 64) {
        const float4 w = load4<VEC>(wr + 4 * k4);
#pragma unroll
        for (int i = 0; i < kPoolRows; ++i)
          if (b0 + i < B) acc[i] = dot4(load4<VEC>(h + (size_t)(b0 + i) * ld + 4 * k4), w, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < kPoolRows; ++i) {
      const float t = wave_sum(acc[i]);
      if (lane == 0 && b0 + i < B) y[(size_t)(b0 + i) * N + n] = TANH ? tanhf(t + bn) : t + bn;
    }
  }
}

// Masked mean: one workgroup per (sequence b, 64-column chunk).  Thread (g, q) of 16 row groups x
// 16 column quads sums the quad over rows g, g + 16, ... (16 lanes read one row's 256 contiguous
// bytes), eight rows in flight per thread -- S = 128 is one memory round trip; a masked-out row is
// loaded beside its mask word and dropped by a select, so whatever it holds (NaN too) stays out of the
// sum.  The groups' sums and token counts meet in LDS and the first wave adds them in group order.
constexpr int kMeanGroups = 16;
constexpr int kMeanUnroll = 8;

template <bool VEC>
__global__ __launch_bounds__(256) void masked_mean_kernel(const float* __restrict__ h,
                                                          const int64_t* __restrict__ mask, float* __restrict__ y,
                                                          int S, int D) {
  __shared__ float part[kMeanGroups][64];
  __shared__ float cnt[kMeanGroups];
  const int b = blockIdx.y, c0 = blockIdx.x * 64;
  const int g = threadIdx.x >> 4, q = threadIdx.x & 15;
  const float* col = h + (size_t)b * S * D + c0 + 4 * q;
  const int64_t* mb = mask ? mask + (size_t)b * S : nullptr;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  for (int s0 = g; s0 < S; s0 += kMeanGroups * kMeanUnroll) {
    float4 v[kMeanUnroll];
    bool on[kMeanUnroll];
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) {
      const int s = s0 + u * kMeanGroups;
      on[u] = s < S && (!mb || mb[s] != 0);
      v[u] = float4{0.f, 0.f, 0.f, 0.f};
      if (s < S) v[u] = load4<VEC>(col + (size_t)s * D);  // does not wait for the mask: dropped below
    }
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) {
      if (!on[u]) v[u] = float4{0.f, 0.f, 0.f, 0.f};
      n += on[u] ? 1.f : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) {
      acc.x += v[u].x;
      acc.y += v[u].y;
      acc.z += v[u].z;
      acc.w += v[u].w;
    }
  }
  part[g][4 * q + 0] = acc.x;
  part[g][4 * q + 1] = acc.y;
  part[g][4 * q + 2] = acc.z;
  part[g][4 * q + 3] = acc.w;
  if (q == 0) cnt[g] = n;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f, c = 0.f;
#pragma unroll
    for (int gg = 0; gg < kMeanGroups; ++gg) {
      t += part[gg][threadIdx.x];
      c += cnt[gg];
    }
    y[(size_t)b * D + c0 + threadIdx.x] = t / fmaxf(c, 1e-9f);
  }
}

void check_dims(const char* op, int B, int D) {
  if (B < 1) throw std::invalid_argument(std::string(op) + ": B >= 1");
  if (D < 64 || D % 64 != 0 || D > 1024) throw std::invalid_argument(std::string(op) + ": D a multiple of 64, <= 1024");
}

template <bool TANH>
void launch_dense_rows(const float* h, size_t ld, const float* W, const float* bias, float* y, int B, int D, int N,
                       hipStream_t s) {
  const dim3 grid((N + 3) / 4);
  const bool vec = aligned(h, 16) && aligned(W, 16) && ld % 4 == 0;
  if (vec && D == 768)
    SPI_LAUNCH((bert_pooler_kernel<true, 3, TANH>), grid, dim3(256), 0, s, h, ld, W, bias, y, B, D, N);
  else if (vec && D == 1024)
    SPI_LAUNCH((bert_pooler_kernel<true, 4, TANH>), grid, dim3(256), 0, s, h, ld, W, bias, y, B, D, N);
  else if (vec)
    SPI_LAUNCH((bert_pooler_kernel<true, 0, TANH>), grid, dim3(256), 0, s, h, ld, W, bias, y, B, D, N);
  else
    SPI_LAUNCH((bert_pooler_kernel<false, 0, TANH>), grid, dim3(256), 0, s, h, ld, W, bias, y, B, D, N);
}

}  // namespace

void bert_dense_rows(const float* h, size_t ld, const float* W, const float* bias, float* y, int B, int D, int N,
                     bool tanh_act, hipStream_t s) {
  check_dims("bert_dense_rows", B, D);
  if (ld < (size_t)D) throw std::invalid_argument("bert_dense_rows: ld >= D");
  if (N < 1 || N > 1024) throw std::invalid_argument("bert_dense_rows: 1 <= N <= 1024");
  if (tanh_act)
    launch_dense_rows<true>(h, ld, W, bias, y, B, D, N, s);
  else
    launch_dense_rows<false>(h, ld, W, bias, y, B, D, N, s);
}

void bert_pooler(const float* h, size_t ld, const float* W, const float* bias, float* y, int B, int D,
                 hipStream_t s) {
  check_dims("bert_pooler", B, D);
  if (ld < (size_t)D) throw std::invalid_argument("bert_pooler: ld >= D");
  launch_dense_rows<true>(h, ld, W, bias, y, B, D, D, s);
}

void masked_mean(const float* h, const int64_t* mask, float* y, int B, int S, int D, hipStream_t s) {
  check_dims("masked_mean", B, D);
  if (S < 1) throw std::invalid_argument("masked_mean: S >= 1");
  if (B > 65535) throw std::invalid_argument("masked_mean: B <= 65535");
  const dim3 grid(D / 64, B);
  if (aligned(h, 16))
    SPI_LAUNCH((masked_mean_kernel<true>), grid, dim3(256), 0, s, h, mask, y, S, D);
  else
    SPI_LAUNCH((masked_mean_kernel<false>), grid, dim3(256), 0, s, h, mask, y, S, D);
}

}  // namespace spi
