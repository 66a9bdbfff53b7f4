// The row-LayerNorm family (gfx950): LayerNorm of fp32 rows and of two-plane fp16 rows, the BERT
// embedding gather + LayerNorm, and the attention-mask bias the embedding also writes.  One wave per
// row, two-pass fp32 statistics in registers; HBM (latency) bound.
#include "../../include/spi_codelet.h"
#include "row_util.hpp"
#include "spi_kernels.hpp"

#include <stdexcept>
#include <type_traits>

namespace spi {
namespace {

// One wave per row, D <= 64*16.  Two-pass mean/variance in fp32 registers.
template <typename T, int VPL>
__device__ __forceinline__ void ln_row(const float (&v)[VPL], int D, const float* g,
                                       const float* b, float eps, float* yf, T* yt,
                                       int lane) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) s += v[j];
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < D) {
      const float t = v[j] - mean;
      q += t * t;
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < D) {
      const float o = (v[j] - mean) * rstd * g[c] + b[c];
      if (yf) yf[c] = o;
      if (yt) yt[c] = cvt<T>(o);
    }
  }
}

// The vector form for D = NV * 256 (BERT-base 768, ViT-L 1024): lane l holds NV float4 groups of 4
// columns (c = 4 (64 j + l)), so a row moves as 16-byte loads and stores (fp16 copies as 8-byte
// stores) -- a quarter of the scalar form's memory instructions.  Group j of a row of float4s:
__device__ __forceinline__ int ln_group(int j, int lane) { return j * 64 + lane; }

// gamma / beta are issued with the row, not after the two reductions: one memory round trip
// fewer on the wave's dependent chain (the kernel is one such chain per row)
template <int NV>
__device__ __forceinline__ void ln_load_gb(const float* g, const float* b, int lane, float4 (&gg)[NV],
                                           float4 (&bb)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    gg[j] = reinterpret_cast<const float4*>(g)[ln_group(j, lane)];
    bb[j] = reinterpret_cast<const float4*>(b)[ln_group(j, lane)];
  }
}

// Normalise and store one row, `row_off` elements into the outputs: fp32 to yf and / or T to yt
// (either may be null; the tests are on the kernel's arguments, so they are scalar branches).
template <typename T, int NV>
__device__ __forceinline__ void ln_store_vec(const float4 (&v)[NV], float mean, float rstd, const float4 (&gg)[NV],
                                             const float4 (&bb)[NV], float* yf, T* yt, size_t row_off, int lane) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float o[4] = {(v[j].x - mean) * rstd * gg[j].x + bb[j].x, (v[j].y - mean) * rstd * gg[j].y + bb[j].y,
                        (v[j].z - mean) * rstd * gg[j].z + bb[j].z, (v[j].w - mean) * rstd * gg[j].w + bb[j].w};
    if (yf) store4(yf + row_off, o, ln_group(j, lane));
    if (yt) store4(yt + row_off, o, ln_group(j, lane));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, int ldx,
                                                        const float* g, const float* b,
                                                        float* yf, T* yt, int ldy,
                                                        int rows, int D, float eps) {
  constexpr int VPL = 16;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * ldx;
  float v[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < D ? xr[c] : 0.f;
  }
  ln_row<T, VPL>(v, D, g, b, eps, yf ? yf + (size_t)row * ldy : nullptr,
                 yt ? yt + (size_t)row * ldy : nullptr, lane);
}

// LayerNorm rows of D = NV * 256 in the vector form.
template <typename T, int NV>
__global__ __launch_bounds__(256) void layernorm_vec_kernel(const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ g,
                                                            const float* __restrict__ b, float* yf, T* yt,
                                                            int ldy, int rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * ldx);
  float4 v[NV], gg[NV], bb[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = xr[ln_group(j, lane)];
  ln_load_gb(g, b, lane, gg, bb);
  // the statistics stay spelled out in the kernel (here and in bert_embed_vec_kernel): inside a shared
  // function the compiler fuses other multiply-add pairs of the second pass, which changes yf's bits
  constexpr int D = NV * 256;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float a0 = v[j].x - mean, a1 = v[j].y - mean, a2 = v[j].z - mean, a3 = v[j].w - mean;
    q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  ln_store_vec(v, mean, rstd, gg, bb, yf, yt, (size_t)row * ldy, lane);
}

// LayerNorm of rows held in two fp16 planes (GemmDesc::res_planes: x = hi + lo, lo `plane`
// elements after hi) -- ViT's final class-token LayerNorm over the two-plane residual stream.
template <typename T>
__global__ __launch_bounds__(256) void layernorm_planes_kernel(const _Float16* xh, size_t plane, int ldx,
                                                               const float* g, const float* b, float* yf, T* yt,
                                                               int ldy, int rows, int D, float eps) {
  constexpr int VPL = 16;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const _Float16* xr = xh + (size_t)row * ldx;
  float v[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < D ? static_cast<float>(xr[c]) + static_cast<float>(xr[c + plane]) : 0.f;
  }
  ln_row<T, VPL>(v, D, g, b, eps, yf ? yf + (size_t)row * ldy : nullptr, yt ? yt + (size_t)row * ldy : nullptr,
                 lane);
}

// The same for D = NV * 256, the groups read as 8-byte hi and lo vectors -- the vector form of
// layernorm_vec_kernel (round 6: the scalar planes kernel ran BERT's output LayerNorm in 10.3 us
// against 4.6 for the fp32 vector one).
template <typename T, int NV>
__global__ __launch_bounds__(256) void layernorm_planes_vec_kernel(const _Float16* __restrict__ xh, size_t plane,
                                                                   int ldx, const float* __restrict__ g,
                                                                   const float* __restrict__ b, float* yf, T* yt,
                                                                   int ldy, int rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  constexpr int D = NV * 256;
  const half4* xr = reinterpret_cast<const half4*>(xh + (size_t)row * ldx);
  const half4* lr = reinterpret_cast<const half4*>(xh + (size_t)row * ldx + plane);
  half4 hv[NV], lv[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    hv[j] = xr[ln_group(j, lane)];
    lv[j] = lr[ln_group(j, lane)];
  }
  float4 v[NV], gg[NV], bb[NV];
  ln_load_gb(g, b, lane, gg, bb);
  // the statistics sum a group's values one after another, not pairwise as layernorm_vec_kernel's do:
  // a different fp32 rounding, kept so that this kernel's outputs stay what they were bit for bit
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j] = float4{(float)hv[j][0] + (float)lv[j][0], (float)hv[j][1] + (float)lv[j][1],
                  (float)hv[j][2] + (float)lv[j][2], (float)hv[j][3] + (float)lv[j][3]};
    s = (((s + v[j].x) + v[j].y) + v[j].z) + v[j].w;
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    q += (v[j].x - mean) * (v[j].x - mean);
    q += (v[j].y - mean) * (v[j].y - mean);
    q += (v[j].z - mean) * (v[j].z - mean);
    q += (v[j].w - mean) * (v[j].w - mean);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  ln_store_vec(v, mean, rstd, gg, bb, yf, yt, (size_t)row * ldy, lane);
}

// The attention's additive key bias of a token with mask word m: (1 - m) * finfo(f32).min.
__device__ __forceinline__ float mask_bias_of(int64_t m) { return m != 0 ? 0.f : -3.4028234663852886e38f; }

__global__ void mask_bias_kernel(const int64_t* mask, float* bias, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    bias[i] = mask_bias_of(mask[i]);
}

// The token-type table row of embedding row `row`: the clamped segment id, or 0 without ids.
__device__ __forceinline__ size_t type_row(const int64_t* types, int row, int type_vocab) {
  if (!types) return 0;
  const int64_t t = types[row];
  return (size_t)(t < 0 ? 0 : (t >= type_vocab ? type_vocab - 1 : t));
}

// SPI_BERT_POS_FROM_IDS (RoBERTa): the position row of embedding row `row`, token s of its sequence, whose
// raw id is `id`: 1 + the non-pad ids among ids[b][0..s], or SPI_ROBERTA_PAD_ID for a pad token.  The wave
// reads its sequence's ids up to s, 64 a step, and counts each step's ballot: an exact integer that
// depends on the sequence alone -- not on B or the grid -- with no LDS, atomics or shuffles.  The trip
// count is wave-uniform (a wave owns one row), so every lane takes part in every ballot.
__device__ __forceinline__ int pos_from_ids(const int64_t* ids, int row, int s, int64_t id, int lane) {
  const int64_t* seq = ids + (row - s);
  int n = 0;
  // four steps' loads are issued together (one L2 round trip per 256 ids, not per 64): a lane past s
  // re-reads ids[b][s], inside the sequence, and its vote is dropped
  for (int c = 0; c <= s; c += 256) {
    int64_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = seq[min(c + 64 * u + lane, s)];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      n += __popcll(__ballot(c + 64 * u + lane <= s && v[u] != SPI_ROBERTA_PAD_ID));
  }
  return id != SPI_ROBERTA_PAD_ID ? SPI_ROBERTA_PAD_ID + n : SPI_ROBERTA_PAD_ID;
}

// POSIDS: the position row is pos_from_ids' instead of s; false leaves the kernel's code what it was.
template <typename T, bool POSIDS>
__global__ __launch_bounds__(256) void bert_embed_kernel(
    const int64_t* ids, const float* word, const float* pos, const float* type0,
    const float* g, const float* b, float* yf, T* yt, int B, int S, int D, int vocab,
    float eps, const int64_t* mask, float* mask_bias, const int64_t* types, int type_vocab) {
  constexpr int VPL = 16;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * S) return;
  if (mask && lane == 0) mask_bias[row] = mask_bias_of(mask[row]);
  const int s = row % S;
  int64_t id = ids[row];
  const int prow = POSIDS ? pos_from_ids(ids, row, s, id, lane) : s;
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float* w = word + (size_t)id * D;
  const float* p = pos + (size_t)prow * D;
  const float* t = type0 + type_row(types, row, type_vocab) * D;
  float v[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < D ? (w[c] + t[c]) + p[c] : 0.f;
  }
  ln_row<T, VPL>(v, D, g, b, eps, yf + (size_t)row * D, yt ? yt + (size_t)row * D : nullptr,
                 lane);
}

// The same for D = NV * 256 in the vector form, with 16-byte gathers (round 6: BERT-base's
// embedding ran 14.6 us in the loop trace, 1.7 % of C3).
template <typename T, int NV, bool POSIDS>
__global__ __launch_bounds__(256) void bert_embed_vec_kernel(const int64_t* ids, const float* __restrict__ word,
                                                             const float* __restrict__ pos,
                                                             const float* __restrict__ type0,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ b, float* yf, T* yt, int B,
                                                             int S, int vocab, float eps, const int64_t* mask,
                                                             float* mask_bias, const int64_t* types,
                                                             int type_vocab) {
  constexpr int D = NV * 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * S) return;
  if (mask && lane == 0) mask_bias[row] = mask_bias_of(mask[row]);
  const int s = row % S;
  int64_t id = ids[row];
  const int prow = POSIDS ? pos_from_ids(ids, row, s, id, lane) : s;
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* w4 = reinterpret_cast<const float4*>(word + (size_t)id * D);
  const float4* p4 = reinterpret_cast<const float4*>(pos + (size_t)prow * D);
  const float4* t4 = reinterpret_cast<const float4*>(type0 + type_row(types, row, type_vocab) * D);
  float4 v[NV], gg[NV], bb[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float4 w = w4[ln_group(j, lane)], t = t4[ln_group(j, lane)], p = p4[ln_group(j, lane)];
    v[j] = float4{(w.x + t.x) + p.x, (w.y + t.y) + p.y, (w.z + t.z) + p.z, (w.w + t.w) + p.w};
  }
  ln_load_gb(g, b, lane, gg, bb);
  float sm = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) sm += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  const float mean = wave_sum(sm) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float a0 = v[j].x - mean, a1 = v[j].y - mean, a2 = v[j].z - mean, a3 = v[j].w - mean;
    q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  ln_store_vec(v, mean, rstd, gg, bb, yf, yt, (size_t)row * D, lane);
}

// f(integral_constant<int, NV>) for the vector kernels' D = NV * 256, D = 768 or 1024.
template <typename F>
void with_nv(int D, F&& f) {
  if (D == 768)
    f(std::integral_constant<int, 3>{});
  else
    f(std::integral_constant<int, 4>{});
}

}  // namespace

void layernorm(const float* x, int ldx, const float* g, const float* b, float* yf, void* yt,
               int ldy, int rows, int D, float eps, bool f16, hipStream_t s) {
  const dim3 grid((rows + 3) / 4);
  const bool vec = (D == 768 || D == 1024) && ldx % 4 == 0 && ldy % 4 == 0 && aligned(x, 16) && aligned(g, 16) &&
                   aligned(b, 16) && (!yf || aligned(yf, 16)) && (!yt || aligned(yt, 8));
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    if (vec)
      with_nv(D, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        SPI_LAUNCH((layernorm_vec_kernel<T, NV>), grid, dim3(256), 0, s, x, ldx, g, b, yf, (T*)yt, ldy, rows, eps);
      });
    else
      SPI_LAUNCH((layernorm_kernel<T>), grid, dim3(256), 0, s, x, ldx, g, b, yf, (T*)yt, ldy, rows, D, eps);
  });
}

void layernorm_planes(const _Float16* xh, size_t plane, int ldx, const float* g, const float* b, float* yf, void* yt,
                      int ldy, int rows, int D, float eps, bool f16, hipStream_t s) {
  if (D > 1024) throw std::invalid_argument("layernorm_planes: D <= 1024");
  const dim3 grid((rows + 3) / 4);
  const bool vec = (D == 768 || D == 1024) && ldx % 4 == 0 && plane % 4 == 0 && ldy % 4 == 0 && aligned(xh, 8) &&
                   aligned(g, 16) && aligned(b, 16) && (!yf || aligned(yf, 16)) && (!yt || aligned(yt, f16 ? 8 : 16));
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    if (vec)
      with_nv(D, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        SPI_LAUNCH((layernorm_planes_vec_kernel<T, NV>), grid, dim3(256), 0, s, xh, plane, ldx, g, b, yf, (T*)yt, ldy,
                   rows, eps);
      });
    else
      SPI_LAUNCH((layernorm_planes_kernel<T>), grid, dim3(256), 0, s, xh, plane, ldx, g, b, yf, (T*)yt, ldy, rows, D,
                 eps);
  });
}

void bert_embed(const int64_t* ids, const float* word, const float* pos, const float* type0,
                const float* g, const float* b, float* yf, void* yt, int B, int S, int D,
                int vocab, float eps, bool f16, hipStream_t s, const int64_t* mask, float* mask_bias,
                const int64_t* types, int type_vocab, bool pos_from_ids) {
  // the scalar kernel stores every row through yf + row D, which is non-null past row 0 whatever yf
  // is (the vector one tests yf itself and would leave the fp32 rows unwritten)
  if (!yf) throw std::invalid_argument("bert_embed: the fp32 output yf is required");
  const dim3 grid((B * S + 3) / 4);
  const bool vec = (D == 768 || D == 1024) && aligned(word, 16) && aligned(pos, 16) && aligned(type0, 16) &&
                   aligned(g, 16) && aligned(b, 16) && aligned(yf, 16) && (!yt || aligned(yt, f16 ? 8 : 16));
  auto launch = [&](auto t, auto posids) {
    using T = decltype(t);
    constexpr bool P = decltype(posids)::value;
    if (vec)
      with_nv(D, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        SPI_LAUNCH((bert_embed_vec_kernel<T, NV, P>), grid, dim3(256), 0, s, ids, word, pos, type0, g, b, yf, (T*)yt, B,
                   S, vocab, eps, mask, mask_bias, types, type_vocab);
      });
    else
      SPI_LAUNCH((bert_embed_kernel<T, P>), grid, dim3(256), 0, s, ids, word, pos, type0, g, b, yf, (T*)yt, B, S, D,
                 vocab, eps, mask, mask_bias, types, type_vocab);
  };
  with_type(f16, [&](auto t) {
    if (pos_from_ids)
      launch(t, std::true_type{});
    else
      launch(t, std::false_type{});
  });
}

void mask_to_bias(const int64_t* mask, float* bias, int n, hipStream_t s) {
  SPI_LAUNCH(mask_bias_kernel, dim3(grid_for(n)), dim3(256), 0, s, mask, bias, n);
}

}  // namespace spi
