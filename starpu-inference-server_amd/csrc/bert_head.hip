// BERT token-level task heads (gfx950): the dense layer of a token tagger (logits [T][L]) or of an
// extractive-QA span scorer (start / end logits [T] each) over the last hidden state, optionally with the
// last LayerNorm taken along so the hidden state never reaches memory.  fp32 in every precision mode, no
// MFMA (L <= 64: under 0.15 GFLOP at bert-base bs8) and deterministic: every sum has a fixed order that
// does not depend on T and there is no floating-point atomic, so a row's logits are the same bits alone
// or inside any batch.
#include "row_util.hpp"
#include "spi_kernels.hpp"

#include <stdexcept>
#include <string>

namespace spi {
namespace {

// A wave owns kHeadRows consecutive token rows and holds them in registers (a row per register group,
// as layernorm.hip holds one), so each weight row it loads serves all of them; a workgroup of four
// waves owns 16 rows.  The weights (at most 64 x 1024 fp32 = 256 KB) are read by every wave and stay in L2.
constexpr int kHeadRows = 4;
constexpr int kHeadBlockRows = 4 * kHeadRows;

// The per-lane partial sums of four rows -> each row's total over the wave, in 7 cross-lane steps
// rather than four butterflies of 6: at the 32- and 16-lane steps a lane keeps half of its values and
// hands the other half to its partner.  Lane class (bit 5, bit 4) ends with row 2 * bit5 + bit4, every
// lane of the class holding the total.  Each total is the butterfly's tree over the 64 lanes (an
// addition of the same two operands at every node, whichever row slot), so it has one order.
__device__ __forceinline__ float reduce_rows4(float a0, float a1, float a2, float a3, int lane) {
  const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0;
  float k0 = h32 ? a2 : a0, k1 = h32 ? a3 : a1;
  k0 += __shfl_xor(h32 ? a0 : a2, 32, 64);
  k1 += __shfl_xor(h32 ? a1 : a3, 32, 64);
  float k = h16 ? k1 : k0;
  k += __shfl_xor(h16 ? k0 : k1, 16, 64);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
  return k;
}

// Values per lane: NV float4 groups (D = NV * 256; element e is column 4 (64 (e / 4) + lane) + e % 4), or
// in the generic form (NV = 0) 16 scalars, element e column lane + 64 e, present while that is below D.
template <int NV>
struct HeadLane {
  static constexpr int NE = NV > 0 ? 4 * NV : 16;
};

// D floats at p into v (columns past D: 0).  NV > 0 needs p 16-byte aligned.
template <int NV>
__device__ __forceinline__ void load_f32(const float* p, int D, int lane, float (&v)[HeadLane<NV>::NE]) {
  if constexpr (NV > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const float4 t = reinterpret_cast<const float4*>(p)[64 * j + lane];
      v[4 * j + 0] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = lane + 64 * e < D ? p[lane + 64 * e] : 0.f;
  }
}

// The same from two fp16 planes: hi at p, lo `plane` elements on (layernorm_planes' sum, hi + lo in fp32).
// NV > 0 needs p and p + plane 8-byte aligned.
template <int NV>
__device__ __forceinline__ void load_planes(const _Float16* p, size_t plane, int D, int lane,
                                            float (&v)[HeadLane<NV>::NE]) {
  if constexpr (NV > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const half4 h = reinterpret_cast<const half4*>(p)[64 * j + lane];
      const half4 l = reinterpret_cast<const half4*>(p + plane)[64 * j + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * j + i] = (float)h[i] + (float)l[i];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = lane + 64 * e;
      v[e] = c < D ? (float)p[c] + (float)p[c + plane] : 0.f;
    }
  }
}

// LayerNorm of the row in registers: two-pass fp32 statistics over the wave, then (v - mean) rstd g + b
// with the products spelled out, so every row slot rounds alike.  Columns past D stay 0.
template <int NV>
__device__ __forceinline__ void normalise_row(float (&v)[HeadLane<NV>::NE], const float (&gg)[HeadLane<NV>::NE],
                                              const float (&bb)[HeadLane<NV>::NE], int D, float eps, int lane) {
  constexpr int NE = HeadLane<NV>::NE;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NE; ++e) s += v[e];
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const float a = (NV > 0 || lane + 64 * e < D) ? v[e] - mean : 0.f;
    q = fmaf(a, a, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int e = 0; e < NE; ++e)
    v[e] = (NV > 0 || lane + 64 * e < D) ? fmaf((v[e] - mean) * rstd, gg[e], bb[e]) : 0.f;
}

// SRC (HeadSrc): what x holds.  Grid: one workgroup per 16 rows.
template <int SRC, int NV>
__global__ __launch_bounds__(256) void bert_token_head_kernel(const void* __restrict__ x, size_t plane,
                                                              const float* __restrict__ g,
                                                              const float* __restrict__ b, float eps,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ y0,
                                                              float* __restrict__ y1, int T, int D, int L) {
  constexpr int NE = HeadLane<NV>::NE;
  const int lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * kHeadBlockRows + (threadIdx.x >> 6) * kHeadRows;
  if (row0 >= T) return;  // the whole wave
  float v[kHeadRows][NE];
#pragma unroll
  for (int r = 0; r < kHeadRows; ++r) {
    const int row = row0 + r;
    if (row < T) {
      if constexpr (SRC == kHeadSrcPlanes)
        load_planes<NV>(static_cast<const _Float16*>(x) + (size_t)row * D, plane, D, lane, v[r]);
      else
        load_f32<NV>(static_cast<const float*>(x) + (size_t)row * D, D, lane, v[r]);
    } else {
#pragma unroll
      for (int e = 0; e < NE; ++e) v[r][e] = 0.f;  // never stored
    }
  }
  float w[NE];
  load_f32<NV>(W, D, lane, w);  // label 0's weights, in flight beside the rows
  if constexpr (SRC != kHeadSrcRows) {
    float gg[NE], bb[NE];
    load_f32<NV>(g, D, lane, gg);
    load_f32<NV>(b, D, lane, bb);
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) normalise_row<NV>(v[r], gg, bb, D, eps, lane);
  }
  // this lane's row after reduce_rows4, and its label within each group of 16
  const int row = row0 + ((lane >> 5) & 1) * 2 + ((lane >> 4) & 1);
  const int lj = lane & 15;
  float o = 0.f;
  for (int l = 0; l < L; ++l) {
    float wn[NE];
    if (l + 1 < L) load_f32<NV>(W + (size_t)(l + 1) * D, D, lane, wn);  // one label ahead
    float acc[kHeadRows] = {};
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[r] = fmaf(v[r][e], w[e], acc[r]);
    const float k = reduce_rows4(acc[0], acc[1], acc[2], acc[3], lane);
    if (lj == (l & 15)) o = k;
    if ((l & 15) == 15 || l == L - 1) {  // 16 labels of a row leave as one 64-byte store
      const int lab = (l & ~15) + lj;
      if (row < T && lab < L) {
        const float out = o + bias[lab];
        if (y1)
          (lab == 0 ? y0 : y1)[row] = out;
        else
          y0[(size_t)row * L + lab] = out;
      }
    }
    if (l + 1 < L) {
#pragma unroll
      for (int e = 0; e < NE; ++e) w[e] = wn[e];
    }
  }
}

template <int SRC>
void launch_head(bool vec, const void* x, size_t plane, const float* g, const float* b, float eps, const float* W,
                 const float* bias, float* y0, float* y1, int T, int D, int L, hipStream_t s) {
  const dim3 grid((T + kHeadBlockRows - 1) / kHeadBlockRows);
  if (vec && D == 768)
    SPI_LAUNCH((bert_token_head_kernel<SRC, 3>), grid, dim3(256), 0, s, x, plane, g, b, eps, W, bias, y0, y1, T, D, L);
  else if (vec && D == 1024)
    SPI_LAUNCH((bert_token_head_kernel<SRC, 4>), grid, dim3(256), 0, s, x, plane, g, b, eps, W, bias, y0, y1, T, D, L);
  else
    SPI_LAUNCH((bert_token_head_kernel<SRC, 0>), grid, dim3(256), 0, s, x, plane, g, b, eps, W, bias, y0, y1, T, D, L);
}

}  // namespace

void bert_token_head(int src, const void* x, size_t plane, const float* g, const float* b, float eps, const float* W,
                     const float* bias, float* y0, float* y1, int T, int D, int L, hipStream_t s) {
  const std::string op = "bert_token_head: ";
  if (src < kHeadSrcRows || src > kHeadSrcPlanes) throw std::invalid_argument(op + "source kind 0, 1 or 2");
  if (!x || !W || !bias || !y0) throw std::invalid_argument(op + "x, W, bias and y0 are required");
  if (T < 1) throw std::invalid_argument(op + "T >= 1");
  if (D < 64 || D % 64 != 0 || D > 1024) throw std::invalid_argument(op + "D a multiple of 64, <= 1024");
  if (L < 1 || L > 64) throw std::invalid_argument(op + "1 <= L <= 64");
  if (y1 && L != 2) throw std::invalid_argument(op + "split outputs need L == 2");
  if (src != kHeadSrcRows && (!g || !b)) throw std::invalid_argument(op + "pre-LayerNorm rows need gamma and beta");
  if (src == kHeadSrcPlanes && plane < (size_t)T * D) throw std::invalid_argument(op + "plane >= T * D");
  // the vector forms: 16-byte groups of fp32 (8-byte groups of the fp16 planes), rows D apart
  bool vec = (D == 768 || D == 1024) && aligned(W, 16);
  if (src == kHeadSrcPlanes)
    vec = vec && aligned(x, 8) && plane % 4 == 0;
  else
    vec = vec && aligned(x, 16);
  if (src != kHeadSrcRows) vec = vec && aligned(g, 16) && aligned(b, 16);
  if (src == kHeadSrcRows)
    launch_head<kHeadSrcRows>(vec, x, plane, g, b, eps, W, bias, y0, y1, T, D, L, s);
  else if (src == kHeadSrcPreLn)
    launch_head<kHeadSrcPreLn>(vec, x, plane, g, b, eps, W, bias, y0, y1, T, D, L, s);
  else
    launch_head<kHeadSrcPlanes>(vec, x, plane, g, b, eps, W, bias, y0, y1, T, D, L, s);
}

}  // namespace spi
