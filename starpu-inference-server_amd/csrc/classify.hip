// Classification outputs of the image replicas (gfx950): softmax and top-k of fp32 logits rows, every
// selected output of a batch in one launch.  One workgroup of four waves per row.  The row is staged in
// LDS once and never modified; all three results are read from it:
//   probabilities  p[j] = exp(x[j] - max) / sum_j exp(x[j] - max), fp32, with one fixed summation order
//                  (a thread's elements in index order, a wave's 64 sums by a fixed tree of DPP
//                  moves, the four waves' sums in wave order): no atomic, the same bits from run to run;
//   top-k          k rounds of a workgroup-wide arg-max over the total order "logit descending, then
//                  class index ascending, 0.0 == -0.0" (torch.sort(descending=True, stable=True)).
//                  Every element has a distinct 64-bit rank in that order, so round r looks for the
//                  largest rank below round r - 1's winner: nothing is retired or written back.
// -inf logits give probability 0; +inf or NaN logits give unspecified results.
#include "spi_kernels.hpp"

#include <stdexcept>

namespace spi {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
// The row's first kRowCap floats live in LDS (with the reduction scratch: under the 64 KiB a workgroup
// may declare); the up to 128 floats past them of a row longer than that are read through the cache.
constexpr int kRowCap = 16384 - 128;

struct Row {
  const float* lds;
  const float* glob;
  __device__ __forceinline__ float operator[](int j) const { return j < kRowCap ? lds[j] : glob[j]; }
};

// Rank of (logit, index) in the top-k order as one unsigned word: larger is better.  The float's bits
// made monotone (negative: all bits flipped, else the sign bit set; -0.0 counts as 0.0), then the
// index complemented so the lower index wins among equal logits.  -inf ranks 0x007fffff, above zero.
__device__ __forceinline__ unsigned long long rank_of(float v, int j) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  const unsigned key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)key << 32) | (unsigned)~(unsigned)j;
}

// Wave-64 reductions by DPP moves (register to register, no LDS crossbar): an inclusive scan inside each
// row of 16 lanes (row_shr 1, 2, 4, 8), then lane 15 of each row into the next row (row_bcast:15) and lane
// 31 into the upper half (row_bcast:31); lane 63 holds the result and every lane reads it.  A lane without
// a source lane keeps `old`, the operation's identity.  The order of a sum is fixed.
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned old, unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xf, 0xf, false);
}
constexpr int kShr1 = 0x111, kShr2 = 0x112, kShr4 = 0x114, kShr8 = 0x118, kBcast15 = 0x142, kBcast31 = 0x143;

template <int CTRL>
__device__ __forceinline__ float max_step(float v) {
  return fmaxf(v, __uint_as_float(dpp<CTRL>(__float_as_uint(v), __float_as_uint(v))));
}
__device__ __forceinline__ float wave_max(float v) {
  v = max_step<kShr1>(v), v = max_step<kShr2>(v), v = max_step<kShr4>(v), v = max_step<kShr8>(v);
  v = max_step<kBcast15>(v), v = max_step<kBcast31>(v);
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}

template <int CTRL>
__device__ __forceinline__ float sum_step(float v) {
  return v + __uint_as_float(dpp<CTRL>(0u, __float_as_uint(v)));
}
__device__ __forceinline__ float wave_sum(float v) {
  v = sum_step<kShr1>(v), v = sum_step<kShr2>(v), v = sum_step<kShr4>(v), v = sum_step<kShr8>(v);
  v = sum_step<kBcast15>(v), v = sum_step<kBcast31>(v);
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}

template <int CTRL>
__device__ __forceinline__ unsigned long long rank_step(unsigned long long v) {
  const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
  const unsigned long long other = ((unsigned long long)dpp<CTRL>(hi, hi) << 32) | dpp<CTRL>(lo, lo);
  return other > v ? other : v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  v = rank_step<kShr1>(v), v = rank_step<kShr2>(v), v = rank_step<kShr4>(v), v = rank_step<kShr8>(v);
  v = rank_step<kBcast15>(v), v = rank_step<kBcast31>(v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, 63), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// The one expression of a probability: the probability output and the top-k values come through it,
// so they hold the same bits.
__device__ __forceinline__ float prob_of(float v, float mx, float sum) { return expf(v - mx) / sum; }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void softmax_topk_kernel(const float* __restrict__ x, size_t ldx,
                                                                float* __restrict__ probs, float* __restrict__ topv,
                                                                long long* __restrict__ topi, int N, int k,
                                                                int topk_probs) {
  __shared__ __attribute__((aligned(16))) float xs[kRowCap];
  __shared__ float red_max[kWaves], red_sum[kWaves];
  __shared__ unsigned long long red_rank[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = blockIdx.x;
  const float* xg = x + row * ldx;
  const int NL = N < kRowCap ? N : kRowCap;  // floats staged in LDS
  if constexpr (VEC) {
    const int n4 = NL >> 2;
    for (int j4 = tid; j4 < n4; j4 += kThreads)
      *reinterpret_cast<float4*>(&xs[4 * j4]) = *reinterpret_cast<const float4*>(xg + 4 * j4);
    for (int j = 4 * n4 + tid; j < NL; j += kThreads) xs[j] = xg[j];
  } else {
    for (int j = tid; j < NL; j += kThreads) xs[j] = xg[j];
  }
  __syncthreads();
  const Row r{xs, xg};

  float mx = 0.f, sum = 1.f;
  if (probs || topk_probs) {
    float m = -INFINITY;
    for (int j = tid; j < N; j += kThreads) m = fmaxf(m, r[j]);
    m = wave_max(m);
    if (lane == 0) red_max[wave] = m;
    __syncthreads();
    mx = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
    float s = 0.f;
    for (int j = tid; j < N; j += kThreads) s += expf(r[j] - mx);
    s = wave_sum(s);
    if (lane == 0) red_sum[wave] = s;
    __syncthreads();
    sum = ((red_sum[0] + red_sum[1]) + red_sum[2]) + red_sum[3];
    if (probs) {
      float* p = probs + row * (size_t)N;
      for (int j = tid; j < N; j += kThreads) p[j] = prob_of(r[j], mx, sum);
    }
  }

  if (k > 0) {
    unsigned long long bound = ~0ull;  // above every rank of a non-NaN logit
    int mine = 0;                      // thread t keeps round t's winner
    for (int round = 0; round < k; ++round) {
      unsigned long long best = 0;  // below every rank
      for (int j = tid; j < N; j += kThreads) {
        const unsigned long long c = rank_of(r[j], j);
        if (c < bound && c > best) best = c;
      }
      best = wave_max(best);
      unsigned long long* slot = red_rank[round & 1];  // two slots: one barrier per round
      if (lane == 0) slot[wave] = best;
      __syncthreads();
      const unsigned long long a = slot[0] > slot[1] ? slot[0] : slot[1];
      const unsigned long long b = slot[2] > slot[3] ? slot[2] : slot[3];
      bound = a > b ? a : b;
      if (round == tid) mine = (int)~(unsigned)bound;
    }
    if (tid < k) {
      // NaN logits can leave a round without a candidate (index past the row): clamp, results unspecified
      mine = (unsigned)mine < (unsigned)N ? mine : N - 1;
      const float v = r[mine];
      topv[row * (size_t)k + tid] = topk_probs ? prob_of(v, mx, sum) : v;
      topi[row * (size_t)k + tid] = mine;
    }
  }
}

}  // namespace

void softmax_topk(const float* x, size_t ldx, float* probs, float* topv, int64_t* topi, int B, int N, int k,
                  bool topk_probs, hipStream_t s) {
  if (!x) throw std::invalid_argument("softmax_topk: x is null");
  if (B < 1) throw std::invalid_argument("softmax_topk: B >= 1");
  if (N < 1 || N > kSoftmaxTopkMaxN) throw std::invalid_argument("softmax_topk: 1 <= N <= 16384");
  if (ldx < (size_t)N) throw std::invalid_argument("softmax_topk: ldx >= N");
  if ((topv == nullptr) != (topi == nullptr))
    throw std::invalid_argument("softmax_topk: top-k values and indices come both or neither");
  if (!probs && !topv) throw std::invalid_argument("softmax_topk: no output selected");
  if (!topv) {
    if (k != 0 || topk_probs) throw std::invalid_argument("softmax_topk: k and topk_probs need the top-k outputs");
  } else if (k < 1 || k > kSoftmaxTopkMaxK || k > N) {
    throw std::invalid_argument("softmax_topk: 1 <= k <= min(N, 64)");
  }
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ldx % 4 == 0;
  long long* ti = reinterpret_cast<long long*>(topi);
  if (vec)
    SPI_LAUNCH((softmax_topk_kernel<true>), dim3(B), dim3(kThreads), 0, s, x, ldx, probs, topv, ti, N, k,
               topk_probs ? 1 : 0);
  else
    SPI_LAUNCH((softmax_topk_kernel<false>), dim3(B), dim3(kThreads), 0, s, x, ldx, probs, topv, ti, N, k,
               topk_probs ? 1 : 0);
}

}  // namespace spi
