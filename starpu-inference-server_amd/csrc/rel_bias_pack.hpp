// Host-side layout of the relative-bias attention variant (the REL instances of attention.hip): the operand is
// one fp32 generator row per head, rows[heads][ld], whose entry half + d is the bias of every (query, key) pair
// with key - query = d -- a Toeplitz bias, so no [S][S] matrix ever exists.  MPNet's rows come from its bucket
// table (HF's MPNetEncoder.relative_position_bucket, restated here); the kernel knows nothing of buckets.  Plain
// C++, shared by the packer (model_pack.cpp), the forward and the op entry points.
#pragma once
#include <cmath>
#include <cstddef>

namespace spi {

// The variant's served set: 64-wide heads, sequences of at most 512 tokens (the LDS slice is sized for them).
constexpr int kRelHeadDim = 64, kRelMaxSeq = 512;
// HF's MPNet never passes max_distance: every checkpoint uses relative_position_bucket's default.
constexpr int kMpnetMaxDistance = 128;
inline bool rel_buckets_supported(int nb) { return nb >= 4 && nb <= 128 && nb % 4 == 0; }
// Row stride for sequences up to P: 2 P - 1 distances, padded to whole 16-byte chunks.
inline int rel_rows_ld(int P) { return (2 * P - 1 + 3) & ~3; }

// HF's bucket of d = key - query: n = -d picks the table's upper half when negative (the key lies behind the
// query); |n| below nb / 4 keeps its own bucket, larger distances share logarithmic ones up to max_distance,
// the last bucket taking all beyond.  The log is evaluated in fp32 and the quotient truncated, as HF does.
inline int rel_bucket(int d, int nb, int max_distance) {
  const int half = nb / 2, exact = half / 2;
  int n = -d, ret = 0;
  if (n < 0) ret = half, n = -n;
  if (n < exact) return ret + n;
  const float v = std::log((float)n / (float)exact) / (float)std::log((double)max_distance / exact) * (float)(half - exact);
  const int large = exact + (int)v;
  return ret + (large < half - 1 ? large : half - 1);
}

// table [nb][heads] -> dst [heads][rel_rows_ld(P)]: entry (h, d + P - 1) = table[bucket(d)][h], the padding zero.
inline void rel_bias_rows(const float* table, int nb, int max_distance, int heads, int P, float* dst) {
  const int ld = rel_rows_ld(P);
  for (int h = 0; h < heads; ++h) {
    float* row = dst + (size_t)h * ld;
    for (int i = 0; i < ld; ++i)
      row[i] = i < 2 * P - 1 ? table[(size_t)rel_bucket(i - (P - 1), nb, max_distance) * heads + h] : 0.f;
  }
}

}  // namespace spi
