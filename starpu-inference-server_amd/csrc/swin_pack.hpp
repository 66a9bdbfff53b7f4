// Host-side layouts of the Swin kernels (window_attn.hip, s2d_ln in dwconv_ln.hip): the supported window
// sizes, the relative-position bias expanded and packed for the attention kernel's accumulator layout, and
// the shift rule of a block.  Plain C++, shared by the packer (model_pack.cpp), the plan and the op entry points.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

namespace spi {

// ws x ws windows of N = ws^2 <= 64 tokens: the kernel's one 64-key tile.  7 is the production case.
constexpr int kWinMin = 2, kWinMax = 8, kWinSlots = 64, kWinHeadDim = 32;
inline bool window_supported(int ws) { return ws >= kWinMin && ws <= kWinMax; }
// fp32 values of one head's packed bias: [16 key quads][64 queries][4 keys].
constexpr size_t kWinBiasHead = (size_t)kWinSlots * kWinSlots;
// s2d_ln's rows: 4 C columns, C a multiple of 32, 4 C <= 2048 (eight float4 per lane).
constexpr int kS2dMaxRow = 2048;
inline bool s2d_ln_supported(int C) { return C >= 32 && C % 32 == 0 && 4 * C <= kS2dMaxRow; }

// torchvision's relative_position_index, recomputed from ws: tokens q = (qy, qx), k = (ky, kx) of a window
// -> row (qy - ky + ws - 1) (2 ws - 1) + (qx - kx + ws - 1) of relative_position_bias_table.
inline int window_rel_index(int ws, int q, int k) {
  return (q / ws - k / ws + ws - 1) * (2 * ws - 1) + (q % ws - k % ws + ws - 1);
}

// relative_position_bias_table [(2 ws - 1)^2][heads] -> the kernel's order, dst [heads][16][64][4] fp32:
// value (head, query q, key k) at ((head 16 + k / 4) 64 + q) 4 + k % 4 -- a lane of the kernel owns one query
// and holds the scores of keys 4 g .. 4 g + 3 per accumulator, so its four biases are one 16-byte load and
// the 16 queries of a lane group lie contiguous.  Keys N .. 63 hold -inf (they drop out of the softmax through
// the bias), query slots N .. 63 hold 0 on the live keys (their scores stay finite; nothing is stored for them).
inline void window_bias_pack(const float* table, int ws, int heads, float* dst) {
  const int N = ws * ws;
  for (int h = 0; h < heads; ++h)
    for (int k = 0; k < kWinSlots; ++k)
      for (int q = 0; q < kWinSlots; ++q) {
        float v = 0.f;
        if (k >= N) v = -INFINITY;
        else if (q < N) v = table[(size_t)window_rel_index(ws, q, k) * heads + h];
        dst[(((size_t)h * 16 + k / 4) * kWinSlots + q) * 4 + k % 4] = v;
      }
}

// Swin v2: the bias table is not learnt but computed, 16 sigmoid(cpb_mlp(coords)) -- torchvision's
// relative_coords_table and cpb_mlp restated.  Row (dy + ws - 1)(2 ws - 1) + (dx + ws - 1), dy, dx in
// -(ws - 1) .. ws - 1 (window_rel_index's rows), has the coordinates t = 8 d / (ws - 1) mapped to
// sign(t) log2(|t| + 1) / 3; the MLP is Linear(2, hidden) + bias, ReLU, Linear(hidden, heads) without bias.
// w0 [hidden][2], b0 [hidden], w2 [heads][hidden] -> table [(2 ws - 1)^2][heads] for window_bias_pack.  Double
// accumulation, one rounding at the end.  ws >= 2.
constexpr int kCpbHidden = 512;  // torchvision's cpb_mlp width
inline void window_cpb_table(const float* w0, const float* b0, const float* w2, int hidden, int ws, int heads, float* table) {
  const int side = 2 * ws - 1;
  auto coord = [&](int d) {
    const double t = 8.0 * d / (ws - 1);
    return (t < 0 ? -1.0 : t > 0 ? 1.0 : 0.0) * std::log2(std::fabs(t) + 1.0) / 3.0;
  };
  for (int iy = 0; iy < side; ++iy)
    for (int ix = 0; ix < side; ++ix) {
      const double cy = coord(iy - (ws - 1)), cx = coord(ix - (ws - 1));
      for (int h = 0; h < heads; ++h) {
        double acc = 0;
        for (int j = 0; j < hidden; ++j) {
          const double a = (double)w0[2 * j] * cy + (double)w0[2 * j + 1] * cx + (double)b0[j];
          if (a > 0) acc += a * (double)w2[(size_t)h * hidden + j];
        }
        table[((size_t)iy * side + ix) * heads + h] = (float)(16.0 / (1.0 + std::exp(-acc)));
      }
    }
}
// tau_h = exp(min(logit_scale_h, log 100)): torchvision's clamp(logit_scale, max = log 100).exp().
inline float window_cos_tau(float logit_scale) { return std::exp(std::min(logit_scale, (float)std::log(100.0))); }

// Block i of a stage over a square map of side H: shift 0 for even i, ws / 2 for odd i, forced to 0 where the
// map equals the window (torchvision zeroes the shift of an axis no longer than the window).
inline int window_block_shift(int i, int ws, int H) { return (i % 2 && H > ws) ? ws / 2 : 0; }

}  // namespace spi
