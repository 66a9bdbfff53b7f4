// Host-side layouts of the ConvNeXt kernels (dwconv_ln.hip): the supported channel counts, the
// depthwise 7x7 weight repack and the 2x2 / stride 2 downsample weight's space-to-depth column order.
// Plain C++, shared by the packer (model_pack.cpp) and the op entry points (ops.cpp).
#pragma once
#include <cstddef>

namespace spi {

// C a multiple of 32 from 32 to 1536: convnext_tiny / small (96 .. 768), base (128 .. 1024), large (192 .. 1536).
constexpr int kDwconvMinC = 32, kDwconvMaxC = 1536, kDwconvTaps = 49;
inline bool dwconv7_supported(int C) { return C >= kDwconvMinC && C <= kDwconvMaxC && C % 32 == 0; }

// torch's depthwise weight [C][1][7][7] -> [49][C] of T (tap-major, channel-contiguous): a lane's weights of one
// tap for its 16-byte channel chunk are one vector load.
template <typename T>
void dwconv7_pack_into(T* dst, const float* w, int C) {
  for (int tap = 0; tap < kDwconvTaps; ++tap)
    for (int c = 0; c < C; ++c) dst[(size_t)tap * C + c] = static_cast<T>(w[(size_t)c * kDwconvTaps + tap]);
}

// The bank rule of the depthwise kernels' halo reads (dwconv_ln.hip states it; mbconv.hip holds its own strides
// against it): lanes chunk-fastest, lane l reading chunk l % nch of the run l / nch, runs `run` pixels of `stride`
// 16-byte chunks apart -- the 16 lanes one LDS pass serves must touch 16 distinct 16-byte bank groups.
constexpr bool dw_reads_disjoint(int nch, int stride, int run) {
  bool seen[16] = {};
  for (int l = 0; l < 16; ++l) {
    const int slot = ((l / nch) * run * stride + l % nch) % 16;
    if (seen[slot]) return false;
    seen[slot] = true;
  }
  return true;
}

// A 2x2 / stride 2 conv weight [N][C][2][2] -> the dense [N][4 C] matrix over ln_space_to_depth's rows:
// column (kh * 2 + kw) * C + c, so the C channels of each of the four source pixels lie contiguous.
inline void s2d_permute_weight(const float* w, int N, int C, float* dst) {
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int q = 0; q < 4; ++q) dst[((size_t)n * 4 + q) * C + c] = w[((size_t)n * C + c) * 4 + q];
}

}  // namespace spi
