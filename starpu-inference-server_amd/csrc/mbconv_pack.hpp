// Host-side layouts of the MBConv kernels (mbconv.hip): the supported sets, the output and pixel-tile
// geometry of dwconv_act (the rows of its pool sums), and the depthwise k x k weight repack.
// Plain C++, shared by the packer (model_pack.cpp), the plans (model_plan.cpp) and the op entry points (ops.cpp).
#pragma once
#include <cstddef>

namespace spi {

// C a multiple of 8 from 8 to 4608 (efficientnet_b7's widest expanded map has 3840 channels), k 3 or 5,
// stride 1 or 2, pad (k - 1) / 2 on all four sides (torchvision's Conv2dNormActivation).
constexpr int kMbMinC = 8, kMbMaxC = 4608, kSeMaxSq = 256;
inline bool mbconv_channels_ok(int C) { return C >= kMbMinC && C <= kMbMaxC && C % 8 == 0; }
inline bool dwconv_supported(int C, int k, int stride) {
  return mbconv_channels_ok(C) && (k == 3 || k == 5) && (stride == 1 || stride == 2);
}
inline bool se_supported(int C, int sq) { return mbconv_channels_ok(C) && sq >= 1 && sq <= kSeMaxSq; }
inline int dwconv_out(int H, int k, int stride) { return (H + 2 * (k / 2) - k) / stride + 1; }

// The output pixel tile of one workgroup: 16 x 8 at stride 1 (lanes take runs of 4 pixels along W), 8 x 8 at
// stride 2 (runs of 2): 32 runs either way, each spanning 4 input columns.
inline int dwconv_tile_h(int stride) { return stride == 1 ? 16 : 8; }
constexpr int kDwTileW = 8;
// Pixel tiles per image = rows per image of the pool sums part[B][tiles][C].
inline int dwconv_tiles(int H, int W, int k, int stride) {
  const int OH = dwconv_out(H, k, stride), OW = dwconv_out(W, k, stride), th = dwconv_tile_h(stride);
  return ((OH + th - 1) / th) * ((OW + kDwTileW - 1) / kDwTileW);
}

// torch's depthwise weight [C][1][k][k] (BatchNorm already folded in, fp32) -> [k k][C] of T, tap-major and
// channel-contiguous: a lane's weights of one tap for its 16-byte channel chunk are one vector load.
template <typename T>
void dwconv_pack_into(T* dst, const float* w, int C, int k) {
  for (int tap = 0; tap < k * k; ++tap)
    for (int c = 0; c < C; ++c) dst[(size_t)tap * C + c] = static_cast<T>(w[(size_t)c * k * k + tap]);
}

}  // namespace spi
