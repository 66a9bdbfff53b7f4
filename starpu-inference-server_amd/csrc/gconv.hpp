// Grouped 3x3 conv (conv_group.hip; a ResNeXt bottleneck's conv2): the supported set, the k order of
// its MFMA steps, the packed-weight layout and the grid decode.  Plain data, no HIP types: the
// packer (model_pack.cpp), the op-level API (ops.cpp) and the kernel share it.
//
// The conv: NHWC fp16, Cin == Cout == C in `groups` groups of cpg = C / groups channels, 3x3, pad 1,
// stride 1 or 2.  Group g reads input channels [g cpg, (g + 1) cpg) and writes the same output channels.
//
// One wave owns a tile of 16 output channels [n0, n0 + 16) and contracts it with
// mfma_f32_16x16x32_f16, weights as the A operand (rows = channels) and pixels as B (columns), so lane
// l = 16 q + r supplies 8 consecutive k of row / column r: k = 8 q + j.  A step's 32 k are
//   cpg <= 16: two taps x the 16 input channels n0 .. n0 + 15 (the tile's own groups; a weight whose
//              input channel lies in another group than its row is packed as zero): tap 2 s + (q >> 1),
//              channel n0 + 8 (q & 1) + j; 5 steps, the last one's second tap (9) all zero;
//   cpg == 32: one tap x the tile's group: tap s, channel 32 (n0 / 32) + 8 q + j; 9 steps;
//   cpg == 64: half a group per step: tap s >> 1, channel 64 (n0 / 64) + 32 (s & 1) + 8 q + j; 18 steps.
//
// Packed weights: fp16 [C / 16 tiles][steps][64 lanes][8], lane l's A fragment of a step as one
// 16-byte chunk, so a wave reads a step as one contiguous KiB and keeps all of them in registers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace spi {

constexpr int kGconvTileN = 16;  // output channels per wave
constexpr int kGconvWaves = 4;   // waves (channel tiles) per workgroup
constexpr int kGconvTileM = 16;  // pixels per accumulator

constexpr bool gconv_supported(int C, int groups) {
  if (C <= 0 || groups < 2 || C % 128 != 0 || C % groups != 0) return false;
  const int cpg = C / groups;
  return cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32 || cpg == 64;
}

constexpr int gconv_steps(int cpg) { return cpg <= 16 ? 5 : cpg == 32 ? 9 : 18; }

// Filter tap (kh 3 + kw; 9: none, zero weights) and first input channel of lane group q in step s.
constexpr int gconv_tap(int cpg, int s, int q) { return cpg <= 16 ? 2 * s + (q >> 1) : cpg == 32 ? s : s >> 1; }
constexpr int gconv_channel(int cpg, int n0, int s, int q) {
  return cpg <= 16 ? n0 + 8 * (q & 1) : cpg == 32 ? n0 / 32 * 32 + 8 * q : n0 / 64 * 64 + 32 * (s & 1) + 8 * q;
}

constexpr size_t gconv_packed_bytes(int C, int groups) {
  return (size_t)(C / kGconvTileN) * gconv_steps(C / groups) * 64 * 8 * sizeof(_Float16);
}

// at(n, c, tap): the folded weight of output channel n, input channel c of n's group (c < cpg), tap.
template <typename F>
void gconv_pack_into(_Float16* dst, int C, int groups, F at) {
  const int cpg = C / groups, steps = gconv_steps(cpg);
  for (int tile = 0; tile < C / kGconvTileN; ++tile)
    for (int s = 0; s < steps; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int q = lane >> 4, n = tile * kGconvTileN + (lane & 15);
        const int tap = gconv_tap(cpg, s, q), c0 = gconv_channel(cpg, tile * kGconvTileN, s, q);
        for (int j = 0; j < 8; ++j) {
          const int ci = c0 + j;
          const bool own = tap < 9 && ci / cpg == n / cpg;
          *dst++ = own ? static_cast<_Float16>(at(n, ci % cpg, tap)) : static_cast<_Float16>(0.f);
        }
      }
}

// Launch grid: x = blocks of nsub 16-pixel tiles, y = blocks of 64 channels.  nsub (the pixel tiles a
// wave walks with its weights in registers) is the largest of 4, 2, 1 that leaves two workgroups per
// compute unit (512), else 1.
struct GconvGrid {
  unsigned gx = 0, gy = 0;
  int nsub = 1;
};
inline GconvGrid gconv_grid(int M, int C) {
  GconvGrid g;
  g.gy = (unsigned)(C / (kGconvTileN * kGconvWaves));
  const long tiles = ((long)M + kGconvTileM - 1) / kGconvTileM;
  for (int nsub : {4, 2, 1}) {
    g.nsub = nsub;
    g.gx = (unsigned)((tiles + nsub - 1) / nsub);
    if ((long)g.gx * g.gy >= 512) break;
  }
  return g;
}

}  // namespace spi
