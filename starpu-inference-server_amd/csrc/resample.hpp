// Resize + centre crop of 8-bit image tasks (spi_model_set_input_resize): the geometry and the tap
// arithmetic of the antialiased bilinear resample, stated in integers where that makes it exact.
// Plain C++17, no HIP header: the kernel (resample.hip) and the host reference
// (spi_op_resize_crop_u8_host, ops.cpp) run the same functions -- the idiom of gemm_args.hpp.
//
// The value of output pixel (oy, ox), channel c, of an H x W source under (resize_short R, crop S):
//   1. resized size (torchvision Resize(int)): the short side becomes R, the long side
//      floor(R long / short) -> RH x RW;
//   2. crop offset (torchvision CenterCrop): top = round_half_even((RH - S) / 2), left alike;
//   3. per axis, output index i of n_out from n_in source pixels (ATen _upsample_bilinear2d_aa,
//      align_corners = false): m = max(n_in, n_out), c2 = n_in (2 i + 1), taps j in [lo, hi),
//        lo = max(0, floor((c2 - 2 m + n_out) / (2 n_out))), hi = min(n_in, floor((c2 + 2 m + n_out) / (2 n_out))),
//        w_j = max(0, 1 - |n_out (2 j + 1) - c2| / (2 m)), normalised by their fp32 sum (ascending j);
//      the rows' horizontal samples first, then the vertical pass over them, each an ascending-j
//      chain of fused multiply-adds from 0 (one rounding per tap); fp32 throughout, never rounded
//      back to 8 bits;
//   4. the input transform of 8-bit tasks, fl(fl(v scale[c]) + shift[c]).
// Every size is at most kResizeMax, so the integer products stay below 2^28.
#pragma once
#include <cmath>

#ifndef SPI_HD
#ifdef __HIP__
#define SPI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SPI_HD inline
#endif
#endif

namespace spi {

constexpr int kResizeMax = 8192;  // largest source side, resize_short and resized long side

struct ResizeGeom {
  int RH, RW;     // the resized image
  int top, left;  // the crop's first row / column in it
};

// round_half_even(d / 2) for d >= 0: d = 0 .. 5 -> 0, 0, 1, 2, 2, 2
SPI_HD int crop_offset(int d) {
  const int k = d >> 1;
  return (d & 1) == 0 || (k & 1) == 0 ? k : k + 1;
}

// R >= S >= 1; the long side may exceed kResizeMax: the caller refuses such a task
SPI_HD ResizeGeom resize_geom(int H, int W, int R, int S) {
  ResizeGeom g;
  if (H <= W) {
    g.RH = R;
    g.RW = (int)((long long)R * W / H);
  } else {
    g.RW = R;
    g.RH = (int)((long long)R * H / W);
  }
  g.top = crop_offset(g.RH - S);
  g.left = crop_offset(g.RW - S);
  return g;
}

// The taps of output index i on one axis.
struct AxisTaps {
  int lo, hi;  // source indices [lo, hi)
  int c2;      // n_in (2 i + 1): twice the centre, in units of 1 / n_out source pixels
  int n_out;
  int m2;      // 2 max(n_in, n_out)
};

SPI_HD AxisTaps axis_taps(int i, int n_in, int n_out) {
  AxisTaps t;
  t.n_out = n_out;
  t.m2 = 2 * (n_in > n_out ? n_in : n_out);
  t.c2 = n_in * (2 * i + 1);
  const int a = t.c2 - t.m2 + n_out, b = t.c2 + t.m2 + n_out;
  t.lo = a < 0 ? 0 : a / (2 * n_out);
  t.hi = b / (2 * n_out);
  if (t.hi > n_in) t.hi = n_in;
  return t;
}

// w_j before normalisation: the integer numerator converts to fp32 exactly (it is below 2^24 wherever
// the weight is not clamped to 0 anyway), then one divide and one subtract, never contracted.
SPI_HD float tap_weight(const AxisTaps& t, int j) {
#pragma clang fp contract(off)
  int num = t.n_out * (2 * j + 1) - t.c2;
  if (num < 0) num = -num;
  const float w = 1.0f - static_cast<float>(num) / static_cast<float>(t.m2);
  return w > 0.0f ? w : 0.0f;
}

// the fp32 sum of an output index's weights, ascending j
SPI_HD float tap_total(const AxisTaps& t) {
#pragma clang fp contract(off)
  float s = 0.0f;
  for (int j = t.lo; j < t.hi; ++j) s = s + tap_weight(t, j);
  return s;
}

// the normalised weight (ATen leaves the weights alone when they sum to 0)
SPI_HD float tap_norm(float w, float total) { return total != 0.0f ? w / total : w; }

// one tap of a dot product: a single rounding
SPI_HD float tap_acc(float w, float v, float acc) { return fmaf(w, v, acc); }

// the input transform on a resampled value: two roundings, never an FMA (as input_xf_apply)
SPI_HD float resample_xf(float v, float sc, float sh) {
#pragma clang fp contract(off)
  const float m = v * sc;
  return m + sh;
}

}  // namespace spi
