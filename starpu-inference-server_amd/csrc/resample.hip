// Resize + centre crop of 8-bit image tasks on the device: bytes [B][3][H][W] or [B][H][W][3] ->
// the normalised fp32 NCHW image [B][3][S][S] that the fp32-source prologue kernels then read.
// The arithmetic is resample.hpp's, shared with the host reference.
//
// A workgroup of 256 threads owns one image's tile of kTY output rows x kTX output columns for all
// three channels and walks the band of source rows the tile's rows need, kRows rows per step:
//   horizontal: thread (ty, ox) resamples source rows ty and ty + kTY of the step at output column
//               ox for the three channels into LDS -- its column's taps, their fp32 sum, are fixed
//               for the whole walk; kTapsInFlight taps of both rows are loaded before any is used
//               (one tap per load round trip left the launch waiting on memory latency; a tap past
//               the column's last one is a clamped address with weight 0, which adds nothing);
//   vertical:   thread (oy, ox) adds the step's rows that lie inside its own row's taps, in
//               ascending order, from LDS.
// Up to kWCap taps per output index (a downscale of up to 8) the workgroup first computes its columns'
// and rows' normalised weights once into LDS; above that every thread computes the weights it uses.
// The tap loops are runtime loops: LDS (9 KiB) and registers do not depend on the source size or
// the ratio, nothing is precomputed on the host, no atomics.  Source bytes come as aligned dwords
// (a byte load costs the texture path what a dword load costs): an NHWC pixel's three bytes from
// the one or two dwords that hold them, one pass over the row for the three channels; an NCHW
// pixel from one dword per plane.  Every dword loaded holds a byte of the image, so it lies in a
// page of the image whatever the buffer's base address.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "resample.hpp"
#include "spi_kernels.hpp"

namespace spi {
namespace {

constexpr int kTX = 32, kTY = 8;    // the tile; kTX * kTY threads
constexpr int kRowsPerThread = 2;   // source rows a thread resamples per step
constexpr int kRows = kTY * kRowsPerThread;
constexpr int kTapsInFlight = 4;
constexpr int kWCap = 16;  // taps per output index up to which a workgroup keeps its weights in LDS

// no output index of an axis has more taps than this: hi - lo <= ceil(2 m / n_out) (resample.hpp)
int axis_max_taps(int n_in, int n_out) { return (2 * std::max(n_in, n_out) + n_out - 1) / n_out; }

struct ResampleArgs {
  const unsigned char* x;
  float* y;
  int H, W, S;
  ResizeGeom g;
  InputXf xf;
};

// (stepping back from p keeps it a pointer into global memory; an address rebuilt from an integer
// becomes a flat load)
__device__ __forceinline__ unsigned aligned_dword(const unsigned char* p) {
  return *reinterpret_cast<const unsigned*>(p - (reinterpret_cast<uintptr_t>(p) & 3));
}

// The three channels of pixel j of a row: the dwords (load), then the values (unpack).
template <bool NHWC>
struct Pixel {
  unsigned d[NHWC ? 2 : 3], sh[NHWC ? 1 : 3];
  __device__ __forceinline__ void load(const unsigned char* row, size_t plane, int j) {
    if constexpr (NHWC) {
      // bytes p[0..2] lie in the aligned dword of p and, past its end, in the one of p + 2 (which is the
      // same dword again when the pixel starts in its first two bytes)
      const unsigned char* p = row + 3 * (size_t)j;
      d[0] = aligned_dword(p);
      d[1] = aligned_dword(p + 2);
      sh[0] = 8u * (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    } else {
      for (int c = 0; c < 3; ++c) {
        const unsigned char* p = row + c * plane + j;
        d[c] = aligned_dword(p);
        sh[c] = 8u * (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
      }
    }
  }
  __device__ __forceinline__ void unpack(float v[3]) const {
    if constexpr (NHWC) {
      const unsigned px = (unsigned)((((unsigned long long)d[1] << 32) | d[0]) >> sh[0]);
      v[0] = static_cast<float>(px & 0xffu);
      v[1] = static_cast<float>((px >> 8) & 0xffu);
      v[2] = static_cast<float>((px >> 16) & 0xffu);
    } else {
      for (int c = 0; c < 3; ++c) v[c] = static_cast<float>((d[c] >> sh[c]) & 0xffu);
    }
  }
};

// CACHED (no output index of the launch has more than kWCap taps on either axis; resize_crop_u8 decides):
// the workgroup computes the normalised weights of its kTX columns and kTY rows once, into LDS, instead of
// every thread recomputing its column's for each of its rows and its row's for each of its columns --
// two IEEE divides a weight, which is what the launch spent its time on.  Same functions, same bits.
template <bool NHWC, bool CACHED>
__global__ __launch_bounds__(kTX * kTY) void resize_crop_u8_kernel(const ResampleArgs a) {
  __shared__ float hbuf[kRows][3][kTX];
  __shared__ float wx[CACHED ? kWCap : 1][kTX], wy[CACHED ? kWCap : 1][kTY];  // [tap][column / row]
  __shared__ float tot[CACHED ? kTX + kTY : 1];
  const int tx = threadIdx.x % kTX, ty = threadIdx.x / kTX;
  const int H = a.H, W = a.W, S = a.S;
  const int ox0 = blockIdx.x * kTX, oy0 = blockIdx.y * kTY;
  const int ox = min(ox0 + tx, S - 1), oy = min(oy0 + ty, S - 1);  // clamped: computed, not stored
  // this thread's column taps (horizontal phase) and row taps (vertical phase)
  const AxisTaps cx = axis_taps(a.g.left + ox, W, a.g.RW);
  const AxisTaps cy = axis_taps(a.g.top + oy, H, a.g.RH);
  float totx = 0.0f, toty = 0.0f;
  if constexpr (CACHED) {
    // the weight sums of the tile's columns and rows (one thread each), then their weights
    const int t = threadIdx.x;
    if (t < kTX + kTY) {
      const AxisTaps c = t < kTX ? axis_taps(a.g.left + min(ox0 + t, S - 1), W, a.g.RW)
                                 : axis_taps(a.g.top + min(oy0 + t - kTX, S - 1), H, a.g.RH);
      tot[t] = tap_total(c);
    }
    __syncthreads();
    for (int e = t; e < kWCap * (kTX + kTY); e += kTX * kTY) {
      const bool col = e < kWCap * kTX;
      const int u = col ? e / kTX : (e - kWCap * kTX) / kTY, i = col ? e % kTX : (e - kWCap * kTX) % kTY;
      const AxisTaps c = col ? axis_taps(a.g.left + min(ox0 + i, S - 1), W, a.g.RW)
                             : axis_taps(a.g.top + min(oy0 + i, S - 1), H, a.g.RH);
      const float w = c.lo + u < c.hi ? tap_norm(tap_weight(c, c.lo + u), tot[col ? i : kTX + i]) : 0.0f;
      if (col)
        wx[u][i] = w;
      else
        wy[u][i] = w;
    }
    __syncthreads();
  } else {
    totx = tap_total(cx);
    toty = tap_total(cy);
  }
  // the tile's band of source rows: the same in every thread
  const int band0 = axis_taps(a.g.top + oy0, H, a.g.RH).lo;
  const int band1 = axis_taps(a.g.top + min(oy0 + kTY, S) - 1, H, a.g.RH).hi;
  const size_t plane = (size_t)H * W;
  const size_t pitch = NHWC ? (size_t)W * 3 : (size_t)W;
  const unsigned char* img = a.x + (size_t)blockIdx.z * plane * 3;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int r0 = band0; r0 < band1; r0 += kRows) {
    float h[kRowsPerThread][3] = {};
    const unsigned char* row[kRowsPerThread];
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q)  // a row past the band: the band's last row again, not stored
      row[q] = img + (size_t)min(r0 + ty + q * kTY, band1 - 1) * pitch;
    for (int j0 = cx.lo; j0 < cx.hi; j0 += kTapsInFlight) {
      Pixel<NHWC> px[kRowsPerThread][kTapsInFlight];
#pragma unroll
      for (int u = 0; u < kTapsInFlight; ++u) {
        const int j = min(j0 + u, cx.hi - 1);
#pragma unroll
        for (int q = 0; q < kRowsPerThread; ++q) px[q][u].load(row[q], plane, j);
      }
#pragma unroll
      for (int u = 0; u < kTapsInFlight; ++u) {
        float w = 0.0f;
        if (j0 + u < cx.hi) {
          if constexpr (CACHED)
            w = wx[j0 + u - cx.lo][tx];
          else
            w = tap_norm(tap_weight(cx, j0 + u), totx);
        }
#pragma unroll
        for (int q = 0; q < kRowsPerThread; ++q) {
          float v[3];
          px[q][u].unpack(v);
#pragma unroll
          for (int c = 0; c < 3; ++c) h[q][c] = tap_acc(w, v[c], h[q][c]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q)
      if (r0 + ty + q * kTY < band1)
#pragma unroll
        for (int c = 0; c < 3; ++c) hbuf[ty + q * kTY][c][tx] = h[q][c];
    __syncthreads();
    const int rend = min(r0 + kRows, band1);
    for (int rr = max(r0, cy.lo); rr < min(rend, cy.hi); ++rr) {
      float w;
      if constexpr (CACHED)
        w = wy[rr - cy.lo][ty];
      else
        w = tap_norm(tap_weight(cy, rr), toty);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = tap_acc(w, hbuf[rr - r0][c][tx], acc[c]);
    }
    __syncthreads();
  }
  if (ox0 + tx < S && oy0 + ty < S) {
    float* y = a.y + ((size_t)blockIdx.z * 3 * S + oy) * S + ox;
    const size_t cs = (size_t)S * S;
    y[0] = resample_xf(acc[0], a.xf.scale[0], a.xf.shift[0]);
    y[cs] = resample_xf(acc[1], a.xf.scale[1], a.xf.shift[1]);
    y[2 * cs] = resample_xf(acc[2], a.xf.scale[2], a.xf.shift[2]);
  }
}

}  // namespace

void resize_crop_u8(const void* x, bool nhwc, int B, int H, int W, int resize_short, int crop, const InputXf& xf,
                    float* y, hipStream_t s) {
  if (!x || !y || B < 1 || B > 65535 || H < 1 || W < 1 || H > kResizeMax || W > kResizeMax || crop < 1 ||
      resize_short < crop || resize_short > kResizeMax)
    throw std::invalid_argument("resize_crop_u8: 1 <= H, W <= 8192, 1 <= crop <= resize_short <= 8192, 1 <= B <= 65535");
  ResampleArgs a;
  a.x = static_cast<const unsigned char*>(x);
  a.y = y;
  a.H = H, a.W = W, a.S = crop;
  a.g = resize_geom(H, W, resize_short, crop);
  if (a.g.RH > kResizeMax || a.g.RW > kResizeMax)
    throw std::invalid_argument("resize_crop_u8: the resized long side " + std::to_string(std::max(a.g.RH, a.g.RW)) +
                                " exceeds 8192");
  a.xf = xf;
  const dim3 grid((crop + kTX - 1) / kTX, (crop + kTY - 1) / kTY, B);
  const bool cached = axis_max_taps(W, a.g.RW) <= kWCap && axis_max_taps(H, a.g.RH) <= kWCap;
  if (nhwc && cached)
    SPI_LAUNCH((resize_crop_u8_kernel<true, true>), grid, dim3(kTX * kTY), 0, s, a);
  else if (nhwc)
    SPI_LAUNCH((resize_crop_u8_kernel<true, false>), grid, dim3(kTX * kTY), 0, s, a);
  else if (cached)
    SPI_LAUNCH((resize_crop_u8_kernel<false, true>), grid, dim3(kTX * kTY), 0, s, a);
  else
    SPI_LAUNCH((resize_crop_u8_kernel<false, false>), grid, dim3(kTX * kTY), 0, s, a);
}

}  // namespace spi
