// Grouped 3x3 conv, fp16 NHWC, Cin == Cout == C (a ResNeXt bottleneck's conv2): gconv.hpp has the
// supported set, the k order of the MFMA steps and the packed-weight layout.
//
// A workgroup is four waves = four tiles of 16 output channels over the same pixels.  A wave loads
// its tile's weight fragments once (gconv_steps(cpg) x 16 bytes per lane, <= 72 VGPRs) and walks
// nsub tiles of 16 pixels: per pixel tile and step it reads the 16-byte channel chunk of its lane's
// pixel at the step's tap straight from global (a padding tap, the zero tap 9 and a pixel past M read
// nothing and contribute zeros), runs the MFMAs (weights = A, pixels = B, so the accumulator holds four
// consecutive channels of one pixel per lane) and stores bias + ReLU as one 8-byte fp16 vector.
// Neighbouring waves read the neighbouring 32 / 64 / 128 bytes of the same pixels, and a pixel's nine
// re-reads come from L1 / L2: the conv has no LDS stage and no barrier.
#include <climits>
#include <stdexcept>

#include "gconv.hpp"
#include "lds_dma.hpp"
#include "spi_kernels.hpp"

namespace spi {
namespace {

constexpr int kThreads = 64 * kGconvWaves;

template <int CPG, bool RELU>
__global__ __launch_bounds__(kThreads) void gconv3x3_kernel(const _Float16* __restrict__ x,
                                                            const half8* __restrict__ wp,
                                                            const float* __restrict__ bias, _Float16* __restrict__ y,
                                                            int H, int W, int C, int OH, int OW, int M, int stride,
                                                            int nsub) {
  constexpr int STEPS = gconv_steps(CPG);
  const int lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int tile = blockIdx.y * kGconvWaves + (threadIdx.x >> 6);
  const int n0 = tile * kGconvTileN;

  half8 wf[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) wf[s] = wp[((size_t)tile * STEPS + s) * 64 + lane];
  floatx4 bv = {0.f, 0.f, 0.f, 0.f};
  if (bias) bv = *reinterpret_cast<const floatx4*>(bias + n0 + 4 * q);

  for (int sub = 0; sub < nsub; ++sub) {
    const int m0 = (blockIdx.x * nsub + sub) * kGconvTileM;
    if (m0 >= M) break;  // the same for every lane of the workgroup
    const int m = m0 + r;
    const bool live = m < M;
    const int mm = live ? m : M - 1;
    const int ow = mm % OW, t = mm / OW, oh = t % OH, img = t / OH;
    const int ih0 = oh * stride - 1, iw0 = ow * stride - 1;
    const _Float16* xi = x + (size_t)img * H * W * C;

    half8 xf[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int tap = gconv_tap(CPG, s, q);
      const int kh = tap / 3, kw = tap - 3 * kh;
      const int ih = ih0 + kh, iw = iw0 + kw;
      const bool in = live && tap < 9 && ih >= 0 && ih < H && iw >= 0 && iw < W;
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (in) v = *reinterpret_cast<const half8*>(xi + ((size_t)ih * W + iw) * C + gconv_channel(CPG, n0, s, q));
      xf[s] = v;
    }
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[s], xf[s], acc, 0, 0, 0);

    if (live) {  // channels n0 + 4 q .. + 3 of pixel m
      half4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[e] + bv[e];
        if (RELU) v = v > 0.f ? v : 0.f;
        o[e] = static_cast<_Float16>(v);
      }
      *reinterpret_cast<half4*>(y + (size_t)m * C + n0 + 4 * q) = o;
    }
  }
}

template <int CPG>
void launch(const _Float16* x, const half8* w, const float* bias, _Float16* y, int H, int W, int C, int OH, int OW,
            int M, int stride, bool relu, hipStream_t s) {
  const GconvGrid g = gconv_grid(M, C);
  const dim3 grid(g.gx, g.gy);
  if (relu)
    SPI_LAUNCH((gconv3x3_kernel<CPG, true>), grid, dim3(kThreads), 0, s, x, w, bias, y, H, W, C, OH, OW, M, stride, g.nsub);
  else
    SPI_LAUNCH((gconv3x3_kernel<CPG, false>), grid, dim3(kThreads), 0, s, x, w, bias, y, H, W, C, OH, OW, M, stride, g.nsub);
}

}  // namespace

void conv_group(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int groups,
                int stride, bool relu, hipStream_t s) {
  if (!gconv_supported(C, groups)) throw std::invalid_argument("conv_group: unsupported channels / groups");
  if (B <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2))
    throw std::invalid_argument("conv_group: B, H, W >= 1 and stride 1 or 2");
  if ((int64_t)B * H * W > INT_MAX) throw std::invalid_argument("conv_group: more than 2^31 - 1 input pixels");
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;  // 3x3, pad 1
  const int M = B * OH * OW;
  const auto* xp = static_cast<const _Float16*>(x);
  const auto* wq = static_cast<const half8*>(w);
  auto* yp = static_cast<_Float16*>(y);
  // cpg 4, 8 and 16 differ only in which packed weights are zero: one instance
  const int cpg = C / groups;
  if (cpg <= 16) return launch<16>(xp, wq, bias, yp, H, W, C, OH, OW, M, stride, relu, s);
  if (cpg == 32) return launch<32>(xp, wq, bias, yp, H, W, C, OH, OW, M, stride, relu, s);
  return launch<64>(xp, wq, bias, yp, H, W, C, OH, OW, M, stride, relu, s);
}

}  // namespace spi
