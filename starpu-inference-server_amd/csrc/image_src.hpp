// What an image task's input buffer holds and the limits of the classification outputs: plain data,
// no HIP, shared by the kernels' host entry points (spi_kernels.hpp) and the replica's host-only I/O
// contract (model_plan.hpp).
#pragma once

namespace spi {

// What an image task's input buffer holds (ResNet / ViT).  The kernels that read it -- the fused
// stem, ingest_nchw, patchify -- take the kind and, for 8-bit pixels, the per-channel input
// transform: pixel p of channel c enters the network as fl(fl((float)p * scale[c]) + shift[c]),
// one fp32 multiply and one fp32 add, each rounded to nearest and never contracted into an FMA.
// The transform travels as a kernel argument; an fp32 image ignores it.
enum SrcKind : int { kSrcF32Nchw = 0, kSrcU8Nchw = 1, kSrcU8Nhwc = 2 };
struct InputXf {
  float scale[3] = {1.f, 1.f, 1.f};
  float shift[3] = {0.f, 0.f, 0.f};
};

// What input 0 of an image task holds: its kind and, for an 8-bit task of a replica with the input
// resize on (H > 0), the source size the prologue resamples to the replica's image first.
struct ImageSrc {
  int kind = kSrcF32Nchw;
  int H = 0, W = 0;
};

// softmax_topk (classify.hip): 1 <= N <= kSoftmaxTopkMaxN, 1 <= k <= min(N, kSoftmaxTopkMaxK)
constexpr int kSoftmaxTopkMaxN = 16384, kSoftmaxTopkMaxK = 64;

}  // namespace spi
