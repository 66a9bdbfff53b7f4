// The GEMM / conv-as-implicit-GEMM problem descriptor, its one conv and one dense builder, and the
// pointers of a launch: plain data, no HIP types, so the host-only planner (gemm_plan.hpp), the
// host-only argument builder (gemm_args.hpp) and the kernels (spi_kernels.hpp) share them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace spi {

enum class Act : int { None = 0, Relu = 1, Gelu = 2 };

// Contraction precision.  F16X3 = split fp16 (fp32 activations, hi/lo fp16
// operands, three MFMAs per fragment): fp32-grade results at the fp16 rate.
enum class Prec : int { F32 = 0, F16 = 1, F16X3 = 2 };

// C[M,N] = act(A[M,K] . W[N,K]^T + bias[N] + residual[M,N])
//
// A is either a dense row-major activation (lda) or, for conv-as-implicit-GEMM,
// an NHWC image gathered on the fly: row m = (img, oh, ow), column
// k = (kh*KW + kw)*Cin + c.  W is pre-packed [Npad][Kpad] (K contiguous,
// zero padded), so both MFMA operands are K-contiguous 16-byte chunks.  For
// Prec::F16X3 each W row is Kpad/32 blocks of [32 hi fp16 | 32 lo fp16].
struct GemmDesc {
  int M = 0, N = 0, K = 0;  // logical sizes
  int Kpad = 0;             // W row stride (multiple of 64)
  size_t wplane = 0;        // elements between the hi and lo weight planes (F16X3)
  int lda = 0;              // dense A row stride (elements)
  int ldc = 0;              // C row stride (elements)
  int ldr = 0;              // residual row stride (elements)
  // conv geometry (conv == true)
  bool conv = false;
  int H = 0, W = 0, Cin = 0, OH = 0, OW = 0, KH = 1, KW = 1, stride = 1, pad = 0;
  Act act = Act::None;
  bool out_f32 = false;  // C is float (else the compute type)
  bool out_f16 = false;  // C is fp16 although the mode's output type is fp32 (F16X3, plain stores)
  bool res_f32 = false;  // residual is float (else the compute type)
  // F16X3 activation split layout: per row, blocks of 32 elements stored as
  // [32 hi fp16 | 32 lo fp16] (128 bytes, the size of 32 fp32), hi = fp16(x),
  // lo = fp16(x - hi).  a_split: A and the residual are split (conv Cin >= 32);
  // out_split: C is written split.
  bool a_split = false;
  bool out_split = false;
  // Fused global average pool + linear layer (ResNet avgpool + fc): A holds
  // pool_rows consecutive rows (pixels) per image; output row b of C is
  // act(mean over image b's rows of A . W^T + bias).  Linearity lets the GEMM
  // run over every pixel and average its own C tile (64 x 64 tiles, one image
  // per tile row, pool_rows <= 64).  M = images x pool_rows.
  int pool_rows = 0;
  // krep = 2 (F16, dense or one-tap-per-step conv A): the packed W holds two k-steps per A
  // k-step -- fp16(w) then fp16(w - fp16(w)) for the same 64 k-values -- and each A k-step is
  // staged twice, so one launch accumulates x.w_hi + x.w_lo (~22-bit weights on fp16 MFMAs).
  // Kpad is the packed (W) row length; K stays the logical A length.
  int krep = 1;
  // W came from pack_matrix_into of an fp16 64 x 576 matrix, whose padding rows 64..127
  // hold the weight-resident conv's LDS image (pack.hpp); conv_wres requires it.
  bool w_image = false;
  // LayerNorm folded across GEMMs (transformer fp16 path; dense F16 A, the
  // vector epilogue only).  Row statistics travel as per-64-column-chunk partials
  // (mean, M2) -- [rows][chunks][2] fp32 -- combined by Chan's formula where they are used.
  //  ln_in_chunks > 0: A holds the rows x BEFORE a LayerNorm (an fp16 copy), W was packed
  //    with the gain folded in (W' = W diag(gamma)), and the epilogue applies
  //    y = rstd[m] * (acc - mean[m] * c1[n]) + bias[n] (bias = b + W beta, c1 = W' 1).
  //  res_ln_chunks > 0: the residual is LN(R) computed on the fly from the fp32 rows R and
  //    their statistics: (R - mean) * rstd * g + b (a post-LN block's input).
  //  ln_out: write the output rows' chunk statistics (N / 64 chunks) and an fp16 copy of
  //    the output (C16, row stride ld16) for the next, folding GEMM.
  int ln_in_chunks = 0;
  float ln_in_eps = 0.f;
  int res_ln_chunks = 0;
  float res_ln_eps = 0.f;
  bool ln_out = false;
  int ld16 = 0;
  // Two-plane fp16 residual stream (round 6, the transformer fold path): a row-major [rows][ld]
  // tensor x kept as hi = fp16(x) at the pointer and lo = fp16(x - hi) `plane` elements further on
  // -- ~22-bit values in the bytes of fp32, and the hi plane is already the fp16 operand the next
  // folding GEMM reads, so a producer writes no separate fp16 copy (LnPtrs::c16 may be null).
  // res_planes: the residual is such a pair; out_planes: C is written as one, and then the
  // residual, if any, is either fp32 (res_f32) or such a pair -- never a plain fp16 tensor.
  bool res_planes = false;
  bool out_planes = false;
  size_t plane = 0;
};


// The desc of a conv over B NHWC images of H x W x Cin (Cin as packed: the padded channel count)
// and of a dense [M, K] x [N, K]^T problem.  They compute the output size, M, K, the packed W row
// length (krep = 2: hi + lo weights, twice as long) and the output strides; the caller sets what is
// its own: activation, operand formats, w_image, the fold fields.
inline GemmDesc conv_desc(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int krep) {
  GemmDesc d;
  d.conv = true;
  d.H = H, d.W = W, d.Cin = Cin;
  d.KH = KH, d.KW = KW;
  d.stride = stride;
  d.pad = pad;
  d.OH = (H + 2 * pad - KH) / stride + 1;
  d.OW = (W + 2 * pad - KW) / stride + 1;
  d.M = B * d.OH * d.OW;
  d.N = Cout;
  d.K = KH * KW * Cin;
  d.krep = krep;
  d.Kpad = (d.K + 63) / 64 * 64 * krep;
  d.ldc = d.ldr = Cout;
  return d;
}
inline GemmDesc dense_desc(int M, int N, int K, int lda, int ldc, int ldr, int krep) {
  GemmDesc d;
  d.M = M;
  d.N = N;
  d.K = K;
  d.krep = krep;
  d.Kpad = (K + 63) / 64 * 64 * krep;
  d.lda = lda;
  d.ldc = ldc;
  d.ldr = ldr;
  return d;
}

// Pointers of the LayerNorm fold (GemmDesc::ln_in_chunks / res_ln_chunks / ln_out).
struct LnPtrs {
  const float* in_stats = nullptr;   // A rows' chunk statistics
  const float* c1 = nullptr;         // [N] per-column sum of the folded weights
  const float* res_stats = nullptr;  // residual rows' chunk statistics
  const float* res_g = nullptr;      // residual LayerNorm gain / bias
  const float* res_b = nullptr;
  float* out_stats = nullptr;        // output rows' chunk statistics
  _Float16* c16 = nullptr;           // fp16 copy of the output (none with GemmDesc::out_planes)
};

struct GemmPtrs {
  const void* A = nullptr;
  const void* W = nullptr;
  const float* bias = nullptr;
  const void* res = nullptr;
  void* C = nullptr;
  float* partial = nullptr;  // split-K slabs (gemm_partial_floats)
  int* counters = nullptr;   // split-K arrival tickets, zero-initialised (gemm_counter_slots)
  const void* zeros = nullptr;  // >= 256 zero bytes (padded / out-of-range chunks; conv_wres: a null bias)
  LnPtrs ln;
};

}  // namespace spi
