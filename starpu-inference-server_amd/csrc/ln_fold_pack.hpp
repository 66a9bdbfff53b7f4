// LayerNorm fold, the host side (ln_fold.hpp is the device side): the arithmetic that turns a
// linear layer behind a LayerNorm, y = LN(x) W^T + b, into the operands of the folding GEMM.
// Plain C++ on host arrays -- shared by model replicas (pack_linear_folded) and the op-level
// API (spi_op_fold_linear), so the packing is testable without a model.
#pragma once
#include <cstddef>

namespace spi {

// w [N][K], b [N] or null, gamma / beta [K] ->
//   w_folded [N][K] = W diag(gamma), rounded to fp32;
//   bias [N]        = b + W beta (accumulated in double);
//   c1 [N]          = sum_k of w_folded as the GEMM's MFMAs will see it -- rounded to fp16 when
//                     f16 (hi + lo, both halves as packed, when hilo), else the fp32 values --
//                     so the epilogue's rstd (x W'^T - mean c1) cancels exactly what was accumulated.
inline void fold_linear(const float* w, const float* b, int N, int K, const float* gamma, const float* beta,
                        bool f16, bool hilo, float* w_folded, float* bias, float* c1) {
  for (int n = 0; n < N; ++n) {
    double bb = b ? b[n] : 0.0, cc = 0.0;
    for (int k = 0; k < K; ++k) {
      const float v = w[(size_t)n * K + k];
      const float f = v * gamma[k];
      w_folded[(size_t)n * K + k] = f;
      bb += (double)beta[k] * v;
      if (f16) {
        const float hi = static_cast<float>(static_cast<_Float16>(f));
        cc += hilo ? (double)hi + (double)static_cast<float>(static_cast<_Float16>(f - hi)) : (double)hi;
      } else {
        cc += (double)f;
      }
    }
    bias[n] = (float)bb;
    c1[n] = (float)cc;
  }
}

}  // namespace spi
