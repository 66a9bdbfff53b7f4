// Shifted-window attention for Swin Transformers (gfx950), head_dim 32, fp16 and fp32.
//
// qkv [B H W][3 C] holds the QKV GEMM's rows in plain NHWC pixel order, ctx [B H W][C] is written in the same
// order.  Window (wy, wx), token (ty, tx) is the pixel ((wy ws + ty + shift) mod H, (wx ws + tx + shift) mod W):
// torch.roll by -shift, the window partition, and their inverses exist only as this address.
//
// One 4-wave workgroup per (window, head); N = ws^2 <= 64 tokens are the 64 query slots (16 per wave) and the
// one 64-key tile:
//   * thread t stages 16-byte chunk t % CPR of token t / CPR (fp32: two rounds) of K and of V into row-major
//     LDS images, rows N .. 63 zero; threads 0 .. 63 write their token's shift region (3 ry + rx) to LDS;
//   * S^T = K Q^T: the key on the MFMA row, the query on the lane -- acc[j][r] is the score of key
//     16 j + 4 fq + r for query fr of the wave.  fp16: one v_mfma_f32_16x16x32_f16 per 16-key block (the head
//     dim is one k-step).  fp32: eight v_mfma_f32_16x16x4_f32, lane group fq holding head dims 8 fq .. 8 fq + 7;
//   * score = acc scale + bias + mask in fp32.  The bias comes packed per (head, key quad, query, 4 keys)
//     (swin_pack.hpp): one 16-byte load per accumulator, -inf on keys N .. 63.  The mask is -100 where the
//     query's and the key's regions differ, taken from the LDS region bytes (4 keys per 32-bit read), and only
//     in windows of the last window row or column of a shifted map -- everywhere else every region is 0;
//   * a lane's 16 scores are its own query's row: max and sum are in-lane plus two xor shuffles.  One key
//     tile, so no running max, no rescale, no key loop;
//   * O^T = V^T P^T with P^T straight from the accumulators.  fp16: converted in registers, V^T's fragments by
//     ds_read_b64_tr_b16 from the row-major image (96-byte rows: eight consecutive rows on disjoint 8-bank
//     spans, attention.hip's arithmetic).  fp32: k-step (j, r) takes key 16 j + 4 fq + r from lane group fq, so
//     the B operand is acc element r itself and the A operand one LDS float (144-byte rows put the four lane
//     groups' rows, 4 apart, 16 banks apart);
//   * 16-key blocks at or past N skip their MFMAs and reads, waves whose 16 slots are all at or past N leave
//     after the staging barrier -- both wave-uniform, EXEC full around the transposed reads; a query slot at
//     or past N stores nothing.
// No atomics, no workspace, one barrier; a launch's bits are fixed.
//
// COS (Swin v2): score = cos(q, k) tau_h + bias + mask, tau fp32 [heads] (the clamp is the host's).  K and Q go
// to the MFMA as they are stored and the two normalisations are factors of the fp32 score epilogue, in place of
// the scale: no operand is rounded a second time and LDS is not read twice.
//   * 1 / max(|k|, 1e-12) per key, from the staging registers: thread t holds chunk t % CPR of key t / CPR, so
//     the squares of its 8 (fp16) / 4 (fp32) elements are summed in fp32 and added over the CPR neighbouring
//     lanes by xor shuffles (1, 2 and, fp32, 4); the lane of chunk 0 writes the factor to a 64-float LDS array in
//     front of the one barrier (fp32: 32 keys per staging round).  Accumulator element r of block j is key
//     16 j + 4 fq + r: a lane's four factors are one 16-byte LDS read, the same address over a lane group;
//   * tau_h / max(|q|, 1e-12) per lane: the lane holds head dims 8 fq .. 8 fq + 7 of its query, so their squares
//     plus the xor shuffles 16 and 32 are |q|^2;
//   * both from 1.f / sqrtf, each correctly rounded (the compiler's default for HIP; no approximate rsq);
//   * a padded key (rows N .. 63 are zero) has factor 1e12 and accumulator exactly 0, a dead query slot factor
//     tau 1e12: the products stay finite (<= 100 * 1e24), so 0 inf never arises, and the -inf bias drops the key.
#include <stdexcept>
#include <string>

#include "row_util.hpp"
#include "spi_kernels.hpp"
#include "swin_pack.hpp"

namespace spi {
namespace {

// Do the 8-bank spans of eight consecutive LDS rows of row_bytes each miss one another (64 banks)?
constexpr bool win_tr_rows_disjoint(int row_bytes) {
  unsigned long long used = 0;
  for (int r = 0; r < 8; ++r)
    for (int k = 0; k < 8; ++k) {
      const unsigned long long bit = 1ull << ((r * row_bytes / 4 + k) % 64);
      if (used & bit) return false;
      used |= bit;
    }
  return true;
}

// The region of rolled coordinate p along an axis of length L (torchvision's three mask slices).
__device__ __forceinline__ int shift_region(int p, int L, int ws, int shift) {
  return p < L - ws ? 0 : p < L - shift ? 1 : 2;
}

// SP: the scale (v1), or tau [heads] (COS).
template <typename T, bool COS, typename SP>
__global__ __launch_bounds__(256) void window_attn_kernel(const T* __restrict__ qkv, const float* __restrict__ bias,
                                                          T* __restrict__ ctx, int H, int W, int heads, int ws,
                                                          int shift, SP scale) {
  constexpr bool F16 = sizeof(T) == 2;
  constexpr int HD = kWinHeadDim, NS = kWinSlots;
  constexpr int EPC = 16 / (int)sizeof(T);  // elements per 16-byte chunk
  constexpr int CPR = HD / EPC;             // chunks per K / V row: 4 (fp16), 8 (fp32)
  constexpr int LD = F16 ? 48 : 36;         // row stride in elements: 96 B (fp16), 144 B (fp32)
  constexpr int ROUNDS = NS * CPR / 256;    // staging rounds: 1 (fp16), 2 (fp32)
  static_assert(!F16 || win_tr_rows_disjoint(LD * 2), "the transposed read's eight rows on disjoint banks");
  static_assert((LD * sizeof(T)) % 16 == 0 && NS * CPR % 256 == 0, "16-byte rows, whole staging rounds");
  __shared__ __attribute__((aligned(16))) T Ks[NS * LD];
  __shared__ __attribute__((aligned(16))) T Vs[NS * LD];
  __shared__ __attribute__((aligned(16))) unsigned char reg[NS];
  __shared__ __attribute__((aligned(16))) float kinv[COS ? NS : 4];  // COS: 1 / max(|k|, 1e-12) per key slot

  const int N = ws * ws, nwx = W / ws, nwy = H / ws;
  const int win = blockIdx.x, h = blockIdx.y;
  const int wx = win % nwx, wy = (win / nwx) % nwy, b = win / (nwx * nwy);
  const int C = heads * HD, ld = 3 * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  // the qkv / ctx row of token t (t < N)
  auto pixel_row = [&](int t) {
    int y = wy * ws + t / ws + shift, x = wx * ws + t % ws + shift;
    y -= y >= H ? H : 0;
    x -= x >= W ? W : 0;
    return ((size_t)b * H + y) * W + x;
  };
  const bool masked = shift > 0 && (wy == nwy - 1 || wx == nwx - 1);  // workgroup-uniform

  uint4 kreg[ROUNDS], vreg[ROUNDS];
#pragma unroll
  for (int i = 0; i < ROUNDS; ++i) {
    const int c = tid + i * 256;
    const int key = c / CPR, dc = c % CPR;
    kreg[i] = vreg[i] = make_uint4(0, 0, 0, 0);
    if (key < N) {
      const T* row = qkv + pixel_row(key) * ld + h * HD + dc * EPC;
      kreg[i] = *reinterpret_cast<const uint4*>(row + C);
      vreg[i] = *reinterpret_cast<const uint4*>(row + 2 * C);
    }
  }
  // this lane's query: slot qa of the window, its Q^T fragment as the B operand
  const int qa = wave * 16 + fr;
  const bool qlive = qa < N;
  const size_t qrow = qlive ? pixel_row(qa) : 0;
  half8 qh = {0, 0, 0, 0, 0, 0, 0, 0};
  floatx4 qf[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
  if (qlive) {
    const T* q = qkv + qrow * ld + h * HD + fq * 8;
    if constexpr (F16) {
      qh = *reinterpret_cast<const half8*>(q);
    } else {
      qf[0] = *reinterpret_cast<const floatx4*>(q);
      qf[1] = *reinterpret_cast<const floatx4*>(q + 4);
    }
  }
#pragma unroll
  for (int i = 0; i < ROUNDS; ++i) {
    const int c = tid + i * 256;
    const int key = c / CPR, dc = c % CPR;
    *reinterpret_cast<uint4*>(Ks + key * LD + dc * EPC) = kreg[i];
    *reinterpret_cast<uint4*>(Vs + key * LD + dc * EPC) = vreg[i];
    if constexpr (COS) {
      float ss = 0.f;
      if constexpr (F16) {
        const half8 kh = __builtin_bit_cast(half8, kreg[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (float)kh[e] * (float)kh[e];
      } else {
        const floatx4 kf = __builtin_bit_cast(floatx4, kreg[i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += kf[e] * kf[e];
      }
#pragma unroll
      for (int o = 1; o < CPR; o <<= 1) ss += __shfl_xor(ss, o, 64);
      if (dc == 0) kinv[key] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    }
  }
  if (tid < NS) {
    const int t = tid < N ? tid : 0;
    reg[tid] = (unsigned char)(3 * shift_region(wy * ws + t / ws, H, ws, shift) + shift_region(wx * ws + t % ws, W, ws, shift));
  }
  __syncthreads();
  if (wave * 16 >= N) return;  // wave-uniform; no barrier follows

  // S^T, bias, mask
  const int nblk = (N + 15) >> 4;  // live 16-key blocks
  const float* bh = bias + (size_t)h * kWinBiasHead + (size_t)qa * 4;
  const int qreg = masked ? reg[qa] : 0;
  float qfac = 0.f;  // COS: tau_h / max(|q|, 1e-12)
  if constexpr (COS) {
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = F16 ? (float)qh[e] : qf[e >> 2][e & 3];
      ss += v * v;
    }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    qfac = scale[h] * (1.f / fmaxf(sqrtf(ss), 1e-12f));
  }
  float sc[4][4];
  float tmax = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= nblk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[j][r] = -INFINITY;
      continue;
    }
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (F16) {
      const half8 kf = *reinterpret_cast<const half8*>(Ks + (j * 16 + fr) * LD + fq * 8);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qh, acc, 0, 0, 0);
    } else {
      const float* kr = reinterpret_cast<const float*>(Ks) + (j * 16 + fr) * LD + fq * 8;
#pragma unroll
      for (int s4 = 0; s4 < 2; ++s4) {
        const floatx4 kv = *reinterpret_cast<const floatx4*>(kr + s4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[e], qf[s4][e], acc, 0, 0, 0);
      }
    }
    const floatx4 bv = *reinterpret_cast<const floatx4*>(bh + (size_t)(j * 4 + fq) * (kWinSlots * 4));
    unsigned kregs = 0;
    if (masked) kregs = *reinterpret_cast<const unsigned*>(reg + j * 16 + fq * 4);
    floatx4 kfac = {0.f, 0.f, 0.f, 0.f};
    if constexpr (COS) kfac = *reinterpret_cast<const floatx4*>(kinv + j * 16 + fq * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v;
      if constexpr (COS) v = acc[r] * kfac[r] * qfac + bv[r];
      else v = acc[r] * scale + bv[r];
      if (masked && (int)((kregs >> (8 * r)) & 0xff) != qreg) v += -100.0f;
      sc[j][r] = v;
      tmax = fmaxf(tmax, v);
    }
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  float rs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[j][r] = __expf(sc[j][r] - tmax);  // P^T; 0 on the excluded keys
      rs += sc[j][r];
    }
  rs += __shfl_xor(rs, 16, 64);
  rs += __shfl_xor(rs, 32, 64);

  // O^T = V^T P^T: o[d][r] is head dim 16 d + 4 fq + r of query fr
  floatx4 o[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
  if constexpr (F16) {
    typedef short short4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) short4v lds_s4;
    // lane (fq, fr) addresses row 4 fq + fr / 4, columns 4 (fr % 4) of a 16-key x 16-column block
    __attribute__((address_space(3))) char* vb =
        (__attribute__((address_space(3))) char*)Vs + ((4 * fq + (fr >> 2)) * LD + 4 * (fr & 3)) * 2;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s * 2 >= nblk) break;
      half8 pf;  // element 4 t + r = key 16 (2 s + t) + 4 fq + r
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[e] = static_cast<_Float16>(sc[2 * s + (e >> 2)][e & 3]);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const half4 lo = __builtin_bit_cast(
            half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(vb + ((32 * s) * LD + 16 * d) * 2)));
        const half4 hi = __builtin_bit_cast(
            half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(vb + ((32 * s + 16) * LD + 16 * d) * 2)));
        const half8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[d], 0, 0, 0);
      }
    }
  } else {
    const float* vr = reinterpret_cast<const float*>(Vs) + (4 * fq) * LD + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nblk) break;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int d = 0; d < 2; ++d)
          o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[(j * 16 + r) * LD + d * 16], sc[j][r], o[d], 0, 0, 0);
    }
  }

  if (qlive) {
    const float inv = 1.f / rs;
    T* out = ctx + qrow * C + h * HD + fq * 4;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const float v[4] = {o[d][0] * inv, o[d][1] * inv, o[d][2] * inv, o[d][3] * inv};
      store4(out + d * 16, v);
    }
  }
}

}  // namespace

namespace {

void check_window(const std::string& what, const void* qkv, const float* rel_bias, const void* ctx, int B, int H, int W,
                  int heads, int hd, int window, int shift) {
  if (hd != kWinHeadDim) throw std::invalid_argument(what + ": head_dim " + std::to_string(hd) + " is not served (32)");
  if (!window_supported(window))
    throw std::invalid_argument(what + ": window " + std::to_string(window) + " is not served (2 .. 8: at most 64 tokens)");
  if (B < 1 || H < window || W < window || H % window || W % window)
    throw std::invalid_argument(what + ": H " + std::to_string(H) + " and W " + std::to_string(W) +
                                " must be positive multiples of the window " + std::to_string(window));
  if (shift < 0 || shift >= window)
    throw std::invalid_argument(what + ": shift " + std::to_string(shift) + " must be in 0 .. window - 1");
  const long long windows = (long long)B * (H / window) * (W / window);
  if (heads < 1 || heads > 65535 || windows > 0x7fffffffLL)
    throw std::invalid_argument(what + ": heads (at most 65535) and B (H / ws) (W / ws) (below 2^31) are the grid");
  if (!aligned(qkv, 16) || !aligned(ctx, 16) || !aligned(rel_bias, 16))
    throw std::invalid_argument(what + ": 16-byte aligned qkv, ctx and rel_bias");
}

}  // namespace

void window_attention(const void* qkv, const float* rel_bias, void* ctx, int B, int H, int W, int heads, int hd,
                      int window, int shift, float scale, bool f16, hipStream_t s) {
  check_window("window_attention", qkv, rel_bias, ctx, B, H, W, heads, hd, window, shift);
  const dim3 grid((unsigned)(B * (H / window) * (W / window)), (unsigned)heads);
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((window_attn_kernel<T, false, float>), grid, dim3(256), 0, s, static_cast<const T*>(qkv), rel_bias,
               static_cast<T*>(ctx), H, W, heads, window, shift, scale);
  });
}

void window_attention_cos(const void* qkv, const float* rel_bias, const float* tau, void* ctx, int B, int H, int W,
                          int heads, int hd, int window, int shift, bool f16, hipStream_t s) {
  check_window("window_attention_cos", qkv, rel_bias, ctx, B, H, W, heads, hd, window, shift);
  if (!tau || !aligned(tau, 4)) throw std::invalid_argument("window_attention_cos: tau must be a 4-byte aligned fp32 [heads]");
  const dim3 grid((unsigned)(B * (H / window) * (W / window)), (unsigned)heads);
  with_type(f16, [&](auto t) {
    using T = decltype(t);
    SPI_LAUNCH((window_attn_kernel<T, true, const float*>), grid, dim3(256), 0, s, static_cast<const T*>(qkv), rel_bias,
               static_cast<T*>(ctx), H, W, heads, window, shift, tau);
  });
}

}  // namespace spi
