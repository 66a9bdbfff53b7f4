// Fused ResNet stem for gfx950: the task's image (NCHW fp32, or 8-bit pixels NCHW /
// NHWC with the per-channel input transform applied at the load) -> 7x7/s2/p3 conv +
// folded BN + ReLU -> 3x3/s2/p1 max pool -> the first stage's NHWC activation,
// in one launch (torchvision's conv1 / bn1 / relu / maxpool; SURVEY.md A14 "cast
// fused into the first kernel").  It replaces three launches of the generic path
// (ingest_nchw, the stem as an implicit GEMM over a padded NHWC copy, max pool):
// the 6.4 MB NHWC copy and the 12.8 MB (bs8, fp16) stem output never reach HBM.
//
// Workgroup = PR pooled rows of one image = R = 2 PR + 1 stem rows (the pool's
// row above is recomputed, (2 PR + 1) / 2 PR).  4 waves; wave w owns output
// channels [16 w, 16 w + 16) (its weights stay in registers for the launch:
// [hi | lo][64][24][8] fp16, 48 VGPRs split, 24 plain).
//
// Contraction order: k = (c, kh, kw) with kw padded to 8 -- 24 groups of 8
// (21 real, 3 zero), 6 k-steps of v_mfma_f32_16x16x32_f16.  A lane's fragment
// is 8 horizontally adjacent input pixels of one (channel, input row):
// columns 2 ow - 3 .. 2 ow + 4 (the kw = 7 weight is zero).  The workgroup's
// input rows are converted once into LDS planes (fp16 hi and, split modes,
// lo = fp16(x - hi)) indexed by column + 3, so the fragment is dwords
// [ow, ow + 4) of its plane.
//
// Phase-interleaved fragments: M-fragment `ph` of a 64-pixel group holds
// pixels ow = 64 grp + 4 i + ph (i = fragment row 0..15).  Its lane window,
// dwords [4 i + ph, 4 i + ph + 4), lies inside the two 16-byte-aligned blocks
// [4 i, 4 i + 8): two ds_read_b128 serve the four phase fragments, each one a
// compile-time selection of 4 of those 8 dwords (a plain per-pixel mapping
// would need 4-byte-aligned ds_read2_b32 at half the LDS rate, once per
// fragment).  Planes are 512 bytes apart, so the lane groups of a b128 read
// hit distinct banks.
//
// Epilogue in registers: with that mapping a lane holds 16 consecutive stem
// columns (64 grp + 16 (lane >> 4) + 4 v + ph) of one channel for every stem
// row; the vertical max is per lane, the horizontal max needs the column to the
// left from lane - 16 (ds_bpermute), and for the first lane group from the
// previous group (carried).  ReLU outputs are >= 0, so invalid pixels (outside
// the map) enter the max as 0; fragment rows past the map read finite LDS bytes
// and are discarded (MFMA rows are independent).  max commutes with the monotone
// fp16 rounding, so pooling the fp32 values and rounding once is what pooling
// the rounded stem outputs gives.
#include "lds_dma.hpp"
#include "pack.hpp"
#include "spi_kernels.hpp"

#include <cstdlib>
#include <stdexcept>
#include <type_traits>

namespace spi {
namespace {

typedef unsigned int u32x8 __attribute__((ext_vector_type(8)));

constexpr int kCout = 64;
constexpr int kGroups = 24;  // (c, kh) groups of 8 kw values: 21 real + 3 zero
constexpr int kSteps = kGroups / 4;

template <int PR>
struct Geom {
  static constexpr int R = 2 * PR + 1;  // stem rows per workgroup
  static constexpr int NR = 2 * R + 5;  // input rows per workgroup
  static constexpr int WP = 256;        // plane width (fp16): columns -3 .. 2 kStemPoolMaxOW + 4, 512 B
  static constexpr int NPL = 3 * NR;    // planes (channel, input row)
  // one plane image in dwords, + slack: the last group's rows past the map read up to
  // 32 dwords beyond the last plane
  static constexpr int PD = NPL * WP / 2 + 32;
};
static_assert(2 * kStemPoolMaxOW + 5 < Geom<1>::WP, "plane covers the valid windows");

// phase PH_'s fragment from an 8-dword block pair: dwords (PH_ & 2) .. (PH_ & 2) + 3
template <int PH_>
__device__ __forceinline__ half8 window(const u32x8& b) {
  if constexpr (PH_ & 2)
    return __builtin_bit_cast(half8, __builtin_shufflevector(b, b, 2, 3, 4, 5));
  else
    return __builtin_bit_cast(half8, __builtin_shufflevector(b, b, 0, 1, 2, 3));
}

// OUT 0: fp16 NHWC [B][PH][PW][64]; 1: split NHWC (per pixel [32 hi | 32 lo] x 2).
// SRC (SrcKind) 0: fp32 NCHW image; 1 / 2: 8-bit pixels, NCHW / NHWC -- only the plane fill differs:
// pixel p of channel c enters as fl(fl(p * scale[c]) + shift[c]) (two fp32 roundings, never an FMA, so
// a host reproduces it bit for bit) and is rounded to the planes exactly as an fp32 input is.  The
// bytes are fetched as aligned dwords at any alignment of the image, of a row or of the batch stride
// (see the fill).  Pixels outside the image enter as 0.0, not as shift[c]: the conv pads the
// transformed image.
// LOM 0: fp16 image x fp16 weights (one MFMA per fragment pair); 1: fp16 image x hi + lo weights
// (two: fp16m, round 5 -- the image's own fp16 rounding costs C2 0.03e-3 of parity margin,
// tools/prec_emulate.py, and its lo planes + third MFMA a third of the launch); 2: split image x
// split weights (three: fp16x3, fp32-grade).
template <int PR, int NW, int LOM, int OUT, int SRC>
__global__ __launch_bounds__(64 * NW) void stem_pool_kernel(const void* __restrict__ xv, const _Float16* __restrict__ w,
                                                            const float* __restrict__ bias, void* __restrict__ y, int H,
                                                            int W, int OH, int OW, int PH, int PW, int diag,
                                                            InputXf xf) {
  using G = Geom<PR>;
  constexpr int R = G::R, NR = G::NR, WP = G::WP, NPL = G::NPL, PD = G::PD, NT = 64 * NW;
  static_assert(NW == 4 || NW == 8, "4 waves (one per 16 channels), or 8 (x 2 pixel groups)");
  static_assert(NW == 4 || kStemPoolMaxOW <= 128, "8 waves: one 64-pixel group per wave");
  constexpr bool LO = LOM == 2;   // lo image planes
  constexpr bool WLO = LOM >= 1;  // lo weights
  // images: [copy 0 hi | copy 1 hi | copy 0 lo | copy 1 lo], copy 1 = copy 0 shifted one dword
  __shared__ __attribute__((aligned(16))) unsigned lds[(LO ? 4 : 2) * PD];
  __shared__ float xch[NW == 8 ? 2 * PR * kCout : 1];  // 8 waves: group 0's last column per pooled row
  const int b = blockIdx.y;
  const int pr0 = blockIdx.x * PR;
  const int sr0 = 2 * pr0 - 1;  // first stem row (the pool's padding row for pr0 = 0)
  const int ir0 = 2 * sr0 - 3;  // first input row
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int n = (wave & 3) * 16 + fr;

  // weights first: L2-resident, their latency overlaps the plane fill
  half8 wh[kSteps], wl[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const _Float16* src = w + ((size_t)n * kGroups + 4 * s + fq) * 8;
    wh[s] = *reinterpret_cast<const half8*>(src);
    if constexpr (WLO) wl[s] = *reinterpret_cast<const half8*>(src + kCout * kGroups * 8);
  }
  const float bn = bias[n];
  if (diag == 3) return;  // diagnostic (SPI_STEM_DIAG): empty launch

  // planes: (c, input row ir0 + r) at lds[(c * NR + r) * WP + col + 3]; zero outside
  // the image.  Unrolled: every thread's loads are in flight before the first LDS
  // store (a rolled loop waits out one memory latency per iteration).
  constexpr int HALF = WP / 2;
  unsigned* ldw = lds;
  auto pack2 = [](_Float16 a, _Float16 b) {
    return __builtin_bit_cast(unsigned short, a) | (unsigned)__builtin_bit_cast(unsigned short, b) << 16;
  };
  if constexpr (SRC == kSrcF32Nchw) {
    constexpr int ITER = (NPL * HALF + NT - 1) / NT;
    float v[ITER][2];
    const float* xb = static_cast<const float*>(xv) + (size_t)b * 3 * H * W;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int e = tid + it * NT;
      const int p = e / HALF, i = (e - p * HALF) * 2;
      const int c = p / NR, r = ir0 + (p - c * NR);
      v[it][0] = v[it][1] = 0.f;
      if (e < NPL * HALF && r >= 0 && r < H && diag != 1) {
        const float* row = xb + ((size_t)c * H + r) * W;
        const int c0 = i - 3;
        if (c0 >= 0 && c0 < W) v[it][0] = row[c0];
        if (c0 + 1 >= 0 && c0 + 1 < W) v[it][1] = row[c0 + 1];
      }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int e = tid + it * NT;
      if (e >= NPL * HALF) continue;
      const _Float16 h0 = static_cast<_Float16>(v[it][0]), h1 = static_cast<_Float16>(v[it][1]);
      const unsigned hw = pack2(h0, h1);
      ldw[e] = hw;
      if (e) ldw[PD + e - 1] = hw;
      if constexpr (LO) {
        const unsigned lw = pack2(static_cast<_Float16>(v[it][0] - static_cast<float>(h0)),
                                  static_cast<_Float16>(v[it][1] - static_cast<float>(h1)));
        ldw[2 * PD + e] = lw;
        if (e) ldw[3 * PD + e - 1] = lw;
      }
    }
  } else {
    // 8-bit pixels.  One wave fills one plane row per step; lane L owns the row's columns
    // 4 L - 3 .. 4 L, i.e. plane dwords 2 L and 2 L + 1 (64 lanes = the 256-column plane).  Bytes
    // are fetched as ALIGNED dwords whatever the row's address: with a0 = the row address & 3, the
    // lane's bytes start `sh` bytes into aligned dword `idx` of the row's first aligned word, so
    // the lane loads that dword, takes the next from lane + 1 (which loaded it) and extracts its
    // bytes with one v_alignbyte.  A byte load costs the texture path as much as a dword load, so
    // this is a quarter of the load instructions of a per-pixel fetch, at any alignment -- rows
    // that start at odd addresses (W % 4 != 0, odd 3 H W, a sliced buffer) take the same path with
    // another shift.  Every dword loaded overlaps the row's bytes, so it shares its 4-byte word,
    // hence its page, with a byte of the image; bytes of it that belong to a neighbouring row (or
    // lie up to 3 bytes outside the image) are discarded by the per-pixel range test, which also
    // makes out-of-image pixels 0.0 rather than shift[c].
    // NHWC: one step is one input row for all three channels -- the lane's 4 pixels are 12
    // consecutive bytes (3 dwords + the next lane's first), byte k = pixel k / 3, channel k % 3.
    constexpr bool NHWC = SRC == kSrcU8Nhwc;
    constexpr int NROW = NHWC ? NR : NPL;  // steps: input rows (NHWC) or planes
    constexpr int ND = NHWC ? 3 : 1;       // dwords a lane loads per step
    constexpr int ITER = (NROW * 64 + NT - 1) / NT;
    const unsigned char* xb = static_cast<const unsigned char*>(xv) + (size_t)b * 3 * H * W;
    const int rowbytes = NHWC ? 3 * W : W;
    unsigned raw[ITER][ND];
    int shv[ITER];
    // the six transform values in scalar registers once: picked per step by the (wave-uniform)
    // channel, not fetched from the kernel arguments at each use
    const float sc0 = xf.scale[0], sc1 = xf.scale[1], sc2 = xf.scale[2];
    const float sh0 = xf.shift[0], sh1 = xf.shift[1], sh2 = xf.shift[2];
    // Branch-free loads: a load under a per-lane or per-step condition is waited for at the end of
    // its block, which serialises the steps on the memory latency.  So every lane loads in every
    // step, from an address clamped into the image -- the step's row into [0, H), the dword into
    // those that overlap the row -- and what a clamp substituted feeds only pixels that the range
    // test below zeroes (a dword that does not overlap the row holds none of its pixels).
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int row = min(wave + it * NW, NROW - 1);  // wave-uniform; a step past the last repeats it
      const int c = NHWC ? 0 : row / NR, r = min(max(ir0 + (NHWC ? row : row - c * NR), 0), H - 1);
      const unsigned char* rp = xb + (NHWC ? (size_t)r * rowbytes : ((size_t)c * H + r) * W);
      const int a0 = (int)(reinterpret_cast<uintptr_t>(rp) & 3);
      // the lane's first byte (column 4 L - 3) is at aligned byte ND 4 (L - 1) + (a0 + ND)
      const int idx = ND * (lane - 1) + ((a0 + ND) >> 2);
      shv[it] = (a0 + ND) & 3;
      const unsigned* ap = reinterpret_cast<const unsigned*>(rp - a0);
      const int klast = (a0 + rowbytes - 1) >> 2;  // dwords 0 .. klast overlap the row's bytes
#pragma unroll
      for (int d = 0; d < ND; ++d) raw[it][d] = ap[min(max(idx + d, 0), klast)];
    }
    // plane dword e of every copy, as the fp32 fill writes it -- without that fill's `if (e)` in front
    // of the shifted copies: dword 0 (plane 0's columns -3, -2, always 0) then lands on the last
    // slack dword of the copy before, which the slack fill below zeroes too
    auto put = [&](int e, float v0, float v1) {
      const _Float16 h0 = static_cast<_Float16>(v0), h1 = static_cast<_Float16>(v1);
      const unsigned hw = pack2(h0, h1);
      ldw[e] = hw;
      ldw[PD + e - 1] = hw;
      if constexpr (LO) {
        const unsigned lw = pack2(static_cast<_Float16>(v0 - static_cast<float>(h0)),
                                  static_cast<_Float16>(v1 - static_cast<float>(h1)));
        ldw[2 * PD + e] = lw;
        ldw[3 * PD + e - 1] = lw;
      }
    };
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int row = wave + it * NW;
      // every lane takes part in the exchange (the step's control flow is wave-uniform); lane 63
      // gets 0, and its columns (249 ..) are past any image
      // (DPP wave_shl:1, a VALU move: lane i reads lane i + 1 without the LDS round trip of a
      // ds_bpermute, which would sit on every step's dependent chain)
      const unsigned next = (unsigned)__builtin_amdgcn_update_dpp(0, (int)raw[it][0], 0x130, 0xf, 0xf, true);
      if (row >= NROW) continue;
      const int c = NHWC ? 0 : row / NR, r = ir0 + (NHWC ? row : row - c * NR);
      const bool rin = r >= 0 && r < H && diag != 1;
      unsigned bytes[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d)
        bytes[d] = __builtin_amdgcn_alignbyte(d + 1 < ND ? raw[it][d + 1] : next, raw[it][d], (unsigned)shv[it]);
      const int c0 = 4 * lane - 3;
#pragma unroll
      for (int ch = 0; ch < (NHWC ? 3 : 1); ++ch) {
        const int cc = NHWC ? ch : c;
        const float sc = cc == 0 ? sc0 : cc == 1 ? sc1 : sc2, sh = cc == 0 ? sh0 : cc == 1 ? sh1 : sh2;
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = NHWC ? 3 * t + ch : t;  // byte of the lane's 4 ND bytes
          const unsigned char px = (unsigned char)(bytes[k >> 2] >> (8 * (k & 3)));
          const float val = input_xf_apply(px, sc, sh);
          v[t] = rin && c0 + t >= 0 && c0 + t < W ? val : 0.f;
        }
        const int e = ((NHWC ? ch * NR + row : row) * HALF) + 2 * lane;
        put(e, v[0], v[1]);
        put(e + 1, v[2], v[3]);
      }
    }
  }
  if (tid < 33) {  // the slack after the last plane: finite bytes for the discarded rows
#pragma unroll
    for (int c = 0; c < (LO ? 4 : 2); ++c) {
      if (c & 1)
        ldw[c * PD + NPL * HALF - 1 + tid] = 0u;  // copy 1: its last dword is copy 0's first slack dword
      else if (tid < 32)
        ldw[c * PD + NPL * HALF + tid] = 0u;
    }
  }
  __syncthreads();

  // per k-step plane (dword offset) of this lane's group (c, kh); zero groups read plane 0
  int goff[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int g = 4 * s + fq;
    const int c = g < 21 ? g / 7 : 0, kh = g < 21 ? g - 7 * (g / 7) : 0;
    goff[s] = (c * NR + kh) * HALF;
  }

  const int NG = diag == 2 ? 0 : (OW + 63) >> 6;  // diagnostic 2: fill only
  // Stem rows of one 64-pixel group, folded as they complete (bias + ReLU, invalid
  // pixels as 0) into the vertical max of each pooled row; lane column t = 4 v + ph
  // is stem column 64 grp + 16 fq + t.
  auto compute = [&](int grp, float (&vm)[PR][16]) {
    const int blk = grp * 64 + 4 * fr;  // dword of this lane's first block
    const int o0 = grp * 64 + 16 * fq;
    float bt[16];  // bias per lane column; -inf past the map, so ReLU sends those to 0
#pragma unroll
    for (int t = 0; t < 16; ++t) bt[t] = o0 + t < OW ? bn : -__builtin_inff();
#pragma unroll
    for (int p = 0; p < PR; ++p)
#pragma unroll
      for (int t = 0; t < 16; ++t) vm[p][t] = 0.f;
    floatx4 acc[4];
    // (stem row, k-step) steps, software-pipelined: step t + 1's blocks are read
    // before step t's twelve (split) / four MFMAs are issued.  A step reads dwords
    // [4 i, 4 i + 8) of copy 0 and of copy 1 (copy 0 shifted one dword) as 8-dword
    // vectors (two ds_read_b128 each, consecutive registers): phase 0 / 2 windows are
    // dwords 0-3 / 2-5 of copy 0, phase 1 / 3 the same of copy 1 -- even-aligned
    // register sub-ranges, so no window needs a register move.
    constexpr int T = kSteps * R;
    constexpr int NB = LO ? 4 : 2;
    u32x8 blk_[2][NB];
    auto load = [&](int t, u32x8(&dst)[NB]) {
      const int r = t / kSteps, s = t - r * kSteps;
      const unsigned* src = ldw + goff[s] + r * WP + blk;
#pragma unroll
      for (int c = 0; c < NB; ++c) dst[c] = *reinterpret_cast<const u32x8*>(src + c * PD);
    };
    load(0, blk_[0]);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int r = t / kSteps, s = t - r * kSteps;
      if (s == 0)
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) acc[ph] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (t + 1 < T) load(t + 1, blk_[(t + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      const u32x8(&bb)[NB] = blk_[t & 1];
      auto mma = [&](auto phc) {
        constexpr int P = decltype(phc)::value;
        const half8 ah = window<P>(bb[P & 1]);
        if constexpr (LO) {
          const half8 al = window<P>(bb[2 + (P & 1)]);
          acc[P] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh[s], acc[P], 0, 0, 0);
        }
        if constexpr (WLO) acc[P] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl[s], acc[P], 0, 0, 0);
        acc[P] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh[s], acc[P], 0, 0, 0);
      };
      mma(std::integral_constant<int, 0>{});
      mma(std::integral_constant<int, 1>{});
      mma(std::integral_constant<int, 2>{});
      mma(std::integral_constant<int, 3>{});
      __builtin_amdgcn_sched_barrier(0);
      // row r complete: fold it into the pooled rows it belongs to (rows outside the
      // map skipped -- a wave-uniform test; columns past the map carry a -inf bias)
      if (s == kSteps - 1 && sr0 + r >= 0 && sr0 + r < OH) {
#pragma unroll
        for (int vv = 0; vv < 4; ++vv)
#pragma unroll
          for (int ph = 0; ph < 4; ++ph) {
            const int tt = 4 * vv + ph;
            const float u = acc[ph][vv] + bt[tt];
#pragma unroll
            for (int p = 0; p < PR; ++p)
              if (r >= 2 * p && r <= 2 * p + 2) vm[p][tt] = __builtin_fmaxf(__builtin_fmaxf(vm[p][tt], u), 0.f);
          }
      }
    }
  };
  // horizontal: pooled columns o0 / 2 + q, q = 0..7 (stem columns o0 + 2q - 1 .. o0 + 2q + 1);
  // column o0 - 1 from lane - 16, or for the first lane group `first` (the previous group's last)
  auto store = [&](int grp, const float (&vm)[PR][16], const float (&first)[PR]) {
    const int o0 = grp * 64 + 16 * fq;
#pragma unroll
    for (int p = 0; p < PR; ++p) {
      float left = __shfl_up(vm[p][15], 16, 64);
      if (fq == 0) left = first[p];
      const int pr = pr0 + p;
      if (pr >= PH) continue;
      const size_t m0 = ((size_t)b * PH + pr) * PW;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float l = q ? vm[p][2 * q - 1] : left;
        const float val = fmaxf(l, fmaxf(vm[p][2 * q], vm[p][2 * q + 1]));
        const int pc = o0 / 2 + q;
        if (pc >= PW) continue;
        const _Float16 hi = static_cast<_Float16>(val);
        if constexpr (OUT == 0) {
          static_cast<_Float16*>(y)[(m0 + pc) * kCout + n] = hi;
        } else {
          _Float16* o = static_cast<_Float16*>(y) + (m0 + pc) * kCout * 2 + (n >> 5) * 64 + (n & 31);
          o[0] = hi;
          o[32] = static_cast<_Float16>(val - static_cast<float>(hi));
        }
      }
    }
  };
  float vm[PR][16];
  if constexpr (NW == 4) {  // one wave walks every group, carrying the boundary column
    float carry[PR];
#pragma unroll
    for (int p = 0; p < PR; ++p) carry[p] = 0.f;
    for (int grp = 0; grp < NG; ++grp) {
      compute(grp, vm);
      store(grp, vm, carry);
#pragma unroll
      for (int p = 0; p < PR; ++p) carry[p] = __shfl(vm[p][15], 48 + fr, 64);
    }
  } else {  // waves 0-3 group 0, waves 4-7 group 1; group 0's last column through LDS
    const int grp = wave >> 2;
    const bool active = grp < NG;
    if (active) {
      compute(grp, vm);
      if (grp == 0 && fq == 3)
#pragma unroll
        for (int p = 0; p < PR; ++p) xch[p * kCout + n] = vm[p][15];
    }
    __syncthreads();
    if (active) {
      float first[PR];
#pragma unroll
      for (int p = 0; p < PR; ++p) first[p] = grp ? xch[p * kCout + n] : 0.f;
      store(grp, vm, first);
    }
  }
}

template <int PR, int NW, int SRC>
void launch_src(const void* x, const _Float16* w, const float* bias, void* y, int B, int H, int W, int OH, int OW,
                int PH, int PW, int lo, bool split, const InputXf& xf, hipStream_t s) {
  // diagnostic builds only (-DSPI_STEM_DIAG=1: no image loads, 2: fill only, 3: empty)
#ifdef SPI_STEM_DIAG
  constexpr int diag = SPI_STEM_DIAG;
#else
  constexpr int diag = 0;
#endif
  const dim3 grid((PH + PR - 1) / PR, B), block(64 * NW);
  if (split)
    SPI_LAUNCH((stem_pool_kernel<PR, NW, 2, 1, SRC>), grid, block, 0, s, x, w, bias, y, H, W, OH, OW, PH, PW, diag,
               xf);
  else if (lo == 2)
    SPI_LAUNCH((stem_pool_kernel<PR, NW, 2, 0, SRC>), grid, block, 0, s, x, w, bias, y, H, W, OH, OW, PH, PW, diag,
               xf);
  else if (lo == 1)
    SPI_LAUNCH((stem_pool_kernel<PR, NW, 1, 0, SRC>), grid, block, 0, s, x, w, bias, y, H, W, OH, OW, PH, PW, diag,
               xf);
  else
    SPI_LAUNCH((stem_pool_kernel<PR, NW, 0, 0, SRC>), grid, block, 0, s, x, w, bias, y, H, W, OH, OW, PH, PW, diag,
               xf);
}

template <int PR, int NW>
void launch_pr(const void* x, const _Float16* w, const float* bias, void* y, int B, int H, int W, int OH, int OW,
               int PH, int PW, int lo, bool split, int src, const InputXf& xf, hipStream_t s) {
  if (src == kSrcU8Nchw)
    launch_src<PR, NW, kSrcU8Nchw>(x, w, bias, y, B, H, W, OH, OW, PH, PW, lo, split, xf, s);
  else if (src == kSrcU8Nhwc)
    launch_src<PR, NW, kSrcU8Nhwc>(x, w, bias, y, B, H, W, OH, OW, PH, PW, lo, split, xf, s);
  else
    launch_src<PR, NW, kSrcF32Nchw>(x, w, bias, y, B, H, W, OH, OW, PH, PW, lo, split, xf, s);
}

}  // namespace

void stem_pool(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int lo, bool split,
               int pr, hipStream_t s, int src, const InputXf& xf) {
  const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
  const int PH = (OH + 2 - 3) / 2 + 1, PW = (OW + 2 - 3) / 2 + 1;
  if (OW > kStemPoolMaxOW || OH < 1 || OW < 1 || B < 1) throw std::runtime_error("stem_pool: unsupported image size");
  if (split && lo != 2) throw std::runtime_error("stem_pool: split output needs the split image and weights");
  if (lo < 0 || lo > 2) throw std::runtime_error("stem_pool: lo is 0, 1 or 2");
  if (src < kSrcF32Nchw || src > kSrcU8Nhwc) throw std::runtime_error("stem_pool: unknown source kind");
  const _Float16* wp = static_cast<const _Float16*>(w);
  // pr: 1 / 2 pooled rows per 4-wave workgroup; 0 (default): two rows per 8-wave
  // workgroup (one 64-pixel group per wave) when the map has two groups, else 1 x 4 waves
  if (pr == 2)
    launch_pr<2, 4>(x, wp, bias, y, B, H, W, OH, OW, PH, PW, lo, split, src, xf, s);
  else if (pr == 1 || OW <= 64)
    launch_pr<1, 4>(x, wp, bias, y, B, H, W, OH, OW, PH, PW, lo, split, src, xf, s);
  else
    launch_pr<2, 8>(x, wp, bias, y, B, H, W, OH, OW, PH, PW, lo, split, src, xf, s);
}

}  // namespace spi
