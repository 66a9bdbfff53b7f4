// Tile geometry of the general GEMM kernel (gemm.hip) as numbers only.  Plain C++17, no HIP
// header: the kernel takes its constants from TileGeo<>, the planner (gemm_plan.hpp) sizes k-steps
// and halo bands by the same definitions.
#pragma once
#include <algorithm>

#include "gemm_desc.hpp"

namespace spi {

// The kernel's modes: a Prec, or F16X3 whose A (and residual) are activations already stored
// split, [32 hi fp16 | 32 lo fp16] per 32 channels (GemmDesc::a_split; kernel-internal).
// Byte-for-byte the same addressing as fp32 A (a 32-k block is 128 bytes either way), so only
// the fragment reads differ: A is read exactly like W.
constexpr int kF16X3S = 3;
constexpr bool split_mode(int mode) { return mode == (int)Prec::F16X3 || mode == kF16X3S; }
// Per mode: bytes of each A / W image row per k-step (RB = 256 for F16X3 measured slower: VGPRs,
// LDS), k-values per step, A elements per 16-byte chunk.
//   F16 64 fp16;  F32 32 fp32;  F16X3 A: 32 fp32, W: [32 hi | 32 lo] fp16;  kF16X3S A like W
constexpr int rb_of(int /*mode*/) { return 128; }
constexpr int estep_of(int mode) { return mode == (int)Prec::F16 ? 64 : 32; }
constexpr int epc_of(int mode) { return mode == (int)Prec::F16 ? 8 : 4; }

// A-operand kinds: dense rows; conv with one (kh, kw) tap per k-step (Cin >= the
// k-step: scalar tap walk + per-row tap mask); conv in general (per-chunk taps:
// the stem); 3x3/s1/p1 conv from an LDS-resident input band (kConvHalo, below).
// Separate instantiations keep each kind's loop free of the others.
enum : int { kDense = 0, kConvTap = 1, kConvGen = 2, kConvHalo = 3, kConvHaloS = 4, kConvTapW = 5 };

// Split-K is compiled into the 64x64 and 128x64 tiles and the halo kinds (no plan
// rule splits 128x128; the reducer costs 36-120 VGPRs there).
constexpr bool split_k_compiled(int bm, int bn, bool halo) {
  return (bm == 64 && bn == 64) || (bm == 128 && bn == 64) || halo;
}
template <int BM, int BN, int KIND>
constexpr bool kSplitK = split_k_compiled(BM, BN, KIND == kConvHalo || KIND == kConvHaloS);

// kConvHalo.  An implicit-GEMM conv stages each (tap, channel block) A tile
// separately: every input pixel crosses the CU nine times, and the vector-memory
// ingest of a CU (~70 GB/s from L2, MI355X_MICROARCH.md "gather into LDS") is
// what bounds these layers (no-DMA diagnostic build: +64 % end to end).  Here a
// tile is a band of whole output rows of one image; per channel block the band's
// input rows plus the 1-pixel border -- (th + 2) x (W + 2) pixels, 128 bytes each,
// swizzled like the ring images -- are DMA'd once into one of two halo buffers,
// and the nine taps read their A fragments from it at a pixel offset of
// kh * (W + 2) + kw.  Only W goes through the per-step ring.  Halo pixels per
// buffer: HQ DMA instructions per wave x NW waves x 8 pixels.
// kConvHaloS: the 64-row kind with 96-pixel buffers (14- and 7-wide layers):
// 48 KiB of LDS instead of 56, three workgroups per CU instead of two.
// NW = 8 (the 256-row kind, 4 x 2 waves): 6 pieces per wave = 384-pixel buffers.
template <int BM, int KIND, int NW>
constexpr int kHaloHQ = KIND == kConvHaloS ? 3 : NW == 8 ? 6 : BM == 64 ? 4 : 8;
template <int BM, int KIND, int NW>
constexpr int kHaloPixels = kHaloHQ<BM, KIND, NW> * NW * 8;
template <int KIND>
constexpr bool kIsHalo = KIND == kConvHalo || KIND == kConvHaloS;
// kConvTapW (round 4): 3x3/s1/p1 tap walk with the three kw taps of a (kh, channel block)
// reading one A window.  For stride 1 and padding 1 (OH = H, OW = W) the input pixel of tap
// (kh, kw) of output row m is the global pixel m + (kh - 1) W + kw - 1, so the 64 rows of a
// tile read, for the three kw taps, the 66 consecutive pixels from m0 + (kh - 1) W - 1 on:
// one DMA'd window of BM + 8 rows (BM / 32 16-byte pieces + one 4-byte piece per wave) feeds
// 3 k-steps -- for 64-row tiles 9 KiB of A per 3 steps instead of 24 (a step's LDS ingest 16 ->
// 11 KiB; 128-row tiles 24 -> 13.7 KiB; the tap walks run at the per-CU ingest ceiling,
// DESIGN.md 3.1.5).
// Taps that fall into the padding read a real neighbour pixel of the window and are zeroed
// at fragment read by the row's tap mask.  Only W goes through the STAGES ring.
template <int BM>
constexpr int kWinRows = BM + 8;
// Dense kinds keep 2 x BM {mean, rstd} pairs past the ring for the LayerNorm fold (the tile's
// row statistics, computed once per row before the epilogue's walk).
template <int BM, int KIND>
constexpr int kLnBytes = KIND == kDense ? 2 * BM * 8 : 0;
// Window kind with NW = 8 (round 5): two K groups of 4 waves in one workgroup, each walking
// half of the slice's super-steps through its own LDS (ring + windows) and reducing through
// LDS at the end -- the intra-workgroup split-K of DESIGN.md 3.1.6.
template <int KIND, int NW>
constexpr int kKGroups = KIND == kConvTapW && NW == 8 ? 2 : 1;
// LDS bytes of one K group (the whole workgroup: kKGroups times this)
template <int BM, int BN, int STAGES, int KIND, int NW>
constexpr int kLdsBytes = kIsHalo<KIND> ? STAGES * BN * 128 + 2 * kHaloHQ<BM, KIND, NW> * NW * 8 * 128 + 16
                          : KIND == kConvTapW ? STAGES * BN * 128 + 2 * kWinRows<BM> * 128 + 16
                                              : STAGES * (BM + BN) * 128 + kLnBytes<BM, KIND> + 16;
// Occupancy asked of the register allocator (the launch bound): 4 / 3 / 2 waves per SIMD by tile
// size per wave (of a K group), capped by what the tile's LDS ring allows (NW / 4 waves
// per SIMD per block, 160 KiB of LDS per CU; RB = 128 bytes per row per stage in every mode).
template <int BM, int BN, int STAGES, int KIND, int NW>
constexpr int kMinWaves = std::max(
    1, std::min(BM * BN * 4 * kKGroups<KIND, NW> / NW <= 64 * 64 ? 4 : BM * BN * 4 * kKGroups<KIND, NW> / NW <= 128 * 64 ? 3 : 2,
                (160 * 1024) / (kKGroups<KIND, NW> * kLdsBytes<BM, BN, STAGES, KIND, NW>) * NW / 4));

// One kernel instance's geometry.  NWA waves per workgroup in KG K groups of NW waves; everything
// else is one group's (its waves, threads, LDS).  The NW waves form an (NW / 2) x 2 grid over the
// tile: wave (wm, wn) owns rows [wm * WTM, ...) x columns [wn * WTN, ...), TI x TJ 16 x 16 fragments.
template <int MODE, int BM_, int BN_, int STAGES_, int KIND, int NWA>
struct TileGeo {
  static constexpr int BM = BM_, BN = BN_, STAGES = STAGES_;
  static constexpr bool CONV = KIND != kDense;
  static constexpr bool TAP = KIND == kConvTap;
  static constexpr bool GEN = KIND == kConvGen;
  static constexpr bool HALO = kIsHalo<KIND>;
  static constexpr bool WIN = KIND == kConvTapW;
  static constexpr bool AR = !HALO && !WIN;  // A tiles go through the ring
  static_assert(!WIN || ((BM == 64 || BM == 128) && BN == 64 && STAGES == 3), "window kind: 64 / 128 x 64 tiles, 3 W stages");
  static_assert(NWA == 4 || NWA == 8, "4- or 8-wave workgroups");
  static constexpr int KG = kKGroups<KIND, NWA>;
  static constexpr int NW = NWA / KG;
  static_assert(NW == 4 || NW == 8, "waves per K group");
  static constexpr int NT = 64 * NW;  // threads per K group
  static constexpr int ESTEP = estep_of(MODE), EPC = epc_of(MODE), RB = rb_of(MODE);
  static constexpr int CPR = RB / 16;                  // chunks per image row
  static constexpr int RPI = 64 / CPR;                 // image rows per 1-KiB DMA instruction
  static constexpr int IMG = (AR ? BM + BN : BN) * RB;  // bytes per ring stage (halo, window: W only)
  static constexpr int AQ = BM / RPI / NW, BQ = BN / RPI / NW;  // DMA instructions per wave per step
  static_assert(!AR || AQ * RPI * NW == BM, "A image rows per wave");
  static_assert(BQ * RPI * NW == BN, "W image rows per wave");
  static constexpr int QPS = (AR ? AQ : 0) + BQ;
  static constexpr int HQ = HALO ? kHaloHQ<BM, KIND, NW> : 1;  // halo DMA instructions per wave per block
  static constexpr int HBUF = HALO ? HQ * NW * RPI * RB : WIN ? kWinRows<BM> * RB : 0;  // bytes per halo / window buffer
  static constexpr int XQ = BM / 32 + 1;  // window kind: DMA pieces per wave per window
  static constexpr int LDSB = kLdsBytes<BM, BN, STAGES, KIND, NW>;
  static_assert(LDSB == STAGES * IMG + 2 * HBUF + kLnBytes<BM, KIND> + 16, "LDS layout");
  static_assert(!WIN || RB == 128, "window rows are 128-byte pixel blocks");
  static_assert(!HALO || (STAGES >= 3 && STAGES <= 6 && RPI == 8), "halo: 9 taps, the next halo at tap 10 - STAGES");
  static constexpr int WTM = BM / (NW / 2), WTN = BN / 2;  // rows, columns per wave
  static constexpr int TI = WTM / 16, TJ = WTN / 16;
  static_assert(BM * BN * 4 <= LDSB - 16, "the epilogue's fp32 C tile must fit the LDS");
  // a pooled problem (GemmDesc::pool_rows) may run on any dense tile SPI_GEMM_PLAN can force: each must
  // hold the pooled epilogue's 256 partial sums behind the C tile, or its [B pool_rows][N] rows would take
  // the ordinary store path into a [B][N] buffer
  static_assert(KIND != kDense || BM * BN * 4 + 256 * 4 <= LDSB - 16, "every dense tile compiles the pooled epilogue");
  // the residual tile prefetch (gemm_epilogue.hpp): 64 x 64 tiles on the vector epilogue path
  static constexpr bool RPF = BM == 64 && BN == 64 && !HALO && NW == 4;
  // the LayerNorm fold lives in the dense fp16 instances only (the transformer GEMMs)
  static constexpr bool LNF = KIND == kDense && MODE == (int)Prec::F16;
};

}  // namespace spi
