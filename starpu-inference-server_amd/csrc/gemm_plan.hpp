// Host-side GEMM planner: which kernel instance runs a GemmDesc, with which tile, ring depth
// and split-K, and the workspace that takes.  Plain C++17 -- no HIP, no kernels, no pointers --
// so a rule change rebuilds in seconds and tests/test_gemm_plan.py checks the rules without a
// GPU.  gemm.hip / gemm256.hip fill kernel arguments from these plans and launch.
#pragma once
#include <cstddef>

#include "gemm_desc.hpp"
#include "gemm_tile.hpp"

namespace spi {

// Kernel constants the planner sizes by, from the kernel's own geometry (gemm_tile.hpp).
// k-values per staged step:
constexpr int estep_of(Prec prec) { return estep_of((int)prec); }
// halo buffer capacity in pixels of the 64-row kinds (kConvHaloS, kConvHalo), the 128-row kind and
// the 8-wave 256-row kind:
constexpr int kHaloPixelsSmall = kHaloPixels<64, kConvHaloS, 4>, kHaloPixels64 = kHaloPixels<64, kConvHalo, 4>,
              kHaloPixels128 = kHaloPixels<128, kConvHalo, 4>, kHaloPixels256 = kHaloPixels<256, kConvHalo, 8>;
// gemm256 split-K: at most this many slices (its reduction holds one accumulator set per slice)
constexpr int kG256MaxSplits = 4;
// gemm256's LayerNorm consumer fold (ln_load / ln_combine) reads the chunk statistics in pairs,
// four per lane group: none, or an even count in 2..16 (D = 768: 12, D = 1024: 16)
constexpr bool gemm256_ln_chunks_ok(int chunks) { return chunks == 0 || (chunks >= 2 && chunks <= 16 && chunks % 2 == 0); }

// The general kernel's plan for one problem.
struct Plan {
  int bm, bn, stages, splits, k_per_split;
  // kConvHalo: waves per workgroup, virtual output rows per band, the virtual-row
  // period (rows per image) and offset (KArgs::h_off), band count, channel blocks
  // per slice
  int halo = 0, nw = 4, th = 0, period = 0, off = 0, tiles_m = 0, bps = 0;
  int win = 0;  // kConvTapW (64 x 64, 3 W stages; slices of whole 3-step super-steps)
};

// Everything the launch and the workspace sizing need to know about one problem.
struct GemmPlan {
  Plan pl;  // the general kernel's plan
  // gemm256 routing by desc (gemm() also needs 16-byte aligned A / W): tile height (0: the general
  // kernel), split-K slices, k-tile buffers of the 128-row tile, tile order (1: column tiles fastest)
  int g256_bm = 0, g256_splits = 1, g256_nbuf = 2, g256_order = 0;
  // split-K workspace: the larger of the two routes (0 when not split)
  size_t partial_floats = 0, counter_slots = 0;
};
GemmPlan plan_gemm(const GemmDesc& d, Prec prec);

// Two conv problems on one input (gemm_pair).
struct PairPlan {
  Plan q0, q1;       // the plans that launch: joint when grouped, else each problem's own
  bool grouped;      // one launch (the plans share a kernel instance)
  int wgs0, wgs;     // problem 0's workgroups, both problems'
  size_t slab_off, ticket_off;  // problem 1's offsets into the split-K slabs / tickets (grouped only)
  // what a caller sizes the workspace for: the two problems' own plans, summed (each joint rule
  // only shrinks problem 0's split, so the joint plans fit in it)
  size_t partial_floats, counter_slots;
};
PairPlan plan_pair(const GemmDesc& d0, const GemmDesc& d1, Prec prec);

// Tiles of a problem under a plan; the XCD rectangles of its tile decode; whether every k-step
// of a conv lies in one (kh, kw) tap (the tap-walk kinds).
int plan_tiles(const GemmDesc& d, const Plan& pl);
void xcd_groups(const GemmDesc& d, Prec prec, int TM, int TN, int& gm, int& gn);
bool cell_uniform(const GemmDesc& d, Prec prec);

// gemm256 (gemm256.hip) routing predicates: eligible when N % 256 == 0, K % 64 == 0 and at least
// min_tiles tiles of bm x 256.
bool gemm256_eligible(const GemmDesc& d, Prec prec, int min_tiles, int bm = 256);
// Split-K slices for a gemm256 problem: 1 with >= target tiles, else enough slices of >= 16
// k-tiles (at most 4, at most max_split when > 0) to reach ~target workgroups (ViT-L's
// N = 1024 GEMMs: 52 tiles -> FFN2 3 slices, out-proj none).
int gemm256_splits(const GemmDesc& d, int target, int max_split, int bm = 256);

// Workspace needed by a GEMM with the chosen split-K (0 when not split).
size_t gemm_partial_floats(const GemmDesc& d, Prec prec);
size_t gemm_counter_slots(const GemmDesc& d, Prec prec);
// Whether a workspace of `floats` slab floats and `slots` tickets holds the problem -- or, with
// d1, the two problems of a gemm_pair.
bool gemm_workspace_fits(const GemmDesc& d, Prec prec, size_t floats, size_t slots, const GemmDesc* d1 = nullptr);
// k-values per staged step (W rows must be padded to a multiple of it).
int gemm_kstep(Prec prec);

// A plan as the 8 integers the debug exports and spi_op_conv_pair report: bm, bn, stages, splits,
// halo kind, window kind, waves, k per slice.
template <class T>
void put_plan(const Plan& pl, T* out) {
  const int v[8] = {pl.bm, pl.bn, pl.stages, pl.splits, pl.halo, pl.win, pl.nw, pl.k_per_split};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
}

// The problems the debug exports (gemm_plan.cpp, gemm_args.cpp) are asked about.  precision as
// spi_ops.h (3 = split activations); flags: bit 0 an activation, 1 res_f32, 2 res_planes,
// 3 out_planes, 4 out_f16, 5 out_f32, bits 8..15 ln_in_chunks, 16..23 res_ln_chunks.
Prec case_prec(int precision);
GemmDesc case_conv_desc(int precision, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
GemmDesc case_dense_desc(int precision, int M, int N, int K, int lda, int krep, int pool_rows, unsigned flags);

}  // namespace spi
