// Kernel arguments of the general GEMM kernel (gemm.hip) and the decode every workgroup runs on
// them: which tile and split-K slice it owns.  Plain C++17, no HIP header: gemm_args.cpp fills
// the arguments and validates a desc on the host, the kernels decode with the same functions, and
// tests/test_gemm_args.py walks a launch's workgroups through them without a GPU.
#pragma once
#include "gemm_desc.hpp"
#include "gemm_plan.hpp"

// The Makefile compiles every source as HIP, and there the decode is host and device code; a plain
// C++ compiler sees plain inline functions.  (__host__ / __device__ come with the language mode,
// not with a header.)
#ifdef __HIP__
#define SPI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SPI_HD inline
#endif

namespace spi {

// n / d for 0 <= n < 2^31 by one high multiply (host-computed magic, Granlund-Montgomery
// round-up form: 2^s < d <= 2^(s+1), magic = ceil(2^(32+s) / d) < 2^32, exact since the
// magic's error (< d) times n stays below 2^(32+s)); d = 1 is magic 0.  The prologue of a
// launch divides a dozen times (tile decode, output row -> image / row / column), and the
// compiler's generic 32-bit division is ~40 instructions of dependent SALU / VALU each.
struct FastDiv {
  unsigned magic;
  int shift;
};
inline FastDiv make_fastdiv(unsigned d) {
  if (d <= 1) return FastDiv{0u, 0};
  int s = 0;
  while ((2ull << s) < d) ++s;  // 2^s < d <= 2^(s+1)
  return FastDiv{(unsigned)(((1ull << (32 + s)) + d - 1) / d), s};
}
// the 64-bit product's high word: one v_mul_hi_u32 / s_mul_hi_u32 on the device, as __umulhi
SPI_HD int fdiv(int n, FastDiv f) {
  return f.magic ? (int)((unsigned)(((unsigned long long)(unsigned)n * f.magic) >> 32) >> f.shift) : n;
}

struct KArgs {
  GemmDesc d;
  GemmPtrs p;
  int k_per_split;  // elements, multiple of the k-step
  int tiles_m, tiles_n;
  int tiles;
  int cin_shift;
  int kw_mul;       // ceil(65536 / KW): cell / KW == (cell * kw_mul) >> 16 for cell < 2^12
  int cell_uniform; // conv with Cin >= k-step: one (kh, kw) cell per step
  int vec_ok;       // C / residual rows allow 16-byte vectors of 8 elements (epilogue)
  int xg_m, xg_n;   // XCD rectangles: tile rows in xg_m groups x tile columns in xg_n groups
  // the rectangles' first tile row per row group (rg_m0[xg_m] = tiles_m) and first tile
  // column per column group (cg_n0[xg_n] = tile columns), and the row-group heights as
  // FastDivs: the decode is compares and high multiplies, no loop, no division
  int rg_m0[9], cg_n0[9];
  FastDiv fd_rows[8];
  FastDiv fd_split;      // / splits
  FastDiv fd_ohw, fd_ow;  // conv: output row m -> image, then row / column
  FastDiv fd_tiles;       // grouped launches: / tiles
  FastDiv fd_period, fd_hwp;  // halo kinds: / h_period, / h_hwp
  int imgs;                   // conv: images (M / (OH * OW))
  // halo conv (kConvHalo): tile row block tm is the band of h_th "virtual" output
  // rows u in [tm * h_th, (tm + 1) * h_th) x the full width.  Virtual rows stack the
  // images with a period of h_period rows: image u / h_period, output row
  // u % h_period - h_off (valid when in [0, OH)).  Aligned bands (h_off 0,
  // h_period = bands per image x h_th) stay inside one image; stacked bands
  // (h_off 1, h_period = OH + 2: a zero row above and below every image) may span
  // several images, so one tile can cover whole small maps of several images and
  // the weights are re-read by fewer tiles.  The band's input rows (+1 pixel of
  // padding around) form an h_hwp-wide halo image of h_hp pixels; h_nblk channel
  // blocks, h_bps of them per split-K slice
  int h_th, h_period, h_off, h_hwp, h_hp, h_nblk, h_bps;
  int win_nblk_shift;  // window kind (kConvTapW): log2 of the channel blocks per tap
  int splits;  // split-K slices (the grid holds tiles x splits workgroups of this problem)
#ifdef SPI_GEMM_TIMELINE
  int tl;  // stamp this launch (tools/gemm_timeline.py; set in gemm.hip)
#endif
};

// One launch, one or two independent problems of the same kernel instance (a
// grouped launch: ResNet's downsample 1x1 conv beside its block's first conv,
// both reading the block input).  Workgroups [0, wgs0) run a[0], the rest a[1].
struct KGroup {
  KArgs a[2];
  int wgs0;
};

// The kernel's modes (gemm_tile.hpp): a Prec, or kF16X3S for F16X3 with split activations.
constexpr Prec prec_of_mode(int mode) { return mode == kF16X3S ? Prec::F16X3 : (Prec)mode; }
constexpr int mode_of(Prec prec, bool a_split) { return prec == Prec::F16X3 && a_split ? kF16X3S : (int)prec; }

// XCD-aware order.  The hardware deals dispatch indices round-robin to the 8 XCDs, so idx & 7
// names the XCD: number each XCD's workgroups consecutively (bijective, chunks of q or q + 1).
SPI_HD int xcd_order(int idx, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = idx & 7, l = idx >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + l;
}

struct TileAt {
  int tile, tm, tn, kslice;
};
// The tile and slice of one workgroup of problem `a`: linear tile `lin` and slice `kslice_in` as
// the grid numbers them, hl the workgroup's dispatch index inside this problem's range;
// split_compiled: the instance has the split-K reducer (split_k_compiled).
SPI_HD TileAt decode_tile(const KArgs& a, const bool split_compiled, const int lin, const int kslice_in, const int hl) {
  // XCD-aware remap: consecutive tiles (same weight columns) land on one XCD's L2.
  int tile = lin, kslice = kslice_in;
  if (split_compiled && a.splits > 1) {
    // split-K: cut that order into tiles of `splits` consecutive slices
    const int wgid = xcd_order(hl, a.tiles * a.splits);
    tile = fdiv(wgid, a.fd_split);
    kslice = wgid - tile * a.splits;
  } else if (a.tiles >= 16) {
    tile = xcd_order(tile, a.tiles);
  }
  // Tile of linear index `tile`: the tile grid is cut into xg_m x xg_n
  // rectangles (row groups i-major), each walked with tm fastest; the chunk of
  // consecutive indices an XCD receives is then (about) one rectangle, so each
  // A row block is fetched by xg_n XCD L2s and each W column block by xg_m
  // (xg_m = 1: every XCD reads all of A -- the plain column-major order).
  const int TN = a.tiles_n;
  int mlo = 0, mhi = a.rg_m0[1];
  FastDiv fdm = a.fd_rows[0];
#pragma unroll
  for (int i = 1; i < 8; ++i)  // row group: the last whose first tile index is <= tile
    if (i < a.xg_m && a.rg_m0[i] * TN <= tile) {
      mlo = a.rg_m0[i];
      mhi = a.rg_m0[i + 1];
      fdm = a.fd_rows[i];
    }
  const int mi = mhi - mlo;
  const int l2 = tile - mlo * TN;  // index inside row group i: mi x TN tiles
  const int c = fdiv(l2, fdm);     // which tile column it falls in
  int nlo = 0;
#pragma unroll
  for (int j = 1; j < 8; ++j)
    if (j < a.xg_n && a.cg_n0[j] <= c) nlo = a.cg_n0[j];
  const int loc = l2 - mi * nlo;
  const int lq = fdiv(loc, fdm);
  return TileAt{tile, mlo + (loc - lq * mi), nlo + lq, kslice};
}

// A grouped launch's 1-D grid is problem-major, then slice, then tile.  Workgroup wg runs
// problem pair_problem(g, wg); index l inside that problem's range is slice pair_slice(a, l).kslice,
// linear tile .lin.  Two steps, so that a kernel takes each problem's KArgs at constant offsets.
SPI_HD int pair_problem(const KGroup& g, int wg) { return wg >= g.wgs0; }
struct PairAt {
  int kslice, lin;
};
SPI_HD PairAt pair_slice(const KArgs& a, int l) {
  const int kslice = fdiv(l, a.fd_tiles);
  return PairAt{kslice, l - kslice * a.tiles};
}

// Kernel arguments of one problem under its plan (mode: a Prec or kF16X3S).
KArgs make_args(int mode, const GemmDesc& d, const GemmPtrs& p, const Plan& pl);
// Both problems of a grouped launch (pp.grouped): problem 1's split-K slabs and tickets follow
// problem 0's in p0's workspace.
KGroup make_group(int mode, const GemmDesc& d0, const GemmPtrs& p0, const GemmDesc& d1, const GemmPtrs& p1,
                  const PairPlan& pp);
// Throws std::invalid_argument for a desc no kernel runs: the krep, pooled-GEMM and split
// activation rules, and what the LayerNorm fold and the two-plane stream ask of the operands.
void validate_gemm(const GemmDesc& d, const GemmPtrs& p, Prec prec);

}  // namespace spi
