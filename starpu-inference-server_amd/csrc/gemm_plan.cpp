// The GEMM planner (gemm_plan.hpp): every rule that decides which kernel instance runs a
// problem, and the knobs that steer it.  Host only.
#include "gemm_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace spi {

// the other kernel files' knob readers (spi_kernels.hpp, which needs HIP)
void conv_wres_reload_env();
void attention_reload_env();
void qkv_attn_reload_env();

namespace {

// Tuning knobs, read once (getenv on every launch cost ~0.5 us each);
// spi_debug_gemm_reload_env() re-reads them for in-process sweeps and tests.  Variants measured and rejected
// in rounds 1-3 (latency plan rule, 128x64 split-K, 256x128 tiles, 3-stage
// 128x128 rings, 4-stage halo rings, XCD-local split-K, per-knob ring depths,
// DESIGN.md 6) are gone; what remains:
//   SPI_GEMM_PLAN="bm,bn,stages,splits"  force one plan for every GEMM (sweeps)
//   SPI_GEMM_MAXSPLIT=S                  cap split-K (default 8; 1: none, 0: uncapped)
//   SPI_GEMM_HALO_CFG                    halo candidates: "0" off, "rows,a|s" forced,
//                                        "OW:rows,a|s;..." per map width
//   SPI_GEMM_WIN=0|1|2|3                 the kw-window tap walk of 3x3/s1 convs (below)
//   SPI_GEMM_256_MIN / SPI_GEMM_256_LONGK / SPI_GEMM_256_ORDER  gemm256 routing (below)
struct Knobs {
  bool forced = false;
  Plan plan{};
  int target = 128;  // round 3 (with the joint pair plan): ResNet-18 fp16m +2 % over 192, BERT / ResNet-152 +-0
  // split-K cap: ResNet-18 bs1 (layer 4: 12 slices, layer 3: 4) +1.8 % at 8 or 6 over uncapped,
  // bs8 +-0.5 % (no conv splits past 6 there); round 6, profiles/r06/maxsplit/
  int max_split = 8;
  int halo = 1;  // 3x3/s1 convs from LDS-resident input bands (kConvHalo)
  // SPI_GEMM_WIN=0: 3x3/s1 tap walks without the kw window (kConvTapW); 2 / 3: 64 x 64 window
  // tiles as two K groups of 4 waves (8-wave workgroups), at the 4-wave plan's slices / half of them
  int win = 1;
  int g256_min = 128;      // SPI_GEMM_256_MIN="T256[,T128]": dense F16 GEMMs with >= T256 tiles of 256^2 -> gemm256 (0 = off)
  // ... else with >= T128 tiles of 128 x 256 -> gemm256's 128-row tile (round 5; 0 = off)
  // round 6: 64 tiles, two buffers -- BERT-base's FFN1 (96 tiles of 128 x 256, K = 768) four-stream
  // +1.5 % (24.25k -> 24.60k, profiles/r06/sweeps/); the long-K rule below keeps ViT-L's N = 1024
  // GEMMs on 256^2 tiles (128 x 256 there: -3 % with three buffers, -7 % with two).  Rounds 3-5
  // had it off (BERT -7 % with the three-buffer schedule, which also raced)
  int g128_min = 64;
  int g128_nbuf = 2;  // third field: k-tile buffers of the 128-row tile (2: 96 KiB, 3: 144 KiB)
  // SPI_GEMM_256_LONGK="tiles,K": also with >= `tiles` tiles when K >= `K` (round 3: 48,1024 -- ViT-L FFN2 /
  // out-proj, 52 tiles: one 256^2 workgroup per CU-time unit does ~1.7x the work of the 128x128 kernel, so
  // under four streams ViT-L goes 6.07k -> 6.70k inf/s though the launch alone is slower; BERT's K = 768
  // GEMMs stay off: -1.3 % with them)
  int g256_longk_tiles = 48, g256_longk_k = 1024;
  // SPI_GEMM_256_LONGK="tiles,K,S": gemm256 split-K up to S slices for grids under T tiles (default
  // 1: none -- round 4 measured ViT-L FFN2 at 3 slices 100 -> 73 us back to back but C5 under the
  // four streams 6.05k -> 5.09k inf/s: the slices' CU-time and slab traffic cost the other streams more)
  int g256_split = 1;
  // SPI_GEMM_256_ORDER: gemm256 tile order, 0 row blocks fastest, 1 column tiles fastest, -1 (default)
  // by shape: column tiles fastest when A is the larger operand (M > N), so an XCD's consecutive
  // workgroups share A row blocks (round 6, PMC FETCH_SIZE: ViT-L FFN2 142 -> 119 MB, out-proj
  // 47.7 -> 41.9 MB; FFN1 (N = 4096) 61 -> 78 MB the other way; C5 four-stream +0.2 %)
  int g256_order = -1;
  int halo_bm = 0;          // SPI_GEMM_HALO_CFG="rows,a|s": force a halo candidate (64 / 128 / 256 rows)
  bool halo_stacked = false;
  struct HaloPick {
    int ow, bm;
    bool stacked;
  };
  HaloPick halo_map[8] = {};  // SPI_GEMM_HALO_CFG="OW:rows,a|s;...": per map width
  int n_halo_map = 0;
};
// Fixed plan constants (each measured in rounds 1-3):
constexpr int kHaloStages = 3;     // W ring of the halo kinds
constexpr int kHaloMinH = 14;      // 7x7 maps: the implicit GEMM measured faster (77 % row use)
constexpr int kHaloMaxTiles = 64;  // halo only when the implicit GEMM has fewer 64x64 tiles
// Ring depth by k-steps per slice (variant builds: tools/build_variant.sh ... -DSPI_ST3_MIN=N /
// -DSPI_ST4_MIN=N).  Round 6: 3 stages from 12 k-steps, no 4-stage ring -- BERT-base's out-proj (12
// k-steps, was 2 stages) and FFN2 (48, was 4: +2.4 % in round 3) then share one kernel instance:
// C3 +1.2 %, each change alone +0.2 %; C2 / C4 +-0.3 % (profiles/r06/ring_depth/)
#ifndef SPI_ST3_MIN
#define SPI_ST3_MIN 12
#endif
#ifndef SPI_ST4_MIN
#define SPI_ST4_MIN (1 << 30)
#endif
constexpr int kSt3Min = SPI_ST3_MIN, kSt4Min = SPI_ST4_MIN;

Knobs read_knobs() {
  Knobs k;
  if (const char* e = std::getenv("SPI_GEMM_PLAN"); e && *e) {
    int bm = 0, bn = 0, st = 0, sp = 0;
    if (std::sscanf(e, "%d,%d,%d,%d", &bm, &bn, &st, &sp) == 4) {
      const bool ok_tile = (bm == 128 && bn == 128) || (bm == 128 && bn == 64) || (bm == 64 && bn == 64);
      const bool ok_st = st >= 2 && st <= 4 && !(bm == 128 && bn == 128 && st > 2) && !(bm == 128 && bn == 64 && st > 3);
      if (ok_tile && ok_st && sp >= 1) {
        k.forced = true;
        k.plan = Plan{bm, bn, st, sp, 0};
      }
    }
  }
  if (const char* e = std::getenv("SPI_GEMM_256_MIN"); e && *e) {
    int a = 0, b = 0, c = 3;
    const int n = std::sscanf(e, "%d,%d,%d", &a, &b, &c);
    k.g256_min = a;
    if (n >= 2) k.g128_min = b;
    if (n >= 3) k.g128_nbuf = c == 2 ? 2 : 3;
  }
  if (const char* e = std::getenv("SPI_GEMM_256_LONGK"); e && *e) {
    int t = 0, kk = 0, sp = 1;
    if (std::sscanf(e, "%d,%d,%d", &t, &kk, &sp) >= 2) {
      k.g256_longk_tiles = t;
      k.g256_longk_k = kk;
      k.g256_split = std::max(1, sp);
    } else {
      k.g256_longk_tiles = 0;  // e.g. "0": off
    }
  }
  if (const char* e = std::getenv("SPI_GEMM_HALO_CFG"); e && *e) {
    // "0": no halo kinds; "rows,a|s" for every halo conv, or per map width
    // "OW:rows,a|s;OW:rows,a|s;..." (OW 0 = any other width; rows 0 = not a halo conv)
    if (std::strcmp(e, "0") == 0) {
      k.halo = 0;
    } else if (std::strchr(e, ':')) {
      for (const char* q = e; q && *q;) {
        int ow = 0, bm = 0;
        char mode = 'a';
        if (std::sscanf(q, "%d:%d,%c", &ow, &bm, &mode) >= 2 && k.n_halo_map < 8)
          k.halo_map[k.n_halo_map++] = {ow, bm, mode == 's'};
        q = std::strchr(q, ';');
        if (q) ++q;
      }
    } else {
      int bm = 0;
      char mode = 'a';
      if (std::sscanf(e, "%d,%c", &bm, &mode) >= 1 && (bm == 64 || bm == 128 || bm == 256)) {
        k.halo_bm = bm;
        k.halo_stacked = mode == 's';
      }
    }
  }
  if (const char* e = std::getenv("SPI_GEMM_256_ORDER"); e && *e) k.g256_order = std::max(-1, std::min(1, std::atoi(e)));
  if (const char* e = std::getenv("SPI_GEMM_MAXSPLIT"); e && *e) k.max_split = std::max(0, std::atoi(e));  // 0: uncapped
  if (const char* e = std::getenv("SPI_GEMM_WIN"); e && *e) k.win = std::max(0, std::min(3, std::atoi(e)));
  return k;
}

Knobs& knobs() {
  static Knobs k = read_knobs();
  return k;
}

// gemm256 routing by desc (gemm() also needs 16-byte aligned A / W): the tile height it runs
// at, 0 = the general kernel.  256^2 tiles for grids of >= T256 of them, or of >= the long-K
// rule's tiles when K is long (ViT-L's N = 1024 GEMMs at bs16: 52 tiles); else 128 x 256 tiles
// for grids of >= T128 of those (BERT-base's FFN1 at bs8: 96).
int route_bm(const GemmDesc& d, Prec prec) {
  const Knobs& k = knobs();
  if (prec != Prec::F16) return 0;
  if (gemm256_eligible(d, prec, k.g256_min)) return 256;
  if (k.g256_longk_tiles > 0 && d.K >= k.g256_longk_k && gemm256_eligible(d, prec, k.g256_longk_tiles)) return 256;
  if (gemm256_eligible(d, prec, k.g128_min, 128)) return 128;
  return 0;
}
int g256_splits(const GemmDesc& d, int bm) {
  const Knobs& k = knobs();
  const int cap = k.max_split > 0 ? std::min(k.max_split, k.g256_split) : k.g256_split;
  return cap > 1 ? gemm256_splits(d, k.target, cap, bm) : 1;
}

Plan finish_plan(Plan pl, int ksteps, int ES, int krep = 1) {
  const Knobs& k = knobs();
  if (k.max_split) pl.splits = std::min(pl.splits, k.max_split);
  if (pl.bn != 64 || (pl.bm != 64 && pl.bm != 128)) pl.splits = 1;  // split-K exists in the 64- and 128-row x 64 kernels only
  if (pl.bm == 128) pl.stages = pl.bn == 128 ? 2 : std::min(pl.stages, 3);  // the instantiated rings
  pl.splits = std::max(1, std::min(pl.splits, ksteps));
  int kt = (ksteps + pl.splits - 1) / pl.splits;
  kt = (kt + krep - 1) / krep * krep;  // krep: slices hold whole (hi, lo) step pairs
  pl.k_per_split = kt * ES;
  pl.splits = (ksteps + kt - 1) / kt;
  return pl;
}

// kConvHalo plan for 3x3/s1/p1 convs with whole channel blocks (split activations
// in F16X3).  Candidates (all 64 columns wide):
//   64 rows, 4 waves (kConvHaloS when the halo fits 96 pixels, else 128-pixel buffers)
//   128 rows, 4 waves (256-pixel buffers); 256 rows, 8 waves (384-pixel buffers)
// each with aligned bands (whole output rows of one image) or stacked bands
// (virtual rows spanning images, for maps too small to fill a tile).  th = as many
// (virtual) rows per band as fit the tile and the halo buffer; split-K over
// channel blocks up to ~T workgroups.  The default picks aligned 128 rows for maps
// wider than 32 pixels, else aligned 64 (the round-1 rule) -- SPI_GEMM_HALO_CFG =
// "rows,a|s" forces a candidate (tools/gemm_bench.py sweeps).  halo = 0 when the
// conv is not eligible.
Plan halo_candidate(const GemmDesc& d, Prec prec, int T, int bm, bool stacked, int smax) {
  Plan no{};
  const int ES = estep_of(prec);
  const int nw = bm == 256 ? 8 : 4;
  const int cap = bm == 256 ? kHaloPixels256 : bm == 128 ? kHaloPixels128 : kHaloPixels64;
  const int imgs = d.M / (d.OH * d.OW);
  int th = stacked ? bm / d.OW : std::min(bm / d.OW, d.OH);
  while (th > 0 && (th + 2) * (d.W + 2) > cap) --th;
  if (th == 0) return no;
  const bool small = bm == 64 && (th + 2) * (d.W + 2) <= kHaloPixelsSmall;  // kConvHaloS
  const int nblk = d.Cin / ES;
  Plan h{bm, 64, kHaloStages, 1, 0};
  h.nw = nw;
  h.th = th;
  if (stacked) {
    h.off = 1;
    h.period = d.OH + 2;
    h.tiles_m = (imgs * h.period + th - 1) / th;
  } else {
    const int nb = (d.OH + th - 1) / th;
    h.off = 0;
    h.period = nb * th;
    h.tiles_m = imgs * nb;
  }
  const int tiles = h.tiles_m * (d.N / 64);
  int sp = 1;
  if (tiles < T) sp = std::min({(T + tiles - 1) / tiles, nblk, smax});
  if (knobs().max_split) sp = std::min(sp, knobs().max_split);
  const int bps = (nblk + sp - 1) / sp;
  h.splits = (nblk + bps - 1) / bps;
  h.halo = small ? 2 : 1;
  h.bps = bps;
  return h;
}

// kConvTapW: 3x3 / stride 1 / padding 1 convs with OH = H, OW = W (a tap's input pixel is
// the output pixel shifted by a constant), whole channel blocks, no Kpad tail, and A in
// 128-byte pixel blocks read as they are (fp16, split fp16x3).
bool window_ok(const GemmDesc& d, Prec prec) {
  const int ES = estep_of(prec);
  return knobs().win && d.conv && !d.pool_rows && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 &&
         d.OH == d.H && d.OW == d.W && d.krep == 1 && d.Cin >= ES && d.Cin % ES == 0 && d.Kpad == d.K &&
         (prec == Prec::F16 || (prec == Prec::F16X3 && d.a_split));
}

Plan halo_plan(const GemmDesc& d, Prec prec, int T) {
  Plan no{};
  const int ES = estep_of(prec);
  if (!knobs().halo || knobs().forced || d.krep != 1 || !d.conv || d.KH != 3 || d.KW != 3 || d.stride != 1 || d.pad != 1 ||
      d.Cin < ES || d.Cin % ES || (prec == Prec::F16X3 && !d.a_split) || d.N % 64 || d.OH != d.H || d.OW != d.W)
    return no;
  if (knobs().halo_bm) return halo_candidate(d, prec, T, knobs().halo_bm, knobs().halo_stacked, 1 << 20);
  for (int i = 0; i < knobs().n_halo_map; ++i) {
    const auto& hm = knobs().halo_map[i];
    if (hm.ow == d.OW || hm.ow == 0) {
      if (hm.bm != 64 && hm.bm != 128 && hm.bm != 256) return no;
      return halo_candidate(d, prec, T, hm.bm, hm.stacked, 1 << 20);
    }
  }
  if (d.OH < kHaloMinH) return no;
  // Under the serving load (four worker streams) the implicit GEMM's many small,
  // LDS-light workgroups keep more kernels co-resident than the halo kinds'
  // 56-90 KiB ones: ResNet-18 bs8 59.3k vs 57.0k inf/s, ResNet-152 bs32 10.7k vs
  // 10.0k (tools/policy_sweep.py).  The halo kinds pay where the grid
  // is small and one forward's latency dominates (ResNet-18 bs1: 13.2k vs 12.1k).
  const auto ceil_div = [](int x, int y) { return (x + y - 1) / y; };
  if (ceil_div(d.M, 64) * ceil_div(d.N, 64) >= kHaloMaxTiles) return no;
  const int bm = d.OW > 32 ? 128 : 64;
  return halo_candidate(d, prec, T, bm, false, bm == 64 ? 1 << 20 : 1);  // round 1: only 64-row tiles split
}

}  // namespace

constexpr int kMinSliceKt = 16;   // k-tiles per slice at least (ViT-L out-proj, K = 1024, 2 x 8: 52.9 us b2b vs 40.2 unsplit)

int gemm256_splits(const GemmDesc& d, int target, int max_split, int bm) {
  const int tiles = (d.M + bm - 1) / bm * (d.N / 256), kt = d.K / 64;
  if (tiles >= target || max_split == 1) return 1;
  int s = std::min({(target + tiles - 1) / tiles, kt / kMinSliceKt, kG256MaxSplits});
  if (max_split > 0) s = std::min(s, max_split);
  if (s <= 1) return 1;
  const int ktp = (kt + s - 1) / s;
  return (kt + ktp - 1) / ktp;
}

bool gemm256_eligible(const GemmDesc& d, Prec prec, int min_tiles, int bm) {
  if (min_tiles <= 0 || prec != Prec::F16 || d.conv || d.krep != 1 || d.a_split || d.out_split || d.pool_rows ||
      d.out_f16)
    return false;
  if (d.res_planes != d.out_planes) return false;  // two planes: residual and output together (RES = 3)
  if ((d.res_f32 || d.res_planes) && d.act != Act::None) return false;  // RES >= 2: no activation instances
  if (d.N % 256 || d.K % 64 || d.Kpad != d.K || d.lda % 8 || d.M < 1) return false;
  // no post-LN residual epilogue here (BERT's out-proj / FFN2 under the LayerNorm fold keep the
  // general kernel at every size; gemm256() rejects them)
  if (d.res_ln_chunks > 0) return false;
  // any other chunk count of the consumer fold takes the general kernel, whose ln_row_stats handles it
  if (!gemm256_ln_chunks_ok(d.ln_in_chunks)) return false;
  return (d.M + bm - 1) / bm * (d.N / 256) >= min_tiles;
}

// XCD rectangles (gemm_kernel's tile decode): the row x column group split
// gm x gn (gm * gn = 8, the XCDs) that minimises the bytes the XCDs' L2s fetch,
// A * gn + W * gm (A: the activation bytes a tile row block reads -- the input
// image for convs; W: the packed weights).
void xcd_groups(const GemmDesc& d, Prec prec, int TM, int TN, int& gm, int& gn) {
  gm = 1;
  gn = std::min(8, TN);
  if (TM * TN < 16) return;
  const double ea = prec == Prec::F16 ? 2 : 4, ew = prec == Prec::F16 ? 2 : 4;
  const double A = d.conv ? (double)(d.M / (d.OH * d.OW)) * d.H * d.W * d.Cin * ea : (double)d.M * d.K * ea;
  const double W = (double)d.N * d.Kpad * ew;
  double best = 1e300;
  for (int m = 1; m <= 8; m *= 2) {
    const int n = 8 / m;
    if (m > TM || n > TN) continue;
    const double cost = A * n + W * m;
    if (cost < best) {
      best = cost;
      gm = m;
      gn = n;
    }
  }
}

int plan_tiles(const GemmDesc& d, const Plan& pl) {
  if (pl.halo) return pl.tiles_m * ((d.N + pl.bn - 1) / pl.bn);
  if (d.pool_rows) return d.M / d.pool_rows * ((d.N + pl.bn - 1) / pl.bn);
  return ((d.M + pl.bm - 1) / pl.bm) * ((d.N + pl.bn - 1) / pl.bn);
}

namespace {
// Plan rule: the largest tile that still yields >= T workgroups, split-K only
// when even 64x64 tiles fall short (then to ~T workgroups, >= 6 k-steps per
// slice).  T in 128..192 measured best with 4 concurrent worker streams
// (ResNet-18 bs8 fp16x3 +8 %, ResNet-152 bs32 +8 %, BERT-base +5 %, ViT-L +7 %
// over a single-stream latency rule); 128 since the joint pair
// plan (round 3).
Plan choose_plan(const GemmDesc& d, Prec prec) {
  const Knobs& k = knobs();
  const int ES = estep_of(prec);
  const int ksteps = d.Kpad / ES;
  if (k.forced) return finish_plan(k.plan, ksteps, ES, d.krep);
  const auto tiles_of = [&](int bm, int bn) { return ((d.M + bm - 1) / bm) * ((d.N + bn - 1) / bn); };
  // a deeper ring pays only on long K loops (4 stages only reach the 64x64 tiles, finish_plan caps the others)
  const auto stages_for = [](int kt) { return kt >= kSt4Min ? 4 : kt >= kSt3Min ? 3 : 2; };
#ifndef SPI_FC_SPLITS  // variant builds: split-K slices of the pooled FC (avgpool + FC in one GEMM)
#define SPI_FC_SPLITS 1
#endif
  if (d.pool_rows)  // one image per tile row
    return finish_plan(Plan{64, 64, stages_for((ksteps + SPI_FC_SPLITS - 1) / SPI_FC_SPLITS), SPI_FC_SPLITS, 0}, ksteps,
                       ES, d.krep);
  if (Plan h = halo_plan(d, prec, k.target); h.halo) return h;
  const int T = k.target;
  if (d.N > 64 && tiles_of(128, 128) >= T) return finish_plan(Plan{128, 128, 2, 1, 0}, ksteps, ES, d.krep);
  if (tiles_of(128, 64) >= T) {
    if (window_ok(d, prec)) {
      Plan w = finish_plan(Plan{128, 64, 3, 1, 0}, ksteps, ES, 3);
      w.win = 1;
      return w;
    }
    return finish_plan(Plan{128, 64, stages_for(ksteps), 1, 0}, ksteps, ES, d.krep);
  }
  const int t64 = tiles_of(64, 64);
  const int sp = t64 >= T ? 1 : std::max(1, std::min((T + t64 - 1) / t64, ksteps / 6));
  const Plan pl = finish_plan(Plan{64, 64, stages_for((ksteps + sp - 1) / sp), sp, 0}, ksteps, ES, d.krep);
  if (window_ok(d, prec)) {
    // the kw-window tap walk: slices of whole (kh, channel block) super-steps
    if (k.win >= 2 && ksteps % 6 == 0) {
      // two K groups per workgroup (8 waves): slices of an even number of super-steps,
      // SPI_GEMM_WIN=2 at the 4-wave plan's slice count, 3 at half of it
      const int sp2 = k.win == 3 ? (sp + 1) / 2 : sp;
      Plan w = finish_plan(Plan{64, 64, 3, sp2, 0}, ksteps, ES, 6);
      w.win = 1;
      w.nw = 8;
      return w;
    }
    Plan w = finish_plan(Plan{64, 64, 3, sp, 0}, ksteps, ES, 3);
    w.win = 1;
    return w;
  }
  return pl;
}

}  // namespace

// one (kh, kw) tap per k-step; the per-row tap mask has 32 bits (taps + the Kpad tail step)
bool cell_uniform(const GemmDesc& d, Prec prec) { return d.conv && d.Cin >= estep_of(prec) && d.KH * d.KW <= 31; }

GemmPlan plan_gemm(const GemmDesc& d, Prec prec) {
  GemmPlan g;
  g.pl = choose_plan(d, prec);
  if (g.pl.splits > 1) {  // one arrival ticket per tile
    g.counter_slots = plan_tiles(d, g.pl);
    g.partial_floats = g.counter_slots * g.pl.splits * g.pl.bm * g.pl.bn;
  }
  g.g256_bm = route_bm(d, prec);
  if (const int bm = g.g256_bm) {
    g.g256_splits = g256_splits(d, bm);
    g.g256_nbuf = knobs().g128_nbuf;
    g.g256_order = knobs().g256_order >= 0 ? knobs().g256_order : d.M > d.N;
    if (g.g256_splits > 1) {  // gemm256 split-K: ticket + published-slab count per tile
      const size_t tiles = (size_t)((d.M + bm - 1) / bm) * (d.N / 256);
      g.partial_floats = std::max(g.partial_floats, tiles * g.g256_splits * bm * 256);
      g.counter_slots = std::max(g.counter_slots, 2 * tiles);
    }
  }
  return g;
}

// Two problems in one launch when their plans share a kernel instance (same
// tile, ring depth and A kind, neither a halo plan); otherwise two launches.
PairPlan plan_pair(const GemmDesc& d0, const GemmDesc& d1, Prec pr) {
  const GemmPlan g0 = plan_gemm(d0, pr), g1 = plan_gemm(d1, pr);
  const Plan &s0 = g0.pl, &s1 = g1.pl;
  Plan q0 = s0, q1 = s1;
  if (!q0.halo && !q1.halo && q0.splits > 1 && q0.bm == 64 && q0.bn == 64 &&
      q1.bm == 64 && q1.bn == 64) {
    // Joint plan: the grouped launch is one grid, so problem 1's workgroups count
    // toward the T workgroups problem 0's split-K was sized for -- fewer slices,
    // fewer fp32 slabs through memory.  Problem 1 (the 1x1 downsample, a few
    // k-steps) takes problem 0's ring depth so the two still share a kernel.
    const int ES = estep_of(pr), ksteps = d0.Kpad / ES;
    const int t64 = plan_tiles(d0, q0), w1 = plan_tiles(d1, q1) * q1.splits;
    const int T0 = std::max(1, knobs().target - w1);
    const int sp = std::max(1, std::min({(T0 + t64 - 1) / t64, ksteps / 6, q0.splits}));
    if (sp < q0.splits) {
      const int kt = (ksteps + sp - 1) / sp;
      q0 = finish_plan(Plan{64, 64, kt >= kSt3Min ? 3 : 2, sp, 0}, ksteps, ES, d0.krep);
      if (q1.splits == 1) q1.stages = q0.stages;
    }
  }
  if (!q0.halo && !q1.halo && q0.splits == 1 && q1.splits == 1 && q0.bm == 64 &&
      q0.bn == 64 && q1.bm == 64 && q1.bn == 64) {
    // the largest common tile whose joint grid still reaches T
    // (the layer-2 pair: 98 + 98 tiles of 128 x 64 instead of 196 + 196 of 64 x 64)
    const auto t = [](const GemmDesc& d, int bm, int bn) { return ((d.M + bm - 1) / bm) * ((d.N + bn - 1) / bn); };
    if (t(d0, 128, 64) + t(d1, 128, 64) >= knobs().target) {
      const int ES = estep_of(pr), k0 = d0.Kpad / ES, k1 = d1.Kpad / ES;
      const int st = std::max(k0, k1) >= kSt3Min ? 3 : 2;
      q0 = finish_plan(Plan{128, 64, st, 1, 0}, k0, ES, d0.krep);
      q1 = finish_plan(Plan{128, 64, st, 1, 0}, k1, ES, d1.krep);
    }
  }
  PairPlan pp{};
  pp.grouped = !q0.halo && !q1.halo && !q0.win && !q1.win && q0.bm == q1.bm && q0.bn == q1.bn &&
               q0.stages == q1.stages && q0.nw == 4 && q1.nw == 4 && cell_uniform(d0, pr) && cell_uniform(d1, pr);
  pp.q0 = pp.grouped ? q0 : s0;
  pp.q1 = pp.grouped ? q1 : s1;
  const int tiles0 = plan_tiles(d0, pp.q0);
  if (pp.grouped && q0.splits > 1) {  // keep clear of problem 0's slabs / tickets
    pp.slab_off = (size_t)tiles0 * q0.splits * q0.bm * q0.bn;
    pp.ticket_off = tiles0;
  }
  pp.wgs0 = tiles0 * pp.q0.splits;
  pp.wgs = pp.wgs0 + plan_tiles(d1, pp.q1) * pp.q1.splits;
  pp.partial_floats = g0.partial_floats + g1.partial_floats;
  pp.counter_slots = g0.counter_slots + g1.counter_slots;
  return pp;
}

// Workspace of the general kernel's plan, or of gemm256's when gemm() may route the desc
// there (routing also needs 16-byte aligned A / W, unknown here: the larger of the two).
size_t gemm_partial_floats(const GemmDesc& d, Prec prec) { return plan_gemm(d, prec).partial_floats; }
size_t gemm_counter_slots(const GemmDesc& d, Prec prec) { return plan_gemm(d, prec).counter_slots; }

bool gemm_workspace_fits(const GemmDesc& d, Prec prec, size_t floats, size_t slots, const GemmDesc* d1) {
  if (d1) {
    const PairPlan pp = plan_pair(d, *d1, prec);
    return pp.partial_floats <= floats && pp.counter_slots <= slots;
  }
  const GemmPlan g = plan_gemm(d, prec);
  return g.partial_floats <= floats && g.counter_slots <= slots;
}

int gemm_kstep(Prec prec) { return estep_of(prec); }

extern "C" void spi_debug_gemm_reload_env(void) {
  knobs() = read_knobs();
  conv_wres_reload_env();
  attention_reload_env();
  qkv_attn_reload_env();
}

Prec case_prec(int precision) { return precision == 0 ? Prec::F32 : precision == 1 ? Prec::F16 : Prec::F16X3; }

GemmDesc case_conv_desc(int precision, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
  GemmDesc d = conv_desc(B, H, W, Cin, Cout, KH, KW, stride, pad, 1);
  d.a_split = d.out_split = precision == 3;
  return d;
}

GemmDesc case_dense_desc(int precision, int M, int N, int K, int lda, int krep, int pool_rows, unsigned flags) {
  GemmDesc d = dense_desc(M, N, K, lda, N, N, krep);
  d.pool_rows = pool_rows;
  d.act = flags & 1 ? Act::Gelu : Act::None;
  d.res_f32 = flags >> 1 & 1;
  d.res_planes = flags >> 2 & 1;
  d.out_planes = flags >> 3 & 1;
  d.out_f16 = flags >> 4 & 1;
  d.out_f32 = flags >> 5 & 1;
  d.ln_in_chunks = flags >> 8 & 255;
  d.res_ln_chunks = flags >> 16 & 255;
  d.a_split = d.out_split = precision == 3;
  return d;
}

// The plan gemm() would pick for a conv (tests: which kind runs): out[0..7] = bm, bn, stages,
// splits, halo kind, window kind, waves, k per slice.  precision as spi_ops.h (3 = split).
extern "C" int spi_debug_conv_plan(int precision, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                   int pad, int* out) {
  if (!out || precision < 0 || precision > 3) return 1;
  put_plan(choose_plan(case_conv_desc(precision, B, H, W, Cin, Cout, KH, KW, stride, pad), case_prec(precision)), out);
  return 0;
}

// The whole plan of a dense problem.  flags: bit 0 an activation, 1 res_f32, 2 res_planes, 3 out_planes,
// 4 out_f16, 5 out_f32, bits 8..15 ln_in_chunks, 16..23 res_ln_chunks (gemm_plan.hpp).  out[0..3] = gemm256 tile height
// (0: the general kernel), slices, k-tile buffers, tile order; out[4..11] = the general kernel's plan as
// spi_debug_conv_plan; out[12], out[13] = split-K workspace floats, ticket slots.
extern "C" int spi_debug_gemm_plan(int precision, int M, int N, int K, int lda, int krep, int pool_rows, unsigned flags,
                                   long long* out) {
  if (!out || precision < 0 || precision > 3 || M < 1 || N < 1 || K < 1 || krep < 1 || krep > 2) return 1;
  const GemmDesc d = case_dense_desc(precision, M, N, K, lda, krep, pool_rows, flags);
  const GemmPlan g = plan_gemm(d, case_prec(precision));
  out[0] = g.g256_bm;
  out[1] = g.g256_splits;
  out[2] = g.g256_nbuf;
  out[3] = g.g256_order;
  put_plan(g.pl, out + 4);
  out[12] = (long long)g.partial_floats;
  out[13] = (long long)g.counter_slots;
  return 0;
}

// The plan of two convs on one input (gemm_pair): out[0..7], out[8..15] = the two plans that launch,
// out[16] = grouped (one launch), out[17] = workgroups of both, out[18], out[19] = problem 1's slab and
// ticket offsets, out[20], out[21] = the summed workspace floats and ticket slots a caller sizes for.
extern "C" int spi_debug_conv_pair_plan(int precision, int B, int H, int W, int Cin, int Cout0, int KH0, int KW0,
                                        int stride0, int pad0, int Cout1, int KH1, int KW1, int stride1, int pad1,
                                        long long* out) {
  if (!out || precision < 0 || precision > 3) return 1;
  const GemmDesc d0 = case_conv_desc(precision, B, H, W, Cin, Cout0, KH0, KW0, stride0, pad0);
  const GemmDesc d1 = case_conv_desc(precision, B, H, W, Cin, Cout1, KH1, KW1, stride1, pad1);
  const Prec prec = case_prec(precision);
  const PairPlan pp = plan_pair(d0, d1, prec);
  put_plan(pp.q0, out);
  put_plan(pp.q1, out + 8);
  out[16] = pp.grouped;
  out[17] = pp.wgs;
  out[18] = (long long)pp.slab_off;
  out[19] = (long long)pp.ticket_off;
  out[20] = (long long)pp.partial_floats;
  out[21] = (long long)pp.counter_slots;
  return 0;
}

}  // namespace spi
