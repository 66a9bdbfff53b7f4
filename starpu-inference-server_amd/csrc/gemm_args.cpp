// Host side of a general-kernel launch (gemm.hip): validation of a desc and the kernel arguments
// of a problem under its plan.  Plain C++17, no HIP: tests/test_gemm_args.py checks it through the
// debug exports below -- the arguments against tests/golden/gemm_args.json, the workgroup -> tile
// map by walking every workgroup of a launch through the kernels' own decode.
#include "gemm_args.hpp"

#include "row_util.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <stdexcept>

namespace spi {
namespace {

int ilog2(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return s;
}

}  // namespace

void validate_gemm(const GemmDesc& d, const GemmPtrs& p, Prec prec) {
  if (d.pool_rows && (d.conv || d.pool_rows > 64 || d.M % d.pool_rows))
    throw std::invalid_argument("pooled GEMM: dense A, pool_rows <= 64 dividing M");
  if (d.krep != 1 && (d.krep != 2 || prec != Prec::F16 || d.Kpad % (2 * estep_of(prec)) ||
                      (d.conv && (d.Cin < estep_of(prec) || d.KH * d.KW > 31))))
    throw std::invalid_argument("krep = 2 needs F16, a packed Kpad of whole step pairs and dense or one-tap-per-step A");
  if (prec == Prec::F16X3 && d.a_split && d.conv && (d.Cin < 32 || d.KH * d.KW > 31))
    throw std::invalid_argument("split activations need Cin >= 32 and <= 31 filter taps");
  if (d.ln_in_chunks > 0 || d.res_ln_chunks > 0 || d.ln_out) {
    // the fold lives in the dense fp16 kernels' vector epilogue: whole 128-column tiles,
    // 16-byte aligned rows everywhere it reads or writes
    const bool ok = prec == Prec::F16 && !d.conv && !d.pool_rows && d.N % 128 == 0 &&
                    d.ldc % 8 == 0 && aligned(p.C, 16) && (!p.bias || aligned(p.bias, 16)) &&
                    (!p.res || (d.ldr % 8 == 0 && aligned(p.res, 16))) &&
                    (d.ln_in_chunks == 0 || (p.ln.in_stats && p.ln.c1 && aligned(p.ln.c1, 16))) &&
                    (d.res_ln_chunks == 0 ||
                     (p.res && (d.res_f32 || d.res_planes) && p.ln.res_stats && aligned(p.ln.res_g, 16) &&
                      aligned(p.ln.res_b, 16))) &&
                    (!d.ln_out ||
                     (p.ln.out_stats && (p.ln.c16 ? aligned(p.ln.c16, 16) && d.ld16 % 8 == 0 : d.out_planes)));
    if (!ok) throw std::invalid_argument("LayerNorm fold: dense fp16 GEMM, N % 128 == 0, aligned vectors");
  }
  if (d.res_planes || d.out_planes) {
    // two fp16 planes: the F16 dense epilogue, 16-byte aligned rows and plane offset
    if (prec != Prec::F16 || d.conv || d.pool_rows || d.plane % 8 || (d.res_planes && (!p.res || d.res_f32)) ||
        (d.out_planes && (d.out_f32 || d.out_f16)))
      throw std::invalid_argument("two-plane residual / output: dense fp16 GEMM, plane offset a multiple of 8");
    // a two-plane output keeps an fp16-typed residual in two planes too (Model::run_gemm's rule; an
    // fp32 residual -- the stream's first block -- is the one other kind)
    if (d.out_planes && p.res && !d.res_f32 && !d.res_planes)
      throw std::invalid_argument("two-plane output: the residual is fp32 or two planes");
  }
}

KArgs make_args(int mode, const GemmDesc& d, const GemmPtrs& p, const Plan& pl) {
  const Prec prec = prec_of_mode(mode);
  KArgs a{};
  a.d = d;
  a.p = p;
  a.k_per_split = pl.k_per_split;
  a.splits = pl.splits;
  a.tiles = plan_tiles(d, pl);
  a.tiles_m = a.tiles / ((d.N + pl.bn - 1) / pl.bn);
  const int TM = a.tiles_m, TN = a.tiles / a.tiles_m;
  a.tiles_n = TN;
  xcd_groups(d, prec, TM, TN, a.xg_m, a.xg_n);
  if (pl.splits > 1) {  // split-K grids: the plain column-major order
    a.xg_m = 1;
    a.xg_n = std::min(8, TN);
  }
  for (int i = 0; i <= 8; ++i) {
    a.rg_m0[i] = std::min(i, a.xg_m) * TM / a.xg_m;
    a.cg_n0[i] = std::min(i, a.xg_n) * TN / a.xg_n;
  }
  for (int i = 0; i < 8; ++i) a.fd_rows[i] = make_fastdiv((unsigned)std::max(1, a.rg_m0[i + 1] - a.rg_m0[i]));
  a.fd_split = make_fastdiv((unsigned)std::max(1, pl.splits));
  a.fd_tiles = make_fastdiv((unsigned)std::max(1, a.tiles));
  if (d.conv) {
    a.fd_ohw = make_fastdiv((unsigned)(d.OH * d.OW));
    a.fd_ow = make_fastdiv((unsigned)d.OW);
    a.imgs = d.M / (d.OH * d.OW);
  }
  a.cin_shift = d.conv ? ilog2(d.Cin) : 0;
  a.kw_mul = (65536 + d.KW - 1) / d.KW;
  a.cell_uniform = cell_uniform(d, prec);
  a.vec_ok = d.ldc % 8 == 0 && aligned(p.C, 16) && (!p.res || (d.ldr % 8 == 0 && aligned(p.res, 16))) &&
             (!p.bias || aligned(p.bias, 16));
  if (pl.halo) {
    a.h_th = pl.th;
    a.h_period = pl.period;
    a.h_off = pl.off;
    a.h_hwp = d.W + 2 * d.pad;
    a.h_hp = (pl.th + 2) * a.h_hwp;
    a.h_nblk = d.Cin / estep_of(prec);
    a.h_bps = pl.bps;
    a.fd_period = make_fastdiv((unsigned)std::max(1, pl.period));
    a.fd_hwp = make_fastdiv((unsigned)a.h_hwp);
  }
  if (pl.win) a.win_nblk_shift = ilog2(d.Cin / estep_of(prec));
  return a;
}

KGroup make_group(int mode, const GemmDesc& d0, const GemmPtrs& p0, const GemmDesc& d1, const GemmPtrs& p1,
                  const PairPlan& pp) {
  KGroup g{};
  g.a[0] = make_args(mode, d0, p0, pp.q0);
  GemmPtrs p1s = p1;
  if (pp.q0.splits > 1) {  // keep clear of problem 0's slabs / tickets
    p1s.partial = p0.partial + pp.slab_off;
    p1s.counters = p0.counters + pp.ticket_off;
  }
  g.a[1] = make_args(mode, d1, p1s, pp.q1);
  g.wgs0 = pp.wgs0;
  return g;
}

// ---------------------------------------------------------------------------
// Debug exports (CPU tests): the case arguments are those of the planner's exports
// (spi_debug_conv_plan, spi_debug_gemm_plan, spi_debug_conv_pair_plan in gemm_plan.cpp).
// ---------------------------------------------------------------------------
namespace {

struct ArgsDigest {  // FNV-1a over the fields' values, 8 bytes each (no padding, no raw bytes)
  unsigned long long h = 1469598103934665603ull;
  void u(long long v) {
    for (int i = 0; i < 8; ++i) {
      h ^= ((unsigned long long)v >> (8 * i)) & 255;
      h *= 1099511628211ull;
    }
  }
  void p(const void* q) { u((long long)reinterpret_cast<uintptr_t>(q)); }
  void f(float v) {
    unsigned b;
    std::memcpy(&b, &v, 4);
    u(b);
  }
};
void digest_args(ArgsDigest& g, const KArgs& a) {
  const GemmDesc& d = a.d;
  for (long long v : std::initializer_list<long long>{
           d.M, d.N, d.K, d.Kpad, (long long)d.wplane, d.lda, d.ldc, d.ldr, d.conv, d.H, d.W, d.Cin, d.OH, d.OW, d.KH,
           d.KW, d.stride, d.pad, (int)d.act, d.out_f32, d.out_f16, d.res_f32, d.a_split, d.out_split, d.pool_rows,
           d.krep, d.w_image, d.ln_in_chunks, d.res_ln_chunks, d.ln_out, d.ld16, d.res_planes, d.out_planes,
           (long long)d.plane})
    g.u(v);
  g.f(d.ln_in_eps);
  g.f(d.res_ln_eps);
  const GemmPtrs& p = a.p;
  for (const void* q : std::initializer_list<const void*>{p.A, p.W, p.bias, p.res, p.C, p.partial, p.counters, p.zeros,
                                                          p.ln.in_stats, p.ln.c1, p.ln.res_stats, p.ln.res_g,
                                                          p.ln.res_b, p.ln.out_stats, p.ln.c16})
    g.p(q);
  // what make_args computes: 32-bit fields without padding from k_per_split to splits, none negative
  for (const unsigned* q = reinterpret_cast<const unsigned*>(&a.k_per_split);
       q <= reinterpret_cast<const unsigned*>(&a.splits); ++q)
    g.u(*q);
}

// fixed, 16-byte aligned pointers that nothing dereferences; unaligned_c moves C off 16 bytes
GemmPtrs debug_ptrs(int unaligned_c) {
  GemmPtrs p;
  p.A = reinterpret_cast<const void*>((uintptr_t)0x10000000);
  p.W = reinterpret_cast<const void*>((uintptr_t)0x20000000);
  p.bias = reinterpret_cast<const float*>((uintptr_t)0x30000000);
  p.res = reinterpret_cast<const void*>((uintptr_t)0x40000000);
  p.C = reinterpret_cast<void*>((uintptr_t)0x50000000 + (unaligned_c ? 2 : 0));
  p.partial = reinterpret_cast<float*>((uintptr_t)0x60000000);
  p.counters = reinterpret_cast<int*>((uintptr_t)0x70000000);
  p.zeros = reinterpret_cast<const void*>((uintptr_t)0x80000000);
  return p;
}

void put_info(const KArgs& a, int* info) {
  const int v[5] = {a.tiles_m, a.tiles_n, a.splits, a.xg_m, a.xg_n};
  for (int i = 0; i < 5; ++i) info[i] = v[i];
}

// (tm, tn, kslice) of every workgroup of gemm_kernel's tiles x splits grid in launch order (x fastest),
// decoded as gemm_kernel does; at most cap workgroups are written
void put_map(const KArgs& a, const Plan& pl, int* map, int cap) {
  const bool sc = split_k_compiled(pl.bm, pl.bn, pl.halo != 0);
  for (int y = 0, n = 0; y < a.splits; ++y)
    for (int x = 0; x < a.tiles && n < cap; ++x, ++n) {
      const TileAt t = decode_tile(a, sc, x, y, x + y * a.tiles);
      map[3 * n] = t.tm, map[3 * n + 1] = t.tn, map[3 * n + 2] = t.kslice;
    }
}

int debug_args(int precision, const GemmDesc& d, int unaligned_c, unsigned long long* digest, int* info, int* map,
               int cap) {
  const Plan pl = plan_gemm(d, case_prec(precision)).pl;
  const KArgs a = make_args(precision, d, debug_ptrs(unaligned_c), pl);
  ArgsDigest g;
  digest_args(g, a);
  *digest = g.h;
  put_info(a, info);
  if (map) put_map(a, pl, map, cap);
  return 0;
}

}  // namespace

// One conv / one dense problem as gemm() would launch it on the general kernel, with fixed fake
// pointers (unaligned_c: C off 16 bytes).  digest: of every KArgs field; info[0..4] = tiles_m, tiles_n,
// splits, xg_m, xg_n; map (may be null): (tm, tn, kslice) per workgroup in launch order, cap workgroups.
extern "C" int spi_debug_conv_args(int precision, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                   int pad, int unaligned_c, unsigned long long* digest, int* info, int* map, int cap) {
  if (!digest || !info || precision < 0 || precision > 3) return 1;
  return debug_args(precision, case_conv_desc(precision, B, H, W, Cin, Cout, KH, KW, stride, pad), unaligned_c, digest,
                    info, map, cap);
}

extern "C" int spi_debug_gemm_args(int precision, int M, int N, int K, int lda, int krep, int pool_rows, unsigned flags,
                                   int unaligned_c, unsigned long long* digest, int* info, int* map, int cap) {
  if (!digest || !info || precision < 0 || precision > 3 || M < 1 || N < 1 || K < 1 || krep < 1 || krep > 2) return 1;
  return debug_args(precision, case_dense_desc(precision, M, N, K, lda, krep, pool_rows, flags), unaligned_c, digest,
                    info, map, cap);
}

// The two convs of a gemm_pair.  info[0..4], info[5..9] as above per problem, info[10] = grouped,
// info[11] = problem 0's workgroups, info[12] = both problems'; map: (problem, tm, tn, kslice) per
// workgroup -- of the one grouped launch as gemm_kernel_pair decodes it, else of the two launches in turn.
extern "C" int spi_debug_conv_pair_args(int precision, int B, int H, int W, int Cin, int Cout0, int KH0, int KW0,
                                        int stride0, int pad0, int Cout1, int KH1, int KW1, int stride1, int pad1,
                                        int unaligned_c, unsigned long long* digest, int* info, int* map, int cap) {
  if (!digest || !info || precision < 0 || precision > 3) return 1;
  const GemmDesc d0 = case_conv_desc(precision, B, H, W, Cin, Cout0, KH0, KW0, stride0, pad0);
  const GemmDesc d1 = case_conv_desc(precision, B, H, W, Cin, Cout1, KH1, KW1, stride1, pad1);
  const PairPlan pp = plan_pair(d0, d1, case_prec(precision));
  const GemmPtrs p0 = debug_ptrs(unaligned_c);
  GemmPtrs p1 = debug_ptrs(unaligned_c);
  p1.C = static_cast<char*>(p1.C) + 0x01000000;
  KGroup g{};
  if (pp.grouped) {
    g = make_group(precision, d0, p0, d1, p1, pp);
  } else {
    g.a[0] = make_args(precision, d0, p0, pp.q0);
    g.a[1] = make_args(precision, d1, p1, pp.q1);
    g.wgs0 = pp.wgs0;
  }
  ArgsDigest h;
  digest_args(h, g.a[0]);
  digest_args(h, g.a[1]);
  h.u(g.wgs0);
  *digest = h.h;
  put_info(g.a[0], info);
  put_info(g.a[1], info + 5);
  info[10] = pp.grouped;
  info[11] = pp.wgs0;
  info[12] = pp.wgs;
  if (!map) return 0;
  const Plan* q[2] = {&pp.q0, &pp.q1};
  for (int wg = 0; wg < pp.wgs && wg < cap; ++wg) {
    const int pr = pp.grouped ? pair_problem(g, wg) : wg >= pp.wgs0;
    const KArgs& a = g.a[pr];
    const int l = wg - (pr ? pp.wgs0 : 0);
    // grouped: gemm_kernel_pair's split; else this problem's own tiles x splits grid
    const PairAt w = pp.grouped ? pair_slice(a, l) : PairAt{l / a.tiles, l % a.tiles};
    const TileAt t = decode_tile(a, split_k_compiled(q[pr]->bm, q[pr]->bn, q[pr]->halo != 0), w.lin, w.kslice, l);
    map[4 * wg] = pr, map[4 * wg + 1] = t.tm, map[4 * wg + 2] = t.tn, map[4 * wg + 3] = t.kslice;
  }
  return 0;
}

// validate_gemm on a dense case (arguments of spi_debug_gemm_plan) with aligned fake pointers, the
// fold's among them: 0 accepted, 2 refused with the message in msg (cap bytes), 1 bad arguments.
extern "C" int spi_debug_validate_gemm(int precision, int M, int N, int K, int lda, int krep, int pool_rows,
                                       unsigned flags, char* msg, int cap) {
  if (!msg || cap < 1 || precision < 0 || precision > 3 || M < 1 || N < 1 || K < 1) return 1;
  const GemmDesc d = case_dense_desc(precision, M, N, K, lda, krep, pool_rows, flags);
  GemmPtrs p = debug_ptrs(0);
  p.ln.in_stats = p.ln.c1 = p.ln.res_stats = p.ln.res_g = p.ln.res_b = reinterpret_cast<const float*>((uintptr_t)0x90000000);
  msg[0] = 0;
  try {
    validate_gemm(d, p, case_prec(precision));
  } catch (const std::invalid_argument& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return 2;
  }
  return 0;
}

}  // namespace spi
