// MFMA GEMM and conv-as-implicit-GEMM for gfx950 (CDNA4).
//
// One kernel body serves every dense contraction of the three model families:
//   * ResNet conv + folded BN (+ residual) (+ ReLU)      -- implicit GEMM over NHWC
//   * ResNet FC, BERT/ViT QKV / out-proj / FFN (+GELU) (+residual) -- dense GEMM
//
// Staging.  Every k-step moves 128 bytes of each A row and each W row:
//   F16   64 fp16 k-values (2 x v_mfma_f32_16x16x32_f16 per fragment pair)
//   F32   32 fp32 k-values (8 x v_mfma_f32_16x16x4_f32; lane l feeds k index
//         (l>>4) of step s with element 8(l>>4)+s of its 32 bytes -- the same
//         permutation on A and B, so the sum is unchanged; exact fp32 FMA chain)
//   F16X3 32 fp32 A values + W row = 32 hi fp16 | 32 lo fp16 (interleaved
//         packing); A is split into hi/lo at fragment-read time; each fragment
//         pair issues lo*hi + hi*lo + hi*hi (fp32-grade at the fp16 rate).
// The tile images are filled with global_load_lds_dwordx4 (LDS-DMA, 1 KiB per
// wave instruction, lane-linear): image row r, 16-byte slot s holds global chunk
// s ^ (r & 7) -- the XOR swizzle is applied on the SOURCE address and undone on
// the ds_read_b128 (cdna_hip_programming.md rule 21), which makes the fp16
// fragment reads bank-conflict free.  Chunks outside the image (conv padding,
// rows past M, k past K) are read from a zeroed line, so the DMA never needs a
// predicate.  STAGES-deep ring: step t+STAGES-1 is issued right after the
// barrier that publishes step t, waits are counted vmcnt + s_barrier in one
// asm statement (no __syncthreads(): its vmcnt(0) would drain the prefetch).
//
// Small-M layers are split along K; the workgroups of a tile publish fp32 slabs
// write-through (sc1) and the last to arrive (relaxed agent-scope ticket) sums
// them with sc1 loads and runs the epilogue -- no second launch, no cache-wide
// fences (cdna_hip_programming.md, "In-launch split-K reduction").
//
// This file holds the kernels, the table of their instances and the launch.  The numbers of a kernel
// instance (modes, A-operand kinds, TileGeo: every constant of the body below and the static_asserts
// that guard them) are gemm_tile.hpp, shared with the planner; the hand-counted LDS-DMA, its waits,
// the swizzled fragment read and static_for are lds_dma.hpp, shared with conv_wres.hip.  What the
// host does before a launch is host-only code, checked without a GPU: the plan (gemm_plan.cpp), the
// desc checks and the kernel arguments (gemm_args.cpp), and in gemm_args.hpp the argument structs and
// the workgroup -> (tile, slice) decode, which the kernels below and the CPU tests both call.
// The diagnostic builds' macros and readers are gemm_diag.hpp.
#include "device_math.hpp"
#include "gemm_args.hpp"
#include "gemm_diag.hpp"
#include "gemm_plan.hpp"
#include "gemm_tile.hpp"
#include "lds_dma.hpp"
#include "ln_fold.hpp"
#include "pack.hpp"
#include "spi_kernels.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <stdexcept>

namespace spi {
namespace {

template <int V>
using IC = std::integral_constant<int, V>;

// Element types of a mode's A operand and (unless the desc says otherwise) its output / residual;
// the modes' numbers are gemm_tile.hpp.
template <int MODE>
struct Traits {
  using A = std::conditional_t<MODE == (int)Prec::F16, _Float16, float>;
  using Out = A;
};

// Split layout index (in fp16 units) of logical element (m, n) of a row-major
// [rows][ld] tensor: hi at the returned index, lo 32 further on.
__device__ __forceinline__ size_t split_idx(int m, int n, int ld) {
  return (size_t)m * ld * 2 + (size_t)(n >> 5) * 64 + (n & 31);
}

__device__ __forceinline__ float apply_act(float v, Act act) {
  if (act == Act::Relu) return v > 0.f ? v : 0.f;
  if (act == Act::Gelu) return gelu(v);
  return v;
}

template <int MODE>
__device__ __forceinline__ float load_res(const KArgs& a, int m, int n) {
  using Out = typename Traits<MODE>::Out;
  if constexpr (MODE == kF16X3S) {  // split residual: hi + lo
    const _Float16* R = static_cast<const _Float16*>(a.p.res);
    const size_t i = split_idx(m, n, a.d.ldr);
    return static_cast<float>(R[i]) + static_cast<float>(R[i + 32]);
  }
  const size_t idx = (size_t)m * a.d.ldr + n;
  if (a.d.res_planes) {  // two fp16 planes: hi + lo
    const _Float16* R = static_cast<const _Float16*>(a.p.res);
    return static_cast<float>(R[idx]) + static_cast<float>(R[idx + a.d.plane]);
  }
  return a.d.res_f32 ? static_cast<const float*>(a.p.res)[idx]
                     : static_cast<float>(static_cast<const Out*>(a.p.res)[idx]);
}

// fp32 A at fragment read (F16X3): 8 values as hi = fp16(x), lo = fp16(x - hi)
__device__ __forceinline__ void split8(const u32x4& x0, const u32x4& x1, half8& hi, half8& lo) {
  const floatx4 f0 = __builtin_bit_cast(floatx4, x0);
  const floatx4 f1 = __builtin_bit_cast(floatx4, x1);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const _Float16 a = static_cast<_Float16>(f0[e]);
    const _Float16 b = static_cast<_Float16>(f1[e]);
    hi[e] = a;
    hi[e + 4] = b;
    lo[e] = static_cast<_Float16>(f0[e] - static_cast<float>(a));
    lo[e + 4] = static_cast<_Float16>(f1[e] - static_cast<float>(b));
  }
}

// NW waves per workgroup in an (NW / 2) x 2 grid over the tile: wave (wm, wn)
// owns rows [wm * BM / (NW / 2), ...) x columns [wn * BN / 2, ...).
// The workgroup body: problem `a`, split-K slice `kslice`, linear tile `lin`.
// gemm_kernel passes its own arguments (constant kernarg offsets, preloadable);
// gemm_kernel_pair selects one of two problems at run time.
template <int MODE, int BM, int BN, int STAGES, int KIND, int NWA>
__device__ __forceinline__ void gemm_body(const KArgs& a, const int kslice_in, const int lin, const int hl) {
  // the instance's numbers (gemm_tile.hpp).  KG K groups of NW waves: everything below is one
  // group's (its waves, threads, LDS)
  using G = TileGeo<MODE, BM, BN, STAGES, KIND, NWA>;
  constexpr bool CONV = G::CONV, TAP = G::TAP, HALO = G::HALO, WIN = G::WIN, AR = G::AR, RPF = G::RPF, LNF = G::LNF;
  constexpr int KG = G::KG, NW = G::NW, NT = G::NT, ESTEP = G::ESTEP, EPC = G::EPC, RB = G::RB, CPR = G::CPR, RPI = G::RPI;
  constexpr int IMG = G::IMG, AQ = G::AQ, BQ = G::BQ, QPS = G::QPS, HQ = G::HQ, HBUF = G::HBUF, XQ = G::XQ, LDSB = G::LDSB;
  constexpr int WTM = G::WTM, WTN = G::WTN, TI = G::TI, TJ = G::TJ;
  using TR = Traits<MODE>;
  using AT = typename TR::A;
  __shared__ __attribute__((aligned(16))) char lds_wg[KG * LDSB];
  // K group (an SGPR) and its LDS: [0, LDSB) for group 0, [LDSB, 2 LDSB) for group 1
  const int grp = KG == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
  char* const lds = KG == 1 ? lds_wg : lds_wg + grp * LDSB;
  int* s_flag = reinterpret_cast<int*>(lds + LDSB - 16);
  [[maybe_unused]] unsigned long long rt_e = 0, rt_l0 = 0, rt_l1 = 0, rt_p1 = 0, rt_p2 = 0;
  SPI_RT(rt_e);
#ifdef SPI_GEMM_TIMELINE
  // kind: 0 plain tile, 1 split-K slice that did not reduce, 2 the reducing slice
  auto tl_out = [&](int kind) {
    unsigned long long rt_x;
    SPI_RT(rt_x);
    if (threadIdx.x == 0 && a.tl) {
      unsigned long long* g = g_gemm_timeline + (size_t)((blockIdx.x + blockIdx.y * gridDim.x) & 65535) * 8;
      g[0] = rt_e;
      g[1] = rt_l0;
      g[2] = rt_l1;
      g[3] = rt_x;
      g[4] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
             ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
      g[5] = (unsigned long long)kind;
      g[6] = rt_p1;
      g[7] = rt_p2;
    }
  };
#else
  auto tl_out = [](int) {};
#endif

  const GemmDesc& d = a.d;
  // wave index in an SGPR: every LDS-DMA destination (M0) is then scalar math.
  const int tid = KG == 1 ? (int)threadIdx.x : (int)threadIdx.x & (NT - 1), lane = tid & 63,
            wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // which tile and slice this workgroup owns: the XCD-aware decode of gemm_args.hpp
  const TileAt at = decode_tile(a, kSplitK<BM, BN, KIND>, lin, kslice_in, hl);
  [[maybe_unused]] const int tile = at.tile;
  const int tm = at.tm, tn = at.tn, kslice = at.kslice;
  const int n0 = tn * BN;
  SPI_RT(rt_p1);
  // m_lim: first row past this tile's valid rows.  Halo tiles map their rows to
  // output rows through the virtual-row bands (halo_m below) instead.
  int m0 = tm * BM, m_lim = d.M;
  if constexpr (!HALO) {
    if (d.pool_rows) {  // fused avgpool + FC: tile row tm = image tm's pixels
      m0 = tm * d.pool_rows;
      m_lim = m0 + d.pool_rows;
    }
  }
  // halo: first virtual output row of the band; halo_m(r) = output row of tile row
  // r (-1: a padding row of the virtual layout, or past the last image)
  const int h_u0 = HALO ? tm * a.h_th : 0;
  if constexpr (HALO) {
    if (!a.h_off) {  // aligned band: contiguous output rows [m0, m_lim) of one image
      const int img = fdiv(h_u0, a.fd_period), oy0 = h_u0 - img * a.h_period;
      m0 = (img * d.OH + oy0) * d.OW;
      m_lim = m0 + min(a.h_th, d.OH - oy0) * d.OW;
    }
  }
  [[maybe_unused]] auto halo_m = [&](int r) {
    const int ty = fdiv(r, a.fd_ow), tx = r - ty * d.OW;
    const int u = h_u0 + ty;
    const int img = fdiv(u, a.fd_period);
    const int oy = u - img * a.h_period - a.h_off;
    return (ty < a.h_th && img < a.imgs && (unsigned)oy < (unsigned)d.OH) ? (img * d.OH + oy) * d.OW + tx
                                                                                      : -1;
  };
  int kbeg = kslice * a.k_per_split;
  int kend = min(d.Kpad, kbeg + a.k_per_split);
  if constexpr (KG == 2) {
    // K groups: the first / second half of the slice's super-steps (the host plans an even
    // count per slice, so both groups run the same number of steps -- and of barriers)
    const int half = (kend - kbeg) / (6 * ESTEP) * (3 * ESTEP);
    if (grp == 0)
      kend = kbeg + half;
    else
      kbeg += half;
  }
  // halo: channel blocks [h_b0, h_b1) of this split-K slice, 9 taps each
  const int h_b0 = HALO ? kslice * a.h_bps : 0;
  const int h_b1 = HALO ? min(a.h_nblk, h_b0 + a.h_bps) : 0;
  const int nsteps = HALO ? (h_b1 - h_b0) * 9 : (kend - kbeg) / ESTEP;

  const char* zeros = static_cast<const char*>(a.p.zeros);
  const AT* __restrict__ Ap = static_cast<const AT*>(a.p.A);
  const char* __restrict__ Wb = static_cast<const char*>(a.p.W);

  // Per-lane source bookkeeping (fixed across k-steps).
  const int slot = lane & (CPR - 1);
  int a_koff[AQ], a_ih0[AQ], a_iw0[AQ];
  bool a_ok[AQ];
  const AT* a_base[AQ];
  const AT* a_pix[AQ];  // conv: image pointer at (ih0, iw0), may point before the image
  const AT* a_src[AQ];  // conv, one tap per step: a_pix + this lane's chunk offset
  // conv, one tap per step: bit (kh*KW + kw) set when that tap of this row lies
  // inside the image (0 for rows past M).  Indexed by the unrolled q only.
  uint32_t a_mask[AQ];
#pragma unroll
  for (int q = 0; q < (AR ? AQ : 0); ++q) {
    const int r = (wave * AQ + q) * RPI + lane / CPR;
    a_koff[q] = (slot ^ (r & (CPR - 1))) * EPC;
    const int m = m0 + r;
    a_ok[q] = m < d.M;
    const int mm = a_ok[q] ? m : 0;
    if constexpr (CONV) {
      const int img = fdiv(mm, a.fd_ohw);
      const int rem = mm - img * (d.OH * d.OW);
      const int oh = fdiv(rem, a.fd_ow);
      const int ow = rem - oh * d.OW;
      a_ih0[q] = oh * d.stride - d.pad;
      a_iw0[q] = ow * d.stride - d.pad;
      a_base[q] = Ap + (size_t)img * d.H * d.W * d.Cin;
      a_pix[q] = a_base[q] + ((ptrdiff_t)(a_ih0[q] * d.W + a_iw0[q]) << a.cin_shift);
      a_src[q] = a_pix[q] + a_koff[q];
      // valid taps: kh in [kh_lo, kh_hi) x kw in [kw_lo, kw_hi) -- one row of column bits
      // replicated per valid filter row (no per-tap compares)
      uint32_t mask = 0u;
      if (TAP && a_ok[q]) {
        const int kh_lo = max(0, -a_ih0[q]), kh_hi = min(d.KH, d.H - a_ih0[q]);
        const int kw_lo = max(0, -a_iw0[q]), kw_hi = min(d.KW, d.W - a_iw0[q]);
        const uint32_t cols = kw_hi > kw_lo ? (1u << kw_hi) - (1u << kw_lo) : 0u;
        for (int kh = kh_lo; kh < kh_hi; ++kh) mask |= cols << (kh * d.KW);
      }
      a_mask[q] = mask;
    } else {
      a_ih0[q] = a_iw0[q] = 0;
      a_base[q] = Ap + (size_t)mm * d.lda;
      a_pix[q] = a_base[q];
      a_src[q] = a_pix[q];
      a_mask[q] = 0u;
    }
  }
  const char* b_src[BQ];
#pragma unroll
  for (int q = 0; q < BQ; ++q) {
    const int r = (wave * BQ + q) * RPI + lane / CPR;
    const int c = slot ^ (r & (CPR - 1));
    // W rows are Kpad elements (F16/F32) or 2*Kpad fp16 (F16X3, 64-element blocks of hi|lo).
    const size_t row_bytes = (MODE == (int)Prec::F16) ? (size_t)d.Kpad * 2 : (size_t)d.Kpad * 4;
    b_src[q] = Wb + (size_t)(n0 + r) * row_bytes + c * 16;
  }

  // Halo bookkeeping.  DMA side: lane of instruction wave*HQ + q fills pixel p
  // (8 per instruction), slot s <- chunk s ^ (p & 7); h_src is its source for
  // channel block 0 (block b adds b * ESTEP elements), zeros when p lies in the
  // padding or past the halo.  Fragment side: h_row[i] = halo pixel of tap (0, 0)
  // for this lane's row of A fragment i (rows past the band read pixel 0; their
  // results are never stored).
  // Virtual input rows: aligned bands read rows of their own image only (row
  // oy0 - 1 + hy); stacked bands read virtual row u0 - 1 + hy, i.e. image
  // (u0 - 1 + hy) / period, row (u0 - 1 + hy) % period - 1 (the padding rows of the
  // stacked layout and rows past the last image read zeros).
  [[maybe_unused]] const AT* h_src[HQ];
  [[maybe_unused]] bool h_ok[HQ];
  [[maybe_unused]] int h_row[WTM / 16];
  if constexpr (HALO) {
    const int imgs = a.imgs;
#pragma unroll
    for (int q = 0; q < HQ; ++q) {
      const int p = (wave * HQ + q) * RPI + lane / CPR;
      const int c = slot ^ (p & (CPR - 1));
      const int hy = fdiv(p, a.fd_hwp), hx = p - hy * a.h_hwp;
      int img, iy;
      if (a.h_off) {
        const int vy = h_u0 - 1 + hy;
        img = vy < 0 ? imgs : fdiv(vy, a.fd_period);
        iy = vy - img * a.h_period - 1;
      } else {
        img = fdiv(h_u0, a.fd_period);
        iy = h_u0 - img * a.h_period - 1 + hy;
      }
      const int ix = hx - 1;
      h_ok[q] = p < a.h_hp && img < imgs && (unsigned)iy < (unsigned)d.H && (unsigned)ix < (unsigned)d.W;
      h_src[q] = Ap + ((size_t)((h_ok[q] ? img : 0) * d.H + (h_ok[q] ? iy : 0)) * d.W + (h_ok[q] ? ix : 0)) * d.Cin +
                 c * EPC;
    }
#pragma unroll
    for (int i = 0; i < WTM / 16; ++i) {
      const int r = (wave >> 1) * WTM + i * 16 + (lane & 15);
      const int ty = fdiv(r, a.fd_ow), tx = r - ty * d.OW;
      h_row[i] = ty < a.h_th ? ty * a.h_hwp + tx : 0;
    }
  }
  auto issue_halo = [&](int blk, int buf) {
    if constexpr (HALO) {
      char* dst = lds + STAGES * IMG + buf * HBUF;
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        const char* src = h_ok[q] ? reinterpret_cast<const char*>(h_src[q] + (size_t)blk * ESTEP) : zeros;
        SPI_DMA_A((const void*)SPI_A_SRC(src), (lds_ptr_t)(dst + (wave * HQ + q) * 1024), 16, 0, 0);
      }
    }
  };
  // Window kind: super-step j of the slice is global super-step w_g0 + j = (kh, channel block
  // cb), kh-major (g = kh * nblk + cb); its k-step 3 j + kw reads W k-step (kh * 3 + kw) *
  // nblk + cb (k = tap * Cin + c).  DMA side of a window: pieces q < BM / 32 of wave w (16
  // bytes a lane) fill rows (BM / 4) w + 8 q + lane / 8, slot lane & 7; the last piece (4 bytes
  // a lane) rows BM + 2 w + lane / 32, slot (lane & 31) / 4 -- w_off: the source byte offset in
  // the pixel's 128-byte block (chunk slot ^ (row & 7), the ring images' swizzle).
  [[maybe_unused]] const int w_g0 = WIN ? kbeg / (3 * ESTEP) : 0;
  [[maybe_unused]] const int w_nbs = WIN ? a.win_nblk_shift : 0;
  [[maybe_unused]] int w_row[XQ], w_off[XQ];
  if constexpr (WIN) {
#pragma unroll
    for (int q = 0; q < XQ - 1; ++q) {
      const int r = wave * (BM / 4) + q * 8 + (lane >> 3);
      w_row[q] = r;
      w_off[q] = ((lane & 7) ^ (r & 7)) << 4;
    }
    const int r = BM + wave * 2 + (lane >> 5);
    w_row[XQ - 1] = r;
    w_off[XQ - 1] = ((((lane & 31) >> 2) ^ (r & 7)) << 4) + ((lane & 3) << 2);
  }
  auto issue_win = [&](int jj, int buf) {
    if constexpr (WIN) {
      constexpr int PSH = __builtin_ctz(sizeof(AT));
      const int g = w_g0 + jj, kh = g >> w_nbs, cb = g & ((1 << w_nbs) - 1);
      const int p0 = m0 + (kh - 1) * d.W - 1;  // global pixel of window row 0
      const char* base = reinterpret_cast<const char*>(Ap) + cb * RB;
      char* dst = lds + STAGES * IMG + buf * HBUF;
#pragma unroll
      for (int q = 0; q < XQ; ++q) {
        const int pix = p0 + w_row[q];
        const char* src = (unsigned)pix < (unsigned)d.M ? base + ((size_t)pix << (a.cin_shift + PSH)) + w_off[q] : zeros;
        if (q < XQ - 1)
          glds16(SPI_A_SRC(src), dst + (wave * (XQ - 1) + q) * 1024);
        else
          glds4(SPI_A_SRC(src), dst + BM * RB + wave * 256);
      }
    }
  };
  [[maybe_unused]] int w_tap0 = 0, w_j = 0;  // the running super-step's kh * 3 and index

  // halo: scalar (block, tap) walk of the issued W steps; k = tap * Cin + c, so
  // step (blk, tap) is W k-step tap * nblk + blk
  int hw_blk = h_b0, hw_tap = 0;
  int hw_blk_next = 0, hw_buf_next = 0;  // the halo issued at tap 7 of the current block

  // Cin >= k-step (one (kh, kw) tap per step): a scalar walk over (tap, channel
  // block), advanced once per issued step (issue() is called for steps 0, 1, 2 ...
  // in order): cu_cell = tap index, cu_off = element offset of (kh, kw, channel)
  // from the row's (ih0, iw0) pixel.  Taps past KH*KW (the Kpad tail) have no
  // mask bit, so they read zeros.
  int cu_cell = 0, cu_kw = 0, cu_ci = 0, cu_off = 0;
  if constexpr (TAP) {
    {
      const int kbeg_a = d.krep == 2 ? kbeg >> 1 : kbeg;  // A k of the slice's first step (slices hold whole krep groups)
      cu_cell = kbeg_a >> a.cin_shift;
      const int kh = (cu_cell * a.kw_mul) >> 16;
      cu_kw = cu_cell - kh * d.KW;
      cu_ci = kbeg_a & (d.Cin - 1);
      cu_off = ((kh * d.W + cu_kw) << a.cin_shift) + cu_ci;
    }
  }
  int w_kb = (kbeg / ESTEP) * RB;  // W byte offset of the next issued step
  auto issue = [&](int step, int stage) {
    const int k0 = kbeg + step * ESTEP;
    char* dst = lds + stage * IMG;
    if constexpr (HALO) {
      const int wstep = hw_tap * a.h_nblk + hw_blk;
#pragma unroll
      for (int q = 0; q < BQ; ++q)
        SPI_DMA_W((const void*)(b_src[q] + (size_t)wstep * RB), (lds_ptr_t)(dst + (wave * BQ + q) * 1024), 16, 0, 0);
      if (++hw_tap == 9) {
        hw_tap = 0;
        ++hw_blk;
      }
      return;
    } else if constexpr (WIN) {
      const int jj = step / 3, kw = step - jj * 3;
      const int g = w_g0 + jj, kh = g >> w_nbs, cb = g & ((1 << w_nbs) - 1);
      const int wstep = ((kh * 3 + kw) << w_nbs) + cb;
#pragma unroll
      for (int q = 0; q < BQ; ++q)
        SPI_DMA_W((const void*)(b_src[q] + (size_t)wstep * RB), (lds_ptr_t)(dst + (wave * BQ + q) * 1024), 16, 0, 0);
      return;
    } else if constexpr (CONV) {
      if constexpr (TAP) {
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
          const bool ok = (a_mask[q] >> cu_cell) & 1u;
          const char* src = ok ? reinterpret_cast<const char*>(a_src[q] + cu_off) : zeros;
          SPI_DMA_A((const void*)SPI_A_SRC(src), (lds_ptr_t)(dst + (wave * AQ + q) * 1024), 16, 0, 0);
        }
        // advance one k-step: next channel block, or the next tap (next pixel,
        // or the next filter row: W - KW + 1 pixels on); krep = 2: after the
        // second (lo-weight) step of the pair only
        if (d.krep == 1 || (step & 1)) {
          cu_ci += ESTEP;
          cu_off += ESTEP;
          if (cu_ci == d.Cin) {
            cu_ci = 0;
            ++cu_cell;
            if (++cu_kw == d.KW) {
              cu_kw = 0;
              cu_off += (d.W - d.KW) << a.cin_shift;
            }
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
          const char* src = zeros;
          const int k = k0 + a_koff[q];
          if (a_ok[q] && k < d.K) {
            const int cell = k >> a.cin_shift;
            const int c = k & (d.Cin - 1);
            const int kh = (cell * a.kw_mul) >> 16;
            const int kw = cell - kh * d.KW;
            const int ih = a_ih0[q] + kh, iw = a_iw0[q] + kw;
            if ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)
              src = reinterpret_cast<const char*>(a_base[q] + ((size_t)(ih * d.W + iw) << a.cin_shift) + c);
          }
#ifndef SPI_DIAG_NO_DMA_GEN  // diagnostic build: general convs (the stem) issue no DMA
          SPI_DMA_A((const void*)SPI_A_SRC(src), (lds_ptr_t)(dst + (wave * AQ + q) * 1024), 16, 0, 0);
#endif
        }
      }
    } else {
      // krep = 2: packed steps 2s and 2s + 1 both stage A step s
      const int ka0 = d.krep == 2 ? (k0 / (2 * ESTEP)) * ESTEP : k0;
#pragma unroll
      for (int q = 0; q < AQ; ++q) {
        const int k = ka0 + a_koff[q];
        const char* src = (a_ok[q] && k < d.K) ? reinterpret_cast<const char*>(a_pix[q] + k) : zeros;
        SPI_DMA_A((const void*)SPI_A_SRC(src), (lds_ptr_t)(dst + (wave * AQ + q) * 1024), 16, 0, 0);
      }
    }
    // k-step byte offset inside a W row: RB bytes per step (advanced per issue).
#ifdef SPI_DIAG_NO_DMA_GEN
    if constexpr (KIND != kConvGen)
#endif
#pragma unroll
    for (int q = 0; q < BQ; ++q)
      SPI_DMA_W((const void*)(b_src[q] + w_kb), (lds_ptr_t)(dst + BM * RB + (wave * BQ + q) * 1024), 16, 0, 0);
    w_kb += RB;
  };

  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  floatx4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  // window kind: taps (bit kh * 3 + kw) inside the image for this lane's A fragment rows
  [[maybe_unused]] uint32_t w_mask[TI];
  if constexpr (WIN) {
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = m0 + wm * WTM + i * 16 + fr;
      uint32_t mask = 0u;
      if (m < d.M) {
        const int img = fdiv(m, a.fd_ohw), rem = m - img * (d.OH * d.OW);
        const int oh = fdiv(rem, a.fd_ow), ow = rem - oh * d.OW;
        const uint32_t cols = (ow > 0 ? 1u : 0u) | 2u | (ow + 1 < d.W ? 4u : 0u);
        mask = (oh > 0 ? cols : 0u) | (cols << 3) | (oh + 1 < d.H ? cols << 6 : 0u);
      }
      w_mask[i] = mask;
    }
  }

  // Residual tile prefetch (64 x 64 tiles on the vector epilogue path): the epilogue's
  // residual loads were the last dependent memory round trip of a launch (~0.5-1 us of a
  // ~1.2 us epilogue, tools/gemm_timeline.py).  The tile's residual rows go into LDS by
  // LDS-DMA at the first k-step that stages no further k-step (step nsteps - STAGES + 1),
  // into the stage region the step before it used (nsteps % STAGES); the epilogue parks its
  // fp32 tile in the last step's region ((nsteps - 1) % STAGES), so the two never meet.
  // Split-K tiles prefetch in the reducing slice only, after its ticket.  res_rb: bytes of a
  // residual tile row (64 fp16 = 128, 64 fp32 or split = 256); rpw: DMA pieces per wave.
  // (residual planes: a row's 64 hi values, then its 64 lo values)
  [[maybe_unused]] const int res_rb =
      (MODE == kF16X3S || sizeof(typename TR::Out) == 4 || d.res_f32 || d.res_planes) ? 256 : 128;
  [[maybe_unused]] const int rpw = res_rb * BM / 1024 / NW;  // 2 or 4
  [[maybe_unused]] const bool rpf_tile = RPF && a.p.res && a.vec_ok && n0 + BN <= d.N && !d.pool_rows;
  // (window kind: into the window buffer the last super-step does not use -- 9 KiB, so fp16
  // residual rows only -- and the tile parks at 0)
  [[maybe_unused]] const bool rpf_loop = rpf_tile && a.splits == 1 && (!WIN || res_rb == 128) && grp == 0;
  [[maybe_unused]] const int rpf_step = max(0, nsteps - STAGES + 1);
  [[maybe_unused]] const int rpf_off = WIN ? STAGES * IMG + ((nsteps / 3) & 1) * HBUF : (nsteps % STAGES) * IMG;
  [[maybe_unused]] const int park_off = WIN ? 0 : ((nsteps - 1) % STAGES) * IMG;
  auto issue_res = [&](char* dst) {
    if constexpr (RPF) {
      const int rpp = 1024 / res_rb, cpr = res_rb / 16;  // rows per piece, 16-byte chunks per row
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < rpw) {  // wave-uniform
          const int piece = wave * rpw + q;
          const int row = piece * rpp + lane / cpr, ch = lane % cpr;
          const int m = m0 + row;
          const char* src = zeros;
          if (m < m_lim) {
            if constexpr (MODE == kF16X3S)
              src = reinterpret_cast<const char*>(static_cast<const _Float16*>(a.p.res) + split_idx(m, n0, d.ldr)) + ch * 16;
            else if (d.res_planes)
              src = reinterpret_cast<const char*>(static_cast<const _Float16*>(a.p.res) + (size_t)m * d.ldr + n0 +
                                                  (ch >= 8 ? d.plane : 0)) + (ch & 7) * 16;
            else
              src = static_cast<const char*>(a.p.res) + ((size_t)m * d.ldr + n0) * (res_rb / 64) + ch * 16;
          }
          glds16(src, dst + piece * 1024);
        }
      }
    }
  };

  SPI_RT(rt_p2);
  if constexpr (HALO) issue_halo(h_b0, 0);  // lands before W step 0 (in-order vmcnt)
  if constexpr (WIN) issue_win(0, 0);
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nsteps) issue(s, s);

  // Epilogue through LDS (the K loop's ring is free by then; cdna_hip_programming.md
  // T21, store-issue-bound tails).  The waves park their raw accumulators as an fp32
  // [BM][BN] tile -- 16-column blocks XOR-swizzled by (row >> 2) & 3, so the
  // ds_write_b32 of a fragment (4 row groups x 16 columns) hits 64 distinct banks --
  // then every thread owns one 8-column group and walks rows, moving bias, residual
  // and output as 16-byte vectors (global_load/store_dwordx4) instead of the 2-4 byte
  // per-element accesses of the fragment layout (a 128x64 split tile: 16 vector
  // accesses per thread instead of 128 scalar ones).  All residual loads of a thread
  // go out before its first store (clamped rows: always-valid addresses, no branch).
  // Tiles crossing N, or unaligned strides, take the per-element path from LDS.
  // toff: byte offset of the parked tile in LDS; rl: the prefetched residual tile (issue_res)
  // or nullptr (the residual, if any, is read from global memory).
  auto finish = [&](floatx4 (&v)[TI][TJ], int toff, const char* rl) {
    using Out = typename TR::Out;
    float* T = reinterpret_cast<float*>(lds + toff);
    // the bias row of this thread's column group, in flight across the park
    const int nb_ = n0 + (tid % (BN / 8)) * 8;
    floatx4 bv0 = floatx4{0.f, 0.f, 0.f, 0.f}, bv1 = bv0;
    if (a.vec_ok && n0 + BN <= d.N && a.p.bias) {
      bv0 = *reinterpret_cast<const floatx4*>(a.p.bias + nb_);
      bv1 = *reinterpret_cast<const floatx4*>(a.p.bias + nb_ + 4);
    }
    // LayerNorm fold: the tile rows' {mean, rstd} once per row into LDS past the ring ([0, BM):
    // the A rows' (consumer), [BM, 2 BM): the residual rows' (res_ln)); read after the park's barrier
    [[maybe_unused]] float2* const ln_s = reinterpret_cast<float2*>(lds + STAGES * IMG + 2 * HBUF);
    if constexpr (LNF) {
      if (d.ln_in_chunks > 0)
        ln_tile_stats(a.p.ln.in_stats, m0, BM, d.M, d.ln_in_chunks, d.ln_in_eps, ln_s, tid, NT);
      if (d.res_ln_chunks > 0)
        ln_tile_stats(a.p.ln.res_stats, m0, BM, d.M, d.res_ln_chunks, d.res_ln_eps, ln_s + BM, tid, NT);
    }
    __syncthreads();  // every wave is done reading the ring
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm * WTM + i * 16 + fq * 4 + r;
          const int col = (wn * WTN + j * 16 + fr) ^ (fq << 4);  // (row >> 2) & 3 == fq
          T[row * BN + col] = v[i][j][r];
        }
    if (rl) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's residual pieces
    __syncthreads();
    if constexpr (!HALO && BM * BN * 4 + 256 * 4 <= LDSB - 16) {
      if (d.pool_rows) {
        // fused avgpool + FC: column means of the tile's pool_rows valid rows,
        // four row-interleaved partial sums per column, combined through LDS
        constexpr int PARTS = NT / BN;
        float* red = T + BM * BN;
        const int col = tid % BN, part = tid / BN;
        float sum = 0.f;
        for (int r = part; r < d.pool_rows; r += PARTS) sum += T[r * BN + (col ^ (((r >> 2) & 3) << 4))];
        red[part * BN + col] = sum;
        __syncthreads();
        if (tid < BN) {
          float tot = 0.f;
#pragma unroll
          for (int q = 0; q < PARTS; ++q) tot += red[q * BN + tid];
          const int n = n0 + tid;
          if (n < d.N) {
            const float y = apply_act(tot / (float)d.pool_rows + (a.p.bias ? a.p.bias[n] : 0.f), d.act);
            if (d.out_f32 || sizeof(typename TR::Out) == 4)
              static_cast<float*>(a.p.C)[(size_t)tm * d.ldc + n] = y;
            else
              static_cast<_Float16*>(a.p.C)[(size_t)tm * d.ldc + n] = static_cast<_Float16>(y);
          }
        }
        return;
      }
    }
    constexpr int G = BN / 8, RSTEP = NT / G, ITEMS = BM / RSTEP;
    const int cg = tid % G, r0 = tid / G;
    const int nb = n0 + cg * 8;
    // 0 fp16, 1 fp32, 2 split layout, 3 two fp16 planes
    const int fmt = (split_mode(MODE) && d.out_split) ? 2 : d.out_planes ? 3 : d.out_f16 ? 0
                    : (d.out_f32 || sizeof(Out) == 4) ? 1 : 0;
    // output row of tile row `row`, -1 when it is not stored
    auto row_m = [&](int row) -> int {
      if constexpr (HALO) {
        if (a.h_off) return halo_m(row);
      }
      const int m = m0 + row;
      return m < m_lim ? m : -1;
    };
    auto tile_vals = [&](int row, float (&y)[8]) {
      const float* src = T + row * BN + ((cg * 8) ^ (((row >> 2) & 3) << 4));
      const floatx4 x0 = *reinterpret_cast<const floatx4*>(src);
      const floatx4 x1 = *reinterpret_cast<const floatx4*>(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y[e] = x0[e];
        y[e + 4] = x1[e];
      }
    };
    auto finish_act = [&](auto& y) {
      constexpr int NI = sizeof(y) / sizeof(y[0]);
      auto apply = [&](auto act_tag) {
        constexpr Act act = decltype(act_tag)::value;
#pragma unroll
        for (int it = 0; it < NI; ++it)
#pragma unroll
          for (int e = 0; e < 8; ++e) y[it][e] = apply_act(y[it][e], act);
      };
      if (d.act == Act::Relu) {
        apply(std::integral_constant<Act, Act::Relu>{});
      } else if (d.act == Act::Gelu && fmt == 0) {
        // fp16 output: the packed degree-7/6 GELU (device_math.hpp gelu2, |erf error| 2.5e-6, 80x
        // under an fp16 half-ulp) at half the VALU of the scalar 13/8 form; fp32 / split outputs
        // keep the 4.5e-7 form (fp32 parity bar)
#pragma unroll
        for (int it = 0; it < NI; ++it)
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const float2v g2 = gelu2(float2v{y[it][e], y[it][e + 1]});
            y[it][e] = g2.x;
            y[it][e + 1] = g2.y;
          }
      } else if (d.act == Act::Gelu) {
        apply(std::integral_constant<Act, Act::Gelu>{});
      } else {
        apply(std::integral_constant<Act, Act::None>{});
      }
    };
    float b[8];
    if (a.vec_ok && n0 + BN <= d.N) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[e] = bv0[e];
        b[e + 4] = bv1[e];
      }
      // LayerNorm fold vectors of this thread's 8 columns: c1 (consumer), gain / bias of the
      // residual's LayerNorm (res_ln)
      [[maybe_unused]] float lnc1[8], lng[8], lnb[8];
      if constexpr (LNF) {
        const auto ld8 = [&](const float* v, float (&o)[8]) {
          const floatx4 x0 = *reinterpret_cast<const floatx4*>(v + nb);
          const floatx4 x1 = *reinterpret_cast<const floatx4*>(v + nb + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = x0[e];
            o[e + 4] = x1[e];
          }
        };
        if (d.ln_in_chunks > 0) ld8(a.p.ln.c1, lnc1);
        if (d.res_ln_chunks > 0) {
          ld8(a.p.ln.res_g, lng);
          ld8(a.p.ln.res_b, lnb);
        }
      }
      // rows in chunks of <= 4 per thread: the residual loads of a chunk are all in
      // flight before its first store, within a bounded register budget
      constexpr int CH = ITEMS < 4 ? ITEMS : 4;
#pragma unroll
      for (int c0 = 0; c0 < ITEMS; c0 += CH) {
        float y[CH][8];
#pragma unroll
        for (int it = 0; it < CH; ++it) {
#pragma unroll
          for (int e = 0; e < 8; ++e) y[it][e] = 0.f;
        }
        if (RPF && rl) {
          // the residual tile from LDS ([row][res_rb] as issue_res laid it out)
#pragma unroll
          for (int it = 0; it < CH; ++it) {
            const char* rr = rl + (r0 + (c0 + it) * RSTEP) * res_rb;
            if constexpr (MODE == kF16X3S) {
              const char* q = rr + (cg >> 2) * 128 + (cg & 3) * 16;
              const half8 hi = *reinterpret_cast<const half8*>(q);
              const half8 lo = *reinterpret_cast<const half8*>(q + 64);
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = static_cast<float>(hi[e]) + static_cast<float>(lo[e]);
            } else if (d.res_planes) {
              const half8 hi = *reinterpret_cast<const half8*>(rr + cg * 16);
              const half8 lo = *reinterpret_cast<const half8*>(rr + 128 + cg * 16);
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = static_cast<float>(hi[e]) + static_cast<float>(lo[e]);
            } else if (d.res_f32 || sizeof(Out) == 4) {
              const floatx4 r0v = *reinterpret_cast<const floatx4*>(rr + cg * 32);
              const floatx4 r1v = *reinterpret_cast<const floatx4*>(rr + cg * 32 + 16);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                y[it][e] = r0v[e];
                y[it][e + 4] = r1v[e];
              }
            } else {
              const half8 r = *reinterpret_cast<const half8*>(rr + cg * 16);
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = static_cast<float>(r[e]);
            }
          }
        } else if (a.p.res) {
#pragma unroll
          for (int it = 0; it < CH; ++it) {
            const int mr = row_m(r0 + (c0 + it) * RSTEP);
            const int m = mr < 0 ? 0 : mr;  // skipped rows load row 0 (always valid)
            if constexpr (MODE == kF16X3S) {
              const _Float16* R = static_cast<const _Float16*>(a.p.res) + split_idx(m, nb, d.ldr);
              const half8 hi = *reinterpret_cast<const half8*>(R);
              const half8 lo = *reinterpret_cast<const half8*>(R + 32);
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = static_cast<float>(hi[e]) + static_cast<float>(lo[e]);
            } else if (d.res_planes) {
              const _Float16* R = static_cast<const _Float16*>(a.p.res) + (size_t)m * d.ldr + nb;
              const half8 hi = *reinterpret_cast<const half8*>(R);
              const half8 lo = *reinterpret_cast<const half8*>(R + d.plane);
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = static_cast<float>(hi[e]) + static_cast<float>(lo[e]);
            } else if (d.res_f32 || sizeof(Out) == 4) {
              const float* R = static_cast<const float*>(a.p.res) + (size_t)m * d.ldr + nb;
              const floatx4 r0v = *reinterpret_cast<const floatx4*>(R);
              const floatx4 r1v = *reinterpret_cast<const floatx4*>(R + 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                y[it][e] = r0v[e];
                y[it][e + 4] = r1v[e];
              }
            } else {
              const half8 r = *reinterpret_cast<const half8*>(static_cast<const _Float16*>(a.p.res) +
                                                              (size_t)m * d.ldr + nb);
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = static_cast<float>(r[e]);
            }
          }
        }
        if constexpr (LNF) {
          // LayerNorm fold (ln_fold.hpp): the residual as LN(R) of the fp32 rows R loaded above
          if (d.res_ln_chunks > 0) {
#pragma unroll
            for (int it = 0; it < CH; ++it) {
              const float2 st = ln_s[BM + r0 + (c0 + it) * RSTEP];
#pragma unroll
              for (int e = 0; e < 8; ++e) y[it][e] = (y[it][e] - st.x) * st.y * lng[e] + lnb[e];
            }
          }
        }
#pragma unroll
        for (int it = 0; it < CH; ++it) {
          float t[8];
          tile_vals(r0 + (c0 + it) * RSTEP, t);
          if constexpr (LNF) {
            if (d.ln_in_chunks > 0) {  // consumer: y = rstd (acc - mean c1) + bias
              const float2 st = ln_s[r0 + (c0 + it) * RSTEP];
#pragma unroll
              for (int e = 0; e < 8; ++e) t[e] = st.y * (t[e] - st.x * lnc1[e]);
            }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) y[it][e] = t[e] + b[e] + y[it][e];  // acc + bias + residual
        }
        finish_act(y);
        if constexpr (LNF) {
          if (d.ln_out) {  // producer: chunk statistics + the fp16 copy of every output row
#pragma unroll
            for (int it = 0; it < CH; ++it) {
              const int m = row_m(r0 + (c0 + it) * RSTEP);
              float mean, m2;
              ln_chunk_stats(y[it], mean, m2);  // lanes of one row: consecutive cg
              if (m < 0) continue;
              if ((cg & 7) == 0)
                reinterpret_cast<float2*>(a.p.ln.out_stats)[(size_t)m * (d.N >> 6) + (nb >> 6)] = float2{mean, m2};
              if (a.p.ln.c16) {  // (two-plane outputs: the hi plane is the copy)
                half8 h;
#pragma unroll
                for (int e = 0; e < 8; ++e) h[e] = static_cast<_Float16>(y[it][e]);
                *reinterpret_cast<half8*>(a.p.ln.c16 + (size_t)m * d.ld16 + nb) = h;
              }
            }
          }
        }
#pragma unroll
        for (int it = 0; it < CH; ++it) {
          const int m = row_m(r0 + (c0 + it) * RSTEP);
          if (m < 0) continue;
          if (fmt == 2) {
            half8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              hi[e] = static_cast<_Float16>(y[it][e]);
              lo[e] = static_cast<_Float16>(y[it][e] - static_cast<float>(hi[e]));
            }
            _Float16* C = static_cast<_Float16*>(a.p.C) + split_idx(m, nb, d.ldc);
            *reinterpret_cast<half8*>(C) = hi;
            *reinterpret_cast<half8*>(C + 32) = lo;
          } else if (fmt == 3) {
            half8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              hi[e] = static_cast<_Float16>(y[it][e]);
              lo[e] = static_cast<_Float16>(y[it][e] - static_cast<float>(hi[e]));
            }
            _Float16* C = static_cast<_Float16*>(a.p.C) + (size_t)m * d.ldc + nb;
            *reinterpret_cast<half8*>(C) = hi;
            *reinterpret_cast<half8*>(C + d.plane) = lo;
          } else if (fmt == 1) {
            float* C = static_cast<float*>(a.p.C) + (size_t)m * d.ldc + nb;
            *reinterpret_cast<floatx4*>(C) = floatx4{y[it][0], y[it][1], y[it][2], y[it][3]};
            *reinterpret_cast<floatx4*>(C + 4) = floatx4{y[it][4], y[it][5], y[it][6], y[it][7]};
          } else {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = static_cast<_Float16>(y[it][e]);
            *reinterpret_cast<half8*>(static_cast<_Float16*>(a.p.C) + (size_t)m * d.ldc + nb) = h;
          }
        }
      }
      return;
    }
    // per-element path (tiles crossing N, unaligned strides)
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (a.p.bias && nb + e < d.N) ? a.p.bias[nb + e] : 0.f;
    for (int it = 0; it < ITEMS; ++it) {
      const int row = r0 + it * RSTEP, m = row_m(row);
      if (m < 0) continue;
      float y[8];
      tile_vals(row, y);
      for (int e = 0; e < 8; ++e) {
        const float r = (a.p.res && nb + e < d.N) ? load_res<MODE>(a, m, nb + e) : 0.f;
        y[e] = apply_act(y[e] + b[e] + r, d.act);
      }
      for (int e = 0; e < 8; ++e) {
        const int n = nb + e;
        if (n >= d.N) break;
        const float val = y[e];
        if (fmt == 2) {
          _Float16* C = static_cast<_Float16*>(a.p.C);
          const size_t k = split_idx(m, n, d.ldc);
          const _Float16 hi = static_cast<_Float16>(val);
          C[k] = hi;
          C[k + 32] = static_cast<_Float16>(val - static_cast<float>(hi));
        } else if (fmt == 3) {
          _Float16* C = static_cast<_Float16*>(a.p.C);
          const size_t k = (size_t)m * d.ldc + n;
          const _Float16 hi = static_cast<_Float16>(val);
          C[k] = hi;
          C[k + d.plane] = static_cast<_Float16>(val - static_cast<float>(hi));
        } else if (fmt == 1) {
          static_cast<float*>(a.p.C)[(size_t)m * d.ldc + n] = val;
        } else {
          static_cast<_Float16*>(a.p.C)[(size_t)m * d.ldc + n] = static_cast<_Float16>(val);
        }
      }
    }
  };

  [[maybe_unused]] unsigned long long st_t0 = 0, st_a = 0, st_b = 0, st_c = 0, st_d = 0, st_wait = 0, st_issue = 0, st_comp = 0;
  SPI_STAMP(st_t0);
  SPI_RT(rt_l0);
  // One k-step; U = t % STAGES is a compile-time constant (the loop below is
  // unrolled by STAGES), so every stage offset -- M0 of the DMAs, the base of
  // the fragment reads -- is an immediate.
  // Halo steps also take the tap (a constant), whether this is the slice's last
  // channel block, and that block's halo buffer.
  // steady_c (std::true_type): a step that issues step t + STAGES - 1, waits for the full ring
  // and is not at or after the residual prefetch -- no per-step checks at all (the loops below
  // run every step that far from the slice's end this way; round 4 had them checked per step,
  // ~55 SALU + 7 branches per step that made the ingest-bound loops 30 % slower)
  auto kstep = [&](int t, auto u_arg, auto tap_arg, bool last_blk, const char* Hs, auto steady_c) {
    const int U = u_arg;  // a constant when u_arg is a std::integral_constant
    constexpr int TP = decltype(tap_arg)::value;
    constexpr bool STEADY = decltype(steady_c)::value;
    SPI_STAMP(st_a);
    // Step t has landed once at most (issued steps after t) DMA groups remain.
    // Halo: W step t + 1 is in flight, and at tap 8 of a block that has a
    // successor the next block's halo too (issued at tap 7, before W step t + 2);
    // the last step of the slice waits for everything.
    if constexpr (HALO) {
      // G W groups in flight behind step t (fewer near the slice's end); the next
      // block's halo goes out at tap 10 - STAGES (before W step t + STAGES - 1 =
      // that block's tap 0), so the waits of the taps after it allow it too
      constexpr int G = STAGES - 2;
      constexpr int GL = G < 8 - TP ? G : 8 - TP;
      constexpr bool XH = TP >= 11 - STAGES;
      if (last_blk)
        dma_wait_barrier<GL * BQ>();
      else if (XH)
        dma_wait_barrier<G * BQ + HQ>();
      else
        dma_wait_barrier<G * BQ>();
    } else if constexpr (WIN) {
      // issue order: window j, ..., W(3j + 2) and window j + 1 at step 3j, W(3j + 3) at 3j + 1,
      // W(3j + 4) at 3j + 2.  Step 3j needs window j and W(3j) (W(3j + 1) in flight), 3j + 1
      // needs W(3j + 1) (W(3j + 2) and window j + 1 in flight), 3j + 2 needs W(3j + 2)
      // (window j + 1 and W(3j + 3)); last_blk: no super-step follows.  The residual
      // prefetch (issued at step 3j + 1 of the last super-step) stays in flight at 3j + 2.
      if constexpr (TP == 0) {
        dma_wait_barrier<BQ>();
      } else if constexpr (TP == 1) {
        if (last_blk)
          dma_wait_barrier<BQ>();
        else
          dma_wait_barrier<BQ + XQ>();
      } else {
        if (!last_blk)
          dma_wait_barrier<XQ + BQ>();
        else if (RPF && rpf_loop)
          dma_wait_barrier<2>();  // rpw = 2: 64 fp16 residual rows
        else
          dma_wait_barrier<0>();
      }
    } else if constexpr (STEADY) {
      dma_wait_barrier<(STAGES - 2) * QPS>();
    } else {
      // steps after the residual prefetch (rpf_loop, issued youngest at rpf_step) also leave
      // its rpw pieces in flight
      const bool rx = RPF && rpf_loop && t > rpf_step;
      auto wait = [&](auto n_c) {
        constexpr int N = decltype(n_c)::value;
        if (!rx)
          dma_wait_barrier<N>();
        else if (rpw == 2)
          dma_wait_barrier<N + 2>();
        else
          dma_wait_barrier<N + 4>();
      };
      if constexpr (STAGES == 4) {
        if (t + 2 < nsteps)
          wait(std::integral_constant<int, 2 * QPS>{});
        else if (t + 1 < nsteps)
          wait(std::integral_constant<int, QPS>{});
        else
          wait(std::integral_constant<int, 0>{});
      } else if constexpr (STAGES == 3) {
        if (t + 1 < nsteps)
          wait(std::integral_constant<int, QPS>{});
        else
          wait(std::integral_constant<int, 0>{});
      } else {
        wait(std::integral_constant<int, 0>{});
      }
    }
    SPI_STAMP(st_b);
    // All of this step's fragment reads go out first, then the next step's
    // DMAs (their issue cost overlaps the LDS latency), then the MFMAs.
    const char* As = lds + U * IMG;
    const char* Bs = AR ? As + BM * RB : As;
    // A fragment i: image and row (halo: pixel of this tap, kh * (W + 2) + kw on; window:
    // row + kw)
    const char* Ab = AR ? As : Hs;
    [[maybe_unused]] const int toff = HALO ? (TP / 3) * a.h_hwp + TP % 3 : 0;
    auto arow = [&](int i) {
      if constexpr (HALO)
        return h_row[i] + toff;
      else if constexpr (WIN)
        return wm * WTM + i * 16 + fr + TP;
      else
        return wm * WTM + i * 16 + fr;
    };
    // window kind: is tap (kh, TP) of fragment row i inside the image
    [[maybe_unused]] auto tap_ok = [&](int i) { return ((w_mask[i] >> (w_tap0 + TP)) & 1u) != 0u; };
    auto issue_next = [&] {
      if constexpr (HALO) {
        if (TP == 10 - STAGES && !last_blk) issue_halo(hw_blk_next, hw_buf_next);
      }
      if (STEADY || t + STAGES - 1 < nsteps) issue(t + STAGES - 1, (U + STAGES - 1) % STAGES);
      if constexpr (WIN) {
        if (TP == 0 && !last_blk) issue_win(w_j + 1, (w_j + 1) & 1);
      }
      if constexpr (!STEADY) {
        if (RPF && rpf_loop && t == rpf_step) issue_res(lds + rpf_off);
      }
    };
    if constexpr (MODE == (int)Prec::F16) {
      half8 af[2][TI], bf[2][TJ];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
          af[kk][i] = __builtin_bit_cast(half8, rd_chunk<RB>(Ab, arow(i), kk * 4 + fq));
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          bf[kk][j] = __builtin_bit_cast(half8, rd_chunk<RB>(Bs, wn * WTN + j * 16 + fr, kk * 4 + fq));
      }
      issue_next();
      SPI_STAMP(st_c);
      if constexpr (WIN) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const bool ok = tap_ok(i);
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) af[kk][i] = ok ? af[kk][i] : half8{};
        }
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
#ifdef SPI_DIAG_NO_MFMA  // diagnostic build: fragments read, no matrix work
            asm volatile("" ::"v"(af[kk][i]), "v"(bf[kk][j]));
#else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
#endif
    } else if constexpr (split_mode(MODE)) {
      static_assert(ESTEP == 32, "one 32-k block per step");
      // fp32 A: two 16-byte chunks split into hi/lo below; split A: hi and lo
      // chunks read like W's (the same conflict-free pattern).
      u32x4 ar0[TI], ar1[TI];
      half8 bh[TJ], bl[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const int row = arow(i);
        ar0[i] = rd_chunk<RB>(Ab, row, MODE == kF16X3S ? fq : 2 * fq);
        ar1[i] = rd_chunk<RB>(Ab, row, MODE == kF16X3S ? 4 + fq : 2 * fq + 1);
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int row = wn * WTN + j * 16 + fr;
        bh[j] = __builtin_bit_cast(half8, rd_chunk<RB>(Bs, row, fq));
        bl[j] = __builtin_bit_cast(half8, rd_chunk<RB>(Bs, row, 4 + fq));
      }
      issue_next();
      SPI_STAMP(st_c);
      if constexpr (WIN) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const bool ok = tap_ok(i);
          ar0[i] = ok ? ar0[i] : u32x4{};
          ar1[i] = ok ? ar1[i] : u32x4{};
        }
      }
      half8 ah[TI], al[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        if constexpr (MODE == kF16X3S) {
          ah[i] = __builtin_bit_cast(half8, ar0[i]);
          al[i] = __builtin_bit_cast(half8, ar1[i]);
        } else {
          split8(ar0[i], ar1[i], ah[i], al[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
#ifdef SPI_DIAG_NO_MFMA
          asm volatile("" ::"v"(al[i]), "v"(ah[i]), "v"(bh[j]), "v"(bl[j]));
#else
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
#endif
        }
    } else {
      floatx4 a0[TI], a1[TI], b0[TJ], b1[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const int row = arow(i);
        a0[i] = __builtin_bit_cast(floatx4, rd_chunk<RB>(Ab, row, 2 * fq));
        a1[i] = __builtin_bit_cast(floatx4, rd_chunk<RB>(Ab, row, 2 * fq + 1));
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int row = wn * WTN + j * 16 + fr;
        b0[j] = __builtin_bit_cast(floatx4, rd_chunk<RB>(Bs, row, 2 * fq));
        b1[j] = __builtin_bit_cast(floatx4, rd_chunk<RB>(Bs, row, 2 * fq + 1));
      }
      issue_next();
      SPI_STAMP(st_c);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i][s], b0[j][s], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][s], b1[j][s], acc[i][j], 0, 0, 0);
    }
#ifdef SPI_GEMM_STAMPS
    // MFMA results are consumed only at the end; force completion so the compute phase is timed.
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) asm volatile("" ::"v"(acc[i][j]));
#endif
    SPI_STAMP(st_d);
    st_wait += st_b - st_a;
    st_issue += st_c - st_b;
    st_comp += st_d - st_c;
  };
  using I0 = IC<0>;
  using I1 = IC<1>;
  using I2 = IC<2>;
  using I3 = IC<3>;
  if constexpr (HALO) {
    // one channel block per iteration, its 9 taps unrolled (3 stages: stage =
    // tap % 3, a constant; deeper rings: a scalar stage counter)
    const int nb = h_b1 - h_b0;
    int u = 0;
    for (int j = 0; j < nb; ++j) {
      const bool lb = j == nb - 1;
      const char* Hs = lds + STAGES * IMG + (j & 1) * HBUF;
      hw_blk_next = h_b0 + j + 1;
      hw_buf_next = (j + 1) & 1;
      const int t = j * 9;
      // (written out: driven by static_for<0, 9>, hipcc allocates the two fp32 halo kernels differently,
      // 160 -> 140 and 154 -> 134 VGPRs, ~40 instructions fewer each -- kept byte-identical instead)
      if constexpr (STAGES == 3) {
        kstep(t + 0, I0{}, std::integral_constant<int, 0>{}, lb, Hs, std::false_type{});
        kstep(t + 1, I1{}, std::integral_constant<int, 1>{}, lb, Hs, std::false_type{});
        kstep(t + 2, I2{}, std::integral_constant<int, 2>{}, lb, Hs, std::false_type{});
        kstep(t + 3, I0{}, std::integral_constant<int, 3>{}, lb, Hs, std::false_type{});
        kstep(t + 4, I1{}, std::integral_constant<int, 4>{}, lb, Hs, std::false_type{});
        kstep(t + 5, I2{}, std::integral_constant<int, 5>{}, lb, Hs, std::false_type{});
        kstep(t + 6, I0{}, std::integral_constant<int, 6>{}, lb, Hs, std::false_type{});
        kstep(t + 7, I1{}, std::integral_constant<int, 7>{}, lb, Hs, std::false_type{});
        kstep(t + 8, I2{}, std::integral_constant<int, 8>{}, lb, Hs, std::false_type{});
      } else {
        auto nx = [&] {
          const int v = u;
          u = u + 1 == STAGES ? 0 : u + 1;
          return v;
        };
        kstep(t + 0, nx(), std::integral_constant<int, 0>{}, lb, Hs, std::false_type{});
        kstep(t + 1, nx(), std::integral_constant<int, 1>{}, lb, Hs, std::false_type{});
        kstep(t + 2, nx(), std::integral_constant<int, 2>{}, lb, Hs, std::false_type{});
        kstep(t + 3, nx(), std::integral_constant<int, 3>{}, lb, Hs, std::false_type{});
        kstep(t + 4, nx(), std::integral_constant<int, 4>{}, lb, Hs, std::false_type{});
        kstep(t + 5, nx(), std::integral_constant<int, 5>{}, lb, Hs, std::false_type{});
        kstep(t + 6, nx(), std::integral_constant<int, 6>{}, lb, Hs, std::false_type{});
        kstep(t + 7, nx(), std::integral_constant<int, 7>{}, lb, Hs, std::false_type{});
        kstep(t + 8, nx(), std::integral_constant<int, 8>{}, lb, Hs, std::false_type{});
      }
    }
  } else if constexpr (WIN) {
    // one super-step (kh, channel block) per iteration, its three kw taps unrolled: the W
    // stage is kw (slices start at a multiple of 3 steps), the window buffer j & 1
    // (every super-step but the last one is steady: constant waits, no residual prefetch)
    const int ns = nsteps / 3;
    for (int j = 0; j < ns - 1; ++j) {
      const char* Ws = lds + STAGES * IMG + (j & 1) * HBUF;
      w_tap0 = ((w_g0 + j) >> w_nbs) * 3;
      w_j = j;
      kstep(3 * j, I0{}, I0{}, false, Ws, std::true_type{});
      kstep(3 * j + 1, I1{}, I1{}, false, Ws, std::true_type{});
      kstep(3 * j + 2, I2{}, I2{}, false, Ws, std::true_type{});
    }
    {
      const int j = ns - 1;
      const char* Ws = lds + STAGES * IMG + (j & 1) * HBUF;
      w_tap0 = ((w_g0 + j) >> w_nbs) * 3;
      w_j = j;
      kstep(3 * j, I0{}, I0{}, true, Ws, std::false_type{});
      kstep(3 * j + 1, I1{}, I1{}, true, Ws, std::false_type{});
      kstep(3 * j + 2, I2{}, I2{}, true, Ws, std::false_type{});
    }
  } else if constexpr (TAP) {
    // unrolled by STAGES: stage offsets are immediates (the conv loop is short;
    // unrolling the large dense-GEMM bodies measured 1-2 % slower end to end)
    // steady iterations while every step of the iteration issues a step (t + 2 STAGES - 2 <
    // nsteps), then the checked ones
    using S1 = std::true_type;
    using S0 = std::false_type;
    int t = 0;
    for (; t + 2 * STAGES - 1 <= nsteps; t += STAGES) {
      kstep(t, I0{}, I0{}, false, nullptr, S1{});
      kstep(t + 1, I1{}, I0{}, false, nullptr, S1{});
      if constexpr (STAGES > 2) kstep(t + 2, I2{}, I0{}, false, nullptr, S1{});
      if constexpr (STAGES > 3) kstep(t + 3, I3{}, I0{}, false, nullptr, S1{});
    }
    for (; t + STAGES <= nsteps; t += STAGES) {
      kstep(t, I0{}, I0{}, false, nullptr, S0{});
      kstep(t + 1, I1{}, I0{}, false, nullptr, S0{});
      if constexpr (STAGES > 2) kstep(t + 2, I2{}, I0{}, false, nullptr, S0{});
      if constexpr (STAGES > 3) kstep(t + 3, I3{}, I0{}, false, nullptr, S0{});
    }
    if (t < nsteps) kstep(t, I0{}, I0{}, false, nullptr, S0{});
    if constexpr (STAGES > 2)
      if (t + 1 < nsteps) kstep(t + 1, I1{}, I0{}, false, nullptr, S0{});
    if constexpr (STAGES > 3)
      if (t + 2 < nsteps) kstep(t + 2, I2{}, I0{}, false, nullptr, S0{});
  } else {
    // steady while step t + STAGES - 1 exists (then t < rpf_step too)
    int t = 0;
    for (; t + STAGES - 1 < nsteps; ++t) kstep(t, t % STAGES, I0{}, false, nullptr, std::true_type{});
    for (; t < nsteps; ++t) kstep(t, t % STAGES, I0{}, false, nullptr, std::false_type{});
  }

  SPI_STAMP(st_d);
  SPI_RT(rt_l1);
#ifdef SPI_GEMM_STAMPS
  if (threadIdx.x == 0) {
    unsigned long long* gs = g_gemm_stamps + (size_t)(blockIdx.x & 65535) * 8;
    gs[0] = st_d - st_t0;
    gs[1] = st_wait;
    gs[2] = st_issue;
    gs[3] = st_comp;
    gs[4] = (unsigned long long)nsteps;
  }
#endif
  if constexpr (KG == 2) {
    // K groups: group 1 parks its partial in fragment order (thread t's accumulator (i, j) is
    // 16 contiguous bytes at ((i TJ + j) NT + t) 16) in its own W stages 0-1 -- free since the
    // last step's barrier (that step reads stage 2 and a window) -- and exits; group 0 adds it
    // to its own and goes on alone (s_barrier waits for the surviving waves only).
    static_assert(TI * TJ * NT * 16 <= 2 * IMG, "group 1's partial fits its W stages 0-1");
    floatx4* const part = reinterpret_cast<floatx4*>(lds_wg + LDSB);
    if (grp == 1) {
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) part[(i * TJ + j) * NT + tid] = acc[i][j];
    }
    lds_barrier();
    if (grp == 1) return;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[i][j] += part[(i * TJ + j) * NT + tid];
  }
  if (!kSplitK<BM, BN, KIND> || a.splits == 1) {
    if (RPF && rpf_loop)
      finish(acc, park_off, lds + rpf_off);
    else
      finish(acc, 0, nullptr);
    tl_out(0);
    return;
  }
  if constexpr (kSplitK<BM, BN, KIND>) {

  // ---- split-K: the last slice to arrive reduces -----------------------------
  // Every slice publishes its slab write-through (sc1) in fragment order (thread tid's
  // accumulator (i, j) is 16 contiguous bytes at ((i*TJ + j)*NT + tid)*16), drains its stores
  // (vmcnt(0)) and takes a relaxed agent-scope ticket; the last to arrive resets the ticket,
  // prefetches the residual, reads the other slabs with sc1 loads (MI355X_MICROARCH.md, the
  // sc1 hand-off) and adds its own partial from registers.  (Round 4 tried tickets first --
  // only the non-last slices store, the last one polls a published-slab count: the poll made
  // the reducer ~1.2 us slower, tools/gemm_timeline.py.)  Partials are summed in split order
  // whichever slice arrives last: deterministic results.
  const int splits = a.splits;
  constexpr int SLAB = BM * BN;
  int* words = a.p.counters + tile;  // the tile's arrival ticket
  float* tile_slabs = a.p.partial + (size_t)tile * splits * SLAB;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(tile_slabs, (short)0, splits * SLAB * 4, 0x00020000);
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int off = (kslice * SLAB + ((i * TJ + j) * NT + tid) * 4) * 4;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rs, off, 0, 16);
    }
  dma_wait_barrier<0>();  // the slab stores are vector memory too
  if (tid == 0) {
    const int ticket = __hip_atomic_fetch_add(words, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == splits - 1;
    if (last) __hip_atomic_store(words, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_flag = last;
  }
  __syncthreads();
  if (!*s_flag) {
    tl_out(1);
    return;
  }
  const bool rpf_red = RPF && rpf_tile;
  char* const red_res = lds + (WIN ? STAGES * IMG : IMG);  // the parked tile takes [0, BM * BN * 4)
  if (rpf_red) issue_res(red_res);
  // ZR splits' slabs in flight per round (two for the small tiles, one when a slab is 8+
  // fragments per thread); loads past the last slab fall outside the descriptor's range and
  // return 0 (no branch, no per-load wait); this slice's own slot is loaded and ignored (its
  // partial is still in registers).
  constexpr int ZR = TI * TJ <= 4 ? 2 : 1;
  floatx4 sum[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) sum[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int z0 = 0; z0 < splits; z0 += ZR) {
    floatx4 v[ZR][TI][TJ];
#pragma unroll
    for (int zz = 0; zz < ZR; ++zz)
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int off = ((z0 + zz) * SLAB + ((i * TJ + j) * NT + tid) * 4) * 4;
          v[zz][i][j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
        }
#pragma unroll
    for (int zz = 0; zz < ZR; ++zz) {
      const bool own = z0 + zz == kslice;
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) sum[i][j] += own ? acc[i][j] : v[zz][i][j];
    }
  }
  finish(sum, 0, rpf_red ? red_res : nullptr);
  tl_out(2);
  }
}

template <int MODE, int BM, int BN, int STAGES, int KIND, int NW = 4>
__global__ __launch_bounds__(64 * NW, (kMinWaves<BM, BN, STAGES, KIND, NW>)) void gemm_kernel(KArgs a) {
  gemm_body<MODE, BM, BN, STAGES, KIND, NW>(a, blockIdx.y, blockIdx.x, blockIdx.x + blockIdx.y * a.tiles);
}

// Grouped launch (KGroup): 1-D grid, problem-major, then slice, then tile.
template <int MODE, int BM, int BN, int STAGES, int KIND, int NW = 4>
__global__ __launch_bounds__(64 * NW, (kMinWaves<BM, BN, STAGES, KIND, NW>)) void gemm_kernel_pair(KGroup g) {
  // One body per problem (a branch on a workgroup-uniform condition), each with constant kernel
  // argument offsets: selecting the problem's KArgs by reference had every field become a select of
  // two loaded values -- SGPR spills to VGPR lanes and the tile decode's FastDiv tables copied to
  // scratch and read back with a dynamic offset (40 bytes of scratch per lane, round 6)
  const int lin = blockIdx.x;
  if (pair_problem(g, lin)) {
    const int l1 = lin - g.wgs0;
    const PairAt w = pair_slice(g.a[1], l1);
    gemm_body<MODE, BM, BN, STAGES, KIND, NW>(g.a[1], w.kslice, w.lin, l1);
  } else {
    const PairAt w = pair_slice(g.a[0], lin);
    gemm_body<MODE, BM, BN, STAGES, KIND, NW>(g.a[0], w.kslice, w.lin, lin);
  }
}

// The instance table of the ring kinds: the plan's (BM, BN, STAGES) as integral constants.  One
// problem (launch_tile) and a grouped pair (dispatch_pair) pick their kernel through it, so a
// grouped launch and its two-launch fallback cannot disagree about the tiles that exist.
template <class F>
void with_tile(const Plan& pl, F&& f) {
  if (pl.bm == 128 && pl.bn == 128) {
    f(IC<128>{}, IC<128>{}, IC<2>{});
  } else if (pl.bm == 128 && pl.stages == 2) {
    f(IC<128>{}, IC<64>{}, IC<2>{});
  } else if (pl.bm == 128) {
    f(IC<128>{}, IC<64>{}, IC<3>{});
  } else if (pl.stages == 2) {
    f(IC<64>{}, IC<64>{}, IC<2>{});
  } else if (pl.stages == 4) {
    f(IC<64>{}, IC<64>{}, IC<4>{});
  } else {
    f(IC<64>{}, IC<64>{}, IC<3>{});
  }
}

template <int MODE, int BM, int BN, int STAGES>
void launch_tile(const KArgs& a, dim3 grid, hipStream_t s) {
  if (a.cell_uniform) {
    SPI_LAUNCH((gemm_kernel<MODE, BM, BN, STAGES, kConvTap>), grid, dim3(256), 0, s, a);
  } else if (a.d.conv) {
    if constexpr (MODE != kF16X3S) {  // split A needs one tap per step (validate_gemm)
      SPI_LAUNCH((gemm_kernel<MODE, BM, BN, STAGES, kConvGen>), grid, dim3(256), 0, s, a);
    }
  } else {
    SPI_LAUNCH((gemm_kernel<MODE, BM, BN, STAGES, kDense>), grid, dim3(256), 0, s, a);
  }
}

// One problem under its plan: grid tiles x splits.
template <int MODE>
void dispatch(const Plan& pl, const KArgs& g, hipStream_t s) {
  const dim3 grid(g.tiles, pl.splits);
  if (pl.halo) {
    if constexpr (MODE != (int)Prec::F16X3) {  // fp32 A is split at fragment read: not a halo mode
      if (pl.bm == 256) {
        SPI_LAUNCH((gemm_kernel<MODE, 256, 64, 3, kConvHalo, 8>), grid, dim3(512), 0, s, g);
      } else if (pl.bm == 128) {
        SPI_LAUNCH((gemm_kernel<MODE, 128, 64, 3, kConvHalo>), grid, dim3(256), 0, s, g);
      } else if (pl.halo == 2) {
        SPI_LAUNCH((gemm_kernel<MODE, 64, 64, 3, kConvHaloS>), grid, dim3(256), 0, s, g);
      } else {
        SPI_LAUNCH((gemm_kernel<MODE, 64, 64, 3, kConvHalo>), grid, dim3(256), 0, s, g);
      }
    }
    return;
  }
  if (pl.win) {
    if constexpr (MODE == (int)Prec::F16 || MODE == kF16X3S) {
      if (pl.nw == 8) {
        // K groups: both must walk the same number of super-steps (their barriers pair up)
        const int ES = estep_of(MODE);
        if (pl.bm != 64 || pl.k_per_split % (6 * ES) || g.d.Kpad % (6 * ES))
          throw std::logic_error("window kind with K groups: slices of an even number of super-steps");
        SPI_LAUNCH((gemm_kernel<MODE, 64, 64, 3, kConvTapW, 8>), grid, dim3(512), 0, s, g);
      } else if (pl.bm == 128) {
        SPI_LAUNCH((gemm_kernel<MODE, 128, 64, 3, kConvTapW>), grid, dim3(256), 0, s, g);
      } else {
        SPI_LAUNCH((gemm_kernel<MODE, 64, 64, 3, kConvTapW>), grid, dim3(256), 0, s, g);
      }
    }
    return;
  }
  with_tile(pl, [&](auto bm, auto bn, auto st) {
    launch_tile<MODE, decltype(bm)::value, decltype(bn)::value, decltype(st)::value>(g, grid, s);
  });
}

// Two tap-walk conv problems sharing pl's tile shape and ring depth: one launch.
template <int MODE>
void dispatch_pair(const Plan& pl, const KGroup& g, int wgs, hipStream_t s) {
  const dim3 grid(wgs);
  with_tile(pl, [&](auto bm, auto bn, auto st) {
    SPI_LAUNCH((gemm_kernel_pair<MODE, decltype(bm)::value, decltype(bn)::value, decltype(st)::value, kConvTap>), grid,
               dim3(256), 0, s, g);
  });
}

// make_args' arguments as launched: a timeline build marks the launches of a stamping thread
KArgs stamped(KArgs a) {
#ifdef SPI_GEMM_TIMELINE
  a.tl = tl_thread();
#endif
  return a;
}

template <int MODE>
void launch(const GemmDesc& d, const GemmPtrs& p, const Plan& pl, hipStream_t s) {
  dispatch<MODE>(pl, stamped(make_args(MODE, d, p, pl)), s);
}

// Two problems in one launch when plan_pair groups them, else one launch each.
template <int MODE>
void launch_pair(const GemmDesc& d0, const GemmPtrs& p0, const GemmDesc& d1, const GemmPtrs& p1, hipStream_t s) {
  const PairPlan pp = plan_pair(d0, d1, prec_of_mode(MODE));
  if (!pp.grouped) {
    launch<MODE>(d0, p0, pp.q0, s);
    launch<MODE>(d1, p1, pp.q1, s);
    return;
  }
  KGroup g = make_group(MODE, d0, p0, d1, p1, pp);
  g.a[0] = stamped(g.a[0]);
  g.a[1] = stamped(g.a[1]);
  dispatch_pair<MODE>(pp.q0, g, pp.wgs, s);
}

// The kernel mode of a launch as an integral constant.
template <class F>
void with_mode(int mode, F&& f) {
  switch (mode) {
    case (int)Prec::F32: return f(IC<(int)Prec::F32>{});
    case (int)Prec::F16: return f(IC<(int)Prec::F16>{});
    case (int)Prec::F16X3: return f(IC<(int)Prec::F16X3>{});
    case kF16X3S: return f(IC<kF16X3S>{});  // split A: one (kh, kw) cell per 32-k step, fp32's addressing
  }
}

}  // namespace

void gemm_pair(const GemmDesc& d0, const GemmPtrs& p0, const GemmDesc& d1, const GemmPtrs& p1, Prec prec,
               hipStream_t s) {
  validate_gemm(d0, p0, prec);
  validate_gemm(d1, p1, prec);
  if (prec == Prec::F16X3 && d0.a_split != d1.a_split) {
    gemm(d0, p0, prec, s);
    gemm(d1, p1, prec, s);
    return;
  }
  with_mode(mode_of(prec, d0.a_split), [&](auto m) { launch_pair<decltype(m)::value>(d0, p0, d1, p1, s); });
}

void gemm(const GemmDesc& d, const GemmPtrs& p, Prec prec, hipStream_t s) {
  validate_gemm(d, p, prec);
  const GemmPlan g = plan_gemm(d, prec);
  // gemm256's producer epilogue exists over an fp32 residual into fp32 and over two planes in place
  // of form (the transformers' out-proj / FFN2); any other producer keeps the general kernel, as the
  // plan cannot tell: it does not see the residual pointer
  const bool g256_producer_ok = !d.ln_out || (p.res && ((d.res_f32 && d.out_f32) || (d.res_planes && d.out_planes)));
  if (prec == Prec::F16 && conv_wres_eligible(d, prec, p))
    conv_wres(d, p, s);
  else if (prec == Prec::F16 && g.g256_bm && g256_producer_ok && (reinterpret_cast<uintptr_t>(p.A) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(p.W) & 15) == 0)  // 16-byte LDS-DMA pieces
    gemm256(d, p, g.g256_splits, s, g.g256_bm, g.g256_nbuf, g.g256_order);
  else
    with_mode(mode_of(prec, d.a_split), [&](auto m) { launch<decltype(m)::value>(d, p, g.pl, s); });
}

// Whether gemm() would hand this spi_op_conv2d call to conv_wres (tests: which kernel runs): 1 or 0, -1 on
// bad arguments.  The desc is the one ops.cpp builds for a weight from spi_op_pack_weight; the pointers are
// placeholders, 16-byte aligned (an unaligned operand keeps the general kernel, which this cannot see).
// Launches nothing, needs no device.
extern "C" int spi_debug_conv_route(int precision, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                    int pad, int has_residual, int act) {
  if (precision < 0 || precision > 3 || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 ||
      stride < 1 || pad < 0 || act < 0 || act > 2)
    return -1;
  const Prec prec = case_prec(precision);
  GemmDesc d = case_conv_desc(precision, B, H, W, Cin, Cout, KH, KW, stride, pad);
  d.act = static_cast<Act>(act);
  d.w_image = packed_has_wres_image(prec, Cout, d.K, round_up_to(Cout, 128), d.Kpad);
  const auto at = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
  GemmPtrs p;
  p.A = at(0x10000000);
  p.W = at(0x20000000);
  p.bias = static_cast<const float*>(at(0x30000000));
  p.res = has_residual ? at(0x40000000) : nullptr;
  p.C = const_cast<void*>(at(0x50000000));
  p.zeros = at(0x80000000);
  return prec == Prec::F16 && conv_wres_eligible(d, prec, p) ? 1 : 0;
}

}  // namespace spi
