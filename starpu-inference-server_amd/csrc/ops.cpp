// Op-level C entry points (include/spi_ops.h): the individual kernels behind
// the forward passes, for kernel-level parity tests and micro-benchmarks.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <exception>
#include <string>
#include <vector>

#include "../../include/spi_ops.h"
#include "gconv.hpp"
#include "gemm_plan.hpp"
#include "ln_fold_pack.hpp"
#include "pack.hpp"
#include "resample.hpp"
#include "row_util.hpp"
#include "spi_kernels.hpp"

extern "C" void spi_set_last_error(const char* msg);

namespace {

constexpr size_t kZeroBytes = 256;
constexpr size_t kTickets = 16384;
constexpr size_t kSlabFloats = (size_t)16 << 20;  // 64 MiB of split-K slabs (gemm256 at ViT-L FFN2: 40 MiB)

bool prec_of(int32_t p, spi::Prec* out) {
  if (p == 0) *out = spi::Prec::F32;
  else if (p == 1) *out = spi::Prec::F16;
  else if (p == 2 || p == 3) *out = spi::Prec::F16X3;  // 3: split activations
  else return false;
  return true;
}

constexpr int32_t kSplitPrecision = 3;

int fail(const std::string& m) {
  spi_set_last_error(m.c_str());
  return 1;
}

int check_launch() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

// The launchers throw std::invalid_argument on a desc they cannot run; no C++ exception may
// cross the C boundary, so every entry point that reaches one runs its body through this.
template <typename F>
int guarded(F&& body) {
  try {
    return body();
  } catch (const std::exception& e) {
    return fail(e.what());
  } catch (...) {
    return fail("unknown C++ exception");
  }
}

spi::GemmPtrs scratch(void* ws) {
  spi::GemmPtrs p;
  char* base = static_cast<char*>(ws);
  p.zeros = base;
  p.counters = reinterpret_cast<int*>(base + kZeroBytes);
  p.partial = reinterpret_cast<float*>(base + kZeroBytes + kTickets * sizeof(int));
  return p;
}

// The tail of every single-GEMM entry point: the workspace must hold the problem (too_large: the
// message when it does not; null: a kind that is never split), then launch on the workspace's scratch.
int run_gemm(const spi::GemmDesc& d, spi::Prec p, const void* A, const void* W, const float* bias, const void* res,
             void* C, const spi::LnPtrs& ln, void* workspace, void* stream, const char* too_large) {
  if (too_large && !spi::gemm_workspace_fits(d, p, kSlabFloats, kTickets)) return fail(too_large);
  spi::GemmPtrs ptrs = scratch(workspace);
  ptrs.A = A;
  ptrs.W = W;
  ptrs.bias = bias;
  ptrs.res = res;
  ptrs.C = C;
  ptrs.ln = ln;
  return guarded([&] {
    spi::gemm(d, ptrs, p, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

}  // namespace

extern "C" {

size_t spi_op_packed_bytes(int32_t precision, int32_t N, int32_t K, int32_t* Npad, int32_t* Kpad) {
  spi::Prec p;
  if (!prec_of(precision, &p) || N <= 0 || K <= 0) return 0;
  const int np = spi::round_up_to(N, 128), kp = spi::round_up_to(K, 64);
  if (Npad) *Npad = np;
  if (Kpad) *Kpad = kp;
  return spi::packed_bytes(p, np, kp);
}

int spi_op_pack_weight(int32_t precision, const float* w, int32_t N, int32_t K, void* dst) {
  spi::Prec p;
  if (!prec_of(precision, &p) || !w || !dst || N <= 0 || K <= 0) return fail("invalid pack arguments");
  const int np = spi::round_up_to(N, 128), kp = spi::round_up_to(K, 64);
  spi::pack_matrix_into(static_cast<char*>(dst), N, K, np, kp, p,
                        [&](int n, int k) { return w[(size_t)n * K + k]; });
  return 0;
}

size_t spi_op_workspace_bytes(void) { return kZeroBytes + kTickets * sizeof(int) + kSlabFloats * sizeof(float); }

int spi_op_gemm(int32_t precision, const void* A, int32_t M, int32_t K, int32_t lda, const void* W, int32_t N,
                const float* bias, const void* residual, int32_t res_f32, int32_t ldr, void* C, int32_t out_f32,
                int32_t ldc, int32_t act, void* workspace, void* stream) {
  spi::Prec p;
  if (!prec_of(precision, &p) || !A || !W || !C || !workspace || M <= 0 || N <= 0 || K <= 0 || lda < K ||
      ldc < N || act < 0 || act > 2)
    return fail("invalid gemm arguments");
  spi::GemmDesc d = spi::dense_desc(M, N, K, lda, ldc, ldr, 1);
  d.act = static_cast<spi::Act>(act);
  d.out_f32 = out_f32 != 0;
  d.res_f32 = res_f32 != 0;
  if (precision == kSplitPrecision) {
    if (K % 32 || N % 32 || lda % 32 || ldc % 32 || out_f32 || res_f32 || (residual && ldr % 32))
      return fail("split gemm needs K, N and strides multiples of 32, no fp32 operands");
    d.a_split = d.out_split = true;
  }
  return run_gemm(d, p, A, W, bias, residual, C, {}, workspace, stream, "gemm too large for the op workspace");
}

namespace {

// The descriptor of one op-level conv, as Model::conv_call builds a layer's; hilo: hi + lo weights.
// Returns an error message, or null.
const char* op_conv_desc(int32_t precision, spi::Prec p, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                         int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t act, bool hilo, bool out_f32,
                         bool res_f32, spi::GemmDesc* out) {
  const int min_cin = precision == 1 ? 8 : 4;  // one 16-byte chunk: 8 fp16 or 4 fp32
  if (B <= 0 || H <= 0 || W <= 0 || Cin < min_cin || (Cin & (Cin - 1)) || Cout <= 0 || KH <= 0 || KW <= 0 ||
      stride <= 0 || pad < 0 || act < 0 || act > 2)
    return "invalid conv arguments";
  spi::GemmDesc d = spi::conv_desc(B, H, W, Cin, Cout, KH, KW, stride, pad, hilo ? 2 : 1);
  if (H + 2 * pad < KH || W + 2 * pad < KW || d.OH <= 0 || d.OW <= 0) return "empty conv output";
  d.act = static_cast<spi::Act>(act);
  d.out_f32 = out_f32;
  d.res_f32 = res_f32;
  if (hilo) {
    if (precision != 1) return "hi + lo weights are an fp16 layout";
    if (Cin < 64 || KH * KW > 31) return "hi + lo conv needs Cin >= 64 and <= 31 filter taps";
  } else {
    // W_packed comes from spi_op_pack_weight (spi_ops.h), which writes the image rows
    d.w_image = spi::packed_has_wres_image(p, Cout, d.K, spi::round_up_to(Cout, 128), d.Kpad);
  }
  if (precision == kSplitPrecision) {
    if (Cin < 32 || Cout % 32 || KH * KW > 31)
      return "split conv needs Cin >= 32, Cout a multiple of 32 and <= 31 filter taps";
    if (out_f32 || res_f32) return "the split layout has no fp32 operands";
    d.a_split = d.out_split = true;
  }
  *out = d;
  return nullptr;
}

}  // namespace

int spi_op_conv2d(int32_t precision, const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* Wp,
                  int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, const float* bias,
                  const void* residual, void* y, int32_t act, void* workspace, void* stream) {
  spi::Prec p;
  if (!prec_of(precision, &p) || !x || !Wp || !y || !workspace) return fail("invalid conv arguments");
  spi::GemmDesc d;
  if (const char* e = op_conv_desc(precision, p, B, H, W, Cin, Cout, KH, KW, stride, pad, act, false, false, false, &d))
    return fail(e);
  return run_gemm(d, p, x, Wp, bias, residual, y, {}, workspace, stream, "conv too large for the op workspace");
}

// ---- hi + lo fp16 weights (GemmDesc::krep = 2) ----

size_t spi_op_packed_bytes_hilo(int32_t N, int32_t K, int32_t* Npad, int32_t* Kpad) {
  if (N <= 0 || K <= 0) return 0;
  const int np = spi::round_up_to(N, 128), kp = 2 * spi::round_up_to(K, 64);
  if (Npad) *Npad = np;
  if (Kpad) *Kpad = kp;
  return spi::packed_bytes(spi::Prec::F16, np, kp);
}

int spi_op_pack_weight_hilo(const float* w, int32_t N, int32_t K, void* dst) {
  if (!w || !dst || N <= 0 || K <= 0) return fail("invalid pack arguments");
  const int np = spi::round_up_to(N, 128), kp = 2 * spi::round_up_to(K, 64);
  // as Packer::pack_weight (model_pack.cpp): a [N][kp] matrix of packed elements; kp is a multiple
  // of 128, so never the 576 columns that carry the weight-resident conv's image rows
  spi::pack_matrix_into(static_cast<char*>(dst), N, kp, np, kp, spi::Prec::F16, [&](int n, int k) {
    return spi::hilo_element(k, K, [&](int kk) { return w[(size_t)n * K + kk]; });
  });
  return 0;
}

int spi_op_gemm_hilo(const void* A, int32_t M, int32_t K, int32_t lda, const void* W, int32_t N, const float* bias,
                     const void* residual, int32_t res_f32, int32_t ldr, void* C, int32_t out_f32, int32_t ldc,
                     int32_t act, void* workspace, void* stream) {
  if (!A || !W || !C || !workspace || M <= 0 || N <= 0 || K <= 0 || lda < K || ldc < N || act < 0 || act > 2 ||
      (residual && ldr < N))
    return fail("invalid gemm_hilo arguments");
  spi::GemmDesc d = spi::dense_desc(M, N, K, lda, ldc, ldr, 2);
  d.act = static_cast<spi::Act>(act);
  d.out_f32 = out_f32 != 0;
  d.res_f32 = res_f32 != 0;
  return run_gemm(d, spi::Prec::F16, A, W, bias, residual, C, {}, workspace, stream,
                  "gemm too large for the op workspace");
}

int spi_op_conv2d_hilo(const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* Wp, int32_t Cout,
                       int32_t KH, int32_t KW, int32_t stride, int32_t pad, const float* bias, const void* residual,
                       int32_t res_f32, void* y, int32_t out_f32, int32_t act, void* workspace, void* stream) {
  if (!x || !Wp || !y || !workspace) return fail("invalid conv arguments");
  spi::GemmDesc d;
  if (const char* e = op_conv_desc(1, spi::Prec::F16, B, H, W, Cin, Cout, KH, KW, stride, pad, act, true,
                                   out_f32 != 0, res_f32 != 0, &d))
    return fail(e);
  return run_gemm(d, spi::Prec::F16, x, Wp, bias, residual, y, {}, workspace, stream,
                  "conv too large for the op workspace");
}

int spi_op_conv_pair(int32_t precision, const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                     const spi_op_conv_spec* c0, const spi_op_conv_spec* c1, void* workspace, void* stream,
                     int64_t* plan_out) {
  spi::Prec p;
  if (!prec_of(precision, &p) || !x || !workspace) return fail("invalid conv_pair arguments");
  if (!c0 || !c1) return fail("conv_pair: null conv spec");
  const spi_op_conv_spec* c[2] = {c0, c1};
  spi::GemmDesc d[2];
  spi::GemmPtrs ptrs[2];
  for (int i = 0; i < 2; ++i) {
    if (!c[i]->W_packed || !c[i]->y) return fail("conv_pair: a spec without weights or output");
    if (const char* e = op_conv_desc(precision, p, B, H, W, Cin, c[i]->Cout, c[i]->KH, c[i]->KW, c[i]->stride,
                                     c[i]->pad, c[i]->act, c[i]->hilo != 0, c[i]->out_f32 != 0, false, &d[i]))
      return fail(e);
    ptrs[i] = scratch(workspace);
    ptrs[i].A = x;
    ptrs[i].W = c[i]->W_packed;
    ptrs[i].bias = c[i]->bias;
    ptrs[i].C = c[i]->y;
  }
  if (!spi::gemm_workspace_fits(d[0], p, kSlabFloats, kTickets, &d[1]))
    return fail("conv pair too large for the op workspace");
  return guarded([&] {
    if (plan_out) {
      const spi::PairPlan pp = spi::plan_pair(d[0], d[1], p);
      spi::put_plan(pp.q0, plan_out);
      spi::put_plan(pp.q1, plan_out + 8);
      plan_out[16] = pp.grouped;
      plan_out[17] = pp.wgs;
      plan_out[18] = (int64_t)pp.slab_off;
      plan_out[19] = (int64_t)pp.ticket_off;
      plan_out[20] = (int64_t)pp.partial_floats;
      plan_out[21] = (int64_t)pp.counter_slots;
    }
    spi::gemm_pair(d[0], ptrs[0], d[1], ptrs[1], p, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

// ---- grouped 3x3 conv (conv_group.hip, gconv.hpp) ----

namespace {

// The part of the supported set that the weights alone decide; null when inside it.
const char* gconv_shape_error(int32_t C, int32_t groups, int32_t KH, int32_t KW) {
  if (C <= 0 || C % 128) return "grouped conv: C must be a multiple of 128";
  if (groups < 2 || C % groups || !spi::gconv_supported(C, groups))
    return "grouped conv: groups >= 2 with 4, 8, 16, 32 or 64 channels per group";
  if (KH != 3 || KW != 3) return "grouped conv: the kernel is 3x3 with pad 1";
  return nullptr;
}

}  // namespace

size_t spi_op_gconv_packed_bytes(int32_t C, int32_t groups, int32_t KH, int32_t KW) {
  return gconv_shape_error(C, groups, KH, KW) ? 0 : spi::gconv_packed_bytes(C, groups);
}

int spi_op_gconv_pack_weight(const float* w, int32_t C, int32_t groups, int32_t KH, int32_t KW, void* dst) {
  if (!w || !dst) return fail("invalid grouped pack arguments");
  if (const char* e = gconv_shape_error(C, groups, KH, KW)) return fail(e);
  const int cpg = C / groups;
  spi::gconv_pack_into(static_cast<_Float16*>(dst), C, groups,
                       [&](int n, int c, int tap) { return w[((size_t)n * cpg + c) * 9 + tap]; });
  return 0;
}

int spi_op_conv2d_grouped(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, const void* Wp, int32_t groups,
                          int32_t KH, int32_t KW, int32_t stride, int32_t pad, const float* bias, void* y,
                          int32_t act, void* stream) {
  if (!x || !Wp || !y) return fail("grouped conv: null x, W_packed or y");
  if (B <= 0 || H <= 0 || W <= 0) return fail("grouped conv: B, H and W must be positive");
  if (const char* e = gconv_shape_error(C, groups, KH, KW)) return fail(e);
  if (pad != 1) return fail("grouped conv: the kernel is 3x3 with pad 1");
  if (stride != 1 && stride != 2) return fail("grouped conv: stride 1 or 2");
  if (act != 0 && act != 1) return fail("grouped conv: act 0 (none) or 1 (relu)");
  for (const void* p : {x, Wp, static_cast<const void*>(y), static_cast<const void*>(bias)})
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail("grouped conv: 16-byte aligned x, W_packed, y and bias");
  return guarded([&] {
    spi::conv_group(x, Wp, bias, y, B, H, W, C, groups, stride, act == 1, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_avgpool_fc(int32_t precision, const void* x, int32_t B, int32_t HW, int32_t C, const void* W, int32_t N,
                      const float* bias, float* y, int32_t act, void* workspace, void* stream) {
  spi::Prec p;
  if (!prec_of(precision, &p) || !x || !W || !y || !workspace || B <= 0 || HW <= 0 || HW > 64 || C <= 0 ||
      N <= 0 || act < 0 || act > 2)
    return fail("invalid avgpool_fc arguments");
  if (precision == kSplitPrecision && C % 32) return fail("split avgpool_fc needs C a multiple of 32");
  spi::GemmDesc d = spi::dense_desc(B * HW, N, C, C, N, N, 1);
  d.act = static_cast<spi::Act>(act);
  d.out_f32 = true;
  d.pool_rows = HW;
  d.a_split = precision == kSplitPrecision;
  // the plan rule never splits a pooled GEMM, a forced SPI_GEMM_PLAN may: its slabs must fit like any other's
  return run_gemm(d, p, x, W, bias, nullptr, y, {}, workspace, stream, "avgpool_fc too large for the op workspace");
}

size_t spi_op_stem_pool_bytes(void) { return spi::stem_pool_bytes(); }

int spi_op_stem_pool_pack(const float* w, void* dst) {
  if (!w || !dst) return fail("invalid stem_pool pack arguments");
  spi::stem_pool_pack(w, static_cast<_Float16*>(dst));
  return 0;
}

int spi_op_stem_pool(int32_t precision, const float* x, int32_t B, int32_t H, int32_t W, const void* Wp,
                     const float* bias, void* y, int32_t rows_per_block, void* stream) {
  if (precision < 1 || precision > 4 || !x || !Wp || !bias || !y || B <= 0 || H <= 0 || W <= 0 ||
      rows_per_block < 0 || rows_per_block > 2)
    return fail("invalid stem_pool arguments");
  if ((W + 6 - 7) / 2 + 1 > spi::kStemPoolMaxOW) return fail("stem_pool: image wider than 224");
  // stem_pool's lo: 0 fp16 weights, 1 hi + lo weights on the fp16 image (the model's fp16m stem),
  // 2 hi + lo weights on the split image (fp32-grade; fp16x3 and the split output)
  const int lo = precision == 1 ? 0 : precision == 2 ? 1 : 2;
  return guarded([&] {
    spi::stem_pool(x, Wp, bias, y, B, H, W, lo, precision == 3, rows_per_block, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

namespace {

// scale / shift: host fp32 [3] each, both null = the default transform
bool input_xf(const float* scale, const float* shift, spi::InputXf* xf) {
  if (!scale && !shift) return true;
  if (!scale || !shift) return false;
  for (int c = 0; c < 3; ++c) {
    xf->scale[c] = scale[c];
    xf->shift[c] = shift[c];
  }
  return true;
}

}  // namespace

int spi_op_stem_pool_u8(int32_t precision, const uint8_t* x, int32_t nhwc, int32_t B, int32_t H, int32_t W,
                        const void* Wp, const float* bias, const float* scale, const float* shift, void* y,
                        int32_t rows_per_block, void* stream) {
  spi::InputXf xf;
  if (precision < 1 || precision > 4 || !x || !Wp || !bias || !y || B <= 0 || H <= 0 || W <= 0 ||
      rows_per_block < 0 || rows_per_block > 2 || !input_xf(scale, shift, &xf))
    return fail("invalid stem_pool_u8 arguments");
  if ((W + 6 - 7) / 2 + 1 > spi::kStemPoolMaxOW) return fail("stem_pool: image wider than 224");
  const int lo = precision == 1 ? 0 : precision == 2 ? 1 : 2;  // as spi_op_stem_pool
  return guarded([&] {
    spi::stem_pool(x, Wp, bias, y, B, H, W, lo, precision == 3, rows_per_block, static_cast<hipStream_t>(stream),
                   nhwc ? spi::kSrcU8Nhwc : spi::kSrcU8Nchw, xf);
    return check_launch();
  });
}

int spi_op_patchify(int32_t src_kind, const void* x, int32_t B, int32_t H, int32_t W, int32_t ps, const float* scale,
                    const float* shift, void* y, int32_t out_f16, void* stream) {
  spi::InputXf xf;
  if (src_kind < 0 || src_kind > 2 || !x || !y || B <= 0 || H <= 0 || W <= 0 || ps <= 0 || H % ps || W % ps ||
      !input_xf(scale, shift, &xf))
    return fail("invalid patchify arguments");
  return guarded([&] {
    spi::patchify(x, y, B, 3, H, W, ps, out_f16 != 0, static_cast<hipStream_t>(stream), src_kind, xf);
    return check_launch();
  });
}

namespace {

const char* resize_crop_check(const void* x, int32_t B, int32_t H, int32_t W, int32_t R, int32_t S, const void* y) {
  if (!x || !y || B < 1 || B > 65535 || H < 1 || W < 1 || H > spi::kResizeMax || W > spi::kResizeMax || S < 1 ||
      R < S || R > spi::kResizeMax)
    return "invalid resize_crop_u8 arguments: 1 <= H, W <= 8192, 1 <= crop <= resize_short <= 8192, 1 <= B <= 65535";
  const spi::ResizeGeom g = spi::resize_geom(H, W, R, S);
  return g.RH > spi::kResizeMax || g.RW > spi::kResizeMax ? "resize_crop_u8: the resized long side exceeds 8192"
                                                           : nullptr;
}

}  // namespace

int spi_op_resize_crop_u8(const uint8_t* x, int32_t nhwc, int32_t B, int32_t H, int32_t W, int32_t resize_short,
                          int32_t crop, const float* scale, const float* shift, float* y, void* stream) {
  spi::InputXf xf;
  if (const char* bad = resize_crop_check(x, B, H, W, resize_short, crop, y)) return fail(bad);
  if (!input_xf(scale, shift, &xf)) return fail("resize_crop_u8: scale and shift come both or neither");
  return guarded([&] {
    spi::resize_crop_u8(x, nhwc != 0, B, H, W, resize_short, crop, xf, y, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

// The kernel's arithmetic on the CPU: per image, the horizontal samples of every source row the crop's
// rows need (ascending taps, resample.hpp), then the vertical pass over them, then the transform.
int spi_op_resize_crop_u8_host(const uint8_t* x, int32_t nhwc, int32_t B, int32_t H, int32_t W, int32_t resize_short,
                               int32_t crop, const float* scale, const float* shift, float* y, void*) {
  spi::InputXf xf;
  if (const char* bad = resize_crop_check(x, B, H, W, resize_short, crop, y)) return fail(bad);
  if (!input_xf(scale, shift, &xf)) return fail("resize_crop_u8: scale and shift come both or neither");
  return guarded([&] {
    const int S = crop;
    const spi::ResizeGeom g = spi::resize_geom(H, W, resize_short, S);
    const int band0 = spi::axis_taps(g.top, H, g.RH).lo, band1 = spi::axis_taps(g.top + S - 1, H, g.RH).hi;
    std::vector<spi::AxisTaps> cx(S);
    std::vector<float> totx(S), hrows((size_t)(band1 - band0) * 3 * S);
    for (int ox = 0; ox < S; ++ox) {
      cx[ox] = spi::axis_taps(g.left + ox, W, g.RW);
      totx[ox] = spi::tap_total(cx[ox]);
    }
    const size_t plane = (size_t)H * W;
    for (int b = 0; b < B; ++b) {
      const uint8_t* img = x + (size_t)b * plane * 3;
      auto pixel = [&](int c, int r, int j) {
        return static_cast<float>(nhwc ? img[((size_t)r * W + j) * 3 + c] : img[(size_t)c * plane + (size_t)r * W + j]);
      };
      for (int r = band0; r < band1; ++r)
        for (int c = 0; c < 3; ++c)
          for (int ox = 0; ox < S; ++ox) {
            float h = 0.0f;
            for (int j = cx[ox].lo; j < cx[ox].hi; ++j)
              h = spi::tap_acc(spi::tap_norm(spi::tap_weight(cx[ox], j), totx[ox]), pixel(c, r, j), h);
            hrows[((size_t)(r - band0) * 3 + c) * S + ox] = h;
          }
      for (int oy = 0; oy < S; ++oy) {
        const spi::AxisTaps cy = spi::axis_taps(g.top + oy, H, g.RH);
        const float toty = spi::tap_total(cy);
        for (int c = 0; c < 3; ++c)
          for (int ox = 0; ox < S; ++ox) {
            float acc = 0.0f;
            for (int r = cy.lo; r < cy.hi; ++r)
              acc = spi::tap_acc(spi::tap_norm(spi::tap_weight(cy, r), toty), hrows[((size_t)(r - band0) * 3 + c) * S + ox], acc);
            y[(((size_t)b * 3 + c) * S + oy) * S + ox] = spi::resample_xf(acc, xf.scale[c], xf.shift[c]);
          }
      }
    }
    return 0;
  });
}

int spi_op_attention(int32_t precision, const void* qkv, const float* mask_bias, void* ctx, int32_t B, int32_t S,
                     int32_t heads, float scale, void* stream) {
  return spi_op_attention_hd(precision, qkv, mask_bias, ctx, B, S, heads, 64, scale, stream);
}

int spi_op_attention_hd(int32_t precision, const void* qkv, const float* mask_bias, void* ctx, int32_t B, int32_t S,
                        int32_t heads, int32_t head_dim, float scale, void* stream) {
  if ((precision != 0 && precision != 1) || !qkv || !ctx || B <= 0 || S <= 0 || heads <= 0)
    return fail("invalid attention arguments");
  if (head_dim != 32 && head_dim != 64) return fail("attention: head_dim must be 32 or 64");
  if ((int64_t)B * heads > 65535) return fail("attention: B * heads is the grid's y extent, at most 65535");
  // the kernels read q / k / v rows in 16-byte chunks and the fp16 ones store ctx 8 bytes at a time
  if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(ctx) & 7))
    return fail("attention: 16-byte aligned qkv and 8-byte aligned ctx");
  return guarded([&] {
    spi::attention(qkv, mask_bias, ctx, B, S, heads, head_dim, scale, precision == 1, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_layernorm(int32_t precision, const float* x, const float* g, const float* b, float* yf, void* yt,
                     int32_t rows, int32_t D, float eps, void* stream) {
  if (precision < 0 || precision > 2 || !x || !g || !b || rows <= 0 || D <= 0 || D > 1024 || (!yf && !yt))
    return fail("invalid layernorm arguments");
  return guarded([&] {
    spi::layernorm(x, D, g, b, yf, yt, D, rows, D, eps, precision == 1, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_fold_linear(int32_t precision, const float* w, const float* b, int32_t N, int32_t K, const float* gamma,
                       const float* beta, int32_t hilo, float* w_folded, float* bias, float* c1) {
  spi::Prec p;
  if (!prec_of(precision, &p) || !w || !gamma || !beta || !w_folded || !bias || !c1 || N <= 0 || K <= 0)
    return fail("invalid fold_linear arguments");
  if (hilo && p != spi::Prec::F16) return fail("hi/lo weight packing is an fp16 layout");
  spi::fold_linear(w, b, N, K, gamma, beta, p == spi::Prec::F16, hilo != 0, w_folded, bias, c1);
  return 0;
}

namespace {

// spi_op_gemm_ln and its hi + lo weight twin (krep = 2: W packed by spi_op_pack_weight_hilo)
int gemm_ln(int krep, const void* A, int32_t M, int32_t K, int32_t lda, const void* W, int32_t N, const float* bias,
            const float* in_stats, const float* c1, const void* residual, int32_t res_kind, int32_t ldr,
            const float* res_stats, const float* res_g, const float* res_b, float eps, void* C, int32_t out_kind,
            int32_t ldc, size_t plane, float* out_stats, void* c16, int32_t ld16, int32_t act, void* workspace,
            void* stream) {
  if (!A || !W || !C || !workspace || M <= 0 || N <= 0 || K <= 0 || lda < K || ldc < N || act < 0 || act > 2 ||
      out_kind < SPI_KIND_F16 || out_kind > SPI_KIND_PLANES ||
      (residual ? res_kind < SPI_KIND_F16 || res_kind > SPI_KIND_PLANES || ldr < N : res_kind != SPI_KIND_NONE))
    return fail("invalid gemm_ln arguments");
  const bool consumer = in_stats || c1, res_ln = res_stats || res_g || res_b, producer = out_stats || c16;
  if ((consumer && K % 64) || ((res_ln || producer) && N % 64))
    return fail("gemm_ln: the LayerNorm fold works on whole 64-column chunks");
  spi::GemmDesc d = spi::dense_desc(M, N, K, lda, ldc, ldr, krep);
  d.wplane = (size_t)spi::round_up_to(N, 128) * d.Kpad;
  d.act = static_cast<spi::Act>(act);
  d.out_f32 = out_kind == SPI_KIND_F32;
  d.res_f32 = res_kind == SPI_KIND_F32;
  d.out_planes = out_kind == SPI_KIND_PLANES;
  d.res_planes = res_kind == SPI_KIND_PLANES;
  d.plane = plane;
  spi::LnPtrs lp;
  if (consumer) {
    d.ln_in_chunks = K / 64;
    d.ln_in_eps = eps;
    lp.in_stats = in_stats;
    lp.c1 = c1;
  }
  if (res_ln) {
    d.res_ln_chunks = N / 64;
    d.res_ln_eps = eps;
    lp.res_stats = res_stats;
    lp.res_g = res_g;
    lp.res_b = res_b;
  }
  if (producer) {
    d.ln_out = true;
    d.ld16 = ld16;
    lp.out_stats = out_stats;
    lp.c16 = static_cast<_Float16*>(c16);
  }
  return run_gemm(d, spi::Prec::F16, A, W, bias, residual, C, lp, workspace, stream,
                  "gemm too large for the op workspace");
}

}  // namespace

int spi_op_gemm_ln(const void* A, int32_t M, int32_t K, int32_t lda, const void* W, int32_t N, const float* bias,
                   const float* in_stats, const float* c1, const void* residual, int32_t res_kind, int32_t ldr,
                   const float* res_stats, const float* res_g, const float* res_b, float eps, void* C,
                   int32_t out_kind, int32_t ldc, size_t plane, float* out_stats, void* c16, int32_t ld16,
                   int32_t act, void* workspace, void* stream) {
  return gemm_ln(1, A, M, K, lda, W, N, bias, in_stats, c1, residual, res_kind, ldr, res_stats, res_g, res_b, eps, C,
                 out_kind, ldc, plane, out_stats, c16, ld16, act, workspace, stream);
}

int spi_op_gemm_ln_hilo(const void* A, int32_t M, int32_t K, int32_t lda, const void* W, int32_t N, const float* bias,
                        const float* in_stats, const float* c1, const void* residual, int32_t res_kind, int32_t ldr,
                        const float* res_stats, const float* res_g, const float* res_b, float eps, void* C,
                        int32_t out_kind, int32_t ldc, size_t plane, float* out_stats, void* c16, int32_t ld16,
                        int32_t act, void* workspace, void* stream) {
  return gemm_ln(2, A, M, K, lda, W, N, bias, in_stats, c1, residual, res_kind, ldr, res_stats, res_g, res_b, eps, C,
                 out_kind, ldc, plane, out_stats, c16, ld16, act, workspace, stream);
}

int spi_op_layernorm_planes(int32_t precision, const void* xh, size_t plane, int32_t ldx, const float* g,
                            const float* b, float* yf, void* yt, int32_t ldy, int32_t rows, int32_t D, float eps,
                            void* stream) {
  if (precision < 0 || precision > 1 || !xh || !g || !b || rows <= 0 || D <= 0 || ldx < D || ldy < D || (!yf && !yt))
    return fail("invalid layernorm_planes arguments");
  return guarded([&] {
    spi::layernorm_planes(static_cast<const _Float16*>(xh), plane, ldx, g, b, yf, yt, ldy, rows, D, eps,
                          precision == 1, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_vit_assemble_planes(const float* patches, const float* cls, const float* pos, void* xh, size_t plane,
                               float* stats, int32_t B, int32_t P, int32_t D, void* stream) {
  if (!patches || !cls || !pos || !xh || B <= 0 || P <= 0 || D <= 0)
    return fail("invalid vit_assemble_planes arguments");
  return guarded([&] {
    spi::vit_assemble_planes(patches, cls, pos, static_cast<_Float16*>(xh), plane, stats, B, P, D,
                             static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_qkv_attention(const void* A, int32_t lda, const void* W, int32_t heads, const float* bias,
                         const float* in_stats, const float* c1, float eps, const float* mask_bias, void* ctx,
                         int32_t B, int32_t S, float scale, void* stream) {
  if (!A || !W || !bias || !ctx || B <= 0 || heads <= 0 || heads > (1 << 20))
    return fail("invalid qkv_attention arguments");
  if ((in_stats == nullptr) != (c1 == nullptr)) return fail("qkv_attention: in_stats and c1 come both or neither");
  const int D = heads * 64;  // the packed Kpad too: D is a multiple of 64
  if (lda < D || !spi::qkv_attention_eligible(S, heads, 64, D, D, 1, lda, D))
    return fail("qkv_attention: 1 <= S <= 256, heads >= 2, lda >= D and a multiple of 8");
  if (in_stats && D > 1024) return fail("qkv_attention: the fold holds at most 16 statistics chunks (D <= 1024)");
  if ((reinterpret_cast<uintptr_t>(ctx) & 7) || (reinterpret_cast<uintptr_t>(in_stats) & 7))
    return fail("qkv_attention: 8-byte aligned ctx and in_stats");
  return guarded([&] {
    spi::qkv_attention(A, lda, W, D, bias, in_stats, c1, D / 64, eps, mask_bias, ctx, B, S, heads, scale,
                       static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_ingest(int32_t src_kind, const void* x, int32_t B, int32_t Cc, int32_t H, int32_t W, int32_t cpad,
                  const float* scale, const float* shift, void* y, int32_t out_f16, void* stream) {
  spi::InputXf xf;
  if (src_kind < 0 || src_kind > 2 || !x || !y || B <= 0 || Cc <= 0 || H <= 0 || W <= 0 || Cc > cpad ||
      (src_kind != 0 && Cc != 3) || !input_xf(scale, shift, &xf))
    return fail("invalid ingest arguments");
  return guarded([&] {
    spi::ingest_nchw(x, y, B, Cc, H, W, cpad, out_f16 != 0, static_cast<hipStream_t>(stream), src_kind, xf);
    return check_launch();
  });
}

namespace {

// 16-byte channel vectors of the pooling kernels: 4 fp32, 8 fp16, a 32-channel block of the split layout
int pool_vec(int32_t precision) { return precision == 0 ? 4 : precision == 1 ? 8 : precision == kSplitPrecision ? 32 : 0; }

}  // namespace

int spi_op_maxpool(int32_t precision, const void* x, int32_t B, int32_t H, int32_t W, int32_t Cc, int32_t k,
                   int32_t stride, int32_t pad, void* y, void* stream) {
  const int vec = pool_vec(precision);
  if (!vec || !x || !y || B <= 0 || H <= 0 || W <= 0 || Cc <= 0 || k <= 0 || stride <= 0 || pad < 0 || pad >= k)
    return fail("invalid maxpool arguments");
  if (Cc % vec) return fail("maxpool: C must be a multiple of 4 (fp32), 8 (fp16) or 32 (split)");
  if (!spi::aligned(x, 16) || !spi::aligned(y, 16)) return fail("maxpool: 16-byte aligned x and y");
  if (H + 2 * pad < k || W + 2 * pad < k) return fail("empty maxpool output");
  const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
  return guarded([&] {
    if (precision == kSplitPrecision)
      spi::maxpool_nhwc_split(x, y, B, H, W, Cc, OH, OW, k, stride, pad, static_cast<hipStream_t>(stream));
    else
      spi::maxpool_nhwc(x, y, B, H, W, Cc, OH, OW, k, stride, pad, precision == 1, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_avgpool(int32_t precision, const void* x, int32_t B, int32_t HW, int32_t Cc, void* y, int32_t out_f32,
                   void* stream) {
  const int vec = pool_vec(precision);
  if (!vec || !x || !y || B <= 0 || HW <= 0 || Cc <= 0) return fail("invalid avgpool arguments");
  if (Cc % vec) return fail("avgpool: C must be a multiple of 4 (fp32), 8 (fp16) or 32 (split)");
  if (!spi::aligned(x, 16) || !spi::aligned(y, 16)) return fail("avgpool: 16-byte aligned x and y");
  return guarded([&] {
    if (precision == kSplitPrecision)
      spi::avgpool_nhwc_split(x, static_cast<float*>(y), B, HW, Cc, static_cast<hipStream_t>(stream));
    else
      spi::avgpool_nhwc(x, y, B, HW, Cc, precision == 1, static_cast<hipStream_t>(stream),
                        precision == 1 && out_f32 != 0);
    return check_launch();
  });
}

int spi_op_bert_embed(int32_t precision, const int64_t* ids, const float* word, const float* pos, const float* type0,
                      const float* g, const float* b, float* yf, void* yt, int32_t B, int32_t S, int32_t D,
                      int32_t vocab, int32_t npos, float eps, const int64_t* mask, float* mask_bias, void* stream) {
  if ((precision != 0 && precision != 1) || !ids || !word || !pos || !type0 || !g || !b || B <= 0 || S <= 0 ||
      D <= 0 || vocab <= 0 || npos <= 0)
    return fail("invalid bert_embed arguments");
  if (!yf) return fail("bert_embed: the fp32 output yf is required");
  if (D > 1024) return fail("bert_embed: D <= 1024");
  if (S > npos) return fail("bert_embed: S exceeds the position table");
  if ((mask == nullptr) != (mask_bias == nullptr)) return fail("bert_embed: mask and mask_bias come both or neither");
  return guarded([&] {
    spi::bert_embed(ids, word, pos, type0, g, b, yf, yt, B, S, D, vocab, eps, precision == 1,
                    static_cast<hipStream_t>(stream), mask, mask_bias);
    return check_launch();
  });
}

int spi_op_bert_embed_types(int32_t precision, const int64_t* ids, const float* word, const float* pos,
                            const float* type_table, int32_t type_vocab, const int64_t* type_ids, const float* g,
                            const float* b, float* yf, void* yt, int32_t B, int32_t S, int32_t D, int32_t vocab,
                            int32_t npos, float eps, const int64_t* mask, float* mask_bias, void* stream) {
  if ((precision != 0 && precision != 1) || !ids || !word || !pos || !type_table || !g || !b || B <= 0 || S <= 0 ||
      D <= 0 || vocab <= 0 || npos <= 0 || type_vocab <= 0)
    return fail("invalid bert_embed_types arguments");
  if (!yf) return fail("bert_embed_types: the fp32 output yf is required");
  if (D > 1024) return fail("bert_embed_types: D <= 1024");
  if (S > npos) return fail("bert_embed_types: S exceeds the position table");
  if ((mask == nullptr) != (mask_bias == nullptr))
    return fail("bert_embed_types: mask and mask_bias come both or neither");
  return guarded([&] {
    spi::bert_embed(ids, word, pos, type_table, g, b, yf, yt, B, S, D, vocab, eps, precision == 1,
                    static_cast<hipStream_t>(stream), mask, mask_bias, type_ids, type_vocab);
    return check_launch();
  });
}

int spi_op_bert_embed_posids(int32_t precision, const int64_t* ids, const float* word, const float* pos,
                             const float* type_table, int32_t type_vocab, const int64_t* type_ids, const float* g,
                             const float* b, float* yf, void* yt, int32_t B, int32_t S, int32_t D, int32_t vocab,
                             int32_t npos, float eps, const int64_t* mask, float* mask_bias, void* stream) {
  if ((precision != 0 && precision != 1) || !ids || !word || !pos || !type_table || !g || !b || B <= 0 || S <= 0 ||
      D <= 0 || vocab <= 0 || npos <= 0 || type_vocab <= 0)
    return fail("invalid bert_embed_posids arguments");
  if (!yf) return fail("bert_embed_posids: the fp32 output yf is required");
  if (D > 1024) return fail("bert_embed_posids: D <= 1024");
  if ((int64_t)S + 2 > npos) return fail("bert_embed_posids: S + 2 exceeds the position table");
  if ((mask == nullptr) != (mask_bias == nullptr))
    return fail("bert_embed_posids: mask and mask_bias come both or neither");
  return guarded([&] {
    spi::bert_embed(ids, word, pos, type_table, g, b, yf, yt, B, S, D, vocab, eps, precision == 1,
                    static_cast<hipStream_t>(stream), mask, mask_bias, type_ids, type_vocab, true);
    return check_launch();
  });
}

int spi_op_bert_pooler(const float* h, int64_t ld, const float* W, const float* bias, float* y, int32_t B, int32_t D,
                       void* stream) {
  if (!h || !W || !bias || !y || B <= 0 || D <= 0 || ld < D) return fail("invalid bert_pooler arguments");
  return guarded([&] {
    spi::bert_pooler(h, (size_t)ld, W, bias, y, B, D, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_masked_mean(const float* h, const int64_t* mask, float* y, int32_t B, int32_t S, int32_t D, void* stream) {
  if (!h || !y || B <= 0 || S <= 0 || D <= 0) return fail("invalid masked_mean arguments");
  return guarded([&] {
    spi::masked_mean(h, mask, y, B, S, D, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_bert_token_head(int32_t src, const void* x, int64_t plane, const float* g, const float* b, float eps,
                           const float* W, const float* bias, float* y0, float* y1, int32_t T, int32_t D, int32_t L,
                           void* stream) {
  if (!x || !W || !bias || !y0 || T <= 0 || D <= 0 || L <= 0 || plane < 0)
    return fail("invalid bert_token_head arguments");
  return guarded([&] {
    spi::bert_token_head(src, x, (size_t)plane, g, b, eps, W, bias, y0, y1, T, D, L, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_bert_dense_rows(const float* h, int64_t ld, const float* W, const float* bias, float* y, int32_t B,
                           int32_t D, int32_t N, int32_t activation, void* stream) {
  if (!h || !W || !bias || !y || B <= 0 || D <= 0 || N <= 0 || ld < D || (activation != 0 && activation != 1))
    return fail("invalid bert_dense_rows arguments");
  return guarded([&] {
    spi::bert_dense_rows(h, (size_t)ld, W, bias, y, B, D, N, activation == 1, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_softmax_topk(const float* x, int64_t ldx, float* probs, float* topv, int64_t* topi, int32_t B, int32_t N,
                        int32_t k, int32_t topk_probs, void* stream) {
  if (!x) return fail("softmax_topk: x is null");
  if (!probs && !topv && !topi) return fail("softmax_topk: no output selected");
  if ((topv == nullptr) != (topi == nullptr))
    return fail("softmax_topk: top-k values and indices come both or neither");
  if (B < 1) return fail("softmax_topk: B >= 1");
  if (N < 1 || N > spi::kSoftmaxTopkMaxN) return fail("softmax_topk: 1 <= N <= 16384");
  if (ldx < N) return fail("softmax_topk: ldx >= N");
  if (topv && (k < 1 || k > spi::kSoftmaxTopkMaxK || k > N)) return fail("softmax_topk: 1 <= k <= min(N, 64)");
  if (!topv && (k != 0 || topk_probs != 0)) return fail("softmax_topk: k and topk_probs need the top-k outputs");
  return guarded([&] {
    spi::softmax_topk(x, (size_t)ldx, probs, topv, topi, B, N, k, topk_probs != 0, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_mask_to_bias(const int64_t* mask, float* bias, int32_t n, void* stream) {
  if (!mask || !bias || n <= 0) return fail("invalid mask_to_bias arguments");
  return guarded([&] {
    spi::mask_to_bias(mask, bias, n, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_vit_assemble(const float* patches, const float* cls, const float* pos, float* x, int32_t B, int32_t P,
                        int32_t D, void* stream) {
  if (!patches || !cls || !pos || !x || B <= 0 || P <= 0 || D <= 0) return fail("invalid vit_assemble arguments");
  return guarded([&] {
    spi::vit_assemble(patches, cls, pos, x, B, P, D, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

int spi_op_gather_rows(const float* x, void* y, int32_t rows, int32_t stride_rows, int32_t D, int32_t out_f16,
                       void* stream) {
  if (!x || !y || rows <= 0 || stride_rows <= 0 || D <= 0) return fail("invalid gather_rows arguments");
  return guarded([&] {
    spi::gather_rows(x, y, rows, stride_rows, D, out_f16 != 0, static_cast<hipStream_t>(stream));
    return check_launch();
  });
}

}  // extern "C"
