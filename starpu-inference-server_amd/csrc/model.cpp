// Model replica: upload of the packed blob (model_pack.cpp); per-stream workspaces; launch
// helpers; forward plans for ResNet (basic / bottleneck), BERT (post-LN) and ViT (pre-LN).
// Reference counterparts: the per-device clones (src/core/inference_runner.cpp:251-275) and the
// forward that LibTorch runs inside the codelet (src/core/starpu_setup.cpp:610).
#include "gconv.hpp"
#include "gemm_plan.hpp"
#include "model.hpp"
#include "resample.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace spi {

constexpr size_t kCounterSlots = 16384;  // >= tiles of any split GEMM (checked per launch)

// Graph capture vs allocation: a hipMalloc on one worker thread while another
// thread's stream is capturing invalidates that capture ("operation failed due
// to a previous error during capture").  Workspace allocation and graph capture
// therefore never overlap, process-wide (all replicas, all worker threads).
std::mutex g_capture_mu;

// Workspace buffers of each family, in allocation order.
// ResNet: the padded NHWC image (unfused stem only); five activation slots the blocks rotate through
// (0: the unfused stem's output, 1: the max pool's output = the first block's input); the
// average-pooled features (when avgpool + FC do not run as one GEMM).
// The logits scratch (here and for ViT): fp32 [max_batch][classes] under SPI_IMAGE_NO_LOGITS, else empty.
// The resampled image (here and for ViT): fp32 NCHW [max_batch][3][image][image] with the input resize on, else empty.
enum RnBuf { kRnIngest, kRnAct0, kRnAct1, kRnAct2, kRnAct3, kRnAct4, kRnPooled, kRnLogits, kRnResized, kRnBufs };
// BERT: hidden rows fp32 (fold: the pre-LN2 rows b as two fp16 planes) and their compute-type copy;
// qkv; ctx; the attention block's output a, fp32 (fold: the pre-LN1 rows as two planes); the FFN
// hidden rows; the LayerNorm-fold row statistics S1 (of a) and S2 (of b); the final LayerNorm's
// class-token rows, fp32 (SPI_BERT_NO_HIDDEN with the pooler alone).
enum BertBuf { kBtHidden, kBtHidden16, kBtQkv, kBtCtx, kBtAttn, kBtFfn, kBtStats1, kBtStats2, kBtCls, kBtBufs };
// ViT: patches; projected patches f32; residual stream x f32 (fold: two fp16 planes); LN output; qkv;
// ctx; mlp hidden; the LayerNorm'd class-token rows; the LayerNorm-fold row statistics of x.
enum VitBuf { kVtPatches, kVtProj, kVtX, kVtLn, kVtQkv, kVtCtx, kVtMlp, kVtCls, kVtStats, kVtLogits, kVtResized, kVtBufs };

// ---------------------------------------------------------------------------
// Workspace: activation buffers for one stream at max_batch.
// ---------------------------------------------------------------------------
struct Workspace {
  std::vector<void*> bufs;
  float* partial = nullptr;
  float* mask_bias = nullptr;
  size_t partial_floats = 0;
  int* counters = nullptr;  // split-K tickets (zeroed once; the reducer re-zeroes its slot)
  bool has_mask = false;
  const int64_t* mask_ids = nullptr;  // BERT: the task's attention_mask (the prologue's; read by the mean pool)
  int final_buf = kRnPooled;  // ResNet: buffer holding the last stage's output
  int final_hw = 0;           // ... and its pixels per image (avgpool window)
  std::map<int, hipGraphExec_t> graphs;
  ~Workspace() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    for (void* b : bufs) (void)hipFree(b);
    if (partial) (void)hipFree(partial);
    if (mask_bias) (void)hipFree(mask_bias);
    if (counters) (void)hipFree(counters);
  }
};

// ---------------------------------------------------------------------------
// Construction
// ---------------------------------------------------------------------------
Model::Model(int device, const spi_model_config& cfg, const spi_named_tensor* params, int n)
    : device_(device), m_(pack_model(cfg, params, n)) {
  if (const char* e = std::getenv("SPI_QKV_ATTN"); e && *e) qkv_fused_ = std::atoi(e);
  std::vector<char> blob = std::move(m_.blob);  // not kept on the host, also for a host-only replica
  m_.blob = {};
  if (device_ < 0) return;  // host-only replica: recognised and packed, never uploaded
  SPI_HIP(hipSetDevice(device_));
  if (m_.blob_bytes) {
    SPI_HIP(hipMalloc(&dblob_, m_.blob_bytes));
    SPI_HIP(hipMemcpy(dblob_, blob.data(), m_.blob_bytes, hipMemcpyHostToDevice));
  }
}

Model::~Model() {
  ws_.clear();
  if (dblob_) (void)hipFree(dblob_);
}

// ---------------------------------------------------------------------------
// I/O contract
// ---------------------------------------------------------------------------
void Model::check_io(const spi_codelet_args& a, const size_t* in_bytes, const size_t* out_bytes) const {
  const int ni = (int)a.num_inputs, no = (int)a.num_outputs, image = m_.image;
  if (ni < 1 || ni > num_inputs_max())
    throw std::runtime_error("model expects " + std::to_string(num_inputs_max()) + " input(s), got " +
                             std::to_string(ni));
  if (no != num_outputs()) throw std::runtime_error("Mismatch between model outputs and StarPU buffers");
  const int64_t B = a.dims[0][0];
  if (B < 1 || B > m_.max_batch)
    throw std::runtime_error("batch " + std::to_string(B) + " exceeds replica max_batch " +
                             std::to_string(m_.max_batch));
  auto elems = [&](int i) {
    int64_t e = 1;
    for (int d = 0; d < a.num_dims[i]; ++d) e *= a.dims[i][d];
    return e;
  };
  size_t expect_out = 0;
  size_t expect_more[3] = {0, 0, 0};  // the outputs after the first (BERT: bert_io; ResNet / ViT: image_io_)
  int i64_out = -1;                   // the output that is SPI_DTYPE_I64 (the top-k indices), if any
  if (m_.family == SPI_FAMILY_AFFINE) {
    if (a.input_types[0] != SPI_DTYPE_F32) throw std::runtime_error("[ERROR] Input type mismatch");
    if (in_bytes[0] < (size_t)elems(0) * 4) throw std::runtime_error("[ERROR] Input buffer too small");
    expect_out = (size_t)elems(0) * 4;
  } else if (m_.family == SPI_FAMILY_RESNET || m_.family == SPI_FAMILY_VIT) {
    const bool u8 = a.input_types[0] == SPI_DTYPE_U8;
    if (!u8 && a.input_types[0] != SPI_DTYPE_F32) throw std::runtime_error("[ERROR] Input type mismatch");
    const std::string sz = std::to_string(image);
    if (u8 && resize_short_) {
      // the input resize: a source of any size in either layout; dims[1] == 3 is NCHW, also when dims[3] == 3
      const int64_t* d = a.dims[0];
      const bool nchw = a.num_dims[0] == 4 && d[1] == 3, nhwc = a.num_dims[0] == 4 && !nchw && d[3] == 3;
      const int64_t H = nchw ? d[2] : d[1], W = nchw ? d[3] : d[2];
      if ((!nchw && !nhwc) || H < 1 || W < 1 || H > kResizeMax || W > kResizeMax)
        throw std::runtime_error("[ERROR] Tensor layout mismatch: expected [B,3,H,W] or [B,H,W,3] with 1 <= H, W <= " +
                                 std::to_string(kResizeMax) + " (input resize " + std::to_string(resize_short_) + ")");
      const ResizeGeom g = resize_geom((int)H, (int)W, resize_short_, image);
      if (std::max(g.RH, g.RW) > kResizeMax)
        throw std::runtime_error("[ERROR] Input resize: a " + std::to_string(H) + "x" + std::to_string(W) +
                                 " source resized to short side " + std::to_string(resize_short_) + " has long side " +
                                 std::to_string(std::max(g.RH, g.RW)) + ", above " + std::to_string(kResizeMax));
    } else {
      const bool nchw = a.num_dims[0] == 4 && a.dims[0][1] == 3 && a.dims[0][2] == image && a.dims[0][3] == image;
      const bool nhwc = a.num_dims[0] == 4 && a.dims[0][1] == image && a.dims[0][2] == image && a.dims[0][3] == 3;
      if (!nchw && !(u8 && nhwc))
        throw std::runtime_error("[ERROR] Tensor layout mismatch: expected [B,3," + sz + "," + sz + "]" +
                                 (u8 ? " or [B," + sz + "," + sz + ",3]" : ""));
    }
    if (in_bytes[0] < (size_t)elems(0) * (u8 ? 1 : 4)) throw std::runtime_error("[ERROR] Input buffer too small");
    expect_out = (size_t)B * m_.classes * 4;
    if (image_io_) {  // logits (unless NO_LOGITS), probabilities, top-k values, top-k indices
      size_t want[4];
      int n = 0;
      if (!(image_io_ & SPI_IMAGE_NO_LOGITS)) want[n++] = expect_out;
      if (image_io_ & SPI_IMAGE_OUT_PROBS) want[n++] = expect_out;
      if (image_io_ & SPI_IMAGE_OUT_TOPK) {
        want[n++] = (size_t)B * top_k_ * 4;
        i64_out = n;
        want[n++] = (size_t)B * top_k_ * 8;
      }
      expect_out = want[0];
      for (int i = 1; i < n; ++i) expect_more[i - 1] = want[i];
    }
  } else {  // BERT: input_ids [B,S] int64, optional attention_mask and (bert_io) token_type_ids, [B,S] int64
    for (int i = 0; i < ni; ++i) {
      if (a.input_types[i] != SPI_DTYPE_I64) throw std::runtime_error("[ERROR] Input type mismatch");
      if (a.num_dims[i] != 2 || a.dims[i][0] != B || a.dims[i][1] != a.dims[0][1])
        throw std::runtime_error("[ERROR] Tensor layout mismatch");
      if (in_bytes[i] < (size_t)elems(i) * 8) throw std::runtime_error("[ERROR] Input buffer too small");
    }
    const int64_t S = a.dims[0][1];
    if (S < 1 || S > m_.seq || S > m_.maxpos)
      throw std::runtime_error("sequence length " + std::to_string(S) + " exceeds " + std::to_string(m_.seq));
    // hidden [B,S,D] unless SPI_BERT_NO_HIDDEN, then the selected [B,D] sentence outputs
    expect_out = (m_.bert_io & SPI_BERT_NO_HIDDEN) ? (size_t)B * m_.D * 4 : (size_t)B * S * m_.D * 4;
    expect_more[0] = expect_more[1] = (size_t)B * m_.D * 4;
  }
  for (int i = 0; i < no; ++i) {
    if (a.output_types[i] != (i == i64_out ? SPI_DTYPE_I64 : SPI_DTYPE_F32))
      throw std::runtime_error("[ERROR] Output type mismatch");
    if (out_bytes[i] != (i == 0 ? expect_out : expect_more[i - 1]))
      throw std::runtime_error("Output buffer size mismatch in bytes");
  }
}

ImageSrc Model::input_kind(const spi_codelet_args& a) const {
  ImageSrc src;
  if ((m_.family != SPI_FAMILY_RESNET && m_.family != SPI_FAMILY_VIT) || a.input_types[0] != SPI_DTYPE_U8) return src;
  const int64_t* d = a.dims[0];
  if (resize_short_) {  // every 8-bit task is resampled, an S x S one too: [B,3,H,W] is NCHW, else [B,H,W,3]
    const bool nchw = d[1] == 3;
    src.kind = nchw ? kSrcU8Nchw : kSrcU8Nhwc;
    src.H = (int)(nchw ? d[2] : d[1]);
    src.W = (int)(nchw ? d[3] : d[2]);
    return src;
  }
  // [B,3,S,S] is NCHW (also when S == 3), else check_io accepted [B,S,S,3]
  src.kind = d[1] == 3 && d[2] == m_.image && d[3] == m_.image ? kSrcU8Nchw : kSrcU8Nhwc;
  return src;
}

int Model::set_input_transform(const float* scale, const float* shift) {
  if (m_.family != SPI_FAMILY_RESNET && m_.family != SPI_FAMILY_VIT) return SPI_ERR_UNSUPPORTED;
  InputXf xf;
  if (scale || shift) {
    if (!scale || !shift) return SPI_ERR_INVALID_ARGUMENT;
    for (int c = 0; c < 3; ++c) {
      if (!std::isfinite(scale[c]) || !std::isfinite(shift[c])) return SPI_ERR_INVALID_ARGUMENT;
      xf.scale[c] = scale[c];
      xf.shift[c] = shift[c];
    }
  }
  input_xf_ = xf;
  return SPI_OK;
}

int Model::set_image_outputs(int io, int top_k, std::string& err) {
  constexpr int known = SPI_IMAGE_OUT_PROBS | SPI_IMAGE_OUT_TOPK | SPI_IMAGE_NO_LOGITS | SPI_IMAGE_TOPK_PROBS;
  auto refuse = [&](int status, const std::string& msg) {
    err = "image outputs: " + msg;
    return status;
  };
  if (m_.family != SPI_FAMILY_RESNET && m_.family != SPI_FAMILY_VIT)
    return refuse(SPI_ERR_UNSUPPORTED, "only ResNet / ViT replicas have classification outputs");
  if (io & ~known) return refuse(SPI_ERR_INVALID_ARGUMENT, "unknown bits " + std::to_string(io & ~known));
  if ((io & SPI_IMAGE_NO_LOGITS) && !(io & (SPI_IMAGE_OUT_PROBS | SPI_IMAGE_OUT_TOPK)))
    return refuse(SPI_ERR_INVALID_ARGUMENT,
                  "SPI_IMAGE_NO_LOGITS leaves no output; select SPI_IMAGE_OUT_PROBS or SPI_IMAGE_OUT_TOPK");
  if ((io & SPI_IMAGE_TOPK_PROBS) && !(io & SPI_IMAGE_OUT_TOPK))
    return refuse(SPI_ERR_INVALID_ARGUMENT, "SPI_IMAGE_TOPK_PROBS needs SPI_IMAGE_OUT_TOPK");
  if (io & SPI_IMAGE_OUT_TOPK) {
    const int kmax = std::min(m_.classes, kSoftmaxTopkMaxK);
    if (top_k < 1 || top_k > kmax)
      return refuse(SPI_ERR_INVALID_ARGUMENT,
                    "top_k " + std::to_string(top_k) + " outside 1 .. min(classes, 64) = " + std::to_string(kmax));
  } else if (top_k != 0) {
    return refuse(SPI_ERR_INVALID_ARGUMENT, "top_k " + std::to_string(top_k) + " without SPI_IMAGE_OUT_TOPK");
  }
  if (io && m_.classes > kSoftmaxTopkMaxN)
    return refuse(SPI_ERR_UNSUPPORTED, std::to_string(m_.classes) + " classes; at most " +
                                           std::to_string(kSoftmaxTopkMaxN) + " (the row is staged in LDS as fp32)");
  std::lock_guard<std::mutex> lk(mu_);
  if (!ws_.empty())
    return refuse(SPI_ERR_INVALID_ARGUMENT,
                  "a stream workspace of the replica exists; call before the first forward or warm-up");
  image_io_ = io;
  top_k_ = top_k;
  rebuild_desc();
  return SPI_OK;
}

int Model::set_input_resize(int resize_short, std::string& err) {
  auto refuse = [&](int status, const std::string& msg) {
    err = "input resize: " + msg;
    return status;
  };
  if (m_.family != SPI_FAMILY_RESNET && m_.family != SPI_FAMILY_VIT)
    return refuse(SPI_ERR_UNSUPPORTED, "only ResNet / ViT replicas take 8-bit image tasks");
  if (resize_short != 0 && (resize_short < m_.image || resize_short > kResizeMax))
    return refuse(SPI_ERR_INVALID_ARGUMENT, "resize_short " + std::to_string(resize_short) + " outside " +
                                                std::to_string(m_.image) + " (the replica's image size) .. " +
                                                std::to_string(kResizeMax) + "; 0 switches the resize off");
  std::lock_guard<std::mutex> lk(mu_);
  if (!ws_.empty())
    return refuse(SPI_ERR_INVALID_ARGUMENT,
                  "a stream workspace of the replica exists; call before the first forward or warm-up");
  resize_short_ = resize_short;
  rebuild_desc();
  return SPI_OK;
}

void Model::rebuild_desc() {
  desc_ext_ = m_.desc;
  if (const int io = image_io_) {
    std::string outs;
    for (const auto& o : {std::make_pair(!(io & SPI_IMAGE_NO_LOGITS), std::string("logits")),
                          std::make_pair((io & SPI_IMAGE_OUT_PROBS) != 0, std::string("probs")),
                          std::make_pair((io & SPI_IMAGE_OUT_TOPK) != 0, "top" + std::to_string(top_k_))})
      if (o.first) outs += (outs.empty() ? "" : ",") + o.second;
    desc_ext_ += " out[" + outs + "]";
  }
  if (resize_short_) desc_ext_ += " resize" + std::to_string(resize_short_);
}

double Model::flops(int64_t B) const {
  double f = 0;
  auto conv_f = [&](const ConvW& c, int OH, int OW) {  // a grouped conv: its own FLOPs on either route
    return 2.0 * B * OH * OW * c.cout * (double)c.kh * c.kw * (c.cin / c.groups);
  };
  if (m_.family == SPI_FAMILY_RESNET) {
    int H = (m_.image + 2 * 3 - 7) / 2 + 1;
    f += conv_f(m_.stem, H, H);
    H = (H + 2 - 3) / 2 + 1;
    for (const auto& b : m_.blocks) {
      const ConvW& st = m_.bottleneck ? b.c2 : b.c1;  // the block's strided conv
      const int H2 = (H + 2 * st.pad - st.kh) / st.stride + 1;
      f += conv_f(b.c1, m_.bottleneck ? H : H2, m_.bottleneck ? H : H2) + conv_f(b.c2, H2, H2);
      if (m_.bottleneck) f += conv_f(b.c3, H2, H2);
      if (b.has_ds) f += conv_f(b.ds, H2, H2);
      H = H2;
    }
    f += 2.0 * B * m_.fc.n * m_.fc.k;
  } else if (m_.family == SPI_FAMILY_BERT || m_.family == SPI_FAMILY_VIT) {
    const double S = m_.family == SPI_FAMILY_BERT ? m_.seq : m_.npatch + 1;
    const double T = B * S;
    for (const auto& L : m_.tf)
      f += 2.0 * T * ((double)L.qkv.n * L.qkv.k + (double)L.out.n * L.out.k + (double)L.ff1.n * L.ff1.k +
                      (double)L.ff2.n * L.ff2.k) +
           4.0 * B * S * S * m_.D;
    if (m_.family == SPI_FAMILY_VIT)
      f += 2.0 * B * m_.npatch * (double)m_.D * m_.patch_proj.k + 2.0 * B * m_.head.n * m_.head.k;
    if (m_.bert_io & SPI_BERT_OUT_POOLER) f += 2.0 * B * (double)m_.D * m_.D;
  }
  return f;
}

// ---------------------------------------------------------------------------
// Launch helpers
// ---------------------------------------------------------------------------
namespace {
// A layer's desc: the shared builders (gemm_desc.hpp) on the packed layer's sizes.  The packer
// (model_pack.cpp) sized the W rows; a row length the builder does not arrive at is a packing bug.
GemmDesc conv_desc(const ConvW& c, int B, int H, int W, int& OH, int& OW) {
  GemmDesc d = spi::conv_desc(B, H, W, c.cin_pad, c.cout, c.kh, c.kw, c.stride, c.pad, c.krep);
  if (d.Kpad != c.kpad) throw std::logic_error("conv_desc: the packed weight rows are not Kpad long");
  OH = d.OH, OW = d.OW;
  d.w_image = c.w_image;
  return d;
}

GemmDesc linear_desc(const LinearW& L, int M, int lda, int ldc) {
  const GemmDesc d = dense_desc(M, L.n, L.k, lda, ldc, ldc, L.krep);
  if (d.Kpad != L.kpad) throw std::logic_error("linear_desc: the packed weight rows are not Kpad long");
  return d;
}

std::string conv_name(const ConvW& c, int M) {
  return "conv" + std::to_string(c.kh) + "x" + std::to_string(c.kw) + "_c" + std::to_string(c.cin) + "_k" +
         std::to_string(c.cout) + "_s" + std::to_string(c.stride) + "_M" + std::to_string(M);
}

void require_fit(const GemmDesc& d, Prec prec, const Workspace& ws, const GemmDesc* d1 = nullptr) {
  if (!gemm_workspace_fits(d, prec, ws.partial_floats, kCounterSlots, d1))
    throw std::runtime_error("split-K workspace too small");
}
}  // namespace

GemmPtrs Model::gemm_ptrs(const void* A, size_t w, size_t bias, const void* res, void* C, const Workspace& ws) const {
  GemmPtrs p;
  p.A = A;
  p.W = ptr<void>(w);
  p.bias = ptr<float>(bias);
  p.res = res;
  p.C = C;
  p.partial = ws.partial;
  p.counters = ws.counters;
  p.zeros = dblob_;  // the blob starts with a zeroed 256-byte line
  return p;
}

size_t Model::conv_partial(const ConvW& c, int B, int H, int W) const {
  int OH, OW;
  GemmDesc d = conv_desc(c, B, H, W, OH, OW);
  d.a_split = m_.split && &c != &m_.stem;  // as run_conv: the plan (halo, split-K) depends on it
  return gemm_partial_floats(d, c.prec);
}

size_t Model::linear_partial(const LinearW& L, int M) const {
  return gemm_partial_floats(linear_desc(L, M, L.k, L.n), L.prec);
}

size_t Model::layers_partial(int T) const {
  size_t partial = 0;
  for (const auto& L : m_.tf)
    partial = std::max({partial, linear_partial(L.qkv, T), linear_partial(L.out, T), linear_partial(L.ff1, T),
                        linear_partial(L.ff2, T)});
  return partial;
}

Model::ConvCall Model::conv_call(const ConvW& c, const void* x, int B, int H, int W, void* y, int& OH, int& OW,
                                 Act act, const void* res, Workspace& ws, bool out_f32, bool res_f32) const {
  ConvCall k;
  GemmDesc& d = k.d;
  d = conv_desc(c, B, H, W, OH, OW);
  d.act = act;
  d.wplane = c.wplane;
  d.out_split = m_.split;
  d.a_split = m_.split && &c != &m_.stem;  // the stem reads the ingested fp32 image
  d.out_f32 = out_f32;
  d.res_f32 = res_f32;
  d.out_f16 = m_.f16 && c.prec == Prec::F16X3 && !out_f32;  // F16M stem: F16X3 contraction, fp16 activations
  const size_t es = m_.f16 ? 2 : 4;
  k.flops = 2.0 * d.M * d.N * (double)c.kh * c.kw * c.cin;
  k.bytes = (double)B * H * W * c.cin_pad * es + (double)c.cout * d.K * es + (double)d.M * d.N * es * (res ? 2 : 1);
  k.p = gemm_ptrs(x, c.w, c.b, res, y, ws);
  k.prec = c.prec;
  return k;
}

void Model::run_conv(const ConvW& c, const void* x, int B, int H, int W, void* y, int& OH, int& OW,
                     Act act, const void* res, Workspace& ws, hipStream_t s, bool out_f32, bool res_f32) {
  const ConvCall k = conv_call(c, x, B, H, W, y, OH, OW, act, res, ws, out_f32, res_f32);
  require_fit(k.d, k.prec, ws);
  prof_op(s, [&] { return conv_name(c, k.d.M); }, k.flops, k.bytes, [&] { gemm(k.d, k.p, k.prec, s); });
}

// A grouped conv packed for the grouped kernel (ConvW::gconv; conv_group.hip): no GEMM plan, no
// split-K workspace.  flops: the conv's own (1 / groups of the dense count).
void Model::run_gconv(const ConvW& c, const void* x, int B, int H, int W, void* y, int& OH, int& OW, Act act,
                      hipStream_t s) {
  OH = (H + 2 * c.pad - c.kh) / c.stride + 1;
  OW = (W + 2 * c.pad - c.kw) / c.stride + 1;
  const int M = B * OH * OW;
  prof_op(s,
          [&] {
            return "gconv3x3_c" + std::to_string(c.cout) + "_g" + std::to_string(c.groups) + "_s" +
                   std::to_string(c.stride) + "_M" + std::to_string(M);
          },
          2.0 * M * c.cout * 9.0 * (c.cin / c.groups),
          ((double)B * H * W * c.cin + (double)M * c.cout) * 2 + (double)gconv_packed_bytes(c.cout, c.groups),
          [&] { conv_group(x, ptr<void>(c.w), ptr<float>(c.b), y, B, H, W, c.cout, c.groups, c.stride, act == Act::Relu, s); });
}

// A block's first conv and its downsample conv read the same input: one grouped
// launch (gemm_pair) instead of two dependent ones.
void Model::run_conv_pair(const ConvW& c0, const void* x, int B, int H, int W, void* y0, int& OH0, int& OW0,
                          Act act0, const ConvW& c1, void* y1, bool out1_f32, Workspace& ws, hipStream_t s) {
  int OH1, OW1;
  const ConvCall k0 = conv_call(c0, x, B, H, W, y0, OH0, OW0, act0, nullptr, ws, false, false);
  const ConvCall k1 = conv_call(c1, x, B, H, W, y1, OH1, OW1, Act::None, nullptr, ws, out1_f32, false);
  if (k0.prec != k1.prec) {
    run_conv(c0, x, B, H, W, y0, OH0, OW0, act0, nullptr, ws, s);
    run_conv(c1, x, B, H, W, y1, OH1, OW1, Act::None, nullptr, ws, s, out1_f32);
    return;
  }
  require_fit(k0.d, k0.prec, ws, &k1.d);
  prof_op(s, [&] { return conv_name(c0, k0.d.M) + "+" + conv_name(c1, k1.d.M); }, k0.flops + k1.flops,
          k0.bytes + k1.bytes, [&] { gemm_pair(k0.d, k0.p, k1.d, k1.p, k0.prec, s); });
}

void Model::run_gemm(const LinearW& L, const void* A, int M, int lda, void* C, int ldc, bool out_f32, Act act,
                     const void* res, bool res_f32, int ldr, Workspace& ws, hipStream_t s, const LnSpec* ln,
                     size_t planes) {
  GemmDesc d = linear_desc(L, M, lda, ldc);
  d.act = act;
  d.out_f32 = out_f32;
  d.res_f32 = res_f32;
  d.ldr = ldr;
  if (planes) {  // C (and an fp16-typed residual) in two fp16 planes `planes` elements apart
    d.out_planes = true;
    d.res_planes = res != nullptr && !res_f32;
    d.plane = planes;
  }
  d.wplane = L.wplane;
  GemmPtrs p = gemm_ptrs(A, L.w, L.b, res, C, ws);
  LnPtrs& lp = p.ln;
  if (ln) {
    if (ln->in_stats) {
      if (!L.c1) throw std::runtime_error("LayerNorm fold: the GEMM's weights were not packed folded");
      d.ln_in_chunks = L.k / 64;
      d.ln_in_eps = m_.eps;
      lp.in_stats = ln->in_stats;
      lp.c1 = ptr<float>(L.c1);
    }
    if (ln->res_stats) {
      d.res_ln_chunks = L.n / 64;
      d.res_ln_eps = m_.eps;
      lp.res_stats = ln->res_stats;
      lp.res_g = ln->res_g;
      lp.res_b = ln->res_b;
    }
    if (ln->out_stats) {
      d.ln_out = true;
      d.ld16 = L.n;
      lp.out_stats = ln->out_stats;
      lp.c16 = static_cast<_Float16*>(ln->c16);
    }
  }
  require_fit(d, L.prec, ws);
  const size_t es = m_.f16 ? 2 : 4;
  prof_op(s, [&] { return "gemm_M" + std::to_string(M) + "_N" + std::to_string(L.n) + "_K" + std::to_string(L.k); },
          2.0 * M * L.n * (double)L.k,
          (double)M * L.k * es + (double)L.n * L.k * es + (double)M * L.n * (out_f32 || planes ? 4 : es) +
              (res ? (double)M * L.n * (res_f32 || planes ? 4 : es) : 0.0),
          [&] { gemm(d, p, L.prec, s); });
}

void Model::run_qkv_attention(const LinearW& L, const void* x, const float* in_stats, void* qkv, void* ctx, int B,
                              int S, Workspace& w, hipStream_t s) {
  const int D = m_.D, heads = m_.heads, T = B * S, hd = D / heads;
  const float scale = 1.0f / std::sqrt((float)hd);
  const float* mask = w.has_mask ? w.mask_bias : nullptr;
  if (qkv_fused_ > 0 && S <= (qkv_fused_ >= 2 ? 256 : 128) && m_.f16 && L.prec == Prec::F16 &&
      qkv_attention_eligible(S, heads, hd, L.k, L.kpad, L.krep, D, L.kpad) && (!in_stats || L.c1)) {
    prof_op(s, [&] { return "qkv_attention_S" + std::to_string(S); }, 2.0 * T * L.n * (double)L.k + 4.0 * B * S * S * D,
            (double)T * D * 2 * 2 + (double)L.n * L.k * 2, [&] {
              qkv_attention(x, D, ptr<void>(L.w), L.kpad, ptr<float>(L.b), in_stats,
                            in_stats ? ptr<float>(L.c1) : nullptr, D / 64, m_.eps, mask, ctx, B, S, heads, scale, s);
            });
    return;
  }
  LnSpec q;
  q.in_stats = in_stats;
  run_gemm(L, x, T, D, qkv, 3 * D, false, Act::None, nullptr, false, 0, w, s, in_stats ? &q : nullptr);
  prof_op(s, [&] { return "attention_S" + std::to_string(S); }, 4.0 * B * S * S * D,
          (double)T * 4 * D * (m_.f16 ? 2 : 4), [&] { attention(qkv, mask, ctx, B, S, heads, hd, scale, m_.f16, s); });
}

// avgpool + fc as one GEMM over every pixel of the last stage with a
// column-mean epilogue (GemmDesc::pool_rows): the split / fp16 / fp32 activation
// is the A operand as is, so the pooled vector never goes through HBM.
bool Model::pooled_fc(int hw) const { return hw > 0 && hw <= 64 && (!m_.split || m_.feat % 32 == 0); }

GemmDesc Model::pooled_fc_desc(int B, int hw) const {
  GemmDesc d = linear_desc(m_.fc, B * hw, m_.feat, m_.classes);
  d.pool_rows = hw;
  d.out_f32 = true;
  d.a_split = m_.split;
  d.wplane = m_.fc.wplane;
  return d;
}

void Model::run_pooled_fc(const void* act, int B, int hw, void* out, Workspace& ws, hipStream_t s) {
  const LinearW& fc = m_.fc;
  const int classes = m_.classes, feat = m_.feat;
  const GemmDesc d = pooled_fc_desc(B, hw);
  require_fit(d, fc.prec, ws);
  const size_t es = m_.f16 ? 2 : 4;
  const GemmPtrs p = gemm_ptrs(act, fc.w, fc.b, nullptr, out, ws);
  prof_op(s, [&] {
            return "avgpool_fc_M" + std::to_string(B * hw) + "_N" + std::to_string(classes) + "_K" + std::to_string(feat);
          },
          2.0 * B * classes * (double)feat,
          (double)B * hw * feat * es + (double)fc.n * fc.k * es + (double)B * classes * 4,
          [&] { gemm(d, p, fc.prec, s); });
}

// ---------------------------------------------------------------------------
// Workspaces
// ---------------------------------------------------------------------------
std::vector<size_t> Model::workspace_sizes_resnet(size_t& partial) const {
  const ConvW& stem = m_.stem;
  const int B = m_.max_batch;
  std::vector<size_t> sz(kRnBufs);
  sz[kRnIngest] = m_.stem_fused ? 256 : (size_t)B * m_.image * m_.image * stem.cin_pad * (stem.prec == Prec::F16 ? 2 : 4);
  int H = m_.image, OH, OW;
  size_t amax = 0;
  // a conv over an h x h input: its split-K slabs, and its output among the activation slots
  auto conv = [&](const ConvW& c, int h, bool stored = true) {
    if (c.gconv) {  // the grouped kernel: no plan, no slabs
      OH = (h + 2 * c.pad - c.kh) / c.stride + 1;
    } else {
      partial = std::max(partial, conv_partial(c, B, h, h));
      conv_desc(c, B, h, h, OH, OW);
    }
    if (stored) amax = std::max(amax, (size_t)B * OH * OH * c.cout);
    return OH;
  };
  H = conv(stem, H, !m_.stem_fused);  // fused: the stem's output is never materialised
  H = (H + 2 - 3) / 2 + 1;
  amax = std::max(amax, (size_t)B * H * H * stem.cout);
  for (const auto& b : m_.blocks) {
    if (b.has_ds) {  // conv1 + downsample in one grouped launch (run_conv_pair)
      partial = std::max(partial, conv_partial(b.c1, B, H, H) + conv_partial(b.ds, B, H, H));
      conv(b.ds, H);
    }
    int H2 = conv(b.c1, H);
    H2 = conv(b.c2, H2);
    if (m_.bottleneck) H2 = conv(b.c3, H2);
    H = H2;
  }
  partial = std::max(partial, linear_partial(m_.fc, B));
  if (pooled_fc(H * H)) partial = std::max(partial, gemm_partial_floats(pooled_fc_desc(B, H * H), m_.fc.prec));
  // F16M: the downsample outputs are fp32 in the same pool
  const size_t ea = m_.mixed ? 4 : m_.f16 ? 2 : 4;
  for (int i = kRnAct0; i <= kRnAct4; ++i) sz[i] = amax * ea;
  sz[kRnPooled] = (size_t)B * m_.feat * ea;  // fp32 under F16M: the FC's A
  sz[kRnLogits] = (image_io_ & SPI_IMAGE_NO_LOGITS) ? (size_t)B * m_.classes * 4 : 0;
  sz[kRnResized] = resize_short_ ? (size_t)B * 3 * m_.image * m_.image * 4 : 0;
  return sz;
}

std::vector<size_t> Model::workspace_sizes_bert(size_t& partial) const {
  const size_t T = (size_t)m_.max_batch * m_.seq, D = m_.D, es = m_.f16 ? 2 : 4;
  std::vector<size_t> sz(kBtBufs);
  sz[kBtHidden] = T * D * 4;
  sz[kBtHidden16] = T * D * es;
  sz[kBtQkv] = T * 3 * D * es;
  sz[kBtCtx] = T * D * es;
  sz[kBtAttn] = T * D * 4;
  sz[kBtFfn] = T * m_.ffn * es;
  sz[kBtStats1] = sz[kBtStats2] = T * (D / 64) * 8;
  sz[kBtCls] = (m_.bert_io & SPI_BERT_NO_HIDDEN) ? (size_t)m_.max_batch * D * 4 : 0;
  partial = std::max(partial, layers_partial((int)T));
  return sz;
}

std::vector<size_t> Model::workspace_sizes_vit(size_t& partial) const {
  const size_t B = m_.max_batch, T = B * (m_.npatch + 1), D = m_.D, es = m_.f16 ? 2 : 4;
  std::vector<size_t> sz(kVtBufs);
  sz[kVtPatches] = B * m_.npatch * m_.patch_proj.k * es;
  sz[kVtProj] = B * m_.npatch * D * 4;
  sz[kVtX] = T * D * 4;
  sz[kVtLn] = T * D * es;
  sz[kVtQkv] = T * 3 * D * es;
  sz[kVtCtx] = T * D * es;
  sz[kVtMlp] = T * m_.ffn * es;
  sz[kVtCls] = B * D * es;
  sz[kVtStats] = T * (D / 64) * 8;
  sz[kVtLogits] = (image_io_ & SPI_IMAGE_NO_LOGITS) ? B * m_.classes * 4 : 0;
  sz[kVtResized] = resize_short_ ? B * 3 * m_.image * m_.image * 4 : 0;
  partial = std::max({partial, linear_partial(m_.patch_proj, (int)B * m_.npatch), layers_partial((int)T),
                      linear_partial(m_.head, (int)B)});
  return sz;
}

Workspace* Model::workspace(hipStream_t s) {
  std::lock_guard<std::mutex> lk(mu_);
  auto it = ws_.find(s);
  if (it != ws_.end()) return it->second.get();
  std::lock_guard<std::mutex> cap(g_capture_mu);
  auto w = std::make_unique<Workspace>();
  size_t partial = 0;
  std::vector<size_t> sizes;  // bytes per buffer
  switch (m_.family) {
    case SPI_FAMILY_RESNET: sizes = workspace_sizes_resnet(partial); break;
    case SPI_FAMILY_BERT: sizes = workspace_sizes_bert(partial); break;
    case SPI_FAMILY_VIT: sizes = workspace_sizes_vit(partial); break;
  }
  if (m_.family == SPI_FAMILY_BERT) SPI_HIP(hipMalloc(&w->mask_bias, (size_t)m_.max_batch * m_.seq * sizeof(float)));
  for (size_t bytes : sizes) {
    void* b = nullptr;
    SPI_HIP(hipMalloc(&b, std::max<size_t>(bytes, 256)));
    w->bufs.push_back(b);
  }
  // Split-K slabs: choose_plan only splits grids of < 128 tiles into <= 512 +
  // tiles workgroups of 64x64, so 640 * 64 * 64 floats bounds every batch size.
  partial = std::max(partial, (size_t)640 * 64 * 64);
  w->partial_floats = partial;
  SPI_HIP(hipMalloc(&w->partial, partial * sizeof(float)));
  SPI_HIP(hipMalloc(&w->counters, kCounterSlots * sizeof(int)));
  // stream-ordered zeroing (a synchronous null-stream memset would also break
  // concurrent captures); it precedes every use of the tickets on this stream
  SPI_HIP(hipMemsetAsync(w->counters, 0, kCounterSlots * sizeof(int), s));
  Workspace* raw = w.get();
  ws_[s] = std::move(w);
  return raw;
}

// ---------------------------------------------------------------------------
// ResNet plan
// ---------------------------------------------------------------------------
// src (SrcKind), here and in the ViT prologue: an 8-bit image task takes the same launch, which then
// reads bytes and applies input_xf_ at the load.  The profile hooks always pass fp32 inputs, so the
// op records' byte counts stay those of an fp32 image.
void Model::prologue_resnet(Workspace& w, int B, const void* x, hipStream_t s, int src) {
  const ConvW& stem = m_.stem;
  const int image = m_.image;
  if (!m_.stem_fused) {
    prof_op(s, "ingest_nchw", 0, (double)B * 3 * image * image * 4 * 2, [&] {
      ingest_nchw(x, w.bufs[kRnIngest], B, 3, image, image, stem.cin_pad, stem.prec == Prec::F16, s, src, input_xf_);
    });
    return;
  }
  // the stem reads the task's NCHW buffer itself and writes the pooled map
  const int OH = (image + 6 - 7) / 2 + 1, PH = (OH + 2 - 3) / 2 + 1;
  prof_op(s, "stem_pool", 2.0 * B * OH * OH * stem.cout * 147.0,
          (double)B * 3 * image * image * 4 + (double)B * PH * PH * stem.cout * (m_.split ? 4 : 2), [&] {
            stem_pool(x, ptr<void>(m_.stem_pool_w), ptr<float>(stem.b), w.bufs[kRnAct1], B, image, image,
                      m_.split ? 2 : stem.prec != Prec::F16 ? 1 : 0, m_.split, stem_pr_, s, src, input_xf_);
          });
}

void Model::body_resnet(Workspace& w, int B, hipStream_t s) {
  const ConvW& stem = m_.stem;
  const bool f16 = m_.f16, split = m_.split;
  int H = m_.image, OH, OW;
  void* const* buf = w.bufs.data();
  if (m_.stem_fused) {  // stem + max pool ran in the prologue
    OH = (H + 6 - 7) / 2 + 1;
    H = (OH + 2 - 3) / 2 + 1;
  } else {
    run_conv(stem, buf[kRnIngest], B, H, H, buf[kRnAct0], OH, OW, Act::Relu, nullptr, w, s);
    H = OH;
    const int PH = (H + 2 - 3) / 2 + 1;
    prof_op(s, "maxpool", 0, (double)B * (H * H + PH * PH) * stem.cout * (f16 ? 2 : 4), [&] {
      if (split)
        maxpool_nhwc_split(buf[kRnAct0], buf[kRnAct1], B, H, H, stem.cout, PH, PH, 3, 2, 1, s);
      else
        maxpool_nhwc(buf[kRnAct0], buf[kRnAct1], B, H, H, stem.cout, PH, PH, 3, 2, 1, f16, s);
    });
    H = PH;
  }
  int cur = kRnAct1;
  auto pick = [&](std::initializer_list<int> busy) {  // the first activation slot not in use
    for (int i = kRnAct0; i <= kRnAct4; ++i)
      if (std::find(busy.begin(), busy.end(), i) == busy.end()) return i;
    return -1;
  };
  for (const auto& b : m_.blocks) {
    int H1, H2, last = pick({cur}), ident = cur;  // last: the slot of the block's latest intermediate
    if (b.has_ds) {  // the downsample reads the block input too: grouped with conv1
      ident = pick({cur, last});  // F16M: hi + lo weights, fp16 out like every conv (round 5: fp32 out kept nothing)
      run_conv_pair(b.c1, buf[cur], B, H, H, buf[last], H1, OW, Act::Relu, b.ds, buf[ident], false, w, s);
    } else {
      run_conv(b.c1, buf[cur], B, H, H, buf[last], H1, OW, Act::Relu, nullptr, w, s);
    }
    H2 = H1;
    if (m_.bottleneck) {  // conv1 is 1x1 / stride 1 (H1 == H); conv2 carries the stride
      const int t2 = pick({cur, last, ident});
      if (b.c2.gconv)
        run_gconv(b.c2, buf[last], B, H1, H1, buf[t2], H2, OW, Act::Relu, s);
      else
        run_conv(b.c2, buf[last], B, H1, H1, buf[t2], H2, OW, Act::Relu, nullptr, w, s);
      last = t2;
    }
    const int o = pick({cur, last, ident});
    run_conv(m_.bottleneck ? b.c3 : b.c2, buf[last], B, H2, H2, buf[o], OH, OW, Act::Relu, buf[ident], w, s);
    cur = o;
    H = H2;
  }
  w.final_buf = cur;
  w.final_hw = H * H;
  if (!pooled_fc(H * H)) {  // else avgpool + fc run as one GEMM in the epilogue
    prof_op(s, "avgpool", 0, (double)B * H * H * m_.feat * (f16 ? 2 : 4), [&] {
      if (split)  // fp32 for the F16X3 FC (as under F16M below)
        avgpool_nhwc_split(buf[cur], static_cast<float*>(buf[kRnPooled]), B, H * H, m_.feat, s);
      else
        avgpool_nhwc(buf[cur], buf[kRnPooled], B, H * H, m_.feat, f16, s, m_.mixed);
    });
    w.final_buf = kRnPooled;
  }
}

// ---------------------------------------------------------------------------
// BERT plan (post-LN)
// ---------------------------------------------------------------------------
void Model::body_bert(Workspace& w, int B, int S, hipStream_t s) {
  if (m_.ln_fold) return body_bert_folded(w, B, S, s);
  const int D = m_.D, ffn = m_.ffn, T = B * S;
  const bool f16 = m_.f16;
  float* hf = static_cast<float*>(w.bufs[kBtHidden]);
  void* ht = f16 ? w.bufs[kBtHidden16] : w.bufs[kBtHidden];
  float* a = static_cast<float*>(w.bufs[kBtAttn]);
  void* ff = w.bufs[kBtFfn];
  auto ln = [&](const LnW& l) {
    prof_op(s, "layernorm", 0, ln_bytes(T, true), [&] {
      layernorm(a, D, ptr<float>(l.g), ptr<float>(l.b), hf, f16 ? ht : nullptr, D, T, D, m_.eps, f16, s);
    });
  };
  for (int i = 0; i < m_.layers; ++i) {
    const TfLayer& L = m_.tf[i];
    run_qkv_attention(L.qkv, ht, nullptr, w.bufs[kBtQkv], w.bufs[kBtCtx], B, S, w, s);
    run_gemm(L.out, w.bufs[kBtCtx], T, D, a, D, true, Act::None, hf, true, D, w, s);
    ln(L.ln1);
    run_gemm(L.ff1, ht, T, D, ff, ffn, false, Act::Gelu, nullptr, false, 0, w, s);
    run_gemm(L.ff2, ff, T, ffn, a, D, true, Act::None, hf, true, D, w, s);
    if (i + 1 < m_.layers) ln(L.ln2);  // the last layer's LN2 is the epilogue's
  }
}

// Post-LN with the LayerNorms folded (ln_fold.hpp) over two-plane fp16 rows (round 6,
// GemmDesc::res_planes: hi = fp16(x), lo = fp16(x - hi), a plane of T x D apart, the bytes of
// fp32): kBtHidden holds the embedding output (fp32, the prologue's), then each layer's pre-LN2
// rows b as planes; kBtAttn the pre-LN1 rows a as planes; S1 / S2 their row statistics.  The hi
// planes are the folding GEMMs' fp16 A operands, so no producer writes an fp16 copy.
// Layer i:
//   qkv  = LN2_{i-1}(b) Wqkv  (folded; layer 0 reads the embedding's fp16 output ht)
//   a    = ctx Wo + LN2_{i-1}(b)    -> S1   (layer 0: + the fp32 embedding output)
//   ff   = GELU(LN1_i(a) W1)  (folded)
//   b    = ff W2 + LN1_i(a)         -> S2
// and the epilogue runs the one LayerNorm left, LN2 of the last layer.
void Model::body_bert_folded(Workspace& w, int B, int S, hipStream_t s) {
  const int D = m_.D, ffn = m_.ffn, T = B * S;
  float* hf = static_cast<float*>(w.bufs[kBtHidden]);
  void* ht = w.bufs[kBtHidden16];
  void* ctx = w.bufs[kBtCtx];
  void* ff = w.bufs[kBtFfn];
  float* S1 = static_cast<float*>(w.bufs[kBtStats1]);
  float* S2 = static_cast<float*>(w.bufs[kBtStats2]);
  _Float16* bh = static_cast<_Float16*>(w.bufs[kBtHidden]);
  _Float16* ah = static_cast<_Float16*>(w.bufs[kBtAttn]);
  const size_t plane = (size_t)T * D;
  for (int i = 0; i < m_.layers; ++i) {
    const TfLayer& L = m_.tf[i];
    run_qkv_attention(L.qkv, i > 0 ? bh : ht, i > 0 ? S2 : nullptr, w.bufs[kBtQkv], ctx, B, S, w, s);
    LnSpec o;
    if (i > 0) {
      o.res_stats = S2;
      o.res_g = ptr<float>(m_.tf[i - 1].ln2.g);
      o.res_b = ptr<float>(m_.tf[i - 1].ln2.b);
    }
    o.out_stats = S1;
    run_gemm(L.out, ctx, T, D, ah, D, false, Act::None, i > 0 ? static_cast<void*>(bh) : hf, i == 0, D, w, s, &o,
             plane);
    LnSpec f1;
    f1.in_stats = S1;
    run_gemm(L.ff1, ah, T, D, ff, ffn, false, Act::Gelu, nullptr, false, 0, w, s, &f1);
    LnSpec f2;
    f2.res_stats = S1;
    f2.res_g = ptr<float>(L.ln1.g);
    f2.res_b = ptr<float>(L.ln1.b);
    f2.out_stats = S2;
    run_gemm(L.ff2, ff, T, ffn, bh, D, false, Act::None, ah, false, D, w, s, &f2, plane);
  }
}

// The last LayerNorm and the outputs bert_io selects, in the order hidden, pooler, mean.  With the
// hidden state selected the LayerNorm writes it as before and the sentence outputs read those fp32
// rows.  Without it (SPI_BERT_NO_HIDDEN) the mean needs every row, so the LayerNorm goes into the fp32
// workspace buffer that is dead after the last FFN2 (the fold's a planes, else the residual rows);
// the pooler alone needs the B class-token rows only (row stride S D, as ViT's layernorm_cls).
void Model::epilogue_bert(Workspace& w, int B, int S, void* const* out, hipStream_t s) {
  const LnW& l = m_.tf.back().ln2;
  const int D = m_.D, T = B * S, io = m_.bert_io;
  const bool hidden = !(io & SPI_BERT_NO_HIDDEN), pooler = (io & SPI_BERT_OUT_POOLER) != 0,
             mean = (io & SPI_BERT_OUT_MEAN) != 0;
  const bool cls_only = !hidden && !mean;
  int o = 0;
  float* rows = hidden     ? static_cast<float*>(out[o++])
                : cls_only ? static_cast<float*>(w.bufs[kBtCls])
                           : static_cast<float*>(w.bufs[m_.ln_fold ? kBtAttn : kBtHidden]);
  const int nrows = cls_only ? B : T, ldx = cls_only ? S * D : D;
  prof_op(s, cls_only ? "layernorm_cls" : "layernorm_out", 0, (double)nrows * D * 8, [&] {
    // the last layer's pre-LN2 rows: the two-plane b under the LayerNorm fold, else a
    if (m_.ln_fold)
      layernorm_planes(static_cast<const _Float16*>(w.bufs[kBtHidden]), (size_t)T * D, ldx, ptr<float>(l.g),
                       ptr<float>(l.b), rows, nullptr, D, nrows, D, m_.eps, m_.f16, s);
    else
      layernorm(static_cast<float*>(w.bufs[kBtAttn]), ldx, ptr<float>(l.g), ptr<float>(l.b), rows, nullptr, D, nrows,
                D, m_.eps, m_.f16, s);
  });
  if (pooler) {
    float* y = static_cast<float*>(out[o++]);
    prof_op(s, "bert_pooler", 2.0 * B * D * (double)D, (double)D * D * 4 + (double)B * D * 8, [&] {
      bert_pooler(rows, cls_only ? (size_t)D : (size_t)S * D, ptr<float>(m_.pool_w), ptr<float>(m_.pool_b), y, B, D, s);
    });
  }
  if (mean) {
    float* y = static_cast<float*>(out[o++]);
    prof_op(s, "bert_mean_pool", 2.0 * T * D, (double)T * D * 4 + (double)B * D * 4, [&] {
      masked_mean(rows, w.has_mask ? w.mask_ids : nullptr, y, B, S, D, s);
    });
  }
}

// ---------------------------------------------------------------------------
// ViT plan (pre-LN)
// ---------------------------------------------------------------------------
void Model::body_vit(Workspace& w, int B, hipStream_t s) {
  const int D = m_.D, ffn = m_.ffn, npatch = m_.npatch, S = npatch + 1, T = B * S;
  const bool f16 = m_.f16;
  void* const* buf = w.bufs.data();
  run_gemm(m_.patch_proj, buf[kVtPatches], B * npatch, m_.patch_proj.k, buf[kVtProj], D, true, Act::None, nullptr,
           false, 0, w, s);
  if (m_.ln_fold) return body_vit_folded(w, B, s);
  float* x = static_cast<float*>(buf[kVtX]);
  prof_op(s, "vit_assemble", 0, (double)T * D * 4 * 3, [&] {
    vit_assemble(static_cast<const float*>(buf[kVtProj]), ptr<float>(m_.cls), ptr<float>(m_.vpos), x, B, npatch, D, s);
  });
  // LN of `rows` rows ldx apart into the compute-type buffer y
  auto ln = [&](const char* name, const LnW& l, int ldx, int rows, void* y) {
    prof_op(s, name, 0, ln_bytes(rows, false), [&] {
      layernorm(x, ldx, ptr<float>(l.g), ptr<float>(l.b), f16 ? nullptr : static_cast<float*>(y), f16 ? y : nullptr, D,
                rows, D, m_.eps, f16, s);
    });
  };
  for (const TfLayer& L : m_.tf) {
    ln("layernorm", L.ln1, D, T, buf[kVtLn]);
    run_qkv_attention(L.qkv, buf[kVtLn], nullptr, buf[kVtQkv], buf[kVtCtx], B, S, w, s);
    run_gemm(L.out, buf[kVtCtx], T, D, x, D, true, Act::None, x, true, D, w, s);
    ln("layernorm", L.ln2, D, T, buf[kVtLn]);
    run_gemm(L.ff1, buf[kVtLn], T, D, buf[kVtMlp], ffn, false, Act::Gelu, nullptr, false, 0, w, s);
    run_gemm(L.ff2, buf[kVtMlp], T, ffn, x, D, true, Act::None, x, true, D, w, s);
  }
  // final LN on the class-token rows only (torchvision: x = ln(x); x = x[:, 0])
  ln("layernorm_cls", m_.final_ln, S * D, B, buf[kVtCls]);
}

// Pre-LN with the LayerNorms folded (ln_fold.hpp) over a two-plane residual stream (round 6,
// GemmDesc::res_planes): x lives in kVtX as hi = fp16(x) and lo = fp16(x - hi), a plane of
// T x D apart -- the bytes of fp32, ~22-bit values.  vit_assemble_planes and the GEMMs that
// update x (out-proj, FFN2: residual and output both two-plane, in place) write the rows'
// chunk statistics Sx; the QKV GEMMs of layers >= 1 and every FFN1 GEMM read the hi plane as
// their fp16 A operand with LN1 / LN2 folded in.  No producer writes an fp16 copy (the hi
// plane is one).  Two LayerNorm launches are left: layer 0's LN1 (the stream's first rows
// come from the patch embedding, whose row means make the folded form lose ~20 % of the fp16
// margin: test_transformer_layernorm_fold, 8.5e-4 folded vs 7.0e-4 at this launch) and the
// class-token LayerNorm at the end.
void Model::body_vit_folded(Workspace& w, int B, hipStream_t s) {
  const int D = m_.D, ffn = m_.ffn, npatch = m_.npatch, S = npatch + 1, T = B * S;
  void* const* buf = w.bufs.data();
  float* Sx = static_cast<float*>(buf[kVtStats]);
  _Float16* xh = static_cast<_Float16*>(buf[kVtX]);
  const size_t plane = (size_t)T * D;
  prof_op(s, "vit_assemble", 0, (double)T * D * 4 * 3, [&] {
    vit_assemble_planes(static_cast<const float*>(buf[kVtProj]), ptr<float>(m_.cls), ptr<float>(m_.vpos), xh, plane,
                        nullptr, B, npatch, D, s);
  });
  for (int i = 0; i < m_.layers; ++i) {
    const TfLayer& L = m_.tf[i];
    if (i == 0)
      prof_op(s, "layernorm", 0, ln_bytes(T, false), [&] {
        layernorm_planes(xh, plane, D, ptr<float>(L.ln1.g), ptr<float>(L.ln1.b), nullptr, buf[kVtLn], D, T, D, m_.eps,
                         m_.f16, s);
      });
    run_qkv_attention(L.qkv, i == 0 ? buf[kVtLn] : xh, i == 0 ? nullptr : Sx, buf[kVtQkv], buf[kVtCtx], B, S, w, s);
    LnSpec o;
    o.out_stats = Sx;
    run_gemm(L.out, buf[kVtCtx], T, D, xh, D, false, Act::None, xh, false, D, w, s, &o, plane);
    LnSpec f1;
    f1.in_stats = Sx;
    run_gemm(L.ff1, xh, T, D, buf[kVtMlp], ffn, false, Act::Gelu, nullptr, false, 0, w, s, &f1);
    run_gemm(L.ff2, buf[kVtMlp], T, ffn, xh, D, false, Act::None, xh, false, D, w, s, &o, plane);
  }
  prof_op(s, "layernorm_cls", 0, ln_bytes(B, false), [&] {
    layernorm_planes(xh, plane, S * D, ptr<float>(m_.final_ln.g), ptr<float>(m_.final_ln.b), nullptr, buf[kVtCls], D,
                     B, D, m_.eps, m_.f16, s);
  });
}

// ---------------------------------------------------------------------------
// Forward: prologue -> body (graph-capturable) -> epilogue, each dispatched by family (model.hpp)
// ---------------------------------------------------------------------------
void Model::prologue(Workspace& w, int B, int S, const void* const* in, hipStream_t s, ImageSrc isrc) {
  const int D = m_.D, image = m_.image;
  const bool f16 = m_.f16;
  int src = isrc.kind;
  const void* image_in = in[0];
  if (isrc.H > 0) {
    // the input resize: one launch writes the normalised fp32 NCHW image into the workspace, and the
    // family's fp32-source prologue below reads it as it reads an fp32 task
    if (!resize_short_) throw std::logic_error("prologue: a resized source without the input resize");
    float* y = static_cast<float*>(w.bufs[m_.family == SPI_FAMILY_RESNET ? (int)kRnResized : (int)kVtResized]);
    prof_op(s, "resize_crop_u8", 0, (double)B * 3 * ((double)isrc.H * isrc.W + (double)image * image * 4), [&] {
      resize_crop_u8(in[0], src == kSrcU8Nhwc, B, isrc.H, isrc.W, resize_short_, image, input_xf_, y, s);
    });
    image_in = y;
    src = kSrcF32Nchw;
  }
  switch (m_.family) {
    case SPI_FAMILY_RESNET: return prologue_resnet(w, B, image_in, s, src);
    case SPI_FAMILY_BERT: {
      const double T = (double)B * S;
      // the attention mask's additive bias is written by the embedding kernel (round 6: one launch
      // fewer per forward than a separate mask_to_bias)
      w.has_mask = in[1] != nullptr;
      w.mask_ids = static_cast<const int64_t*>(in[1]);
      // SPI_BERT_TOKEN_TYPES: the whole type table and, when the task brings them, its segment ids
      const bool typed = (m_.bert_io & SPI_BERT_TOKEN_TYPES) != 0;
      const int64_t* types = typed ? static_cast<const int64_t*>(in[2]) : nullptr;
      return prof_op(s, "bert_embed", 0, T * D * (4 * 3 + 4 + (f16 ? 2 : 0)) + (w.has_mask ? T * 12 : 0) + (types ? T * 8 : 0), [&] {
        bert_embed(static_cast<const int64_t*>(in[0]), ptr<float>(m_.word), ptr<float>(m_.pos),
                   ptr<float>(typed ? m_.type_table : m_.type0), ptr<float>(m_.emb_ln.g), ptr<float>(m_.emb_ln.b),
                   static_cast<float*>(w.bufs[kBtHidden]), f16 ? w.bufs[kBtHidden16] : nullptr, B, S, D, m_.vocab,
                   m_.eps, f16, s, w.has_mask ? w.mask_ids : nullptr, w.has_mask ? w.mask_bias : nullptr, types,
                   m_.type_vocab);
      });
    }
    case SPI_FAMILY_VIT:
      return prof_op(s, "patchify", 0, (double)B * 3 * image * image * (4 + (f16 ? 2 : 4)), [&] {
        patchify(image_in, w.bufs[kVtPatches], B, 3, image, image, m_.patch, f16, s, src, input_xf_);
      });
  }
}

void Model::body(Workspace& w, int B, int S, hipStream_t s) {
  switch (m_.family) {
    case SPI_FAMILY_RESNET: return body_resnet(w, B, s);
    case SPI_FAMILY_BERT: return body_bert(w, B, S, s);
    case SPI_FAMILY_VIT: return body_vit(w, B, s);
  }
}

// ResNet / ViT: the classifier layer writes the logits (into the task's first output, or the workspace
// scratch under SPI_IMAGE_NO_LOGITS); with image_io_ set one more launch derives the other outputs.
void Model::epilogue(Workspace& w, int B, int S, void* const* out, hipStream_t s) {
  switch (m_.family) {
    case SPI_FAMILY_RESNET: {
      float* logits = logits_dst(w.bufs[kRnLogits], out);
      if (pooled_fc(w.final_hw))
        run_pooled_fc(w.bufs[w.final_buf], B, w.final_hw, logits, w, s);
      else
        run_gemm(m_.fc, w.bufs[kRnPooled], B, m_.feat, logits, m_.classes, true, Act::None, nullptr, false, 0, w, s);
      return run_image_outputs(logits, B, out, s);
    }
    case SPI_FAMILY_BERT: return epilogue_bert(w, B, S, out, s);
    case SPI_FAMILY_VIT: {
      float* logits = logits_dst(w.bufs[kVtLogits], out);
      run_gemm(m_.head, w.bufs[kVtCls], B, m_.D, logits, m_.classes, true, Act::None, nullptr, false, 0, w, s);
      return run_image_outputs(logits, B, out, s);
    }
  }
}

// The outputs image_io_ selects beside the logits, in the order probabilities, top-k values, top-k
// indices: one launch (classify.hip), none with only the logits selected.
void Model::run_image_outputs(const float* logits, int B, void* const* out, hipStream_t s) {
  const int io = image_io_, N = m_.classes, k = top_k_;
  if (!(io & (SPI_IMAGE_OUT_PROBS | SPI_IMAGE_OUT_TOPK))) return;
  int o = (io & SPI_IMAGE_NO_LOGITS) ? 0 : 1;
  float* probs = (io & SPI_IMAGE_OUT_PROBS) ? static_cast<float*>(out[o++]) : nullptr;
  float* topv = nullptr;
  int64_t* topi = nullptr;
  if (io & SPI_IMAGE_OUT_TOPK) {
    topv = static_cast<float*>(out[o++]);
    topi = static_cast<int64_t*>(out[o++]);
  }
  prof_op(s, "softmax_topk", 0, (double)B * N * 4 * (probs ? 2 : 1) + (double)B * k * 12, [&] {
    softmax_topk(logits, (size_t)N, probs, topv, topi, B, N, k, (io & SPI_IMAGE_TOPK_PROBS) != 0, s);
  });
}

void Model::forward(hipStream_t s, int B, int S, size_t n, const void* const* in, void* const* out, ImageSrc src) {
  if (device_ < 0) throw std::runtime_error("host-only replica (device < 0) cannot run a forward");
  if (m_.family == SPI_FAMILY_AFFINE) {
    affine(static_cast<const float*>(in[0]), static_cast<float*>(out[0]), n, m_.aff_scale, m_.aff_shift, s);
    return;
  }
  if (m_.family != SPI_FAMILY_BERT) S = 0;  // only BERT's graphs depend on the sequence length
  Workspace* w = workspace(s);
  prologue(*w, B, S, in, s, src);
  if (graphs_ && s != nullptr) {
    SPI_HIP(hipGraphLaunch(graph(*w, B, S, s), s));
  } else {
    body(*w, B, S, s);
  }
  epilogue(*w, B, S, out, s);
}

// The captured body for (batch, mask, S) on this stream's workspace, captured
// on first use (or ahead of time by warmup()).
hipGraphExec_t Model::graph(Workspace& w, int B, int S, hipStream_t s) {
  const int key = (B * 2 + (w.has_mask ? 1 : 0)) * 4096 + S;
  auto it = w.graphs.find(key);
  if (it != w.graphs.end()) return it->second;
  std::lock_guard<std::mutex> cap(g_capture_mu);
  SPI_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  hipGraph_t g = nullptr;
  try {
    body(w, B, S, s);
  } catch (...) {
    // Leave the worker stream usable: end the capture before rethrowing,
    // otherwise every later task on this stream fails.
    if (hipStreamEndCapture(s, &g) == hipSuccess && g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    throw;
  }
  SPI_HIP(hipStreamEndCapture(s, &g));
  hipGraphExec_t e = nullptr;
  const hipError_t ie = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  SPI_HIP(ie);
  return w.graphs.emplace(key, e).first->second;
}

// Per-worker warm-up (the reference warms each worker up before serving,
// inference_runner.cpp:507-560): allocate this stream's workspace and capture
// the body graph for (batch, S, mask) now, so no capture or allocation lands on
// a live request.  Runs nothing on the device.
void Model::warmup(hipStream_t s, int B, int S, bool mask) {
  const bool bert = m_.family == SPI_FAMILY_BERT;
  if (device_ < 0) throw std::runtime_error("host-only replica (device < 0) cannot run a forward");
  if (m_.family == SPI_FAMILY_AFFINE) return;
  if (B < 1 || B > m_.max_batch) throw std::runtime_error("warmup batch exceeds replica max_batch");
  if (bert && (S < 1 || S > m_.seq)) throw std::runtime_error("warmup sequence length out of range");
  Workspace* w = workspace(s);
  if (!graphs_ || s == nullptr) return;
  w->has_mask = bert && mask;
  (void)graph(*w, B, bert ? S : 0, s);
}

}  // namespace spi
