// The host-only forward plans of a model replica (model_plan.hpp).
#include "model_plan.hpp"

#include <cmath>
#include <stdexcept>
#include <utility>

#include "resample.hpp"

namespace spi {

namespace {
bool image_family(const PackedModel& m) { return m.family == SPI_FAMILY_RESNET || m.family == SPI_FAMILY_VIT; }
}  // namespace

// ---------------------------------------------------------------------------
// I/O contract
// ---------------------------------------------------------------------------
int num_inputs_max(const PackedModel& m) {
  return m.family != SPI_FAMILY_BERT ? 1 : (m.bert_io & SPI_BERT_TOKEN_TYPES) ? 3 : 2;
}

int num_outputs(const PackedModel& m, const ReplicaOptions& o) {
  if (o.image_io)
    return !(o.image_io & SPI_IMAGE_NO_LOGITS) + !!(o.image_io & SPI_IMAGE_OUT_PROBS) + 2 * !!(o.image_io & SPI_IMAGE_OUT_TOPK);
  if (m.family != SPI_FAMILY_BERT) return 1;
  return !(m.bert_io & SPI_BERT_NO_HIDDEN) + !!(m.bert_io & SPI_BERT_OUT_POOLER) + !!(m.bert_io & SPI_BERT_OUT_MEAN) +
         !!(m.bert_io & (SPI_BERT_HEAD_SEQUENCE | SPI_BERT_HEAD_TOKEN)) + 2 * !!(m.bert_io & SPI_BERT_HEAD_QA);
}

void check_io(const PackedModel& m, const ReplicaOptions& o, const spi_codelet_args& a, const size_t* in_bytes,
              const size_t* out_bytes) {
  const int ni = (int)a.num_inputs, no = (int)a.num_outputs, image = m.image;
  if (ni < 1 || ni > num_inputs_max(m))
    throw std::runtime_error("model expects " + std::to_string(num_inputs_max(m)) + " input(s), got " +
                             std::to_string(ni));
  if (no != num_outputs(m, o)) throw std::runtime_error("Mismatch between model outputs and StarPU buffers");
  const int64_t B = a.dims[0][0];
  if (B < 1 || B > m.max_batch)
    throw std::runtime_error("batch " + std::to_string(B) + " exceeds replica max_batch " +
                             std::to_string(m.max_batch));
  auto elems = [&](int i) {
    int64_t e = 1;
    for (int d = 0; d < a.num_dims[i]; ++d) e *= a.dims[i][d];
    return e;
  };
  size_t expect_out = 0;
  size_t expect_more[4] = {0, 0, 0, 0};  // the outputs after the first (BERT: bert_io; ResNet / ViT: image_io)
  int i64_out = -1;                   // the output that is SPI_DTYPE_I64 (the top-k indices), if any
  if (m.family == SPI_FAMILY_AFFINE) {
    if (a.input_types[0] != SPI_DTYPE_F32) throw std::runtime_error("[ERROR] Input type mismatch");
    if (in_bytes[0] < (size_t)elems(0) * 4) throw std::runtime_error("[ERROR] Input buffer too small");
    expect_out = (size_t)elems(0) * 4;
  } else if (image_family(m)) {
    const bool u8 = a.input_types[0] == SPI_DTYPE_U8;
    if (!u8 && a.input_types[0] != SPI_DTYPE_F32) throw std::runtime_error("[ERROR] Input type mismatch");
    const std::string sz = std::to_string(image);
    if (u8 && o.resize_short) {
      // the input resize: a source of any size in either layout; dims[1] == 3 is NCHW, also when dims[3] == 3
      const int64_t* d = a.dims[0];
      const bool nchw = a.num_dims[0] == 4 && d[1] == 3, nhwc = a.num_dims[0] == 4 && !nchw && d[3] == 3;
      const int64_t H = nchw ? d[2] : d[1], W = nchw ? d[3] : d[2];
      if ((!nchw && !nhwc) || H < 1 || W < 1 || H > kResizeMax || W > kResizeMax)
        throw std::runtime_error("[ERROR] Tensor layout mismatch: expected [B,3,H,W] or [B,H,W,3] with 1 <= H, W <= " +
                                 std::to_string(kResizeMax) + " (input resize " + std::to_string(o.resize_short) + ")");
      const ResizeGeom g = resize_geom((int)H, (int)W, o.resize_short, image);
      if (std::max(g.RH, g.RW) > kResizeMax)
        throw std::runtime_error("[ERROR] Input resize: a " + std::to_string(H) + "x" + std::to_string(W) +
                                 " source resized to short side " + std::to_string(o.resize_short) + " has long side " +
                                 std::to_string(std::max(g.RH, g.RW)) + ", above " + std::to_string(kResizeMax));
    } else {
      const bool nchw = a.num_dims[0] == 4 && a.dims[0][1] == 3 && a.dims[0][2] == image && a.dims[0][3] == image;
      const bool nhwc = a.num_dims[0] == 4 && a.dims[0][1] == image && a.dims[0][2] == image && a.dims[0][3] == 3;
      if (!nchw && !(u8 && nhwc))
        throw std::runtime_error("[ERROR] Tensor layout mismatch: expected [B,3," + sz + "," + sz + "]" +
                                 (u8 ? " or [B," + sz + "," + sz + ",3]" : ""));
    }
    if (in_bytes[0] < (size_t)elems(0) * (u8 ? 1 : 4)) throw std::runtime_error("[ERROR] Input buffer too small");
    expect_out = (size_t)B * m.classes * 4;
    if (const int io = o.image_io) {  // logits (unless NO_LOGITS), probabilities, top-k values, top-k indices
      size_t want[4];
      int n = 0;
      if (!(io & SPI_IMAGE_NO_LOGITS)) want[n++] = expect_out;
      if (io & SPI_IMAGE_OUT_PROBS) want[n++] = expect_out;
      if (io & SPI_IMAGE_OUT_TOPK) {
        want[n++] = (size_t)B * o.top_k * 4;
        i64_out = n;
        want[n++] = (size_t)B * o.top_k * 8;
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
    if (S < 1 || S > m.seq || S > m.maxpos)
      throw std::runtime_error("sequence length " + std::to_string(S) + " exceeds " + std::to_string(m.seq));
    // hidden [B,S,D] unless SPI_BERT_NO_HIDDEN, then the selected [B,D] sentence outputs, then the head's:
    // [B,L] (sequence), [B,S,L] (token) or [B,S] twice (QA)
    const int io = m.bert_io;
    size_t want[5];
    int n = 0;
    if (!(io & SPI_BERT_NO_HIDDEN)) want[n++] = (size_t)B * S * m.D * 4;
    if (io & SPI_BERT_OUT_POOLER) want[n++] = (size_t)B * m.D * 4;
    if (io & SPI_BERT_OUT_MEAN) want[n++] = (size_t)B * m.D * 4;
    if (io & SPI_BERT_HEAD_SEQUENCE) want[n++] = (size_t)B * m.num_labels * 4;
    if (io & SPI_BERT_HEAD_TOKEN) want[n++] = (size_t)B * S * m.num_labels * 4;
    if (io & SPI_BERT_HEAD_QA) want[n++] = (size_t)B * S * 4, want[n++] = (size_t)B * S * 4;
    expect_out = want[0];
    for (int i = 1; i < n; ++i) expect_more[i - 1] = want[i];
  }
  for (int i = 0; i < no; ++i) {
    if (a.output_types[i] != (i == i64_out ? SPI_DTYPE_I64 : SPI_DTYPE_F32))
      throw std::runtime_error("[ERROR] Output type mismatch");
    if (out_bytes[i] != (i == 0 ? expect_out : expect_more[i - 1]))
      throw std::runtime_error("Output buffer size mismatch in bytes");
  }
}

ImageSrc input_kind(const PackedModel& m, const ReplicaOptions& o, const spi_codelet_args& a) {
  ImageSrc src;
  if (!image_family(m) || a.input_types[0] != SPI_DTYPE_U8) return src;
  const int64_t* d = a.dims[0];
  if (o.resize_short) {  // every 8-bit task is resampled, an S x S one too: [B,3,H,W] is NCHW, else [B,H,W,3]
    const bool nchw = d[1] == 3;
    src.kind = nchw ? kSrcU8Nchw : kSrcU8Nhwc;
    src.H = (int)(nchw ? d[2] : d[1]);
    src.W = (int)(nchw ? d[3] : d[2]);
    return src;
  }
  // [B,3,S,S] is NCHW (also when S == 3), else check_io accepted [B,S,S,3]
  src.kind = d[1] == 3 && d[2] == m.image && d[3] == m.image ? kSrcU8Nchw : kSrcU8Nhwc;
  return src;
}

std::string replica_desc(const PackedModel& m, const ReplicaOptions& o) {
  std::string desc = m.desc;
  if (const int io = o.image_io) {
    std::string outs;
    for (const auto& e : {std::make_pair(!(io & SPI_IMAGE_NO_LOGITS), std::string("logits")),
                          std::make_pair((io & SPI_IMAGE_OUT_PROBS) != 0, std::string("probs")),
                          std::make_pair((io & SPI_IMAGE_OUT_TOPK) != 0, "top" + std::to_string(o.top_k))})
      if (e.first) outs += (outs.empty() ? "" : ",") + e.second;
    desc += " out[" + outs + "]";
  }
  if (o.resize_short) desc += " resize" + std::to_string(o.resize_short);
  return desc;
}

int check_input_transform(const PackedModel& m, const float* scale, const float* shift, InputXf& xf) {
  if (!image_family(m)) return SPI_ERR_UNSUPPORTED;
  xf = InputXf{};
  if (scale || shift) {
    if (!scale || !shift) return SPI_ERR_INVALID_ARGUMENT;
    for (int c = 0; c < 3; ++c) {
      if (!std::isfinite(scale[c]) || !std::isfinite(shift[c])) return SPI_ERR_INVALID_ARGUMENT;
      xf.scale[c] = scale[c];
      xf.shift[c] = shift[c];
    }
  }
  return SPI_OK;
}

int check_image_outputs(const PackedModel& m, int io, int top_k, std::string& err) {
  constexpr int known = SPI_IMAGE_OUT_PROBS | SPI_IMAGE_OUT_TOPK | SPI_IMAGE_NO_LOGITS | SPI_IMAGE_TOPK_PROBS;
  auto refuse = [&](int status, const std::string& msg) {
    err = "image outputs: " + msg;
    return status;
  };
  if (!image_family(m))
    return refuse(SPI_ERR_UNSUPPORTED, "only ResNet / ViT replicas have classification outputs");
  if (io & ~known) return refuse(SPI_ERR_INVALID_ARGUMENT, "unknown bits " + std::to_string(io & ~known));
  if ((io & SPI_IMAGE_NO_LOGITS) && !(io & (SPI_IMAGE_OUT_PROBS | SPI_IMAGE_OUT_TOPK)))
    return refuse(SPI_ERR_INVALID_ARGUMENT,
                  "SPI_IMAGE_NO_LOGITS leaves no output; select SPI_IMAGE_OUT_PROBS or SPI_IMAGE_OUT_TOPK");
  if ((io & SPI_IMAGE_TOPK_PROBS) && !(io & SPI_IMAGE_OUT_TOPK))
    return refuse(SPI_ERR_INVALID_ARGUMENT, "SPI_IMAGE_TOPK_PROBS needs SPI_IMAGE_OUT_TOPK");
  if (io & SPI_IMAGE_OUT_TOPK) {
    const int kmax = std::min(m.classes, kSoftmaxTopkMaxK);
    if (top_k < 1 || top_k > kmax)
      return refuse(SPI_ERR_INVALID_ARGUMENT,
                    "top_k " + std::to_string(top_k) + " outside 1 .. min(classes, 64) = " + std::to_string(kmax));
  } else if (top_k != 0) {
    return refuse(SPI_ERR_INVALID_ARGUMENT, "top_k " + std::to_string(top_k) + " without SPI_IMAGE_OUT_TOPK");
  }
  if (io && m.classes > kSoftmaxTopkMaxN)
    return refuse(SPI_ERR_UNSUPPORTED, std::to_string(m.classes) + " classes; at most " +
                                           std::to_string(kSoftmaxTopkMaxN) + " (the row is staged in LDS as fp32)");
  return SPI_OK;
}

int check_input_resize(const PackedModel& m, int resize_short, std::string& err) {
  auto refuse = [&](int status, const std::string& msg) {
    err = "input resize: " + msg;
    return status;
  };
  if (!image_family(m)) return refuse(SPI_ERR_UNSUPPORTED, "only ResNet / ViT replicas take 8-bit image tasks");
  if (resize_short != 0 && (resize_short < m.image || resize_short > kResizeMax))
    return refuse(SPI_ERR_INVALID_ARGUMENT, "resize_short " + std::to_string(resize_short) + " outside " +
                                                std::to_string(m.image) + " (the replica's image size) .. " +
                                                std::to_string(kResizeMax) + "; 0 switches the resize off");
  return SPI_OK;
}

// ---------------------------------------------------------------------------
// Layer descriptors
// ---------------------------------------------------------------------------
namespace {
GemmDesc linear_desc(const LinearW& L, int M, int lda, int ldc) {
  GemmDesc d = dense_desc(M, L.n, L.k, lda, ldc, ldc, L.krep);
  if (d.Kpad != L.kpad) throw std::logic_error("linear_desc: the packed weight rows are not Kpad long");
  d.wplane = L.wplane;
  return d;
}
}  // namespace

GemmDesc conv_layer_desc(const PackedModel& m, const ConvW& c, int B, int H, int W, Act act, bool out_f32,
                         bool res_f32) {
  GemmDesc d = conv_desc(B, H, W, c.cin_pad, c.cout, c.kh, c.kw, c.stride, c.pad, c.krep);
  if (d.Kpad != c.kpad) throw std::logic_error("conv_desc: the packed weight rows are not Kpad long");
  d.w_image = c.w_image;
  d.act = act;
  d.wplane = c.wplane;
  d.out_split = m.split;
  d.a_split = m.split && &c != &m.stem;  // the stem reads the ingested fp32 image
  d.out_f32 = out_f32;
  d.res_f32 = res_f32;
  d.out_f16 = m.f16 && c.prec == Prec::F16X3 && !out_f32;  // F16M stem: F16X3 contraction, fp16 activations
  return d;
}

GemmDesc linear_layer_desc(const LinearW& L, int M) {
  GemmDesc d = linear_desc(L, M, L.k, L.n);
  d.out_f32 = true;
  d.ldr = 0;
  return d;
}

bool pooled_fc(const PackedModel& m, int hw) { return hw > 0 && hw <= 64 && (!m.split || m.feat % 32 == 0); }

GemmDesc pooled_fc_desc(const PackedModel& m, int B, int hw) {
  GemmDesc d = linear_desc(m.fc, B * hw, m.feat, m.classes);
  d.pool_rows = hw;
  d.out_f32 = true;
  d.a_split = m.split;
  return d;
}

// Unfolded, both families: out-proj and FFN2 add the fp32 residual stream and write fp32.
// Folded (ln_fold.hpp): the rows they write are two fp16 planes T x D apart plus
// their chunk statistics (ln_out); FFN1, and QKV from layer 1 on, read pre-LN rows with the
// LayerNorm folded into their weights (ln_in_chunks).  BERT (post-LN) also normalises the residual
// on the fly (res_ln_chunks): out-proj's from layer 1 on -- layer 0 adds the fp32 embedding
// output -- and every FFN2's.
GemmDesc tf_gemm_desc(const PackedModel& m, int layer, TfGemm g, int T) {
  const LinearW& L = tf_linear(m.tf[layer], g);
  const bool wide = g == kQkv || g == kFf1;  // reads the D-wide rows, writes 3 D / FFN columns
  GemmDesc d = linear_desc(L, T, L.k, L.n);
  if (g == kFf1) d.act = Act::Gelu;
  d.ldr = wide ? 0 : L.n;
  const bool fold_in = m.ln_fold && (g == kFf1 || (g == kQkv && layer > 0));
  if (fold_in) {
    if (!L.c1) throw std::runtime_error("LayerNorm fold: the GEMM's weights were not packed folded");
    d.ln_in_chunks = L.k / 64;
    d.ln_in_eps = m.eps;
  }
  if (wide) return d;
  if (!m.ln_fold) {
    d.out_f32 = d.res_f32 = true;
    return d;
  }
  const bool bert = m.family == SPI_FAMILY_BERT;
  d.res_f32 = bert && g == kOut && layer == 0;
  d.out_planes = true;  // C (and an fp16-typed residual) in two fp16 planes `plane` elements apart
  d.res_planes = !d.res_f32;
  d.plane = (size_t)T * L.n;
  if (bert && !d.res_f32) {
    d.res_ln_chunks = L.n / 64;
    d.res_ln_eps = m.eps;
  }
  d.ln_out = true;
  d.ld16 = L.n;
  return d;
}

// ---------------------------------------------------------------------------
// FLOPs
// ---------------------------------------------------------------------------
namespace {
struct FlopsVisitor {
  double f = 0;
  void add(int B, const RnConv& k) {  // a grouped conv: its own FLOPs on either route
    const ConvW& c = k.c;
    const double OH = conv_out(k.H, c);
    f += 2.0 * B * OH * OH * c.cout * (double)c.kh * c.kw * (c.cin / c.groups);
  }
  const PackedModel& m;
  explicit FlopsVisitor(const PackedModel& m_) : m(m_) {}
  void stem(int B, const StemGeom&) { add(B, RnConv{m.stem, m.image, 0, 0, -1}); }
  void conv(int B, const RnConv& k) { add(B, k); }
  void conv_pair(int B, const RnConv& k0, const RnConv& k1) { add(B, k0), add(B, k1); }
  void tail(int B, int, int, bool) { f += 2.0 * B * m.fc.n * m.fc.k; }
};
}  // namespace

double model_flops(const PackedModel& m, int64_t B) {
  if (m.family == SPI_FAMILY_RESNET) {
    FlopsVisitor v(m);
    walk_resnet(m, (int)B, v);
    return v.f;
  }
  double f = 0;
  if (m.family == SPI_FAMILY_BERT || m.family == SPI_FAMILY_VIT) {
    const double S = m.family == SPI_FAMILY_BERT ? m.seq : m.npatch + 1;
    const double T = B * S;
    for (const auto& L : m.tf)
      f += 2.0 * T * ((double)L.qkv.n * L.qkv.k + (double)L.out.n * L.out.k + (double)L.ff1.n * L.ff1.k +
                      (double)L.ff2.n * L.ff2.k) +
           4.0 * B * S * S * m.D;
    if (m.family == SPI_FAMILY_VIT)
      f += 2.0 * B * m.npatch * (double)m.D * m.patch_proj.k + 2.0 * B * m.head.n * m.head.k;
    // the pooler once, as an output or under the sequence head; then the head's dense layer
    if (m.bert_io & (SPI_BERT_OUT_POOLER | SPI_BERT_HEAD_SEQUENCE)) f += 2.0 * B * (double)m.D * m.D;
    if (m.bert_io & SPI_BERT_HEAD_SEQUENCE) f += 2.0 * B * (double)m.D * m.num_labels;
    if (m.bert_io & (SPI_BERT_HEAD_TOKEN | SPI_BERT_HEAD_QA)) f += 2.0 * T * (double)m.D * m.num_labels;
  }
  return f;
}

// ---------------------------------------------------------------------------
// Workspace
// ---------------------------------------------------------------------------
namespace {
// The launches of the ResNet graph, each as the desc(s) Model::body_resnet builds for it: `on_gemm`
// gets (step name, desc, prec, second desc of a pair or null).  Sizing takes the slab maximum from it,
// plan_check holds each against the planned workspace.
template <class F>
struct RnGemmVisitor {
  const PackedModel& m;
  F on_gemm;
  size_t amax = 0;  // elements of the largest map kept in an activation slot
  void stored(int B, int OH, int cout) { amax = std::max(amax, (size_t)B * OH * OH * cout); }
  GemmDesc desc(int B, const RnConv& k, Act act) { return conv_layer_desc(m, k.c, B, k.H, k.H, act); }
  void stem(int B, const StemGeom& g) {
    // (sized under the fused stem too, whose launch needs no slabs: the sizes are the recorded ones)
    on_gemm("stem", desc(B, RnConv{m.stem, m.image, kRnIngest, kRnAct0, -1}, Act::Relu), m.stem.prec, nullptr);
    if (!m.stem_fused) stored(B, g.OH, m.stem.cout);  // fused: the stem's output is never materialised
    stored(B, g.PH, m.stem.cout);
  }
  void conv(int B, const RnConv& k) {
    stored(B, conv_out(k.H, k.c), k.c.cout);
    if (k.c.gconv) return;  // the grouped kernel: no plan, no slabs
    on_gemm("conv", desc(B, k, Act::Relu), k.c.prec, nullptr);
  }
  void conv_pair(int B, const RnConv& k0, const RnConv& k1) {
    stored(B, conv_out(k0.H, k0.c), k0.c.cout);
    stored(B, conv_out(k1.H, k1.c), k1.c.cout);
    const GemmDesc d0 = desc(B, k0, Act::Relu), d1 = desc(B, k1, Act::None);
    if (k0.c.prec == k1.c.prec) return on_gemm("conv_pair", d0, k0.c.prec, &d1);
    on_gemm("conv", d0, k0.c.prec, nullptr);  // two launches (Model::run_conv_pair)
    on_gemm("conv", d1, k1.c.prec, nullptr);
  }
  void tail(int B, int, int hw, bool fused) {
    if (fused) on_gemm("avgpool_fc", pooled_fc_desc(m, B, hw), m.fc.prec, nullptr);
    else on_gemm("fc", linear_layer_desc(m.fc, B), m.fc.prec, nullptr);
  }
};

template <class F>
RnGemmVisitor<F> walk_resnet_gemms(const PackedModel& m, int B, F&& f) {
  RnGemmVisitor<F> v{m, std::forward<F>(f)};
  walk_resnet(m, B, v);
  return v;
}
}  // namespace

WorkspacePlan workspace_plan(const PackedModel& m, const ReplicaOptions& o) {
  WorkspacePlan p;
  std::vector<size_t>& sz = p.bytes;
  size_t& partial = p.partial_planned;
  const size_t B = m.max_batch, D = m.D, es = m.f16 ? 2 : 4;
  const size_t logits = (o.image_io & SPI_IMAGE_NO_LOGITS) ? B * m.classes * 4 : 0;
  const size_t resized = o.resize_short ? B * 3 * m.image * m.image * 4 : 0;
  auto slabs = [&](const GemmDesc& d, Prec prec, const GemmDesc* d1 = nullptr) {
    partial = std::max(partial, d1 ? plan_pair(d, *d1, prec).partial_floats : gemm_partial_floats(d, prec));
  };
  if (m.family == SPI_FAMILY_RESNET) {
    const ConvW& stem = m.stem;
    sz.assign(kRnBufs, 0);
    sz[kRnIngest] = m.stem_fused ? 256 : B * m.image * m.image * stem.cin_pad * (stem.prec == Prec::F16 ? 2 : 4);
    const auto v = walk_resnet_gemms(
        m, (int)B, [&](const char*, const GemmDesc& d, Prec prec, const GemmDesc* d1) { slabs(d, prec, d1); });
    slabs(linear_layer_desc(m.fc, (int)B), m.fc.prec);  // also where avgpool + FC run as one GEMM
    // F16M: the downsample outputs are fp32 in the same pool
    const size_t ea = m.mixed ? 4 : m.f16 ? 2 : 4;
    for (int i = kRnAct0; i <= kRnAct4; ++i) sz[i] = v.amax * ea;
    sz[kRnPooled] = B * m.feat * ea;  // fp32 under F16M: the FC's A
    sz[kRnLogits] = logits;
    sz[kRnResized] = resized;
  } else if (m.family == SPI_FAMILY_BERT) {
    const size_t T = B * m.seq;
    sz.assign(kBtBufs, 0);
    sz[kBtHidden] = T * D * 4;
    sz[kBtHidden16] = T * D * es;
    sz[kBtQkv] = T * 3 * D * es;
    sz[kBtCtx] = T * D * es;
    sz[kBtAttn] = T * D * 4;
    sz[kBtFfn] = T * m.ffn * es;
    sz[kBtStats1] = sz[kBtStats2] = T * (D / 64) * 8;
    sz[kBtCls] = (bert_cls_rows_floats(m) + bert_pooled_ws_floats(m)) * 4;
  } else if (m.family == SPI_FAMILY_VIT) {
    const size_t T = B * (m.npatch + 1);
    sz.assign(kVtBufs, 0);
    sz[kVtPatches] = B * m.npatch * m.patch_proj.k * es + vit_patches_tail_bytes(m);
    sz[kVtProj] = B * m.npatch * D * 4;
    sz[kVtX] = T * D * 4;
    sz[kVtLn] = T * D * es;
    sz[kVtQkv] = T * 3 * D * es;
    sz[kVtCtx] = T * D * es;
    sz[kVtMlp] = T * m.ffn * es;
    sz[kVtCls] = B * D * es;
    sz[kVtStats] = T * (D / 64) * 8;
    sz[kVtLogits] = logits;
    sz[kVtResized] = resized;
  }
  if (m.family == SPI_FAMILY_BERT || m.family == SPI_FAMILY_VIT)
    walk_transformer_gemms(m, (int)B, m.seq, [&](const char*, const LinearW& L, const GemmDesc& d) { slabs(d, L.prec); });
  // Split-K slabs: choose_plan only splits grids of < 128 tiles into <= 512 +
  // tiles workgroups of 64x64, so 640 * 64 * 64 floats bounds every batch size.
  p.partial_floats = std::max(partial, (size_t)640 * 64 * 64);
  return p;
}

int plan_check(const PackedModel& m, const ReplicaOptions& o, int B, int S) {
  if (B < 1 || B > m.max_batch) throw std::runtime_error("plan_check: batch outside 1 .. max_batch");
  const size_t floats = workspace_plan(m, o).partial_floats;
  int steps = 0;
  auto hold = [&](const std::string& what, const GemmDesc& d, Prec prec, const GemmDesc* d1) {
    if (!launch_fits(d, prec, floats, d1))
      throw std::runtime_error("split-K workspace too small: step " + std::to_string(steps) + " (" + what + " M" +
                               std::to_string(d.M) + " N" + std::to_string(d.N) + " K" + std::to_string(d.K) +
                               ") at batch " + std::to_string(B));
    ++steps;
  };
  if (m.family == SPI_FAMILY_RESNET) {
    walk_resnet_gemms(m, B, [&](const char* name, const GemmDesc& d, Prec prec, const GemmDesc* d1) { hold(name, d, prec, d1); });
  } else if (m.family == SPI_FAMILY_BERT || m.family == SPI_FAMILY_VIT) {
    if (m.family == SPI_FAMILY_BERT && (S < 1 || S > m.seq)) throw std::runtime_error("plan_check: sequence outside 1 .. seq");
    walk_transformer_gemms(m, B, S, [&](const char* name, const LinearW& L, const GemmDesc& d) { hold(name, d, L.prec, nullptr); });
  }
  return steps;
}

}  // namespace spi
