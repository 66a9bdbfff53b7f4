// Model replica: upload of the packed blob (model_pack.cpp); per-stream workspaces; launch
// helpers; forward plans for ResNet (basic / bottleneck), BERT (post-LN) and ViT (pre-LN).
// Reference counterparts: the per-device clones (src/core/inference_runner.cpp:251-275) and the
// forward that LibTorch runs inside the codelet (src/core/starpu_setup.cpp:610).
#include "gconv.hpp"
#include "model.hpp"

#include <cmath>
#include <cstdlib>

namespace spi {

// Graph capture vs allocation: a hipMalloc on one worker thread while another
// thread's stream is capturing invalidates that capture ("operation failed due
// to a previous error during capture").  Workspace allocation and graph capture
// therefore never overlap, process-wide (all replicas, all worker threads).
std::mutex g_capture_mu;

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
    : device_(device), m_(pack_model(cfg, params, n)), desc_(m_.desc) {
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
// Options: the argument checks are model_plan.cpp's; the lock, the refusal once a stream
// workspace exists and the assignment are here
// ---------------------------------------------------------------------------
int Model::set_input_transform(const float* scale, const float* shift) {
  InputXf xf;
  const int st = check_input_transform(m_, scale, shift, xf);
  if (st == SPI_OK) input_xf_ = xf;
  return st;
}

template <typename F>
int Model::set_options(const char* what, std::string& err, F&& assign) {
  std::lock_guard<std::mutex> lk(mu_);
  if (!ws_.empty()) {
    err = std::string(what) + ": a stream workspace of the replica exists; call before the first forward or warm-up";
    return SPI_ERR_INVALID_ARGUMENT;
  }
  assign(opt_);
  desc_ = replica_desc(m_, opt_);
  return SPI_OK;
}

int Model::set_image_outputs(int io, int top_k, std::string& err) {
  if (const int st = check_image_outputs(m_, io, top_k, err); st != SPI_OK) return st;
  return set_options("image outputs", err, [&](ReplicaOptions& o) { o.image_io = io, o.top_k = top_k; });
}

int Model::set_input_resize(int resize_short, std::string& err) {
  if (const int st = check_input_resize(m_, resize_short, err); st != SPI_OK) return st;
  return set_options("input resize", err, [&](ReplicaOptions& o) { o.resize_short = resize_short; });
}

// ---------------------------------------------------------------------------
// Launch helpers: a finished desc (model_plan.hpp) plus pointers, FLOPs and bytes
// ---------------------------------------------------------------------------
namespace {
std::string conv_name(const ConvW& c, int M) {
  return "conv" + std::to_string(c.kh) + "x" + std::to_string(c.kw) + "_c" + std::to_string(c.cin) + "_k" +
         std::to_string(c.cout) + "_s" + std::to_string(c.stride) + "_M" + std::to_string(M);
}

void require_fit(const GemmDesc& d, Prec prec, const Workspace& ws, const GemmDesc* d1 = nullptr) {
  if (!launch_fits(d, prec, ws.partial_floats, d1)) throw std::runtime_error("split-K workspace too small");
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

Model::ConvCall Model::conv_call(const ConvW& c, const GemmDesc& d, const void* x, void* y, const void* res,
                                 const Workspace& ws) const {
  ConvCall k;
  const size_t es = m_.f16 ? 2 : 4;
  const double in_px = (double)(d.M / (d.OH * d.OW)) * d.H * d.W;
  k.flops = 2.0 * d.M * d.N * (double)c.kh * c.kw * c.cin;
  k.bytes = in_px * c.cin_pad * es + (double)c.cout * d.K * es + (double)d.M * d.N * es * (res ? 2 : 1);
  k.p = gemm_ptrs(x, c.w, c.b, res, y, ws);
  return k;
}

void Model::run_conv(const ConvW& c, const GemmDesc& d, const void* x, void* y, const void* res, Workspace& ws,
                     hipStream_t s) {
  const ConvCall k = conv_call(c, d, x, y, res, ws);
  require_fit(d, c.prec, ws);
  prof_op(s, [&] { return conv_name(c, d.M); }, k.flops, k.bytes, [&] { gemm(d, k.p, c.prec, s); });
}

// A grouped conv packed for the grouped kernel (ConvW::gconv; conv_group.hip): no GEMM plan, no
// split-K workspace.  flops: the conv's own (1 / groups of the dense count).
void Model::run_gconv(const ConvW& c, const void* x, int B, int H, void* y, Act act, hipStream_t s) {
  const int OH = conv_out(H, c), M = B * OH * OH;
  prof_op(s,
          [&] {
            return "gconv3x3_c" + std::to_string(c.cout) + "_g" + std::to_string(c.groups) + "_s" +
                   std::to_string(c.stride) + "_M" + std::to_string(M);
          },
          2.0 * M * c.cout * 9.0 * (c.cin / c.groups),
          ((double)B * H * H * c.cin + (double)M * c.cout) * 2 + (double)gconv_packed_bytes(c.cout, c.groups),
          [&] { conv_group(x, ptr<void>(c.w), ptr<float>(c.b), y, B, H, H, c.cout, c.groups, c.stride, act == Act::Relu, s); });
}

// A block's first conv and its downsample conv read the same input: one grouped
// launch (gemm_pair) instead of two dependent ones.
void Model::run_conv_pair(const void* x, const ConvW& c0, const GemmDesc& d0, void* y0, const ConvW& c1,
                          const GemmDesc& d1, void* y1, Workspace& ws, hipStream_t s) {
  if (c0.prec != c1.prec) {
    run_conv(c0, d0, x, y0, nullptr, ws, s);
    run_conv(c1, d1, x, y1, nullptr, ws, s);
    return;
  }
  const ConvCall k0 = conv_call(c0, d0, x, y0, nullptr, ws), k1 = conv_call(c1, d1, x, y1, nullptr, ws);
  require_fit(d0, c0.prec, ws, &d1);
  prof_op(s, [&] { return conv_name(c0, d0.M) + "+" + conv_name(c1, d1.M); }, k0.flops + k1.flops,
          k0.bytes + k1.bytes, [&] { gemm_pair(d0, k0.p, d1, k1.p, c0.prec, s); });
}

// ln: the statistics / gain / bias pointers of the LayerNorm fold the desc asks for (c1 is the layer's own)
void Model::run_gemm(const LinearW& L, const GemmDesc& d, const void* A, void* C, const void* res, const LnPtrs& ln,
                     Workspace& ws, hipStream_t s) {
  if ((d.ln_in_chunks > 0) != (ln.in_stats != nullptr) || (d.res_ln_chunks > 0) != (ln.res_stats != nullptr) ||
      d.ln_out != (ln.out_stats != nullptr))
    throw std::logic_error("run_gemm: the LayerNorm-fold pointers are not the ones the desc asks for");
  GemmPtrs p = gemm_ptrs(A, L.w, L.b, res, C, ws);
  p.ln = ln;
  if (d.ln_in_chunks) p.ln.c1 = ptr<float>(L.c1);
  require_fit(d, L.prec, ws);
  const size_t es = m_.f16 ? 2 : 4;
  const double MN = (double)d.M * d.N;
  prof_op(s, [&] { return "gemm_M" + std::to_string(d.M) + "_N" + std::to_string(d.N) + "_K" + std::to_string(d.K); },
          2.0 * d.M * d.N * (double)d.K,
          (double)d.M * d.K * es + (double)d.N * d.K * es + MN * (d.out_f32 || d.out_planes ? 4 : es) +
              (res ? MN * (d.res_f32 || d.out_planes ? 4 : es) : 0.0),
          [&] { gemm(d, p, L.prec, s); });
}

void Model::run_tf_gemm(int layer, TfGemm g, int T, const void* A, void* C, const void* res, Workspace& ws,
                        hipStream_t s, const LnPtrs& ln) {
  run_gemm(tf_linear(m_.tf[layer], g), tf_gemm_desc(m_, layer, g, T), A, C, res, ln, ws, s);
}

void Model::run_qkv_attention(int layer, const void* x, const float* in_stats, void* qkv, void* ctx, int B, int S,
                              Workspace& w, hipStream_t s) {
  const LinearW& L = m_.tf[layer].qkv;
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
  LnPtrs ln;
  ln.in_stats = in_stats;
  run_tf_gemm(layer, kQkv, T, x, qkv, nullptr, w, s, ln);
  prof_op(s, [&] { return "attention_S" + std::to_string(S); }, 4.0 * B * S * S * D,
          (double)T * 4 * D * (m_.f16 ? 2 : 4), [&] { attention(qkv, mask, ctx, B, S, heads, hd, scale, m_.f16, s); });
}

void Model::run_pooled_fc(const void* act, int B, int hw, void* out, Workspace& ws, hipStream_t s) {
  const LinearW& fc = m_.fc;
  const int classes = m_.classes, feat = m_.feat;
  const GemmDesc d = pooled_fc_desc(m_, B, hw);
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
Workspace* Model::workspace(hipStream_t s) {
  std::lock_guard<std::mutex> lk(mu_);
  auto it = ws_.find(s);
  if (it != ws_.end()) return it->second.get();
  std::lock_guard<std::mutex> cap(g_capture_mu);
  auto w = std::make_unique<Workspace>();
  const WorkspacePlan plan = workspace_plan(m_, opt_);  // bytes per buffer; the split-K slabs with their floor
  if (m_.family == SPI_FAMILY_BERT) SPI_HIP(hipMalloc(&w->mask_bias, (size_t)m_.max_batch * m_.seq * sizeof(float)));
  for (size_t bytes : plan.bytes) {
    void* b = nullptr;
    SPI_HIP(hipMalloc(&b, std::max<size_t>(bytes, 256)));
    w->bufs.push_back(b);
  }
  // ViT patch rows that are no whole number of 16-byte chunks (vit_patches_tail_bytes): the patch
  // projection's last A chunk of a row runs into the row behind it, against zero weights -- so what lies
  // behind a task's last row, another task's rows or the buffer's tail, must be finite from the start.
  // Stream-ordered, like the tickets below; patchify writes whole rows only, so the tail stays zero.
  if (vit_patches_tail_bytes(m_))
    SPI_HIP(hipMemsetAsync(w->bufs[kVtPatches], 0, plan.bytes[kVtPatches], s));
  w->partial_floats = plan.partial_floats;
  SPI_HIP(hipMalloc(&w->partial, plan.partial_floats * sizeof(float)));
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
  const int OH = stem_geom(m_).OH, PH = stem_geom(m_).PH;
  prof_op(s, "stem_pool", 2.0 * B * OH * OH * stem.cout * 147.0,
          (double)B * 3 * image * image * 4 + (double)B * PH * PH * stem.cout * (m_.split ? 4 : 2), [&] {
            stem_pool(x, ptr<void>(m_.stem_pool_w), ptr<float>(stem.b), w.bufs[kRnAct1], B, image, image,
                      m_.split ? 2 : stem.prec != Prec::F16 ? 1 : 0, m_.split, stem_pr_, s, src, input_xf_);
          });
}

// The launching visitor of walk_resnet (model_plan.hpp).
void Model::body_resnet(Workspace& w, int B, hipStream_t s) {
  struct Launch {
    Model& M;
    Workspace& w;
    hipStream_t s;
    const PackedModel& m = M.m_;
    void* const* buf = w.bufs.data();
    GemmDesc desc(int B, const RnConv& k, Act act) const { return conv_layer_desc(m, k.c, B, k.H, k.H, act); }
    void stem(int B, const StemGeom& g) {
      if (m.stem_fused) return;  // stem + max pool ran in the prologue
      const ConvW& stem = m.stem;
      const int H = g.OH, PH = g.PH;
      M.run_conv(stem, desc(B, RnConv{stem, m.image, kRnIngest, kRnAct0, -1}, Act::Relu), buf[kRnIngest], buf[kRnAct0],
                 nullptr, w, s);
      M.prof_op(s, "maxpool", 0, (double)B * (H * H + PH * PH) * stem.cout * (m.f16 ? 2 : 4), [&] {
        if (m.split)
          maxpool_nhwc_split(buf[kRnAct0], buf[kRnAct1], B, H, H, stem.cout, PH, PH, 3, 2, 1, s);
        else
          maxpool_nhwc(buf[kRnAct0], buf[kRnAct1], B, H, H, stem.cout, PH, PH, 3, 2, 1, m.f16, s);
      });
    }
    void conv(int B, const RnConv& k) {
      if (k.c.gconv) return M.run_gconv(k.c, buf[k.in], B, k.H, buf[k.out], Act::Relu, s);
      M.run_conv(k.c, desc(B, k, Act::Relu), buf[k.in], buf[k.out], k.res < 0 ? nullptr : buf[k.res], w, s);
    }
    // F16M: the downsample's hi + lo weights, fp16 out like every conv (round 5: fp32 out kept nothing)
    void conv_pair(int B, const RnConv& k0, const RnConv& k1) {
      M.run_conv_pair(buf[k0.in], k0.c, desc(B, k0, Act::Relu), buf[k0.out], k1.c, desc(B, k1, Act::None), buf[k1.out],
                      w, s);
    }
    void tail(int B, int slot, int hw, bool fused) {
      w.final_buf = slot;
      w.final_hw = hw;
      if (fused) return;  // avgpool + fc run as one GEMM in the epilogue
      M.prof_op(s, "avgpool", 0, (double)B * hw * m.feat * (m.f16 ? 2 : 4), [&] {
        if (m.split)  // fp32 for the F16X3 FC (as under F16M below)
          avgpool_nhwc_split(buf[slot], static_cast<float*>(buf[kRnPooled]), B, hw, m.feat, s);
        else
          avgpool_nhwc(buf[slot], buf[kRnPooled], B, hw, m.feat, m.f16, s, m.mixed);
      });
      w.final_buf = kRnPooled;
    }
  };
  walk_resnet(m_, B, Launch{*this, w, s});
}

// ---------------------------------------------------------------------------
// BERT plan (post-LN)
// ---------------------------------------------------------------------------
void Model::body_bert(Workspace& w, int B, int S, hipStream_t s) {
  if (m_.ln_fold) return body_bert_folded(w, B, S, s);
  const int D = m_.D, T = B * S;
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
    run_qkv_attention(i, ht, nullptr, w.bufs[kBtQkv], w.bufs[kBtCtx], B, S, w, s);
    run_tf_gemm(i, kOut, T, w.bufs[kBtCtx], a, hf, w, s);
    ln(L.ln1);
    run_tf_gemm(i, kFf1, T, ht, ff, nullptr, w, s);
    run_tf_gemm(i, kFf2, T, ff, a, hf, w, s);
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
  const int T = B * S;
  float* hf = static_cast<float*>(w.bufs[kBtHidden]);
  void* ht = w.bufs[kBtHidden16];
  void* ctx = w.bufs[kBtCtx];
  void* ff = w.bufs[kBtFfn];
  float* S1 = static_cast<float*>(w.bufs[kBtStats1]);
  float* S2 = static_cast<float*>(w.bufs[kBtStats2]);
  _Float16* bh = static_cast<_Float16*>(w.bufs[kBtHidden]);
  _Float16* ah = static_cast<_Float16*>(w.bufs[kBtAttn]);
  auto res_ln = [&](const float* stats, const LnW& l) {  // the residual is LN(rows) from their statistics
    LnPtrs p;
    p.res_stats = stats;
    p.res_g = ptr<float>(l.g);
    p.res_b = ptr<float>(l.b);
    return p;
  };
  for (int i = 0; i < m_.layers; ++i) {
    const TfLayer& L = m_.tf[i];
    run_qkv_attention(i, i > 0 ? bh : ht, i > 0 ? S2 : nullptr, w.bufs[kBtQkv], ctx, B, S, w, s);
    LnPtrs o = i > 0 ? res_ln(S2, m_.tf[i - 1].ln2) : LnPtrs{};
    o.out_stats = S1;
    run_tf_gemm(i, kOut, T, ctx, ah, i > 0 ? static_cast<void*>(bh) : hf, w, s, o);
    LnPtrs f1;
    f1.in_stats = S1;
    run_tf_gemm(i, kFf1, T, ah, ff, nullptr, w, s, f1);
    LnPtrs f2 = res_ln(S1, L.ln1);
    f2.out_stats = S2;
    run_tf_gemm(i, kFf2, T, ff, bh, ah, w, s, f2);
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
  // The task head (SPI_BERT_HEAD_*) writes last.  The sequence head reads the pooled vector, so it runs
  // the pooler whether or not that is an output.  A token-level head (token, QA) reads every normalised
  // row: the hidden output's or the mean's where one of them is written anyway, else the pre-LN2 rows
  // themselves, normalised in the head kernel's registers -- then no LayerNorm launch covers all rows.
  const bool seq_head = (io & SPI_BERT_HEAD_SEQUENCE) != 0, tok_head = (io & (SPI_BERT_HEAD_TOKEN | SPI_BERT_HEAD_QA)) != 0;
  const bool pooled = pooler || seq_head;
  const bool cls_only = !hidden && !mean;  // no launch needs all rows normalised in memory
  const int L = m_.num_labels;
  int o = 0;
  float* rows = hidden     ? static_cast<float*>(out[o++])
                : cls_only ? static_cast<float*>(w.bufs[kBtCls])
                           : static_cast<float*>(w.bufs[m_.ln_fold ? kBtAttn : kBtHidden]);
  const int nrows = cls_only ? B : T, ldx = cls_only ? S * D : D;
  if (!cls_only || pooled)
    prof_op(s, cls_only ? "layernorm_cls" : "layernorm_out", 0, (double)nrows * D * 8, [&] {
      // the last layer's pre-LN2 rows: the two-plane b under the LayerNorm fold, else a
      if (m_.ln_fold)
        layernorm_planes(static_cast<const _Float16*>(w.bufs[kBtHidden]), (size_t)T * D, ldx, ptr<float>(l.g),
                         ptr<float>(l.b), rows, nullptr, D, nrows, D, m_.eps, m_.f16, s);
      else
        layernorm(static_cast<float*>(w.bufs[kBtAttn]), ldx, ptr<float>(l.g), ptr<float>(l.b), rows, nullptr, D, nrows,
                  D, m_.eps, m_.f16, s);
    });
  float* pool_y = nullptr;
  if (pooled) {
    // an output, or the workspace place behind the class-token rows (model_plan.hpp: kBtCls' two parts)
    pool_y = pooler ? static_cast<float*>(out[o++]) : static_cast<float*>(w.bufs[kBtCls]) + bert_cls_rows_floats(m_);
    prof_op(s, "bert_pooler", 2.0 * B * D * (double)D, (double)D * D * 4 + (double)B * D * 8, [&] {
      bert_pooler(rows, cls_only ? (size_t)D : (size_t)S * D, ptr<float>(m_.pool_w), ptr<float>(m_.pool_b), pool_y, B, D, s);
    });
  }
  if (mean) {
    float* y = static_cast<float*>(out[o++]);
    prof_op(s, "bert_mean_pool", 2.0 * T * D, (double)T * D * 4 + (double)B * D * 4, [&] {
      masked_mean(rows, w.has_mask ? w.mask_ids : nullptr, y, B, S, D, s);
    });
  }
  if (seq_head) {
    float* y = static_cast<float*>(out[o++]);
    prof_op(s, "bert_seq_head", 2.0 * B * D * (double)L, (double)L * D * 4 + (double)B * (D + L) * 4, [&] {
      bert_dense_rows(pool_y, (size_t)D, ptr<float>(m_.head_w), ptr<float>(m_.head_b), y, B, D, L, false, s);
    });
  }
  if (tok_head) {
    float* y0 = static_cast<float*>(out[o++]);
    float* y1 = (io & SPI_BERT_HEAD_QA) ? static_cast<float*>(out[o++]) : nullptr;
    const double flops = 2.0 * T * D * (double)L, wy = (double)L * D * 4 + (double)T * L * 4;
    if (!cls_only)
      prof_op(s, "bert_token_head", flops, (double)T * D * 4 + wy, [&] {
        bert_token_head(kHeadSrcRows, rows, 0, nullptr, nullptr, 0.f, ptr<float>(m_.head_w), ptr<float>(m_.head_b), y0,
                        y1, T, D, L, s);
      });
    else  // fused with the last LayerNorm: the fold's two-plane b, else the fp32 rows a
      prof_op(s, "bert_ln_token_head", flops, (double)T * D * 4 + wy, [&] {
        bert_token_head(m_.ln_fold ? kHeadSrcPlanes : kHeadSrcPreLn, w.bufs[m_.ln_fold ? kBtHidden : kBtAttn],
                        (size_t)T * D, ptr<float>(l.g), ptr<float>(l.b), m_.eps, ptr<float>(m_.head_w),
                        ptr<float>(m_.head_b), y0, y1, T, D, L, s);
      });
  }
}

// ---------------------------------------------------------------------------
// ViT plan (pre-LN)
// ---------------------------------------------------------------------------
void Model::body_vit(Workspace& w, int B, hipStream_t s) {
  const int D = m_.D, npatch = m_.npatch, S = npatch + 1, T = B * S;
  const bool f16 = m_.f16;
  void* const* buf = w.bufs.data();
  run_gemm(m_.patch_proj, linear_layer_desc(m_.patch_proj, B * npatch), buf[kVtPatches], buf[kVtProj], nullptr, LnPtrs{},
           w, s);
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
  for (int i = 0; i < m_.layers; ++i) {
    const TfLayer& L = m_.tf[i];
    ln("layernorm", L.ln1, D, T, buf[kVtLn]);
    run_qkv_attention(i, buf[kVtLn], nullptr, buf[kVtQkv], buf[kVtCtx], B, S, w, s);
    run_tf_gemm(i, kOut, T, buf[kVtCtx], x, x, w, s);
    ln("layernorm", L.ln2, D, T, buf[kVtLn]);
    run_tf_gemm(i, kFf1, T, buf[kVtLn], buf[kVtMlp], nullptr, w, s);
    run_tf_gemm(i, kFf2, T, buf[kVtMlp], x, x, w, s);
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
  const int D = m_.D, npatch = m_.npatch, S = npatch + 1, T = B * S;
  void* const* buf = w.bufs.data();
  float* Sx = static_cast<float*>(buf[kVtStats]);
  _Float16* xh = static_cast<_Float16*>(buf[kVtX]);
  const size_t plane = (size_t)T * D;
  prof_op(s, "vit_assemble", 0, (double)T * D * 4 * 3, [&] {
    vit_assemble_planes(static_cast<const float*>(buf[kVtProj]), ptr<float>(m_.cls), ptr<float>(m_.vpos), xh, plane,
                        nullptr, B, npatch, D, s);
  });
  LnPtrs o, f1;  // out-proj and FFN2 write x's statistics; FFN1 (and QKV from layer 1 on) read them
  o.out_stats = Sx;
  f1.in_stats = Sx;
  for (int i = 0; i < m_.layers; ++i) {
    const TfLayer& L = m_.tf[i];
    if (i == 0)
      prof_op(s, "layernorm", 0, ln_bytes(T, false), [&] {
        layernorm_planes(xh, plane, D, ptr<float>(L.ln1.g), ptr<float>(L.ln1.b), nullptr, buf[kVtLn], D, T, D, m_.eps,
                         m_.f16, s);
      });
    run_qkv_attention(i, i == 0 ? buf[kVtLn] : xh, i == 0 ? nullptr : Sx, buf[kVtQkv], buf[kVtCtx], B, S, w, s);
    run_tf_gemm(i, kOut, T, buf[kVtCtx], xh, xh, w, s, o);
    run_tf_gemm(i, kFf1, T, xh, buf[kVtMlp], nullptr, w, s, f1);
    run_tf_gemm(i, kFf2, T, buf[kVtMlp], xh, xh, w, s, o);
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
    if (!opt_.resize_short) throw std::logic_error("prologue: a resized source without the input resize");
    float* y = static_cast<float*>(w.bufs[m_.family == SPI_FAMILY_RESNET ? (int)kRnResized : (int)kVtResized]);
    prof_op(s, "resize_crop_u8", 0, (double)B * 3 * ((double)isrc.H * isrc.W + (double)image * image * 4), [&] {
      resize_crop_u8(in[0], src == kSrcU8Nhwc, B, isrc.H, isrc.W, opt_.resize_short, image, input_xf_, y, s);
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
      // SPI_BERT_POS_FROM_IDS: row (b, s) also reads its sequence's ids up to s, 8 (S + 1) / 2 bytes on average
      const double ids_reread = m_.pos_from_ids ? T * 4 * (S + 1) : 0;
      return prof_op(s, "bert_embed", 0, T * D * (4 * 3 + 4 + (f16 ? 2 : 0)) + (w.has_mask ? T * 12 : 0) + (types ? T * 8 : 0) + ids_reread, [&] {
        bert_embed(static_cast<const int64_t*>(in[0]), ptr<float>(m_.word), ptr<float>(m_.pos),
                   ptr<float>(typed ? m_.type_table : m_.type0), ptr<float>(m_.emb_ln.g), ptr<float>(m_.emb_ln.b),
                   static_cast<float*>(w.bufs[kBtHidden]), f16 ? w.bufs[kBtHidden16] : nullptr, B, S, D, m_.vocab,
                   m_.eps, f16, s, w.has_mask ? w.mask_ids : nullptr, w.has_mask ? w.mask_bias : nullptr, types,
                   m_.type_vocab, m_.pos_from_ids);
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
// scratch under SPI_IMAGE_NO_LOGITS); with image outputs selected one more launch derives the other outputs.
void Model::epilogue(Workspace& w, int B, int S, void* const* out, hipStream_t s) {
  switch (m_.family) {
    case SPI_FAMILY_RESNET: {
      float* logits = logits_dst(w.bufs[kRnLogits], out);
      if (pooled_fc(m_, w.final_hw))
        run_pooled_fc(w.bufs[w.final_buf], B, w.final_hw, logits, w, s);
      else
        run_gemm(m_.fc, linear_layer_desc(m_.fc, B), w.bufs[kRnPooled], logits, nullptr, LnPtrs{}, w, s);
      return run_image_outputs(logits, B, out, s);
    }
    case SPI_FAMILY_BERT: return epilogue_bert(w, B, S, out, s);
    case SPI_FAMILY_VIT: {
      float* logits = logits_dst(w.bufs[kVtLogits], out);
      run_gemm(m_.head, linear_layer_desc(m_.head, B), w.bufs[kVtCls], logits, nullptr, LnPtrs{}, w, s);
      return run_image_outputs(logits, B, out, s);
    }
  }
}

// The outputs image_io selects beside the logits, in the order probabilities, top-k values, top-k
// indices: one launch (classify.hip), none with only the logits selected.
void Model::run_image_outputs(const float* logits, int B, void* const* out, hipStream_t s) {
  const int io = opt_.image_io, N = m_.classes, k = opt_.top_k;
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
