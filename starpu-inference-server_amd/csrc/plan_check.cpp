// Stand-alone check of the host-only forward plans (make plan_check): packs pack_check's three small
// models (same closed-form tensors) in every precision and, for each, counts the FLOPs, plans the
// workspace, walks the forward at every batch 1 .. max_batch against it (plan_check: the checks of each
// launch, with no launch) and holds one accepted and one refused task against the I/O contract; prints
// one line per model; then the BERT with task heads (SPI_BERT_HEAD_*): output counts up to five, their byte
// sizes, the pooled vector's place in the workspace.  Built with the address and undefined-behaviour
// sanitizers, no HIP.
#include <cstdio>
#include <deque>
#include <initializer_list>
#include <stdexcept>

#include "model_plan.hpp"

namespace spi {
// the kernel files' knob readers, which gemm_plan.cpp's spi_debug_gemm_reload_env calls; no kernels here
void conv_wres_reload_env() {}
void attention_reload_env() {}
void qkv_attn_reload_env() {}
}  // namespace spi

struct Tensors {
  std::deque<std::string> names;
  std::deque<std::vector<float>> data;
  std::vector<spi_named_tensor> t;
  void add(const std::string& name, std::initializer_list<int64_t> shape) {
    uint32_t crc = ~0u;  // zlib's crc32 of the name
    for (unsigned char ch : name) {
      crc ^= ch;
      for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    crc = ~crc;
    int64_t n = 1;
    for (int64_t d : shape) n *= d;
    const bool var = name.size() >= 11 && name.compare(name.size() - 11, 11, "running_var") == 0;
    const bool gain = shape.size() == 1 && name.size() >= 7 && name.compare(name.size() - 7, 7, ".weight") == 0;
    std::vector<float> v((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t h = (uint32_t)((uint64_t)i * 2654435761ull + crc);
      const double u = (double)(h >> 8) / 16777216.0 - 0.5;
      v[(size_t)i] = (float)(var ? u + 1.0 : gain ? u * 0.25 + 1.0 : u * 0.125);
    }
    names.push_back(name);
    data.push_back(std::move(v));
    spi_named_tensor nt{names.back().c_str(), data.back().data(), SPI_DTYPE_F32, (int32_t)shape.size(), {}};
    int k = 0;
    for (int64_t d : shape) nt.shape[k++] = d;
    t.push_back(nt);
  }
  void norm(const std::string& p, int64_t c, bool bn) {  // LayerNorm, or BatchNorm with running statistics
    for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"})
      if (bn || s[1] != 'r') add(p + s, {c});
  }
  void linear(const std::string& p, int64_t n, int64_t k) { add(p + ".weight", {n, k}), add(p + ".bias", {n}); }
};

// One task of B inputs of `dims` (after the batch) and one output of out_bytes: whether check_io takes it.
static bool accepted(const spi::PackedModel& m, const spi::ReplicaOptions& o, int32_t in_type, int64_t B,
                     std::initializer_list<int64_t> dims, size_t elem, size_t out_bytes) {
  spi_codelet_args a{};
  a.num_inputs = a.num_outputs = 1;
  a.input_types[0] = in_type;
  a.output_types[0] = SPI_DTYPE_F32;
  a.dims[0][0] = B;
  a.num_dims[0] = 1;
  size_t in_bytes = (size_t)B * elem;
  for (int64_t d : dims) a.dims[0][a.num_dims[0]++] = d, in_bytes *= (size_t)d;
  try {
    spi::check_io(m, o, a, &in_bytes, &out_bytes);
    (void)spi::input_kind(m, o, a);
    return true;
  } catch (const std::runtime_error&) {
    return false;
  }
}

int main() {
  Tensors rn, bt, vt;
  rn.add("conv1.weight", {64, 3, 7, 7}), rn.norm("bn1", 64, true);
  for (int64_t L = 1, cin = 64; L <= 4; ++L) {
    const int64_t c = 32 << L;
    const std::string p = "layer" + std::to_string(L) + ".0.";
    rn.add(p + "conv1.weight", {c, cin, 3, 3}), rn.norm(p + "bn1", c, true);
    rn.add(p + "conv2.weight", {c, c, 3, 3}), rn.norm(p + "bn2", c, true);
    if (L > 1) rn.add(p + "downsample.0.weight", {c, cin, 1, 1}), rn.norm(p + "downsample.1", c, true);
    cin = c;
  }
  rn.linear("fc", 1000, 512);
  bt.add("bert.embeddings.word_embeddings.weight", {64, 128}), bt.add("bert.embeddings.position_embeddings.weight", {32, 128});
  bt.add("bert.embeddings.token_type_embeddings.weight", {2, 128}), bt.norm("bert.embeddings.LayerNorm", 128, false);
  vt.add("conv_proj.weight", {128, 3, 16, 16}), vt.add("conv_proj.bias", {128}), vt.add("class_token", {1, 1, 128});
  vt.add("encoder.pos_embedding", {1, 5, 128}), vt.norm("encoder.ln", 128, false), vt.linear("heads.head", 10, 128);
  for (int i = 0; i < 2; ++i) {
    const std::string b = "bert.encoder.layer." + std::to_string(i) + ".", v = "encoder.layers.encoder_layer_" + std::to_string(i) + ".";
    for (const char* n : {"query", "key", "value"}) bt.linear(b + "attention.self." + n, 128, 128);
    bt.linear(b + "attention.output.dense", 128, 128), bt.norm(b + "attention.output.LayerNorm", 128, false);
    bt.linear(b + "intermediate.dense", 256, 128), bt.linear(b + "output.dense", 128, 256), bt.norm(b + "output.LayerNorm", 128, false);
    vt.norm(v + "ln_1", 128, false), vt.norm(v + "ln_2", 128, false);
    vt.add(v + "self_attention.in_proj_weight", {384, 128}), vt.add(v + "self_attention.in_proj_bias", {384});
    vt.linear(v + "self_attention.out_proj", 128, 128), vt.linear(v + "mlp.0", 256, 128), vt.linear(v + "mlp.3", 128, 256);
  }
  struct Case { const char* name; Tensors* t; int heads, seq, image; } cases[] = {
      {"resnet_basic", &rn, 0, 0, 64}, {"bert_d128", &bt, 2, 16, 0}, {"vit_d128", &vt, 2, 0, 32},
      {"bert_d128_h4", &bt, 4, 16, 0}, {"vit_d128_h4", &vt, 4, 0, 32}};  // the last two: 32-wide heads
  const struct { const char* name; int prec; } precs[] = {{"fp16", SPI_PREC_F16}, {"fp16x3", SPI_PREC_F16X3}, {"fp16m", SPI_PREC_F16M}};
  int rc = 0;
  for (const Case& c : cases)
    for (const auto& pr : precs) {
      spi_model_config cfg{};
      cfg.family = SPI_FAMILY_AUTO, cfg.precision = pr.prec, cfg.max_batch = 8;
      cfg.num_heads = c.heads, cfg.seq_len = c.seq, cfg.image_size = c.image;
      const spi::PackedModel m = spi::pack_model(cfg, c.t->t.data(), (int)c.t->t.size());
      const bool bert = m.family == SPI_FAMILY_BERT;
      spi::ReplicaOptions o;
      std::string err;
      if (!bert) {  // the sizes that depend on the options: logits scratch, resampled image
        if (spi::check_image_outputs(m, SPI_IMAGE_OUT_PROBS | SPI_IMAGE_NO_LOGITS, 0, err) != SPI_OK ||
            spi::check_input_resize(m, 2 * m.image, err) != SPI_OK ||
            spi::check_image_outputs(m, SPI_IMAGE_NO_LOGITS, 0, err) == SPI_OK ||
            spi::check_input_resize(m, m.image - 1, err) == SPI_OK) {
          std::fprintf(stderr, "%s|%s: option checks: %s\n", c.name, pr.name, err.c_str());
          rc = 1;
        }
        o.resize_short = 2 * m.image;
      }
      const spi::WorkspacePlan plan = spi::workspace_plan(m, o);
      size_t bytes = 0;
      for (size_t b : plan.bytes) bytes += b;
      int steps = 0;
      try {
        for (int B = 1; B <= m.max_batch; ++B)
          for (int S : {1, m.seq / 2 + 1, m.seq})
            if (bert || S == m.seq) steps += spi::plan_check(m, o, B, S);
      } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s|%s: %s\n", c.name, pr.name, e.what());
        rc = 1;
      }
      // one accepted and one refused task: BERT [2,16] ids (then 17 tokens); an image of the replica's size
      // (then one row short; with the resize on, an 8-bit source of any size is accepted too)
      const size_t out = bert ? (size_t)2 * 16 * m.D * 4 : (size_t)2 * m.classes * 4;
      const bool ok = bert ? accepted(m, o, SPI_DTYPE_I64, 2, {16}, 8, out) && !accepted(m, o, SPI_DTYPE_I64, 2, {17}, 8, out)
                           : accepted(m, o, SPI_DTYPE_F32, 2, {3, m.image, m.image}, 4, out) &&
                                 !accepted(m, o, SPI_DTYPE_F32, 2, {3, m.image - 1, m.image}, 4, out) &&
                                 accepted(m, o, SPI_DTYPE_U8, 2, {100, 75, 3}, 1, out) &&
                                 !accepted(m, o, SPI_DTYPE_U8, 2, {100, 75, 4}, 1, out);
      if (!ok) {
        std::fprintf(stderr, "%s|%s: check_io took a refused task or refused an accepted one\n", c.name, pr.name);
        rc = 1;
      }
      std::printf("%s|%s| flops(1) %.0f flops(3) %.0f workspace %zu bytes in %zu buffers, slabs %zu (planned %zu), %d steps fit, %s\n",
                  c.name, pr.name, spi::model_flops(m, 1), spi::model_flops(m, 3), bytes, plan.bytes.size(),
                  plan.partial_floats, plan.partial_planned, steps, spi::replica_desc(m, o).c_str());
    }
  // BERT task heads: the output count and byte sizes check_io holds a task to -- up to five outputs (hidden,
  // pooler, mean, start, end) -- the pooled vector's place in the workspace, and the walk at max_batch.
  bt.linear("bert.pooler.dense", 128, 128), bt.linear("classifier", 5, 128), bt.linear("qa_outputs", 2, 128);
  const int64_t B = 2, S = 16, D = 128, Lh = 5;
  // Then RoBERTa's position rule (SPI_BERT_POS_FROM_IDS: the plan of the plain replica, sequences up to position
  // rows - 2) and the two-layer sequence head (classifier.dense + classifier.out_proj, 3 labels, added to the
  // tensors when its case comes: from then on the names select it).
  const struct { const char* name; int io; std::vector<size_t> out; size_t cls; bool two_layer; } heads[] = {
      {"seq_head", SPI_BERT_HEAD_SEQUENCE, {(size_t)(B * S * D), (size_t)(B * Lh)}, 8 * 128 * 4},
      {"no_hidden|seq_head", SPI_BERT_NO_HIDDEN | SPI_BERT_HEAD_SEQUENCE, {(size_t)(B * Lh)}, 2 * 8 * 128 * 4},
      {"no_hidden|token_head", SPI_BERT_NO_HIDDEN | SPI_BERT_HEAD_TOKEN, {(size_t)(B * S * Lh)}, 8 * 128 * 4},
      {"pooler|mean|qa_head", SPI_BERT_OUT_POOLER | SPI_BERT_OUT_MEAN | SPI_BERT_HEAD_QA,
       {(size_t)(B * S * D), (size_t)(B * D), (size_t)(B * D), (size_t)(B * S), (size_t)(B * S)}, 0},
      {"pos_from_ids", SPI_BERT_POS_FROM_IDS, {(size_t)(B * S * D)}, 0},
      {"pos_from_ids|no_hidden|seq_head2", SPI_BERT_POS_FROM_IDS | SPI_BERT_NO_HIDDEN | SPI_BERT_HEAD_SEQUENCE,
       {(size_t)(B * 3)}, 2 * 8 * 128 * 4, true}};
  for (const auto& h : heads) {
    if (h.two_layer) bt.linear("classifier.dense", 128, 128), bt.linear("classifier.out_proj", 3, 128);
    spi_model_config cfg{};
    cfg.family = SPI_FAMILY_AUTO, cfg.precision = SPI_PREC_F16, cfg.max_batch = 8, cfg.num_heads = 2, cfg.seq_len = 16;
    cfg.bert_io = h.io;
    const spi::PackedModel m = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
    const spi::ReplicaOptions o;
    spi_codelet_args a{};
    a.num_inputs = 2, a.num_outputs = (uint32_t)h.out.size();
    size_t in_bytes[2] = {(size_t)(B * S * 8), (size_t)(B * S * 8)}, out_bytes[SPI_MAX_OUTPUTS] = {};
    for (int i = 0; i < 2; ++i) a.input_types[i] = SPI_DTYPE_I64, a.num_dims[i] = 2, a.dims[i][0] = B, a.dims[i][1] = S;
    for (size_t i = 0; i < h.out.size(); ++i) a.output_types[i] = SPI_DTYPE_F32, out_bytes[i] = h.out[i] * 4;
    auto takes = [&] {
      try {
        spi::check_io(m, o, a, in_bytes, out_bytes);
        return true;
      } catch (const std::runtime_error&) {
        return false;
      }
    };
    bool ok = spi::num_outputs(m, o) == (int)h.out.size() && takes();
    out_bytes[h.out.size() - 1] += 4;  // the last output one element too long
    ok = ok && !takes();
    out_bytes[h.out.size() - 1] -= 4;
    a.num_outputs -= 1;  // one output too few
    ok = ok && !takes();
    const spi::WorkspacePlan plan = spi::workspace_plan(m, o);
    int steps = 0;
    try {
      steps = spi::plan_check(m, o, m.max_batch, m.seq);
    } catch (const std::runtime_error& e) {
      std::fprintf(stderr, "bert_d128|fp16|%s: %s\n", h.name, e.what());
      ok = false;
    }
    if (h.io & SPI_BERT_POS_FROM_IDS) {  // seq_len 0: the 32-row table serves 30 tokens, and 31 are refused
      cfg.seq_len = 0;
      const spi::PackedModel longest = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
      ok = ok && longest.seq == 30 && m.pos_from_ids && spi::plan_check(longest, o, 1, 30) > 0;
      try {
        spi::plan_check(longest, o, 1, 31);
        ok = false;
      } catch (const std::runtime_error&) {
      }
      ok = ok && (!h.two_layer || m.num_labels == 3);
    }
    if (!ok || plan.bytes.size() != (size_t)spi::kBtBufs || plan.bytes[spi::kBtCls] != h.cls) {
      std::fprintf(stderr, "bert_d128|fp16|%s: outputs, check_io or the workspace plan are not the expected ones\n", h.name);
      rc = 1;
    }
    std::printf("bert_d128|fp16|%s| %d outputs, %d labels, flops(3) %.0f, class-token buffer %zu bytes, %d steps fit, %s\n",
                h.name, spi::num_outputs(m, o), m.num_labels, spi::model_flops(m, 3), plan.bytes[spi::kBtCls], steps,
                spi::replica_desc(m, o).c_str());
  }
  return rc;
}
