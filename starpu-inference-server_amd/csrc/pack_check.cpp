// Stand-alone check of the host-only packer (make pack_check): packs three small models whose
// tensors are synthesised here with the closed-form fill of tests/golden/make_replica_digests.py
// and prints the digests, which equal that table's resnet_basic / bert_d128 / vit_d128 entries; then the
// BERT once more with every spi_model_config.bert_io bit set, and once per task head (SPI_BERT_HEAD_*),
// checking what the bits append to the blob; then RoBERTa's position rule, which appends nothing, and the
// two-layer sequence head.
// Built with the address and undefined-behaviour sanitizers, no HIP.
#include <cstdio>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <stdexcept>

#include "model_pack.hpp"

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
  for (const Case& c : cases)
    for (const auto& pr : precs) {
      spi_model_config cfg{};
      cfg.family = SPI_FAMILY_AUTO, cfg.precision = pr.prec, cfg.max_batch = 8;
      cfg.num_heads = c.heads, cfg.seq_len = c.seq, cfg.image_size = c.image;
      const spi::PackedModel m = spi::pack_model(cfg, c.t->t.data(), (int)c.t->t.size());
      std::printf("%s|%s| %016llx %zu %s\n", c.name, pr.name, (unsigned long long)m.digest, m.blob_bytes, m.desc.c_str());
    }
  // bert_io: the same BERT plus its pooler, packed with every bit set.  The blob only grows by the
  // appended fp32 type table [2][128] and pooler [128][128] + [128], each on its own 256-byte line.
  bt.linear("bert.pooler.dense", 128, 128);
  spi_model_config cfg{};
  cfg.family = SPI_FAMILY_AUTO, cfg.precision = SPI_PREC_F16, cfg.max_batch = 8, cfg.num_heads = 2, cfg.seq_len = 16;
  const spi::PackedModel plain = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
  cfg.bert_io = SPI_BERT_OUT_POOLER | SPI_BERT_OUT_MEAN | SPI_BERT_NO_HIDDEN | SPI_BERT_TOKEN_TYPES;
  const spi::PackedModel io = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
  std::printf("bert_d128|fp16|bert_io=15 %016llx %zu %s\n", (unsigned long long)io.digest, io.blob_bytes, io.desc.c_str());
  const size_t grown = (2 * 128 + 128 * 128 + 128) * sizeof(float);
  if (io.blob_bytes < plain.blob_bytes + grown || io.blob_bytes > plain.blob_bytes + grown + 3 * 256 ||
      io.digest == plain.digest || io.type_table < plain.blob_bytes || io.pool_w <= io.type_table ||
      io.pool_b + 128 * sizeof(float) != io.blob_bytes) {
    std::fprintf(stderr, "bert_io packing: unexpected blob growth %zu -> %zu\n", plain.blob_bytes, io.blob_bytes);
    return 1;
  }
  // Task heads: the head's parameters sit beside the `bert.` prefix, not under it.  One case per head; each
  // appends its fp32 [L][128] weight and [L] bias on 256-byte lines (the sequence head the pooler too).
  bt.linear("classifier", 5, 128), bt.linear("qa_outputs", 2, 128);
  const struct { const char* name; int bit, labels; size_t pooler; const char* out; } heads[] = {
      {"seq_head", SPI_BERT_HEAD_SEQUENCE, 5, 128 * 128 + 128, "out[hidden,seq_logits5] in[ids,mask]"},
      {"token_head", SPI_BERT_HEAD_TOKEN, 5, 0, "out[hidden,token_logits5] in[ids,mask]"},
      {"qa_head", SPI_BERT_HEAD_QA, 2, 0, "out[hidden,qa_start,qa_end] in[ids,mask]"}};
  for (const auto& h : heads) {
    cfg.bert_io = h.bit;
    const spi::PackedModel m = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
    std::printf("bert_d128|fp16|%s %016llx %zu %s\n", h.name, (unsigned long long)m.digest, m.blob_bytes, m.desc.c_str());
    const size_t grow = (h.pooler + (size_t)h.labels * 128 + h.labels) * sizeof(float);
    const std::string want = h.out;
    if (m.num_labels != h.labels || m.blob_bytes < plain.blob_bytes + grow || m.blob_bytes > plain.blob_bytes + grow + 3 * 256 ||
        m.head_w < plain.blob_bytes || m.head_b + h.labels * sizeof(float) != m.blob_bytes || m.digest == plain.digest ||
        m.desc.size() < want.size() || m.desc.compare(m.desc.size() - want.size(), want.size(), want) != 0) {
      std::fprintf(stderr, "%s packing: unexpected blob %zu -> %zu, %d labels, %s\n", h.name, plain.blob_bytes,
                   m.blob_bytes, m.num_labels, m.desc.c_str());
      return 1;
    }
  }
  // SPI_BERT_POS_FROM_IDS: the plain blob, byte for byte, and the plain description plus a marker; seq_len 0
  // resolves to the 32-row table's 30 tokens and 31 are refused.
  cfg.bert_io = SPI_BERT_POS_FROM_IDS;
  const spi::PackedModel rp = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
  std::printf("bert_d128|fp16|pos_from_ids %016llx %zu %s\n", (unsigned long long)rp.digest, rp.blob_bytes, rp.desc.c_str());
  cfg.seq_len = 0;
  const int longest = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size()).seq;
  bool refused = false;
  try {
    cfg.seq_len = 31;
    spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
  } catch (const std::runtime_error& e) {
    refused = std::string(e.what()).find("32 rows") != std::string::npos;
  }
  if (rp.digest != plain.digest || rp.blob_bytes != plain.blob_bytes || rp.desc != plain.desc + " pos[ids]" ||
      !rp.pos_from_ids || rp.bert_io != 0 || longest != 30 || !refused) {
    std::fprintf(stderr, "pos_from_ids packing: %s, longest sequence %d, seq_len 31 %s\n", rp.desc.c_str(), longest,
                 refused ? "refused" : "not refused as expected");
    return 1;
  }
  // The two-layer sequence head (HF's RobertaClassificationHead): its names select it, dense [128][128] goes where
  // the pooler's tensors go and out_proj [3][128] is the head; with the pooler output it is refused.
  bt.linear("classifier.dense", 128, 128), bt.linear("classifier.out_proj", 3, 128);
  cfg.seq_len = 16, cfg.bert_io = SPI_BERT_POS_FROM_IDS | SPI_BERT_HEAD_SEQUENCE;
  const spi::PackedModel two = spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
  std::printf("bert_d128|fp16|pos_from_ids|seq_head2 %016llx %zu %s\n", (unsigned long long)two.digest, two.blob_bytes,
              two.desc.c_str());
  const float* dense = bt.data[bt.data.size() - 4].data();  // classifier.dense.weight as synthesised
  const size_t grow2 = (128 * 128 + 128 + 3 * 128 + 3) * sizeof(float);
  bool refused2 = false;
  try {
    cfg.bert_io |= SPI_BERT_OUT_POOLER;
    spi::pack_model(cfg, bt.t.data(), (int)bt.t.size());
  } catch (const std::runtime_error& e) {
    refused2 = std::string(e.what()).find("classifier.out_proj.weight") != std::string::npos;
  }
  if (two.num_labels != 3 || two.blob_bytes < plain.blob_bytes + grow2 || two.blob_bytes > plain.blob_bytes + grow2 + 4 * 256 ||
      two.pool_w < plain.blob_bytes || two.head_w <= two.pool_b || two.head_b + 3 * sizeof(float) != two.blob_bytes ||
      std::memcmp(two.blob.data() + two.pool_w, dense, 128 * 128 * sizeof(float)) != 0 || !refused2 ||
      two.desc != plain.desc + " out[hidden,seq_logits3] in[ids,mask] pos[ids]") {
    std::fprintf(stderr, "two-layer sequence head packing: unexpected blob %zu -> %zu, %d labels, %s\n", plain.blob_bytes,
                 two.blob_bytes, two.num_labels, two.desc.c_str());
    return 1;
  }
  return 0;
}
