// Weight packer: recognise -> fold -> pack into one blob (model_pack.hpp).  Reference
// counterparts: model loading (src/core/inference_runner.cpp:243-275) and the model graphs the
// reference exports (models/import_resnet.py:25-73, models/import_vit.py:10-62,
// models/import_bert-base-uncased.py:8-39).
#include "model_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <stdexcept>

#include "convnext_pack.hpp"
#include "rel_bias_pack.hpp"
#include "swin_pack.hpp"
#include "gconv.hpp"
#include "ln_fold_pack.hpp"
#include "mbconv_pack.hpp"
#include "pack.hpp"

// F16M: plain fp16 FC weights since round 5 (hi + lo kept the logits 0.06e-3 closer on 8 emulated
// seeds and cost 1 % of C2); define SPI_FC_HILO=1 for the hi + lo packing
#ifndef SPI_FC_HILO
#define SPI_FC_HILO 0
#endif

namespace spi {
namespace {

using PMap = std::map<std::string, const spi_named_tensor*>;

int64_t numel(const spi_named_tensor* t) {
  int64_t n = 1;
  for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
  return n;
}

const float* fdata(const spi_named_tensor* t) {
  if (t->dtype != SPI_DTYPE_F32)
    throw std::runtime_error(std::string("parameter ") + t->name + " must be fp32");
  return static_cast<const float*>(t->data);
}

const spi_named_tensor* need(const PMap& p, const std::string& k) {
  auto it = p.find(k);
  if (it == p.end()) throw std::runtime_error("missing parameter '" + k + "'");
  return it->second;
}

bool has(const PMap& p, const std::string& k) { return p.count(k) != 0; }

bool ends_with(const std::string& k, const std::string& anchor) {
  return k.size() >= anchor.size() && k.compare(k.size() - anchor.size(), anchor.size(), anchor) == 0;
}

bool ends_with(const PMap& p, const std::string& anchor) {
  return std::any_of(p.begin(), p.end(), [&](const auto& kv) { return ends_with(kv.first, anchor); });
}

// Strip the common prefix in front of an anchor name ("bert.embeddings..." ->
// "embeddings..."), so wrapped modules are recognised.
PMap strip_prefix(const PMap& in, const std::string& anchor) {
  std::string prefix;
  for (auto& kv : in) {
    if (!ends_with(kv.first, anchor)) continue;
    const std::string pre = kv.first.substr(0, kv.first.size() - anchor.size());
    if (pre.empty() || pre.back() == '.') {
      prefix = pre;
      break;
    }
  }
  if (prefix.empty()) return in;
  PMap out;
  for (auto& kv : in)
    if (kv.first.compare(0, prefix.size(), prefix) == 0) out[kv.first.substr(prefix.size())] = kv.second;
  return out;
}

struct Blob {
  std::vector<char> data;
  size_t add(const void* src, size_t bytes) {  // 256-byte aligned; zero-filled without a source
    const size_t off = (data.size() + 255) & ~size_t(255);
    data.resize(off + bytes);
    if (src) std::memcpy(data.data() + off, src, bytes);
    return off;
  }
};

// Eval BatchNorm folded into a conv: w' = w * gamma / sqrt(var + eps) (fp64, then
// fp32), bias' = beta - mean * gamma / sqrt(var + eps) (or the conv's own bias).
struct FoldedConv {
  int cout = 0, cin = 0, kh = 1, kw = 1;
  std::vector<float> w;  // [cout][cin][kh][kw]
  std::vector<float> b;  // [cout]
};

FoldedConv fold_conv(const PMap& p, const std::string& wname, const std::string& bn, float bn_eps) {
  const spi_named_tensor* wt = need(p, wname + ".weight");
  if (wt->ndim != 4) throw std::runtime_error(wname + ".weight must be 4-D");
  FoldedConv f;
  f.cout = (int)wt->shape[0];
  f.cin = (int)wt->shape[1];
  f.kh = (int)wt->shape[2];
  f.kw = (int)wt->shape[3];
  std::vector<double> scale(f.cout, 1.0), shift(f.cout, 0.0);
  if (!bn.empty()) {
    const float* g = fdata(need(p, bn + ".weight"));
    const float* b = fdata(need(p, bn + ".bias"));
    const float* m = fdata(need(p, bn + ".running_mean"));
    const float* v = fdata(need(p, bn + ".running_var"));
    for (int o = 0; o < f.cout; ++o) {
      const double s = (double)g[o] / std::sqrt((double)v[o] + (double)bn_eps);
      scale[o] = s;
      shift[o] = (double)b[o] - (double)m[o] * s;
    }
  } else if (has(p, wname + ".bias")) {
    const float* b = fdata(need(p, wname + ".bias"));
    for (int o = 0; o < f.cout; ++o) shift[o] = b[o];
  }
  const float* w = fdata(wt);
  const size_t per = (size_t)f.cin * f.kh * f.kw;
  f.w.resize((size_t)f.cout * per);
  f.b.resize(f.cout);
  for (int o = 0; o < f.cout; ++o) {
    for (size_t i = 0; i < per; ++i) f.w[o * per + i] = (float)((double)w[o * per + i] * scale[o]);
    f.b[o] = (float)shift[o];
  }
  return f;
}

// The LayerNorm fold is an fp16 path, on by default where it measured faster; SPI_LN_FOLD=0 / 1
// forces the separate launches / the fold (A/B runs).
bool ln_fold_enabled(Prec prec, bool by_default) {
  const char* e = std::getenv("SPI_LN_FOLD");
  const bool on = (e && *e) ? std::atoi(e) != 0 : by_default;
  return prec == Prec::F16 && on;
}
// BERT-base: fold +3.9 % four-stream (same process, round 4).  ViT-L: off in rounds 4-5 (5.93k
// folded against 6.30k, profiles/r04/fixed/vit_fold_ab.txt: the producer epilogues' fp16 copy and
// the consumers' statistics round trip + spills cost more than the 46 removed launches); on since
// round 6 over the two-plane residual stream (no copy; statistics loaded under the last k-tile):
// 6.68k folded against 6.59k (profiles/r06/vit_fold/).  On rows whose mean exceeds their spread (the
// folded form's cancellation case; test_vit_layernorm_fold_outliers, pos_embedding += 1) the fold
// measures 7.2e-4 against the oracle, the separate launches 6.7e-4: both inside the 1e-3 bar
constexpr bool kBertLnFold = true;
constexpr bool kVitLnFold = true;

// One replica being packed: the blob it fills and the tables it returns.  An object per
// pack_model call, so replicas can be packed concurrently (one per device, clone_model_to_gpus).
struct Packer {
  PackedModel m;
  Blob blob;
  int window_cfg = 0;  // Swin v2's window where no tensor states it: the side of spi_model_config.seq_len = ws^2 tokens
  bool image_stated = false;  // spi_model_config.image_size > 0

  // Pack the [N][K] fp32 matrix at(n, k) into t.w as [npad][kpad] of t.prec (pack.hpp) and set t's
  // geometry.  hilo (F16 only): every 64-k block twice -- fp16(w), then fp16(w - fp16(w)) -- for a
  // krep = 2 contraction (GemmDesc::krep).
  template <typename T, typename F>
  void pack_weight(T& t, int N, int K, bool hilo, F at) {
    if (hilo && t.prec != Prec::F16) throw std::runtime_error("hi/lo weight packing is an F16 layout");
    t.krep = hilo ? 2 : 1;
    t.kpad = round_up_to(K, 64) * t.krep;
    t.npad = round_up_to(N, 128);
    t.wplane = (size_t)t.npad * t.kpad;
    t.w = blob.add(nullptr, packed_bytes(t.prec, t.npad, t.kpad));
    char* dst = blob.data.data() + t.w;
    if (hilo)
      pack_matrix_into(dst, N, t.kpad, t.npad, t.kpad, t.prec,
                       [&](int n, int kp) { return hilo_element(kp, K, [&](int k) { return at(n, k); }); });
    else
      pack_matrix_into(dst, N, K, t.npad, t.kpad, t.prec, at);
  }

  size_t pack_vec(const float* v, int n) { return blob.add(v, (size_t)n * sizeof(float)); }

  // Folded conv weight [Cout][Cin][KH][KW] -> [Npad][Kpad], k = (kh*KW + kw)*cin_pad + c.
  // groups > 1: f.cin is the channels per group and the packed matrix the dense block-diagonal
  // expansion over all groups * f.cin input channels, zero off the row's group.
  ConvW pack_conv(const FoldedConv& f, int stride, int cin_pad, Prec prec, bool hilo = false, int groups = 1) {
    ConvW c;
    c.cout = f.cout;
    c.cin = f.cin * groups;
    c.groups = groups;
    c.kh = f.kh;
    c.kw = f.kw;
    c.stride = stride;
    c.pad = c.kh / 2;
    c.cin_pad = std::max(cin_pad, c.cin);
    const int K = c.kh * c.kw * c.cin_pad;
    const int cin = c.cin, kh = c.kh, kw = c.kw, cp = c.cin_pad, cpg = f.cin, npg = f.cout / groups;
    c.prec = prec;
    pack_weight(c, c.cout, K, hilo, [&](int n, int k) -> float {
      const int cell = k / cp, ci = k % cp;
      if (ci >= cin || ci / cpg != n / npg) return 0.f;
      const int y = cell / kw, x = cell % kw;
      return f.w[(((size_t)n * cpg + ci % cpg) * kh + y) * kw + x];
    });
    c.w_image = !hilo && packed_has_wres_image(prec, c.cout, K, c.npad, c.kpad);
    c.b = pack_vec(f.b.data(), c.cout);
    return c;
  }

  // A grouped 3x3 conv for the grouped kernel (gconv.hpp): fp16, no GEMM geometry.
  ConvW pack_gconv(const FoldedConv& f, int stride, int groups) {
    ConvW c;
    c.cout = f.cout;
    c.cin = c.cin_pad = f.cin * groups;
    c.groups = groups;
    c.gconv = true;
    c.kh = f.kh;
    c.kw = f.kw;
    c.stride = stride;
    c.pad = 1;
    c.prec = Prec::F16;
    c.w = blob.add(nullptr, gconv_packed_bytes(c.cout, groups));
    const int cpg = f.cin;
    gconv_pack_into(reinterpret_cast<_Float16*>(blob.data.data() + c.w), c.cout, groups,
                    [&](int n, int ci, int tap) { return f.w[((size_t)n * cpg + ci) * 9 + tap]; });
    c.b = pack_vec(f.b.data(), c.cout);
    return c;
  }

  ConvW pack_conv(const PMap& p, const std::string& pre, const char* conv, const char* bn, int stride, bool hilo = false) {
    return pack_conv(fold_conv(p, pre + conv, pre + bn, m.eps), stride, 0, m.prec, hilo);
  }

  LinearW pack_linear(const float* w, const float* b, int N, int K, bool hilo) {
    LinearW L;
    L.n = N;
    L.k = K;
    L.prec = m.prec;
    pack_weight(L, N, K, hilo, [&](int n, int k) { return w[(size_t)n * K + k]; });
    std::vector<float> zeros;
    if (!b) {
      zeros.assign(N, 0.f);
      b = zeros.data();
      L.has_bias = false;
    }
    L.b = pack_vec(b, N);
    return L;
  }

  LinearW pack_linear_named(const PMap& p, const std::string& name, bool hilo) {
    const spi_named_tensor* wt = need(p, name + ".weight");
    if (wt->ndim != 2) throw std::runtime_error(name + ".weight must be 2-D");
    const float* b = has(p, name + ".bias") ? fdata(need(p, name + ".bias")) : nullptr;
    return pack_linear(fdata(wt), b, (int)wt->shape[0], (int)wt->shape[1], hilo);
  }

  // The weights of a GEMM whose input rows are LayerNorm'd (y = LN(x) W^T + b), packed for
  // the fold (ln_fold.hpp): W' = W diag(gamma) in the compute type, bias' = b + W beta, and
  // c1[n] = sum_k W'[n][k] over the packed (rounded) values, so the epilogue's
  // rstd (x W'^T - mean c1) cancels exactly what the MFMAs accumulated.
  // hilo (transformer F16M): W' packed hi + lo (krep = 2); c1 sums both halves as packed.
  // `ln` names the LayerNorm whose gain and bias are folded in.
  LinearW pack_linear_folded(const float* w, const float* b, int N, int K, const PMap& p, const std::string& ln) {
    std::vector<float> wf((size_t)N * K), bf(N);
    std::vector<float> c1(N);
    fold_linear(w, b, N, K, fdata(need(p, ln + ".weight")), fdata(need(p, ln + ".bias")), m.prec == Prec::F16,
                m.mixed, wf.data(), bf.data(), c1.data());
    LinearW L = pack_linear(wf.data(), bf.data(), N, K, m.mixed);
    L.c1 = pack_vec(c1.data(), N);
    return L;
  }

  LnW pack_ln(const PMap& p, const std::string& name) {
    LnW l;
    const spi_named_tensor* g = need(p, name + ".weight");
    l.g = pack_vec(fdata(g), (int)numel(g));
    l.b = pack_vec(fdata(need(p, name + ".bias")), (int)numel(g));
    return l;
  }

  void check_heads() {  // transformers: 32- or 64-wide heads, num_heads 0 = as many 64-wide ones as fit
    if (m.D <= 0 || m.D % 64 != 0 || m.D > 1024)
      throw std::runtime_error("hidden size must be a multiple of 64, <= 1024");
    if (m.heads <= 0) m.heads = m.D / 64;
    if (m.D % m.heads != 0 || (m.D / m.heads != 32 && m.D / m.heads != 64))
      throw std::runtime_error("hidden size " + std::to_string(m.D) + " over " + std::to_string(m.heads) +
                               " attention heads: head_dim must be 32 or 64");
  }
  void build_resnet(const PMap& p);
  void build_bert(const PMap& p, const PMap& all);
  void pack_bert_head(const PMap& all, bool two_layer);
  void build_vit(const PMap& p);
  void build_convnext(const PMap& p);
  void build_swin(const PMap& p);
  void build_efficientnet(const PMap& p);
  SwBlock pack_swin_v2_block(const PMap& p, const std::string& pre, int C, int H, int stage);
};

void Packer::build_resnet(const PMap& p) {
  // Stages: torchvision layer1..layer4, stride 2 on the first block of 2..4
  // (on conv1 for BasicBlock, conv2 for Bottleneck: torchvision v1.5).
  m.bottleneck = has(p, "layer1.0.conv3.weight");
  // Stem input channels padded to one 16-byte chunk per pixel: 4 fp32
  // (F32, and F16X3 whose A is fp32) or 8 fp16 (F16).
  // SPI_PREC_F16M: the stem reads the fp32 image with split weights (F16X3) and
  // writes fp16; the downsample convs and the (avgpool-fused) FC carry hi + lo
  // weights (krep = 2) (these layers set the fp16 error).
  const Prec stem_prec = m.mixed ? Prec::F16X3 : m.prec;
  const FoldedConv stem_folded = fold_conv(p, "conv1", "bn1", m.eps);
  m.stem = pack_conv(stem_folded, 2, stem_prec == Prec::F16 ? 8 : 4, stem_prec);
  if (m.stem.kh != 7 || m.stem.cin != 3) throw std::runtime_error("resnet stem must be 7x7 over 3 channels");
  // SPI_GCONV=0: the dense expansion of grouped convs in the fp16 modes too (A/B runs, tests)
  const char* ge = std::getenv("SPI_GCONV");
  const bool gconv_on = !(ge && *ge && std::atoi(ge) == 0);
  std::vector<int> block_groups;  // conv2's groups, per block
  for (int L = 1; L <= 4; ++L) {
    int nb = 0;
    while (has(p, "layer" + std::to_string(L) + "." + std::to_string(nb) + ".conv1.weight")) ++nb;
    if (nb == 0) throw std::runtime_error("resnet layer" + std::to_string(L) + " missing");
    m.stage_blocks.push_back(nb);
    for (int i = 0; i < nb; ++i) {
      const std::string pre = "layer" + std::to_string(L) + "." + std::to_string(i) + ".";
      const int s = (L > 1 && i == 0) ? 2 : 1;
      ResBlock blk;
      blk.c1 = pack_conv(p, pre, "conv1", "bn1", m.bottleneck ? 1 : s);
      // A bottleneck's conv2 may be grouped (ResNeXt): weight.shape[1] = C / groups.  Inside the
      // grouped kernel's set (gconv.hpp) the fp16 modes pack for it and the fp32-grade modes (and
      // SPI_GCONV=0) the dense expansion; anything else is packed as it stands and fails the
      // channel chain below.
      const FoldedConv f2 = fold_conv(p, pre + "conv2", pre + "bn2", m.eps);
      const int C = blk.c1.cout;
      int groups = 1;
      if (m.bottleneck && f2.cin > 0 && f2.cin != C && f2.cout == C && C % f2.cin == 0 && f2.kh == 3 &&
          f2.kw == 3 && gconv_supported(C, C / f2.cin))
        groups = C / f2.cin;
      block_groups.push_back(groups);
      if (groups > 1 && m.prec == Prec::F16 && gconv_on)
        blk.c2 = pack_gconv(f2, s, groups);
      else
        blk.c2 = pack_conv(f2, m.bottleneck ? s : 1, 0, m.prec, false, groups);
      if (m.bottleneck) blk.c3 = pack_conv(p, pre, "conv3", "bn3", 1);
      blk.has_ds = has(p, pre + "downsample.0.weight");
      if (blk.has_ds) blk.ds = pack_conv(p, pre, "downsample.0", "downsample.1", s, m.mixed);
      m.blocks.push_back(blk);
    }
  }
  m.fc = pack_linear_named(p, "fc", m.mixed && SPI_FC_HILO);
  m.classes = m.fc.n;
  m.feat = m.fc.k;
  // Channel chain: every conv must read exactly the channels its producer
  // writes.  A grouped conv (ResNeXt, models/import_resnet.py variants) stores
  // weight.shape[1] = C/groups, which would otherwise be packed as a dense conv
  // over too few channels and give garbage without an error.
  auto bad = [](const std::string& what) { throw std::runtime_error("resnet: grouped/unsupported conv (" + what + ")"); };
  auto reads = [](const char* conv, int got, int of, const char* unit = "channels") {
    return std::string(conv) + " reads " + std::to_string(got) + " of " + std::to_string(of) + " " + unit;
  };
  int ch = m.stem.cout;
  for (size_t i = 0; i < m.blocks.size(); ++i) {
    const ResBlock& b = m.blocks[i];
    const std::string id = "block " + std::to_string(i) + " ";
    if (b.c1.cin != ch) bad(id + reads("conv1", b.c1.cin, ch));
    if (b.c2.cin != b.c1.cout) bad(id + reads("conv2", b.c2.cin, b.c1.cout));
    if (m.bottleneck && b.c3.cin != b.c2.cout) bad(id + reads("conv3", b.c3.cin, b.c2.cout));
    const int out = m.bottleneck ? b.c3.cout : b.c2.cout;
    if (b.has_ds) {
      if (b.ds.cin != ch || b.ds.cout != out) bad(id + "downsample shape");
    } else if (ch != out) {
      bad(id + "identity residual with " + std::to_string(ch) + " -> " + std::to_string(out) + " channels");
    }
    ch = out;
  }
  if (m.fc.k != ch) bad(reads("fc", m.fc.k, ch, "features"));
  m.groups = block_groups.front();
  for (size_t i = 0; i < block_groups.size(); ++i)
    if (block_groups[i] != m.groups)
      bad("block " + std::to_string(i) + " conv2 has " + std::to_string(block_groups[i]) + " groups, block 0 has " +
          std::to_string(m.groups));
  // Split activations need every activation's channel count to be a multiple
  // of 32 (the split block) and every non-stem conv to read >= 32 channels.
  m.split = m.prec == Prec::F16X3 && m.stem.cout % 32 == 0;
  for (auto& b : m.blocks)
    for (const ConvW* c : {&b.c1, &b.c2, &b.c3, &b.ds}) {
      if (!c->cout) continue;
      if (c->cin_pad % 8 != 0 || (c->cin_pad & (c->cin_pad - 1)))
        throw std::runtime_error("resnet conv channels must be a power of two >= 8");
      if (c->cin_pad < 32 || c->cout % 32 != 0 || c->kh * c->kw > 31) m.split = false;
    }
  // Fused stem (stem.hip: NCHW image -> conv + BN + ReLU -> max pool, one launch)
  // for the fp16-activation modes and split fp16x3; fp32 keeps ingest + stem GEMM +
  // max pool.  SPI_STEM_FUSED=0 selects the unfused path (A/B, tests).
  const char* fe = std::getenv("SPI_STEM_FUSED");
  const int stem_ow = (m.image + 6 - 7) / 2 + 1;
  m.stem_fused = !(fe && *fe && std::atoi(fe) == 0) && m.stem.cout == 64 && m.stem.stride == 2 &&
                 stem_ow <= kStemPoolMaxOW && (m.prec == Prec::F16 || m.split);
  if (m.stem_fused) {
    std::vector<_Float16> packed(stem_pool_bytes() / sizeof(_Float16));
    stem_pool_pack(stem_folded.w.data(), packed.data());
    m.stem_pool_w = blob.add(packed.data(), stem_pool_bytes());
  }
}

// The one tensor of the unstripped parameter list named `name` or ending in ".name": the task heads'
// parameters sit beside the `bert.` prefix strip_prefix removes, not under it.
const spi_named_tensor* find_head_param(const PMap& all, const std::string& name, const char* bit) {
  const spi_named_tensor* found = nullptr;
  int n = 0;
  for (const auto& kv : all)
    if (kv.first == name || ends_with(kv.first, "." + name)) found = kv.second, ++n;
  if (n == 0) throw std::runtime_error(std::string("bert_io: ") + bit + " needs parameter '" + name + "'");
  if (n > 1)
    throw std::runtime_error(std::string("bert_io: ") + bit + ": parameter '" + name + "' is ambiguous (" +
                             std::to_string(n) + " tensors end in it)");
  return found;
}

// Whether the unstripped list holds a tensor find_head_param would find under `name`.
bool has_head_param(const PMap& all, const std::string& name) {
  return std::any_of(all.begin(), all.end(),
                     [&](const auto& kv) { return kv.first == name || ends_with(kv.first, "." + name); });
}

// The task head's dense layer, appended as plain fp32 [L][D] and [L], each on its own 256-byte line.
// two_layer: the sequence head's last layer is classifier.out_proj (build_bert packed classifier.dense).
void Packer::pack_bert_head(const PMap& all, bool two_layer) {
  const int io = m.bert_io, D = m.D;
  const bool qa = (io & SPI_BERT_HEAD_QA) != 0, seq = (io & SPI_BERT_HEAD_SEQUENCE) != 0;
  const char* bit = qa ? "SPI_BERT_HEAD_QA" : seq ? "SPI_BERT_HEAD_SEQUENCE" : "SPI_BERT_HEAD_TOKEN";
  const std::string name = qa ? "qa_outputs" : two_layer ? "classifier.out_proj" : "classifier";
  const spi_named_tensor* w = find_head_param(all, name + ".weight", bit);
  const spi_named_tensor* b = find_head_param(all, name + ".bias", bit);
  if (w->ndim != 2 || w->shape[1] != D || w->shape[0] < 1 || b->ndim != 1 || b->shape[0] != w->shape[0])
    throw std::runtime_error("bert: " + name + ".weight must be [L][D] with D = " + std::to_string(D) + " and " + name +
                             ".bias [L]");
  const int64_t L = w->shape[0];
  if (qa && L != 2)
    throw std::runtime_error("bert_io: SPI_BERT_HEAD_QA needs qa_outputs.weight [2][D], got " + std::to_string(L) + " rows");
  const int64_t lmax = seq ? 1024 : 64;
  if (L > lmax)
    throw std::runtime_error(std::string("bert_io: ") + bit + " takes 1 .. " + std::to_string(lmax) + " labels, " + name +
                             ".weight has " + std::to_string(L));
  m.num_labels = (int)L;
  m.head_w = pack_vec(fdata(w), (int)numel(w));
  m.head_b = pack_vec(fdata(b), (int)L);
}

void Packer::build_bert(const PMap& p, const PMap& all) {
  const spi_named_tensor* we = need(p, "embeddings.word_embeddings.weight");
  m.vocab = (int)we->shape[0];
  const int D = m.D = (int)we->shape[1];
  const spi_named_tensor* pe = need(p, "embeddings.position_embeddings.weight");
  m.maxpos = (int)pe->shape[0];
  check_heads();
  auto layer = [](int i) { return "encoder.layer." + std::to_string(i) + "."; };
  // MPNet is told apart by its names: the bucket table beside attention.attn.{q,k,v,o}.  One without the other, or
  // either beside BERT's attention.self.query, is refused.
  const std::string rel_name = "encoder.relative_attention_bias.weight";
  const bool rel_tab = has(p, rel_name), mp_attn = has(p, layer(0) + "attention.attn.q.weight");
  const bool mpnet = rel_tab && mp_attn;
  if ((rel_tab || mp_attn) && (!mpnet || has(p, layer(0) + "attention.self.query.weight")))
    throw std::runtime_error("bert: mixed BERT and MPNet attention names: '" + rel_name + "' and '" + layer(0) +
                             "attention.attn.q.weight' need each other and exclude '" + layer(0) +
                             "attention.self.query.weight'");
  if (mpnet) {
    const spi_named_tensor* rt = need(p, rel_name);
    if (m.D / m.heads != kRelHeadDim)
      throw std::runtime_error("mpnet: '" + rel_name + "': the relative-bias attention serves 64-wide heads only, hidden " +
                               std::to_string(m.D) + " over " + std::to_string(m.heads) + " heads is " +
                               std::to_string(m.D / m.heads));
    if (rt->ndim != 2 || rt->shape[1] != m.heads)
      throw std::runtime_error("mpnet: '" + rel_name + "' must be [nb][heads] with heads = " + std::to_string(m.heads));
    if (!rel_buckets_supported((int)std::min<int64_t>(rt->shape[0], 1 << 20)))
      throw std::runtime_error("mpnet: '" + rel_name + "' has " + std::to_string(rt->shape[0]) +
                               " buckets; served: a multiple of 4 in 4 .. 128");
    if (m.bert_io & SPI_BERT_TOKEN_TYPES)
      throw std::runtime_error("bert_io: SPI_BERT_TOKEN_TYPES: an MPNet replica has no token-type table");
    m.rel_buckets = (int)rt->shape[0];
    m.pos_from_ids = true;  // HF's MPNet counts positions from the ids, pad id 1, as RoBERTa does
    if (m.seq > kRelMaxSeq)
      throw std::runtime_error("mpnet: seq_len " + std::to_string(m.seq) + ": the relative-bias attention serves at most " +
                               std::to_string(kRelMaxSeq) + " tokens");
    if (m.seq <= 0) m.seq = std::min(m.maxpos - 2, kRelMaxSeq);  // checked against the table below
  }
  if (m.pos_from_ids) {
    // position ids run 2 .. S + 1 (row 1 is the pad token's, row 0 unused), so the table serves rows - 2 tokens
    const std::string rule = "position table has " + std::to_string(m.maxpos) +
                             " rows and SPI_BERT_POS_FROM_IDS reads rows 1 .. S + 1, so S <= rows - 2";
    if (m.maxpos < 3) throw std::runtime_error("bert_io: " + rule);
    if (m.seq > m.maxpos - 2)
      throw std::runtime_error("bert_io: seq_len " + std::to_string(m.seq) + " is too long: the " + rule + " = " +
                               std::to_string(m.maxpos - 2));
    if (m.seq <= 0) m.seq = m.maxpos - 2;
  }
  if (m.seq <= 0) m.seq = m.maxpos;
  m.word = pack_vec(fdata(we), (int)numel(we));
  m.pos = pack_vec(fdata(pe), (int)numel(pe));
  const spi_named_tensor* te = mpnet ? nullptr : need(p, "embeddings.token_type_embeddings.weight");
  m.type0 = te ? pack_vec(fdata(te), D) : blob.add(nullptr, sizeof(float) * D);  // token_type_ids buffer is all zeros
  m.emb_ln = pack_ln(p, "embeddings.LayerNorm");
  // HF's names of the layer's tensors: BERT's, or MPNet's (attention.attn.{q,k,v,o}, attention.LayerNorm)
  const char* qkv_names[3] = {mpnet ? "attention.attn.q" : "attention.self.query", mpnet ? "attention.attn.k" : "attention.self.key",
                              mpnet ? "attention.attn.v" : "attention.self.value"};
  const char* out_name = mpnet ? "attention.attn.o" : "attention.output.dense";
  const char* ln1_name = mpnet ? "attention.LayerNorm" : "attention.output.LayerNorm";
  while (has(p, layer(m.layers) + qkv_names[0] + ".weight")) ++m.layers;
  if (m.layers == 0) throw std::runtime_error("bert: no encoder layers");
  if (const std::string other = layer(m.layers) + (mpnet ? "attention.self.query" : "attention.attn.q") + ".weight"; has(p, other))
    throw std::runtime_error("bert: mixed BERT and MPNet attention names: '" + other + "' follows " +
                             std::to_string(m.layers) + " layers of the other kind");
  // Q, K, V stacked into one [3D][D] projection.
  std::vector<float> qw((size_t)3 * D * D), qb((size_t)3 * D);
  auto stack_qkv = [&](const std::string& pre) {
    for (int j = 0; j < 3; ++j) {
      const std::string nm = pre + qkv_names[j];
      std::memcpy(qw.data() + (size_t)j * D * D, fdata(need(p, nm + ".weight")), sizeof(float) * D * D);
      std::memcpy(qb.data() + (size_t)j * D, fdata(need(p, nm + ".bias")), sizeof(float) * D);
    }
  };
  for (int i = 0; i < m.layers; ++i) {
    const std::string pre = layer(i);
    TfLayer L;
    stack_qkv(pre);
    L.qkv = pack_linear(qw.data(), qb.data(), 3 * D, D, m.mixed);
    L.out = pack_linear_named(p, pre + out_name, m.mixed);
    L.ln1 = pack_ln(p, pre + ln1_name);
    L.ff1 = pack_linear_named(p, pre + "intermediate.dense", m.mixed);
    L.ff2 = pack_linear_named(p, pre + "output.dense", m.mixed);
    L.ln2 = pack_ln(p, pre + "output.LayerNorm");
    m.ffn = L.ff1.n;
    m.tf.push_back(L);
  }
  // post-LN: FFN1 of layer i reads LN1_i(a), QKV of layer i >= 1 reads LN2_{i-1}(b).  The plain
  // copies packed above stay in the blob unused (follow-up).
  m.ln_fold = m.ln_fold && D % 128 == 0 && m.ffn % 128 == 0;
  for (int i = 0; m.ln_fold && i < m.layers; ++i) {
    const std::string pre = layer(i);
    m.tf[i].ff1 = pack_linear_folded(fdata(need(p, pre + "intermediate.dense.weight")),
                                     fdata(need(p, pre + "intermediate.dense.bias")), m.ffn, D, p, pre + ln1_name);
    if (i == 0) continue;
    stack_qkv(pre);
    m.tf[i].qkv = pack_linear_folded(qw.data(), qb.data(), 3 * D, D, p, layer(i - 1) + "output.LayerNorm");
  }
  // bert_io appends only: a replica without bits keeps the blob above, byte for byte
  m.type_vocab = te ? (int)te->shape[0] : 1;
  if (m.bert_io & SPI_BERT_TOKEN_TYPES) {
    if (te->ndim != 2 || te->shape[1] != D) throw std::runtime_error("bert: token_type_embeddings.weight must be [types][D]");
    m.type_table = pack_vec(fdata(te), (int)numel(te));
  }
  // HF's RobertaClassificationHead: classifier.dense [D,D] + tanh on token 0, then classifier.out_proj [L,D].
  // The names decide.  dense goes where the pooler's tensors go, so bert_pooler + bert_seq_head compute it.
  const bool two_layer = (m.bert_io & SPI_BERT_HEAD_SEQUENCE) && has_head_param(all, "classifier.out_proj.weight");
  if (two_layer) {
    if (m.bert_io & SPI_BERT_OUT_POOLER)
      throw std::runtime_error(
          "bert_io: SPI_BERT_OUT_POOLER cannot be combined with the two-layer sequence head 'classifier.dense.weight' + "
          "'classifier.out_proj.weight': that model has no pooler, and classifier.dense takes its place");
    const spi_named_tensor* pw = find_head_param(all, "classifier.dense.weight", "SPI_BERT_HEAD_SEQUENCE");
    const spi_named_tensor* pb = find_head_param(all, "classifier.dense.bias", "SPI_BERT_HEAD_SEQUENCE");
    if (pw->ndim != 2 || pw->shape[0] != D || pw->shape[1] != D || numel(pb) != D)
      throw std::runtime_error("bert: classifier.dense must be [D][D] with a [D] bias, D = " + std::to_string(D));
    m.pool_w = pack_vec(fdata(pw), (int)numel(pw));
    m.pool_b = pack_vec(fdata(pb), D);
  } else if (m.bert_io & (SPI_BERT_OUT_POOLER | SPI_BERT_HEAD_SEQUENCE)) {  // the sequence head reads the pooled vector
    for (const char* nm : {"pooler.dense.weight", "pooler.dense.bias"})
      if (!has(p, nm))
        throw std::runtime_error(std::string("bert_io: SPI_BERT_OUT_POOLER needs parameter '") + nm +
                                 "' (a model built with add_pooling_layer=False has no pooler)");
    const spi_named_tensor* pw = need(p, "pooler.dense.weight");
    const spi_named_tensor* pb = need(p, "pooler.dense.bias");
    if (pw->ndim != 2 || pw->shape[0] != D || pw->shape[1] != D || numel(pb) != D)
      throw std::runtime_error("bert: pooler.dense must be [D][D] with a [D] bias");
    m.pool_w = pack_vec(fdata(pw), (int)numel(pw));
    m.pool_b = pack_vec(fdata(pb), D);
  }
  if (m.bert_io & (SPI_BERT_HEAD_SEQUENCE | SPI_BERT_HEAD_TOKEN | SPI_BERT_HEAD_QA)) pack_bert_head(all, two_layer);
  if (mpnet) {  // the bias rows for the replica's longest sequence, behind everything else
    m.rel_ld = rel_rows_ld(m.seq);
    m.rel_half = m.seq - 1;
    m.rel_rows = blob.add(nullptr, sizeof(float) * m.heads * m.rel_ld);
    rel_bias_rows(fdata(need(p, rel_name)), m.rel_buckets, kMpnetMaxDistance, m.heads, m.seq,
                  reinterpret_cast<float*>(blob.data.data() + m.rel_rows));
  }
}

void Packer::build_vit(const PMap& p) {
  const spi_named_tensor* cw = need(p, "conv_proj.weight");
  const int D = m.D = (int)cw->shape[0];
  m.patch = (int)cw->shape[2];
  if (cw->shape[1] != 3 || cw->shape[3] != m.patch) throw std::runtime_error("vit conv_proj must be PxP over 3 channels");
  if (m.image % m.patch) throw std::runtime_error("image size must be a multiple of the patch size");
  m.npatch = (m.image / m.patch) * (m.image / m.patch);
  check_heads();
  m.patch_proj = pack_linear(fdata(cw), has(p, "conv_proj.bias") ? fdata(need(p, "conv_proj.bias")) : nullptr, D,
                             3 * m.patch * m.patch, m.mixed);
  m.cls = pack_vec(fdata(need(p, "class_token")), D);
  const spi_named_tensor* pe = need(p, "encoder.pos_embedding");
  if (numel(pe) != (int64_t)(m.npatch + 1) * D) throw std::runtime_error("pos_embedding does not match image/patch size");
  m.vpos = pack_vec(fdata(pe), (int)numel(pe));
  auto layer = [](int i) { return "encoder.layers.encoder_layer_" + std::to_string(i) + "."; };
  auto mlp1 = [&](const std::string& pre) { return has(p, pre + "mlp.0.weight") ? pre + "mlp.0" : pre + "mlp.linear_1"; };
  while (has(p, layer(m.layers) + "ln_1.weight")) ++m.layers;
  if (m.layers == 0) throw std::runtime_error("vit: no encoder layers");
  for (int i = 0; i < m.layers; ++i) {
    const std::string pre = layer(i);
    TfLayer L;
    L.ln1 = pack_ln(p, pre + "ln_1");
    const spi_named_tensor* iw = need(p, pre + "self_attention.in_proj_weight");
    L.qkv = pack_linear(fdata(iw), fdata(need(p, pre + "self_attention.in_proj_bias")), (int)iw->shape[0],
                        (int)iw->shape[1], m.mixed);
    L.out = pack_linear_named(p, pre + "self_attention.out_proj", m.mixed);
    L.ln2 = pack_ln(p, pre + "ln_2");
    L.ff1 = pack_linear_named(p, mlp1(pre), m.mixed);
    L.ff2 = pack_linear_named(p, has(p, pre + "mlp.3.weight") ? pre + "mlp.3" : pre + "mlp.linear_2", m.mixed);
    m.ffn = L.ff1.n;
    m.tf.push_back(L);
  }
  // pre-LN: QKV of layer i >= 1 reads LN1_i(x) (layer 0's LN1 stays a launch, model body),
  // FFN1 of layer i reads LN2_i(x).  The plain copies packed above stay in the blob unused.
  m.ln_fold = m.ln_fold && D % 128 == 0 && m.ffn % 128 == 0;
  for (int i = 0; m.ln_fold && i < m.layers; ++i) {
    const std::string pre = layer(i);
    const spi_named_tensor* f1 = need(p, mlp1(pre) + ".weight");
    m.tf[i].ff1 = pack_linear_folded(fdata(f1), fdata(need(p, mlp1(pre) + ".bias")), (int)f1->shape[0],
                                     (int)f1->shape[1], p, pre + "ln_2");
    if (i == 0) continue;
    const spi_named_tensor* iw = need(p, pre + "self_attention.in_proj_weight");
    m.tf[i].qkv = pack_linear_folded(fdata(iw), fdata(need(p, pre + "self_attention.in_proj_bias")),
                                     (int)iw->shape[0], (int)iw->shape[1], p, pre + "ln_1");
  }
  m.final_ln = pack_ln(p, "encoder.ln");
  m.head = pack_linear_named(p, "heads.head", m.mixed);
  m.classes = m.head.n;
  m.seq = m.npatch + 1;
}

// torchvision's ConvNeXt: features.0 the stem (4x4 / stride 4 conv, LayerNorm2d), features.1, 3, 5, 7 the
// stages of CNBlocks, features.2, 4, 6 the downsamples (LayerNorm2d, 2x2 / stride 2 conv), classifier.0 / .2.
void Packer::build_convnext(const PMap& p) {
  auto refuse = [](const std::string& what) { throw std::runtime_error("convnext: " + what); };
  auto feat = [](int i) { return "features." + std::to_string(i) + "."; };
  if (m.image % 32) refuse("image size " + std::to_string(m.image) + " must be a multiple of 32");
  const spi_named_tensor* sw = need(p, "features.0.0.weight");
  if (sw->ndim != 4 || sw->shape[1] != 3 || sw->shape[2] != 4 || sw->shape[3] != 4)
    refuse("features.0.0.weight must be a 4x4 conv over 3 channels");
  auto width_ok = [&](int C) {
    if (!dwconv7_supported(C)) refuse("stage width " + std::to_string(C) + " must be a multiple of 32, at most 1536");
  };
  int C = (int)sw->shape[0];
  width_ok(C);
  // patchify's (c, kh, kw) column order is the conv weight's own flattening, as ViT's conv_proj
  m.cn_stem = pack_linear(fdata(sw), has(p, "features.0.0.bias") ? fdata(need(p, "features.0.0.bias")) : nullptr, C, 48, false);
  m.cn_stem_ln = pack_ln(p, "features.0.1");
  const size_t es = m.f16 ? 2 : 4;
  int H = m.image / 4;  // the map's side: every downsample halves it and needs it even
  for (int stage = 0; has(p, feat(2 * stage + 1) + "0.block.0.weight"); ++stage) {
    if (stage > 0) {
      const std::string pre = feat(2 * stage);
      if (H % 2)
        refuse("the downsample before stage " + std::to_string(stage) + " would halve a map of odd side " + std::to_string(H) +
               " (image " + std::to_string(m.image) + " over " + std::to_string(stage) + " stages)");
      H /= 2;
      const spi_named_tensor* dw = need(p, pre + "1.weight");
      if (dw->ndim != 4 || dw->shape[1] != C || dw->shape[2] != 2 || dw->shape[3] != 2)
        refuse(pre + "1.weight must be a 2x2 conv over the " + std::to_string(C) + " channels of stage " + std::to_string(stage - 1));
      const int N = (int)dw->shape[0];
      if (N != 2 * C)
        refuse("stage " + std::to_string(stage) + " has " + std::to_string(N) + " channels: a downsample must double the " +
               std::to_string(C) + " before it");
      width_ok(N);
      CnDown d;
      d.ln = pack_ln(p, pre + "0");
      std::vector<float> wp((size_t)N * 4 * C);
      s2d_permute_weight(fdata(dw), N, C, wp.data());
      d.conv = pack_linear(wp.data(), has(p, pre + "1.bias") ? fdata(need(p, pre + "1.bias")) : nullptr, N, 4 * C, false);
      m.cn_down.push_back(d);
      C = N;
    }
    m.cn_dims.push_back(C);
    int nb = 0;
    for (;; ++nb) {
      const std::string pre = feat(2 * stage + 1) + std::to_string(nb) + ".";
      if (!has(p, pre + "block.0.weight")) break;
      const spi_named_tensor* dw = need(p, pre + "block.0.weight");
      if (dw->ndim != 4 || dw->shape[0] != C || dw->shape[1] != 1 || dw->shape[2] != 7 || dw->shape[3] != 7)
        refuse(pre + "block.0.weight must be a depthwise [C][1][7][7] weight with C = " + std::to_string(C));
      CnBlock blk;
      blk.C = C;
      blk.dw_w = blob.add(nullptr, (size_t)kDwconvTaps * C * es);
      if (m.f16)
        dwconv7_pack_into(reinterpret_cast<_Float16*>(blob.data.data() + blk.dw_w), fdata(dw), C);
      else
        dwconv7_pack_into(reinterpret_cast<float*>(blob.data.data() + blk.dw_w), fdata(dw), C);
      std::vector<float> zeros(C, 0.f);
      blk.dw_b = pack_vec(has(p, pre + "block.0.bias") ? fdata(need(p, pre + "block.0.bias")) : zeros.data(), C);
      blk.ln = pack_ln(p, pre + "block.2");
      blk.fc1 = pack_linear_named(p, pre + "block.3", false);
      // layer_scale [C][1][1] folded into block.5 in fp32, before the compute type's rounding
      const spi_named_tensor* w2 = need(p, pre + "block.5.weight");
      const spi_named_tensor* ls = need(p, pre + "layer_scale");
      if (blk.fc1.k != C || blk.fc1.n < 1 || w2->ndim != 2 || w2->shape[0] != C || w2->shape[1] != blk.fc1.n || numel(ls) != C)
        refuse(pre + "block.3 / block.5 / layer_scale do not chain over " + std::to_string(C) + " channels");
      const int K = blk.fc1.n;
      const float *wsrc = fdata(w2), *g = fdata(ls), *bsrc = fdata(need(p, pre + "block.5.bias"));
      std::vector<float> wf((size_t)C * K), bf(C);
      for (int n = 0; n < C; ++n) {
        for (int k = 0; k < K; ++k) wf[(size_t)n * K + k] = g[n] * wsrc[(size_t)n * K + k];
        bf[n] = g[n] * bsrc[n];
      }
      blk.fc2 = pack_linear(wf.data(), bf.data(), C, K, false);
      m.cn_blocks.push_back(blk);
    }
    m.stage_blocks.push_back(nb);
  }
  if (m.cn_blocks.empty()) refuse("no blocks (features.1.0.block.0.weight)");
  m.final_ln = pack_ln(p, "classifier.0");
  m.fc = pack_linear_named(p, "classifier.2", false);
  if (m.fc.k != C) refuse("classifier.2 reads " + std::to_string(m.fc.k) + " of " + std::to_string(C) + " features");
  m.classes = m.fc.n;
  m.feat = m.fc.k;
}

// torchvision's SwinTransformer (v1): features.0 the stem (4x4 / stride 4 conv, Permute, LayerNorm),
// features.1, 3, 5, 7 the stages of SwinTransformerBlocks, features.2, 4, 6 the PatchMerging layers, norm, head.
// Embed dim, depths, heads per stage and the window are read from the tensors: the bias table is
// [(2 ws - 1)^2][heads].
// SwinTransformer v2 (swin_v2_*) has the same layout with SwinTransformerBlockV2 / PatchMergingV2: every attention
// carries logit_scale [heads,1,1] and cpb_mlp.0.weight [512,2], cpb_mlp.0.bias [512], cpb_mlp.2.weight [heads,512]
// and none a bias table; the names decide the generation, for the whole model.  Heads come from logit_scale, the
// window from the buffer relative_coords_table [1][2 ws - 1][2 ws - 1][2] or, without it, from the config.  Packed
// per block: the bias of 16 sigmoid(cpb_mlp(coords)) (window_cpb_table), tau = exp(min(logit_scale, log 100)), and
// attn.qkv.bias with its K third zeroed, as torchvision's v2 forward zeroes it on every call.
SwBlock Packer::pack_swin_v2_block(const PMap& p, const std::string& pre, int C, int H, int stage) {
  auto refuse = [](const std::string& what) { throw std::runtime_error("swin: " + what); };
  for (const char* name : {"logit_scale", "cpb_mlp.0.weight", "cpb_mlp.0.bias", "cpb_mlp.2.weight"})
    if (!has(p, pre + "attn." + name))
      refuse("Swin-v2: '" + pre + "attn." + name + "' is missing (every attention needs logit_scale, cpb_mlp.0.weight, "
             "cpb_mlp.0.bias and cpb_mlp.2.weight)");
  const spi_named_tensor* ls = need(p, pre + "attn.logit_scale");
  const spi_named_tensor* w0 = need(p, pre + "attn.cpb_mlp.0.weight");
  const spi_named_tensor* b0 = need(p, pre + "attn.cpb_mlp.0.bias");
  const spi_named_tensor* w2 = need(p, pre + "attn.cpb_mlp.2.weight");
  const int heads = (int)numel(ls), ws = m.sw_window;
  if (heads < 1 || C % heads || C / heads != kWinHeadDim)
    refuse(pre + "attn: " + std::to_string(C) + " channels over " + std::to_string(heads) + " heads: head_dim must be 32");
  if (w0->ndim != 2 || w0->shape[1] != 2 || w0->shape[0] < 1 || numel(b0) != w0->shape[0] || w2->ndim != 2 ||
      w2->shape[0] != heads || w2->shape[1] != w0->shape[0])
    refuse("Swin-v2: " + pre + "attn.cpb_mlp must be Linear(2, hidden) + bias and Linear(hidden, " + std::to_string(heads) +
           ") without bias");
  if (H % ws)
    refuse("stage " + std::to_string(stage) + "'s map of side " + std::to_string(H) + " (image " + std::to_string(m.image) +
           ") is no multiple of the window " + std::to_string(ws) + " (padded windows are not served)");
  SwBlock blk;
  blk.C = C;
  blk.heads = heads;
  std::vector<float> table((size_t)(2 * ws - 1) * (2 * ws - 1) * heads), tau(heads);
  window_cpb_table(fdata(w0), fdata(b0), fdata(w2), (int)w0->shape[0], ws, heads, table.data());
  blk.bias = blob.add(nullptr, (size_t)heads * kWinBiasHead * sizeof(float));
  window_bias_pack(table.data(), ws, heads, reinterpret_cast<float*>(blob.data.data() + blk.bias));
  for (int h = 0; h < heads; ++h) tau[h] = window_cos_tau(fdata(ls)[h]);
  blk.tau = pack_vec(tau.data(), heads);
  blk.ln1 = pack_ln(p, pre + "norm1");
  blk.ln2 = pack_ln(p, pre + "norm2");
  const spi_named_tensor* qw = need(p, pre + "attn.qkv.weight");
  if (qw->ndim != 2 || qw->shape[0] != 3 * C || qw->shape[1] != C)
    refuse(pre + "attn.qkv.weight must be [" + std::to_string(3 * C) + "][" + std::to_string(C) + "]");
  std::vector<float> qb(3 * (size_t)C, 0.f);
  if (has(p, pre + "attn.qkv.bias")) {
    const spi_named_tensor* b = need(p, pre + "attn.qkv.bias");
    if (numel(b) != (int64_t)qb.size()) refuse(pre + "attn.qkv.bias must hold " + std::to_string(3 * C) + " values");
    std::copy(fdata(b), fdata(b) + 3 * C, qb.begin());
    std::fill(qb.begin() + C, qb.begin() + 2 * C, 0.f);  // the K third
  }
  blk.qkv = pack_linear(fdata(qw), qb.data(), 3 * C, C, false);
  blk.proj = pack_linear_named(p, pre + "attn.proj", false);
  blk.fc1 = pack_linear_named(p, pre + "mlp.0", false);
  blk.fc2 = pack_linear_named(p, pre + "mlp.3", false);
  if (blk.proj.k != C || blk.proj.n != C || blk.fc1.k != C || blk.fc1.n < 1 || blk.fc2.k != blk.fc1.n || blk.fc2.n != C)
    refuse(pre + "attn.proj / mlp.0 / mlp.3 do not chain over " + std::to_string(C) + " channels");
  return blk;
}

void Packer::build_swin(const PMap& p) {
  auto refuse = [](const std::string& what) { throw std::runtime_error("swin: " + what); };
  auto feat = [](int i) { return "features." + std::to_string(i) + "."; };
  const spi_named_tensor* coords = nullptr;
  std::string v1_name, v2_name;
  for (const auto& kv : p) {
    if (kv.first.find("logit_scale") != std::string::npos || kv.first.find("cpb_mlp") != std::string::npos) v2_name = kv.first;
    if (ends_with(kv.first, "relative_position_bias_table")) v1_name = kv.first;
    if (ends_with(kv.first, "relative_coords_table")) coords = kv.second;
  }
  if (!v1_name.empty() && !v2_name.empty())
    refuse("'" + v2_name + "' is a Swin-v2 parameter (logit_scale / cpb_mlp) beside the v1 table '" + v1_name +
           "': a model is served as one generation");
  m.sw_v2 = !v2_name.empty();
  if (m.sw_v2) {
    int ws = window_cfg;
    if (coords) {
      if (coords->ndim != 4 || coords->shape[1] != coords->shape[2] || coords->shape[1] % 2 == 0 || coords->shape[3] != 2)
        refuse("Swin-v2: relative_coords_table must be [1][2 ws - 1][2 ws - 1][2]");
      ws = (int)(coords->shape[1] + 1) / 2;
    }
    if (ws == 0)
      refuse("Swin-v2: no tensor states the window (no relative_coords_table buffer): set spi_model_config.seq_len to the "
             "tokens of a window, ws^2");
    if (ws < 0) refuse("Swin-v2: seq_len must be the tokens of a square window, ws^2 for ws of 2 .. 8");
    if (!window_supported(ws)) refuse("Swin-v2: window " + std::to_string(ws) + ": a window ws of 2 .. 8 is served");
    m.sw_window = ws;
    if (!image_stated) m.image = 256;  // torchvision's swin_v2_* are trained at 256: 64 / 32 / 16 / 8 maps on 8 x 8 windows
  }
  if (m.image % 4) refuse("image size " + std::to_string(m.image) + " must be a multiple of 4");
  const spi_named_tensor* sw = need(p, "features.0.0.weight");
  if (sw->ndim != 4 || sw->shape[1] != 3 || sw->shape[2] != 4 || sw->shape[3] != 4)
    refuse("features.0.0.weight must be a 4x4 conv over 3 channels");
  auto width_ok = [&](int C) {
    if (!dwconv7_supported(C))
      refuse("stage width " + std::to_string(C) + " must be a multiple of 32, at most 1536 (the LayerNorm row kernel's range)");
  };
  int C = (int)sw->shape[0];
  width_ok(C);
  m.sw_stem = pack_linear(fdata(sw), has(p, "features.0.0.bias") ? fdata(need(p, "features.0.0.bias")) : nullptr, C, 48, false);
  m.sw_stem_ln = pack_ln(p, "features.0.2");
  int H = m.image / 4;
  for (int stage = 0; has(p, feat(2 * stage + 1) + "0.attn.qkv.weight"); ++stage) {
    if (stage > 0) {
      const std::string pre = feat(2 * stage);
      if (H % 2)
        refuse("the merge before stage " + std::to_string(stage) + " would halve a map of odd side " + std::to_string(H));
      if (!s2d_ln_supported(C))
        refuse("the merge before stage " + std::to_string(stage) + (m.sw_v2 ? " gathers rows of " : " normalises rows of ") +
               std::to_string(4 * C) + " columns: at most 2048 (the merge row kernel's range)");
      const spi_named_tensor* rw = need(p, pre + "reduction.weight");
      if (rw->ndim != 2 || rw->shape[1] != 4 * C)
        refuse(pre + "reduction.weight must read the " + std::to_string(4 * C) + " gathered columns of stage " + std::to_string(stage - 1));
      const int N = (int)rw->shape[0];
      if (N != 2 * C)
        refuse("stage " + std::to_string(stage) + " has " + std::to_string(N) + " channels: a merge must double the " +
               std::to_string(C) + " before it");
      width_ok(N);
      SwMerge g;
      g.ln = pack_ln(p, pre + "norm");
      if (m.sw_v2 && numel(need(p, pre + "norm.weight")) != N)
        refuse(pre + "norm: Swin-v2 normalises the " + std::to_string(N) + " columns behind the reduction");
      g.red = pack_linear_named(p, pre + "reduction", false);
      m.sw_merge.push_back(g);
      C = N;
      H /= 2;
    }
    m.sw_dims.push_back(C);
    int nb = 0;
    for (;; ++nb) {
      const std::string pre = feat(2 * stage + 1) + std::to_string(nb) + ".";
      if (!has(p, pre + "attn.qkv.weight")) break;
      if (m.sw_v2) {
        m.sw_blocks.push_back(pack_swin_v2_block(p, pre, C, H, stage));
        continue;
      }
      const spi_named_tensor* tb = need(p, pre + "attn.relative_position_bias_table");
      if (tb->ndim != 2 || tb->shape[1] < 1) refuse(pre + "attn.relative_position_bias_table must be [(2 ws - 1)^2][heads]");
      int ws = 0;
      for (int w = 1; w <= 64 && !ws; ++w)
        if ((int64_t)(2 * w - 1) * (2 * w - 1) == tb->shape[0]) ws = w;
      if (!window_supported(ws))
        refuse(pre + "attn.relative_position_bias_table has " + std::to_string(tb->shape[0]) +
               " rows: (2 ws - 1)^2 for a window ws of 2 .. 8 is served");
      if (m.sw_window && ws != m.sw_window)
        refuse(pre + "attn: window " + std::to_string(ws) + " differs from the " + std::to_string(m.sw_window) + " of the blocks before");
      m.sw_window = ws;
      const int heads = (int)tb->shape[1];
      if (C % heads || C / heads != kWinHeadDim)
        refuse(pre + "attn: " + std::to_string(C) + " channels over " + std::to_string(heads) + " heads: head_dim must be 32");
      if (H % ws)
        refuse("stage " + std::to_string(stage) + "'s map of side " + std::to_string(H) + " (image " + std::to_string(m.image) +
               ") is no multiple of the window " + std::to_string(ws) + " (padded windows are not served)");
      SwBlock blk;
      blk.C = C;
      blk.heads = heads;
      blk.bias = blob.add(nullptr, (size_t)heads * kWinBiasHead * sizeof(float));
      window_bias_pack(fdata(tb), ws, heads, reinterpret_cast<float*>(blob.data.data() + blk.bias));
      blk.ln1 = pack_ln(p, pre + "norm1");
      blk.ln2 = pack_ln(p, pre + "norm2");
      blk.qkv = pack_linear_named(p, pre + "attn.qkv", false);
      blk.proj = pack_linear_named(p, pre + "attn.proj", false);
      blk.fc1 = pack_linear_named(p, pre + "mlp.0", false);
      blk.fc2 = pack_linear_named(p, pre + "mlp.3", false);
      if (blk.qkv.k != C || blk.qkv.n != 3 * C || blk.proj.k != C || blk.proj.n != C || blk.fc1.k != C || blk.fc1.n < 1 ||
          blk.fc2.k != blk.fc1.n || blk.fc2.n != C)
        refuse(pre + "attn.qkv / attn.proj / mlp.0 / mlp.3 do not chain over " + std::to_string(C) + " channels");
      m.sw_blocks.push_back(blk);
    }
    m.stage_blocks.push_back(nb);
  }
  if (m.sw_blocks.empty()) refuse("no blocks (features.1.0.attn.qkv.weight)");
  m.final_ln = pack_ln(p, "norm");
  m.fc = pack_linear_named(p, "head", false);
  if (m.fc.k != C) refuse("head reads " + std::to_string(m.fc.k) + " of " + std::to_string(C) + " features");
  m.classes = m.fc.n;
  m.feat = m.fc.k;
}

// torchvision's EfficientNet (b0 .. b7): features.0 the stem (3x3 / stride 2 conv, BatchNorm, SiLU), features.1 .. 7
// the stages of MBConv blocks, features.8 the 1x1 head conv, classifier.1 the Linear.  A block's `block` holds
// [expand 1x1 (absent at expand ratio 1)], depthwise k x k, squeeze-excitation (fc1, fc2), project 1x1.  The
// strides are not in the parameters: torchvision's stages open with strides 1, 2, 2, 2, 1, 2, 1.
void Packer::build_efficientnet(const PMap& p) {
  auto refuse = [](const std::string& what) { throw std::runtime_error("efficientnet: " + what); };
  static const int kStageStride[7] = {1, 2, 2, 2, 1, 2, 1};
  if (m.image % 32) refuse("image size " + std::to_string(m.image) + " must be a multiple of 32");
  auto channels_ok = [&](const std::string& what, int C) {
    if (!mbconv_channels_ok(C)) refuse(what + " has " + std::to_string(C) + " channels: a multiple of 8 from 8 to 4608 is served");
  };
  // a 1x1 conv + BatchNorm as a dense layer over NHWC rows
  auto pointwise = [&](const std::string& pre, int cin) {
    const FoldedConv f = fold_conv(p, pre + "0", pre + "1", m.eps);
    if (f.kh != 1 || f.kw != 1 || f.cin != cin)
      refuse(pre + "0.weight must be a 1x1 conv over " + std::to_string(cin) + " channels");
    return pack_linear(f.w.data(), f.b.data(), f.cout, f.cin, false);
  };
  const FoldedConv sf = fold_conv(p, "features.0.0", "features.0.1", m.eps);
  if (sf.cin != 3 || sf.kh != 3 || sf.kw != 3) refuse("features.0.0.weight must be a 3x3 conv over 3 channels");
  channels_ok("the stem", sf.cout);
  m.stem = pack_conv(sf, 2, m.f16 ? 8 : 4, m.prec);
  const size_t es = m.f16 ? 2 : 4;
  int C = sf.cout, stage = 0;
  for (; has(p, "features." + std::to_string(stage + 1) + ".0.block.0.0.weight"); ++stage) {
    if (stage >= 7) refuse("more than 7 MBConv stages: their strides are torchvision's 1, 2, 2, 2, 1, 2, 1");
    int nb = 0;
    for (;; ++nb) {
      const std::string pre = "features." + std::to_string(stage + 1) + "." + std::to_string(nb) + ".block.";
      if (!has(p, pre + "0.0.weight")) break;
      MbBlock b;
      b.cin = C;
      b.stride = nb == 0 ? kStageStride[stage] : 1;
      b.has_expand = has(p, pre + "3.0.weight");
      const int e = b.has_expand ? 1 : 0;
      const std::string dw = pre + std::to_string(e) + ".", se = pre + std::to_string(e + 1) + ".", pj = pre + std::to_string(e + 2) + ".";
      if (b.has_expand) b.expand = pointwise(pre + "0.", C);
      b.mid = b.has_expand ? b.expand.n : C;
      channels_ok(pre + "'s expanded map", b.mid);
      const FoldedConv df = fold_conv(p, dw + "0", dw + "1", m.eps);
      if (df.cin != 1 && df.cin == C && df.kh == 3)
        refuse(dw + "0.weight is a dense 3x3 conv over " + std::to_string(C) +
               " channels where the depthwise conv belongs: EfficientNetV2's fused-MBConv blocks are not served");
      if (df.cout != b.mid || df.cin != 1 || df.kh != df.kw || (df.kh != 3 && df.kh != 5))
        refuse(dw + "0.weight must be a depthwise [C][1][3|5][3|5] weight with C = " + std::to_string(b.mid) +
               (b.has_expand ? "" : " (a block without an expand conv: expand ratio 1)"));
      b.k = df.kh;
      b.dw_w = blob.add(nullptr, (size_t)b.k * b.k * b.mid * es);
      if (m.f16)
        dwconv_pack_into(reinterpret_cast<_Float16*>(blob.data.data() + b.dw_w), df.w.data(), b.mid, b.k);
      else
        dwconv_pack_into(reinterpret_cast<float*>(blob.data.data() + b.dw_w), df.w.data(), b.mid, b.k);
      b.dw_b = pack_vec(df.b.data(), b.mid);
      if (!has(p, se + "fc1.weight") || !has(p, se + "fc2.weight"))
        refuse(se + "fc1 / fc2 are missing: an MBConv block without squeeze-and-excitation is not an EfficientNet's");
      const spi_named_tensor *w1 = need(p, se + "fc1.weight"), *w2 = need(p, se + "fc2.weight");
      const spi_named_tensor *b1 = need(p, se + "fc1.bias"), *b2 = need(p, se + "fc2.bias");
      b.sq = w1->ndim == 4 ? (int)w1->shape[0] : 0;
      if (b.sq < 1 || numel(w1) != (int64_t)b.sq * b.mid || w2->ndim != 4 || w2->shape[0] != b.mid ||
          numel(w2) != (int64_t)b.sq * b.mid || numel(b1) != b.sq || numel(b2) != b.mid)
        refuse(se + "fc1 / fc2 must be 1x1 convs " + std::to_string(b.mid) + " -> squeeze -> " + std::to_string(b.mid));
      if (b.sq > kSeMaxSq) refuse(se + "fc1 squeezes to " + std::to_string(b.sq) + " channels: at most 256 are served");
      b.se_w1 = pack_vec(fdata(w1), b.sq * b.mid), b.se_b1 = pack_vec(fdata(b1), b.sq);
      b.se_w2 = pack_vec(fdata(w2), b.sq * b.mid), b.se_b2 = pack_vec(fdata(b2), b.mid);
      b.project = pointwise(pj, b.mid);
      b.cout = b.project.n;
      channels_ok(pj + "0", b.cout);
      b.residual = b.stride == 1 && b.cin == b.cout;
      m.mb_blocks.push_back(b);
      C = b.cout;
    }
    m.stage_blocks.push_back(nb);
  }
  if (m.mb_blocks.empty()) refuse("no blocks (features.1.0.block.0.0.weight)");
  const std::string head = "features." + std::to_string(stage + 1) + ".";
  m.mb_head = pointwise(head, C);
  m.fc = pack_linear_named(p, "classifier.1", false);
  if (m.fc.k != m.mb_head.n)
    refuse("classifier.1 reads " + std::to_string(m.fc.k) + " of " + std::to_string(m.mb_head.n) + " features");
  m.classes = m.fc.n;
  m.feat = m.fc.k;
}

}  // namespace

PackedModel pack_model(const spi_model_config& cfg, const spi_named_tensor* params, int n) {
  const bool f16 = cfg.precision == SPI_PREC_F16 || cfg.precision == SPI_PREC_F16M;
  if (!f16 && cfg.precision != SPI_PREC_F32 && cfg.precision != SPI_PREC_F16X3)
    throw std::runtime_error("unsupported precision");
  Packer pk;
  PackedModel& m = pk.m;
  m.family = cfg.family;
  m.prec = f16 ? Prec::F16 : cfg.precision == SPI_PREC_F16X3 ? Prec::F16X3 : Prec::F32;
  m.f16 = f16;
  m.max_batch = std::max(1, cfg.max_batch);
  // F16M: ResNet stem / downsample, every transformer GEMM with hi + lo weights
  m.mixed = cfg.precision == SPI_PREC_F16M && cfg.family != SPI_FAMILY_AFFINE;
  m.heads = cfg.num_heads;
  if (cfg.image_size > 0) m.image = cfg.image_size;
  for (int w = 1; w <= 256 && cfg.seq_len > 0; ++w)
    if (w * w >= cfg.seq_len) {
      pk.window_cfg = w * w == cfg.seq_len ? w : -1;  // -1: not a square
      break;
    }
  pk.image_stated = cfg.image_size > 0;
  PMap p;
  for (int i = 0; i < n; ++i) {
    if (!params[i].name) throw std::runtime_error("parameter without a name");
    p[params[i].name] = &params[i];
  }
  if (m.family == SPI_FAMILY_AUTO) {
    if (ends_with(p, "embeddings.word_embeddings.weight")) m.family = SPI_FAMILY_BERT;
    else if (ends_with(p, "conv_proj.weight") && ends_with(p, "class_token")) m.family = SPI_FAMILY_VIT;
    else if (ends_with(p, "layer1.0.conv1.weight")) m.family = SPI_FAMILY_RESNET;
    else if (ends_with(p, "features.0.0.weight") && ends_with(p, "features.1.0.block.0.weight") &&
             ends_with(p, "features.1.0.layer_scale"))
      m.family = SPI_FAMILY_CONVNEXT;
    else if (ends_with(p, "features.0.0.weight") && (ends_with(p, "features.1.0.attn.relative_position_bias_table") ||
                                                     ends_with(p, "features.1.0.attn.logit_scale")))
      m.family = SPI_FAMILY_SWIN;
    else if (ends_with(p, "features.0.0.weight") && ends_with(p, "features.1.0.block.0.0.weight") &&
             ends_with(p, "classifier.1.weight"))
      m.family = SPI_FAMILY_EFFICIENTNET;
    else throw std::runtime_error("unrecognised model: no ResNet/BERT/ViT/ConvNeXt/Swin/EfficientNet parameter names");
  }
  if (const int io = cfg.bert_io) {  // spi_codelet.h: enum spi_bert_io
    constexpr int heads = SPI_BERT_HEAD_SEQUENCE | SPI_BERT_HEAD_TOKEN | SPI_BERT_HEAD_QA;
    constexpr int known =
        SPI_BERT_OUT_POOLER | SPI_BERT_OUT_MEAN | SPI_BERT_NO_HIDDEN | SPI_BERT_TOKEN_TYPES | heads | SPI_BERT_POS_FROM_IDS;
    if (io & ~known) throw std::runtime_error("bert_io: unknown bits " + std::to_string(io & ~known));
    if (m.family != SPI_FAMILY_BERT) throw std::runtime_error("bert_io is set, but the model is not a BERT");
    if ((io & heads) & ((io & heads) - 1))
      throw std::runtime_error("bert_io: at most one of SPI_BERT_HEAD_SEQUENCE, SPI_BERT_HEAD_TOKEN, SPI_BERT_HEAD_QA");
    if ((io & SPI_BERT_NO_HIDDEN) && !(io & (SPI_BERT_OUT_POOLER | SPI_BERT_OUT_MEAN | heads)))
      throw std::runtime_error("bert_io: SPI_BERT_NO_HIDDEN leaves no output; select SPI_BERT_OUT_POOLER or SPI_BERT_OUT_MEAN");
    m.bert_io = io & ~SPI_BERT_POS_FROM_IDS;
    m.pos_from_ids = (io & SPI_BERT_POS_FROM_IDS) != 0;
  }
  pk.blob.add(nullptr, 256);  // offset 0: zero line read by the GEMM for padded chunks
  std::ostringstream os;
  if (m.family == SPI_FAMILY_AFFINE) {
    m.aff_scale = cfg.affine_scale;
    m.aff_shift = cfg.affine_shift;
    os << "affine(x*" << m.aff_scale << "+" << m.aff_shift << ") f32";
  } else if (m.family == SPI_FAMILY_RESNET) {
    m.eps = cfg.eps > 0 ? cfg.eps : 1e-5f;
    pk.build_resnet(strip_prefix(p, "layer1.0.conv1.weight"));
    os << "resnet" << (m.bottleneck ? "-bottleneck[" : "-basic[");
    for (size_t i = 0; i < m.stage_blocks.size(); ++i) os << (i ? "," : "") << m.stage_blocks[i];
    os << "]";
    if (m.groups > 1) os << " g" << m.groups;
    os << " img" << m.image << " classes" << m.classes;
  } else if (m.family == SPI_FAMILY_BERT) {
    m.eps = cfg.eps > 0 ? cfg.eps : 1e-12f;
    m.ln_fold = ln_fold_enabled(m.prec, kBertLnFold);
    m.seq = cfg.seq_len;
    pk.build_bert(strip_prefix(p, "embeddings.word_embeddings.weight"), p);
    os << "bert L" << m.layers << " D" << m.D << " H" << m.heads << " FF" << m.ffn << " S<=" << m.seq;
  } else if (m.family == SPI_FAMILY_VIT) {
    m.eps = cfg.eps > 0 ? cfg.eps : 1e-6f;
    m.ln_fold = ln_fold_enabled(m.prec, kVitLnFold);
    pk.build_vit(strip_prefix(p, "conv_proj.weight"));
    os << "vit L" << m.layers << " D" << m.D << " H" << m.heads << " MLP" << m.ffn << " patch" << m.patch
       << " img" << m.image << " classes" << m.classes;
  } else if (m.family == SPI_FAMILY_CONVNEXT) {
    if (cfg.precision != SPI_PREC_F16 && cfg.precision != SPI_PREC_F32)
      throw std::runtime_error(
          "convnext: SPI_PREC_F16X3 and SPI_PREC_F16M are not served for this family; use SPI_PREC_F16 or SPI_PREC_F32");
    m.eps = cfg.eps > 0 ? cfg.eps : 1e-6f;
    pk.build_convnext(strip_prefix(p, "features.0.0.weight"));
    os << "convnext[";
    for (size_t i = 0; i < m.stage_blocks.size(); ++i) os << (i ? "," : "") << m.stage_blocks[i];
    os << "] C" << m.cn_dims.front() << " img" << m.image << " classes" << m.classes;
  } else if (m.family == SPI_FAMILY_SWIN) {
    if (cfg.precision != SPI_PREC_F16 && cfg.precision != SPI_PREC_F32)
      throw std::runtime_error(
          "swin: SPI_PREC_F16X3 and SPI_PREC_F16M are not served for this family; use SPI_PREC_F16 or SPI_PREC_F32");
    m.eps = cfg.eps > 0 ? cfg.eps : 1e-5f;
    pk.build_swin(strip_prefix(p, "features.0.0.weight"));
    os << (m.sw_v2 ? "swin_v2[" : "swin[");
    for (size_t i = 0; i < m.stage_blocks.size(); ++i) os << (i ? "," : "") << m.stage_blocks[i];
    os << "] C" << m.sw_dims.front() << " ws" << m.sw_window << " img" << m.image << " classes" << m.classes;
  } else if (m.family == SPI_FAMILY_EFFICIENTNET) {
    if (cfg.precision != SPI_PREC_F16 && cfg.precision != SPI_PREC_F32)
      throw std::runtime_error(
          "efficientnet: SPI_PREC_F16X3 and SPI_PREC_F16M are not served for this family; use SPI_PREC_F16 or SPI_PREC_F32");
    m.eps = cfg.eps > 0 ? cfg.eps : 1e-5f;
    pk.build_efficientnet(strip_prefix(p, "features.0.0.weight"));
    os << "efficientnet[";
    for (size_t i = 0; i < m.stage_blocks.size(); ++i) os << (i ? "," : "") << m.stage_blocks[i];
    os << "] C" << m.stem.cout << " img" << m.image << " classes" << m.classes;
  } else {
    throw std::runtime_error("unsupported model family");
  }
  os << (m.mixed ? " f16m" : m.prec == Prec::F16 ? " f16" : m.prec == Prec::F16X3 ? " f16x3" : " f32") << " maxB"
     << m.max_batch;
  if (m.bert_io) {
    std::string outs;
    for (const auto& o : {std::make_pair(!(m.bert_io & SPI_BERT_NO_HIDDEN), "hidden"),
                          std::make_pair((m.bert_io & SPI_BERT_OUT_POOLER) != 0, "pooler"),
                          std::make_pair((m.bert_io & SPI_BERT_OUT_MEAN) != 0, "mean")})
      if (o.first) outs += (outs.empty() ? "" : ",") + std::string(o.second);
    const std::string L = std::to_string(m.num_labels);
    const std::string head = (m.bert_io & SPI_BERT_HEAD_SEQUENCE) ? "seq_logits" + L
                             : (m.bert_io & SPI_BERT_HEAD_TOKEN)  ? "token_logits" + L
                             : (m.bert_io & SPI_BERT_HEAD_QA)     ? "qa_start,qa_end"
                                                                  : "";
    if (!head.empty()) outs += (outs.empty() ? "" : ",") + head;
    os << " out[" << outs << "] in[ids,mask" << ((m.bert_io & SPI_BERT_TOKEN_TYPES) ? ",types]" : "]");
  }
  if (m.pos_from_ids) os << " pos[ids]";
  if (m.rel_buckets) os << " relbias" << m.rel_buckets;
  m.desc = os.str();
  m.blob = std::move(pk.blob.data);
  m.blob_bytes = m.blob.size();
  uint64_t h = 1469598103934665603ull;  // FNV-1a 64
  for (char c : m.blob) h = (h ^ (uint8_t)c) * 1099511628211ull;
  m.digest = h;
  return std::move(pk.m);
}

}  // namespace spi
