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

#include "gconv.hpp"
#include "ln_fold_pack.hpp"
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
  const spi_named_tensor* te = need(p, "embeddings.token_type_embeddings.weight");
  m.type0 = pack_vec(fdata(te), D);  // token_type_ids buffer is all zeros
  m.emb_ln = pack_ln(p, "embeddings.LayerNorm");
  auto layer = [](int i) { return "encoder.layer." + std::to_string(i) + "."; };
  while (has(p, layer(m.layers) + "attention.self.query.weight")) ++m.layers;
  if (m.layers == 0) throw std::runtime_error("bert: no encoder layers");
  // Q, K, V stacked into one [3D][D] projection.
  std::vector<float> qw((size_t)3 * D * D), qb((size_t)3 * D);
  auto stack_qkv = [&](const std::string& pre) {
    const char* names[3] = {"query", "key", "value"};
    for (int j = 0; j < 3; ++j) {
      const std::string nm = pre + "attention.self." + names[j];
      std::memcpy(qw.data() + (size_t)j * D * D, fdata(need(p, nm + ".weight")), sizeof(float) * D * D);
      std::memcpy(qb.data() + (size_t)j * D, fdata(need(p, nm + ".bias")), sizeof(float) * D);
    }
  };
  for (int i = 0; i < m.layers; ++i) {
    const std::string pre = layer(i);
    TfLayer L;
    stack_qkv(pre);
    L.qkv = pack_linear(qw.data(), qb.data(), 3 * D, D, m.mixed);
    L.out = pack_linear_named(p, pre + "attention.output.dense", m.mixed);
    L.ln1 = pack_ln(p, pre + "attention.output.LayerNorm");
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
                                     fdata(need(p, pre + "intermediate.dense.bias")), m.ffn, D, p,
                                     pre + "attention.output.LayerNorm");
    if (i == 0) continue;
    stack_qkv(pre);
    m.tf[i].qkv = pack_linear_folded(qw.data(), qb.data(), 3 * D, D, p, layer(i - 1) + "output.LayerNorm");
  }
  // bert_io appends only: a replica without bits keeps the blob above, byte for byte
  m.type_vocab = (int)te->shape[0];
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
  PMap p;
  for (int i = 0; i < n; ++i) {
    if (!params[i].name) throw std::runtime_error("parameter without a name");
    p[params[i].name] = &params[i];
  }
  if (m.family == SPI_FAMILY_AUTO) {
    if (ends_with(p, "embeddings.word_embeddings.weight")) m.family = SPI_FAMILY_BERT;
    else if (ends_with(p, "conv_proj.weight") && ends_with(p, "class_token")) m.family = SPI_FAMILY_VIT;
    else if (ends_with(p, "layer1.0.conv1.weight")) m.family = SPI_FAMILY_RESNET;
    else throw std::runtime_error("unrecognised model: no ResNet/BERT/ViT parameter names");
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
  m.desc = os.str();
  m.blob = std::move(pk.blob.data);
  m.blob_bytes = m.blob.size();
  uint64_t h = 1469598103934665603ull;  // FNV-1a 64
  for (char c : m.blob) h = (h ^ (uint8_t)c) * 1099511628211ull;
  m.digest = h;
  return std::move(pk.m);
}

}  // namespace spi
