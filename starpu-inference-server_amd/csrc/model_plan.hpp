// Host-only forward plans of a model replica: the I/O contract, the descriptor of every GEMM / conv
// a forward launches, the one walk over the ResNet graph, the FLOP count and the workspace sizes.
// Plain C++17, no HIP: Model (model.cpp) launches from these descs and this walk and allocates from
// workspace_plan, so what sizes a launch is what launches; `make plan_check` runs it all under the
// sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "gemm_plan.hpp"
#include "image_src.hpp"
#include "model_pack.hpp"

namespace spi {

constexpr size_t kCounterSlots = 16384;  // >= tiles of any split GEMM (checked per launch)

// What the setters of a replica select (Model::set_image_outputs, set_input_resize).
struct ReplicaOptions {
  int image_io = 0, top_k = 0;  // ResNet / ViT: SPI_IMAGE_* bits and the top-k count
  int resize_short = 0;         // ResNet / ViT: the input resize of 8-bit tasks, 0 = off
};

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
// class-token rows, fp32 (SPI_BERT_NO_HIDDEN with the pooler alone), followed max_batch x D floats on by
// the sequence head's pooled vector when the pooler is not an output.
enum BertBuf { kBtHidden, kBtHidden16, kBtQkv, kBtCtx, kBtAttn, kBtFfn, kBtStats1, kBtStats2, kBtCls, kBtBufs };
// ViT: patches (plus vit_patches_tail_bytes, zeroed, where the rows are ragged); projected patches f32; residual stream x f32 (fold: two fp16 planes); LN output; qkv;
// ctx; mlp hidden; the LayerNorm'd class-token rows; the LayerNorm-fold row statistics of x.
enum VitBuf { kVtPatches, kVtProj, kVtX, kVtLn, kVtQkv, kVtCtx, kVtMlp, kVtCls, kVtStats, kVtLogits, kVtResized, kVtBufs };

// ---------------------------------------------------------------------------
// I/O contract
// ---------------------------------------------------------------------------
int num_inputs_max(const PackedModel& m);
// BERT: the outputs bert_io selects, in order hidden, pooler, mean, the head's.  ResNet / ViT: the outputs
// image_io selects, in order logits, probabilities, top-k values, top-k indices.
int num_outputs(const PackedModel& m, const ReplicaOptions& o);
// Validates the task's I/O against the replica; throws std::runtime_error with the reference's
// message wording on mismatch.
void check_io(const PackedModel& m, const ReplicaOptions& o, const spi_codelet_args& a, const size_t* in_bytes,
              const size_t* out_bytes);
// What input 0 of a task that passed check_io holds: fp32 NCHW, or for a ResNet / ViT task of
// SPI_DTYPE_U8 the layout its dims name ([B,3,S,S] NCHW, [B,S,S,3] NHWC) -- with the input resize on,
// [B,3,H,W] / [B,H,W,3] and the source size, which sends the task through the resample first.
ImageSrc input_kind(const PackedModel& m, const ReplicaOptions& o, const spi_codelet_args& a);
// The packer's description plus " out[...]" (image_io) and " resize<R>" (resize_short).
std::string replica_desc(const PackedModel& m, const ReplicaOptions& o);
// The argument checks of the setters: an spi_status and, on refusal, the message in `err` (the input
// transform: the checked values in `xf`; null pointers reset it to scale 1, shift 0).
int check_image_outputs(const PackedModel& m, int image_io, int top_k, std::string& err);
int check_input_resize(const PackedModel& m, int resize_short, std::string& err);
int check_input_transform(const PackedModel& m, const float* scale, const float* shift, InputXf& xf);

// ---------------------------------------------------------------------------
// Layer descriptors: the only places in the model layer that set fields of a GemmDesc.  The shared
// builders (gemm_desc.hpp) on the packed layer's sizes; the packer (model_pack.cpp) sized the W rows,
// and a row length the builder does not arrive at is a packing bug (std::logic_error).
// ---------------------------------------------------------------------------
// A conv of the ResNet graph over B maps of H x W.  (The stem reads the ingested fp32 image: no a_split.)
GemmDesc conv_layer_desc(const PackedModel& m, const ConvW& c, int B, int H, int W, Act act, bool out_f32 = false,
                         bool res_f32 = false);
// A linear layer outside the encoder stack over M dense rows, fp32 out: ViT's patch projection and
// head, the ResNet FC on the pooled features.
GemmDesc linear_layer_desc(const LinearW& L, int M);
// avgpool + fc as one GEMM over every pixel of the last stage with a column-mean epilogue
// (GemmDesc::pool_rows): the split / fp16 / fp32 activation is the A operand as is, so the pooled
// vector never goes through HBM.
bool pooled_fc(const PackedModel& m, int hw);
GemmDesc pooled_fc_desc(const PackedModel& m, int B, int hw);
// The four GEMMs of encoder layer `layer` over T token rows, as the family's body launches them: plain
// (BERT post-LN, ViT pre-LN), or under PackedModel::ln_fold with the LayerNorms folded in -- then
// layer 0 differs, its input rows are not yet two-plane.  Throws when a folding GEMM's weights were
// not packed folded.
enum TfGemm { kQkv, kOut, kFf1, kFf2 };
inline const LinearW& tf_linear(const TfLayer& L, TfGemm g) {
  return g == kQkv ? L.qkv : g == kOut ? L.out : g == kFf1 ? L.ff1 : L.ff2;
}
GemmDesc tf_gemm_desc(const PackedModel& m, int layer, TfGemm g, int T);

// Every GEMM a transformer forward of B tasks (BERT: of S tokens each) may launch, in order:
// f(name, layer weights, desc).  The QKV GEMM is listed also where the fused QKV + attention kernel
// runs instead.
template <class F>
void walk_transformer_gemms(const PackedModel& m, int B, int S, F&& f) {
  const bool vit = m.family == SPI_FAMILY_VIT;
  const int T = B * (vit ? m.npatch + 1 : S);
  static const char* const kNames[] = {"qkv", "out", "ff1", "ff2"};
  if (vit) f("patch_proj", m.patch_proj, linear_layer_desc(m.patch_proj, B * m.npatch));
  for (int i = 0; i < m.layers; ++i)
    for (TfGemm g : {kQkv, kOut, kFf1, kFf2}) f(kNames[g], tf_linear(m.tf[i], g), tf_gemm_desc(m, i, g, T));
  if (vit) f("head", m.head, linear_layer_desc(m.head, B));
}

// ---------------------------------------------------------------------------
// The ResNet graph, walked once: Model::body_resnet launches from it, model_flops counts it,
// workspace_plan sizes it.
// ---------------------------------------------------------------------------
inline int conv_out(int H, const ConvW& c) { return (H + 2 * c.pad - c.kh) / c.stride + 1; }
struct StemGeom {
  int OH, PH;  // the 7x7 / stride 2 / pad 3 stem's output side, the 3x3 / stride 2 / pad 1 max pool's
};
inline StemGeom stem_geom(const PackedModel& m) {
  const int OH = conv_out(m.image, m.stem);
  return {OH, (OH + 2 - 3) / 2 + 1};
}
// One conv over H x H maps: activation slots (RnBuf) of its input, output and residual (-1: none).
struct RnConv {
  const ConvW& c;
  int H, in, out, res;
};
// The visitor V sees, in launch order:
//   v.stem(B, g)             the stem conv + max pool, kRnIngest -> kRnAct0 -> kRnAct1 (fused, PackedModel::
//                            stem_fused: one launch of the prologue's, straight into kRnAct1)
//   v.conv(B, RnConv)        a conv + ReLU (ConvW::gconv: the grouped kernel), with its residual if any
//   v.conv_pair(B, c1, ds)   a block's first conv (+ ReLU) and its downsample conv: same input
//   v.tail(B, slot, hw, fused) the last stage's output: avgpool into kRnPooled then the FC, or (fused)
//                            the pooled FC on the slot itself
template <class V>
void walk_resnet(const PackedModel& m, int B, V&& v) {
  v.stem(B, stem_geom(m));
  int H = stem_geom(m).PH, cur = kRnAct1;
  auto pick = [](std::initializer_list<int> busy) {  // the first activation slot not in use
    for (int i = kRnAct0; i <= kRnAct4; ++i)
      if (std::find(busy.begin(), busy.end(), i) == busy.end()) return i;
    return -1;
  };
  for (const ResBlock& b : m.blocks) {
    int last = pick({cur}), ident = cur;  // last: the slot of the block's latest intermediate
    if (b.has_ds) {  // the downsample reads the block input too: grouped with conv1
      ident = pick({cur, last});
      v.conv_pair(B, RnConv{b.c1, H, cur, last, -1}, RnConv{b.ds, H, cur, ident, -1});
    } else {
      v.conv(B, RnConv{b.c1, H, cur, last, -1});
    }
    H = conv_out(H, b.c1);
    if (m.bottleneck) {  // conv1 is 1x1 / stride 1; conv2 (dense or grouped) carries the stride
      const int t2 = pick({cur, last, ident});
      v.conv(B, RnConv{b.c2, H, last, t2, -1});
      H = conv_out(H, b.c2);
      last = t2;
    }
    const int o = pick({cur, last, ident});
    v.conv(B, RnConv{m.bottleneck ? b.c3 : b.c2, H, last, o, ident});
    cur = o;
  }
  v.tail(B, cur, H * H, pooled_fc(m, H * H));
}

// ---------------------------------------------------------------------------
// FLOPs and workspace
// ---------------------------------------------------------------------------
double model_flops(const PackedModel& m, int64_t B);

// BERT's kBtCls buffer: the class-token rows [max_batch][D] fp32 under SPI_BERT_NO_HIDDEN, then the sequence
// head's pooled vector [max_batch][D] fp32 when the pooler is not an output.  workspace_plan sizes the buffer
// and the epilogue addresses the pooled vector from these two.
inline size_t bert_cls_rows_floats(const PackedModel& m) {
  return (m.bert_io & SPI_BERT_NO_HIDDEN) ? (size_t)m.max_batch * m.D : 0;
}
inline size_t bert_pooled_ws_floats(const PackedModel& m) {
  return (m.bert_io & SPI_BERT_HEAD_SEQUENCE) && !(m.bert_io & SPI_BERT_OUT_POOLER) ? (size_t)m.max_batch * m.D : 0;
}
// ViT's kVtPatches rows are patch_proj.k elements long and the dense GEMM stages A in 16-byte chunks, taking a
// chunk whenever its first element lies inside K.  With a row that is no whole number of chunks (patch 14:
// K = 588 fp16) the last chunk runs into the next row -- finite values against zero weights -- and on the
// last row past the rows: the buffer ends with this many zeroed bytes for it to read.
inline size_t vit_patches_tail_bytes(const PackedModel& m) {
  return m.family == SPI_FAMILY_VIT && ((size_t)m.patch_proj.k * (m.f16 ? 2 : 4)) % 16 != 0 ? 16 : 0;
}

struct WorkspacePlan {
  std::vector<size_t> bytes;   // per buffer of the family's enum, at max_batch
  size_t partial_floats = 0;   // the split-K slabs: the floor below at least
  size_t partial_planned = 0;  // ... before the floor: the largest any launch at max_batch plans
};
WorkspacePlan workspace_plan(const PackedModel& m, const ReplicaOptions& o);

// Walks the forward at batch B (BERT: sequence S) launching nothing, and holds every GEMM, conv and conv
// pair against the planned workspace as the launch does (gemm_workspace_fits with kCounterSlots).
// Returns the number of steps; throws std::runtime_error naming the first step that does not fit.
int plan_check(const PackedModel& m, const ReplicaOptions& o, int B, int S);
inline bool launch_fits(const GemmDesc& d, Prec prec, size_t partial_floats, const GemmDesc* d1 = nullptr) {
  return gemm_workspace_fits(d, prec, partial_floats, kCounterSlots, d1);
}

}  // namespace spi
