// Host-only weight packer of a model replica: recognise the torchvision / HF parameter names, fold
// BN (and, on the fp16 transformers, the LayerNorms) into the weights, pack every contraction weight
// [Npad][Kpad] in the compute type, and lay everything out in one blob.  Plain data in, plain data
// out, no HIP: Model (model.hpp) uploads the blob and runs the forward plans over the offset tables.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/spi_codelet.h"
#include "gemm_desc.hpp"

namespace spi {

struct ConvW {
  size_t w = 0, b = 0;  // blob offsets (packed weight, fp32 bias)
  int cout = 0, cin = 0, cin_pad = 0, kh = 1, kw = 1, stride = 1, pad = 0;
  int kpad = 0, npad = 0;
  size_t wplane = 0;
  Prec prec = Prec::F16;  // packing / contraction precision of this conv
  int krep = 1;           // 2: hi + lo weight steps per A step (GemmDesc::krep; SPI_PREC_F16M)
  bool w_image = false;   // the packed rows 64..127 hold conv_wres's LDS image (GemmDesc::w_image)
  // A grouped conv (ResNeXt conv2): cin stays the full channel count, group g reads and writes channels
  // [g cin / groups, ...).  gconv: w holds the grouped kernel's layout (gconv.hpp; kpad = npad = 0, no
  // GEMM plan); else w is the dense [cout][kh][kw][cin] expansion with zeros off the group.
  int groups = 1;
  bool gconv = false;
};

struct LinearW {
  size_t w = 0, b = 0;
  size_t c1 = 0;  // LayerNorm fold (GemmDesc::ln_in_chunks): sum_k W'[n][k] of the folded weights, else 0
  int n = 0, k = 0, kpad = 0, npad = 0;
  size_t wplane = 0;
  bool has_bias = true;
  Prec prec = Prec::F16;
  int krep = 1;
};

struct LnW {
  size_t g = 0, b = 0;
};

struct ResBlock {
  ConvW c1, c2, c3;  // c3 only for bottleneck
  bool has_ds = false;
  ConvW ds;  // SPI_PREC_F16M: packed hi + lo (krep = 2), fp32 output
};

struct TfLayer {  // BERT (post-LN) / ViT (pre-LN) encoder layer
  LinearW qkv, out, ff1, ff2;
  LnW ln1, ln2;
};

struct CnBlock {  // ConvNeXt block: depthwise 7x7 + LayerNorm (dwconv_ln.hip), Linear C -> 4C, GELU, Linear 4C -> C
  int C = 0;
  size_t dw_w = 0, dw_b = 0;  // [49][C] in the compute type, fp32 [C]
  LnW ln;
  LinearW fc1, fc2;  // fc2 with layer_scale folded in: W' = diag(gamma) W, b' = gamma b
};

struct CnDown {  // ConvNeXt stage change: LayerNorm2d, then the 2x2 / stride 2 conv as a dense GEMM with K = 4 C
  LnW ln;
  LinearW conv;  // [2 C][(kh 2 + kw) C + c] (convnext_pack.hpp)
};

struct SwBlock {  // Swin block: norm1, QKV, shifted-window attention (window_attn.hip), proj + x, norm2, MLP + x
  // v2 (PackedModel::sw_v2), residual-post-norm: QKV on x, cosine attention, proj, x + norm1(.), MLP, x + norm2(.)
  int C = 0, heads = 0;
  size_t bias = 0;  // fp32 [heads][16][64][4] (swin_pack.hpp: window_bias_pack); v2: of window_cpb_table's table
  size_t tau = 0;   // v2: fp32 [heads], exp(min(logit_scale, log 100))
  LnW ln1, ln2;
  LinearW qkv, proj, fc1, fc2;
};

struct SwMerge {  // Swin patch merging: gather 2x2 + LayerNorm over 4 C (s2d_ln), then the bias-free Linear 4 C -> 2 C
  // v2: gather (s2d_rows), the Linear, then LayerNorm over 2 C (ln_rows)
  LnW ln;
  LinearW red;  // torch's [2 C][4 C] as it is
};

struct MbBlock {  // EfficientNet MBConv: [1x1 expand + SiLU], depthwise k x k + SiLU, squeeze-excite, 1x1 project [+ x]
  int cin = 0, mid = 0, cout = 0, k = 3, stride = 1, sq = 0;
  bool has_expand = false, residual = false;  // expand ratio 1 has no expand conv; stride 1 and cin == cout add x
  LinearW expand, project;     // the 1x1 convs as dense layers over NHWC rows, BatchNorm folded in
  size_t dw_w = 0, dw_b = 0;   // [k k][mid] in the compute type (BatchNorm folded in fp32, rounded once), fp32 [mid]
  size_t se_w1 = 0, se_b1 = 0, se_w2 = 0, se_b2 = 0;  // fp32 [sq][mid], [sq], [mid][sq], [mid]
};

struct PackedModel {
  int family = 0;
  Prec prec = Prec::F16;
  bool f16 = true;     // activations stored as fp16 (Prec::F16 only)
  bool mixed = false;  // SPI_PREC_F16M: ResNet stem in F16X3 + downsample hi + lo; transformers: hi + lo on every GEMM
  // ResNet under Prec::F16X3: conv outputs / pool inputs in the split layout
  // (GemmDesc::a_split), so the GEMM main loop never splits A on the VALU.
  bool split = false;
  int max_batch = 1;
  // AFFINE
  float aff_scale = 1.f, aff_shift = 0.f;
  // ResNet
  bool bottleneck = false;
  std::vector<int> stage_blocks;
  int groups = 1;  // of every bottleneck conv2 (ResNeXt: 32)
  ConvW stem;
  bool stem_fused = false;  // stem + max pool in one launch on the NCHW input (stem.hip)
  size_t stem_pool_w = 0;   // its weights, [hi | lo][64][24][8] fp16
  std::vector<ResBlock> blocks;
  LinearW fc;
  int image = 224, classes = 1000, feat = 512;
  // transformers
  int D = 768, heads = 12, ffn = 3072, seq = 128, layers = 0, vocab = 0, maxpos = 0;
  float eps = 1e-12f;
  // LayerNorm folded across the GEMMs (fp16, D and FFN multiples of 128; SPI_LN_FOLD=0: the
  // separate LayerNorm launches): no LN launch inside the encoder stack
  bool ln_fold = false;
  size_t word = 0, pos = 0, type0 = 0;
  // BERT outputs / inputs (spi_model_config.bert_io, SPI_BERT_* bits); 0 leaves the blob as it was.
  // SPI_BERT_TOKEN_TYPES appends the whole fp32 [type_vocab][D] table, SPI_BERT_OUT_POOLER
  // pooler.dense as plain fp32 [D][D] plus its bias.
  int bert_io = 0, type_vocab = 1;
  // SPI_BERT_POS_FROM_IDS (RoBERTa's position rule), kept out of bert_io: it selects the embedding kernel's
  // form and bounds seq by maxpos - 2, and changes no packed byte, output or workspace size
  bool pos_from_ids = false;
  size_t type_table = 0, pool_w = 0, pool_b = 0;
  // The task head (SPI_BERT_HEAD_*): classifier / qa_outputs as plain fp32 [num_labels][D] plus its bias,
  // appended after the above; SPI_BERT_HEAD_SEQUENCE also packs the pooler (once).  0 labels: no head.
  // A sequence head named classifier.dense / classifier.out_proj (HF's RobertaClassificationHead) packs
  // dense as pool_w / pool_b and out_proj as the head: the same two launches compute it.
  int num_labels = 0;
  size_t head_w = 0, head_b = 0;
  // MPNet (told by its names: encoder.relative_attention_bias.weight [nb][heads] beside attention.attn.{q,k,v,o}):
  // post-LN BERT whose every attention adds a bucketed relative-position bias.  rel_rows: the generator rows fp32
  // [heads][rel_ld] (rel_bias_pack.hpp) packed once for seq tokens, rel_half = seq - 1, appended last; rel_buckets
  // = nb, 0 for every other replica.  No token-type table (type0 is a zero row); pos_from_ids is implied.
  int rel_buckets = 0, rel_ld = 0, rel_half = 0;
  size_t rel_rows = 0;
  LnW emb_ln, final_ln;
  std::vector<TfLayer> tf;
  // ViT
  int patch = 16, npatch = 196;
  LinearW patch_proj, head;
  size_t cls = 0, vpos = 0;

  // ConvNeXt: the 4x4 / stride 4 stem as a linear layer over patchify's rows + its LayerNorm; the blocks in
  // order (stage_blocks counts them per stage, cn_dims holds the stage widths); the downsample in front of
  // stages 1..; classifier.0 (final_ln) and classifier.2 (fc; classes, feat as for ResNet)
  LinearW cn_stem;
  LnW cn_stem_ln;
  std::vector<int> cn_dims;
  std::vector<CnBlock> cn_blocks;
  std::vector<CnDown> cn_down;

  // Swin: the 4x4 / stride 4 stem as a linear layer over patchify's rows + its LayerNorm; the blocks in order
  // (stage_blocks per stage, sw_dims the stage widths); the merge in front of stages 1..; the window side;
  // `norm` (final_ln, over every pixel of the last map) and `head` (fc; classes, feat as for ResNet)
  LinearW sw_stem;
  LnW sw_stem_ln;
  std::vector<int> sw_dims;
  std::vector<SwBlock> sw_blocks;
  std::vector<SwMerge> sw_merge;
  int sw_window = 0;
  bool sw_v2 = false;  // torchvision's swin_v2_*: cosine attention, cpb_mlp bias, post-norm blocks, PatchMergingV2

  // EfficientNet: the 3x3 / stride 2 stem is `stem` (a ConvW over the ingested image, SiLU); the MBConv blocks in
  // order (stage_blocks per stage); features.8 (mb_head, 1x1 + SiLU) and classifier.1 (fc; classes, feat)
  std::vector<MbBlock> mb_blocks;
  LinearW mb_head;

  std::string desc;
  uint64_t digest = 0;  // FNV-1a 64 of the blob
  size_t blob_bytes = 0;
  std::vector<char> blob;  // starts with a zeroed 256-byte line; Model drops it after the upload
};

// Throws std::runtime_error on unrecognised names, unsupported shapes or precisions.
PackedModel pack_model(const spi_model_config& cfg, const spi_named_tensor* params, int n);

}  // namespace spi
