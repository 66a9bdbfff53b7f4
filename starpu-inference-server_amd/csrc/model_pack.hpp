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
  LnW emb_ln, final_ln;
  std::vector<TfLayer> tf;
  // ViT
  int patch = 16, npatch = 196;
  LinearW patch_proj, head;
  size_t cls = 0, vpos = 0;

  std::string desc;
  uint64_t digest = 0;  // FNV-1a 64 of the blob
  size_t blob_bytes = 0;
  std::vector<char> blob;  // starts with a zeroed 256-byte line; Model drops it after the upload
};

// Throws std::runtime_error on unrecognised names, unsupported shapes or precisions.
PackedModel pack_model(const spi_model_config& cfg, const spi_named_tensor* params, int n);

}  // namespace spi
