// Internal launch interface of the HIP/CDNA4 kernels (gfx950 only).
// Every launcher enqueues on the given stream and never synchronises, so a
// forward pass can be captured into a hipGraph (cdna_hip_programming.md G9).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include <vector>

#include "gemm_desc.hpp"
#include "image_src.hpp"

namespace spi {

// Every kernel launch goes through SPI_LAUNCH.  While a forward is profiled
// (Model::launch_table) each launch is recorded with its kernel and grid, so a
// rocprofv3 kernel trace of graph-replayed forwards -- which knows kernels and grids,
// not ops -- can be attributed to the forward's ops (tools/trace_ops.py --launches).
// Outside profiling the cost is one thread-local pointer test per launch.
struct LaunchRec {
  const char* kernel;  // __PRETTY_FUNCTION__ of kernel_id<F>: "... [F = &spi::...::name<args>]"
  unsigned gx, gy, gz, block;
};
std::vector<LaunchRec>*& launch_log();
template <auto F>
inline const char* kernel_id() {
  return __PRETTY_FUNCTION__;
}
#define SPI_LAUNCH(F, G, B, SH, S, ...)                                                                  \
  do {                                                                                                   \
    if (auto* spi_log_ = ::spi::launch_log())                                                            \
      spi_log_->push_back({::spi::kernel_id<F>(), dim3(G).x, dim3(G).y, dim3(G).z, dim3(B).x});          \
    hipLaunchKernelGGL(F, G, B, SH, S, __VA_ARGS__);                                                     \
  } while (0)

// GemmDesc, GemmPtrs and LnPtrs: gemm_desc.hpp.
// Plans, routing and workspace sizing (gemm_partial_floats / gemm_counter_slots / gemm_kstep /
// gemm_workspace_fits) are host-only: gemm_plan.hpp.
void gemm(const GemmDesc& d, const GemmPtrs& p, Prec prec, hipStream_t s);
// Two independent problems of one precision in a single launch when their plans
// share a kernel instance (else two launches); problem 1's split-K slabs and
// tickets follow problem 0's (size the workspace for both: gemm_partial_floats /
// gemm_counter_slots summed).
void gemm_pair(const GemmDesc& d0, const GemmPtrs& p0, const GemmDesc& d1, const GemmPtrs& p1, Prec prec,
               hipStream_t s);

// 8-wave phased fp16 GEMM (gemm256.hip), tiles of bm x 256 (bm = 256 or 128) for the dense
// F16 contractions; gemm() routes a desc to it when gemm256_eligible (N % 256 == 0,
// K % 64 == 0, at least min_tiles tiles of bm x 256; routing rule in gemm_plan.cpp).
void gemm256(const GemmDesc& d, const GemmPtrs& p, int splits, hipStream_t s, int bm = 256, int nbuf = 2,
             int n_fast = 0);

// Fused QKV projection + attention for S <= 128 (qkv_attn.hip): one workgroup per (sequence,
// head) runs the head's q | k | v GEMM (A rows lda apart, packed W rows ldw apart; with
// ln_stats: the LayerNorm consumer fold, ln_fold.hpp) and the attention on the LDS-resident
// result, writing ctx [B S][heads 64] fp16.  64-wide heads only: qkv_attention_eligible refuses any
// other hd and the caller runs the QKV GEMM + attention().
bool qkv_attention_eligible(int S, int heads, int hd, int K, int kpad, int krep, int lda, int ldw);
void qkv_attention(const void* A, int lda, const void* W, int ldw, const float* bias, const float* ln_stats,
                   const float* c1, int ln_chunks, float ln_eps, const float* mask_bias, void* ctx, int B, int S,
                   int heads, float scale, hipStream_t s);

// Weight-resident 3x3/s1/p1 conv, 64 -> 64 channels, fp16 NHWC (conv_wres.hip): the
// folded weights stay in LDS while a workgroup walks bands of output rows; gemm()
// routes an eligible desc to it (SPI_CONV_WRES=0: never).
bool conv_wres_eligible(const GemmDesc& d, Prec prec, const GemmPtrs& p);
void conv_wres(const GemmDesc& d, const GemmPtrs& p, hipStream_t s);
void conv_wres_reload_env();
void attention_reload_env();  // SPI_ATTN_WHOLE
void qkv_attn_reload_env();   // SPI_QKV_HP

// Grouped 3x3 / pad 1 conv, stride 1 or 2, fp16 NHWC, Cin == Cout == C (conv_group.hip): x [B][H][W][C]
// -> y [B][OH][OW][C] = act(conv + bias), fp32 accumulation.  w: gconv_packed_bytes() from
// gconv_pack_into() (gconv.hpp, which also defines the supported C / groups); bias fp32 [C] or null.
// x, w, y and bias 16-byte aligned.  Throws std::invalid_argument outside the supported set.
void conv_group(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int groups,
                int stride, bool relu, hipStream_t s);

// The kind of an image task's input buffer (SrcKind) and its 8-bit input transform (InputXf): image_src.hpp.
// The transform of one pixel of channel c.  Contraction is switched off for the two operations:
// HIP compiles with -ffp-contract=fast, under which __fmul_rn / __fadd_rn are a plain * and + that
// the backend may still fuse; without the contract flag it cannot.  The channel is picked by
// selects, so the by-value kernel argument stays in scalar registers (no indexed copy in scratch).
__device__ __forceinline__ float input_xf_apply(unsigned char p, float sc, float sh) {
#pragma clang fp contract(off)
  const float m = static_cast<float>(p) * sc;
  return m + sh;
}
__device__ __forceinline__ float input_xf_apply(unsigned char p, const InputXf& xf, int c) {
  const float sc = c == 0 ? xf.scale[0] : c == 1 ? xf.scale[1] : xf.scale[2];
  const float sh = c == 0 ? xf.shift[0] : c == 1 ? xf.shift[1] : xf.shift[2];
  return input_xf_apply(p, sc, sh);
}

// Resize + centre crop of 8-bit pixels (resample.hip; arithmetic: resample.hpp): x bytes [B][3][H][W], or
// [B][H][W][3] with nhwc, at any byte address -> y fp32 NCHW [B][3][crop][crop], the antialiased bilinear
// resample to short side resize_short, centre-cropped, under the transform xf.  1 <= H, W <= 8192,
// 1 <= crop <= resize_short <= 8192, resized long side <= 8192, B <= 65535; else throws
// std::invalid_argument before any launch.  One launch, no workspace.
void resize_crop_u8(const void* x, bool nhwc, int B, int H, int W, int resize_short, int crop, const InputXf& xf,
                    float* y, hipStream_t s);

// Image (3 channels for an 8-bit source) -> NHWC (compute type) with channels zero-padded to cpad
// (elementwise.hip).
void ingest_nchw(const void* x, void* y, int B, int C, int H, int W, int cpad,
                 bool f16, hipStream_t s, int src = kSrcF32Nchw, const InputXf& xf = InputXf{});
// Fused ResNet stem (stem.hip): NCHW fp32 image [B][3][H][W] -> 7x7/s2/p3 conv
// (64 output channels, folded BN) + ReLU -> 3x3/s2/p1 max pool -> NHWC [B][PH][PW][64]:
// fp16 (split false) or the split layout (split true, needs lo).  lo: hi + lo
// weights and image (three fp16 MFMAs per fragment, fp32-grade); else fp16 only.
// w: stem_pool_bytes() from stem_pool_pack() (pack.hpp, which also bounds the stem's output width:
// kStemPoolMaxOW); pr: 0 auto, 1 / 2 pooled rows per 4-wave workgroup.
// lo: 0 fp16 weights, 1 hi + lo weights on the fp16 image (fp16m), 2 hi + lo weights on the split
// image (fp16x3; required for the split output).  src / xf: the image's kind (above); an 8-bit image
// is [B][3][H][W] or [B][H][W][3] bytes at any byte address.
void stem_pool(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int lo,
               bool split, int pr, hipStream_t s, int src = kSrcF32Nchw, const InputXf& xf = InputXf{});
// 3x3/s2/p1 max pool on NHWC (the pools: pool.hip).  They work on whole 16-byte channel vectors:
// C % 8 == 0 (fp16), C % 4 == 0 (fp32), else they throw.
void maxpool_nhwc(const void* x, void* y, int B, int H, int W, int C, int OH,
                  int OW, int k, int stride, int pad, bool f16, hipStream_t s);
// Global average pool NHWC [B,HW,C] -> [B,C] (compute type).
void avgpool_nhwc(const void* x, void* y, int B, int HW, int C, bool f16,
                  hipStream_t s, bool out_f32 = false);  // out_f32: fp16 in, fp32 out
// The same two on F16X3 split activations (GemmDesc::a_split layout, C % 32 == 0):
// max pool split -> split, average pool split -> fp32 [B,C].
void maxpool_nhwc_split(const void* x, void* y, int B, int H, int W, int C, int OH,
                        int OW, int k, int stride, int pad, hipStream_t s);
void avgpool_nhwc_split(const void* x, float* y, int B, int HW, int C, hipStream_t s);
// Row LayerNorm over D (the LayerNorm family, the BERT embedding and mask_to_bias: layernorm.hip):
// y = LN(x) * g + b.  x fp32 [rows, ldx]; writes fp32
// (yf, may alias x) and/or compute-type (yt) outputs.
void layernorm(const float* x, int ldx, const float* g, const float* b,
               float* yf, void* yt, int ldy, int rows, int D, float eps, bool f16,
               hipStream_t s);
// BERT embeddings: LN(word[ids] + pos[s] + type[0]) -> fp32 + compute type; with a mask, each
// token's additive attention bias too (mask_to_bias's, one launch fewer per forward).  yf is
// required (throws on null); yt may be null.  With types (int64 [B,S] segment ids), type0 is the
// whole [type_vocab][D] table and row (b, s) adds its row clamp(types[b][s], 0, type_vocab - 1);
// null types add row 0, the same sums in the same order.  pos_from_ids (SPI_BERT_POS_FROM_IDS): the position
// row is 1 + the non-pad ids of ids[b][0..s], or 1 for a pad id, instead of s; the table needs S + 2 rows.
void bert_embed(const int64_t* ids, const float* word, const float* pos,
                const float* type0, const float* g, const float* b, float* yf,
                void* yt, int B, int S, int D, int vocab, float eps, bool f16,
                hipStream_t s, const int64_t* mask = nullptr, float* mask_bias = nullptr,
                const int64_t* types = nullptr, int type_vocab = 1, bool pos_from_ids = false);
// BERT sentence outputs (bert_pool.hip): fp32, fixed summation order, D % 64 == 0 and D <= 1024.
// Pooler: y[b][n] = tanh(bias[n] + sum_k h[b ld + k] W[n][k]); W fp32 [D][D], y [B][D].
void bert_pooler(const float* h, size_t ld, const float* W, const float* bias, float* y, int B, int D,
                 hipStream_t s);
// The pooler's kernel as a dense layer over N columns: y[b][n] = act(bias[n] + sum_k h[b ld + k] W[n][k]),
// W fp32 [N][D], y [B][N], act = tanh or none; 1 <= N <= 1024.  N = D with tanh is bert_pooler, bit for bit.
void bert_dense_rows(const float* h, size_t ld, const float* W, const float* bias, float* y, int B, int D, int N,
                     bool tanh_act, hipStream_t s);
// Token-level task head (bert_head.hip): y[t][l] = bias[l] + sum_c h[t][c] W[l][c], t < T, l < L <= 64, fp32,
// fixed summation order, a row's result independent of T and of the row's place.  h[t] by source kind:
// normalised fp32 rows; pre-LayerNorm fp32 rows, normalised in registers with g / b / eps and never stored;
// or pre-LayerNorm rows in two fp16 planes (hi at x, lo `plane` elements on), likewise.  Rows are D apart;
// D % 64 == 0, D <= 1024.  y1 null: y0 is [T][L]; else L == 2 and label 0 goes to y0 [T], label 1 to y1 [T].
enum HeadSrc { kHeadSrcRows = 0, kHeadSrcPreLn = 1, kHeadSrcPlanes = 2 };
void bert_token_head(int src, const void* x, size_t plane, const float* g, const float* b, float eps, const float* W,
                     const float* bias, float* y0, float* y1, int T, int D, int L, hipStream_t s);
// Masked mean: y[b] = sum_s m[b][s] h[b][s] / max(sum_s m[b][s], 1e-9), m = (mask != 0); a null mask
// counts every token.  h [B][S][D], y [B][D].
void masked_mean(const float* h, const int64_t* mask, float* y, int B, int S, int D, hipStream_t s);
// Classification outputs (classify.hip): softmax and / or top-k of B fp32 logits rows of N, ldx floats
// apart, in one launch.  probs fp32 [B][N] or null: exp(x - max) / sum, fixed summation order.  topv fp32
// [B][k] and topi int64 [B][k], both or neither: the row's k best by logit descending, equal logits
// (0.0 == -0.0) by index ascending; topv holds the logits' own bits, or with topk_probs the bits probs
// holds (or would hold) there.  1 <= N <= kSoftmaxTopkMaxN, 1 <= k <= min(N, kSoftmaxTopkMaxK) (0 without
// top-k).  -inf logits give probability 0; +inf / NaN logits give unspecified results.  Throws
// std::invalid_argument before any launch.
void softmax_topk(const float* x, size_t ldx, float* probs, float* topv, int64_t* topi, int B, int N, int k,
                  bool topk_probs, hipStream_t s);
// int64 attention mask [B,S] -> additive fp32 bias [B,S] (0 or finfo.min).
void mask_to_bias(const int64_t* mask, float* bias, int n, hipStream_t s);
// ViT (patchify, the two assemblies, gather_rows and affine: elementwise.hip): image (NCHW fp32, or
// 8-bit pixels of kind src, C = 3) -> patch rows [B*P, C*ps*ps] (compute type).
void patchify(const void* x, void* y, int B, int C, int H, int W, int ps,
              bool f16, hipStream_t s, int src = kSrcF32Nchw, const InputXf& xf = InputXf{});
// ViT: x[b, 0] = cls + pos[0]; x[b, 1+p] = patch[b, p] + pos[1+p]  (fp32).
void vit_assemble(const float* patches, const float* cls, const float* pos,
                  float* x, int B, int P, int D, hipStream_t s);
// The same into the two-plane residual stream (GemmDesc::res_planes: hi at xh, lo plane elements
// on) plus, when stats is not null, each row's per-64-column chunk statistics [rows][D / 64][2]
// (ln_fold.hpp).
void vit_assemble_planes(const float* patches, const float* cls, const float* pos, _Float16* xh, size_t plane,
                         float* stats, int B, int P, int D, hipStream_t s);
// layernorm() over rows held in two fp16 planes (x = hi + lo), D <= 1024 (layernorm.hip).
void layernorm_planes(const _Float16* xh, size_t plane, int ldx, const float* g, const float* b, float* yf, void* yt,
                      int ldy, int rows, int D, float eps, bool f16, hipStream_t s);
// Gather rows: y[i] = x[i * stride_rows] (fp32 -> compute type) for CLS pooling.
void gather_rows(const float* x, void* y, int rows, int stride_rows, int D,
                 bool f16, hipStream_t s);
// y = x * scale + shift, fp32 elementwise (AFFINE toy family).
void affine(const float* x, float* y, size_t n, float scale, float shift,
            hipStream_t s);

// Multi-head attention over a packed qkv buffer [B*S, 3*D] (compute type):
// ctx[b*S+i, h*hd:(h+1)*hd] = softmax(q k^T * scale + mask_bias[b]) v.  hd 32 or 64; any other
// width throws std::invalid_argument.
// mask_bias: fp32 [B, S] additive bias or nullptr.
void attention(const void* qkv, const float* mask_bias, void* ctx, int B, int S,
               int heads, int hd, float scale, bool f16, hipStream_t s);

}  // namespace spi
