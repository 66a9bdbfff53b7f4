/*
 * spi_ops.h — op-level C entry points of the MI355X kernels.
 *
 * Not part of the codelet boundary (that is spi_codelet.h): these expose the
 * individual HIP kernels the forward passes are built from, for kernel-level
 * parity tests against a plain fp32 reference and for micro-benchmarks.  All
 * pointers are device pointers unless marked host; every call only enqueues
 * on `stream`.  Return 0 on success, non-zero on invalid arguments / HIP error
 * (message in spi_last_error()).
 *
 * precision: 0 fp32, 1 fp16, 2 fp16x3 (fp32 activations split into hi/lo fp16
 * at fragment read), 3 fp16x3 on SPLIT activations: every activation operand
 * (A, residual, C) uses the split layout the fp16x3 ResNet forward keeps in
 * HBM -- per row, blocks of 32 elements stored as [32 hi fp16 | 32 lo fp16]
 * (128 bytes, the size of 32 fp32), hi = fp16(x), lo = fp16(x - hi).  It needs
 * K (GEMM) / Cin (conv) and N / Cout to be multiples of 32 and <= 31 filter taps.
 */
#ifndef SPI_OPS_H
#define SPI_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Packed weight layout for a [N][K] fp32 matrix: rows padded to Npad = 128k,
 * columns to Kpad = 64k; fp16 / fp32 elements, or for fp16x3 (2 and 3) per
 * 32-k block [32 hi fp16 | 32 lo fp16].  Returns the packed byte count; writes Npad/Kpad.
 * One exception to "zero padded": an fp16 [64][576] matrix (a 3x3 conv over 64 channels)
 * carries, in its padding rows 64..127, the weight-resident conv's LDS image of rows 0..63
 * (per tap t, row n, 16-byte slot s: chunk s ^ (n & 7) of row n's taps-t block), and
 * spi_op_conv2d routes such convs to that kernel, which reads those rows.  Packed weights
 * for spi_op_conv2d / spi_op_gemm must therefore come from spi_op_pack_weight, whole. */
size_t spi_op_packed_bytes(int32_t precision, int32_t N, int32_t K, int32_t* Npad, int32_t* Kpad);
/* Host-side packing: w_host fp32 [N][K] -> dst_host (spi_op_packed_bytes bytes). */
int spi_op_pack_weight(int32_t precision, const float* w_host, int32_t N, int32_t K, void* dst_host);

/* Bytes of device scratch a GEMM / conv call needs (zero line, split-K slabs
 * and tickets).  The scratch must be zero-filled once before first use. */
size_t spi_op_workspace_bytes(void);

/* C[M,N] = act(A[M,K] . W^T + bias + residual); act: 0 none, 1 relu, 2 gelu.
 * A: fp16 (precision fp16), fp32 (fp32 / fp16x3) or split (3), row stride lda
 * (elements).  residual: same element type as A unless res_f32; C: fp32 when
 * out_f32 (not with split). */
int spi_op_gemm(int32_t precision, const void* A, int32_t M, int32_t K, int32_t lda,
                const void* W_packed, int32_t N, const float* bias, const void* residual,
                int32_t res_f32, int32_t ldr, void* C, int32_t out_f32, int32_t ldc,
                int32_t act, void* workspace, void* stream);

/* NHWC conv as implicit GEMM: x [B][H][W][Cin] (Cin a power of two >= 8 for fp16,
 * >= 4 for fp32 / fp16x3, >= 32 for split), W packed from [Cout][KH][KW][Cin]
 * order, y [B][OH][OW][Cout]; residual (optional) shaped like y. */
int spi_op_conv2d(int32_t precision, const void* x, int32_t B, int32_t H, int32_t W,
                  int32_t Cin, const void* W_packed, int32_t Cout, int32_t KH, int32_t KW,
                  int32_t stride, int32_t pad, const float* bias, const void* residual,
                  void* y, int32_t act, void* workspace, void* stream);

/* ---- hi + lo fp16 weights (the fp16m layers: GemmDesc::krep = 2) ----
 * A [N][K] fp32 matrix packed for fp16 activations at ~22 weight bits: rows padded to Npad = 128k, and per
 * 64 logical k one 128-element packed block [64 hi | 64 lo], hi = fp16(w), lo = fp16(w - hi), so
 * Kpad = 2 round_up(K, 64).  The kernel stages each A k-step twice, against the hi and the lo block, and
 * accumulates both in fp32.  Padding (k >= K, rows N..Npad) is zero: this layout never carries the
 * weight-resident conv's image rows, and spi_op_conv2d_hilo never routes to that kernel. */
size_t spi_op_packed_bytes_hilo(int32_t N, int32_t K, int32_t* Npad, int32_t* Kpad);
int spi_op_pack_weight_hilo(const float* w_host, int32_t N, int32_t K, void* dst_host);

/* spi_op_gemm at precision fp16 on hi + lo weights (W_packed from spi_op_pack_weight_hilo): A fp16,
 * residual fp16 unless res_f32, C fp16 unless out_f32.  Always the general kernel (gemm.hip). */
int spi_op_gemm_hilo(const void* A, int32_t M, int32_t K, int32_t lda, const void* W_packed, int32_t N,
                     const float* bias, const void* residual, int32_t res_f32, int32_t ldr, void* C,
                     int32_t out_f32, int32_t ldc, int32_t act, void* workspace, void* stream);

/* spi_op_conv2d at precision fp16 on hi + lo weights: x fp16, Cin a power of two >= 64 (one filter tap
 * per k-step), KH KW <= 31; residual fp16 unless res_f32, y fp16 unless out_f32. */
int spi_op_conv2d_hilo(const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* W_packed,
                       int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, const float* bias,
                       const void* residual, int32_t res_f32, void* y, int32_t out_f32, int32_t act,
                       void* workspace, void* stream);

/* One conv of spi_op_conv_pair. */
typedef struct spi_op_conv_spec {
  const void* W_packed; /* spi_op_pack_weight at the call's precision, or spi_op_pack_weight_hilo when hilo */
  int32_t Cout, KH, KW, stride, pad;
  const float* bias;    /* fp32 [Cout] or null */
  int32_t act;          /* 0 none, 1 relu, 2 gelu */
  int32_t hilo;         /* hi + lo weights (precision fp16 only; Cin >= 64, KH KW <= 31) */
  int32_t out_f32;      /* y is fp32 (not with the split layout) */
  void* y;              /* [B][OH][OW][Cout] */
} spi_op_conv_spec;

/* Two convs on one input x [B][H][W][Cin] -- a ResNet block's first conv and its downsample conv -- as the
 * model runs them: one grouped launch when their plans share a kernel instance (a joint split-K plan,
 * conv 1's slabs and tickets behind conv 0's in the workspace), else one launch each.  No residual.
 * precision, x and Cin as spi_op_conv2d.  plan_out (host, nullable) receives 22 integers in
 * spi_debug_conv_pair_plan's order -- the two 8-field plans that launch, grouped, workgroups of both,
 * conv 1's slab and ticket offsets, the summed workspace floats and ticket slots -- for the descriptors
 * this call runs (hilo included, which the debug export cannot express). */
int spi_op_conv_pair(int32_t precision, const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                     const spi_op_conv_spec* c0, const spi_op_conv_spec* c1, void* workspace, void* stream,
                     int64_t* plan_out);

/* ---- Grouped 3x3 conv (conv_group.hip; a ResNeXt bottleneck's conv2), fp16 ----
 * x [B][H][W][C] fp16 NHWC -> y [B][OH][OW][C] fp16 = act(conv(x) + bias), OH = (H - 1) / stride + 1 (OW
 * alike): Cin == Cout == C in `groups` groups of cpg = C / groups channels, group g reading and writing
 * channels [g cpg, (g + 1) cpg); 3x3, pad 1 (padding taps contribute zero), stride 1 or 2; bias fp32 [C] or
 * null; act 0 none, 1 relu; fp32 accumulation; no residual, no workspace.
 * Supported: C a multiple of 128, groups >= 2, cpg 4, 8, 16, 32 or 64.
 *
 * Packed layout (spi_op_gconv_pack_weight of the torch-order weight [C][cpg][3][3]): fp16
 * [C / 16][steps][64][8].  A wave owns 16 output channels n0 .. n0 + 15 and contracts them in `steps`
 * mfma_f32_16x16x32_f16 with the weights as the A operand; entry [tile][s][l][j] is the weight of output
 * channel 16 tile + (l & 15) at k-element 8 (l >> 4) + j of step s, q = l >> 4:
 *   cpg <= 16 (5 steps): tap 2 s + (q >> 1), input channel n0 + 8 (q & 1) + j -- two taps of the tile's own
 *     16 channels; an input channel of another group than the row's is stored as zero, and so is tap 9;
 *   cpg 32 (9 steps): tap s, input channel 32 (n0 / 32) + 8 q + j;
 *   cpg 64 (18 steps): tap s >> 1, input channel 64 (n0 / 64) + 32 (s & 1) + 8 q + j;
 * tap = kh 3 + kw.
 *
 * A consequence of the zero-packed off-group weights (cpg 4 and 8; cpg 16 shares nothing): groups of one
 * 16-channel slice share MFMAs, so a non-finite activation (inf, NaN) in one group reaches the other
 * groups of that slice as 0 inf = NaN, where PyTorch keeps it inside its group.  Finite values never leak:
 * their products with the zeros are exact zeros, and the other groups' outputs keep their bits.
 *
 * Rejected before any launch, with a message in spi_last_error(): C not a multiple of 128; cpg outside the
 * five values or groups < 2; a kernel other than 3x3 with pad 1; a stride other than 1 or 2; null x,
 * W_packed or y; B, H or W <= 0; x, y, W_packed (or a non-null bias) off 16-byte alignment; act other
 * than 0 / 1.  spi_op_gconv_packed_bytes returns 0 for an unsupported shape. */
size_t spi_op_gconv_packed_bytes(int32_t C, int32_t groups, int32_t KH, int32_t KW);
int spi_op_gconv_pack_weight(const float* w_host /* [C][C/groups][KH][KW], torch order */, int32_t C,
                             int32_t groups, int32_t KH, int32_t KW, void* dst_host);
int spi_op_conv2d_grouped(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, const void* W_packed,
                          int32_t groups, int32_t KH, int32_t KW, int32_t stride, int32_t pad, const float* bias,
                          void* y, int32_t act, void* stream);

/* Fused global average pool + linear layer (ResNet avgpool + fc in one launch):
 * x [B][HW][C] (fp32 / fp16 / split by precision, HW <= 64), W packed from the
 * [N][C] fc weight; y fp32 [B][N] = act(mean_hw(x) . W^T + bias). */
int spi_op_avgpool_fc(int32_t precision, const void* x, int32_t B, int32_t HW, int32_t C, const void* W_packed,
                      int32_t N, const float* bias, float* y, int32_t act, void* workspace, void* stream);

/* Fused ResNet stem: x NCHW fp32 [B][3][H][W] -> 7x7/s2/p3 conv (64 channels,
 * BN folded into w / bias) + ReLU -> 3x3/s2/p1 max pool -> y NHWC [B][PH][PW][64].
 * precision 1: fp16 image and weights, fp16 y; 2: the fp16m stem -- fp16 image x hi + lo fp16
 * weights, fp16 y; 3: hi + lo image x hi + lo weights (fp32-grade), y in the split layout (the
 * fp16x3 stem); 4: as 3 with fp16 y.  W_packed: spi_op_stem_pool_bytes()
 * of device memory filled from spi_op_stem_pool_pack(w_host fp32 [64][3][7][7]).
 * rows_per_block: 0 = default (2 pooled rows per 8-wave workgroup for maps wider than 64,
 * else 1 per 4 waves), 1 or 2 = that many per 4-wave workgroup.  W <= 224. */
size_t spi_op_stem_pool_bytes(void);
int spi_op_stem_pool_pack(const float* w_host, void* dst_host);
int spi_op_stem_pool(int32_t precision, const float* x, int32_t B, int32_t H, int32_t W,
                     const void* W_packed, const float* bias, void* y, int32_t rows_per_block, void* stream);

/* The same stem on 8-bit pixels: x is [B][3][H][W] (nhwc 0) or [B][H][W][3] (nhwc 1) bytes at
 * any byte address; pixel p of channel c enters as fl(fl((float)p * scale[c]) + shift[c]) (two
 * fp32 roundings, no FMA; spi_codelet.h: spi_model_set_input_transform) and from there is
 * treated exactly as an fp32 image holding those values: same precision codes, same y.
 * scale / shift: host fp32 [3]; both null = scale 1, shift 0. */
int spi_op_stem_pool_u8(int32_t precision, const uint8_t* x, int32_t nhwc, int32_t B, int32_t H, int32_t W,
                        const void* W_packed, const float* bias, const float* scale_host, const float* shift_host,
                        void* y, int32_t rows_per_block, void* stream);

/* ViT patchify of a 3-channel image: y [B (H/ps) (W/ps)][3 ps ps] (fp16 when out_f16, else fp32),
 * row (b, ph, pw), column c ps ps + kh ps + kw (the conv weight's flatten order).  src_kind: 0 x is
 * fp32 [B][3][H][W]; 1 bytes [B][3][H][W]; 2 bytes [B][H][W][3], both under the transform above
 * (scale / shift ignored for src_kind 0).  H and W multiples of ps. */
int spi_op_patchify(int32_t src_kind, const void* x, int32_t B, int32_t H, int32_t W, int32_t ps,
                    const float* scale_host, const float* shift_host, void* y, int32_t out_f16, void* stream);

/* Resize + centre crop of 8-bit pixels (resample.hip; the contract and the arithmetic: spi_codelet.h,
 * spi_model_set_input_resize): x bytes [B][3][H][W] (nhwc 0) or [B][H][W][3] (nhwc 1) at any byte address ->
 * y fp32 NCHW [B][3][crop][crop]: the antialiased bilinear resample to short side resize_short, centre crop,
 * then fl(fl(v scale[c]) + shift[c]).  scale / shift: host fp32 [3]; both null = scale 1, shift 0.
 * 1 <= H, W <= 8192, 1 <= crop <= resize_short <= 8192, resized long side <= 8192, B <= 65535; rejected
 * before any launch otherwise.  One launch, no workspace, no atomics. */
int spi_op_resize_crop_u8(const uint8_t* x, int32_t nhwc, int32_t B, int32_t H, int32_t W, int32_t resize_short,
                          int32_t crop, const float* scale_host, const float* shift_host, float* y, void* stream);
/* The same arguments on host pointers (stream ignored): the same arithmetic (csrc/resample.hpp, shared with
 * the kernel) run on the CPU, the reference the device op is compared with. */
int spi_op_resize_crop_u8_host(const uint8_t* x, int32_t nhwc, int32_t B, int32_t H, int32_t W, int32_t resize_short,
                               int32_t crop, const float* scale_host, const float* shift_host, float* y, void* stream);

/* Multi-head attention over packed qkv [B*S][3*D] (fp16 or fp32), D = heads * 64: ctx [B*S][D] =
 * softmax(q k^T scale + mask_bias) v per (batch, head); mask_bias fp32 [B][S] added to every query's
 * scores, or null.  Rejected before any launch: a precision other than 0 (fp32) or 1 (fp16), a null
 * qkv or ctx, B, S or heads <= 0, B * heads > 65535 (the grid's y extent), qkv off 16-byte alignment
 * (q / k / v rows are read in 16-byte chunks), ctx off 8-byte alignment (the fp16 kernels' stores). */
int spi_op_attention(int32_t precision, const void* qkv, const float* mask_bias, void* ctx,
                     int32_t B, int32_t S, int32_t heads, float scale, void* stream);
/* The same with the head width stated: D = heads * head_dim, head_dim 32 or 64 (any other value is
 * rejected before any launch, like the above).  spi_op_attention is this with head_dim 64. */
int spi_op_attention_hd(int32_t precision, const void* qkv, const float* mask_bias, void* ctx, int32_t B,
                        int32_t S, int32_t heads, int32_t head_dim, float scale, void* stream);

/* Row LayerNorm: x fp32 [rows][D] -> yf fp32 and/or yt (fp16 when precision fp16). */
int spi_op_layernorm(int32_t precision, const float* x, const float* gamma, const float* beta,
                     float* yf, void* yt, int32_t rows, int32_t D, float eps, void* stream);

/* ---- LayerNorm folded across GEMMs (transformer fp16 path) ----
 * Row statistics travel as per-64-column-chunk partials, fp32 [rows][D / 64][2] of (mean, M2 = sum of
 * squared deviations from the chunk's mean), combined by Chan's formula where they are read.  A two-plane
 * tensor is a row-major [rows][ld] fp32-grade tensor kept as hi = fp16(x) at the pointer and
 * lo = fp16(x - hi) `plane` elements (a multiple of 8) further on. */

/* Host arithmetic of the fold for y = LN(x) W^T + b: w_folded [N][K] = W diag(gamma) (fp32),
 * bias_out [N] = b + W beta, c1_out [N] = sum_k of w_folded as packed -- rounded to fp16 for precision
 * fp16 (hi + lo when hilo), else the fp32 values.  b may be null.  All host fp32 arrays; pack w_folded
 * with spi_op_pack_weight (spi_op_pack_weight_hilo when hilo). */
int spi_op_fold_linear(int32_t precision, const float* w_host, const float* b_host, int32_t N, int32_t K,
                       const float* gamma_host, const float* beta_host, int32_t hilo, float* w_folded_out,
                       float* bias_out, float* c1_out);

/* Element kinds of spi_op_gemm_ln's residual and output. */
#define SPI_KIND_NONE 0   /* (residual only) no residual */
#define SPI_KIND_F16 1
#define SPI_KIND_F32 2
#define SPI_KIND_PLANES 3 /* two fp16 planes, `plane` elements apart */

/* The dense fp16 GEMM C = act(A . W^T + bias + residual) with every fold field settable (N % 128 == 0;
 * bias, C, residual, c1, res_g, res_b, c16 16-byte aligned; ldc, ldr, ld16 multiples of 8):
 *   consumer (in_stats and c1 non-null; K % 64 == 0): A holds the fp16 rows x before a LayerNorm, in_stats
 *     their statistics [M][K / 64][2], W / bias / c1 come from spi_op_fold_linear, and the epilogue
 *     computes rstd (acc - mean c1) + bias;
 *   residual: res_kind says how it is stored; a two-plane output takes an fp16-typed residual as planes;
 *   residual LayerNorm (res_stats, res_g, res_b non-null; fp32 or two-plane residual): the residual added
 *     is LN(R) g + b, from R's statistics [M][N / 64][2];
 *   producer (out_stats non-null): writes the output rows' statistics [M][N / 64][2] and, when c16 is not
 *     null, an fp16 copy of the output (row stride ld16); c16 may be null only for a two-plane output.
 * eps serves both LayerNorms.  residual == C (in place) is allowed. */
int spi_op_gemm_ln(const void* A, int32_t M, int32_t K, int32_t lda, const void* W_packed, int32_t N,
                   const float* bias, const float* in_stats, const float* c1, const void* residual,
                   int32_t res_kind, int32_t ldr, const float* res_stats, const float* res_g, const float* res_b,
                   float eps, void* C, int32_t out_kind, int32_t ldc, size_t plane, float* out_stats, void* c16,
                   int32_t ld16, int32_t act, void* workspace, void* stream);

/* spi_op_gemm_ln on hi + lo weights (the fp16m transformers' GEMMs): W_packed from spi_op_pack_weight_hilo
 * of spi_op_fold_linear(hilo = 1)'s w_folded, c1 from the same call.  Same parameters, same rules; always
 * the general kernel. */
int spi_op_gemm_ln_hilo(const void* A, int32_t M, int32_t K, int32_t lda, const void* W_packed, int32_t N,
                        const float* bias, const float* in_stats, const float* c1, const void* residual,
                        int32_t res_kind, int32_t ldr, const float* res_stats, const float* res_g,
                        const float* res_b, float eps, void* C, int32_t out_kind, int32_t ldc, size_t plane,
                        float* out_stats, void* c16, int32_t ld16, int32_t act, void* workspace, void* stream);

/* Row LayerNorm over rows held in two fp16 planes (x = hi + lo), D <= 1024, input row stride ldx:
 * yf fp32 and/or yt (fp16 when precision fp16, else fp32), row stride ldy. */
int spi_op_layernorm_planes(int32_t precision, const void* xh, size_t plane, int32_t ldx, const float* gamma,
                            const float* beta, float* yf, void* yt, int32_t ldy, int32_t rows, int32_t D,
                            float eps, void* stream);

/* ViT stream assembly into two planes: row (b, 0) = cls + pos[0], row (b, 1 + p) = patches[b][p] + pos[1 + p]
 * (all fp32, D % 64 == 0), plus the rows' chunk statistics [B (P + 1)][D / 64][2] when stats is not null. */
int spi_op_vit_assemble_planes(const float* patches, const float* cls, const float* pos, void* xh, size_t plane,
                               float* stats, int32_t B, int32_t P, int32_t D, void* stream);

/* ---- Fused QKV projection + attention (qkv_attn.hip) ----
 * ctx [B S][D] fp16 = attention over q | k | v = A . W^T + bias, D = 64 heads: 64-wide heads only (32-wide
 * heads run the QKV GEMM + spi_op_attention_hd, which measured faster).  A: fp16 [B S][lda];
 * W_packed: spi_op_pack_weight(fp16, [3 D][D]) (rows q, k, v; row stride the packed Kpad = D); bias fp32
 * [3 D], required.  in_stats / c1 (both or neither): the LayerNorm fold's consumer -- A holds the rows
 * before the LayerNorm, in_stats their chunk statistics [B S][D / 64][2], W / bias / c1 come from
 * spi_op_fold_linear; needs D <= 1024.  mask_bias: fp32 [B S] additive key bias, or null.
 * 1 <= S <= 256, heads >= 2, lda >= D and a multiple of 8, A and W_packed 16-byte aligned, ctx and
 * in_stats 8-byte aligned.  Always the fused kernel (SPI_QKV_ATTN is the model's switch); SPI_QKV_HP
 * applies as in the model. */
int spi_op_qkv_attention(const void* A, int32_t lda, const void* W_packed, int32_t heads, const float* bias,
                         const float* in_stats, const float* c1, float eps, const float* mask_bias, void* ctx,
                         int32_t B, int32_t S, float scale, void* stream);

/* ---- The HBM-bound kernels around the contractions (elementwise.hip, pool.hip, layernorm.hip) ---- */

/* Image -> NHWC with the channels zero-padded to cpad: y [B][H][W][cpad] (fp16 when out_f16, else fp32).
 * src_kind, scale_host, shift_host as in spi_op_patchify; x is [B][C][H][W] fp32 (src_kind 0) or 8-bit
 * pixels with C = 3 at any byte address.  1 <= C <= cpad. */
int spi_op_ingest(int32_t src_kind, const void* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t cpad,
                  const float* scale_host, const float* shift_host, void* y, int32_t out_f16, void* stream);

/* k x k max pool, NHWC: x [B][H][W][C] -> y [B][OH][OW][C], OH = (H + 2 pad - k) / stride + 1 (OW alike),
 * padding never wins.  precision 0 fp32, 1 fp16, 3 split -> split; 0 <= pad < k; C a multiple of the
 * 16-byte vector: 4 (fp32), 8 (fp16), 32 (split). */
int spi_op_maxpool(int32_t precision, const void* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                   int32_t stride, int32_t pad, void* y, void* stream);

/* Global average pool x [B][HW][C] -> y [B][C]; precisions and C as spi_op_maxpool.  y is fp32 for
 * precision 0 and 3 (the split form always writes fp32); for fp16, fp16 or -- with out_f32 -- fp32. */
int spi_op_avgpool(int32_t precision, const void* x, int32_t B, int32_t HW, int32_t C, void* y, int32_t out_f32,
                   void* stream);

/* BERT embeddings: row (b, s) = LN(word[clamp(ids[b][s], 0, vocab - 1)] + type0 + pos[s]) gamma + beta ->
 * yf fp32 [B S][D] (required) and, when yt is not null, yt (fp16 for precision 1, fp32 for 0).  ids int64
 * [B S]; word [vocab][D], pos [npos][D], type0 / gamma / beta [D] fp32.  mask (int64 [B S]) and mask_bias
 * (fp32 [B S], written 0 where mask != 0, else the lowest finite fp32) come both or neither.  D <= 1024,
 * S <= npos. */
int spi_op_bert_embed(int32_t precision, const int64_t* ids, const float* word, const float* pos,
                      const float* type0, const float* gamma, const float* beta, float* yf, void* yt, int32_t B,
                      int32_t S, int32_t D, int32_t vocab, int32_t npos, float eps, const int64_t* mask,
                      float* mask_bias, void* stream);

/* spi_op_bert_embed with segment ids: `type0` becomes type_table [type_vocab][D] and row (b, s) adds
 * type_table[clamp(type_ids[b][s], 0, type_vocab - 1)].  type_ids int64 [B S], or null for row 0 --
 * then, and with all-zero ids, the output has the bits of spi_op_bert_embed on type_table's first row. */
int spi_op_bert_embed_types(int32_t precision, const int64_t* ids, const float* word, const float* pos,
                            const float* type_table, int32_t type_vocab, const int64_t* type_ids,
                            const float* gamma, const float* beta, float* yf, void* yt, int32_t B, int32_t S,
                            int32_t D, int32_t vocab, int32_t npos, float eps, const int64_t* mask,
                            float* mask_bias, void* stream);

/* spi_op_bert_embed_types with RoBERTa's position rule (SPI_BERT_POS_FROM_IDS, spi_codelet.h): row (b, s)
 * reads pos[1 + #{j <= s : ids[b][j] != 1}], or pos[1] where ids[b][s] == 1 (SPI_ROBERTA_PAD_ID), instead
 * of pos[s].  The count is over the raw ids and exact.  The same checks, and S + 2 <= npos.  On pad-free
 * ids the outputs have the bits of spi_op_bert_embed_types given pos + 2 D. */
int spi_op_bert_embed_posids(int32_t precision, const int64_t* ids, const float* word, const float* pos,
                             const float* type_table, int32_t type_vocab, const int64_t* type_ids,
                             const float* gamma, const float* beta, float* yf, void* yt, int32_t B, int32_t S,
                             int32_t D, int32_t vocab, int32_t npos, float eps, const int64_t* mask,
                             float* mask_bias, void* stream);

/* ---- BERT sentence outputs (bert_pool.hip); fp32 throughout, deterministic (no atomics) ---- */

/* BERT pooler: y[b][n] = tanh(bias[n] + sum_k h[b ld + k] W[n][k]), b < B, n < D.  h: fp32 rows of D, ld
 * floats between consecutive b (ld >= D: D for packed rows, S D for the class-token rows of a [B][S][D]
 * hidden state); W fp32 [D][D] row-major (pooler.dense.weight), bias fp32 [D]; y fp32 [B][D].
 * B >= 1, D a multiple of 64 and <= 1024. */
int spi_op_bert_pooler(const float* h, int64_t ld, const float* W, const float* bias, float* y, int32_t B,
                       int32_t D, void* stream);

/* Masked mean over the sequence: y[b][:] = sum_s m[b][s] h[b][s][:] / max(sum_s m[b][s], 1e-9),
 * m = (mask[b][s] != 0); mask int64 [B][S], or null = every token counts.  h fp32 [B][S][D], y fp32 [B][D].
 * B >= 1, S >= 1, D a multiple of 64 and <= 1024. */
int spi_op_masked_mean(const float* h, const int64_t* mask, float* y, int32_t B, int32_t S, int32_t D,
                       void* stream);

/* ---- BERT task heads (bert_head.hip, bert_pool.hip); fp32 throughout, deterministic (no atomics) ---- */

/* Token-level head: y[t][l] = bias[l] + sum_c h[t][c] W[l][c], t < T, l < L.  h[t] by `src`:
 *   0  x: fp32 rows [T][D], already normalised;
 *   1  x: fp32 pre-LayerNorm rows [T][D]; the kernel normalises each row in registers with gamma / beta
 *      [D] and eps and never stores it;
 *   2  x: pre-LayerNorm rows as two fp16 planes, hi [T][D] at x and lo `plane` elements (>= T D) after
 *      it, the row being hi + lo; normalised as under 1.
 * gamma, beta, eps and plane are ignored where the source does not use them (may be null / 0).
 * W fp32 [L][D] row-major, bias fp32 [L].  y1 null: y0 is fp32 [T][L]; else L must be 2 and label 0 goes
 * to y0 [T], label 1 to y1 [T] (QA start / end logits).  T >= 1, D a multiple of 64 and <= 1024,
 * 1 <= L <= 64.  A row's result does not depend on T or on the row's place.  A pointer that is not
 * 16-byte aligned (8 for the fp16 planes) takes scalar loads. */
int spi_op_bert_token_head(int32_t src, const void* x, int64_t plane, const float* gamma, const float* beta, float eps,
                           const float* W, const float* bias, float* y0, float* y1, int32_t T, int32_t D, int32_t L,
                           void* stream);

/* The pooler's kernel as a dense layer: y[b][n] = act(bias[n] + sum_k h[b ld + k] W[n][k]), b < B, n < N;
 * h as for spi_op_bert_pooler, W fp32 [N][D], bias fp32 [N], y fp32 [B][N]; activation 0 = none, 1 = tanh.
 * B >= 1, D a multiple of 64 and <= 1024, 1 <= N <= 1024.  N = D with tanh gives spi_op_bert_pooler's bits;
 * without an activation it is the sequence-classification head on pooler_output. */
int spi_op_bert_dense_rows(const float* h, int64_t ld, const float* W, const float* bias, float* y, int32_t B,
                           int32_t D, int32_t N, int32_t activation, void* stream);

/* bias[i] = mask[i] != 0 ? 0 : the lowest finite fp32, i < n. */
int spi_op_mask_to_bias(const int64_t* mask, float* bias, int32_t n, void* stream);

/* ViT stream assembly, fp32: x [B][P + 1][D], row (b, 0) = cls + pos[0], row (b, 1 + p) = patches[b][p] + pos[1 + p]. */
int spi_op_vit_assemble(const float* patches, const float* cls, const float* pos, float* x, int32_t B, int32_t P,
                        int32_t D, void* stream);

/* ---- Classification outputs (classify.hip); fp32, deterministic (no atomics), one launch ---- */

/* Softmax and / or top-k of fp32 logits rows.
 * x fp32 [B] rows of N, ldx floats apart (ldx >= N). probs fp32 [B][N] or null; topv fp32 [B][k] and
 * topi int64 [B][k] both or neither; topk_probs: topv holds probabilities. 1 <= N <= 16384, 1 <= k <= min(N, 64).
 * probs[b][j] = exp(x[b][j] - max_j x[b]) / sum_j exp(x[b][j] - max_j x[b]).  Top-k: the row's k best by
 * logit descending, equal logits (0.0 == -0.0) by index ascending, as torch.sort(descending=True,
 * stable=True); topv carries the logits' own bits, or with topk_probs the bits probs holds (or would
 * hold) at those indices.  Without topv / topi, k and topk_probs must be 0.  -inf logits give probability
 * 0; +inf or NaN logits give unspecified results.  Everything is validated before any launch. */
int spi_op_softmax_topk(const float* x, int64_t ldx, float* probs, float* topv, int64_t* topi,
                        int32_t B, int32_t N, int32_t k, int32_t topk_probs, void* stream);

/* y[i] = x[i stride_rows] for i < rows: rows of D fp32 -> fp16 when out_f16, else fp32. */
int spi_op_gather_rows(const float* x, void* y, int32_t rows, int32_t stride_rows, int32_t D, int32_t out_f16,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPI_OPS_H */
