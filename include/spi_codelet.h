/*
 * spi_codelet.h — C-ABI drop-in boundary of the MI355X inference codelet.
 *
 * This header is the whole contract between a StarPU-Inference-Server style
 * host (task submission, slot pools, StarPU workers) and the HIP/CDNA4
 * forward pass.  It carries no C++ and no torch types: plain pointers, sizes,
 * fixed-size arrays and C function pointers.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference repository daxmawal/StarPU-Inference-Server):
 *
 *   spi_hip_inference_func   <- InferenceCodelet::cuda_inference_func
 *                               src/core/starpu_setup.cpp:807-846
 *   spi_cpu_inference_func   <- InferenceCodelet::cpu_inference_func
 *                               src/core/starpu_setup.cpp:784-801
 *   spi_codelet_init         <- InferenceCodelet::InferenceCodelet
 *                               src/core/starpu_setup.cpp:559-568
 *   spi_codelet_args         <- struct InferenceParams
 *                               src/core/inference_params.hpp:20-92
 *   spi_buffer_byte_size     <- starpu_setup_detail::buffer_byte_size
 *                               src/core/starpu_setup.cpp:515-542
 *   spi_select_replica       <- select_gpu_module
 *                               src/core/starpu_setup.cpp:725-778
 *   spi_model_create         <- clone_model_to_gpus / load_model
 *                               src/core/inference_runner.cpp:243-275
 *                               (one device-resident weight replica per device)
 *
 * Buffer convention (src/core/inference_task.cpp:802-822): buffers[0..ni) are
 * the inputs (STARPU_R), buffers[ni..ni+no) the outputs (STARPU_W); each
 * buffers[i] points at a StarPU vector or variable interface whose layout is
 * mirrored below.  On a GPU worker `ptr` is a device (HBM) address.
 *
 * Errors never cross this ABI as exceptions (the reference throws
 * StarPUCodeletException through StarPU's C frames, starpu_setup.cpp:710-716):
 * they are returned in args->status / args->error, and the host adapter turns
 * them into its own exception type.
 */
#ifndef SPI_CODELET_H
#define SPI_CODELET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPI_ABI_VERSION 1u

/* src/utils/inference_limits.hpp:6-8 */
#define SPI_MAX_INPUTS 16
#define SPI_MAX_OUTPUTS 16
#define SPI_MAX_DIMS 8
#define SPI_MAX_REPLICAS 32
#define SPI_ERROR_LEN 256

/* ---------------------------------------------------------------------------
 * StarPU 1.4 data-interface layouts (starpu_data_interfaces.h).  The codelet
 * reads only id, ptr, nx and elemsize, exactly like the reference
 * (starpu_setup.cpp:515-542, tensor_builder.cpp:120).  The id values follow
 * StarPU 1.4's enum starpu_data_interface_id; a build against the real
 * <starpu.h> static_asserts them (csrc/spi_starpu_adapter.cpp, -DSPI_WITH_STARPU).
 * ------------------------------------------------------------------------- */
enum spi_interface_id {
  SPI_STARPU_MATRIX_INTERFACE_ID = 0,
  SPI_STARPU_BLOCK_INTERFACE_ID = 1,
  SPI_STARPU_VECTOR_INTERFACE_ID = 2,
  SPI_STARPU_CSR_INTERFACE_ID = 3,
  SPI_STARPU_BCSR_INTERFACE_ID = 4,
  SPI_STARPU_VARIABLE_INTERFACE_ID = 5
};

/* Field widths: StarPU 1.4 declares the vector's nx (and slice_base) size_t --
 * its register call takes `size_t nx`, which the reference's own link-time
 * override of starpu_vector_data_register has to match exactly
 * (tests/support/starpu_task_submit_override.cpp:117-119; the Dockerfile pins
 * StarPU 1.4.8, Dockerfile:58).  A resize writes the full 8 bytes
 * (resize_starpu_vector_interface, starpu_vector_resize_utils.hpp:19-64). */
typedef struct spi_vector_interface {
  int32_t id; /* enum starpu_data_interface_id */
  uintptr_t ptr;
  uintptr_t dev_handle;
  size_t offset;
  size_t nx;
  size_t elemsize;
  size_t slice_base;
  size_t allocsize;
} spi_vector_interface;

typedef struct spi_variable_interface {
  int32_t id;
  uintptr_t ptr;
  uintptr_t dev_handle;
  size_t offset;
  size_t elemsize;
} spi_variable_interface;

/* Element types use at::ScalarType's numeric codes, so a LibTorch caller can
 * pass static_cast<int>(scalar_type) (datatype_utils.hpp:20-46). */
enum spi_dtype {
  SPI_DTYPE_U8 = 0,
  SPI_DTYPE_I8 = 1,
  SPI_DTYPE_I16 = 2,
  SPI_DTYPE_I32 = 3,
  SPI_DTYPE_I64 = 4,
  SPI_DTYPE_F16 = 5,
  SPI_DTYPE_F32 = 6,
  SPI_DTYPE_F64 = 7,
  SPI_DTYPE_BOOL = 11,
  SPI_DTYPE_BF16 = 15
};

/* DeviceType (src/core/device_type.hpp) */
enum spi_device_type { SPI_DEVICE_UNKNOWN = 0, SPI_DEVICE_CPU = 1, SPI_DEVICE_GPU = 2 };

/* Status codes mirroring the reference exception taxonomy
 * (src/utils/exceptions.hpp:11-157). */
enum spi_status {
  SPI_OK = 0,
  SPI_ERR_INVALID_ARGUMENT = 1,   /* InferenceExecutionException (layout/limits) */
  SPI_ERR_NO_REPLICA = 2,         /* "No GPU model replica available ..." */
  SPI_ERR_OUTPUT_MISMATCH = 3,    /* "Output buffer size mismatch in bytes" */
  SPI_ERR_UNSUPPORTED = 4,        /* unsupported interface id / dtype / model */
  SPI_ERR_DEVICE = 5,             /* HIP runtime error */
  SPI_ERR_MODEL = 6,              /* model recognition / weight packing */
  SPI_ERR_CPU_FORWARD = 7         /* host forward callback failed */
};

/* Opaque per-device weight replica (BN-folded, MFMA-packed, in HBM). */
typedef struct spi_model spi_model;

/* One host-side view handed to the CPU forward callback. */
typedef struct spi_tensor_view {
  void* data;
  int32_t dtype;
  int32_t ndim;
  int64_t shape[SPI_MAX_DIMS];
} spi_tensor_view;

/* CPU forward (the reference's LibTorch model_cpu->forward): the host binds
 * its own CPU model here; the codelet does views, stamps and checked copies.
 * Returns 0 on success; on failure writes a message into err. */
typedef int (*spi_cpu_forward_fn)(void* model_cpu, const spi_tensor_view* inputs,
                                  int num_inputs, spi_tensor_view* outputs,
                                  int num_outputs, char* err, size_t errlen);

/* The cl_arg block (InferenceParams, inference_params.hpp:77-92), as POD.
 * The caller owns it for the task's lifetime (inference_task.hpp:41-64). */
typedef struct spi_codelet_args {
  uint32_t abi_version; /* = SPI_ABI_VERSION */
  uint32_t num_inputs;
  uint32_t num_outputs;
  int32_t request_id;
  int64_t batch_size;
  int32_t verbosity;
  int32_t _pad0;

  /* TensorLayout: dims[i][0] is the effective batch
   * (inference_task.cpp:606-613). */
  int64_t dims[SPI_MAX_INPUTS][SPI_MAX_DIMS];
  int64_t num_dims[SPI_MAX_INPUTS];
  int32_t input_types[SPI_MAX_INPUTS];
  /* expected output element types (copy_output_to_buffer's expected_type) */
  int32_t output_types[SPI_MAX_OUTPUTS];

  /* Limits */
  uint64_t max_inputs;
  uint64_t max_dims;

  /* ModelPointers: replica i serves device_ids[i] (or worker_ids[i]). */
  void* model_cpu;
  spi_cpu_forward_fn cpu_forward;
  int32_t num_replicas;
  int32_t num_device_ids;
  int32_t num_worker_ids;
  int32_t _pad1;
  int32_t device_ids[SPI_MAX_REPLICAS];
  int32_t worker_ids[SPI_MAX_REPLICAS];
  spi_model* models_gpu[SPI_MAX_REPLICAS];

  /* Timing out-fields: CLOCK_MONOTONIC nanoseconds (MonotonicClock). */
  int64_t codelet_start_ns;
  int64_t codelet_end_ns;
  int64_t inference_start_ns;

  /* DeviceInfo out-fields */
  int32_t executed_on; /* enum spi_device_type */
  int32_t worker_id;
  int32_t device_id;

  /* Result */
  int32_t status;
  char error[SPI_ERROR_LEN];
} spi_codelet_args;

/* ---------------------------------------------------------------------------
 * Codelet entry points (starpu_cpu_func_t / starpu_hip_func_t signature).
 * ------------------------------------------------------------------------- */

/* GPU codelet: enqueues the whole forward pass on the worker's HIP stream and
 * returns without synchronising (STARPU_HIP_ASYNC).  Outputs are written by the
 * last kernel straight into the W buffers. */
void spi_hip_inference_func(void** buffers, void* cl_arg);

/* CPU codelet: views over host buffers -> args->cpu_forward -> checked memcpy
 * (tensor_builder.cpp:162-190). */
void spi_cpu_inference_func(void** buffers, void* cl_arg);

/* Fills a `struct starpu_codelet` (passed as void*) when the library is built
 * with <starpu.h> (SPI_WITH_STARPU); returns SPI_ERR_UNSUPPORTED otherwise. */
int spi_codelet_init(void* starpu_codelet);

/* Worker context for the calling thread: what starpu_worker_get_id(),
 * starpu_worker_get_devid() and starpu_hip_get_local_stream() return inside a
 * StarPU worker.  The mini-runtime and tests set it; with SPI_WITH_STARPU the
 * codelet queries StarPU instead when no context was set. */
void spi_set_worker_context(int32_t worker_id, int32_t device_id, void* hip_stream);
void spi_clear_worker_context(void);

/* Helpers that mirror reference utilities (exposed for host-side tests). */
int spi_buffer_byte_size(const void* buffer_iface, size_t* out_bytes);
int spi_select_replica(const spi_codelet_args* args, int32_t worker_id,
                       int32_t device_id, int32_t* out_index);
size_t spi_dtype_size(int32_t dtype);
void spi_args_init(spi_codelet_args* args);

/* ---------------------------------------------------------------------------
 * Model replicas.
 * ------------------------------------------------------------------------- */
enum spi_family {
  SPI_FAMILY_AUTO = 0,   /* recognise from parameter names */
  /* torchvision ResNet naming: resnet18/34/50/101/152, wide_resnet50_2/101_2 and the grouped
   * resnext50_32x4d / resnext101_32x8d.  A grouped conv is accepted as the bottleneck conv2 only, with one
   * group count on every block, widths that are multiples of 128 and 4, 8, 16, 32 or 64 channels per group;
   * anything else fails with "grouped/unsupported conv".  SPI_PREC_F16 / F16M run it on the grouped kernel;
   * SPI_PREC_F32 / F16X3 (and SPI_GCONV=0 at replica build) pack its dense block-diagonal expansion for
   * the dense kernels: same results at their parity bar, 32x the conv's MFMA work and weight bytes
   * (resnext101_32x8d: 170 MiB grouped in fp16, 801 MiB expanded, twice that in fp32). */
  SPI_FAMILY_RESNET = 1,
  SPI_FAMILY_BERT = 2,   /* HF BertModel naming, returns last_hidden_state */
  SPI_FAMILY_VIT = 3,    /* torchvision vit_*_16 naming */
  SPI_FAMILY_AFFINE = 4  /* y = x * scale + shift (toy models of the reference tests) */
};

/* SPI_PREC_F16X3: split fp16 -- fp32 activations, each MFMA operand split into
 * hi + lo fp16 halves, hi*hi + hi*lo + lo*hi per fragment (fp32-grade
 * results at the fp16 MFMA rate).
 * SPI_PREC_F16M, ResNet: fp16 activations and fp16 MFMA operands everywhere except
 * the precision-critical layers -- the stem (the image rounded to fp16 x hi + lo
 * weights, fp16 out) and the downsample 1x1 convs (fp16 activations x hi + lo weights,
 * fp16 out); the FC runs on plain fp16 weights (round 5: CPU emulation worst case
 * 0.74e-3 over 8 input seeds against the 1e-3 bar, GPU 0.60-0.69e-3).  BERT / ViT: the
 * F16 path with hi + lo weights on every GEMM (two fp16 MFMAs per fragment pair: the
 * weights' rounding is the largest of the fp16 path's error sites,
 * tools/prec_emulate_bert.py). */
enum spi_precision { SPI_PREC_F32 = 0, SPI_PREC_F16 = 1, SPI_PREC_F16X3 = 2, SPI_PREC_F16M = 3 };

typedef struct spi_named_tensor {
  const char* name; /* parameter/buffer name as in named_parameters() */
  const void* data; /* host pointer, fp32, contiguous */
  int32_t dtype;    /* SPI_DTYPE_F32 */
  int32_t ndim;
  int64_t shape[SPI_MAX_DIMS];
} spi_named_tensor;

typedef struct spi_model_config {
  int32_t family;     /* enum spi_family */
  int32_t precision;  /* enum spi_precision: MFMA operand type */
  int32_t max_batch;  /* largest dims[0] the replica will see */
  int32_t num_heads;  /* transformers: attention heads; hidden / num_heads must be 32 or 64 (hidden a
                         multiple of 64, <= 1024, so 32-wide models have an even count).  0 = hidden / 64:
                         a 32-wide model (MiniLM: 384 over 12) must state its count.  Any other width is
                         refused at creation with a message naming hidden, heads and the two widths. */
  int32_t seq_len;    /* BERT: max sequence length (0 = from position table) */
  int32_t image_size; /* ResNet/ViT: input H = W (0 = 224) */
  float eps;          /* norm epsilon (0 = family default) */
  float affine_scale; /* AFFINE only */
  float affine_shift; /* AFFINE only */
  int32_t bert_io;    /* BERT only: SPI_BERT_* bits; 0 = [ids, mask] -> last_hidden_state */
} spi_model_config;

/* spi_model_config.bert_io: which outputs a BERT replica writes and whether it takes segment ids.
 * The field replaces a padding word, so a zeroed config keeps the one-output contract.
 *
 * Outputs, always in this order and all fp32: last_hidden_state [B,S,D] (unless
 * SPI_BERT_NO_HIDDEN), then pooler_output [B,D], then the masked mean [B,D].  With
 * SPI_BERT_OUT_POOLER alone that is HF's BertModel(..., return_dict=False) tuple.
 *   pooler_output = tanh(W_p . last_hidden_state[:, 0] + b_p)   (pooler.dense.weight / .bias)
 *   masked mean   = sum_s m[b,s] h[b,s,:] / max(sum_s m[b,s], 1e-9), m = (attention_mask != 0),
 *                   the rule the attention bias uses; without a mask input every token counts.
 * Inputs: input_ids, then attention_mask, then -- with SPI_BERT_TOKEN_TYPES only --
 * token_type_ids, each [B,S] int64 and each optional from the end.  Type ids are clamped to
 * [0, type_vocab - 1] like word ids; all-zero ids, or a two-input task, give the bits of a
 * replica without the flag.
 * spi_model_create refuses, with a message: unknown bits; any bit on another family;
 * SPI_BERT_NO_HIDDEN with neither pooled output; SPI_BERT_OUT_POOLER on a model without
 * pooler.dense.weight / .bias (add_pooling_layer=False).
 * The measurement hooks (spi_model_profile, _profile_op, _launch_table) read `inputs` up to
 * the replica's input count (absent inputs null) and `outputs` in the order above.
 *
 * Task heads (SPI_BERT_HEAD_*): the one dense layer of a fine-tuned BERT, written on the device.  At
 * most one head per replica (two of them share the parameter name `classifier`); its output(s), fp32,
 * follow hidden, pooler and mean, so a replica has at most five outputs.  L, the label count, is the
 * head weight's first dimension (spi_model_bert_num_labels), not a config field.
 *   SPI_BERT_HEAD_SEQUENCE  logits [B,L] = W_c . pooler_output + b_c: HF BertForSequenceClassification
 *                           in eval.  classifier.weight [L,D], classifier.bias [L], 1 <= L <= 1024, and
 *                           pooler.dense.*; the pooler runs whether or not SPI_BERT_OUT_POOLER also
 *                           makes it an output.
 *   SPI_BERT_HEAD_TOKEN     logits [B,S,L] = W_c . last_hidden_state + b_c on every token, padded ones
 *                           included: HF BertForTokenClassification.  classifier.weight [L,D],
 *                           classifier.bias [L], 1 <= L <= 64.
 *   SPI_BERT_HEAD_QA        two outputs, start_logits [B,S] then end_logits [B,S]: rows 0 and 1 of
 *                           qa_outputs.weight [2,D] / .bias [2], HF BertForQuestionAnswering.
 * The head's parameters sit outside the `bert.` prefix the other names share: they are the one tensor
 * named `classifier.weight` or ending in `.classifier.weight` (likewise .bias, qa_outputs.*).
 * SPI_BERT_NO_HIDDEN is also satisfied by a head bit: logits alone are a valid replica, and for a
 * token-level head the hidden state is then never written to memory.
 * Independence: a row's logits depend on that row's inputs alone -- not on B, not on the row's
 * position in the batch, not on graphs being on -- so dynamic batching changes nobody's answer.  Every
 * sum has a fixed order and there are no floating-point atomics: two runs give the same bits.
 * spi_model_create also refuses: two head bits; a head bit on another family; a missing or ambiguous
 * head parameter (named); a weight that is not [L,D] or a bias that is not [L]; L outside the head's
 * range (QA: L != 2); SPI_BERT_HEAD_SEQUENCE without pooler.dense.weight / .bias.
 *
 * The two-layer sequence head.  With SPI_BERT_HEAD_SEQUENCE, a parameter list that holds a tensor named
 * `classifier.out_proj.weight` (or ending in `.classifier.out_proj.weight`) is HF's
 * RobertaClassificationHead: logits [B,L] = W_o . tanh(W_d . last_hidden_state[:, 0] + b_d) + b_o with
 * classifier.dense.weight [D,D] / .bias [D] and classifier.out_proj.weight [L,D] / .bias [L], 1 <= L <=
 * 1024.  The names decide, not SPI_BERT_POS_FROM_IDS.  The pooler's and the sequence head's launches
 * compute it (dense is packed where pooler.dense goes), so the logits have the bits of a replica whose
 * tensors are named pooler.dense.* and classifier.*.  Refused, naming the tensors: together with
 * SPI_BERT_OUT_POOLER (that model has no pooler); a missing classifier.dense.*; wrong shapes.
 *
 * SPI_BERT_POS_FROM_IDS: RoBERTa's position rule (roberta, xlm-roberta, camembert checkpoints; HF's
 * create_position_ids_from_input_ids).  Embedding row (b, s) is
 *   n(b,s) = #{ j <= s : ids[b][j] != SPI_ROBERTA_PAD_ID }       (raw int64 ids, before any clamp)
 *   p(b,s) = ids[b][s] != SPI_ROBERTA_PAD_ID ? 1 + n(b,s) : 1
 *   row    = LN( (word[clamp(ids[b][s])] + type_row) + pos[p(b,s)] ) * gamma + beta
 * -- the fp32 sum, in the order, of a replica without the bit; only the position row differs.  A pad
 * token reads position row 1, whatever it holds.  The position depends on input_ids only, never on
 * attention_mask; segment ids (SPI_BERT_TOKEN_TYPES) combine with it unchanged.  The pad id is fixed at
 * SPI_ROBERTA_PAD_ID = 1, the value of every published RoBERTa / XLM-R / CamemBERT-family checkpoint;
 * a model with another pad id is out of scope and must not be served with this bit.
 * The replica's longest sequence is then position rows - 2 (512 for a 514-row table): seq_len = 0
 * resolves to it, spi_model_create refuses a larger seq_len (the message names the rows and the rule),
 * and a longer task is refused like any over-long task.  The bit changes no packed byte, FLOP count or
 * workspace size; spi_model_describe appends " pos[ids]".  Without the bit nothing changes.
 * Independence: a row's embedding depends on its own sequence's ids alone -- the count is an exact
 * integer taken by the row's own wave -- not on B, the row's place in the batch or graphs being on; two
 * runs give the same bits.
 * Bits 16, 32 and 64 stay unknown. */
#define SPI_ROBERTA_PAD_ID 1
enum spi_bert_io {
  SPI_BERT_OUT_POOLER = 1,
  SPI_BERT_OUT_MEAN = 2,
  SPI_BERT_NO_HIDDEN = 4,
  SPI_BERT_TOKEN_TYPES = 8,
  SPI_BERT_HEAD_SEQUENCE = 128,
  SPI_BERT_HEAD_TOKEN = 256,
  SPI_BERT_HEAD_QA = 512,
  SPI_BERT_POS_FROM_IDS = 1024
};

spi_model* spi_model_create(int32_t device_id, const spi_model_config* config,
                            const spi_named_tensor* params, int32_t num_params,
                            char* err, size_t errlen);
void spi_model_destroy(spi_model* model);
/* Device bytes of the packed weight blob. */
size_t spi_model_weight_bytes(const spi_model* model);
/* FNV-1a 64 digest of the packed weight blob (computed on the host at build
 * time): identical inputs give identical digests, whichever thread built it. */
uint64_t spi_model_weight_digest(const spi_model* model);
/* Algorithmic FLOPs of one forward at the given batch (roofline numerator). */
double spi_model_flops(const spi_model* model, int64_t batch);
/* Short description ("resnet[2,2,2,2] basic f16 ..."). */
const char* spi_model_describe(const spi_model* model);
/* The label count L of a BERT replica's task head (SPI_BERT_HEAD_*), 0 without one.  Works on a
 * host-only replica. */
int32_t spi_model_bert_num_labels(const spi_model* model);
/* Measurement hook (not on the task path): runs one forward on `stream` with
 * every kernel launch bracketed by hipEvents, synchronises, and returns the
 * number of ops; per op: device milliseconds, algorithmic FLOPs, algorithmic
 * HBM bytes and a name (name_len bytes each).  Returns -1 on error. */
int spi_model_profile(spi_model* model, void* stream, int64_t batch, int64_t seq,
                      const void* const* inputs, void* const* outputs, float* op_ms,
                      double* op_flops, double* op_bytes, char* op_names, int32_t name_len,
                      int32_t max_ops);
/* Measurement hook: the same eager forward with the op named `op_name` (its
 * first occurrence) launched `reps` times back to back between one pair of
 * hipEvents; returns its device milliseconds per launch and its algorithmic
 * FLOPs / HBM bytes per launch.  Returns 0, or -1 (unknown op, bad arguments). */
int spi_model_profile_op(spi_model* model, void* stream, int64_t batch, int64_t seq,
                         const void* const* inputs, void* const* outputs, const char* op_name,
                         int32_t reps, float* ms_per_launch, double* flops, double* bytes);
/* Measurement hook: one eager forward on `stream` with every kernel launch recorded,
 * as text, one line per launch: "op_index\top_name\tkernel\tgrid_x\tgrid_y\tgrid_z\tblock\n"
 * (grid in workgroups).  It maps a rocprofv3 kernel trace of graph-replayed forwards,
 * which names kernels and grids only, back to ops (tools/trace_ops.py --launches).
 * Writes at most buflen - 1 bytes plus a NUL; returns the full length, or -1 on error. */
int64_t spi_model_launch_table(spi_model* model, void* stream, int64_t batch, int64_t seq,
                               const void* const* inputs, void* const* outputs, char* buf, size_t buflen);
/* Debug hooks of the replica's host-only forward plan (csrc/model_plan.hpp); neither needs a device, so
 * both work on a host-only replica (device_id -1).
 * spi_model_workspace_plan: the bytes of each per-stream workspace buffer at max_batch under the options
 * in force, in allocation order (bytes_out[0 .. min(*n, cap))), the buffer count in *n, the split-K slab
 * floats a workspace gets and what the launches at max_batch plan before the allocation's floor.
 * spi_model_plan_check: walks one forward at `batch` (BERT: `seq` tokens) launching nothing and holds every
 * GEMM, conv and conv pair against the planned workspace exactly as the launch does; *steps = the number of
 * launches held.  Both return an spi_status; a step that does not fit is SPI_ERR_INVALID_ARGUMENT with the
 * step named in spi_last_error(). */
int spi_model_workspace_plan(const spi_model* model, size_t* bytes_out, int32_t cap, int32_t* n,
                             size_t* partial_floats, size_t* partial_before_floor);
int spi_model_plan_check(const spi_model* model, int64_t batch, int64_t seq, int32_t* steps);
/* 8-bit image tasks.  A ResNet / ViT replica also takes tasks whose input_types[0] is
 * SPI_DTYPE_U8: decoded pixels, one byte per element, laid out as the task's dims say --
 * [B,3,S,S] (NCHW) or [B,S,S,3] (NHWC, what image decoders produce), S the replica's
 * image size.  The kernel that reads the task's buffer (the fused stem, or the layout
 * ingest / ViT patchify) loads the bytes itself, so no fp32 image is built on the host and
 * a quarter of the bytes cross the host link.  Pixel p of channel c enters the network as
 *     (float)p * scale[c] + shift[c]
 * computed as one fp32 multiply rounded to nearest, then one fp32 add rounded to nearest,
 * never a fused multiply-add: a host that does the same two operations in float32
 * (numpy x * s + b, ATen x.float().mul(s).add(b)) reproduces the value bit for bit, and
 * the forward then equals the one of an fp32 task holding that image.  The conv's zero
 * padding is zero after the transform, as in PyTorch on a normalised image.
 * The default is scale 1, shift 0; passing NULL for both resets to it.  Returns
 * SPI_ERR_INVALID_ARGUMENT for a non-finite value or a single NULL, SPI_ERR_UNSUPPORTED for
 * a replica of another family.  The values travel as kernel arguments of each forward:
 * nothing is allocated on the device or captured into a graph, and fp32 tasks ignore them,
 * so one replica serves fp32 and 8-bit tasks interleaved.  Call it before serving: it is
 * not synchronised with forwards being enqueued on other threads.
 * The measurement hooks above (spi_model_profile, _profile_op, _launch_table) carry no
 * element type and always read fp32 NCHW inputs. */
int spi_model_set_input_transform(spi_model* model, const float scale[3], const float shift[3]);
/* Resize + centre crop of 8-bit image tasks on the device (opt-in): the first two steps of torchvision's
 * weights.transforms() preset -- resize the short side, centre-crop -- in front of the transform above.
 * resize_short 0 (the default) leaves the replica as it is: an 8-bit task must be [B,3,S,S] or [B,S,S,3].
 * S <= resize_short <= 8192 (S, the replica's image size, is the crop) switches it on for a ResNet / ViT
 * replica; other values return SPI_ERR_INVALID_ARGUMENT, another family SPI_ERR_UNSUPPORTED, and any call
 * once a stream workspace of the replica exists (after the first forward or warm-up) is refused like
 * spi_model_set_image_outputs: the resampled image, max_batch x 3 x S x S fp32, belongs to the workspace.
 * Every refusal leaves a message in spi_last_error().  spi_model_describe appends " resize<R>" (" resize256");
 * FLOPs, weight bytes and the digest do not change.
 *
 * With the resize on, an SPI_DTYPE_U8 task may be [B,3,H,W] or [B,H,W,3] with any 1 <= H, W <= 8192:
 * dims[1] == 3 means NCHW (also when dims[3] == 3), otherwise dims[3] == 3 means NHWC, anything else is the
 * layout-mismatch error; the buffer is checked at one byte per element; a task whose resized long side would
 * exceed 8192 is refused.  An S x S task takes the same path (one rule, not two).  fp32 tasks keep the strict
 * [B,3,S,S] check and run as before.  One kernel launch in front of the forward writes the fp32 image the
 * network reads; its value at output pixel (oy, ox), channel c:
 *   1. resized size (torchvision Resize(int)): short = min(H,W) becomes R = resize_short, the long side
 *      floor(R long / short); call the result RH x RW;
 *   2. crop offset (torchvision CenterCrop): top = round_half_even((RH - S) / 2) -- with d = RH - S, k = d >> 1:
 *      k if d or k is even, else k + 1 (d = 0..5: 0, 0, 1, 2, 2, 2) -- and left likewise;
 *   3. antialiased bilinear resample (ATen _upsample_bilinear2d_aa, align_corners = false), separable, per
 *      axis in integers: for output index i of n_out from n_in source pixels, m = max(n_in, n_out),
 *      c2 = n_in (2 i + 1), taps j in [xmin, xmax) with xmin = max(0, floor((c2 - 2 m + n_out) / (2 n_out)))
 *      and xmax = min(n_in, floor((c2 + 2 m + n_out) / (2 n_out))), weights
 *      w_j = max(0, 1 - |n_out (2 j + 1) - c2| / (2 m)) -- the integer numerator converted to fp32 exactly, one
 *      fp32 divide, one subtract -- normalised by their fp32 sum; rows first horizontally, then the vertical
 *      pass, each sum in ascending j with one rounding per tap; only the crop's rows and columns are computed;
 *   4. the transform above on the fp32 result v: fl(fl(v scale[c]) + shift[c]).
 * Intermediate and result are fp32 and are NOT rounded back to 8 bits: torchvision's Resize on a uint8 tensor
 * rounds to the nearest pixel level, so the two differ by at most half a level (scale[c] / 2 after the
 * transform).  Against the same resample in float64 the value is within 255 (Kx + Ky + 4) 2^-24 pixel levels
 * (Kx, Ky the largest tap counts).  For H = W = R = S the weights are exactly {1, 0} and the forward equals
 * the plain 8-bit task's bit for bit.  The result for an image does not depend on the batch, its place in it,
 * or on graphs being on. */
int spi_model_set_input_resize(spi_model* model, int32_t resize_short);
/* Classification outputs of a ResNet / ViT replica: what it hands back beside, or instead of, its
 * [B,classes] fp32 logits.  One more kernel launch after the classifier layer writes every selected
 * output of the batch; with nothing selected (image_io 0, the default) the replica is unchanged.
 *
 * Outputs, always in this order: the logits [B,classes] fp32 (unless SPI_IMAGE_NO_LOGITS), the
 * probabilities [B,classes] fp32 (SPI_IMAGE_OUT_PROBS), then with SPI_IMAGE_OUT_TOPK the top-k values
 * [B,top_k] fp32 and the top-k indices [B,top_k] SPI_DTYPE_I64 (what torch.topk / torch.sort return).
 *   probabilities  p[j] = exp(x[j] - max_j x) / sum_j exp(x[j] - max_j x) in fp32, summed in one fixed
 *                  order without atomics: the same bits from run to run.  -inf logits give
 *                  probability 0; +inf or NaN logits give unspecified results.
 *   top-k          the row's top_k entries by logit, descending; equal logits by ascending class index,
 *                  0.0 == -0.0: torch.sort(x, descending=True, stable=True).  The order is always the
 *                  logits', so the indices do not depend on SPI_IMAGE_TOPK_PROBS.  The values are the
 *                  logits' own bits at those indices; with SPI_IMAGE_TOPK_PROBS, the bits the
 *                  probability output holds (or would hold) there.
 * Refused, with a message in spi_last_error(): unknown bits; a replica of another family
 * (SPI_ERR_UNSUPPORTED); SPI_IMAGE_NO_LOGITS with neither other output; SPI_IMAGE_TOPK_PROBS without
 * SPI_IMAGE_OUT_TOPK; top_k outside 1 .. min(classes, 64) with SPI_IMAGE_OUT_TOPK, or non-zero without;
 * more than 16384 classes; and any call once a stream workspace of the replica exists (after the first
 * forward or warm-up: the logits scratch of a SPI_IMAGE_NO_LOGITS replica, max_batch x classes x 4
 * bytes, belongs to the workspace).  (0, 0) before that point resets to the one-output contract.
 * The measurement hooks read `outputs` in the order above; spi_model_describe appends
 * " out[logits,probs,top5]" (the selected names) when bits are set.  FLOPs, weight bytes and the digest
 * do not change. */
enum spi_image_io {
  SPI_IMAGE_OUT_PROBS = 1,  /* softmax(logits) [B,classes] fp32 */
  SPI_IMAGE_OUT_TOPK = 2,   /* top-k values [B,k] fp32 and indices [B,k] int64 */
  SPI_IMAGE_NO_LOGITS = 4,  /* the logits are not an output */
  SPI_IMAGE_TOPK_PROBS = 8  /* top-k values are probabilities, not logits */
};
int spi_model_set_image_outputs(spi_model* model, int32_t image_io, int32_t top_k);
/* Capture launch-bound forwards into hipGraphs (per stream, per batch). */
void spi_model_set_graphs(spi_model* model, int32_t enable);
/* Per-worker warm-up (inference_runner.cpp:507-560): allocate `stream`'s
 * workspace and, with graphs on, capture the forward body for (batch, seq,
 * with_mask) now rather than inside a live request.  Enqueues no work.
 * seq / with_mask matter for BERT only.  Returns SPI_OK or an error status
 * (message in spi_last_error()). */
int spi_model_warmup(spi_model* model, void* stream, int64_t batch, int64_t seq, int32_t with_mask);

/* ---------------------------------------------------------------------------
 * Small device utilities so hosts without a HIP runtime binding (ctypes,
 * cgo, JNI) can allocate and move buffers.
 * ------------------------------------------------------------------------- */
int spi_device_count(void);
int spi_set_device(int32_t device_id);
void* spi_device_malloc(size_t bytes);
void spi_device_free(void* ptr);
void* spi_host_malloc(size_t bytes); /* pinned (hipHostMalloc portable) */
void spi_host_free(void* ptr);
int spi_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int spi_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int spi_memset_d(void* dst, int value, size_t bytes, void* stream);
void* spi_stream_create(void);
void spi_stream_destroy(void* stream);
int spi_stream_synchronize(void* stream);
const char* spi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SPI_CODELET_H */
