/*
 * spi_torch.h — the LibTorch side of the boundary: TorchScript loading, the
 * CPU codelet's forward, and the C++ weight extractor that feeds
 * spi_model_create.  Built as libspi_torch.so (links libtorch_cpu + libspi_hip),
 * so libspi_hip.so itself never depends on LibTorch.
 *
 * Reference interfaces each entry point replaces:
 *
 *   spi_torch_load            <- load_model (torch::jit::load + eval)
 *                                src/core/inference_runner.cpp:243-249
 *   spi_torch_cpu_forward     <- the body of run_inference on the CPU codelet:
 *                                forward under c10::InferenceMode, IValue
 *                                flattening (append_ivalue), output-count check
 *                                and TensorBuilder::copy_output_to_buffer
 *                                src/core/starpu_setup.cpp:594-624, 784-801,
 *                                496-513; src/core/tensor_builder.cpp:162-190.
 *                                It is an spi_cpu_forward_fn: the host puts it in
 *                                spi_codelet_args.cpu_forward with model_cpu =
 *                                the spi_torch_module*, and spi_cpu_inference_func
 *                                does the views, stamps and buffer checks.
 *   spi_torch_named_tensors   <- named_parameters()/named_buffers() of the
 *                                loaded module (what clone_model_to_gpus copies,
 *                                inference_runner.cpp:251-275), as fp32 arrays
 *   spi_torch_create_replica  <- clone_model_to_gpus for one device: extract +
 *                                spi_model_create (BN-fold, pack, upload)
 *   spi_torch_cpu_bench       <- N StarPU CPU workers draining a closed loop of
 *                                CPU-codelet tasks; inf/s = inferences /
 *                                (last response - first request)
 *                                (src/grpc/client/inference_client.cpp:259-270),
 *                                linear-interpolated percentiles
 *                                (src/core/latency_statistics.hpp:52-93).
 *                                Worker layouts: one worker with all cores as
 *                                intra-op threads (group_cpu_by_numa,
 *                                starpu_setup.cpp:299-385) or one per NUMA node.
 */
#ifndef SPI_TORCH_H
#define SPI_TORCH_H

#include "spi_codelet.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spi_torch_module spi_torch_module;

spi_torch_module* spi_torch_load(const char* path, char* err, size_t errlen);
void spi_torch_free(spi_torch_module* module);

/* spi_cpu_forward_fn over a spi_torch_module* (see above). */
int spi_torch_cpu_forward(void* model_cpu, const spi_tensor_view* inputs, int num_inputs,
                          spi_tensor_view* outputs, int num_outputs, char* err, size_t errlen);

/* 8-bit image tasks on a CPU worker (the counterpart of spi_model_set_input_transform): once
 * set, when input 0 of a task is a 4-D SPI_DTYPE_U8 view -- [B,3,H,W] (NCHW) or [B,H,W,3]
 * (NHWC, permuted first) -- spi_torch_cpu_forward feeds the module the contiguous fp32 NCHW
 * tensor x.float().mul(scale[c]).add(shift[c]): the same two fp32 roundings as the GPU
 * codelet, so both workers see the same image bit for bit.  Without a transform (the default;
 * NULL, NULL clears it) the byte tensor goes to the module unchanged.  Returns SPI_OK or
 * SPI_ERR_INVALID_ARGUMENT (non-finite value, a single NULL).  Set it before serving. */
int spi_torch_set_input_transform(spi_torch_module* module, const float scale[3], const float shift[3]);

/* Resize + centre crop of 8-bit image tasks on a CPU worker (the counterpart of spi_model_set_input_resize;
 * here the crop is given, a module has no image size): once set, a 4-D SPI_DTYPE_U8 input 0 of any size up to
 * 8192 -- [B,3,H,W], or [B,H,W,3] when dims[1] != 3 -- is resampled with ATen's antialiased bilinear
 * interpolation in float64 (upsample_bilinear2d_aa, align_corners false) to the size the GPU codelet resizes
 * to (short side resize_short, long side floor(resize_short long / short)), cropped to crop x crop at the same
 * round-half-even offsets and cast to fp32; the input transform (scale 1, shift 0 when none is set) then
 * applies as above.  The GPU codelet computes the same resample in fp32 (its header states the bound), so the
 * two workers' images agree to that bound, not bit for bit.  (0, 0) clears it.  Returns SPI_OK, or
 * SPI_ERR_INVALID_ARGUMENT unless 1 <= crop <= resize_short <= 8192; a task whose resized long side would
 * exceed 8192 fails at the forward. */
int spi_torch_set_input_resize(spi_torch_module* module, int32_t resize_short, int32_t crop);

/* Classification outputs on a CPU worker (the counterpart of spi_model_set_image_outputs, same bits,
 * same output order and element types): after the module's forward, whose single output is the
 * [B,classes] logits, spi_torch_cpu_forward emits logits.float() (unless SPI_IMAGE_NO_LOGITS),
 * softmax(logits.float(), -1), and the first top_k values / int64 indices of the stable descending sort
 * of the logits (values gathered from the probabilities with SPI_IMAGE_TOPK_PROBS), through the same
 * checked copy.  Refused (SPI_ERR_INVALID_ARGUMENT): unknown bits; SPI_IMAGE_NO_LOGITS with neither
 * other output; SPI_IMAGE_TOPK_PROBS without SPI_IMAGE_OUT_TOPK; top_k outside 1 .. 64 with
 * SPI_IMAGE_OUT_TOPK, or non-zero without.  The class count is known at the forward only: a task whose
 * logits have fewer than top_k or more than 16384 classes fails there.  (0, 0) resets. */
int spi_torch_set_image_outputs(spi_torch_module* module, int32_t image_io, int32_t top_k);

/* Floating named_parameters() then named_buffers() (first occurrence of a name
 * wins), each copied to contiguous fp32 and owned by the module handle.
 * Returns the count, or -1 on error. */
int32_t spi_torch_named_tensors(spi_torch_module* module, const spi_named_tensor** out);

spi_model* spi_torch_create_replica(spi_torch_module* module, int32_t device_id,
                                    const spi_model_config* config, char* err, size_t errlen);

/* at::set_num_threads / at::get_num_threads for the calling thread. */
void spi_torch_set_num_threads(int32_t n);
int32_t spi_torch_get_num_threads(void);

typedef struct spi_cpu_bench_result {
  int64_t tasks;            /* codelet calls completed */
  int64_t inferences;       /* tasks x batch */
  double seconds;           /* last response - first request */
  double inferences_per_s;
  double p50_ms, p95_ms;    /* per-task codelet latency */
  int32_t failed;
  char error[SPI_ERROR_LEN];
} spi_cpu_bench_result;

/* Closed loop through spi_cpu_inference_func: `workers` threads, each with
 * `threads_per_worker` intra-op threads and its own copy of the inputs
 * (host views, dims from the layout), run tasks until `seconds` have passed
 * or `max_tasks` tasks completed (0 = no cap).  `inputs` describe one batch;
 * outputs are sized from output_bytes. */
int spi_torch_cpu_bench(spi_torch_module* module, const spi_tensor_view* inputs, int32_t num_inputs,
                        const size_t* output_bytes, const int32_t* output_types, int32_t num_outputs,
                        int32_t workers, int32_t threads_per_worker, double seconds, int64_t max_tasks,
                        spi_cpu_bench_result* result);

#ifdef __cplusplus
}
#endif
#endif /* SPI_TORCH_H */
