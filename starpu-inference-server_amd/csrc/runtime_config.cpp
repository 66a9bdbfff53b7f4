#include "runtime_config.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" void spi_runtime_config_init(spi_runtime_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->workers_per_device = 4;
  c->coalesce_max_jobs = 1;
  c->pipeline_depth = 2;
  c->copy_threads = 4;
  c->h2d_mode = SPI_H2D_AUTO;
  c->batching.kind = SPI_BATCHING_FIXED;
}

namespace spi {

std::string resolve_runtime_config(const spi_runtime_config* c, double gflop_at_max_batch, bool hsa_agents,
                                   ResolvedConfig& out) {
  if (!c || c->num_devices < 1 || c->num_devices > SPI_MAX_REPLICAS || c->max_batch < 1 || c->num_inputs < 1 ||
      c->num_inputs > SPI_MAX_INPUTS || c->num_outputs < 1 || c->num_outputs > SPI_MAX_OUTPUTS ||
      c->h2d_mode < 0 || c->h2d_mode > SPI_H2D_WORKER_SDMA || c->batching.kind < 0 ||
      c->batching.kind > SPI_BATCHING_ADAPTIVE)
    return "invalid runtime configuration";
  out = ResolvedConfig{};
  out.cfg = *c;
  spi_runtime_config& cfg = out.cfg;
  if (cfg.workers_per_device <= 0) cfg.workers_per_device = 4;
  if (cfg.pipeline_depth <= 0) cfg.pipeline_depth = 2;
  if (cfg.copy_threads <= 0) cfg.copy_threads = 4;
  if (cfg.slots_per_device <= 0) cfg.slots_per_device = std::max(2, cfg.workers_per_device * cfg.pipeline_depth);
  if (cfg.batching.batch_limit <= 0 || cfg.batching.batch_limit > cfg.max_batch) cfg.batching.batch_limit = cfg.max_batch;
  for (int i = 0; i < c->num_inputs; ++i) {
    size_t n = spi_dtype_size(c->input_types[i]);
    if (!n || c->input_ndims[i] < 0 || c->input_ndims[i] >= SPI_MAX_DIMS) return "invalid input spec";
    for (int d = 0; d < c->input_ndims[i]; ++d) n *= (size_t)c->input_dims[i][d];
    out.in_sample_bytes.push_back(n);
  }
  for (int i = 0; i < c->num_outputs; ++i) {
    const size_t es = spi_dtype_size(c->output_types[i]);
    if (!es || c->output_elems[i] <= 0) return "invalid output spec";
    out.out_sample_bytes.push_back(es * (size_t)c->output_elems[i]);
  }
  if (cfg.h2d_mode == SPI_H2D_AUTO) {
    // SDMA-engine copies when the task's input keeps the PCIe link busy: at least 120 KiB of
    // input per GFLOP of the forward.  The threshold sits on a measured crossover
    // (tools/sdma_crossover.py, bs8, 4 workers, 32 in flight, profiles/r03/sdma_crossover.log):
    // SDMA / stream e2e = 1.116 for ResNet-18 (162 KiB/GFLOP), 0.952 ResNet-34 (80), 0.930
    // ResNet-50 (72), 0.949 ResNet-101 (38), 0.950 ResNet-152 (26); ViT-L (5) and BERT (0.1)
    // lose too.  The compute-bound side loses because the device's kernels run slower beside
    // the SDMA traffic, not because the worker waits for the copy: pinning the copies to a
    // free engine (a round-3 option, since removed) cut ResNet-152's per-task copy wait from ~7 ms
    // to ~1 ms and the rate still fell (9.2k vs 10.6k inf/s on the streams); round 4 re-measured
    // C4 / C5 at 10.1k / 4.56k on SDMA against 11.2k / 4.79k on the streams (tools/sdma_ab.py).
    // Below the threshold: a shared copy stream for <= 3 workers, the worker streams beyond
    // (four busy streams per device)
    size_t task_in = 0;
    for (size_t b : out.in_sample_bytes) task_in += b * (size_t)cfg.max_batch;
    const double gflop = gflop_at_max_batch;
    const bool sdma = hsa_agents && gflop > 0.0 && (double)task_in / gflop >= 120.0 * 1024.0;
    cfg.h2d_mode = sdma ? SPI_H2D_WORKER_SDMA
                        : cfg.workers_per_device <= 3 ? SPI_H2D_DEVICE_STREAM : SPI_H2D_WORKER_STREAM;
  }
  {
    // HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4)
    // round-robin; worker streams sharing a queue run serially.
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    const int queues = q ? std::atoi(q) : 4;
    const int need = cfg.workers_per_device + (cfg.h2d_mode == SPI_H2D_DEVICE_STREAM ? 1
                                               : cfg.h2d_mode == SPI_H2D_WORKER_COPY ? cfg.workers_per_device : 0);
    if (queues < need + 1) {
      char msg[256];
      std::snprintf(msg, sizeof(msg),
                    "spi_runtime: GPU_MAX_HW_QUEUES=%d < %d streams + 1; streams will share hardware queues and "
                    "serialize (set it before the first HIP call)\n",
                    queues, need);
      out.queue_warning = msg;
    }
  }
  for (int dv = 0; dv < c->num_devices; ++dv)
    if (!c->models[dv]) return "missing replica for device " + std::to_string(c->device_ids[dv]);
  // Per-worker warm-up (spi_runtime_config.warmup_batches): every batch size the batchers can
  // compose up to the asked one, and always max_batch.
  if (cfg.warmup_batches >= 0) {
    const int upto = cfg.warmup_batches == 0 ? cfg.max_batch : std::min(cfg.warmup_batches, cfg.max_batch);
    for (int b = 1; b <= upto; ++b) out.warmup.push_back(b);
  }
  if (out.warmup.empty() || out.warmup.back() != cfg.max_batch) out.warmup.push_back(cfg.max_batch);
  return "";
}

}  // namespace spi
