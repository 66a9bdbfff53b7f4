// From the caller's spi_runtime_config to what spi_runtime_create works with: validation,
// defaults, per-sample byte sizes, the concrete H2D mode and the warm-up batch list.  Plain
// C++17, no HIP header; runtime_check.cpp checks every rule without a GPU.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/spi_runtime.h"

namespace spi {

struct ResolvedConfig {
  spi_runtime_config cfg{};  // defaults filled in, h2d_mode one of the concrete modes
  std::vector<size_t> in_sample_bytes, out_sample_bytes;
  std::vector<int> warmup;   // batch sizes every worker warms up, ascending, max_batch last
  std::string queue_warning; // GPU_MAX_HW_QUEUES too small for the streams ("" = fine); may be
                             // set beside an error, as the check precedes the replica check
};

// Returns "" and fills `out`, or the error message.  gflop_at_max_batch (the model's forward at
// max_batch, 0 = unknown) and hsa_agents (every device has its HSA agents) are consulted for
// SPI_H2D_AUTO only.
std::string resolve_runtime_config(const spi_runtime_config* c, double gflop_at_max_batch, bool hsa_agents,
                                   ResolvedConfig& out);

}  // namespace spi
