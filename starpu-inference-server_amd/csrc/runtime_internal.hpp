// What runtime.cpp shares with loadgen.cpp beside the public spi_runtime.h: the clock of every
// spi_job_timing stamp, and the three facts the load generator reads of a runtime.
#pragma once
#include <time.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/spi_runtime.h"

namespace spi {

inline int64_t now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (int64_t)ts.tv_sec * 1000000000LL + ts.tv_nsec;
}

struct RuntimeShape {
  int32_t max_batch, num_outputs;
  const std::vector<size_t>* out_sample_bytes;  // [output], owned by the runtime
};
RuntimeShape runtime_shape(const spi_runtime* rt);  // runtime.cpp

}  // namespace spi
