// AdaptiveBatchingStrategy (batching_strategy.cpp:195-360), runtime-pressure path (no congestion
// monitor): queue fill + internal backlog pressure.  Pure arithmetic behind spi_batching_decide
// (include/spi_runtime.h); plain C++17, no HIP header.  tests/test_batching.py is its specification,
// runtime_check.cpp links it under the host sanitizers.
#pragma once
#include "../../include/spi_runtime.h"

namespace spi {

struct Pressure {
  bool congested = false, high = false, low = false, severe = false;
};

Pressure resolve_pressure(const spi_batching_config& c, const spi_batching_pressure& p);
int low_streak_threshold(const spi_batching_config& c);
int high_step(const spi_batching_config& c, int limit, bool severe);
int coalesce_timeout(const spi_batching_config& c, bool congested, int target);

}  // namespace spi
