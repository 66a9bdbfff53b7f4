// The batching strategy's decisions (batching.hpp) and their C entry point spi_batching_decide.
#include "batching.hpp"

#include <algorithm>
#include <climits>

namespace spi {

constexpr double kInternalHigh = 0.75, kInternalLow = 0.25, kInternalSevere = 0.95;
constexpr double kPreparedHigh = 1.0, kPreparedSevere = 2.0;

Pressure resolve_pressure(const spi_batching_config& c, const spi_batching_pressure& p) {
  Pressure r;
  if (!c.congestion_enabled) return r;
  const double fill_high = std::clamp(c.fill_high, 0.0, 1.0);
  const double fill_low = std::clamp(std::min(c.fill_low, c.fill_high), 0.0, fill_high);
  // sample_internal_pressure
  bool ih = false, il = false, is = false;
  const int64_t backlog = p.prepared_depth + p.inflight_tasks;
  if (p.max_inflight_tasks > 0) {
    const double inflight = (double)p.inflight_tasks / (double)p.max_inflight_tasks;
    const double back = (double)backlog / (double)p.max_inflight_tasks;
    ih = inflight >= kInternalHigh || back >= kInternalHigh;
    il = inflight <= kInternalLow && back <= kInternalLow;
    is = inflight >= kInternalSevere || back >= kInternalSevere;
  } else {
    const double ref = std::max(1, c.batch_limit);
    const double prepared = (double)p.prepared_depth / ref;
    ih = prepared >= kPreparedHigh;
    il = p.prepared_depth == 0;
    is = prepared >= kPreparedSevere;
  }
  // resolve_runtime_pressure
  const double fill = p.queue_capacity > 0 ? (double)p.queue_size / (double)p.queue_capacity : 0.0;
  r.congested = p.congested != 0;
  r.high = fill >= fill_high || ih;
  r.low = !r.congested && fill <= fill_low && il;
  r.severe = r.congested || is;
  return r;
}

int low_streak_threshold(const spi_batching_config& c) {
  if (!c.congestion_enabled) return 1;
  const int tick = std::max(1, c.tick_interval_us);
  return std::max(1, std::max(tick, c.exit_horizon_us) / tick);
}

int high_step(const spi_batching_config& c, int limit, bool severe) {
  if (limit <= 1 || !c.congestion_enabled) return 1;
  const int tick = std::max(1, c.tick_interval_us);
  const int entry_ticks = std::max(1, std::max(tick, c.entry_horizon_us) / tick);
  const int base = std::max(1, limit / entry_ticks);
  if (!severe) return base;
  return std::max(base, std::max(1, limit / std::max(1, low_streak_threshold(c))));
}

int coalesce_timeout(const spi_batching_config& c, bool congested, int target) {
  const int configured = std::max(0, c.coalesce_timeout_us);
  if (!c.congestion_enabled || !congested) return configured;
  const int tick = std::max(1, c.tick_interval_us);
  return std::max(configured, std::max(1, tick / std::max(1, target)));
}

}  // namespace spi

using namespace spi;

extern "C" int spi_batching_decide(spi_batching_state* st, const spi_batching_config* c,
                                   const spi_batching_pressure* p, int64_t now, int32_t* out_target,
                                   int32_t* out_timeout_us) {
  if (!st || !c || !p || !out_target || !out_timeout_us) return SPI_ERR_INVALID_ARGUMENT;
  const Pressure pr = resolve_pressure(*c, *p);
  const int limit = std::max(1, c->batch_limit);
  const int min_limit = std::clamp(c->min_batch_limit, 1, limit);
  if (c->kind == SPI_BATCHING_DISABLED) {
    *out_target = 1;
    *out_timeout_us = 0;
    return SPI_OK;
  }
  if (c->kind == SPI_BATCHING_FIXED) {
    *out_target = limit;
    *out_timeout_us = std::max(0, c->coalesce_timeout_us);
    return SPI_OK;
  }
  if (limit <= min_limit) {
    st->target = min_limit;
    st->initialized = 1;
    st->low_streak = 0;
    *out_target = min_limit;
    *out_timeout_us = coalesce_timeout(*c, pr.congested, min_limit);
    return SPI_OK;
  }
  if (!c->congestion_enabled) {
    st->low_streak = 0;
    *out_target = limit;
    *out_timeout_us = std::max(0, c->coalesce_timeout_us);
    return SPI_OK;
  }
  if (!st->initialized) {
    st->target = limit;
    st->initialized = 1;
  }
  // update_target_batch_limit
  st->target = std::clamp(st->target, min_limit, limit);
  bool refresh = true;
  const int64_t tick_ns = (int64_t)std::max(1, c->tick_interval_us) * 1000;
  if (st->has_marker && now - st->last_update_ns < tick_ns) refresh = false;
  if (refresh) {
    st->has_marker = 1;
    st->last_update_ns = now;
    if (pr.congested) {
      st->target = limit;
      st->low_streak = 0;
    } else if (pr.high) {
      st->low_streak = 0;
      st->target = std::min(limit, st->target + high_step(*c, limit, pr.severe));
    } else if (pr.low) {
      if (st->low_streak < INT_MAX) ++st->low_streak;
      if (st->low_streak >= low_streak_threshold(*c)) {
        st->target = std::max(min_limit, st->target - 1);
        st->low_streak = 0;
      }
    } else {
      st->low_streak = 0;
    }
  }
  const int target = std::clamp(st->target, 1, limit);
  *out_target = target;
  *out_timeout_us = coalesce_timeout(*c, pr.congested, target);
  return SPI_OK;
}
