// The load generator's statistics: from the per-request records to spi_loadgen_result, with the
// reference client's percentile definition.  Plain C++17, no HIP header; runtime_check.cpp checks
// the figures without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/spi_runtime.h"

namespace spi {

// What the load generator keeps of one request: CLOCK_MONOTONIC stamps (ns) and the task that
// ran it.  status -1: never completed; SPI_ERR_QUEUE_FULL: rejected at submission.
struct LoadgenRecord {
  int64_t submit = 0, complete = 0, dequeue = 0, cstart = 0;
  int32_t status = -1, jobs = 0, batch = 0;
};

// Percentile p of the sorted xs by linear interpolation (latency_statistics.hpp:52-93).
inline double pct(const std::vector<double>& xs, double p) {
  if (xs.empty()) return NAN;
  if (xs.size() == 1) return xs[0];
  const double pos = p / 100.0 * (double)(xs.size() - 1);
  const size_t lo = (size_t)std::floor(pos), hi = std::min(lo + 1, xs.size() - 1);
  return xs[lo] + (xs[hi] - xs[lo]) * (pos - (double)lo);
}

// Fills every field of res but `error` (Rec: LoadgenRecord or a type derived from it).  Rejected
// requests are skipped, other failures only counted; the run's window is first submit -> last
// completion of the requests that succeeded.
template <class Rec>
void loadgen_reduce(const std::vector<Rec>& reqs, int64_t request_batch, int64_t rejected, spi_loadgen_result* res) {
  std::vector<double> lat, qlat, slat, dlat;
  int64_t first = INT64_MAX, last = 0, ok = 0, bad = 0, worst_submit = 0;
  double jobs = 0, batch = 0, sum = 0, mx = 0;
  for (const LoadgenRecord& r : reqs) {
    if (r.status == SPI_ERR_QUEUE_FULL) continue;
    if (r.status != SPI_OK) {
      ++bad;
      continue;
    }
    ++ok;
    first = std::min(first, r.submit);
    last = std::max(last, r.complete);
    const double ms = (r.complete - r.submit) * 1e-6;
    lat.push_back(ms);
    qlat.push_back((r.dequeue - r.submit) * 1e-6);
    slat.push_back((r.cstart - r.dequeue) * 1e-6);
    dlat.push_back((r.complete - r.cstart) * 1e-6);
    sum += ms;
    if (ms > mx) worst_submit = r.submit;
    mx = std::max(mx, ms);
    jobs += r.jobs;
    batch += r.batch;
  }
  std::sort(lat.begin(), lat.end());
  std::sort(qlat.begin(), qlat.end());
  std::sort(slat.begin(), slat.end());
  std::sort(dlat.begin(), dlat.end());
  res->completed = ok;
  res->failed = bad;
  res->rejected = rejected;
  res->inferences = ok * request_batch;
  res->seconds = ok ? (last - first) * 1e-9 : 0.0;
  res->inferences_per_s = res->seconds > 0 ? res->inferences / res->seconds : 0.0;
  res->p50_ms = pct(lat, 50);
  res->p95_ms = pct(lat, 95);
  res->p99_ms = pct(lat, 99);
  res->mean_ms = ok ? sum / ok : NAN;
  res->max_ms = mx;
  res->mean_jobs_per_task = ok ? jobs / ok : 0;
  res->mean_task_batch = ok ? batch / ok : 0;
  res->p50_queue_ms = pct(qlat, 50);
  res->p99_queue_ms = pct(qlat, 99);
  res->p50_stage_ms = pct(slat, 50);
  res->p99_stage_ms = pct(slat, 99);
  res->p50_device_ms = pct(dlat, 50);
  res->p99_device_ms = pct(dlat, 99);
  res->worst_at_frac = ok && last > first ? (double)(worst_submit - first) / (double)(last - first) : 0.0;
}

}  // namespace spi
