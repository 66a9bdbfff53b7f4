// The runtime's queued work: one eager shared queue in priority order, one deque of pinned jobs
// per worker, and the rule that composes a task's jobs from them.  Everything here is guarded by
// the runtime's mutex: every method is called with it held, except configure (before the workers
// start) and priority_of (reads what configure set).  Plain C++17, no HIP header;
// runtime_check.cpp checks the composition rule without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <deque>
#include <map>
#include <utility>
#include <vector>

#include "../../include/spi_runtime.h"

namespace spi {

struct Job {
  int32_t request_id;
  int32_t fixed_worker;
  int32_t priority;
  int64_t batch;
  std::vector<const void*> in;
  std::vector<void*> out;
  spi_job_done_fn done;
  void* user;
  int64_t submit_ns;
  int64_t dequeue_ns = 0;
};

using QueueKey = std::pair<int64_t, uint64_t>;  // (-priority, submission sequence)

class JobQueue {
 public:
  // max_queue 0 = unbounded; the priorities are the scheduler's range (0 / 0 with eager)
  void configure(int workers, int64_t max_queue, int32_t min_priority, int32_t max_priority) {
    fixed_.assign((size_t)workers, {});
    max_queue_ = max_queue;
    min_priority_ = min_priority;
    max_priority_ = max_priority;
  }

  // The job's own priority if it has one, else InferenceTask::create_task's:
  // priority = max(min_prio, max_prio - request_id)
  int32_t priority_of(const spi_job_desc& d) const {
    return d.has_priority ? d.priority
                          : (int32_t)std::max<int64_t>(min_priority_, (int64_t)max_priority_ - d.request_id);
  }

  // Queues the job on its pinned worker (fixed_worker >= 0) or in the shared queue, FIFO within
  // a priority.  SPI_ERR_QUEUE_FULL while the shared queue holds max_queue jobs: pinned jobs do
  // not count towards the bound but are rejected with the rest.
  int push(Job&& j) {
    if (max_queue_ > 0 && (int64_t)shared_.size() >= max_queue_) return SPI_ERR_QUEUE_FULL;
    if (j.fixed_worker >= 0) {
      fixed_[(size_t)j.fixed_worker].push_back(std::move(j));
    } else {
      const QueueKey key{-(int64_t)j.priority, seq_++};
      shared_.emplace(key, std::move(j));
    }
    return SPI_OK;
  }

  size_t shared_size() const { return shared_.size(); }
  // jobs `worker` may take: the shared queue and its own pinned ones
  size_t queued_for(int worker) const { return shared_.size() + fixed_[(size_t)worker].size(); }

  // Batch composition: the worker's pinned jobs first, then the shared queue's head in priority
  // order, while the samples fit the target and the task has fewer than max_jobs jobs.  A head
  // that does not fit ends the walk: no job is taken past it.
  void take(int worker, int target, int max_jobs, std::vector<Job>& jobs, int64_t& total) {
    std::deque<Job>& fixed = fixed_[(size_t)worker];
    while ((int)jobs.size() < max_jobs && !fixed.empty() && total + fixed.front().batch <= target) {
      total += fixed.front().batch;
      jobs.push_back(std::move(fixed.front()));
      fixed.pop_front();
    }
    while ((int)jobs.size() < max_jobs && !shared_.empty() && total + shared_.begin()->second.batch <= target) {
      total += shared_.begin()->second.batch;
      jobs.push_back(std::move(shared_.begin()->second));
      shared_.erase(shared_.begin());
    }
  }

  // The head alone, whatever its size (it exceeds an adaptive target): the worker's pinned front
  // if it has one, else the shared head.  queued_for(worker) must be > 0.
  void take_head(int worker, std::vector<Job>& jobs, int64_t& total) {
    std::deque<Job>& fixed = fixed_[(size_t)worker];
    if (!fixed.empty()) {
      jobs.push_back(std::move(fixed.front()));
      fixed.pop_front();
    } else {
      jobs.push_back(std::move(shared_.begin()->second));
      shared_.erase(shared_.begin());
    }
    total = jobs.back().batch;
  }

 private:
  std::map<QueueKey, Job> shared_;
  std::vector<std::deque<Job>> fixed_;  // [worker]
  uint64_t seq_ = 0;
  int64_t max_queue_ = 0;
  int32_t min_priority_ = 0, max_priority_ = 0;
};

}  // namespace spi
