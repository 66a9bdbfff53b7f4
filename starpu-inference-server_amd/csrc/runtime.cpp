// Mini-runtime around spi_hip_inference_func (include/spi_runtime.h): per-device workers with a
// pipeline of tasks in flight, per-device pinned slot pools, H2D on a copy stream joined by
// events or on the SDMA engines, D2H and completion.  The host-only parts live beside it:
// batching.cpp (strategy), job_queue.hpp (queues and batch composition), copy_pool.hpp (host
// staging), runtime_config.cpp (validation and defaults); sdma_copy.cpp holds the HSA calls and
// loadgen.cpp the client load generator.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "copy_pool.hpp"
#include "job_queue.hpp"
#include "runtime_config.hpp"
#include "runtime_internal.hpp"
#include "sdma_copy.hpp"

extern "C" void spi_set_last_error(const char* msg);

using namespace spi;

namespace {

// One slot: pinned host staging for inputs/outputs and their HBM buffers.
struct Slot {
  std::vector<void*> h_in, h_out, d_in, d_out;
  hipEvent_t h2d = nullptr, done = nullptr;
  // SPI_H2D_WORKER_SDMA: completion signal of this slot's SDMA copies (value = copies in flight)
  SdmaSignal sig;
};

// SlotPoolBase::acquire / try_acquire / release (slot_pool_base.hpp:32-75).
struct SlotPool {
  int device = 0;
  std::vector<Slot> slots;
  std::vector<int> free_list;
  std::mutex mu;
  std::condition_variable cv;
  hipStream_t copy_stream = nullptr;  // SPI_H2D_DEVICE_STREAM
  SdmaAgents agents;                  // SPI_H2D_WORKER_SDMA

  int acquire() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !free_list.empty(); });
    const int s = free_list.back();
    free_list.pop_back();
    return s;
  }
  int try_acquire() {
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.empty()) return -1;
    const int s = free_list.back();
    free_list.pop_back();
    return s;
  }
  void release(int s) {
    {
      std::lock_guard<std::mutex> lk(mu);
      free_list.push_back(s);
    }
    cv.notify_one();
  }
};

struct Task {
  std::vector<Job> jobs;
  std::vector<int64_t> offs;
  int64_t total = 0;
  int slot = -1;
  int status = SPI_OK;
  std::string err;
  int64_t cs = 0, ce = 0;

  void fail(int s, const char* m) {
    status = s;
    err = m;
  }
};

struct Worker {
  int32_t worker_id = 0;  // also its index in the runtime's workers and in the job queue
  int32_t device = 0;
  int pool = 0;  // index into the runtime's pools
  spi_model* model = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // H2D stream (may be the pool's shared one)
  bool own_copy_stream = false;
  std::deque<Task> inflight;
  std::thread thread;
  // where the worker thread's time goes (spi_runtime_worker_times): tasks, slot wait,
  // host staging, H2D + codelet + D2H enqueue, completion-event wait (ns)
  std::atomic<int64_t> t_tasks{0}, t_slot{0}, t_stage{0}, t_enqueue{0}, t_event{0};
};

// A pinned host buffer and its HBM twin, appended to a slot's lists (nullptr where it failed).
bool alloc_pair(size_t bytes, std::vector<void*>& host, std::vector<void*>& dev) {
  void *h = nullptr, *d = nullptr;
  bool ok = hipHostMalloc(&h, bytes, hipHostMallocPortable) == hipSuccess;
  host.push_back(h);
  ok = ok && hipMalloc(&d, bytes) == hipSuccess;
  dev.push_back(d);
  return ok;
}

// The SDMA side of SPI_H2D_AUTO (c not validated yet: an out-of-range device count is rejected
// by resolve_runtime_config whatever this returns).
bool every_device_has_hsa_agents(const spi_runtime_config& c) {
  SdmaAgents a;
  for (int dv = 0; dv < std::min(c.num_devices, SPI_MAX_REPLICAS); ++dv)
    if (!find_hsa_agents(c.device_ids[dv], a)) return false;
  return true;
}

}  // namespace

struct spi_runtime {
  spi_runtime_config cfg{};
  std::vector<size_t> in_sample_bytes, out_sample_bytes;
  std::vector<int> warmup;  // batch sizes of the per-worker warm-up
  std::vector<std::unique_ptr<SlotPool>> pools;
  std::vector<std::unique_ptr<Worker>> workers;
  std::unique_ptr<CopyPool> copier;
  // mu guards the queue and the fields down to last_target
  mutable std::mutex mu;
  std::condition_variable cv_job, cv_idle;
  JobQueue queue;
  int64_t inflight_jobs = 0;   // submitted, not completed
  int64_t inflight_tasks = 0;  // codelet calls enqueued, not finalized
  bool stop = false;
  bool congested = false;      // a submission was rejected since the last decision
  spi_batching_state bstate{};
  int32_t last_target = 0;
  double warmup_s = 0.0;  // spi_runtime_create's per-worker warm-up
  std::atomic<int64_t> completed{0}, failed{0};

  // spi_runtime_create's steps after the configuration: "" or the error message
  std::string add_pool(int dv);
  std::string add_workers(int dv);
  std::string warm_transfers();
  std::string warm_replicas();
  void destroy_resources();

  void run(Worker* w);
  bool compose(Worker* w, std::unique_lock<std::mutex>& lk, std::vector<Job>& jobs);
  void launch(Worker* w, std::vector<Job>&& jobs);
  void finalize_oldest(Worker* w);
  // launch's steps
  int acquire_slot(Worker* w);
  void stage(Task& t, Slot& slot);
  void enqueue_h2d(Worker* w, Task& t, Slot& slot);
  void call_codelet(Worker* w, Task& t, Slot& slot);
  void enqueue_d2h(Worker* w, Task& t, Slot& slot);
};

// Batch composition under the batching strategy (caller holds mu, and w has
// work): JobQueue::take's rule (merge_input_tensors needs equal per-sample
// shapes, which the runtime config fixes).
bool spi_runtime::compose(Worker* w, std::unique_lock<std::mutex>& lk, std::vector<Job>& jobs) {
  const spi_batching_config& bc = cfg.batching;
  int target = cfg.max_batch, max_jobs = 1, timeout_us = 0;
  if (bc.kind == SPI_BATCHING_ADAPTIVE) {
    spi_batching_pressure p{};
    p.queue_size = (int64_t)queue.shared_size();
    p.queue_capacity = cfg.max_queue;
    p.prepared_depth = 0;
    p.inflight_tasks = inflight_tasks;
    p.max_inflight_tasks = (int64_t)workers.size() * cfg.pipeline_depth;
    p.congested = congested ? 1 : 0;
    congested = false;
    spi_batching_decide(&bstate, &bc, &p, now_ns(), &target, &timeout_us);
    target = std::clamp(target, 1, cfg.max_batch);
    max_jobs = INT_MAX;
  } else if (bc.kind == SPI_BATCHING_FIXED) {
    max_jobs = std::max(1, cfg.coalesce_max_jobs);
    timeout_us = max_jobs > 1 ? cfg.coalesce_delay_us : 0;
  }
  last_target = target;
  int64_t total = 0;
  queue.take(w->worker_id, target, max_jobs, jobs, total);
  // the head alone exceeds an adaptive target: run it alone
  if (jobs.empty()) queue.take_head(w->worker_id, jobs, total);
  // Coalescing wait only when this worker has nothing in flight: with tasks in
  // flight the GPU is busy anyway and their completions must not be delayed.
  // idle_dispatch (this build's tuning): an idle worker does not wait at all -- on the
  // reference's CI workload the 10 ms coalescer held requests while the GPU sat idle
  // (p50 queue 8.25 of 11.2 ms); under load the queue fills while every worker is busy
  // and the next free worker takes a batch of it anyway.  The adaptive strategy's option only:
  // the FIXED kind keeps its coalesce_max_jobs / coalesce_delay_us merging.
  const bool idle_now = bc.idle_dispatch && bc.kind == SPI_BATCHING_ADAPTIVE;
  if (timeout_us > 0 && w->inflight.empty() && !idle_now) {
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(timeout_us);
    while (!stop && (int)jobs.size() < max_jobs && total < target) {
      if (cv_job.wait_until(lk, deadline) == std::cv_status::timeout) {
        queue.take(w->worker_id, target, max_jobs, jobs, total);
        break;
      }
      queue.take(w->worker_id, target, max_jobs, jobs, total);
    }
  }
  if (queue.shared_size() > 0) cv_job.notify_one();  // leftovers belong to another worker
  return !jobs.empty();
}

// A free slot: never block while this worker still holds finished work.
int spi_runtime::acquire_slot(Worker* w) {
  SlotPool& pool = *pools[w->pool];
  int s = pool.try_acquire();
  while (s < 0 && !w->inflight.empty()) {
    finalize_oldest(w);
    s = pool.try_acquire();
  }
  return s < 0 ? pool.acquire() : s;
}

// copy_job_inputs_to_slot: every job's samples at its row offset.
void spi_runtime::stage(Task& t, Slot& slot) {
  std::vector<CopyPool::Chunk> ops;
  for (const Job& j : t.jobs) {
    t.offs.push_back(t.total);
    for (int i = 0; i < cfg.num_inputs; ++i)
      ops.push_back(CopyPool::Chunk{static_cast<char*>(slot.h_in[i]) + t.total * in_sample_bytes[i],
                                    static_cast<const char*>(j.in[i]), (size_t)j.batch * in_sample_bytes[i],
                                    nullptr});
    t.total += j.batch;
  }
  copier->copy(ops);
}

// H2D into the slot's HBM buffers (StarPU's fetch of the R handles).
void spi_runtime::enqueue_h2d(Worker* w, Task& t, Slot& slot) {
  const int ni = cfg.num_inputs;
  if (cfg.h2d_mode == SPI_H2D_WORKER_SDMA) {
    // SDMA engine copies (HIP's own hipMemcpyAsync takes a shader copy kernel for a
    // share of these 4.8 MB copies, 256 workgroups for ~120 us each, competing with
    // the forwards: DESIGN.md 5.1); the slot's HBM buffers are free (the slot was
    // released after its last task's completion event), so is its signal
    const SdmaAgents& agents = pools[w->pool]->agents;
    sdma_expect(slot.sig, ni);
    for (int i = 0; i < ni; ++i)
      if (!sdma_h2d(agents, slot.d_in[i], slot.h_in[i], (size_t)t.total * in_sample_bytes[i], slot.sig)) {
        t.fail(SPI_ERR_DEVICE, "SDMA H2D copy failed");
        sdma_cancel(slot.sig, ni - i);
        break;
      }
    // The worker thread waits (round 4 measured the alternative -- the worker stream waiting on
    // the signal's value word with hipStreamWaitValue64 -- releasing 46-55 ms after the copy on
    // this stack, tools/sdma_streamwait.cpp).
    if (sdma_wait(slot.sig) < 0 && t.status == SPI_OK) t.fail(SPI_ERR_DEVICE, "SDMA H2D failed");
  } else {
    hipStream_t h2d = w->copy_stream ? w->copy_stream : w->stream;
    for (int i = 0; i < ni && t.status == SPI_OK; ++i)
      if (hipMemcpyAsync(slot.d_in[i], slot.h_in[i], (size_t)t.total * in_sample_bytes[i], hipMemcpyHostToDevice,
                         h2d) != hipSuccess)
        t.fail(SPI_ERR_DEVICE, "H2D copy failed");
    if (h2d != w->stream && t.status == SPI_OK &&
        (hipEventRecord(slot.h2d, h2d) != hipSuccess || hipStreamWaitEvent(w->stream, slot.h2d, 0) != hipSuccess))
      t.fail(SPI_ERR_DEVICE, "H2D event join failed");
  }
}

// The codelet over vector interfaces resized to this task's payload.
void spi_runtime::call_codelet(Worker* w, Task& t, Slot& slot) {
  if (t.status != SPI_OK) return;
  const int ni = cfg.num_inputs, no = cfg.num_outputs;
  spi_codelet_args args;
  spi_args_init(&args);
  args.num_inputs = ni;
  args.num_outputs = no;
  args.request_id = t.jobs.front().request_id;
  args.batch_size = t.total;
  for (int i = 0; i < ni; ++i) {
    args.num_dims[i] = cfg.input_ndims[i] + 1;
    args.dims[i][0] = t.total;
    for (int d = 0; d < cfg.input_ndims[i]; ++d) args.dims[i][d + 1] = cfg.input_dims[i][d];
    args.input_types[i] = cfg.input_types[i];
  }
  for (int i = 0; i < no; ++i) args.output_types[i] = cfg.output_types[i];
  args.num_replicas = 1;
  args.models_gpu[0] = w->model;
  args.num_device_ids = 1;
  args.device_ids[0] = w->device;
  spi_vector_interface ifaces[SPI_MAX_INPUTS + SPI_MAX_OUTPUTS];
  void* buffers[SPI_MAX_INPUTS + SPI_MAX_OUTPUTS];
  for (int i = 0; i < ni; ++i) {
    const size_t es = spi_dtype_size(cfg.input_types[i]);
    ifaces[i] = spi_vector_interface{SPI_STARPU_VECTOR_INTERFACE_ID, (uintptr_t)slot.d_in[i], 0, 0,
                                     t.total * in_sample_bytes[i] / es, es, 0,
                                     (size_t)cfg.max_batch * in_sample_bytes[i]};
    buffers[i] = &ifaces[i];
  }
  for (int i = 0; i < no; ++i) {
    const size_t es = spi_dtype_size(cfg.output_types[i]);
    ifaces[ni + i] = spi_vector_interface{SPI_STARPU_VECTOR_INTERFACE_ID, (uintptr_t)slot.d_out[i], 0, 0,
                                          t.total * out_sample_bytes[i] / es, es, 0,
                                          (size_t)cfg.max_batch * out_sample_bytes[i]};
    buffers[ni + i] = &ifaces[ni + i];
  }
  spi_hip_inference_func(buffers, &args);
  t.cs = args.codelet_start_ns;
  t.ce = args.codelet_end_ns;
  if (args.status != SPI_OK) t.fail(args.status, args.error);
}

// D2H on the worker stream and the task's completion event (recorded for a failed task too:
// finalize_oldest waits on it).
void spi_runtime::enqueue_d2h(Worker* w, Task& t, Slot& slot) {
  if (t.status == SPI_OK)
    for (int i = 0; i < cfg.num_outputs; ++i)
      if (hipMemcpyAsync(slot.h_out[i], slot.d_out[i], (size_t)t.total * out_sample_bytes[i],
                         hipMemcpyDeviceToHost, w->stream) != hipSuccess)
        t.fail(SPI_ERR_DEVICE, "D2H copy failed");
  if (hipEventRecord(slot.done, w->stream) != hipSuccess && t.status == SPI_OK)
    t.fail(SPI_ERR_DEVICE, "completion event failed");
}

void spi_runtime::launch(Worker* w, std::vector<Job>&& jobs) {
  Task t;
  t.jobs = std::move(jobs);
  const int64_t c0 = now_ns();
  t.slot = acquire_slot(w);
  Slot& slot = pools[w->pool]->slots[t.slot];
  const int64_t c1 = now_ns();
  stage(t, slot);
  const int64_t c2 = now_ns();
  enqueue_h2d(w, t, slot);
  call_codelet(w, t, slot);
  enqueue_d2h(w, t, slot);
  {
    std::lock_guard<std::mutex> lk(mu);
    ++inflight_tasks;
  }
  w->inflight.push_back(std::move(t));
  const int64_t c3 = now_ns();
  w->t_tasks += 1;
  w->t_slot += c1 - c0;
  w->t_stage += c2 - c1;
  w->t_enqueue += c3 - c2;
}

// starpu_output_callback: wait for the task's completion event, hand each job
// its rows of every output (slice_outputs_for_sub_job), run its callback,
// release the slot.
void spi_runtime::finalize_oldest(Worker* w) {
  Task t = std::move(w->inflight.front());
  w->inflight.pop_front();
  SlotPool& pool = *pools[w->pool];
  Slot& slot = pool.slots[t.slot];
  const int64_t e0 = now_ns();
  const hipError_t se = hipEventSynchronize(slot.done);
  if (se != hipSuccess && t.status == SPI_OK) t.fail(SPI_ERR_DEVICE, "stream synchronisation failed");
  w->t_event += now_ns() - e0;
  const int no = cfg.num_outputs;
  for (size_t k = 0; k < t.jobs.size(); ++k) {
    const Job& j = t.jobs[k];
    if (t.status == SPI_OK)
      for (int i = 0; i < no; ++i)
        std::memcpy(j.out[i], static_cast<const char*>(slot.h_out[i]) + t.offs[k] * out_sample_bytes[i],
                    (size_t)j.batch * out_sample_bytes[i]);
    spi_job_timing tm{};
    tm.submit_ns = j.submit_ns;
    tm.dequeue_ns = j.dequeue_ns;
    tm.codelet_start_ns = t.cs;
    tm.codelet_end_ns = t.ce;
    tm.device_id = w->device;
    tm.worker_id = w->worker_id;
    tm.task_batch = (int32_t)t.total;
    tm.task_jobs = (int32_t)t.jobs.size();
    tm.complete_ns = now_ns();
    (t.status == SPI_OK ? completed : failed).fetch_add(1);
    if (j.done) j.done(j.user, j.request_id, t.status, t.status == SPI_OK ? "" : t.err.c_str(), &tm);
  }
  pool.release(t.slot);
  {
    std::lock_guard<std::mutex> lk(mu);
    --inflight_tasks;
    inflight_jobs -= (int64_t)t.jobs.size();
    if (inflight_jobs == 0) cv_idle.notify_all();
  }
}

void spi_runtime::run(Worker* w) {
  (void)hipSetDevice(w->device);
  spi_set_worker_context(w->worker_id, w->device, w->stream);
  const size_t depth = (size_t)std::max(1, cfg.pipeline_depth);
  for (;;) {
    // deliver whatever already finished
    while (!w->inflight.empty() && hipEventQuery(pools[w->pool]->slots[w->inflight.front().slot].done) == hipSuccess)
      finalize_oldest(w);
    // a full pipeline takes no new work: jobs stay in the shared queue for
    // workers that can start them now (eager scheduling)
    if (w->inflight.size() >= depth) {
      finalize_oldest(w);
      continue;
    }
    std::vector<Job> jobs;
    bool quit = false;
    {
      std::unique_lock<std::mutex> lk(mu);
      cv_job.wait(lk, [&] { return stop || queue.queued_for(w->worker_id) > 0 || !w->inflight.empty(); });
      if (queue.queued_for(w->worker_id) > 0) {
        compose(w, lk, jobs);
        const int64_t t = now_ns();
        for (Job& j : jobs) j.dequeue_ns = t;
      } else if (stop && w->inflight.empty()) {
        quit = true;
      }
    }
    if (quit) break;
    if (jobs.empty()) {  // nothing new: wait for the oldest task in flight
      finalize_oldest(w);
      continue;
    }
    launch(w, std::move(jobs));
  }
  while (!w->inflight.empty()) finalize_oldest(w);
  spi_clear_worker_context();
}

// Device dv's slot pool: slots_per_device slots of max_batch samples, their events, and what
// the H2D mode needs (a shared copy stream, or the HSA agents and a signal per slot).
std::string spi_runtime::add_pool(int dv) {
  const std::string dev = std::to_string(cfg.device_ids[dv]);
  auto owned = std::make_unique<SlotPool>();
  owned->device = cfg.device_ids[dv];
  if (hipSetDevice(owned->device) != hipSuccess) return "hipSetDevice failed";
  pools.push_back(std::move(owned));  // from here on destroy_resources frees what it holds
  SlotPool& pool = *pools.back();
  pool.slots.resize(cfg.slots_per_device);
  bool ok = true;
  for (int s = 0; s < cfg.slots_per_device && ok; ++s) {
    Slot& sl = pool.slots[s];
    for (size_t b : in_sample_bytes) ok = ok && alloc_pair(b * cfg.max_batch, sl.h_in, sl.d_in);
    for (size_t b : out_sample_bytes) ok = ok && alloc_pair(b * cfg.max_batch, sl.h_out, sl.d_out);
    ok = ok && hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) == hipSuccess;
    pool.free_list.push_back(cfg.slots_per_device - 1 - s);
  }
  if (ok && cfg.h2d_mode == SPI_H2D_DEVICE_STREAM)
    ok = hipStreamCreateWithFlags(&pool.copy_stream, hipStreamNonBlocking) == hipSuccess;
  if (ok && cfg.h2d_mode == SPI_H2D_WORKER_SDMA) {
    if (!find_hsa_agents(pool.device, pool.agents)) return "no HSA agents for device " + dev;
    for (Slot& sl : pool.slots) ok = ok && sdma_signal_create(sl.sig);
  }
  return ok ? "" : "slot pool allocation failed on device " + dev;
}

// Device dv's workers: a stream each, and the H2D stream of the mode.
std::string spi_runtime::add_workers(int dv) {
  for (int k = 0; k < cfg.workers_per_device; ++k) {
    auto w = std::make_unique<Worker>();
    w->worker_id = (int32_t)workers.size();
    w->device = cfg.device_ids[dv];
    w->pool = dv;
    w->model = cfg.models[dv];
    bool ok = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) == hipSuccess;
    if (cfg.h2d_mode == SPI_H2D_DEVICE_STREAM) {
      w->copy_stream = pools[dv]->copy_stream;
    } else if (cfg.h2d_mode == SPI_H2D_WORKER_COPY) {
      ok = ok && hipStreamCreateWithFlags(&w->copy_stream, hipStreamNonBlocking) == hipSuccess;
      w->own_copy_stream = true;
    }
    workers.push_back(std::move(w));
    if (!ok) return "stream creation failed for worker " + std::to_string(workers.size() - 1);
  }
  return "";
}

// Every slot's transfer path exercised once before serving: the first SDMA copy from a
// pinned buffer (or the first copy on a stream) costs far more than the steady state --
// the first measured requests of a fresh runtime had shown 10-19 ms latencies beside a
// 3 ms p50 (tools/e2e_tail.py) -- so the copy engines, queues and mappings are set up now.
std::string spi_runtime::warm_transfers() {
  for (size_t dv = 0; dv < pools.size(); ++dv) {
    SlotPool& pl = *pools[dv];
    const std::string dev = std::to_string(pl.device);
    (void)hipSetDevice(pl.device);
    Worker* w0 = nullptr;
    for (auto& w : workers)
      if (w->pool == (int)dv) {
        w0 = w.get();
        break;
      }
    hipStream_t st = pl.copy_stream ? pl.copy_stream : w0->stream;
    for (Slot& sl : pl.slots) {
      for (size_t i = 0; i < sl.h_in.size(); ++i) {
        const size_t bytes = in_sample_bytes[i] * (size_t)cfg.max_batch;
        std::memset(sl.h_in[i], 0, bytes);
        if (cfg.h2d_mode == SPI_H2D_WORKER_SDMA) {
          sdma_expect(sl.sig, 1);
          if (!sdma_h2d(pl.agents, sl.d_in[i], sl.h_in[i], bytes, sl.sig) || sdma_wait(sl.sig) < 0)
            return "SDMA warm-up copy failed on device " + dev;
        } else if (hipMemcpyAsync(sl.d_in[i], sl.h_in[i], bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
          return "H2D warm-up copy failed on device " + dev;
        }
      }
      for (size_t i = 0; i < sl.h_out.size(); ++i)
        if (hipMemcpyAsync(sl.h_out[i], sl.d_out[i], out_sample_bytes[i] * (size_t)cfg.max_batch,
                           hipMemcpyDeviceToHost, w0->stream) != hipSuccess)
          return "D2H warm-up copy failed on device " + dev;
    }
    if (hipStreamSynchronize(st) != hipSuccess || hipStreamSynchronize(w0->stream) != hipSuccess)
      return "transfer warm-up failed on device " + dev;
  }
  return "";
}

// Per-worker warm-up before serving (the reference warms every worker through the
// pipeline, inference_runner.cpp:507-560): the workspace and the graph of every batch
// size the batchers can compose, so no capture (serialised process-wide) or workspace
// allocation ever lands on a live request.
std::string spi_runtime::warm_replicas() {
  const int64_t seq = cfg.input_ndims[0] >= 1 ? cfg.input_dims[0][0] : 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (auto& w : workers) {
    (void)hipSetDevice(w->device);
    for (int b : warmup)
      if (spi_model_warmup(w->model, w->stream, b, seq, cfg.num_inputs >= 2) != SPI_OK)
        return std::string("warm-up failed for worker ") + std::to_string(w->worker_id) + " batch " +
               std::to_string(b) + ": " + spi_last_error();
  }
  warmup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return "";
}

void spi_runtime::destroy_resources() {
  for (auto& w : workers) {
    (void)hipSetDevice(w->device);
    if (w->own_copy_stream && w->copy_stream) (void)hipStreamDestroy(w->copy_stream);
    if (w->stream) (void)hipStreamDestroy(w->stream);
  }
  for (auto& p : pools) {
    (void)hipSetDevice(p->device);
    for (Slot& s : p->slots) {
      for (void* x : s.h_in) (void)hipHostFree(x);
      for (void* x : s.h_out) (void)hipHostFree(x);
      for (void* x : s.d_in) (void)hipFree(x);
      for (void* x : s.d_out) (void)hipFree(x);
      if (s.h2d) (void)hipEventDestroy(s.h2d);
      if (s.done) (void)hipEventDestroy(s.done);
      sdma_signal_destroy(s.sig);
    }
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
  }
}

RuntimeShape spi::runtime_shape(const spi_runtime* rt) {
  return RuntimeShape{rt->cfg.max_batch, rt->cfg.num_outputs, &rt->out_sample_bytes};
}

extern "C" {

spi_runtime* spi_runtime_create(const spi_runtime_config* c, char* err, size_t errlen) {
  auto fail = [&](const std::string& m) -> spi_runtime* {
    spi_set_last_error(m.c_str());
    if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str());
    return nullptr;
  };
  // resolve the configuration; SPI_H2D_AUTO asks what the device side knows
  double gflop = 0.0;
  bool agents = false;
  if (c && c->h2d_mode == SPI_H2D_AUTO) {
    gflop = c->models[0] ? spi_model_flops(c->models[0], c->max_batch) * 1e-9 : 0.0;
    agents = every_device_has_hsa_agents(*c);
  }
  ResolvedConfig rc;
  const std::string bad = resolve_runtime_config(c, gflop, agents, rc);
  if (!rc.queue_warning.empty()) std::fputs(rc.queue_warning.c_str(), stderr);
  if (!bad.empty()) return fail(bad);
  auto rt = std::make_unique<spi_runtime>();
  rt->cfg = rc.cfg;
  rt->in_sample_bytes = std::move(rc.in_sample_bytes);
  rt->out_sample_bytes = std::move(rc.out_sample_bytes);
  rt->warmup = std::move(rc.warmup);
  const spi_runtime_config& cfg = rt->cfg;
  rt->queue.configure(cfg.num_devices * cfg.workers_per_device, cfg.max_queue, cfg.min_priority, cfg.max_priority);
  auto cleanup_fail = [&](const std::string& m) {
    rt->destroy_resources();
    return fail(m);
  };
  std::string e;
  for (int dv = 0; dv < cfg.num_devices; ++dv) {
    if (!(e = rt->add_pool(dv)).empty()) return cleanup_fail(e);
    if (!(e = rt->add_workers(dv)).empty()) return cleanup_fail(e);
  }
  if (!(e = rt->warm_transfers()).empty()) return cleanup_fail(e);
  if (!(e = rt->warm_replicas()).empty()) return cleanup_fail(e);
  rt->copier = std::make_unique<CopyPool>(cfg.copy_threads - 1);
  rt->last_target = cfg.max_batch;
  for (auto& w : rt->workers) w->thread = std::thread(&spi_runtime::run, rt.get(), w.get());
  return rt.release();
}

int spi_runtime_submit_job(spi_runtime* rt, const spi_job_desc* d) {
  if (!rt || !d || !d->inputs || !d->outputs || d->batch < 1 || d->batch > rt->cfg.max_batch)
    return SPI_ERR_INVALID_ARGUMENT;
  if (d->fixed_worker >= (int32_t)rt->workers.size()) return SPI_ERR_INVALID_ARGUMENT;
  Job j;
  j.request_id = d->request_id;
  j.fixed_worker = d->fixed_worker;
  j.priority = rt->queue.priority_of(*d);
  j.batch = d->batch;
  j.in.assign(d->inputs, d->inputs + rt->cfg.num_inputs);
  j.out.assign(d->outputs, d->outputs + rt->cfg.num_outputs);
  j.done = d->done;
  j.user = d->user;
  j.submit_ns = now_ns();
  {
    std::lock_guard<std::mutex> lk(rt->mu);
    if (rt->stop) return SPI_ERR_INVALID_ARGUMENT;
    if (rt->queue.push(std::move(j)) != SPI_OK) {
      rt->congested = true;
      return SPI_ERR_QUEUE_FULL;
    }
    ++rt->inflight_jobs;
  }
  if (d->fixed_worker >= 0)
    rt->cv_job.notify_all();  // the pinned worker must see it
  else
    rt->cv_job.notify_one();
  return SPI_OK;
}

int spi_runtime_submit(spi_runtime* rt, int32_t request_id, int64_t batch, const void* const* inputs,
                       void* const* outputs, spi_job_done_fn done, void* user) {
  spi_job_desc d{};
  d.request_id = request_id;
  d.fixed_worker = -1;
  d.batch = batch;
  d.inputs = inputs;
  d.outputs = outputs;
  d.done = done;
  d.user = user;
  return spi_runtime_submit_job(rt, &d);
}

int spi_runtime_drain(spi_runtime* rt) {
  if (!rt) return SPI_ERR_INVALID_ARGUMENT;
  std::unique_lock<std::mutex> lk(rt->mu);
  rt->cv_idle.wait(lk, [&] { return rt->inflight_jobs == 0; });
  return SPI_OK;
}

void spi_runtime_stats(const spi_runtime* rt, int64_t* completed, int64_t* failed) {
  if (completed) *completed = rt ? rt->completed.load() : 0;
  if (failed) *failed = rt ? rt->failed.load() : 0;
}

int32_t spi_runtime_num_workers(const spi_runtime* rt) { return rt ? (int32_t)rt->workers.size() : 0; }

int spi_runtime_worker_times(const spi_runtime* rt, int32_t worker, int64_t* out) {
  if (!rt || !out || worker < 0 || worker >= (int32_t)rt->workers.size()) return SPI_ERR_INVALID_ARGUMENT;
  const auto& w = *rt->workers[worker];
  out[0] = w.t_tasks.load();
  out[1] = w.t_slot.load();
  out[2] = w.t_stage.load();
  out[3] = w.t_enqueue.load();
  out[4] = w.t_event.load();
  return SPI_OK;
}

int32_t spi_runtime_h2d_mode(const spi_runtime* rt) { return rt ? rt->cfg.h2d_mode : -1; }

double spi_runtime_warmup_seconds(const spi_runtime* rt) { return rt ? rt->warmup_s : 0.0; }

int32_t spi_runtime_batch_target(const spi_runtime* rt) {
  if (!rt) return 0;
  std::lock_guard<std::mutex> lk(rt->mu);
  return rt->last_target;
}

void spi_runtime_destroy(spi_runtime* rt) {
  if (!rt) return;
  spi_runtime_drain(rt);
  {
    std::lock_guard<std::mutex> lk(rt->mu);
    rt->stop = true;
  }
  rt->cv_job.notify_all();
  for (auto& w : rt->workers)
    if (w->thread.joinable()) w->thread.join();
  rt->copier.reset();
  rt->destroy_resources();
  delete rt;
}

}  // extern "C"
