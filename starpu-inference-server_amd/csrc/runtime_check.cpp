// Stand-alone check of the mini-runtime's host-only parts (make runtime_check): the copy pool, the
// job queue and its batch composition, the configuration resolver, the batching strategy and the
// load generator's statistics.  Built twice, with the address + undefined-behaviour sanitizers
// and with the thread sanitizer, no HIP; argv[1] labels the build in the output.  Prints one
// "<label> <group> ok" line per case group and exits non-zero on any mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "batching.hpp"
#include "copy_pool.hpp"
#include "job_queue.hpp"
#include "loadgen_stats.hpp"
#include "runtime_config.hpp"

using namespace spi;

// the one symbol the host-only files take from the codelet library (codelet.cpp's table)
extern "C" size_t spi_dtype_size(int32_t dtype) {
  switch (dtype) {
    case SPI_DTYPE_U8:
    case SPI_DTYPE_I8:
    case SPI_DTYPE_BOOL:
      return 1;
    case SPI_DTYPE_I16:
    case SPI_DTYPE_F16:
    case SPI_DTYPE_BF16:
      return 2;
    case SPI_DTYPE_I32:
    case SPI_DTYPE_F32:
      return 4;
    case SPI_DTYPE_I64:
    case SPI_DTYPE_F64:
      return 8;
    default:
      return 0;
  }
}

static int g_bad = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++g_bad;                                                           \
    }                                                                    \
  } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-9 * std::max(1.0, std::fabs(b)); }

// ---------------------------------------------------------------------------------------------
static std::vector<char> pattern(size_t n, unsigned seed) {
  std::vector<char> v(n);
  unsigned x = seed * 2654435761u + 1u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    v[i] = (char)(x >> 24);
  }
  return v;
}

static void check_copy_pool() {
  constexpr size_t MiB = 1 << 20;
  {
    // two callers on 3 helpers: multi-chunk copies, each caller draining the other's chunks too
    CopyPool pool(3);
    bool same[2] = {false, false};
    auto caller = [&](int k, size_t bytes) {
      const std::vector<char> src = pattern(bytes, 7 + k);
      bool ok = true;
      for (int it = 0; it < 20; ++it) {
        std::vector<char> dst(bytes, 0);
        pool.copy({CopyPool::Chunk{dst.data(), src.data(), bytes, nullptr}});
        ok = ok && dst == src;
      }
      same[k] = ok;
    };
    std::thread a(caller, 0, 5 * MiB), b(caller, 1, 3 * MiB);
    a.join();
    b.join();
    CHECK(same[0] && same[1]);
    // one call, several ops of uneven sizes
    const size_t sizes[] = {0, 1, MiB, MiB + 1, 3 * MiB + 17, 12345};
    std::vector<std::vector<char>> src, dst;
    std::vector<CopyPool::Chunk> ops;
    for (size_t n : sizes) {
      src.push_back(pattern(n, (unsigned)n));
      dst.emplace_back(n, 0);
    }
    for (size_t i = 0; i < src.size(); ++i) ops.push_back(CopyPool::Chunk{dst[i].data(), src[i].data(), sizes[i], nullptr});
    pool.copy(ops);
    for (size_t i = 0; i < src.size(); ++i) CHECK(dst[i] == src[i]);
    pool.copy({});  // nothing to do
  }
  {
    CopyPool inline_pool(0);  // no helpers: the caller copies inline
    const std::vector<char> src = pattern(2 * MiB + 3, 3);
    std::vector<char> dst(src.size(), 0);
    inline_pool.copy({CopyPool::Chunk{dst.data(), src.data(), src.size(), nullptr}});
    CHECK(dst == src);
  }
  {
    CopyPool idle(3);  // destroyed with an idle queue
  }
}

// ---------------------------------------------------------------------------------------------
static Job job(int32_t id, int64_t batch, int32_t priority = 0, int32_t fixed_worker = -1) {
  Job j{};
  j.request_id = id;
  j.fixed_worker = fixed_worker;
  j.priority = priority;
  j.batch = batch;
  return j;
}

static std::vector<int> ids(const std::vector<Job>& jobs) {
  std::vector<int> v;
  for (const Job& j : jobs) v.push_back(j.request_id);
  return v;
}

static void check_job_queue() {
  enum { F = 100, A, B, C, X, Y };
  {  // pinned first, then the shared queue by priority, while the samples fit
    JobQueue q;
    q.configure(2, 0, 0, 0);
    CHECK(q.push(job(A, 3, 0)) == SPI_OK && q.push(job(B, 2, 5)) == SPI_OK && q.push(job(C, 4, 0)) == SPI_OK);
    CHECK(q.push(job(F, 2, 0, 1)) == SPI_OK);
    CHECK(q.shared_size() == 3 && q.queued_for(1) == 4 && q.queued_for(0) == 3);
    std::vector<Job> jobs;
    int64_t total = 0;
    q.take(1, 8, INT32_MAX, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{F, B, A}) && total == 7);
    CHECK(q.shared_size() == 1 && q.queued_for(1) == 1);
    jobs.clear(), total = 0;
    q.take(0, 8, INT32_MAX, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{C}) && total == 4 && q.queued_for(0) == 0);
  }
  {  // a head that does not fit is not skipped
    JobQueue q;
    q.configure(1, 0, 0, 0);
    q.push(job(X, 6)), q.push(job(Y, 1)), q.push(job(F, 2, 0, 0));
    std::vector<Job> jobs;
    int64_t total = 0;
    q.take(0, 6, INT32_MAX, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{F}) && total == 2 && q.shared_size() == 2);
  }
  {  // the head alone when it exceeds the target: the shared head, or the pinned front if any
    JobQueue q;
    q.configure(1, 0, 0, 0);
    q.push(job(X, 4));
    std::vector<Job> jobs;
    int64_t total = 0;
    q.take(0, 2, INT32_MAX, jobs, total);
    CHECK(jobs.empty() && total == 0);
    q.take_head(0, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{X}) && total == 4 && q.queued_for(0) == 0);
    q.push(job(X, 4)), q.push(job(F, 3, 0, 0));
    jobs.clear(), total = 0;
    q.take(0, 2, INT32_MAX, jobs, total);
    CHECK(jobs.empty());
    q.take_head(0, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{F}) && total == 3 && q.shared_size() == 1);
  }
  {  // max_jobs 1; equal priorities leave in submission order
    JobQueue q;
    q.configure(1, 0, 0, 0);
    for (int i = 0; i < 4; ++i) q.push(job(i, 1, 3));
    std::vector<Job> jobs;
    int64_t total = 0;
    q.take(0, 8, 1, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{0}) && total == 1);
    q.take(0, 8, INT32_MAX, jobs, total);
    CHECK((ids(jobs) == std::vector<int>{0, 1, 2, 3}) && total == 4);
  }
  {  // priorities
    JobQueue q;
    q.configure(1, 0, 0, 10);
    spi_job_desc d{};
    d.request_id = 3;
    CHECK(q.priority_of(d) == 7);
    d.request_id = 50;
    CHECK(q.priority_of(d) == 0);
    d.has_priority = 1, d.priority = -4;
    CHECK(q.priority_of(d) == -4);
  }
  {  // max_queue counts the shared queue and rejects pinned jobs with the rest
    JobQueue q;
    q.configure(1, 2, 0, 0);
    CHECK(q.push(job(F, 1, 0, 0)) == SPI_OK);  // pinned: not counted
    CHECK(q.push(job(A, 1)) == SPI_OK && q.push(job(B, 1)) == SPI_OK);
    CHECK(q.push(job(C, 1)) == SPI_ERR_QUEUE_FULL);
    CHECK(q.push(job(F, 1, 0, 0)) == SPI_ERR_QUEUE_FULL);
    CHECK(q.shared_size() == 2 && q.queued_for(0) == 3);
  }
}

// ---------------------------------------------------------------------------------------------
static spi_model* const kReplica = reinterpret_cast<spi_model*>(uintptr_t{0x10});  // never dereferenced

// one device, one fp32 [3,224,224] input and one int64 [128] input, one fp32 output of 1000
static spi_runtime_config base_config() {
  spi_runtime_config c;
  spi_runtime_config_init(&c);
  c.num_devices = 1;
  c.device_ids[0] = 5;
  c.models[0] = kReplica;
  c.max_batch = 8;
  c.num_inputs = 2;
  c.input_types[0] = SPI_DTYPE_F32;
  c.input_ndims[0] = 3;
  c.input_dims[0][0] = 3, c.input_dims[0][1] = 224, c.input_dims[0][2] = 224;
  c.input_types[1] = SPI_DTYPE_I64;
  c.input_ndims[1] = 1;
  c.input_dims[1][0] = 128;
  c.num_outputs = 1;
  c.output_types[0] = SPI_DTYPE_F32;
  c.output_elems[0] = 1000;
  c.h2d_mode = SPI_H2D_WORKER_STREAM;
  return c;
}

static std::string resolve(const spi_runtime_config& c, ResolvedConfig& out, double gflop = 0.0, bool agents = false) {
  return resolve_runtime_config(&c, gflop, agents, out);
}

static int auto_mode(size_t input_bytes, double gflop, bool agents, int workers) {
  spi_runtime_config c = base_config();
  c.h2d_mode = SPI_H2D_AUTO;
  c.max_batch = 1;
  c.num_inputs = 1;
  c.input_types[0] = SPI_DTYPE_U8;
  c.input_ndims[0] = 1;
  c.input_dims[0][0] = (int64_t)input_bytes;
  c.workers_per_device = workers;
  ResolvedConfig r;
  CHECK(resolve(c, r, gflop, agents).empty());
  return r.cfg.h2d_mode;
}

static std::vector<int> warm_list(int max_batch, int warmup_batches) {
  spi_runtime_config c = base_config();
  c.max_batch = max_batch;
  c.warmup_batches = warmup_batches;
  ResolvedConfig r;
  CHECK(resolve(c, r).empty());
  return r.warmup;
}

static void check_runtime_config() {
  {  // spi_runtime_config_init and a zeroed struct resolve to the same defaults
    spi_runtime_config c = base_config();
    CHECK(c.workers_per_device == 4 && c.pipeline_depth == 2 && c.copy_threads == 4 && c.coalesce_max_jobs == 1);
    c.workers_per_device = c.pipeline_depth = c.copy_threads = 0;
    c.batching.batch_limit = 64;
    ResolvedConfig r;
    CHECK(resolve(c, r).empty());
    CHECK(r.cfg.workers_per_device == 4 && r.cfg.pipeline_depth == 2 && r.cfg.copy_threads == 4);
    CHECK(r.cfg.slots_per_device == 8 && r.cfg.batching.batch_limit == 8 && r.cfg.h2d_mode == SPI_H2D_WORKER_STREAM);
    CHECK((r.in_sample_bytes == std::vector<size_t>{602112, 1024}) && (r.out_sample_bytes == std::vector<size_t>{4000}));
    c.workers_per_device = 1, c.pipeline_depth = 1, c.batching.batch_limit = 3, c.slots_per_device = 0;
    CHECK(resolve(c, r).empty());
    CHECK(r.cfg.slots_per_device == 2 && r.cfg.batching.batch_limit == 3);
    c.slots_per_device = 5;
    CHECK(resolve(c, r).empty() && r.cfg.slots_per_device == 5);
  }
  {  // SPI_H2D_AUTO: SDMA from 120 KiB of task input per GFLOP, with agents; else by the worker count
    const size_t edge = 120 * 1024;
    CHECK(auto_mode(edge, 1.0, true, 4) == SPI_H2D_WORKER_SDMA);
    CHECK(auto_mode(edge - 1, 1.0, true, 4) == SPI_H2D_WORKER_STREAM);
    CHECK(auto_mode(edge, 1.0, false, 4) == SPI_H2D_WORKER_STREAM);
    CHECK(auto_mode(edge, 0.0, true, 4) == SPI_H2D_WORKER_STREAM);
    CHECK(auto_mode(edge - 1, 1.0, true, 3) == SPI_H2D_DEVICE_STREAM);
    CHECK(auto_mode(edge, 1.0, true, 3) == SPI_H2D_WORKER_SDMA);
  }
  CHECK((warm_list(8, -1) == std::vector<int>{8}));
  CHECK((warm_list(8, 0) == std::vector<int>{1, 2, 3, 4, 5, 6, 7, 8}));
  CHECK((warm_list(8, 3) == std::vector<int>{1, 2, 3, 8}));
  CHECK((warm_list(8, 20) == std::vector<int>{1, 2, 3, 4, 5, 6, 7, 8}));
  {  // rejected configurations keep their messages, and their order
    ResolvedConfig r;
    CHECK(resolve_runtime_config(nullptr, 0.0, false, r) == "invalid runtime configuration");
    spi_runtime_config c = base_config();
    c.num_devices = 0;
    CHECK(resolve(c, r) == "invalid runtime configuration");
    c = base_config(), c.num_inputs = SPI_MAX_INPUTS + 1;
    CHECK(resolve(c, r) == "invalid runtime configuration");
    c = base_config(), c.h2d_mode = SPI_H2D_WORKER_SDMA + 1;
    CHECK(resolve(c, r) == "invalid runtime configuration");
    c = base_config(), c.batching.kind = SPI_BATCHING_ADAPTIVE + 1;
    CHECK(resolve(c, r) == "invalid runtime configuration");
    c = base_config(), c.input_types[1] = 9;
    CHECK(resolve(c, r) == "invalid input spec");
    c = base_config(), c.output_elems[0] = 0;
    CHECK(resolve(c, r) == "invalid output spec");
    c = base_config(), c.models[0] = nullptr;
    CHECK(resolve(c, r) == "missing replica for device 5");
    c.output_elems[0] = 0;  // an invalid spec fails before the missing replica
    CHECK(resolve(c, r) == "invalid output spec");
  }
  {  // the hardware-queue warning: streams + 1 queues wanted
    spi_runtime_config c = base_config();
    ResolvedConfig r;
    setenv("GPU_MAX_HW_QUEUES", "5", 1);
    CHECK(resolve(c, r).empty() && r.queue_warning.empty());
    c.h2d_mode = SPI_H2D_DEVICE_STREAM;
    CHECK(resolve(c, r).empty());
    CHECK(r.queue_warning ==
          "spi_runtime: GPU_MAX_HW_QUEUES=5 < 5 streams + 1; streams will share hardware queues and serialize (set it "
          "before the first HIP call)\n");
    unsetenv("GPU_MAX_HW_QUEUES");
  }
}

// ---------------------------------------------------------------------------------------------
// tests/test_batching.py's harness: tick 10, entry horizon 40, exit horizon 30, fill 0.80 / 0.60
static spi_batching_config adaptive(int limit, int timeout = 0) {
  spi_batching_config c{};
  c.kind = SPI_BATCHING_ADAPTIVE;
  c.min_batch_limit = 1;
  c.batch_limit = limit;
  c.coalesce_timeout_us = timeout;
  c.congestion_enabled = 1;
  c.tick_interval_us = 10;
  c.entry_horizon_us = 40;
  c.exit_horizon_us = 30;
  c.fill_high = 0.80;
  c.fill_low = 0.60;
  return c;
}

static void check_batching() {
  const int64_t now = 1000000000000LL;
  int32_t target = 0, timeout = 0;
  {  // test_expands_on_high_pressure
    spi_batching_state s{};
    s.target = 1, s.initialized = 1, s.low_streak = 5;
    spi_batching_config c = adaptive(4);
    spi_batching_pressure p{};
    p.prepared_depth = 4;
    CHECK(spi_batching_decide(&s, &c, &p, now, &target, &timeout) == SPI_OK);
    CHECK(target == 2 && s.target == 2 && s.low_streak == 0);
  }
  {  // test_inflight_pressure_and_congested_timeout, second half
    spi_batching_state s{};
    s.target = 2, s.initialized = 1;
    spi_batching_config c = adaptive(8);
    spi_batching_pressure p{};
    p.congested = 1;
    CHECK(spi_batching_decide(&s, &c, &p, now, &target, &timeout) == SPI_OK);
    CHECK(target == 8 && timeout == 1);
  }
  {  // test_fixed_and_disabled_kinds
    spi_batching_state s{};
    spi_batching_config c{};
    c.kind = SPI_BATCHING_FIXED, c.batch_limit = 8, c.coalesce_timeout_us = 300;
    spi_batching_pressure p{};
    CHECK(spi_batching_decide(&s, &c, &p, now, &target, &timeout) == SPI_OK && target == 8 && timeout == 300);
    c.kind = SPI_BATCHING_DISABLED;
    CHECK(spi_batching_decide(&s, &c, &p, now, &target, &timeout) == SPI_OK && target == 1 && timeout == 0);
    CHECK(spi_batching_decide(nullptr, &c, &p, now, &target, &timeout) == SPI_ERR_INVALID_ARGUMENT);
  }
}

// ---------------------------------------------------------------------------------------------
static LoadgenRecord record(int32_t status, int64_t submit, int64_t dequeue, int64_t cstart, int64_t complete,
                            int32_t jobs, int32_t batch) {
  LoadgenRecord r;
  r.status = status, r.submit = submit, r.dequeue = dequeue, r.cstart = cstart, r.complete = complete;
  r.jobs = jobs, r.batch = batch;
  return r;
}

static void check_loadgen_stats() {
  const std::vector<double> xs{10, 20, 30, 40};
  CHECK(near(pct(xs, 50), 25.0) && near(pct(xs, 95), 38.5) && near(pct(xs, 99), 39.7));
  CHECK(std::isnan(pct({}, 50)) && pct({7.5}, 99) == 7.5);
  {
    const std::vector<LoadgenRecord> recs{
        record(SPI_OK, 1000000, 1100000, 1200000, 3000000, 2, 4),  // 2 ms
        record(SPI_ERR_QUEUE_FULL, 1500000, 0, 0, 0, 0, 0),        // rejected: skipped
        record(SPI_ERR_DEVICE, 500000, 600000, 700000, 9000000, 1, 1),  // failed: counted, not timed
        record(SPI_OK, 2000000, 2000000, 2500000, 7000000, 1, 2),  // 5 ms, the slowest
        record(SPI_OK, 4000000, 4200000, 4400000, 5000000, 3, 6),  // 1 ms
    };
    spi_loadgen_result res{};
    loadgen_reduce(recs, 2, 1, &res);
    CHECK(res.completed == 3 && res.failed == 1 && res.rejected == 1 && res.inferences == 6);
    CHECK(near(res.seconds, 0.006) && near(res.inferences_per_s, 1000.0));
    CHECK(near(res.mean_ms, 8.0 / 3.0) && near(res.max_ms, 5.0) && near(res.p50_ms, 2.0));
    CHECK(near(res.p99_ms, 2.0 + 3.0 * 0.98) && near(res.p95_ms, 2.0 + 3.0 * 0.9));
    CHECK(near(res.mean_jobs_per_task, 2.0) && near(res.mean_task_batch, 4.0));
    CHECK(near(res.worst_at_frac, 1.0 / 6.0));
    CHECK(near(res.p50_queue_ms, 0.1) && near(res.p50_stage_ms, 0.2) && near(res.p50_device_ms, 1.8));
  }
  {  // no completion at all
    const std::vector<LoadgenRecord> recs{record(SPI_ERR_QUEUE_FULL, 1, 0, 0, 0, 0, 0),
                                          record(SPI_ERR_DEVICE, 2, 3, 4, 5, 1, 1), LoadgenRecord{}};
    spi_loadgen_result res{};
    loadgen_reduce(recs, 4, 1, &res);
    CHECK(res.completed == 0 && res.failed == 2 && res.rejected == 1 && res.inferences == 0);
    CHECK(res.seconds == 0.0 && res.inferences_per_s == 0.0 && std::isnan(res.mean_ms) && std::isnan(res.p50_ms));
    CHECK(res.max_ms == 0.0 && res.mean_jobs_per_task == 0.0 && res.worst_at_frac == 0.0);
  }
}

int main(int argc, char** argv) {
  const char* label = argc > 1 ? argv[1] : "plain";
  struct Group {
    const char* name;
    void (*run)();
  };
  const Group groups[] = {{"copy_pool", check_copy_pool},
                          {"job_queue", check_job_queue},
                          {"runtime_config", check_runtime_config},
                          {"batching", check_batching},
                          {"loadgen_stats", check_loadgen_stats}};
  for (const Group& g : groups) {
    const int before = g_bad;
    g.run();
    std::printf("runtime_check %s %s %s\n", label, g.name, g_bad == before ? "ok" : "FAILED");
  }
  return g_bad ? 1 : 0;
}
