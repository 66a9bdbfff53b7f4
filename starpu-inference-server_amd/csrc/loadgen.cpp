// The client load generator (spi_runtime_loadgen, include/spi_runtime.h) on top of
// spi_runtime_submit / spi_runtime_drain; its statistics are loadgen_stats.hpp's.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "loadgen_stats.hpp"
#include "runtime_internal.hpp"

using namespace spi;

namespace {
struct LoadGen {
  struct Req : LoadgenRecord {
    int buf = -1;
    LoadGen* gen = nullptr;
  };
  std::vector<Req> reqs;
  std::vector<std::vector<std::vector<char>>> out_bufs;  // [buffer][output]
  std::vector<int> free_bufs;
  std::mutex mu;
  std::condition_variable cv;
  int64_t outstanding = 0;
  std::string first_err;

  static void done(void* user, int32_t, int32_t status, const char* error, const spi_job_timing* t) {
    Req* r = static_cast<Req*>(user);
    LoadGen* g = r->gen;
    r->complete = t->complete_ns;
    r->dequeue = t->dequeue_ns;
    r->cstart = t->codelet_start_ns;
    r->status = status;
    r->jobs = t->task_jobs;
    r->batch = t->task_batch;
    {
      std::lock_guard<std::mutex> lk(g->mu);
      if (status != SPI_OK && g->first_err.empty()) g->first_err = error ? error : "";
      g->free_bufs.push_back(r->buf);
      --g->outstanding;
    }
    g->cv.notify_all();
  }
};

void sleep_until_ns(int64_t t) {
  for (;;) {
    const int64_t now = now_ns();
    if (now >= t) return;
    const int64_t left = t - now;
    if (left > 200000) {
      timespec ts{0, (long)(left - 100000)};
      nanosleep(&ts, nullptr);
    } else {
      std::this_thread::yield();
    }
  }
}
}  // namespace

extern "C" int spi_runtime_loadgen(spi_runtime* rt, const spi_loadgen_config* c, const void* const* inputs,
                                   spi_loadgen_result* res) {
  if (!rt || !c || !inputs || !res) return SPI_ERR_INVALID_ARGUMENT;
  const RuntimeShape shape = runtime_shape(rt);
  if (c->request_batch < 1 || c->request_batch > shape.max_batch) return SPI_ERR_INVALID_ARGUMENT;
  std::memset(res, 0, sizeof(*res));
  const bool open = c->num_segments > 0;
  int64_t n = c->requests;
  if (open) {
    n = 0;
    for (int i = 0; i < c->num_segments; ++i) n += std::max<int64_t>(0, c->segments[i].repeat);
  }
  const int nbuf = std::max(1, open ? std::max(c->inflight, 256) : c->inflight);
  LoadGen g;
  g.out_bufs.resize(nbuf);
  for (auto& b : g.out_bufs)
    for (size_t bytes : *shape.out_sample_bytes) b.emplace_back(bytes * c->request_batch);
  for (int i = nbuf - 1; i >= 0; --i) g.free_bufs.push_back(i);
  auto submit = [&](LoadGen::Req& r, int32_t id) -> int {
    int buf;
    {
      std::unique_lock<std::mutex> lk(g.mu);
      g.cv.wait(lk, [&] { return !g.free_bufs.empty() && (open || g.outstanding < c->inflight); });
      buf = g.free_bufs.back();
      g.free_bufs.pop_back();
      ++g.outstanding;
    }
    r.buf = buf;
    r.gen = &g;
    void* outs[SPI_MAX_OUTPUTS];
    for (int i = 0; i < shape.num_outputs; ++i) outs[i] = g.out_bufs[buf][i].data();
    r.submit = now_ns();
    const int rc = spi_runtime_submit(rt, id, c->request_batch, inputs, outs, &LoadGen::done, &r);
    if (rc != SPI_OK) {
      std::lock_guard<std::mutex> lk(g.mu);
      g.free_bufs.push_back(buf);
      --g.outstanding;
    }
    return rc;
  };
  // warm-up (not measured)
  if (c->warmup_requests > 0) {
    std::vector<LoadGen::Req> warm(c->warmup_requests);
    for (int i = 0; i < c->warmup_requests; ++i)
      while (submit(warm[i], -1 - i) == SPI_ERR_QUEUE_FULL) std::this_thread::yield();
    spi_runtime_drain(rt);
  }
  g.reqs.resize(n);
  int64_t rejected = 0;
  if (!open) {
    for (int64_t i = 0; i < n; ++i) {
      int rc;
      while ((rc = submit(g.reqs[i], (int32_t)i)) == SPI_ERR_QUEUE_FULL) std::this_thread::yield();
      if (rc != SPI_OK) {
        std::snprintf(res->error, SPI_ERROR_LEN, "submit failed (%d)", rc);
        spi_runtime_drain(rt);
        return rc;
      }
    }
  } else {
    int64_t t = now_ns(), i = 0;
    for (int s = 0; s < c->num_segments; ++s)
      for (int64_t k = 0; k < c->segments[s].repeat; ++k, ++i) {
        t += c->segments[s].delta_us * 1000;
        sleep_until_ns(t);
        const int rc = submit(g.reqs[i], (int32_t)i);
        if (rc == SPI_ERR_QUEUE_FULL) {
          ++rejected;
          g.reqs[i].status = SPI_ERR_QUEUE_FULL;
        }
      }
  }
  spi_runtime_drain(rt);
  loadgen_reduce(g.reqs, c->request_batch, rejected, res);
  std::snprintf(res->error, SPI_ERROR_LEN, "%s", g.first_err.c_str());
  return res->failed ? SPI_ERR_DEVICE : SPI_OK;
}
