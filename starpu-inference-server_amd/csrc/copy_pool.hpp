// Host staging: a pool of copy threads shared by the runtime's workers.  A worker splits its
// copies into chunks, queues them, works on the queue itself and waits for its own chunks
// (parallel_for_each_index, slot_manager_component.cpp:56-95).  Plain C++17, no HIP header;
// runtime_check.cpp runs it under the thread and address sanitizers.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace spi {

class CopyPool {
 public:
  struct Batch {
    std::atomic<int> remaining{0};
  };
  struct Chunk {
    char* dst;
    const char* src;
    size_t bytes;
    Batch* batch;
  };

  explicit CopyPool(int helpers) {
    for (int i = 0; i < helpers; ++i) threads_.emplace_back([this] { loop(); });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }

  // Copies every (dst, src, bytes) and returns when all are done.
  void copy(const std::vector<Chunk>& ops) {
    constexpr size_t kChunk = 1 << 20;
    std::vector<Chunk> chunks;
    Batch batch;
    for (const Chunk& op : ops)
      for (size_t off = 0; off < op.bytes; off += kChunk)
        chunks.push_back(Chunk{op.dst + off, op.src + off, std::min(kChunk, op.bytes - off), &batch});
    if (chunks.empty()) return;
    if (threads_.empty() || chunks.size() == 1) {
      for (const Chunk& c : chunks) std::memcpy(c.dst, c.src, c.bytes);
      return;
    }
    batch.remaining.store((int)chunks.size());
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (const Chunk& c : chunks) q_.push_back(c);
    }
    cv_.notify_all();
    // help: drain the queue (any worker's chunks) until ours are all done
    while (batch.remaining.load(std::memory_order_acquire) > 0) {
      Chunk c{};
      bool got = false;
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (!q_.empty()) {
          c = q_.front();
          q_.pop_front();
          got = true;
        }
      }
      if (got) {
        run(c);
      } else {
        std::this_thread::yield();
      }
    }
  }

 private:
  static void run(const Chunk& c) {
    std::memcpy(c.dst, c.src, c.bytes);
    c.batch->remaining.fetch_sub(1, std::memory_order_acq_rel);
  }
  void loop() {
    for (;;) {
      Chunk c{};
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (stop_ && q_.empty()) return;
        c = q_.front();
        q_.pop_front();
      }
      run(c);
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<Chunk> q_;
  bool stop_ = false;
  std::vector<std::thread> threads_;
};

}  // namespace spi
