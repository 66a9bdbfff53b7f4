// Host -> device copies on the SDMA engines (SPI_H2D_WORKER_SDMA): the HSA agents of a HIP
// device, a completion signal per slot, the copy and the wait.  The HSA headers stay in
// sdma_copy.cpp: the handles below have the layout of hsa_agent_t / hsa_signal_t.
#pragma once
#include <cstddef>
#include <cstdint>

namespace spi {

struct SdmaAgents {
  uint64_t gpu = 0, cpu = 0;  // the device's GPU agent and the first CPU agent
};
struct SdmaSignal {
  uint64_t handle = 0;  // 0: none
};

// The agents of HIP device `device`; false when they cannot be told (then the stream H2D modes
// serve).  Resolved once per device and cached.
bool find_hsa_agents(int device, SdmaAgents& out);

bool sdma_signal_create(SdmaSignal& sig);
void sdma_signal_destroy(SdmaSignal& sig);
// The signal counts the copies in flight: set it before the first sdma_h2d of a round ...
void sdma_expect(SdmaSignal sig, int copies);
// ... and take off the copies of that round that were never submitted.
void sdma_cancel(SdmaSignal sig, int copies);
// One host -> device copy; completion decrements sig, a failed copy leaves it negative.
bool sdma_h2d(const SdmaAgents& agents, void* dst, const void* src, size_t bytes, SdmaSignal sig);
// Waits (actively) until every expected copy is done; returns the final value: 0, or negative
// when a copy failed.
int64_t sdma_wait(SdmaSignal sig);

}  // namespace spi
