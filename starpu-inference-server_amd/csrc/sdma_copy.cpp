#include "sdma_copy.hpp"

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstring>
#include <map>
#include <mutex>

namespace spi {
namespace {

// HIP device -> its HSA GPU agent and the first CPU agent, for
// SPI_H2D_WORKER_SDMA.  Matched by the agent UUID (hipDeviceGetUuid carries the
// 16 hex digits of HSA_AMD_AGENT_INFO_UUID's body), so partitions of one GPU
// that share a PCI bus / device (CPX / TPX modes) are told apart; without a
// UUID, by PCI domain / bus / device / function, accepted only when exactly one
// agent matches.  hsa_init / hsa_shut_down are paired around the enumeration:
// HIP holds its own reference, which keeps the agent handles valid for the process.
bool resolve_hsa_agents(int device, hsa_agent_t& gpu, hsa_agent_t& cpu) {
  hipUUID uuid{};
  const bool have_uuid = hipDeviceGetUuid(&uuid, device) == hipSuccess;
  int bus = 0, dev = 0, dom = 0;
  if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device) != hipSuccess ||
      hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, device) != hipSuccess ||
      hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainId, device) != hipSuccess)
    return false;
  struct Find {
    char uuid[16];
    bool have_uuid;
    uint32_t bdf, dom;
    hsa_agent_t by_uuid{}, by_bdf{}, cpu{};
    int n_uuid = 0, n_bdf = 0;
    bool c = false;
  } f{};
  std::memcpy(f.uuid, uuid.bytes, 16);
  f.have_uuid = have_uuid;
  f.bdf = (uint32_t)((bus << 8) | (dev << 3));
  f.dom = (uint32_t)dom;
  if (hsa_init() != HSA_STATUS_SUCCESS) return false;
  hsa_iterate_agents(
      [](hsa_agent_t a, void* u) {
        Find& f = *static_cast<Find*>(u);
        hsa_device_type_t t;
        if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
        if (t == HSA_DEVICE_TYPE_CPU && !f.c) {
          f.cpu = a;
          f.c = true;
        } else if (t == HSA_DEVICE_TYPE_GPU) {
          char id[32] = {};
          if (f.have_uuid && hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_UUID, id) == HSA_STATUS_SUCCESS &&
              std::strncmp(id, "GPU-", 4) == 0 && std::strlen(id) >= 20 && std::memcmp(id + 4, f.uuid, 16) == 0) {
            f.by_uuid = a;
            ++f.n_uuid;
          }
          uint32_t bdf = 0, dom = 0;
          hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf);
          hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom);
          if ((bdf & ~7u) == f.bdf && dom == f.dom) {
            f.by_bdf = a;
            ++f.n_bdf;
          }
        }
        return HSA_STATUS_SUCCESS;
      },
      &f);
  (void)hsa_shut_down();
  cpu = f.cpu;
  if (f.n_uuid == 1) {
    gpu = f.by_uuid;
  } else if (f.n_uuid == 0 && f.n_bdf == 1) {
    gpu = f.by_bdf;
  } else {
    return false;  // ambiguous (partitioned GPU without UUIDs): the stream H2D modes
  }
  return f.c;
}

}  // namespace

bool find_hsa_agents(int device, SdmaAgents& out) {
  struct Entry {
    bool ok;
    hsa_agent_t gpu, cpu;
  };
  static std::mutex mu;
  static std::map<int, Entry> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(device);
  if (it == cache.end()) {
    Entry e{};
    e.ok = resolve_hsa_agents(device, e.gpu, e.cpu);
    it = cache.emplace(device, e).first;
  }
  out.gpu = it->second.gpu.handle;
  out.cpu = it->second.cpu.handle;
  return it->second.ok;
}

bool sdma_signal_create(SdmaSignal& sig) {
  hsa_signal_t s{};
  if (hsa_signal_create(0, 0, nullptr, &s) != HSA_STATUS_SUCCESS) return false;
  sig.handle = s.handle;
  return true;
}

void sdma_signal_destroy(SdmaSignal& sig) {
  if (sig.handle) (void)hsa_signal_destroy(hsa_signal_t{sig.handle});
  sig.handle = 0;
}

void sdma_expect(SdmaSignal sig, int copies) { hsa_signal_store_screlease(hsa_signal_t{sig.handle}, copies); }

void sdma_cancel(SdmaSignal sig, int copies) { hsa_signal_subtract_screlease(hsa_signal_t{sig.handle}, copies); }

// On the engine ROCr assigns (pinning one engine measured no different, round 3).
bool sdma_h2d(const SdmaAgents& agents, void* dst, const void* src, size_t bytes, SdmaSignal sig) {
  return hsa_amd_memory_async_copy(dst, hsa_agent_t{agents.gpu}, src, hsa_agent_t{agents.cpu}, bytes, 0, nullptr,
                                   hsa_signal_t{sig.handle}) == HSA_STATUS_SUCCESS;
}

// A wait may return before the condition holds (the HSA spec allows it; ROCclr loops too): wait
// until the value drops below 1.  Each completed copy decrements it; a failed copy leaves it
// negative.
int64_t sdma_wait(SdmaSignal sig) {
  const hsa_signal_t s{sig.handle};
  hsa_signal_value_t v = hsa_signal_load_scacquire(s);
  while (v >= 1) v = hsa_signal_wait_scacquire(s, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_ACTIVE);
  return v;
}

}  // namespace spi
