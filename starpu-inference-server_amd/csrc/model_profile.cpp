// Profiling hooks of the model replica: per-op event records around the forward's launches
// (Model::prof_op), the launch table, and the repeated-op timing of profile_op.
#include "model.hpp"

#include <cstdio>
#include <cstring>

namespace spi {

thread_local std::vector<Model::OpRecord>* Model::prof_ = nullptr;
thread_local Model::ProfRepeat* Model::prof_rep_ = nullptr;

std::vector<LaunchRec>*& launch_log() {
  static thread_local std::vector<LaunchRec>* log = nullptr;
  return log;
}
#ifdef SPI_GEMM_TIMELINE
extern "C" void spi_debug_gemm_timeline_enable(int on, hipStream_t s);
#endif

namespace {
void destroy_events(const Model::OpRecord& r) {
  (void)hipEventDestroy(r.start);
  (void)hipEventDestroy(r.stop);
}
}  // namespace

int Model::op_begin(hipStream_t s, const std::string& name, double flops, double bytes) {
  OpRecord r{name, flops, bytes, nullptr, nullptr, 1};
  if (prof_rep_ && !prof_rep_->done && name == prof_rep_->name) {  // the op profile_op() repeats
    prof_rep_->done = true;
    r.reps = prof_rep_->reps;
#ifdef SPI_GEMM_TIMELINE
    spi_debug_gemm_timeline_enable(1, s);  // stamp only the repeated op's launches
#endif
  }
  SPI_HIP(hipEventCreate(&r.start));
  SPI_HIP(hipEventCreate(&r.stop));
  SPI_HIP(hipEventRecord(r.start, s));
  prof_->push_back(r);
  launch_log() = &prof_->back().launches;  // until op_end (no other record is pushed meanwhile)
  return r.reps;
}

void Model::op_end(hipStream_t s) {
  launch_log() = nullptr;
  SPI_HIP(hipEventRecord(prof_->back().stop, s));
#ifdef SPI_GEMM_TIMELINE
  if (prof_->back().reps > 1) spi_debug_gemm_timeline_enable(0, s);
#endif
}

void Model::run_profiled(hipStream_t s, int B, int S, const void* const* in, void* const* out,
                         std::vector<OpRecord>& recs) {
  if (device_ < 0) throw std::runtime_error("host-only replica (device < 0) cannot run a forward");
  Workspace* w = workspace(s);
  prof_ = &recs;
  try {
    prologue(*w, B, S, in, s);
    body(*w, B, S, s);
    epilogue(*w, B, S, out, s);
  } catch (...) {
    prof_ = nullptr;
    launch_log() = nullptr;
    for (auto& r : recs) destroy_events(r);
    recs.clear();
    throw;
  }
  prof_ = nullptr;
  SPI_HIP(hipStreamSynchronize(s));
}

int Model::profile(hipStream_t s, int B, int S, const void* const* in, void* const* out, float* ms,
                   double* flops, double* bytes, char* names, int name_len, int max_ops) {
  if (m_.family == SPI_FAMILY_AFFINE) return 0;
  std::vector<OpRecord> recs;
  run_profiled(s, B, S, in, out, recs);
  int n = 0;
  for (auto& r : recs) {
    if (n < max_ops) {
      float t = 0.f;
      SPI_HIP(hipEventElapsedTime(&t, r.start, r.stop));
      if (ms) ms[n] = t / r.reps;  // per launch
      if (flops) flops[n] = r.flops;
      if (bytes) bytes[n] = r.bytes;
      if (names && name_len > 0) std::snprintf(names + (size_t)n * name_len, name_len, "%s", r.name.c_str());
      ++n;
    }
    destroy_events(r);
  }
  return n;
}

std::string Model::launch_table(hipStream_t s, int B, int S, const void* const* in, void* const* out) {
  if (m_.family == SPI_FAMILY_AFFINE) return "";
  std::vector<OpRecord> recs;
  run_profiled(s, B, S, in, out, recs);
  std::string t;
  for (size_t i = 0; i < recs.size(); ++i) {
    for (const LaunchRec& l : recs[i].launches) {
      // kernel_id's __PRETTY_FUNCTION__: "... [F = &spi::(anonymous namespace)::name<args>]"
      std::string k = l.kernel;
      const size_t a = k.find("F = &");
      if (a != std::string::npos) k = k.substr(a + 5, k.size() - (a + 5) - (k.back() == ']' ? 1 : 0));
      t += std::to_string(i) + "\t" + recs[i].name + "\t" + k + "\t" + std::to_string(l.gx) + "\t" +
           std::to_string(l.gy) + "\t" + std::to_string(l.gz) + "\t" + std::to_string(l.block) + "\n";
    }
    destroy_events(recs[i]);
  }
  return t;
}

int Model::profile_op(hipStream_t s, int B, int S, const void* const* in, void* const* out, const char* name,
                      int reps, float* ms, double* flops, double* bytes) {
  if (!name || reps < 1) throw std::runtime_error("profile_op: name and reps >= 1 required");
  ProfRepeat rep{name, reps, false};
  prof_rep_ = &rep;
  std::vector<float> t(4096);
  std::vector<double> f(4096), b(4096);
  std::vector<char> names((size_t)4096 * 96);
  int n = 0;
  try {
    n = profile(s, B, S, in, out, t.data(), f.data(), b.data(), names.data(), 96, 4096);
  } catch (...) {
    prof_rep_ = nullptr;
    throw;
  }
  prof_rep_ = nullptr;
  for (int i = 0; i < n; ++i)
    if (std::strcmp(names.data() + (size_t)i * 96, name) == 0) {
      if (ms) *ms = t[i];
      if (flops) *flops = f[i];
      if (bytes) *bytes = b[i];
      return 0;
    }
  throw std::runtime_error(std::string("profile_op: no op named ") + name);
}

}  // namespace spi
