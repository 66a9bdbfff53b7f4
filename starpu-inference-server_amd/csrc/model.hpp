// Device-resident model replica: the MI355X replacement for the per-device
// TorchScript clones of inference_runner.cpp:251-275.  The weights are recognised, folded and
// packed on the host (model_pack.hpp) and the whole replica lives in one HBM blob.
// Activations live in per-stream workspaces (one per StarPU worker stream: replicas are
// shared read-only by the workers of a device, starpu_setup.cpp:725-778 /
// docs/server_guide.md:116).  Layers: packer (model_pack.cpp) -> host-only forward plans: I/O
// contract, layer descs, the ResNet walk, FLOPs, workspace sizes (model_plan.cpp) -> replica,
// workspaces, launch helpers and the per-family launches (model.cpp) -> profiling hooks
// (model_profile.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "model_plan.hpp"
#include "spi_kernels.hpp"

#define SPI_HIP(x)                                                                  \
  do {                                                                              \
    hipError_t e__ = (x);                                                           \
    if (e__ != hipSuccess)                                                          \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e__) + \
                               " at " #x);                                          \
  } while (0)

#ifndef SPI_STEM_PR  // variant builds: 1 / 2 pooled rows per 4-wave workgroup (stem.hip)
#define SPI_STEM_PR 0
#endif

namespace spi {

struct Workspace;

class Model {
 public:
  Model(int device, const spi_model_config& cfg, const spi_named_tensor* params, int n);
  ~Model();

  int device() const { return device_; }
  int family() const { return m_.family; }
  bool f16() const { return m_.f16; }
  int max_batch() const { return m_.max_batch; }
  size_t weight_bytes() const { return m_.blob_bytes; }
  uint64_t weight_digest() const { return m_.digest; }
  const std::string& describe() const { return desc_; }
  int bert_num_labels() const { return m_.num_labels; }  // the task head's label count, 0 without a head
  double flops(int64_t batch) const { return model_flops(m_, batch); }
  // Debug exports (spi_model_workspace_plan, spi_model_plan_check): what workspace() allocates, and the
  // forward walked without a launch against it; both work on a host-only replica.
  WorkspacePlan planned_workspace() const { return workspace_plan(m_, opt_); }
  int check_plan(int batch, int S) const { return plan_check(m_, opt_, batch, S); }
  void set_graphs(bool on) { graphs_ = on; }

  // The task's I/O against the replica and what its input 0 holds (model_plan.hpp).
  void check_io(const spi_codelet_args& a, const size_t* in_bytes, const size_t* out_bytes) const {
    spi::check_io(m_, opt_, a, in_bytes, out_bytes);
  }
  ImageSrc input_kind(const spi_codelet_args& a) const { return spi::input_kind(m_, opt_, a); }
  // The input transform of 8-bit image tasks (spi_model_set_input_transform); null pointers reset
  // it to scale 1, shift 0.  Returns an spi_status.  Not synchronised with forwards in flight.
  int set_input_transform(const float* scale, const float* shift);
  // The classification outputs of a ResNet / ViT replica (spi_model_set_image_outputs): SPI_IMAGE_* bits
  // and the top-k count.  Returns an spi_status and, on refusal, the message in `err`.  Refused once a
  // stream workspace exists: the logits scratch of SPI_IMAGE_NO_LOGITS is sized with the workspace.
  int set_image_outputs(int image_io, int top_k, std::string& err);
  // Resize + centre crop of 8-bit image tasks (spi_model_set_input_resize): 0 off, else the short side the
  // source is resized to before the centre crop to the replica's image.  Returns an spi_status and, on
  // refusal, the message in `err`.  Refused once a stream workspace exists: the resampled image lives there.
  int set_input_resize(int resize_short, std::string& err);
  // Enqueue the forward on `s`; never synchronises.
  // S: BERT sequence length (ignored otherwise); n: AFFINE element count; src: what input 0 holds
  // (input_kind; read by the prologue only -- the captured body does not depend on it).
  void forward(hipStream_t s, int batch, int S, size_t n, const void* const* in, void* const* out,
               ImageSrc src = ImageSrc{});
  // Allocate the stream's workspace and capture its (batch, S, mask) graph ahead of serving.
  void warmup(hipStream_t s, int batch, int S, bool mask);

  // Per-op profile of one forward: each launch bracketed by hipEvents on `s`.
  struct OpRecord {
    std::string name;
    double flops;
    double bytes;
    hipEvent_t start, stop;
    int reps;  // launches between start and stop (profile_op)
    std::vector<LaunchRec> launches;  // the op's kernel launches (SPI_LAUNCH), in order
  };
  int profile(hipStream_t s, int batch, int S, const void* const* in, void* const* out, float* ms,
              double* flops, double* bytes, char* names, int name_len, int max_ops);
  // One profiled eager forward as text, one line per kernel launch:
  // "op_index\top_name\tkernel\tgrid_x\tgrid_y\tgrid_z\tblock\n" (spi_model_launch_table).
  std::string launch_table(hipStream_t s, int batch, int S, const void* const* in, void* const* out);
  // The same forward with op `name` launched `reps` times back to back; its time per launch.
  int profile_op(hipStream_t s, int batch, int S, const void* const* in, void* const* out, const char* name,
                 int reps, float* ms, double* flops, double* bytes);

 private:
  Workspace* workspace(hipStream_t s);
  hipGraphExec_t graph(Workspace& w, int batch, int S, hipStream_t s);
  // Forward: prologue (reads the task's input buffers) -> body (workspace only, graph-capturable)
  // -> epilogue (writes the task's output buffer); each dispatches once to its family's plan.
  void prologue(Workspace& w, int batch, int S, const void* const* in, hipStream_t s, ImageSrc src = ImageSrc{});
  void body(Workspace& w, int batch, int S, hipStream_t s);
  void epilogue(Workspace& w, int batch, int S, void* const* out, hipStream_t s);
  void prologue_resnet(Workspace& w, int B, const void* x, hipStream_t s, int src);
  void body_resnet(Workspace& w, int B, hipStream_t s);
  void body_bert(Workspace& w, int B, int S, hipStream_t s);
  void body_bert_folded(Workspace& w, int B, int S, hipStream_t s);
  void body_vit(Workspace& w, int B, hipStream_t s);
  void body_vit_folded(Workspace& w, int B, hipStream_t s);
  void epilogue_bert(Workspace& w, int B, int S, void* const* out, hipStream_t s);
  // ResNet / ViT with image outputs: where the classifier writes its logits (the first output, or the
  // workspace scratch under SPI_IMAGE_NO_LOGITS), and the launch that derives the other outputs from them
  float* logits_dst(void* scratch, void* const* out) const {
    return static_cast<float*>((opt_.image_io & SPI_IMAGE_NO_LOGITS) ? scratch : out[0]);
  }
  void run_image_outputs(const float* logits, int B, void* const* out, hipStream_t s);
  // One GEMM from its finished desc (linear_layer_desc / tf_gemm_desc) plus pointers; ln: the LayerNorm
  // fold's statistics / gain / bias pointers the desc asks for (ln_fold.hpp), else empty.
  void run_gemm(const LinearW& L, const GemmDesc& d, const void* A, void* C, const void* res, const LnPtrs& ln,
                Workspace& ws, hipStream_t s);
  // GEMM g of encoder layer `layer` over T token rows: the desc is tf_gemm_desc's
  void run_tf_gemm(int layer, TfGemm g, int T, const void* A, void* C, const void* res, Workspace& ws,
                   hipStream_t s, const LnPtrs& ln = LnPtrs{});
  // QKV projection + attention of encoder layer `layer`: the fused kernel (qkv_attn.hip) when
  // the shape allows it, else the QKV GEMM into qkv and the attention launch
  void run_qkv_attention(int layer, const void* x, const float* in_stats, void* qkv, void* ctx, int B, int S,
                         Workspace& ws, hipStream_t s);
  // Convs from their finished descs (conv_layer_desc): the launchers add pointers, FLOPs and bytes.
  struct ConvCall {  // the op's name (conv_name) is built only while profiling
    GemmPtrs p;
    double flops = 0, bytes = 0;
  };
  ConvCall conv_call(const ConvW& c, const GemmDesc& d, const void* x, void* y, const void* res,
                     const Workspace& ws) const;
  void run_conv(const ConvW& c, const GemmDesc& d, const void* x, void* y, const void* res, Workspace& ws,
                hipStream_t s);
  void run_gconv(const ConvW& c, const void* x, int B, int H, void* y, Act act, hipStream_t s);
  void run_conv_pair(const void* x, const ConvW& c0, const GemmDesc& d0, void* y0, const ConvW& c1, const GemmDesc& d1,
                     void* y1, Workspace& ws, hipStream_t s);
  void run_pooled_fc(const void* act, int B, int hw, void* out, Workspace& ws, hipStream_t s);
  template <typename P>
  const P* ptr(size_t off) const {
    return reinterpret_cast<const P*>(static_cast<const char*>(dblob_) + off);
  }
  // The pointers of one GEMM / conv launch: weight and bias at their blob offsets, the stream's
  // split-K workspace, and the blob's leading zero line.
  GemmPtrs gemm_ptrs(const void* A, size_t w, size_t bias, const void* res, void* C, const Workspace& ws) const;

  int device_ = 0;
  PackedModel m_;  // what the packer recognised and laid out; its host blob is dropped after the upload
  bool graphs_ = false;
  void* dblob_ = nullptr;
  int stem_pr_ = SPI_STEM_PR;  // the fused stem's workgroup shape (0 = auto, stem.hip)
  InputXf input_xf_;  // ResNet / ViT: the transform of 8-bit image tasks, passed to the prologue's kernel
  ReplicaOptions opt_;  // set_image_outputs, set_input_resize
  std::string desc_;    // replica_desc(m_, opt_)
  // The setters' common end: under mu_, refuse once a stream workspace exists, else assign and re-describe.
  template <typename F>
  int set_options(const char* what, std::string& err, F&& assign);
  // SPI_QKV_ATTN: 0 the QKV GEMM + attention launches (A/B); 1 (default) the fused kernel for S <= 128;
  // 2 also for 129..256 tokens (ViT-L at 197: correct, but -4 % under the four streams)
  int qkv_fused_ = 1;

  std::mutex mu_;
  std::map<hipStream_t, std::unique_ptr<Workspace>> ws_;
  void run_profiled(hipStream_t s, int B, int S, const void* const* in, void* const* out, std::vector<OpRecord>& recs);
  // Set only inside profile(), on the profiling thread: concurrent forwards on other threads never see it.
  static thread_local std::vector<OpRecord>* prof_;
  struct ProfRepeat {
    std::string name;
    int reps;
    bool done;
  };
  static thread_local ProfRepeat* prof_rep_;
  // Starts an op record; returns how many times the op is to be launched (1, or
  // profile_op's repeat count for the op it names).
  int op_begin(hipStream_t s, const std::string& name, double flops, double bytes);
  void op_end(hipStream_t s);
  // Profiled launch (bytes = algorithmic traffic); a plain call when not profiling.  `name` is a
  // string literal or a callable returning the name, which runs only while profiling.
  template <typename N, typename F>
  void prof_op(hipStream_t s, N&& name, double flops, double bytes, F&& launch) {
    if (!prof_) return launch();
    int nrep;
    if constexpr (std::is_invocable_v<N>) nrep = op_begin(s, name(), flops, bytes);
    else nrep = op_begin(s, name, flops, bytes);
    for (int r = 0; r < nrep; ++r) launch();
    op_end(s);
  }
  // LayerNorm over rows x D: fp32 in + fp32 out (+ compute-type copy).
  double ln_bytes(double rows, bool f32_out) const {
    return rows * m_.D * (4 + (f32_out ? 4 : 0) + (m_.f16 ? 2 : (f32_out ? 0 : 4)));
  }
};

}  // namespace spi

struct spi_model {
  std::unique_ptr<spi::Model> impl;
};
