// Host-side machinery shared by the five network handles -- sdeo_* (net_handle.h with net.hip / net_weights.hip / net_build.hip),
// sdeo_clip_* (clip.hip), sdeo_clip_vision_* (clip_vision.hip), sdeo_resampler_* (resampler.hip) and sdeo_hed_* (hed.hip): the weight
// registry / slab / loader and the program runner with its per-launch profiler.  A handle registers its tensors (take / add),
// allocates the slab once, forwards its *_weight_info / *_load_weight / *_finalize_weights entry points here, and unrolls its network
// into a Program at configure time.  The four handles that run one program over one activation block share more than that: their
// state, configure-time helpers and entry-point bodies are program_handle.h's ProgramHandle, and the CLIP layer of the two towers is
// clip_layers.h.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "arena.h"
#include "kernels.h"

extern "C" const char* sdeo_last_error(void);

namespace sdeo {

// how sdeo_*_load_weight stores a tensor: fp16 KRSC [O][R][S][ipad] conv weight, fp16 [rows][cols] matrix, fp32 as is, and
// ff.net.0.proj with its value / gate rows interleaved
enum WKind { W_CONV, W_LINEAR, W_VEC, W_GEGLU_W, W_GEGLU_B };
struct WEntry {
  std::string name;
  int64_t dims[4];
  int ndim;
  WKind kind;
  size_t off;      // byte offset into the weight slab
  int ipad;        // conv: stored (padded) input channels
  bool loaded;
};

struct WeightStore {
  std::vector<WEntry> entries;
  std::unordered_map<std::string, int> index;
  size_t size = 0;           // bytes handed out by take()
  char* slab = nullptr;
  size_t slab_bytes = 0;
  float* stage = nullptr;    // fp32 upload buffer of the largest tensor: allocated by the first load, freed by require_all
  size_t stage_bytes = 0;

  size_t take(size_t bytes) {
    const size_t off = align_up(size, 256);
    size = off + bytes;
    return off;
  }
  // `off` is the caller's: tensors stacked into one matrix (q | k | v) share one take()
  void add(const std::string& name, WKind kind, std::initializer_list<int64_t> dims, size_t off, int ipad = 0) {
    WEntry w{name, {1, 1, 1, 1}, (int)dims.size(), kind, off, ipad, false};
    int i = 0;
    for (auto d : dims) w.dims[i++] = d;
    index[name] = (int)entries.size();
    entries.push_back(w);
  }
  const WEntry* find(const std::string& name) const {
    auto it = index.find(name);
    return it == index.end() ? nullptr : &entries[it->second];
  }
  template <class T>
  const T* ptr(const std::string& name) const { return reinterpret_cast<const T*>(slab + entries[index.at(name)].off); }

  // (re)allocate the slab for everything registered so far; nothing loaded survives
  int alloc(const char* who, bool zero_fill) {
    destroy();
    slab_bytes = align_up(size, 256);
    if (hipMalloc((void**)&slab, slab_bytes) != hipSuccess) {
      slab = nullptr;
      return fail("%s: cannot allocate %zu bytes of weights", who, slab_bytes);
    }
    if (zero_fill) SDEO_HIP(hipMemset(slab, 0, slab_bytes));
    size_t mx = 0;
    for (auto& w : entries) mx = std::max(mx, (size_t)(w.dims[0] * w.dims[1] * w.dims[2] * w.dims[3]));
    stage_bytes = mx * sizeof(float);
    return 0;
  }
  void destroy() {
    if (slab) (void)hipFree(slab);
    if (stage) (void)hipFree(stage);
    slab = nullptr; stage = nullptr;
    lora_free_backups();
    lora_release_stage();
  }

  // dims[k] = pad for k in [ndim, ndims); null outputs are skipped (each entry point checks the ones it requires)
  void info(int i, const char** name, int64_t* dims, int ndims, int64_t pad, int* ndim) const {
    const WEntry& w = entries[i];
    if (name) *name = w.name.c_str();
    if (ndim) *ndim = w.ndim;
    if (dims) for (int k = 0; k < ndims; ++k) dims[k] = k < w.ndim ? w.dims[k] : pad;
  }

  // `who` is the public entry point and `name` what its caller passed (both only for messages); `key` is the registry name
  int load(const char* who, const char* name, const std::string& key, const float* host_data, const int64_t* dims, int ndim, int strict) {
    auto it = index.find(key);
    if (it == index.end()) {
      if (strict) return fail("%s: unexpected tensor '%s'", who, name);
      return 0;
    }
    WEntry& w = entries[it->second];
    SDEO_CHECK(ndim == w.ndim, "%s: %s has %d dims, expected %d", who, name, ndim, w.ndim);
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      SDEO_CHECK(dims[i] == w.dims[i], "%s: %s dim %d is %lld, expected %lld", who, name, i, (long long)dims[i], (long long)w.dims[i]);
      n *= (size_t)dims[i];
    }
    if (!stage) SDEO_HIP(hipMalloc((void**)&stage, stage_bytes));
    SDEO_HIP(hipMemcpy(stage, host_data, n * sizeof(float), hipMemcpyDefault));
    void* dst = slab + w.off;
    int rc = 0;
    switch (w.kind) {
      case W_CONV: rc = oihw_f32_to_ohwi_f16((f16*)dst, stage, (int)w.dims[0], (int)w.dims[1], (int)w.dims[2], (int)w.dims[3], w.ipad, 0); break;
      case W_LINEAR: rc = f32_to_f16((f16*)dst, stage, (int64_t)n, 0); break;
      case W_VEC: SDEO_HIP(hipMemcpy(dst, stage, n * sizeof(float), hipMemcpyDeviceToDevice)); break;
      case W_GEGLU_W: rc = geglu_interleave_f32_to_f16((f16*)dst, stage, (int)(w.dims[0] / 2), (int)w.dims[1], 0); break;
      case W_GEGLU_B: rc = geglu_interleave_f32((float*)dst, stage, (int)(w.dims[0] / 2), 0); break;
    }
    if (rc) return rc;
    SDEO_HIP(hipDeviceSynchronize());
    w.loaded = true;
    return 0;
  }

  int require_all(const char* who) {
    std::string missing;
    int nmiss = 0;
    for (auto& w : entries)
      if (!w.loaded) {
        if (nmiss < 5) missing += (nmiss ? ", " : "") + w.name;
        ++nmiss;
      }
    SDEO_CHECK(nmiss == 0, "%s: %d tensors missing (%s%s)", who, nmiss, missing.c_str(), nmiss > 5 ? ", ..." : "");
    if (stage) { (void)hipFree(stage); stage = nullptr; }
    return 0;
  }

  // ---- LoRA adapters (include/sdeo.h: sdeo_lora_* / sdeo_clip_lora_*).  An adapter is merged IN PLACE into the
  // raw tensor of the slab (lora_merge_f16), so everything that reads weights by address -- programs, captured graphs -- stays valid.
  // The first apply on a tensor saves its raw bytes (copy-on-first-write); restore copies every backup back and frees it.  The owner
  // re-derives what it derives from the raw tensors (folds, composed products) and counts lora_backup_bytes in its device bytes.
  struct LoraBackup { int entry; void* data; size_t bytes; };
  std::vector<LoraBackup> lora_backups;
  size_t lora_backup_bytes = 0;
  float* lora_stage = nullptr;      // down | up of the apply under way (grows, freed by lora_release_stage)
  size_t lora_stage_bytes = 0;

  static size_t raw_bytes(const WEntry& w) {      // of rows 0 .. dims[0] of a matrix or conv weight
    return (size_t)w.dims[0] * (w.kind == W_CONV ? (size_t)w.dims[2] * w.dims[3] * w.ipad : (size_t)w.dims[1]) * sizeof(f16);
  }
  int lora_touched() const { return (int)lora_backups.size(); }
  void lora_release_stage() {
    if (lora_stage) (void)hipFree(lora_stage);
    lora_stage = nullptr; lora_stage_bytes = 0;
  }
  void lora_free_backups() {
    for (auto& b : lora_backups) (void)hipFree(b.data);
    lora_backups.clear();
    lora_backup_bytes = 0;
  }

  // Every refusal happens before the first device call and leaves the store untouched.  not_ready: why the handle cannot take an
  // adapter now (null: it can).  The three formats share the refusals, the staging buffer and the first-write backup:
  //   adapter_entry   null argument, unknown name, vector                          (then the format's own: rank, operand set, shapes)
  //   adapter_ready   non-finite scale, handle not ready, non-square filter
  //   adapter_stage   the staging buffer grown to `floats`;  adapter_backup: the tensor's raw bytes saved on its first write
  int adapter_entry(const char* who, const char* name, const std::string& key, bool operands, int* entry) const {
    SDEO_CHECK(name && operands, "%s: null argument", who);
    auto it = index.find(key);
    SDEO_CHECK(it != index.end(), "%s: unknown tensor '%s'", who, name);
    const WEntry& w = entries[it->second];
    SDEO_CHECK(w.kind == W_LINEAR || w.kind == W_CONV || w.kind == W_GEGLU_W, "%s: %s is a vector (bias / norm), an adapter applies to a matrix or a conv weight", who, name);
    *entry = it->second;
    return 0;
  }
  int adapter_ready(const char* who, const char* name, const WEntry& w, float scale, const char* not_ready) const {
    SDEO_CHECK(scale == scale && scale - scale == 0.f, "%s: scale is not finite", who);
    SDEO_CHECK(!not_ready, "%s: %s", who, not_ready);
    SDEO_CHECK(w.kind != W_CONV || w.dims[2] == w.dims[3], "%s: %s has a %lld x %lld filter (square filters only)", who, name, (long long)w.dims[2], (long long)w.dims[3]);
    return 0;
  }
  int adapter_stage(size_t floats) {
    const size_t need = floats * sizeof(float);
    if (need > lora_stage_bytes) {
      lora_release_stage();
      SDEO_HIP(hipMalloc((void**)&lora_stage, need));
      lora_stage_bytes = need;
    }
    return 0;
  }
  int adapter_backup(const char* who, const char* name, int entry, hipStream_t stream) {
    const WEntry& w = entries[entry];
    bool saved = false;
    for (auto& b : lora_backups) saved = saved || b.entry == entry;
    if (!saved) {
      LoraBackup b{entry, nullptr, raw_bytes(w)};
      if (hipMalloc(&b.data, b.bytes) != hipSuccess) return fail("%s: cannot allocate %zu bytes to save %s", who, b.bytes, name);
      if (hipMemcpyAsync(b.data, slab + w.off, b.bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        (void)hipFree(b.data);
        return fail("%s: cannot save %s", who, name);
      }
      lora_backups.push_back(b);
      lora_backup_bytes += b.bytes;
    }
    return 0;
  }

  // down [rank][in * kh * kw] / up [out][rank] fp32, host or device pointers (hipMemcpyDefault, as load).
  // Synchronises `stream` (the staging buffer is reused by the next apply).
  int lora_apply(const char* who, const char* name, const std::string& key, const float* down, const float* up, int rank, float scale,
                 const char* not_ready, hipStream_t stream) {
    int e;
    if (int rc = adapter_entry(who, name, key, down && up, &e)) return rc;
    WEntry& w = entries[e];
    SDEO_CHECK(rank >= 1 && rank <= 1024, "%s: rank %d out of range (1..1024)", who, rank);
    if (int rc = adapter_ready(who, name, w, scale, not_ready)) return rc;
    const int O = (int)w.dims[0], I = (int)w.dims[1], k = w.kind == W_CONV ? (int)w.dims[2] : 1;
    const size_t nd = (size_t)rank * I * k * k, nu = (size_t)O * rank;
    if (int rc = adapter_stage(nd + nu)) return rc;
    SDEO_HIP(hipMemcpy(lora_stage, down, nd * sizeof(float), hipMemcpyDefault));
    SDEO_HIP(hipMemcpy(lora_stage + nd, up, nu * sizeof(float), hipMemcpyDefault));
    if (int rc = adapter_backup(who, name, e, stream)) return rc;
    if (int rc = lora_merge_f16((f16*)(slab + w.off), w.kind, O, I, k, w.ipad, lora_stage, lora_stage + nd, rank, scale, stream)) return rc;
    SDEO_HIP(hipStreamSynchronize(stream));
    return 0;
  }

  // LoHa / LoKr (kernels.h: LycoOps; include/sdeo.h defines the forms): the operands as the file holds them, host or device pointers.
  // loha_apply and lokr_apply differ only in how the entry point filled `ops`.
  int lyco_apply(const char* who, const char* name, const std::string& key, const LycoOps& ops, float scale, const char* not_ready,
                 hipStream_t stream) {
    int e;
    if (int rc = adapter_entry(who, name, key, true, &e)) return rc;
    WEntry& w = entries[e];
    const int O = (int)w.dims[0], I = (int)w.dims[1], k = w.kind == W_CONV ? (int)w.dims[2] : 1;
    if (int rc = lyco_check(who, ops, w.kind, O, I, k)) return rc;
    if (int rc = adapter_ready(who, name, w, scale, not_ready)) return rc;
    if (int rc = adapter_stage(lyco_stage_floats(ops, O, I, k))) return rc;
    if (int rc = adapter_backup(who, name, e, stream)) return rc;
    if (int rc = lyco_merge_f16((f16*)(slab + w.off), w.kind, O, I, k, w.ipad, ops, lora_stage, scale, stream)) return rc;
    SDEO_HIP(hipStreamSynchronize(stream));
    return 0;
  }
  int loha_apply(const char* who, const char* name, const std::string& key, const float* w1_a, const float* w1_b, const float* w2_a,
                 const float* w2_b, const float* t1, const float* t2, int rank, float scale, const char* not_ready, hipStream_t stream) {
    LycoOps ops;
    ops.algo = LYCO_LOHA; ops.a1 = w1_a; ops.b1 = w1_b; ops.t1 = t1; ops.a2 = w2_a; ops.b2 = w2_b; ops.t2 = t2; ops.rank1 = ops.rank2 = rank;
    return lyco_apply(who, name, key, ops, scale, not_ready, stream);
  }
  int lokr_apply(const char* who, const char* name, const std::string& key, const float* w1, const float* w1_a, const float* w1_b, int rank1,
                 const float* w2, const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale,
                 const char* not_ready, hipStream_t stream) {
    LycoOps ops;
    ops.algo = LYCO_LOKR; ops.w1 = w1; ops.a1 = w1_a; ops.b1 = w1_b; ops.rank1 = rank1; ops.w2 = w2; ops.a2 = w2_a; ops.b2 = w2_b; ops.t2 = t2;
    ops.rank2 = rank2; ops.out_l = out_l; ops.in_m = in_m;
    return lyco_apply(who, name, key, ops, scale, not_ready, stream);
  }

  // copy every backup back and free it: the raw tensors are bit for bit what load left
  int lora_restore() {
    for (auto& b : lora_backups) SDEO_HIP(hipMemcpy(slab + entries[b.entry].off, b.data, b.bytes, hipMemcpyDeviceToDevice));
    SDEO_HIP(hipDeviceSynchronize());
    lora_free_backups();
    lora_release_stage();
    return 0;
  }

  // the inverse of load: the current RAW tensor as fp32 in PyTorch layout (GEGLU rows de-interleaved, KRSC -> OIHW without the pad);
  // out is a host or a device pointer
  int read(const char* who, const char* name, const std::string& key, float* out) {
    SDEO_CHECK(name && out, "%s: null argument", who);
    auto it = index.find(key);
    SDEO_CHECK(it != index.end(), "%s: unknown tensor '%s'", who, name);
    const WEntry& w = entries[it->second];
    SDEO_CHECK(w.loaded, "%s: %s is not loaded", who, name);
    SDEO_CHECK(w.kind != W_GEGLU_B, "%s: %s is the interleaved GEGLU bias, which this call does not read back", who, name);
    const size_t n = (size_t)(w.dims[0] * w.dims[1] * w.dims[2] * w.dims[3]);
    if (w.kind == W_VEC) {
      SDEO_HIP(hipMemcpy(out, slab + w.off, n * sizeof(float), hipMemcpyDefault));
      return 0;
    }
    float* tmp = nullptr;
    SDEO_HIP(hipMalloc((void**)&tmp, n * sizeof(float)));
    int rc = lora_read_f32(tmp, (const f16*)(slab + w.off), w.kind, (int)w.dims[0], (int)w.dims[1], w.kind == W_CONV ? (int)w.dims[2] : 1, w.ipad, 0);
    if (!rc && hipMemcpy(out, tmp, n * sizeof(float), hipMemcpyDefault) != hipSuccess) rc = fail("%s: cannot copy %s out", who, name);
    (void)hipFree(tmp);
    return rc;
  }
};

struct Op {          // one launch of a program + what it is for the profiler
  std::function<int(hipStream_t)> fn;
  const char* key = "other";
  std::string tag;           // problem shape, shown by the profiler when SDEO_PROFILE_DETAIL=1
  double flops = 0, bytes = 0;
  bool zero_conv = false;    // net_build.hip's ControlNet program: a zero conv (skipped when the UNet decoder applies the zero convs itself)
  bool freeu = false;        // net_build.hip's UNet decoders: a FreeU launch (only in the programs a handle runs with sdeo_set_freeu on)
  // net_build.hip's fused UNet decoder: a launch that applies control net zc_net's zero convs (-1: any other launch) in the form
  // zc_form, bits ZC_COND (the first half of the batch only) | ZC_FIRST (no active net in front: the residual is the skip).  A handle
  // with sdeo_enable_control_modes holds every form and runs, per net, the one its mode asks for (net.hip: run_decoder)
  signed char zc_net = -1, zc_form = 0;
  template <class F>
  Op(F f, const char* key_ = "other", double flops_ = 0, double bytes_ = 0, std::string tag_ = std::string())
      : fn(std::move(f)), key(key_), tag(std::move(tag_)), flops(flops_), bytes(bytes_) {}
  int operator()(hipStream_t s) const { return fn(s); }
};
typedef std::vector<Op> Program;

// HIP events around every launch between begin() and end(); end() synchronises and reports per key
struct Profiler {
  struct Rec { std::string key; double flops, bytes; hipEvent_t a, b; };
  bool on = false;
  std::vector<Rec> recs;
  std::string report;

  void begin() {
    for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    recs.clear();
    on = true;
  }
  int record(const Op& op, hipStream_t s) {
    static const bool detail = [] { const char* v = getenv("SDEO_PROFILE_DETAIL"); return v && atoi(v) != 0; }();
    Rec r{detail && !op.tag.empty() ? std::string(op.key) + " | " + op.tag : std::string(op.key), op.flops, op.bytes, nullptr, nullptr};
    SDEO_HIP(hipEventCreate(&r.a));
    SDEO_HIP(hipEventCreate(&r.b));
    SDEO_HIP(hipEventRecord(r.a, s));
    if (int rc = op(s)) return rc;
    SDEO_HIP(hipEventRecord(r.b, s));
    recs.push_back(r);
    return 0;
  }
  // JSON array [{"kernel", "launches", "total_ms", "flops", "bytes"}] in order of first appearance
  const char* end() {
    on = false;
    (void)hipDeviceSynchronize();
    struct Agg { long n = 0; double ms = 0, flops = 0, bytes = 0; };
    std::vector<std::pair<std::string, Agg>> aggs;
    for (auto& r : recs) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r.a, r.b);
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
      size_t i = 0;
      for (; i < aggs.size(); ++i) if (aggs[i].first == r.key) break;
      if (i == aggs.size()) aggs.push_back({r.key, Agg()});
      aggs[i].second.n += 1; aggs[i].second.ms += ms; aggs[i].second.flops += r.flops; aggs[i].second.bytes += r.bytes;
    }
    recs.clear();
    report = "[";
    char buf[768];
    for (size_t i = 0; i < aggs.size(); ++i) {
      snprintf(buf, sizeof(buf), "%s{\"kernel\": \"%s\", \"launches\": %ld, \"total_ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}",
               i ? ", " : "", aggs[i].first.c_str(), aggs[i].second.n, aggs[i].second.ms, aggs[i].second.flops, aggs[i].second.bytes);
      report += buf;
    }
    report += "]";
    return report.c_str();
  }
};

// The split-K workspace of a handle is sized by the largest conv_gemm_workspace_bytes of its programs, so it is allocated after they
// are built: a launch reads where it is through this.
struct WorkspaceRef { float* const* p; const size_t* bytes; };

// THE constructor of a conv / GEMM launch: binds the workspace (and whatever else `late` sets) at launch time, names the kernel of
// p's plan for the profiler with 2 M N K flops and the algorithmic bytes of x, w and y, and raises *max_ws to what p's plan needs.
// tagged: shape in the profiler key; flop_k: the K that counts when the stored one is padded (HED's first conv: 3 image channels in 8)
static inline Op conv_gemm_op(const ConvGemm& p0, WorkspaceRef ws, size_t* max_ws, bool tagged = false, int flop_k = 0,
                              std::function<void(ConvGemm&)> late = nullptr) {
  *max_ws = std::max(*max_ws, conv_gemm_workspace_bytes(p0));
  return Op([p = p0, ws, late](hipStream_t s) mutable {
    p.workspace = *ws.p;
    p.workspace_bytes = *ws.bytes;
    if (late) late(p);
    return conv_gemm(p, s);
  }, conv_gemm_kernel_name(p0), 2.0 * p0.M * p0.N * (double)(flop_k ? flop_k : p0.K),
     2.0 * ((double)p0.M * p0.Cin + (double)p0.N * p0.K + (double)p0.M * p0.N),
     !tagged ? std::string() : "M" + std::to_string(p0.M) + " N" + std::to_string(p0.N) + " K" + std::to_string(p0.K) + " R" +
         std::to_string(p0.R) + " s" + std::to_string(p0.stride) + " u" + std::to_string(p0.ups));
}

// Several unsplit conv / GEMM problems on one tile as ONE launch (kernels.h: conv_gemm_multi_plan).  The device table is written here,
// once, and lives as long as the op; scale_host[i] (optional, may hold nulls) is problem i's `scale`, read when the launch runs.  A
// set of problems the launcher refuses gives an op that fails with that message.  Profile key: the tile's kernel + "multi xN".
// m_live (optional, one per problem): the live-row form (conv_gemm_multi_launch_live); flops and bytes then count the live rows.
static inline Op conv_gemm_multi_op(const std::vector<ConvGemm>& ps, int tile, std::vector<const float*> scale_host = {},
                                    std::vector<int> m_live = {}) {
  static std::set<std::string> keys;       // Op::key is a C string that outlives the op
  auto pl = std::make_shared<ConvGemmMultiPlan>();
  std::shared_ptr<void> dev;
  std::string err;
  if (conv_gemm_multi_plan(ps, tile, pl.get())) {
    err = sdeo_last_error();
  } else {
    void* d = nullptr;
    if (hipMalloc(&d, pl->table.size()) != hipSuccess || hipMemcpy(d, pl->table.data(), pl->table.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      err = "conv_gemm_multi: cannot place the problem table in device memory";
    }
    dev.reset(d, [](void* q) { if (q) (void)hipFree(q); });
  }
  scale_host.resize(ps.size(), nullptr);
  const char* key = keys.insert(std::string(err.empty() ? pl->name : "conv_gemm multi") + (m_live.empty() ? "" : " live") + " x" + std::to_string(ps.size())).first->c_str();
  if (!m_live.empty() && m_live.size() != ps.size() && err.empty()) err = "conv_gemm_multi: one live-row count per problem";
  double flops = pl->flops, bytes = pl->bytes;
  if (!m_live.empty() && err.empty()) {
    flops = bytes = 0;
    for (size_t i = 0; i < ps.size(); ++i) {
      flops += 2.0 * m_live[i] * ps[i].N * (double)ps[i].K;
      bytes += 2.0 * ((double)m_live[i] * ps[i].Cin + (double)ps[i].N * ps[i].K + (double)ps[i].M * ps[i].N);
    }
  }
  return Op([pl, dev, err, scale_host, m_live](hipStream_t s) {
    if (!err.empty()) return fail("%s", err.c_str());
    float sc[kMultiMax];
    for (int i = 0; i < pl->count; ++i) sc[i] = scale_host[i] ? *scale_host[i] : pl->scale[i];
    if (!m_live.empty()) return conv_gemm_multi_launch_live(*pl, dev.get(), sc, m_live.data(), s);
    return conv_gemm_multi_launch(*pl, dev.get(), sc, s);
  }, key, flops, bytes, "tiles" + std::to_string(pl->tiles) + (m_live.empty() ? "" : " live"));
}

// profiling off (or no profiler): one std::function call per op and nothing else
static inline int run_program(const Program& p, hipStream_t s, Profiler* prof = nullptr) {
  if (!prof || !prof->on) {
    for (auto& op : p)
      if (int rc = op(s)) return rc;
    return 0;
  }
  for (auto& op : p)
    if (int rc = prof->record(op, s)) return rc;
  return 0;
}

}  // namespace sdeo
