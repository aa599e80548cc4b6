// The base of the handles that run ONE program over one activation block (clip.hip, clip_vision.hip, resampler.hip, hed.hip), on top
// of handle_common.h: the state they share, the configure-time helpers (activation layout, op constructors, split-K workspace) and
// the bodies of the entry points every door has.  Host code only.  A handle derives from ProgramHandle, adds its config and what its
// forward call binds, and writes its registry, its configure and one-line extern "C" forwards that pass their own name as `who`.
#pragma once
#include <string.h>

#include "handle_common.h"

namespace sdeo {

struct ProgramHandle {
  WeightStore ws;
  bool finalized = false;
  // configured state
  char* act = nullptr;
  size_t act_bytes = 0;
  float* splitk_ws = nullptr;
  size_t splitk_bytes = 0;
  Program prog;

  // ---- activation layout: take() every buffer, alloc_act() once, at<T>() for the pointers
  size_t take(size_t bytes) {
    const size_t off = align_up(act_bytes, 256);
    act_bytes = off + bytes;
    return off;
  }
  int alloc_act() {
    act_bytes = align_up(act_bytes, 256);
    SDEO_HIP(hipMalloc((void**)&act, act_bytes));
    SDEO_HIP(hipMemset(act, 0, act_bytes));
    return 0;
  }
  template <class T>
  T* at(size_t off) const { return reinterpret_cast<T*>(act + off); }

  // ---- op constructors.  push: any conv / GEMM (flop_k and late as conv_gemm_op takes them); gemm: y[M][N] = act(x[M][K] w[N][K]^T
  // + bias) + res, all row-major and dense, into y (fp16) or y32 (fp32)
  void push(const ConvGemm& p, int flop_k = 0, std::function<void(ConvGemm&)> late = nullptr) {
    prog.push_back(conv_gemm_op(p, WorkspaceRef{&splitk_ws, &splitk_bytes}, &splitk_bytes, false, flop_k, std::move(late)));
  }
  void gemm(const f16* x, int M, int K, const f16* w, int N, const float* bias, int act_code, const f16* res, f16* y, float* y32 = nullptr,
            std::function<void(ConvGemm&)> late = nullptr) {
    ConvGemm p;
    p.x = x; p.w = w; p.y = y; p.y32 = y32; p.bias = bias; p.res = res; p.ldres = N;
    p.B = M; p.Cin = K; p.M = M; p.N = N; p.K = K; p.ldx = K; p.ldw = K; p.ldy = N; p.act = act_code;
    push(p, 0, std::move(late));
  }
  // y[rows][C] (dense) = LayerNorm(x rows of stride ldx), eps 1e-5
  void ln(f16* y, const f16* x, int ldx, const float* g, const float* b, int rows, int C) {
    prog.push_back(Op([=](hipStream_t s) { return layernorm(y, C, x, ldx, g, b, rows, C, 1e-5f, s); }, "layernorm", 0, 4.0 * rows * C));
  }
  // after the last push: the workspace the largest split-K plan of the program needs
  int alloc_splitk() {
    if (splitk_bytes) SDEO_HIP(hipMalloc((void**)&splitk_ws, splitk_bytes));
    return 0;
  }

  void free_configured() {
    if (act) (void)hipFree(act);
    if (splitk_ws) (void)hipFree(splitk_ws);
    act = nullptr; splitk_ws = nullptr;
    act_bytes = splitk_bytes = 0;
    prog.clear();
  }
  size_t device_bytes() const { return ws.slab_bytes + act_bytes + splitk_bytes + ws.lora_backup_bytes; }
};

// everything up to and including `prefix` stripped: the registry name of a checkpoint key
static inline std::string registry_key(const char* name, const char* prefix) {
  std::string key(name ? name : "");
  const size_t pos = key.find(prefix);
  return pos == std::string::npos ? key : key.substr(pos + strlen(prefix));
}

// ---- bodies of the entry points.  H derives from ProgramHandle and has free_configured(), which resets its own fields and calls the
// base's.  `e` is new, with its registry built: the tail of *_create
template <class H>
int handle_created(const char* who, H* e, H** out) {
  if (int rc = e->ws.alloc(who, /*zero_fill=*/false)) {
    delete e;
    return rc;
  }
  *out = e;
  return 0;
}

template <class H>
int handle_destroy(H* h) {
  if (!h) return 0;
  h->free_configured();
  h->ws.destroy();
  delete h;
  return 0;
}

// the body of *_configure after its argument checks: a build that fails part-way leaves the handle unconfigured
template <class H, class F>
int handle_configure(H* h, F build) {
  h->free_configured();
  const int rc = build();
  if (rc) h->free_configured();
  return rc;
}

static inline int handle_num_weights(const ProgramHandle* h) { return h ? (int)h->ws.entries.size() : 0; }

// ndims / pad: the length of the door's dims array and what fills it beyond the tensor's rank
static inline int handle_weight_info(const char* who, const ProgramHandle* h, int i, const char** name, int64_t* dims, int ndims, int64_t pad,
                                     int* ndim) {
  SDEO_CHECK(h && i >= 0 && i < (int)h->ws.entries.size() && name && dims && ndim, "%s: bad argument", who);
  h->ws.info(i, name, dims, ndims, pad, ndim);
  return 0;
}

static inline int handle_finalize_weights(const char* who, ProgramHandle* h) {
  SDEO_CHECK(h, "%s: null handle", who);
  if (int rc = h->ws.require_all(who)) return rc;
  h->finalized = true;
  return 0;
}

static inline size_t handle_device_bytes(const ProgramHandle* h) { return h ? h->device_bytes() : 0; }

}  // namespace sdeo
