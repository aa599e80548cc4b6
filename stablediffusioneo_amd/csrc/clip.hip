// CLIP text transformer (the step before the DDIM loop): `FrozenCLIPEmbedder.forward`
// (`ldm/modules/encoders/modules.py:123-141`) calls HuggingFace `CLIPTextModel` (transformers, an un-vendored
// dependency of the reference) and returns `last_hidden_state`.  The published algorithm restated here:
//   x = token_embedding[ids] + position_embedding[0..T)
//   per layer:  x += out_proj(softmax_causal((q_proj(LN1 x) * d^-1/2) k_proj(LN1 x)^T) v_proj(LN1 x))
//               x += fc2(quick_gelu(fc1(LN2 x)))          quick_gelu(v) = v * sigmoid(1.702 v)
//   out = final_layer_norm(x)                              (LayerNorm eps 1e-5 throughout)
// `FrozenOpenCLIPEmbedder.encode_with_transformer` (`modules.py:186-203`, the SD-2.x text tower) is the same program with erf GELU in
// the MLP and, for layer = "penultimate", without the last block (sdeo_clip_set_variant).
// Built from the same hand-written kernels as the UNet (layernorm, LDS-DMA GEMM with fused bias / activation /
// residual epilogues, flash attention with a causal mask).  q_proj and k_proj are stacked into one GEMM.
#include "../../include/sdeo.h"
#include "clip_layers.h"

using namespace sdeo;

struct sdeo_clip_handle_s : ProgramHandle {
  sdeo_clip_config cfg{};
  int hidden_act = 0, skip_last = 0;       // sdeo_clip_set_variant: erf GELU in the MLP; blocks at the end that are loaded but not run
  // configured state
  int batch = 0;
  int32_t* tokens = nullptr;
  f16* out16 = nullptr;

  void free_configured() {
    if (tokens) (void)hipFree(tokens);
    tokens = nullptr;
    batch = 0;
    ProgramHandle::free_configured();
  }
};

namespace {

typedef sdeo_clip_handle_s Clip;

// names follow the HuggingFace state dict below "text_model." (the SD checkpoint stores them as
// "cond_stage_model.transformer.text_model.*"; clip_key strips everything up to "text_model.")
static void build_registry(Clip* e) {
  const sdeo_clip_config& c = e->cfg;
  WeightStore& r = e->ws;
  const int W = c.width;
  r.add("embeddings.token_embedding.weight", W_LINEAR, {c.vocab, W}, r.take((size_t)c.vocab * W * 2));
  r.add("embeddings.position_embedding.weight", W_LINEAR, {c.positions, W}, r.take((size_t)c.positions * W * 2));
  clip_layers_register(r, c.layers, W, c.ffn);
  r.add("final_layer_norm.weight", W_VEC, {W}, r.take((size_t)W * 4));
  r.add("final_layer_norm.bias", W_VEC, {W}, r.take((size_t)W * 4));
}

static std::string clip_key(const char* name) { return registry_key(name, "text_model."); }

// the body of sdeo_clip_configure after its checks
static int configure_impl(Clip* e, int B) {
  const sdeo_clip_config& c = e->cfg;
  const int T = c.positions, W = c.width, F = c.ffn;
  const int rows = B * T;
  // activation buffers (fp16): xa, xb, a [rows][W]; qkv [rows][3W]; o [rows][W]; hid [rows][F]
  const size_t o_xa = e->take((size_t)rows * W * 2), o_xb = e->take((size_t)rows * W * 2), o_a = e->take((size_t)rows * W * 2),
               o_qkv = e->take((size_t)rows * 3 * W * 2), o_o = e->take((size_t)rows * W * 2), o_h = e->take((size_t)rows * F * 2);
  if (int rc = e->alloc_act()) return rc;
  SDEO_HIP(hipMalloc((void**)&e->tokens, (size_t)rows * sizeof(int32_t)));
  const ClipLayerBufs b{e->at<f16>(o_xa), e->at<f16>(o_xb), e->at<f16>(o_a), e->at<f16>(o_qkv), e->at<f16>(o_o), e->at<f16>(o_h)};
  const f16* tok = e->ws.ptr<f16>("embeddings.token_embedding.weight");
  const f16* pos = e->ws.ptr<f16>("embeddings.position_embedding.weight");
  const int32_t* ids = e->tokens;
  const int vocab = c.vocab;
  f16* xa = b.x;
  e->prog.push_back(Op([=](hipStream_t s) { return embed_tokens(xa, ids, tok, pos, B, T, W, vocab, s); }, "embed_tokens"));
  const f16* x = clip_layers_push(*e, b, c.layers - e->skip_last, B, T, W, F, c.heads, /*causal=*/1, e->hidden_act ? 5 : 2);
  e->ln(b.a, x, W, e->ws.ptr<float>("final_layer_norm.weight"), e->ws.ptr<float>("final_layer_norm.bias"), rows, W);
  e->out16 = b.a;
  if (int rc = e->alloc_splitk()) return rc;
  e->batch = B;
  return 0;
}

}  // namespace

extern "C" {

int sdeo_clip_create(const sdeo_clip_config* cfg, sdeo_clip_handle* out) {
  SDEO_CHECK(cfg && out, "sdeo_clip_create: null argument");
  SDEO_CHECK(cfg->vocab > 0 && cfg->positions > 0 && cfg->layers > 0 && cfg->heads > 0 && cfg->ffn > 0, "sdeo_clip_create: empty config");
  SDEO_CHECK(cfg->width % 8 == 0 && cfg->ffn % 8 == 0 && cfg->width % cfg->heads == 0, "sdeo_clip_create: width %d / ffn %d must be multiples of 8, width divisible by heads %d",
             cfg->width, cfg->ffn, cfg->heads);
  const int d = cfg->width / cfg->heads;
  SDEO_CHECK(d % 8 == 0 && d <= 160, "sdeo_clip_create: head dim %d unsupported (multiple of 8, <= 160)", d);
  Clip* e = new Clip();
  e->cfg = *cfg;
  build_registry(e);
  return handle_created("sdeo_clip_create", e, out);
}

int sdeo_clip_destroy(sdeo_clip_handle h) { return handle_destroy(h); }

int sdeo_clip_num_weights(sdeo_clip_handle h) { return handle_num_weights(h); }

int sdeo_clip_weight_info(sdeo_clip_handle h, int i, const char** name, int64_t dims[2], int* ndim) {
  return handle_weight_info("sdeo_clip_weight_info", h, i, name, dims, 2, 0, ndim);
}

int sdeo_clip_load_weight(sdeo_clip_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict) {
  SDEO_CHECK(h && name && host_data && dims, "sdeo_clip_load_weight: null argument");
  return h->ws.load("sdeo_clip_load_weight", name, clip_key(name), host_data, dims, ndim, strict);
}

int sdeo_clip_finalize_weights(sdeo_clip_handle h) { return handle_finalize_weights("sdeo_clip_finalize_weights", h); }

int sdeo_clip_set_variant(sdeo_clip_handle h, int hidden_act, int skip_last_layers) {
  SDEO_CHECK(h, "sdeo_clip_set_variant: null handle");
  SDEO_CHECK(hidden_act == 0 || hidden_act == 1, "sdeo_clip_set_variant: hidden_act %d (0 quick-GELU, 1 erf GELU)", hidden_act);
  SDEO_CHECK(skip_last_layers >= 0 && skip_last_layers < h->cfg.layers, "sdeo_clip_set_variant: cannot skip %d of %d layers", skip_last_layers,
             h->cfg.layers);
  SDEO_CHECK(h->batch == 0, "sdeo_clip_set_variant: call it before sdeo_clip_configure");
  h->hidden_act = hidden_act;
  h->skip_last = skip_last_layers;
  return 0;
}

int sdeo_clip_configure(sdeo_clip_handle h, int batch) {
  SDEO_CHECK(h && h->finalized, "sdeo_clip_configure: weights not finalized");
  SDEO_CHECK(batch >= 1 && batch <= 64, "sdeo_clip_configure: batch=%d out of range", batch);
  return handle_configure(h, [&] { return configure_impl(h, batch); });
}

int sdeo_clip_encode(sdeo_clip_handle h, const int32_t* tokens, int batch, float* out, void* stream) {
  SDEO_CHECK(h && tokens && out, "sdeo_clip_encode: null argument");
  SDEO_CHECK(h->batch > 0 && batch == h->batch, "sdeo_clip_encode: batch %d != configured %d", batch, h->batch);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t rows = (size_t)batch * h->cfg.positions;
  SDEO_HIP(hipMemcpyAsync(h->tokens, tokens, rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (int rc = run_program(h->prog, s)) return rc;
  return f16_to_f32(out, h->out16, (int64_t)rows * h->cfg.width, s);
}

size_t sdeo_clip_device_bytes(sdeo_clip_handle h) { return handle_device_bytes(h); }

// ---- LoRA adapters.  The text tower runs on the raw tensors and caches nothing between encodes, so commit has
// nothing to rebuild or invalidate: it only lets the staging buffer go.
int sdeo_clip_lora_apply(sdeo_clip_handle h, const char* name, const float* down, const float* up, int rank, float scale, void* stream) {
  SDEO_CHECK(h, "sdeo_clip_lora_apply: null handle");
  return h->ws.lora_apply("sdeo_clip_lora_apply", name, clip_key(name), down, up, rank, scale,
                          h->finalized ? nullptr : "weights not finalized (call sdeo_clip_finalize_weights)", reinterpret_cast<hipStream_t>(stream));
}

int sdeo_clip_loha_apply(sdeo_clip_handle h, const char* name, const float* w1_a, const float* w1_b, const float* w2_a, const float* w2_b,
                         const float* t1, const float* t2, int rank, float scale, void* stream) {
  SDEO_CHECK(h, "sdeo_clip_loha_apply: null handle");
  return h->ws.loha_apply("sdeo_clip_loha_apply", name, clip_key(name), w1_a, w1_b, w2_a, w2_b, t1, t2, rank, scale,
                          h->finalized ? nullptr : "weights not finalized (call sdeo_clip_finalize_weights)", reinterpret_cast<hipStream_t>(stream));
}

int sdeo_clip_lokr_apply(sdeo_clip_handle h, const char* name, const float* w1, const float* w1_a, const float* w1_b, int rank1, const float* w2,
                         const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale, void* stream) {
  SDEO_CHECK(h, "sdeo_clip_lokr_apply: null handle");
  return h->ws.lokr_apply("sdeo_clip_lokr_apply", name, clip_key(name), w1, w1_a, w1_b, rank1, w2, w2_a, w2_b, t2, rank2, out_l, in_m, scale,
                          h->finalized ? nullptr : "weights not finalized (call sdeo_clip_finalize_weights)", reinterpret_cast<hipStream_t>(stream));
}

int sdeo_clip_lora_commit(sdeo_clip_handle h) {
  SDEO_CHECK(h, "sdeo_clip_lora_commit: null handle");
  SDEO_CHECK(h->finalized, "sdeo_clip_lora_commit: weights not finalized (call sdeo_clip_finalize_weights)");
  h->ws.lora_release_stage();
  return 0;
}

int sdeo_clip_lora_clear(sdeo_clip_handle h) {
  SDEO_CHECK(h, "sdeo_clip_lora_clear: null handle");
  SDEO_CHECK(h->finalized, "sdeo_clip_lora_clear: weights not finalized (call sdeo_clip_finalize_weights)");
  return h->ws.lora_restore();
}

int sdeo_clip_lora_touched(sdeo_clip_handle h) { return h ? h->ws.lora_touched() : 0; }

int sdeo_clip_read_weight(sdeo_clip_handle h, const char* name, float* out) {
  SDEO_CHECK(h, "sdeo_clip_read_weight: null handle");
  return h->ws.read("sdeo_clip_read_weight", name, clip_key(name), out);
}

}  // extern "C"
