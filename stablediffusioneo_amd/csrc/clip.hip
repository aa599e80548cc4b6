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
#include "handle_common.h"

using namespace sdeo;

struct sdeo_clip_handle_s {
  sdeo_clip_config cfg{};
  int hidden_act = 0, skip_last = 0;       // sdeo_clip_set_variant: erf GELU in the MLP; blocks at the end that are loaded but not run
  WeightStore ws;
  bool finalized = false;
  // configured state
  int batch = 0;
  char* act = nullptr;
  size_t act_bytes = 0;
  float* splitk_ws = nullptr;
  size_t splitk_bytes = 0;
  int32_t* tokens = nullptr;
  Program prog;
  f16* out16 = nullptr;
};

namespace {

typedef sdeo_clip_handle_s Clip;

// names follow the HuggingFace state dict below "text_model." (the SD checkpoint stores them as
// "cond_stage_model.transformer.text_model.*"; sdeo_clip_load_weight strips everything up to "text_model.")
static void build_registry(Clip* e) {
  const sdeo_clip_config& c = e->cfg;
  WeightStore& r = e->ws;
  const int W = c.width, F = c.ffn;
  auto mat = [&](const std::string& n, int rows, int cols, size_t off) { r.add(n, W_LINEAR, {rows, cols}, off); };
  auto vec = [&](const std::string& n, int len, size_t off) { r.add(n, W_VEC, {len}, off); };
  mat("embeddings.token_embedding.weight", c.vocab, W, r.take((size_t)c.vocab * W * 2));
  mat("embeddings.position_embedding.weight", c.positions, W, r.take((size_t)c.positions * W * 2));
  for (int l = 0; l < c.layers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    // q_proj, k_proj and v_proj stacked: one [3W][W] matrix and one [3W] bias (one GEMM; the attention kernel reads V row-major)
    const size_t qkv = r.take((size_t)3 * W * W * 2), qkvb = r.take((size_t)3 * W * 4);
    mat(p + "self_attn.q_proj.weight", W, W, qkv);
    mat(p + "self_attn.k_proj.weight", W, W, qkv + (size_t)W * W * 2);
    mat(p + "self_attn.v_proj.weight", W, W, qkv + (size_t)2 * W * W * 2);
    vec(p + "self_attn.q_proj.bias", W, qkvb);
    vec(p + "self_attn.k_proj.bias", W, qkvb + (size_t)W * 4);
    vec(p + "self_attn.v_proj.bias", W, qkvb + (size_t)2 * W * 4);
    mat(p + "self_attn.out_proj.weight", W, W, r.take((size_t)W * W * 2));
    vec(p + "self_attn.out_proj.bias", W, r.take((size_t)W * 4));
    vec(p + "layer_norm1.weight", W, r.take((size_t)W * 4));
    vec(p + "layer_norm1.bias", W, r.take((size_t)W * 4));
    mat(p + "mlp.fc1.weight", F, W, r.take((size_t)F * W * 2));
    vec(p + "mlp.fc1.bias", F, r.take((size_t)F * 4));
    mat(p + "mlp.fc2.weight", W, F, r.take((size_t)W * F * 2));
    vec(p + "mlp.fc2.bias", W, r.take((size_t)W * 4));
    vec(p + "layer_norm2.weight", W, r.take((size_t)W * 4));
    vec(p + "layer_norm2.bias", W, r.take((size_t)W * 4));
  }
  vec("final_layer_norm.weight", W, r.take((size_t)W * 4));
  vec("final_layer_norm.bias", W, r.take((size_t)W * 4));
}

static void free_configured(Clip* e) {
  if (e->act) (void)hipFree(e->act);
  if (e->splitk_ws) (void)hipFree(e->splitk_ws);
  if (e->tokens) (void)hipFree(e->tokens);
  e->act = nullptr; e->splitk_ws = nullptr; e->tokens = nullptr;
  e->prog.clear();
  e->batch = 0; e->splitk_bytes = 0;
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
  if (int rc = e->ws.alloc("sdeo_clip_create", /*zero_fill=*/false)) {
    delete e;
    return rc;
  }
  *out = e;
  return 0;
}

int sdeo_clip_destroy(sdeo_clip_handle h) {
  if (!h) return 0;
  free_configured(h);
  h->ws.destroy();
  delete h;
  return 0;
}

int sdeo_clip_num_weights(sdeo_clip_handle h) { return h ? (int)h->ws.entries.size() : 0; }

int sdeo_clip_weight_info(sdeo_clip_handle h, int i, const char** name, int64_t dims[2], int* ndim) {
  SDEO_CHECK(h && i >= 0 && i < (int)h->ws.entries.size() && name && dims && ndim, "sdeo_clip_weight_info: bad argument");
  h->ws.info(i, name, dims, 2, 0, ndim);
  return 0;
}

int sdeo_clip_load_weight(sdeo_clip_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict) {
  SDEO_CHECK(h && name && host_data && dims, "sdeo_clip_load_weight: null argument");
  std::string key(name);
  const size_t pos = key.find("text_model.");
  if (pos != std::string::npos) key = key.substr(pos + 11);
  return h->ws.load("sdeo_clip_load_weight", name, key, host_data, dims, ndim, strict);
}

int sdeo_clip_finalize_weights(sdeo_clip_handle h) {
  SDEO_CHECK(h, "sdeo_clip_finalize_weights: null handle");
  if (int rc = h->ws.require_all("sdeo_clip_finalize_weights")) return rc;
  h->finalized = true;
  return 0;
}

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
  free_configured(h);
  Clip* e = h;
  const sdeo_clip_config& c = e->cfg;
  const int B = batch, T = c.positions, W = c.width, F = c.ffn, H = c.heads, d = W / H;
  const int rows = B * T;
  // activation buffers (fp16): xa, xb, a [rows][W]; qkv [rows][3W]; o [rows][W]; hid [rows][F]
  size_t off = 0;
  auto take = [&](size_t elems) { const size_t o = align_up(off, 256); off = o + elems * 2; return o; };
  const size_t o_xa = take((size_t)rows * W), o_xb = take((size_t)rows * W), o_a = take((size_t)rows * W),
               o_qkv = take((size_t)rows * 3 * W), o_o = take((size_t)rows * W), o_h = take((size_t)rows * F);
  e->act_bytes = align_up(off, 256);
  SDEO_HIP(hipMalloc((void**)&e->act, e->act_bytes));
  SDEO_HIP(hipMemset(e->act, 0, e->act_bytes));
  SDEO_HIP(hipMalloc((void**)&e->tokens, (size_t)rows * sizeof(int32_t)));
  auto P = [&](size_t o) { return reinterpret_cast<f16*>(e->act + o); };
  f16 *xa = P(o_xa), *xb = P(o_xb), *a = P(o_a), *qkv = P(o_qkv), *o = P(o_o), *hid = P(o_h);

  auto gemm = [&](const f16* x, int K, const f16* w, int N, const float* bias, int act, const f16* res, f16* y) {
    ConvGemm p;
    p.x = x; p.w = w; p.y = y; p.bias = bias; p.res = res; p.ldres = N;
    p.B = rows; p.Cin = K; p.M = rows; p.N = N; p.K = K; p.ldx = K; p.ldw = K; p.ldy = N; p.act = act;
    e->prog.push_back(conv_gemm_op(p, WorkspaceRef{&e->splitk_ws, &e->splitk_bytes}, &e->splitk_bytes));
  };
  auto ln = [&](const f16* xi, const float* g, const float* b) {
    e->prog.push_back(Op([=](hipStream_t s) { return layernorm(a, W, xi, W, g, b, rows, W, 1e-5f, s); }, "layernorm", 0, 4.0 * rows * W));
  };
  auto wp = [&](const std::string& n) { return e->ws.ptr<f16>(n); };
  auto vp = [&](const std::string& n) { return e->ws.ptr<float>(n); };
  const f16* tok = wp("embeddings.token_embedding.weight");
  const f16* pos = wp("embeddings.position_embedding.weight");
  const int32_t* ids = e->tokens;
  const int vocab = c.vocab;
  e->prog.push_back(Op([=](hipStream_t s) { return embed_tokens(xa, ids, tok, pos, B, T, W, vocab, s); }, "embed_tokens"));
  f16* x = xa;
  f16* xn = xb;
  const float scale = 1.0f / sqrtf((float)d);
  const int mlp_act = e->hidden_act ? 5 : 2;
  for (int l = 0; l < c.layers - e->skip_last; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    ln(x, vp(p + "layer_norm1.weight"), vp(p + "layer_norm1.bias"));
    gemm(a, W, wp(p + "self_attn.q_proj.weight"), 3 * W, vp(p + "self_attn.q_proj.bias"), 0, nullptr, qkv);
    e->prog.push_back(Op([=](hipStream_t s) {
      return attention(o, W, qkv, 3 * W, qkv + W, 3 * W, qkv + 2 * W, 3 * W, B, H, T, T, T, T, d, scale, s, /*causal=*/1);
    }, "attention", 4.0 * B * H * (double)T * T * d, 2.0 * B * H * d * (2.0 * T + 2.0 * T)));
    gemm(o, W, wp(p + "self_attn.out_proj.weight"), W, vp(p + "self_attn.out_proj.bias"), 0, x, xn);
    std::swap(x, xn);
    ln(x, vp(p + "layer_norm2.weight"), vp(p + "layer_norm2.bias"));
    gemm(a, W, wp(p + "mlp.fc1.weight"), F, vp(p + "mlp.fc1.bias"), mlp_act, nullptr, hid);
    gemm(hid, F, wp(p + "mlp.fc2.weight"), W, vp(p + "mlp.fc2.bias"), 0, x, xn);
    std::swap(x, xn);
  }
  ln(x, vp("final_layer_norm.weight"), vp("final_layer_norm.bias"));
  e->out16 = a;
  if (e->splitk_bytes) SDEO_HIP(hipMalloc((void**)&e->splitk_ws, e->splitk_bytes));
  e->batch = B;
  return 0;
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

size_t sdeo_clip_device_bytes(sdeo_clip_handle h) { return h ? h->ws.slab_bytes + h->act_bytes + h->splitk_bytes + h->ws.lora_backup_bytes : 0; }

// ---- LoRA adapters.  The text tower runs on the raw tensors and caches nothing between encodes, so commit has
// nothing to rebuild or invalidate: it only lets the staging buffer go.
static std::string clip_key(const char* name) {
  std::string key(name ? name : "");
  const size_t pos = key.find("text_model.");
  return pos == std::string::npos ? key : key.substr(pos + 11);
}

int sdeo_clip_lora_apply(sdeo_clip_handle h, const char* name, const float* down, const float* up, int rank, float scale, void* stream) {
  SDEO_CHECK(h, "sdeo_clip_lora_apply: null handle");
  return h->ws.lora_apply("sdeo_clip_lora_apply", name, clip_key(name), down, up, rank, scale,
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
