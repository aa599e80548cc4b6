// The CLIP encoder layer both towers run (clip.hip: text, causal; clip_vision.hip: vision, no mask), once: its tensors and its launches.
//   x += out_proj(softmax((q_proj(LN1 x) * d^-1/2) k_proj(LN1 x)^T) v_proj(LN1 x));  x += fc2(act(fc1(LN2 x)))
// Host code only.
#pragma once
#include <math.h>

#include "program_handle.h"

namespace sdeo {

// q_proj, k_proj and v_proj are stacked: one [3W][W] matrix and one [3W] bias (one GEMM; the attention kernel reads V row-major), which
// the program addresses by their first tensor
static const char* const kClipQkvWeight = "self_attn.q_proj.weight";
static const char* const kClipQkvBias = "self_attn.q_proj.bias";

// registers "encoder.layers.{l}.*" for l < layers under the HuggingFace names
static inline void clip_layers_register(WeightStore& r, int layers, int W, int F) {
  auto mat = [&](const std::string& n, int rows, int cols, size_t off) { r.add(n, W_LINEAR, {rows, cols}, off); };
  auto vec = [&](const std::string& n, int len, size_t off) { r.add(n, W_VEC, {len}, off); };
  for (int l = 0; l < layers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    const size_t qkv = r.take((size_t)3 * W * W * 2), qkvb = r.take((size_t)3 * W * 4);
    mat(p + kClipQkvWeight, W, W, qkv);
    mat(p + "self_attn.k_proj.weight", W, W, qkv + (size_t)W * W * 2);
    mat(p + "self_attn.v_proj.weight", W, W, qkv + (size_t)2 * W * W * 2);
    vec(p + kClipQkvBias, W, qkvb);
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
}

// fp16 buffers of the layer loop: the stream x and its ping-pong partner xn, a (LayerNorm output), o (attention output) [B T][W];
// qkv [B T][3W]; hid [B T][F]
struct ClipLayerBufs { f16 *x, *xn, *a, *qkv, *o, *hid; };

// Pushes layers [0, n) onto e.prog and returns the buffer the stream is in afterwards (b.x or b.xn).  mlp_act: the ConvGemm::act code
// of fc1 (2 quick-GELU, 5 erf GELU); before(l, x), when set, runs in front of layer l with the stream's buffer.
static inline f16* clip_layers_push(ProgramHandle& e, ClipLayerBufs b, int n, int B, int T, int W, int F, int H, int causal, int mlp_act,
                                    const std::function<void(int, const f16*)>& before = nullptr) {
  const int rows = B * T, d = W / H;
  const float scale = 1.0f / sqrtf((float)d);
  f16 *x = b.x, *xn = b.xn, *a = b.a, *qkv = b.qkv, *o = b.o, *hid = b.hid;
  for (int l = 0; l < n; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    auto wp = [&](const char* t) { return e.ws.ptr<f16>(p + t); };
    auto vp = [&](const char* t) { return e.ws.ptr<float>(p + t); };
    if (before) before(l, x);
    e.ln(a, x, W, vp("layer_norm1.weight"), vp("layer_norm1.bias"), rows, W);
    e.gemm(a, rows, W, wp(kClipQkvWeight), 3 * W, vp(kClipQkvBias), 0, nullptr, qkv);
    e.prog.push_back(Op([=](hipStream_t s) {
      return attention(o, W, qkv, 3 * W, qkv + W, 3 * W, qkv + 2 * W, 3 * W, B, H, T, T, T, T, d, scale, s, causal);
    }, "attention", 4.0 * B * H * (double)T * T * d, 2.0 * B * H * d * (2.0 * T + 2.0 * T)));
    e.gemm(o, rows, W, wp("self_attn.out_proj.weight"), W, vp("self_attn.out_proj.bias"), 0, x, xn);
    std::swap(x, xn);
    e.ln(a, x, W, vp("layer_norm2.weight"), vp("layer_norm2.bias"), rows, W);
    e.gemm(a, rows, W, wp("mlp.fc1.weight"), F, vp("mlp.fc1.bias"), mlp_act, nullptr, hid);
    e.gemm(hid, rows, F, wp("mlp.fc2.weight"), W, vp("mlp.fc2.bias"), 0, x, xn);
    std::swap(x, xn);
  }
  return x;
}

}  // namespace sdeo
