// CLIP vision tower with projection (HuggingFace `CLIPVisionModelWithProjection`; OpenCLIP ViT-H/14 is the tower the ip-adapter_sd15
// files are trained against): a picture -> the image embedding `sdeo_set_ip_tokens`' projection starts from.  The published algorithm:
//   patches = conv(pixel_values, patch_embedding, stride = patch)            (no bias)        [P = (S / p)^2][W]
//   x = pre_layrnorm(cat(class_embedding, patches) + position_embedding)                      [T = P + 1][W]
//   per layer:  x += out_proj(softmax((q_proj(LN1 x) * d^-1/2) k_proj(LN1 x)^T) v_proj(LN1 x))         (no mask)
//               x += fc2(gelu_erf(fc1(LN2 x)))
//   image_embeds = visual_projection(post_layernorm(x[:, 0]))                (no bias)        [proj]
//   hidden_states[-2] = x in front of the last layer (un-normalised)
// It is the text tower's program (clip.hip) on the same kernels; what is new is everything in front of the transformer:
//   * CLIPImageProcessor on the device (sdeo_clip_image_preprocess_u8): PIL's integer bicubic resample of the shortest side to S, the
//     centre crop, 1/255, (v - mean) / std, written straight as the patch rows the patch GEMM reads;
//   * class token + position embedding + pre_layrnorm in one pass (embed_ln_kernel).
// Patch rows / patch matrix: one row per patch, Kp = 3 p^2 rounded up to a multiple of 8 columns (592 for p = 14), column
// k = (py * p + px) * 3 + c -- the order of the bytes of an HWC image, so a thread's 8 columns are 8 consecutive source bytes; columns
// >= 3 p^2 are zero on both sides.  K = 592 is no multiple of 64, so the patch GEMM runs the register-staged kernel, whose K-steps of 32
// mask their tail per 8-column chunk (conv_gemm.hip: kok).
#include "../../include/sdeo.h"
#include "clip_layers.h"

using namespace sdeo;

namespace {

// OPENAI_CLIP_MEAN / OPENAI_CLIP_STD, the constants of every CLIP preprocessor_config.json
__constant__ float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
__constant__ float kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

// CLIPImageProcessor's arithmetic on one 8-bit value (pinned against transformers 5.15): the rescale is a double product rounded to
// fp32, the normalisation two fp32 operations
__device__ __forceinline__ float clip_normalise(int u, int c) {
  const float v = (float)((double)u * (1.0 / 255.0));
  return (v - kClipMean[c]) / kClipStd[c];
}
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// horizontal pass of PIL's ImagingResample for the S columns of the crop and the source rows [row0, row0 + rows) the crop's rows tap:
// tmp[r][j][c] = clip8((2^21 + sum_t img[row0 + r][first[j] + t][c] * coef[j][t]) >> 22).  One thread per output byte (c fastest: a
// wave reads a contiguous run of source bytes per tap).  Table entries are clamped, so no table can make it read outside the image.
__global__ __launch_bounds__(256) void resample_h_kernel(uint8_t* __restrict__ tmp, const uint8_t* __restrict__ img, int iw, int S, int row0,
                                                         int rows, const int* __restrict__ first, const int* __restrict__ count,
                                                         const int* __restrict__ coef, int taps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * S * 3) return;
  const int c = i % 3, j = (i / 3) % S, r = i / (3 * S);
  const uint8_t* src = img + (size_t)(row0 + r) * iw * 3 + c;
  const int x0 = first[j], n = min(max(count[j], 0), taps);
  int acc = 1 << 21;
  for (int t = 0; t < n; ++t) acc += (int)src[(size_t)min(max(x0 + t, 0), iw - 1) * 3] * coef[j * taps + t];
  tmp[i] = (uint8_t)clip8(acc >> 22);
}

// vertical pass + crop output + normalisation + patchify: one thread per 8 columns of a patch row (one 16-byte store).  Columns
// >= 3 p^2 are written as zero.
__global__ __launch_bounds__(256) void resample_v_patchify_kernel(f16* __restrict__ rows_out, uint8_t* __restrict__ crop, const uint8_t* __restrict__ tmp,
                                                                  int S, int p, int Kp, int row0, int rows, const int* __restrict__ first,
                                                                  const int* __restrict__ count, const int* __restrict__ coef, int taps) {
  const int chunks = Kp / 8, g = S / p;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g * g * chunks) return;
  const int chunk = i % chunks, patch = i / chunks;
  const int gy = patch / g, gx = patch - gy * g;
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = chunk * 8 + e;
    float v = 0.f;
    if (k < 3 * p * p) {
      const int c = k % 3, px = (k / 3) % p, py = k / (3 * p);
      const int y = gy * p + py, x = gx * p + px;
      const int y0 = first[y], n = min(max(count[y], 0), taps);
      int acc = 1 << 21;
      for (int t = 0; t < n; ++t)
        acc += (int)tmp[((size_t)min(max(y0 + t - row0, 0), rows - 1) * S + x) * 3 + c] * coef[y * taps + t];
      const int u = clip8(acc >> 22);
      if (crop) crop[((size_t)y * S + x) * 3 + c] = (uint8_t)u;
      v = clip_normalise(u, c);
    }
    o[e] = (f16)v;
  }
  *reinterpret_cast<f16x8*>(rows_out + (size_t)patch * Kp + chunk * 8) = o;
}

// pixel_values fp32 NCHW [B][3][S][S] -> patch rows [B * P][Kp] fp16, the same column order
__global__ __launch_bounds__(256) void patchify_f32_kernel(f16* __restrict__ rows_out, const float* __restrict__ pix, int B, int S, int p, int Kp) {
  const int chunks = Kp / 8, g = S / p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * g * g * chunks) return;
  const int chunk = (int)(i % chunks);
  const int64_t row = i / chunks;
  const int patch = (int)(row % (g * g)), b = (int)(row / (g * g));
  const int gy = patch / g, gx = patch - gy * g;
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = chunk * 8 + e;
    float v = 0.f;
    if (k < 3 * p * p) {
      const int c = k % 3, px = (k / 3) % p, py = k / (3 * p);
      v = pix[(((size_t)b * 3 + c) * S + gy * p + py) * S + gx * p + px];
    }
    o[e] = (f16)v;
  }
  *reinterpret_cast<f16x8*>(rows_out + (size_t)row * Kp + chunk * 8) = o;
}

// embeddings.patch_embedding.weight fp32 [W][3][p][p] -> the [W][Kp] GEMM matrix in the patch rows' column order, pad columns zero
__global__ __launch_bounds__(256) void patch_weight_kernel(f16* __restrict__ w_out, const float* __restrict__ w, int W, int p, int Kp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)W * Kp) return;
  const int k = (int)(i % Kp), o = (int)(i / Kp);
  float v = 0.f;
  if (k < 3 * p * p) {
    const int c = k % 3, px = (k / 3) % p, py = k / (3 * p);
    v = w[(((size_t)o * 3 + c) * p + py) * p + px];
  }
  w_out[i] = (f16)v;
}

// x[b * T + t] = pre_layrnorm((t == 0 ? class_embedding : patches[b * P + t - 1]) + position_embedding[t]): the sum in fp32 as the
// published model forms it, LayerNorm two-pass in registers, one fp16 rounding.  One wave per row, 4 rows per block, W <= 2048.
__global__ __launch_bounds__(256) void embed_ln_kernel(f16* __restrict__ x, const float* __restrict__ patches, const float* __restrict__ cls,
                                                       const f16* __restrict__ pos, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       int rows, int T, int W, float eps) {
  constexpr int VPL = 8;             // 4-float vectors per lane: 64 * 8 * 4 = 2048 columns
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = row / T, t = row - b * T;
  const float* src = t == 0 ? cls : patches + ((size_t)b * (T - 1) + t - 1) * W;
  const int nvec = W / 4;
  f32x4 v[VPL];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      v[i] = *reinterpret_cast<const f32x4*>(src + vi * 4);
      const f16x4 pv = *reinterpret_cast<const f16x4*>(pos + (size_t)t * W + vi * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[i][j] += (float)pv[j]; s += v[i][j]; }
    }
  }
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; q += d * d; }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)W + eps);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gamma + vi * 4), bv = *reinterpret_cast<const f32x4*>(beta + vi * 4);
      f16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (f16)((v[i][j] - mean) * rstd * gv[j] + bv[j]);
      *reinterpret_cast<f16x4*>(x + (size_t)row * W + vi * 4) = o;
    }
  }
}

static inline int patch_kp(int patch) { return (int)align_up((size_t)3 * patch * patch, 8); }

static int preprocess_check(const char* who, const void* patch_rows, const uint8_t* img, int ih, int iw, int S, int patch, const int32_t* x_first,
                            const int32_t* x_count, const int32_t* x_coeffs, int x_taps, const int32_t* y_first, const int32_t* y_count,
                            const int32_t* y_coeffs, int y_taps, int src_row0, int src_rows, const void* workspace, size_t workspace_bytes) {
  SDEO_CHECK(patch_rows && img && x_first && x_count && x_coeffs && y_first && y_count && y_coeffs && workspace, "%s: null argument", who);
  SDEO_CHECK(ih >= 1 && iw >= 1 && ih <= 16384 && iw <= 16384, "%s: image %d x %d out of range (1..16384)", who, ih, iw);
  SDEO_CHECK(S >= 1 && S <= 1024 && patch >= 1 && S % patch == 0, "%s: crop size %d must be a multiple of the patch %d (and <= 1024)", who, S, patch);
  SDEO_CHECK(x_taps >= 1 && y_taps >= 1, "%s: empty coefficient tables (%d, %d taps)", who, x_taps, y_taps);
  SDEO_CHECK(src_row0 >= 0 && src_rows >= 1 && src_row0 + src_rows <= ih, "%s: source rows [%d, %d) are not inside the image's %d rows", who, src_row0,
             src_row0 + src_rows, ih);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(patch_rows) & 15) == 0, "%s: the patch rows must be 16-byte aligned", who);
  const size_t need = (size_t)src_rows * S * 3;
  SDEO_CHECK(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  return 0;
}

static int preprocess_launch(f16* patch_rows, uint8_t* crop, const uint8_t* img, int iw, int S, int patch, const int32_t* x_first, const int32_t* x_count,
                             const int32_t* x_coeffs, int x_taps, const int32_t* y_first, const int32_t* y_count, const int32_t* y_coeffs, int y_taps,
                             int src_row0, int src_rows, void* workspace, hipStream_t s) {
  uint8_t* tmp = static_cast<uint8_t*>(workspace);
  const int Kp = patch_kp(patch), g = S / patch;
  hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(src_rows * S * 3, 256)), dim3(256), 0, s, tmp, img, iw, S, src_row0, src_rows, x_first, x_count,
                     x_coeffs, x_taps);
  SDEO_HIP(hipGetLastError());
  hipLaunchKernelGGL(resample_v_patchify_kernel, dim3(cdiv(g * g * (Kp / 8), 256)), dim3(256), 0, s, patch_rows, crop, tmp, S, patch, Kp, src_row0,
                     src_rows, y_first, y_count, y_coeffs, y_taps);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace

struct sdeo_clip_vision_handle_s : ProgramHandle {
  sdeo_clip_vision_config cfg{};
  // configured state
  int batch = 0, want_hidden = 0;
  f16* rows = nullptr;           // patch rows [batch * P][Kp]: what the two ways in fill
  f16* keep = nullptr;           // want_hidden: the residual stream in front of the last layer [batch * T][W]
  float* out = nullptr;          // the caller's image_embeds of the encode under way (the projection GEMM writes it)
  unsigned filled = 0;           // bit b: slot b's patch rows were filled since the last encode

  void free_configured() {
    rows = nullptr; keep = nullptr;
    batch = 0; want_hidden = 0; filled = 0;
    ProgramHandle::free_configured();
  }
};

namespace {

typedef sdeo_clip_vision_handle_s Vis;
const char* const kPatchWeight = "embeddings.patch_embedding.weight";

static int tokens_of(const sdeo_clip_vision_config& c) { return (c.image / c.patch) * (c.image / c.patch) + 1; }

// names follow the HuggingFace state dict below "vision_model.", plus "visual_projection.weight"
static void build_registry(Vis* e) {
  const sdeo_clip_vision_config& c = e->cfg;
  WeightStore& r = e->ws;
  const int W = c.width, T = tokens_of(c);
  auto mat = [&](const std::string& n, int rows, int cols, size_t off) { r.add(n, W_LINEAR, {rows, cols}, off); };
  auto vec = [&](const std::string& n, int len, size_t off) { r.add(n, W_VEC, {len}, off); };
  vec("embeddings.class_embedding", W, r.take((size_t)W * 4));
  // stored [W][Kp] by sdeo_clip_vision_load_weight itself (patch_weight_kernel); WeightStore::load never sees it
  r.add(kPatchWeight, W_CONV, {W, 3, c.patch, c.patch}, r.take((size_t)W * patch_kp(c.patch) * 2));
  mat("embeddings.position_embedding.weight", T, W, r.take((size_t)T * W * 2));
  vec("pre_layrnorm.weight", W, r.take((size_t)W * 4));
  vec("pre_layrnorm.bias", W, r.take((size_t)W * 4));
  clip_layers_register(r, c.layers, W, c.ffn);
  vec("post_layernorm.weight", W, r.take((size_t)W * 4));
  vec("post_layernorm.bias", W, r.take((size_t)W * 4));
  mat("visual_projection.weight", c.proj, W, r.take((size_t)c.proj * W * 2));
}

// the body of sdeo_clip_vision_configure after its checks
static int configure_impl(Vis* e, int B, int want_hidden) {
  const sdeo_clip_vision_config& c = e->cfg;
  const int T = tokens_of(c), P = T - 1, W = c.width, F = c.ffn, Kp = patch_kp(c.patch);
  const int rows = B * T;
  // activation buffers: patch rows [B P][Kp] fp16; patches [B P][W] fp32; xa, xb, a [rows][W]; qkv [rows][3W]; o [rows][W]; hid [rows][F];
  // cls [B][W] fp16; keep [rows][W] (want_hidden)
  const size_t o_rows = e->take((size_t)B * P * Kp * 2), o_pe = e->take((size_t)B * P * W * 4), o_xa = e->take((size_t)rows * W * 2),
               o_xb = e->take((size_t)rows * W * 2), o_a = e->take((size_t)rows * W * 2), o_qkv = e->take((size_t)rows * 3 * W * 2),
               o_o = e->take((size_t)rows * W * 2), o_h = e->take((size_t)rows * F * 2), o_cls = e->take((size_t)B * W * 2),
               o_keep = want_hidden ? e->take((size_t)rows * W * 2) : 0;
  if (int rc = e->alloc_act()) return rc;
  const ClipLayerBufs b{e->at<f16>(o_xa), e->at<f16>(o_xb), e->at<f16>(o_a), e->at<f16>(o_qkv), e->at<f16>(o_o), e->at<f16>(o_h)};
  f16 *xa = b.x, *cls = e->at<f16>(o_cls);
  float* pe = e->at<float>(o_pe);
  e->rows = e->at<f16>(o_rows);
  e->keep = want_hidden ? e->at<f16>(o_keep) : nullptr;

  auto wp = [&](const std::string& n) { return e->ws.ptr<f16>(n); };
  auto vp = [&](const std::string& n) { return e->ws.ptr<float>(n); };
  // 1. patch GEMM: fp32 out, so the embedding sum below is formed from unrounded products
  e->gemm(e->rows, B * P, Kp, wp(kPatchWeight), W, nullptr, 0, nullptr, nullptr, pe);
  // 2. class token + position embedding + pre_layrnorm
  {
    const float *ce = vp("embeddings.class_embedding"), *g = vp("pre_layrnorm.weight"), *bt = vp("pre_layrnorm.bias");
    const f16* pos = wp("embeddings.position_embedding.weight");
    e->prog.push_back(Op([=](hipStream_t s) {
      hipLaunchKernelGGL(embed_ln_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, xa, pe, ce, pos, g, bt, rows, T, W, 1e-5f);
      SDEO_HIP(hipGetLastError());
      return 0;
    }, "embed_ln", 0, 4.0 * B * P * W + 2.0 * rows * W));
  }
  // 3. the text tower's layers without the mask, erf GELU; hidden_states[-2] is copied out in front of the last one (the ping-pong
  // buffers overwrite it)
  const f16* x = clip_layers_push(*e, b, c.layers, B, T, W, F, c.heads, /*causal=*/0, /*mlp_act=*/5, [&](int l, const f16* src) {
    if (!want_hidden || l != c.layers - 1) return;
    f16* keep = e->keep;
    e->prog.push_back(Op([=](hipStream_t s) {
      SDEO_HIP(hipMemcpyAsync(keep, src, (size_t)rows * W * 2, hipMemcpyDeviceToDevice, s));
      return 0;
    }, "keep_hidden", 0, 4.0 * rows * W));
  });
  // 4. post_layernorm over the class-token rows only (row stride T W)
  e->ln(cls, x, T * W, vp("post_layernorm.weight"), vp("post_layernorm.bias"), B, W);
  // 5. visual_projection, fp32 into the caller's buffer of this encode
  e->gemm(cls, B, W, wp("visual_projection.weight"), c.proj, nullptr, 0, nullptr, nullptr, nullptr, [e](ConvGemm& p) { p.y32 = e->out; });
  if (int rc = e->alloc_splitk()) return rc;
  e->batch = B;
  e->want_hidden = want_hidden ? 1 : 0;
  return 0;
}

}  // namespace

extern "C" {

size_t sdeo_clip_image_preprocess_workspace_bytes(int ih, int iw, int S) {
  (void)iw;
  return ih > 0 && S > 0 ? (size_t)ih * S * 3 : 0;
}

int sdeo_clip_image_preprocess_u8(void* patch_rows, uint8_t* crop_u8, const uint8_t* img_hwc, int ih, int iw, int S, int patch,
                                  const int32_t* x_first, const int32_t* x_count, const int32_t* x_coeffs, int x_taps, const int32_t* y_first,
                                  const int32_t* y_count, const int32_t* y_coeffs, int y_taps, int src_row0, int src_rows, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (int rc = preprocess_check("sdeo_clip_image_preprocess_u8", patch_rows, img_hwc, ih, iw, S, patch, x_first, x_count, x_coeffs, x_taps, y_first,
                                y_count, y_coeffs, y_taps, src_row0, src_rows, workspace, workspace_bytes))
    return rc;
  return preprocess_launch(static_cast<f16*>(patch_rows), crop_u8, img_hwc, iw, S, patch, x_first, x_count, x_coeffs, x_taps, y_first, y_count, y_coeffs,
                           y_taps, src_row0, src_rows, workspace, reinterpret_cast<hipStream_t>(stream));
}

int sdeo_clip_vision_create(const sdeo_clip_vision_config* cfg, sdeo_clip_vision_handle* out) {
  SDEO_CHECK(cfg && out, "sdeo_clip_vision_create: null argument");
  SDEO_CHECK(cfg->image > 0 && cfg->patch > 0 && cfg->width > 0 && cfg->layers > 0 && cfg->heads > 0 && cfg->ffn > 0 && cfg->proj > 0,
             "sdeo_clip_vision_create: empty config");
  SDEO_CHECK(cfg->image % cfg->patch == 0, "sdeo_clip_vision_create: image %d is no multiple of the patch %d", cfg->image, cfg->patch);
  SDEO_CHECK(cfg->image <= 1024, "sdeo_clip_vision_create: image %d > 1024 unsupported", cfg->image);
  SDEO_CHECK(cfg->width % 8 == 0 && cfg->ffn % 8 == 0 && cfg->proj % 8 == 0, "sdeo_clip_vision_create: width %d / ffn %d / proj %d must be multiples of 8",
             cfg->width, cfg->ffn, cfg->proj);
  SDEO_CHECK(cfg->width <= 2048, "sdeo_clip_vision_create: width %d > 2048 unsupported (LayerNorm)", cfg->width);
  SDEO_CHECK(cfg->width % cfg->heads == 0, "sdeo_clip_vision_create: width %d is not divisible by heads %d", cfg->width, cfg->heads);
  const int d = cfg->width / cfg->heads, T = tokens_of(*cfg);
  SDEO_CHECK(d % 8 == 0 && d <= 160 && attention_kernel_name(1, cfg->heads, T, T, d, 0) != nullptr,
             "sdeo_clip_vision_create: head dim %d unsupported (8..96 in steps of 8, 120, 128, 152, 160)", d);
  Vis* e = new Vis();
  e->cfg = *cfg;
  build_registry(e);
  return handle_created("sdeo_clip_vision_create", e, out);
}

int sdeo_clip_vision_destroy(sdeo_clip_vision_handle h) { return handle_destroy(h); }

int sdeo_clip_vision_num_weights(sdeo_clip_vision_handle h) { return handle_num_weights(h); }

int sdeo_clip_vision_weight_info(sdeo_clip_vision_handle h, int i, const char** name, int64_t dims[4], int* ndim) {
  return handle_weight_info("sdeo_clip_vision_weight_info", h, i, name, dims, 4, 1, ndim);
}

int sdeo_clip_vision_load_weight(sdeo_clip_vision_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict) {
  const char* who = "sdeo_clip_vision_load_weight";
  SDEO_CHECK(h && name && host_data && dims, "%s: null argument", who);
  const std::string key = registry_key(name, "vision_model.");
  if (key != kPatchWeight) return h->ws.load(who, name, key, host_data, dims, ndim, strict);
  WeightStore& r = h->ws;
  WEntry& w = r.entries[r.index.at(key)];
  SDEO_CHECK(ndim == 4, "%s: %s has %d dims, expected 4", who, name, ndim);
  for (int i = 0; i < 4; ++i) SDEO_CHECK(dims[i] == w.dims[i], "%s: %s dim %d is %lld, expected %lld", who, name, i, (long long)dims[i], (long long)w.dims[i]);
  const int W = h->cfg.width, p = h->cfg.patch, Kp = patch_kp(p);
  if (!r.stage) SDEO_HIP(hipMalloc((void**)&r.stage, r.stage_bytes));
  SDEO_HIP(hipMemcpy(r.stage, host_data, (size_t)W * 3 * p * p * sizeof(float), hipMemcpyDefault));
  hipLaunchKernelGGL(patch_weight_kernel, dim3((unsigned)cdiv64((int64_t)W * Kp, 256)), dim3(256), 0, 0, reinterpret_cast<f16*>(r.slab + w.off), r.stage, W, p, Kp);
  SDEO_HIP(hipGetLastError());
  SDEO_HIP(hipDeviceSynchronize());
  w.loaded = true;
  return 0;
}

int sdeo_clip_vision_finalize_weights(sdeo_clip_vision_handle h) { return handle_finalize_weights("sdeo_clip_vision_finalize_weights", h); }

int sdeo_clip_vision_configure(sdeo_clip_vision_handle h, int batch, int want_hidden) {
  SDEO_CHECK(h && h->finalized, "sdeo_clip_vision_configure: weights not finalized");
  SDEO_CHECK(batch >= 1 && batch <= 16, "sdeo_clip_vision_configure: batch=%d out of range (1..16)", batch);
  return handle_configure(h, [&] { return configure_impl(h, batch, want_hidden); });
}

int sdeo_clip_vision_set_pixels(sdeo_clip_vision_handle h, const float* pixel_values, int batch, void* stream) {
  SDEO_CHECK(h && pixel_values, "sdeo_clip_vision_set_pixels: null argument");
  SDEO_CHECK(h->batch > 0, "sdeo_clip_vision_set_pixels: the handle is not configured (call sdeo_clip_vision_configure)");
  SDEO_CHECK(batch == h->batch, "sdeo_clip_vision_set_pixels: batch %d != configured %d", batch, h->batch);
  const sdeo_clip_vision_config& c = h->cfg;
  const int Kp = patch_kp(c.patch), P = tokens_of(c) - 1;
  hipLaunchKernelGGL(patchify_f32_kernel, dim3((unsigned)cdiv64((int64_t)batch * P * (Kp / 8), 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     h->rows, pixel_values, batch, c.image, c.patch, Kp);
  SDEO_HIP(hipGetLastError());
  h->filled = (1u << batch) - 1u;
  return 0;
}

int sdeo_clip_vision_set_image_u8(sdeo_clip_vision_handle h, int slot, const uint8_t* img_hwc, int ih, int iw, const int32_t* x_first,
                                  const int32_t* x_count, const int32_t* x_coeffs, int x_taps, const int32_t* y_first, const int32_t* y_count,
                                  const int32_t* y_coeffs, int y_taps, int src_row0, int src_rows, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const char* who = "sdeo_clip_vision_set_image_u8";
  SDEO_CHECK(h, "%s: null handle", who);
  SDEO_CHECK(h->batch > 0, "%s: the handle is not configured (call sdeo_clip_vision_configure)", who);
  SDEO_CHECK(slot >= 0 && slot < h->batch, "%s: slot %d outside the configured batch %d", who, slot, h->batch);
  const sdeo_clip_vision_config& c = h->cfg;
  f16* dst = h->rows + (size_t)slot * (tokens_of(c) - 1) * patch_kp(c.patch);
  if (int rc = preprocess_check(who, dst, img_hwc, ih, iw, c.image, c.patch, x_first, x_count, x_coeffs, x_taps, y_first, y_count, y_coeffs, y_taps,
                                src_row0, src_rows, workspace, workspace_bytes))
    return rc;
  if (int rc = preprocess_launch(dst, nullptr, img_hwc, iw, c.image, c.patch, x_first, x_count, x_coeffs, x_taps, y_first, y_count, y_coeffs, y_taps,
                                 src_row0, src_rows, workspace, reinterpret_cast<hipStream_t>(stream)))
    return rc;
  h->filled |= 1u << slot;
  return 0;
}

int sdeo_clip_vision_encode(sdeo_clip_vision_handle h, int batch, float* image_embeds, float* hidden, void* stream) {
  const char* who = "sdeo_clip_vision_encode";
  SDEO_CHECK(h && image_embeds, "%s: null argument", who);
  SDEO_CHECK(h->finalized, "%s: weights not finalized (call sdeo_clip_vision_finalize_weights)", who);
  SDEO_CHECK(h->batch > 0, "%s: the handle is not configured (call sdeo_clip_vision_configure)", who);
  SDEO_CHECK(batch == h->batch, "%s: batch %d != configured %d", who, batch, h->batch);
  SDEO_CHECK(!hidden || h->want_hidden, "%s: hidden asked of a handle configured without want_hidden", who);
  const unsigned all = (1u << batch) - 1u;
  if ((h->filled & all) != all) {
    int miss = 0;
    while ((h->filled >> miss) & 1u) ++miss;
    return fail("%s: slot %d of %d was not filled since the last encode (sdeo_clip_vision_set_pixels / sdeo_clip_vision_set_image_u8)", who, miss, batch);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  h->out = image_embeds;
  if (int rc = run_program(h->prog, s)) return rc;
  h->filled = 0;
  if (hidden) return f16_to_f32(hidden, h->keep, (int64_t)batch * tokens_of(h->cfg) * h->cfg.width, s);
  return 0;
}

size_t sdeo_clip_vision_device_bytes(sdeo_clip_vision_handle h) { return handle_device_bytes(h); }

}  // extern "C"
