/* libsdeo -- C ABI of the MI355X-native ControlNet / Stable-Diffusion hot path.
 *
 * This is the drop-in boundary for the reference's TensorRT seam.  Paths below are relative to the
 * reference tree (MarToonLi/StableDiffusionEO).
 *
 *   reference seam                                               replaced by
 *   ------------------------------------------------------------ ------------------------------------
 *   Engine.load / activate / allocate_buffers (Engine.py:99-121)  sdeo_create, sdeo_load_weight,
 *                                                                 sdeo_finalize_weights, sdeo_configure
 *   context.set_tensor_address + execute_async_v3                 sdeo_controlnet_forward, sdeo_unet_forward,
 *     (Engine.py:136-137,145,155-157) for ControlNet.plan /       sdeo_vae_decode, sdeo_apply_model
 *     ControlledUnet.plan / Decoder.plan
 *   cudaStreamBeginCapture / cudaGraphLaunch (Engine.py:139-152)  every call is capturable by the caller's hipGraph
 *   p_sample_ddim tail in torch (cldm/ddim_hacked.py:192,208-231) sdeo_cfg_ddim_step
 *   GroupNormPlugin::enqueue (plugin/groupNormPlugin/              sdeo_groupnorm_nhwc_f16
 *     groupNormPlugin.cpp:179-228), libplugin.so via ctypes.CDLL
 *     (onnx2trt_static_plugin.py:7-10)
 *   CUASSERT / "ERROR: inference failed." (Engine.py:38-44,146)   int return codes + sdeo_last_error()
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; sdeo_last_error() returns the message of
 *     the calling thread's last failure (the Python Engine maps non-zero to the reference's
 *     ValueError("ERROR: inference failed.")).
 *   - all pointers are raw DEVICE pointers unless a parameter name starts with `host_`; `stream` is a
 *     hipStream_t passed as void* (NULL = default stream).  Nothing here synchronises, allocates or frees
 *     caller memory, so every call is hipGraph-capturable.
 *   - fp16 activations are NHWC ("pixel rows" of `ld*` elements); the NCHW fp32 tensors of the reference
 *     surface are converted at the net-level entry points.
 *   - a handle is not thread-safe (same as a TensorRT execution context); one handle per GPU / process.
 */
#ifndef SDEO_H
#define SDEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdeo_handle_s* sdeo_handle;

const char* sdeo_last_error(void);
/* ABI version: bumped whenever the meaning of an argument of an existing entry point changes (not only its C type), so that a binding
 * built against an older header fails loudly instead of computing with re-interpreted operands.
 *   100  first release
 *   101  sdeo_attention_f16 / sdeo_attention_causal_f16: arguments 7, 8, 14 are V ROW-MAJOR with its row stride and per-batch row count
 *        (they were V transposed, ldvt and the batch stride of V^T) */
#define SDEO_ABI_VERSION 101
int sdeo_version(void);
/* GEMM plan table: (tile, split-K) per problem shape key {M,N,K,Cin,R,stride,ups,Hi,Wi,B}.  Known shapes come from the
 * table, which stablediffusioneo_amd/tuned_plans_gfx950.json pre-loads so that runs are reproducible and start fast;
 * unknown shapes use the deterministic heuristic (SDEO_AUTOTUNE=1 measures them on the device at sdeo_configure instead:
 * a tuning aid, plans and hence fp32 summation orders may then differ from run to run). */
void sdeo_set_tuned_gemm_plan(const int* key10, int tile, int splitk);
const char* sdeo_tuned_gemm_plans_json(void);

/* ------------------------------------------------------------------ op-level entry points (used by tests)

 * GroupNorm(+Swish) on NHWC fp16 -- operand contract of the reference plugin (x/y fp16 NHWC, gamma/beta fp32,
 * attrs epsilon + bSwish, groupNormPlugin.cpp:136-160,291-292) with epsilon actually applied.
 * workspace: >= sdeo_groupnorm_workspace_bytes(n, h*w, groups) bytes. */
size_t sdeo_groupnorm_workspace_bytes(int n, int hw, int groups);
int sdeo_groupnorm_nhwc_f16(void* y, const void* x, const float* gamma, const float* beta, int n, int h, int w, int c,
                            int groups, float eps, int with_swish, void* workspace, void* stream);

/* FreeU on one decoder concat buffer, in place (steps 2 and 3 of the definition at sdeo_set_freeu; the stage rule is the caller's).
 * buf: fp16 NHWC [n * h * w][ld], 16-byte aligned; h in columns [0, c_h), the skip in [c_h, c_h + c_skip); columns from c_h / 2 to c_h
 * and from c_h + c_skip on are not touched.  c_h % 16 == 0, c_skip % 8 == 0, ld % 8 == 0, ld >= c_h + c_skip, h and w at most 512.
 * b, s in [0, SDEO_FREEU_MAX]; version 1 or 2.  b == 1 leaves the h half bit for bit as it is, s == 1 the skip half.
 * workspace: >= sdeo_freeu_workspace_bytes(n, h, w) bytes (the version-2 mean map; may be NULL for version 1 or b == 1).
 * Two launches at most (version 1: one), no allocation, no synchronisation: capturable. */
size_t sdeo_freeu_workspace_bytes(int n, int h, int w);
int sdeo_freeu_nhwc_f16(void* buf, int ld, int n, int h, int w, int c_h, int c_skip, float b, float s, int version, void* workspace,
                        void* stream);

/* conv2d on NHWC fp16 activations with KRSC fp16 weights (implicit GEMM on MFMA).
 *   y[n][ho][wo][cout] = act( conv(x, w) + bias[cout] + bias2[n][cout] ) * scale + res[n][ho][wo][cout]
 * cin/cout are the STORED channel counts (cin % 8 == 0, cout % 4 == 0); upsample2x=1 folds a nearest x2
 * upsample of x in front of the conv.  bias/bias2 fp32 or NULL, res fp16 NHWC or NULL. act: 0 none, 1 SiLU,
 * 4 ReLU (plans exactly like act 0).  sdeo_conv2d_pad_nhwc_f16 and sdeo_gemm_f16 take the same codes (sdeo_gemm_f16 also 2 = quick-GELU
 * and 5 = erf GELU, F.gelu's default, planned like act 0).
 * workspace (split-K partials): >= sdeo_conv2d_workspace_bytes(...) bytes, may be NULL when that is 0. */
size_t sdeo_conv2d_workspace_bytes(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x);
int sdeo_conv2d_nhwc_f16(void* y, const void* x, const void* w_krsc, const float* bias, const float* bias2, const void* res,
                         int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int act, float scale,
                         void* workspace, size_t workspace_bytes, void* stream);

/* sdeo_conv2d_nhwc_f16 with explicit zero padding: pad_before rows / columns at the top / left, pad_after at the bottom / right
 * (each < ksize; pad_before = pad_after = ksize / 2 is exactly sdeo_conv2d_nhwc_f16, same plan, same bits).  ho = (h' + pad_before +
 * pad_after - ksize) / stride + 1 with h' = h or 2h (upsample2x), likewise wo.  The VAE encoder's Downsample (F.pad(x, (0,1,0,1)) then
 * conv3x3 stride 2 pad 0, ldm/modules/diffusionmodules/model.py:78-86) is ksize 3, stride 2, pad_before 0, pad_after 1.  1x1 filters take
 * symmetric padding only.  workspace: >= sdeo_conv2d_pad_workspace_bytes(...) bytes. */
size_t sdeo_conv2d_pad_workspace_bytes(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int pad_before,
                                       int pad_after);
int sdeo_conv2d_pad_nhwc_f16(void* y, const void* x, const void* w_krsc, const float* bias, const float* bias2, const void* res,
                             int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int pad_before, int pad_after,
                             int act, float scale, void* workspace, size_t workspace_bytes, void* stream);

/* GEMM  y[m][n] = act(x[m][k] . w[n][k]^T + bias) * scale + res   (both operands K-contiguous; nn.Linear layout).
 * out_f32=1 writes fp32.  bias_per_row=1 indexes bias by m.  ld* in elements. */
size_t sdeo_gemm_workspace_bytes(int m, int n, int k);
int sdeo_gemm_f16(void* y, int ldy, const void* x, int ldx, const void* w, int ldw, const float* bias, const void* res,
                  int ldres, int m, int n, int k, int act, float scale, int out_f32, int bias_per_row, void* workspace,
                  size_t workspace_bytes, void* stream);

/* LayerNorm over the last dim of [rows][c] fp16, fp32 gamma/beta. */
int sdeo_layernorm_f16(void* y, const void* x, const float* gamma, const float* beta, int rows, int c, float eps,
                       void* stream);

/* Fused attention O = softmax(Q K^T scale) V.  Q [b][tq][ldq], K [b][tk_stride][ldk], V [b][v_batch_stride][ldv] (all
 * row-major, head h at column h*d: column blocks of one fused q/k/v projection work as they are);  O [b][tq][ldo].
 * Keys >= tk are masked.  Operands 16-byte aligned, ld* multiples of 8.  Head dim d: 8..96 in steps of 8, 120, 128, 152, 160 (the UNet /
 * ControlNet / CLIP heads), or 256 / 512 (the VAE AttnBlock's single head, `ldm/modules/diffusionmodules/model.py:179-203`:
 * the four waves of a workgroup split the channels); scores are never materialised for any of them. */
int sdeo_attention_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int b,
                       int heads, int tq, int tk, int tk_stride, int v_batch_stride, int d, float scale, void* stream);

/* O = softmax(Q K^T scale) V + weight2 * softmax(Q K2^T scale) V2: two key sets, two softmaxes, one launch.
 * The decoupled cross-attention of an image-prompt adapter: K / V are the text keys, K2 / V2 a few image tokens.  Q, K, V, O as
 * sdeo_attention_f16 takes them; K2 [b][tk2_stride][ldk2], V2 [b][v2_batch_stride][ldv2], 1 <= tk2 <= 64, keys >= tk2 masked.  Both
 * normalised terms and their sum are formed in fp32 and rounded to fp16 once; weight2 = 0 gives the bits of sdeo_attention_f16 wherever
 * that runs its one-wave-per-query-block form (tk < 128, or d >= 88).  Head dim d: 8..96 in steps of 8, 120, 128, 152, 160.
 * Refused before any device call, each with its own message: a null operand, tk2 outside 1..64, a non-finite weight2, another head
 * dim, operands that are not 16-byte aligned or ld* that are no multiples of 8 (ldo: 4). */
int sdeo_attention2_f16(void* o, int ldo, const void* q, int ldq,
                        const void* k, int ldk, const void* v, int ldv, int tk, int tk_stride, int v_batch_stride,
                        const void* k2, int ldk2, const void* v2, int ldv2, int tk2, int tk2_stride, int v2_batch_stride,
                        float weight2, int b, int heads, int tq, int d, float scale, void* stream);

/* as sdeo_attention_f16 with the causal mask of the CLIP text transformer: key j is masked for query t when j > t
 * (needs tq == tk) */
int sdeo_attention_causal_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int b,
                              int heads, int tq, int tk, int tk_stride, int v_batch_stride, int d, float scale,
                              void* stream);

/* GEGLU: y[r][0:c] = a[r][0:c] * gelu_erf(a[r][c:2c]) */
int sdeo_geglu_f16(void* y, const void* a, int rows, int c, void* stream);

/* sinusoidal timestep embedding (util.py:154-174): t int64[b] -> out fp16 [b][dim] */
int sdeo_timestep_embedding_f16(void* out, const int64_t* t, int b, int dim, void* stream);

/* classifier-free guidance + DDIM update on fp32 latents (ddim_hacked.py:192,208-231).
 * eps_u may be NULL (no guidance), noise may be NULL (eta = 0), pred_x0 may be NULL. */
int sdeo_cfg_ddim_step(float* x_prev, float* pred_x0, const float* x, const float* eps_c, const float* eps_u,
                       const float* noise, float cfg_scale, float a_t, float a_prev, float sigma_t,
                       float sqrt_one_minus_at, int64_t n, void* stream);
/* The same step for a v-prediction model (SD-2.x 768-v; ddim_hacked.py:194-197,214-217 with upstream LatentDiffusion's
 * predict_eps_from_z_and_v / predict_start_from_z_and_v): the operands in the places of eps_c / eps_u are the model's v outputs.
 *   v = v_u + cfg_scale (v_c - v_u);  e = sqrt(a_t) v + sqrt(1 - a_t) x;  pred_x0 = sqrt(a_t) x - sqrt(1 - a_t) v;
 *   x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma_t^2) e + sigma_t noise */
int sdeo_cfg_ddim_step_v(float* x_prev, float* pred_x0, const float* x, const float* v_c, const float* v_u,
                         const float* noise, float cfg_scale, float a_t, float a_prev, float sigma_t,
                         float sqrt_one_minus_at, int64_t n, void* stream);

/* CFG + one linear-multistep update on fp32 latents: D as pred_x0 of sdeo_cfg_ddim_step(_v) (flags & SDEO_STEP_V_PREDICTION),
 * x_next = k_x x + k_d D + k_p d(on entry); d receives D.  m_u may be NULL; d may be NULL only when k_p == 0.
 * DPM-Solver++(2M) (Lu et al. 2022) with alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma), h = lambda_next - lambda_t,
 * phi = -expm1(-h), r = h_prev / h:  k_x = sigma_next / sigma_t, k_d = alpha_next phi (1 + 1 / (2r)), k_p = -alpha_next phi / (2r);
 * first order: k_d = alpha_next phi, k_p = 0 (the eta = 0 DDIM step).  The host computes the coefficients; the kernel never sees lambda. */
int sdeo_cfg_dpmpp_2m_step(float* x_next, float* d, const float* x, const float* m_c, const float* m_u, float cfg_scale, float a_t,
                           float sqrt_one_minus_at, float k_x, float k_d, float k_p, int flags, int64_t n, void* stream);

/* The stochastic member of the same family, DPM-Solver++(2M) SDE: sdeo_cfg_dpmpp_2m_step with a fourth term,
 *   x_next = k_x x + k_d D + k_p D_prev + k_n noise,   d <- D,
 * noise fp32, n elements like x; the host folds exp(-eta h) and the noise level into the four coefficients (cldm/dpm_solver.py,
 * sde_coefficients).  noise may be NULL only when k_n == 0: then this IS sdeo_cfg_dpmpp_2m_step (the same launch, the same bits).  A
 * null noise with k_n != 0 and a non-finite k_n are refused before any device call, next to what sdeo_cfg_dpmpp_2m_step refuses. */
int sdeo_cfg_dpmpp_2m_sde_step(float* x_next, float* d, const float* x, const float* m_c, const float* m_u, const float* noise,
                               float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, float k_n,
                               int flags, int64_t n, void* stream);

/* The sampler's mask / x0 blend (cldm/ddim_hacked.py:154-157: img = q_sample(x0, t) * mask + (1 - mask) * img) on fp32 NCHW latents,
 * IN PLACE on x:   x <- mask * (sqrt_a * orig + sqrt_one_minus_a * noise) + (1 - mask) * x
 *   x, orig, noise [n][c][hw];  mask [mask_n][mask_c][hw] with mask_n in {1, n} and mask_c in {1, c} (the broadcasts torch allows a
 *   (b|1, 1|C, h, w) mask);  sqrt_a / sqrt_one_minus_a: the fp32 entries of sqrt_alphas_cumprod[t] / sqrt_one_minus_alphas_cumprod[t],
 *   the tables q_sample reads (nothing is recomputed from alpha on the device).
 * Every operation rounds once, in the order of the torch expression (two products and a sum for q_sample, then q * mask, 1 - mask,
 * (1 - mask) * x and a sum; no fused multiply-add), so the result is bit-equal to it.  Null pointers and a mask_n / mask_c outside the
 * allowed values are refused before any device call, each with its own message. */
int sdeo_mask_blend(float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c, float sqrt_a,
                    float sqrt_one_minus_a, int n, int c, int hw, void* stream);

/* Inpainting composite on uint8 NHWC images [h][w][c] (c in 1..4, any h, w >= 1) with a uint8 mask [h][w], integer arithmetic:
 *   dst = (gen * m + orig * (255 - m) + 127) / 255        (m = 255: gen, m = 0: orig, exactly).  dst may be gen or orig. */
int sdeo_composite_u8(uint8_t* dst, const uint8_t* gen, const uint8_t* orig, const uint8_t* mask, int h, int w, int c, void* stream);

/* Canny edge map: replaces `cv2.Canny(img, low_threshold, high_threshold)` of annotator/canny/__init__.py:4-6
 * (aperture 3, L1 gradient magnitude; called at canny2image_torch.py:33 on the HWC3 uint8 image) and the control preparation of
 * canny2image_torch.py:34-38.  img_hwc: device uint8 [h][w][c], c in 1..4.  edges (optional): device uint8 [h][w], 0 / 255.
 * control_chw (optional): device fp32 [3][h][w] = edges / 255 on three identical channels (HWC3 + /255 + HWC->CHW).
 * workspace: >= sdeo_canny_workspace_bytes(h, w) bytes of device memory, 4-byte aligned.  Asynchronous on `stream` and
 * hipGraph-capturable like every other entry point (hysteresis is a union-find labelling, not a host-driven iteration). */
size_t sdeo_canny_workspace_bytes(int h, int w);
int sdeo_canny_u8(const uint8_t* img_hwc, int h, int w, int c, float low_threshold, float high_threshold, uint8_t* edges,
                  float* control_chw, void* workspace, size_t workspace_bytes, void* stream);

/* cv2.resize(img, (dst_w, dst_h), interpolation) of annotator/util.py:37 for 8-bit HWC images (c in 1..4), both on the device.
 * The per-axis coefficient tables depend only on the sizes and are built by the host (stablediffusioneo_amd/annotator/util.py):
 *   INTER_LANCZOS4: per destination index the first of its 8 taps (may be negative: indices are clamped to the image) and the
 *     8 coefficients as OpenCV stores them (short, x 2048);
 *   INTER_AREA: per destination index a run [start[d], start[d+1]) of (source index, float weight) pairs. */
int sdeo_resize_lanczos4_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dst_h, int dst_w, const int32_t* x_first_tap,
                            const int16_t* x_coeffs, const int32_t* y_first_tap, const int16_t* y_coeffs, void* stream);
int sdeo_resize_area_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dst_h, int dst_w, const int32_t* x_start,
                        const int32_t* x_index, const float* x_weight, const int32_t* y_start, const int32_t* y_index,
                        const float* y_weight, void* stream);
/* INTER_AREA when both axes shrink by INTEGER factors (h % dst_h == 0, w % dst_w == 0; error otherwise): OpenCV's resizeAreaFast_
 * arithmetic -- 2 x 2 cells (a + b + c + d + 2) >> 2, other cells the integer cell sum times the float 1 / area, ties to even.  No
 * tables.  (cv2.resize picks this path by itself; stablediffusioneo_amd/annotator/util.py: resize_u8 does the same.) */
int sdeo_resize_area_fast_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dst_h, int dst_w, void* stream);

/* layout helpers at the NCHW boundary */
int sdeo_nchw_f32_to_nhwc_f16(void* y, int ldy, const float* x, int n, int c, int hw, void* stream);
int sdeo_nhwc_f16_to_nchw_f32(float* y, const void* x, int ldx, int n, int c, int hw, float scale, void* stream);
int sdeo_oihw_f32_to_krsc_f16(void* y, const float* w, int o, int i, int r, int s, int i_pad, void* stream);

/* The kernel of sdeo_lora_apply on one stored tensor (csrc/lora.hip):  w[o][j] <- fp16(fp32(w[o][j]) + scale * sum_r up[o][r] down[r][j]).
 * kind: how the tensor is stored -- 1 = matrix [out][in]; 0 = KRSC conv weight [out][k][k][ipad], down in [in][k][k] order, the pad
 * channels in..ipad-1 neither read nor written; 3 = the GEGLU projection [out = 2H][in] with its value / gate rows interleaved in blocks
 * of 16 (H % 16 == 0).  k = 1 for matrices; ipad is read for kind 0 only.  up [out][rank], down [rank][in * k * k]: fp32, host or device
 * pointers (staged with hipMemcpyDefault).  rank 1..1024, scale finite.  Allocates, synchronises `stream` and frees: not capturable. */
int sdeo_lora_merge_f16(void* w, int kind, int out, int in, int k, int ipad, const float* down, const float* up, int rank, float scale,
                        void* stream);
/* The kernels of sdeo_loha_apply / sdeo_lokr_apply on one stored tensor (csrc/lora.hip); w, kind, out, in, k, ipad as above, the forms
 * and the operands as defined at sdeo_loha_apply below: fp32, host or device pointers, in the layout the file holds them, absent
 * operands null.  w <- fp16(fp32(w) + scale * dW), the multiplier alpha / rank already inside `scale`.  Every refusal (a null w, a bad
 * kind / shape, a missing or mixed operand set, a rank outside 1..1024, factor shapes that do not fit the tensor, a non-finite scale)
 * comes before any device call.  Allocate, synchronise `stream` and free: not capturable. */
int sdeo_loha_merge_f16(void* w, int kind, int out, int in, int k, int ipad, const float* w1_a, const float* w1_b, const float* w2_a,
                        const float* w2_b, const float* t1, const float* t2, int rank, float scale, void* stream);
int sdeo_lokr_merge_f16(void* w, int kind, int out, int in, int k, int ipad, const float* w1, const float* w1_a, const float* w1_b, int rank1,
                        const float* w2, const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale,
                        void* stream);

/* ------------------------------------------------------------------ net-level entry points */

typedef struct sdeo_config {
  /* UNet / ControlNet (cldm_v15.yaml values) */
  int in_channels, out_channels, hint_channels, model_channels, num_res_blocks;
  int channel_mult[8];
  int num_levels;
  int attention_resolutions[8];
  int num_attention_resolutions;
  int num_heads, context_dim, context_len;
  /* VAE decoder */
  int vae_ch, vae_out_ch, vae_ch_mult[8], vae_num_levels, vae_num_res_blocks, vae_z_channels;
  float vae_scale_factor;
} sdeo_config;

/* Create / destroy an engine instance on the current HIP device. */
int sdeo_create(const sdeo_config* cfg, sdeo_handle* out);
/* The layout switches of the SD-2.x family (cldm_v21.yaml; cldm/cldm.py:64,77,184-207, ldm/modules/attention.py:409-449), kept out of
 * sdeo_config so that its layout does not change.  sdeo_create(cfg, out) is sdeo_create_ex(cfg, NULL, out).  Checked before any
 * device call, each with its own message: num_head_channels divides the channel count of every attention block, and is a head dim
 * sdeo_attention_f16 accepts. */
typedef struct sdeo_config_ext {
  int size;                        /* = sizeof(sdeo_config_ext), checked */
  int num_head_channels;           /* 0 / -1 = use cfg->num_heads; else heads = C / num_head_channels per block */
  int use_linear_in_transformer;   /* 0 = conv1x1 proj_in / proj_out, weights (C,C,1,1); 1 = nn.Linear, weights (C,C) */
} sdeo_config_ext;
int sdeo_create_ex(const sdeo_config* cfg, const sdeo_config_ext* ext, sdeo_handle* out);
int sdeo_destroy(sdeo_handle h);

/* Weights: one call per checkpoint tensor, names exactly as in the reference state dict
 * ("model.diffusion_model.*", "control_model.*", "first_stage_model.*"; cldm/model.py:12-21).
 * host_data points to fp32 data in PyTorch layout (OIHW conv, [out][in] linear); it may be a host OR a device
 * pointer (copied with hipMemcpyDefault).
 * Unknown names return 0 and are ignored when `strict` is 0.  After the last tensor call
 * sdeo_finalize_weights (fails listing what is missing). */
int sdeo_load_weight(sdeo_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict);
int sdeo_finalize_weights(sdeo_handle h);
/* Weight precision of the UNet / ControlNet matrices (the reference's switch is the TensorRT builder flag,
 * onnx2trt_static_plugin.py:40-42): 16 = fp16 (default), 8 = OCP e4m3fn with one power-of-two scale per output channel, packed by
 * sdeo_finalize_weights; activations, accumulation, biases, norms and the VAE stay as they are.  Call before
 * sdeo_finalize_weights.  The weight-bound shapes (<= 512 rows) stream the one-byte codes; every other kernel reads an fp16 copy
 * holding the same dequantised values. */
int sdeo_set_weight_precision(sdeo_handle h, int bits);
/* Activation precision of the large GEMMs (Linear / conv1x1 with >= min_rows rows and K a multiple of 128), meaningful with 8-bit
 * weights only: 16 = fp16 activations (default); 8 = block-scaled fp8 on both sides -- the activations are packed to e4m3fn codes with
 * one e8m0 scale per 32 channels right in front of the GEMM, the matrix is packed the same way by sdeo_finalize_weights, and the
 * product runs on the block-scaled fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, twice the fp16 rate).  The GEMMs that consume a
 * LayerNorm (to_q / k / v, ff.net.0: the norm is folded into them and they read the raw rows) keep fp16 activations: e4m3 rounds a
 * row relative to its mean, which the fold cannot cancel.  Everything else (3x3 convs, attention, small GEMMs, norms, VAE) stays
 * as with sdeo_set_weight_precision(h, 8).  Call before sdeo_finalize_weights.
 * min_rows <= 0 selects the default threshold (2048). */
int sdeo_set_activation_precision(sdeo_handle h, int bits, int min_rows);
/* Number of expected tensors and the i-th expected name/shape (ndim<=4), for loaders and tests. */
int sdeo_num_weights(sdeo_handle h);
int sdeo_weight_info(sdeo_handle h, int i, const char** name, int64_t dims[4], int* ndim);

/* Image-prompt adapter (IP-Adapter, decoupled cross-attention): every UNet cross-attention gets a second key / value projection over
 * num_tokens image tokens with a softmax of its own,  O = softmax(Q K_text^T s) V_text + ip_scale * softmax(Q K_ip^T s) V_ip,  in front
 * of to_out.  One launch per cross-attention as before (sdeo_attention2_f16): the step's dispatch count does not change.
 * sdeo_enable_ip_adapter: after sdeo_create[_ex], before the first sdeo_load_weight.  num_tokens 1..64 (4 = ip-adapter_sd15, 16 = the
 *   "plus" token count).  Registers, for every UNet attention block (the control networks get none),
 *   model.diffusion_model.<block>.transformer_blocks.0.attn2.to_k_ip.weight and ...to_v_ip.weight, [C][context_dim], no bias, behind
 *   everything registered at that moment: existing offsets do not move.  A handle that never calls it is bit for bit what it was.
 *   Refused on such a handle, each with its own message: sdeo_finalize_weights after sdeo_set_weight_precision(h, 8); sdeo_lora_apply on
 *   a to_k_ip / to_v_ip name.
 * sdeo_set_ip_tokens: tokens fp32 [n][num_tokens][context_dim], device.  Projects them into the K_ip | V_ip of every cross-attention
 *   (one GEMM each), once per image prompt; the forwards and steps read the result by address, so a captured step sees new tokens
 *   without re-capture.  Only launches: capturable.
 * sdeo_set_ip_scale: ip_scale of the following forwards, read at launch like the control scales (a captured step bakes it in).
 *   Default 1; sdeo_configure resets it to 1.  0 gives the bits of a handle without the adapter. */
int sdeo_enable_ip_adapter(sdeo_handle h, int num_tokens);
int sdeo_set_ip_tokens(sdeo_handle h, const float* tokens, void* stream);
int sdeo_set_ip_scale(sdeo_handle h, float scale);

/* FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; diffusers' enable_freeu): backbone scaling and a Fourier filter of the skip
 * in front of the UNet decoder's concats.  No weights.  Parameters b1, b2, s1, s2 and version in {1, 2}; mc = model_channels.
 * In ControlledUnetModel.forward, for every output block, just before h = cat([h, skip], 1) -- skip being exactly what enters the concat:
 * hs.pop() without control or with only_mid_control, hs.pop() + control.pop() otherwise (with extra control networks: the sum over
 * the nets under their scales):
 *   1. stage, by the channel count C of h: C == 4 mc -> (b, s) = (b1, s1); C == 2 mc -> (b, s) = (b2, s2); any other block is untouched.
 *      (SD-1.5 / 2.x: the authors' h.shape[1] == 1280 / == 640, output blocks 0..6 and 7..9.)
 *   2. backbone, on the first half of h's channels.  version 1: h[:, :C/2] *= b.  version 2 (what diffusers ships): m = h.mean(1) over
 *      all C channels ([n][H][W]); per image m = (m - min m) / (max m - min m); h[:, :C/2] *= (b - 1) m + 1.  Where max m == min m the
 *      factor is 1 (the torch expression gives NaN there: the one stated deviation).
 *   3. skip, the Fourier filter with threshold 1: X = fftshift(fftn(skip, dim = (-2, -1))); rows H/2-1 : H/2+1 and columns W/2-1 : W/2+1
 *      of X times s; skip = ifftn(ifftshift(X)).real.  Equivalently, per image and channel, with K(N) = {0} for N == 1, else {-1, 0}:
 *        y[u][v] = x[u][v] + (s - 1) / (H W) * sum over a in K(H), b in K(W) of (A_ab cos t - B_ab sin t),
 *        t = 2 pi (a u / H + b v / W),  A_ab = sum x cos t,  B_ab = -sum x sin t      (at most seven fp32 sums per channel)
 * All arithmetic is fp32 on the fp16 values, every output element is rounded to fp16 once, the sines and cosines are the device
 * library's double-precision ones (no fast intrinsics), every sum runs in a fixed order.
 *
 * sdeo_set_freeu: FreeU on for the following sdeo_unet_forward, sdeo_apply_model and all six fused steps (paired, SDEO_STEP_UNGUIDED,
 *   masked, stochastic; with extra control networks, an image-prompt adapter, the 2.x layout).  The control networks, the shared
 *   prefix and the VAE are untouched.  sdeo_configure builds every UNet decoder program twice, without and with the FreeU launches (at
 *   most two per affected concat, one with version 1; they allocate nothing); on / off selects which one runs, so a handle with FreeU
 *   off -- never set, or set and turned off -- runs exactly the programs of a handle that knows nothing of it: same weights, same
 *   device bytes, same launches, same bits.  The four values and the version are read at launch (a captured step bakes them in, like
 *   ip_scale); sdeo_configure turns FreeU off, as it resets ip_scale.  Callable before sdeo_configure only to be reset by it.
 *   Refused before any device call, naming the argument: a value that is not finite, negative or above SDEO_FREEU_MAX (8: b times an
 *   fp16 activation of up to 65504 / 8 stays finite), a version other than 1 or 2.  A refused call leaves the handle as it was.
 *   No item of the cache contract depends on it: hint features, context K / V, the table and the staged latent are computed in front
 *   of the decoder.
 * sdeo_clear_freeu: off.
 * Untested: handles with fp8 weights or activations (nothing refuses them). */
#define SDEO_FREEU_MAX 8
int sdeo_set_freeu(sdeo_handle h, float b1, float b2, float s1, float s2, int version);
int sdeo_clear_freeu(sdeo_handle h);

/* Fix the problem size (allocate_buffers equivalent): n = images per call of the *_forward functions
 * (the CFG pair counts as 2), latent h x w.  Allocates the activation arena once. */
int sdeo_configure(sdeo_handle h, int n, int latent_h, int latent_w);

/* flags of the *_forward / apply_model entry points.  The hint block depends only on the hint and the
 * cross-attention K / V projections only on the text context, so a sampler that keeps both fixed over the
 * DDIM loop passes the *_CACHED flags after the first step (the corresponding pointers may then be NULL). */
#define SDEO_HINT_CACHED 1
#define SDEO_CONTEXT_CACHED 2
/* SDEO_NO_CONTROL: apply_model only, the c_concat=None branch (UNet without ControlNet) */
#define SDEO_NO_CONTROL 4
/* The time embedding (timestep_embedding -> time_embed MLP -> every ResBlock's emb_layers, openaimodel.py:777-781, 255-275)
 * depends only on t.  A sampler that knows its schedule hands it over once (sdeo_set_timestep_table) and then passes
 * SDEO_TIMESTEP_ROW(i) instead of a timesteps pointer: every image of the batch runs at timestep i of that table. */
#define SDEO_TIMESTEP_ROW(i) (8 | ((i) << 8))
#define SDEO_MAX_TABLE_STEPS 128

/* State a handle keeps between calls, and who may read it (the cache contract).
 * Five items outlive a call.  The fast paths read them by address and on the caller's word (a *_CACHED flag, SDEO_TIMESTEP_ROW, a fused
 * sdeo_*_step, SDEO_STEP_LATENT_STAGED), so the handle keeps a host-side record (csrc/cache_record.h: one type, one transition per
 * "filled by" / "cleared by" entry below, one check per "read by" entry) of what each holds and checks it before the first
 * device call of every entry point: a read is either right -- bit-identical to the same call given the inputs the cache was filled
 * from -- or refused, with a message that names the flag (or the step) and the call that fills the cache.  A refused call touches
 * nothing: not the caller's tensors (x, pred_x0, d, eps, controls), not the caches, not this record.  The checks run on the host when
 * the call is made, so a captured call is checked at capture and costs nothing at replay.
 *
 *   item                      filled by                                   cleared by                          read by
 *   ------------------------- ------------------------------------------- ----------------------------------- -----------------------------
 *   hint features, per        net 0: sdeo_apply_model /                   sdeo_configure, sdeo_lora_commit,   SDEO_HINT_CACHED (that net);
 *   control network           sdeo_controlnet_forward given the hint;     sdeo_lora_clear                     sdeo_apply_model with control
 *                             net j >= 1: sdeo_set_control_hint,                                              (every extra net); every
 *                             sdeo_controlnet_forward_net given the hint                                      sdeo_*_step (every net)
 *   context K / V, per side   a forward given the context: both sides by  sdeo_configure, sdeo_lora_commit,   SDEO_CONTEXT_CACHED (the sides
 *   (the UNet; the control    sdeo_apply_model with control; the UNet's   sdeo_lora_clear                     the call runs); every
 *   networks)                 by sdeo_unet_forward and SDEO_NO_CONTROL;                                       sdeo_*_step (both sides)
 *                             the control networks' by
 *                             sdeo_controlnet_forward[_net]
 *   timestep table            sdeo_set_timestep_table                     sdeo_configure, sdeo_lora_commit,   SDEO_TIMESTEP_ROW(i); every
 *                                                                         sdeo_lora_clear                     sdeo_*_step (table_row)
 *   staged fp16 latent        every sdeo_*_step that succeeds (for the    sdeo_configure, sdeo_apply_model,   SDEO_STEP_LATENT_STAGED
 *                             x it updated)                               sdeo_unet_forward,
 *                                                                         sdeo_controlnet_forward[_net]
 *   image-prompt K / V        sdeo_set_ip_tokens                          sdeo_configure                      every call that runs the UNet
 *   (handles with                                                                                             on such a handle:
 *   sdeo_enable_ip_adapter)                                                                                   sdeo_unet_forward,
 *                                                                                                             sdeo_apply_model, every
 *                                                                                                             sdeo_*_step
 *
 *   - sdeo_lora_commit / sdeo_lora_clear do not clear the image-prompt K / V: no adapter can touch the ip matrices they were computed
 *     with (sdeo_lora_apply refuses a to_k_ip / to_v_ip name).
 *   - Every staged context has an epoch.  A call that reads the K / V of both sides from the cache (sdeo_apply_model with control and
 *     SDEO_CONTEXT_CACHED, every sdeo_*_step) needs both computed from the same staged context: after sdeo_controlnet_forward,
 *     sdeo_unet_forward or an SDEO_NO_CONTROL call given another context the two sides hold two prompts, and such a call is refused until
 *     one sdeo_apply_model with control is given the context again.  A call that reads one side reads what that side was last given.
 *   - SDEO_STEP_LATENT_STAGED is accepted only for the very x pointer the previous fused step updated, with no call from the "cleared
 *     by" column in between.  The masked steps refuse the flag outright.
 *   - All six fused steps (sdeo_ddim_step, sdeo_dpmpp_2m_step, their _masked forms, sdeo_ddim_step_eta, sdeo_dpmpp_2m_sde_step) are one
 *     step core given six descriptions, and refuse up front what their update kernel would refuse after the networks ran: an invalid
 *     schedule (a_t <= 0, 1 - a_prev < 0), a non-finite k_x / k_d / k_p, d null with k_p != 0, next to the operand, flag, cache and table
 *     checks.  A step refused for a coefficient has launched nothing and leaves the staged-latent record as it was.
 *   - SDEO_STEP_UNGUIDED changes what a step reads, not whom it asks: the hint features and context K / V are those of the configured n
 *     images (filled by sdeo_apply_model on those n), the table rows are the same rows, and the staged latent is recorded for the x it
 *     updated, n latents of it, together with the kind of step: a pair step stages n / 2 latents twice, an unguided one n latents
 *     once, so SDEO_STEP_LATENT_STAGED after a step of the other kind is refused like a staged step on another x.
 *   - sdeo_set_control_hint, sdeo_set_control_scales, sdeo_set_timestep_table, sdeo_vae_decode and sdeo_vae_encode leave every item
 *     other than the one they fill as it is (the arena keeps the persistent tensors apart from the VAE programs). */

/* ControlNet.forward (cldm/cldm.py:284-305).  NCHW fp32 at the boundary:
 *   x_noisy [n][4][h][w], hint [n][3][8h][8w] in [0,1], timesteps int64 [n], context [n][77][768],
 *   controls[13]: NCHW fp32 outputs in the reference's binding order (export_onnx_all.py:242-256);
 *   entries may be NULL to skip the copy-out. */
int sdeo_controlnet_forward(sdeo_handle h, const float* x_noisy, const float* hint, const int64_t* timesteps,
                            const float* context, float* const* controls, int flags, void* stream);

/* ControlledUnetModel.forward (cldm/cldm.py:22-45).  controls may be NULL (control=None branch);
 * control_scales fp32[13] HOST pointer or NULL (= 1.0), applied as in apply_model (cldm/cldm.py:338);
 * only_mid_control as in the reference. */
int sdeo_unet_forward(sdeo_handle h, const float* x_noisy, const int64_t* timesteps, const float* context,
                      const float* const* controls, const float* host_control_scales, int only_mid_control, float* eps,
                      int flags, void* stream);

/* ControlLDM.apply_model (cldm/cldm.py:328-341) without the NCHW fp32 round trip of the 13 control tensors:
 * ControlNet -> scaled controls -> UNet, all fp16 NHWC inside the arena. */
int sdeo_apply_model(sdeo_handle h, const float* x_noisy, const float* hint, const int64_t* timesteps,
                     const float* context, const float* host_control_scales, int only_mid_control, int flags,
                     float* eps, void* stream);

/* Time-embedding table of a sampling schedule: host_timesteps int64[count] (HOST pointer, count <= SDEO_MAX_TABLE_STEPS), e.g.
 * np.flip(ddim_timesteps) of cldm/ddim_hacked.py:137.  Runs the embedding MLPs of both networks once for all rows; the table stays
 * valid until the next sdeo_configure / sdeo_set_timestep_table.  Not capturable (synchronises `stream`). */
int sdeo_set_timestep_table(sdeo_handle h, const int64_t* host_timesteps, int count, void* stream);

/* One DDIM step of the classifier-free-guidance pair, eta = 0 (p_sample_ddim, cldm/ddim_hacked.py:183-231, with the two
 * apply_model calls batched as [x; x] -- configured n = 2 x latents, conditional half first, as sdeo_apply_model sees it from the
 * sampler): eps = apply_model([x; x]) with the hint block and context K / V cached by an earlier sdeo_apply_model call and the
 * time embedding of row `table_row`; e = eps_u + cfg_scale (eps_c - eps_u); pred_x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t);
 * x <- sqrt(a_prev) pred_x0 + sqrt(1 - a_prev) e.  x [n/2][4][h][w] fp32 is updated IN PLACE, pred_x0 (may be NULL) receives the
 * prediction.  Arithmetic and rounding are those of sdeo_apply_model + sdeo_cfg_ddim_step (bit-identical results); what is saved
 * is the NCHW fp32 round trip of eps and the latent between the two.  flags: SDEO_STEP_LATENT_STAGED = x is exactly what the
 * previous fused step on this handle left (its fp16 copy is already staged; skips one conversion launch).  The handle checks both this
 * flag and the caches (the cache contract above): a step on a handle whose hint, context or table is missing, or a staged step on
 * another x, is refused.
 * The two halves of [x; x] differ only in their text context, so the UNet computes input_blocks.1 up to its cross-attention once, on
 * the first half (same kernels, same plans: the results do not change).  SDEO_STEP_HINT_SHARED = the cached hint of image i + n/2 is
 * that of image i (the sampler passed the same control image for the conditional and the unconditional half): the ControlNet does
 * the same.  Without the flag the ControlNet runs both halves in full.  Capturable. */
#define SDEO_STEP_LATENT_STAGED 16
#define SDEO_STEP_HINT_SHARED 32
/* the model predicts v: the update is that of sdeo_cfg_ddim_step_v.  Without the flag nothing about the step changes. */
#define SDEO_STEP_V_PREDICTION 64
/* No guidance: the un-paired member of all six fused steps (the `unconditional_conditioning is None or scale == 1` branch of
 * cldm/ddim_hacked.py:188-189).  x, pred_x0 / d, noise, orig and mask_noise are [n][4][h][w] with n the CONFIGURED count, any n >= 1;
 * mask_n is in {1, n}.  The forward runs on x once per image (the plain programs: no shared prefix applies), the model output of image
 * i is used as it is, and cfg_scale is neither read nor checked.  Bit-identical to sdeo_apply_model on x followed by the matching
 * unfused call with a null eps_u / m_u (sdeo_cfg_ddim_step(_v), sdeo_cfg_dpmpp_2m_step, sdeo_cfg_dpmpp_2m_sde_step); with blend operands
 * to sdeo_mask_blend followed by the unmasked call; staged to unstaged.  SDEO_STEP_HINT_SHARED together with it is refused (there is no
 * second half); SDEO_STEP_LATENT_STAGED, SDEO_STEP_V_PREDICTION, the blend operands, the cache contract and the table checks keep their
 * meaning, and every refusal precedes the first device call.  Without the flag every step does what it did, the refusal of an odd n
 * included.  Capturable. */
#define SDEO_STEP_UNGUIDED 128
int sdeo_ddim_step(sdeo_handle h, float* x, float* pred_x0, int table_row, float cfg_scale, float a_t, float a_prev,
                   float sqrt_one_minus_at, const float* host_control_scales, int only_mid_control, int flags, void* stream);

/* the fused CFG-pair step, as sdeo_ddim_step with that update: same flags, same caches, same table rows; capturable.
 * x <- k_x x + k_d D + k_p d(on entry), d <- D (see sdeo_cfg_dpmpp_2m_step); the caller owns d [n/2][4][h][w] fp32 (NULL only when
 * k_p == 0).  Bit-identical to sdeo_apply_model on [x; x] followed by sdeo_cfg_dpmpp_2m_step.  With SDEO_STEP_UNGUIDED: x and d are
 * [n][4][h][w], and the reference is sdeo_apply_model on x followed by sdeo_cfg_dpmpp_2m_step with m_u == NULL. */
int sdeo_dpmpp_2m_step(sdeo_handle h, float* x, float* d, int table_row, float cfg_scale, float a_t, float sqrt_one_minus_at,
                       float k_x, float k_d, float k_p, const float* host_control_scales, int only_mid_control, int flags, void* stream);

/* The fused steps with the mask / x0 blend of sdeo_mask_blend in front: x <- blend(x) IN PLACE, then exactly what sdeo_ddim_step /
 * sdeo_dpmpp_2m_step do on the blended latent (the same forward, the same update kernel).  orig, noise [n/2][4][h][w] fp32, mask
 * [mask_n][mask_c][h*w] fp32 with mask_n in {1, n/2}, mask_c in {1, 4}; sqrt_a / sqrt_one_minus_a as in sdeo_mask_blend; every other
 * argument as in the unmasked step.  The blend runs in the launch that stages the fp16 copy of [x; x] (it takes the place of that
 * launch), so a masked step has the dispatch count of an unstaged unmasked step.
 * Contract:
 *   - x, pred_x0 / d are bit-identical to sdeo_mask_blend followed by the unmasked step without SDEO_STEP_LATENT_STAGED;
 *   - SDEO_STEP_LATENT_STAGED is refused (the blend changes the latent, so it is always restaged); SDEO_STEP_HINT_SHARED and
 *     SDEO_STEP_V_PREDICTION keep their meaning;
 *   - every argument check happens before the first device call, each with its own message: a null x / orig / noise / mask, mask_n or
 *     mask_c outside the allowed values, an unconfigured handle, an odd configured n, a table row outside the table, an invalid
 *     schedule (what the update kernel would refuse), d null with k_p != 0.  A refused call leaves x, pred_x0 and d untouched;
 *   - with SDEO_STEP_UNGUIDED every [n/2] above reads [n] (x, pred_x0 / d, orig, noise; mask_n in {1, n}), an odd n is accepted, and the
 *     blend runs in the launch that stages the fp16 copy of x, each image once;
 *   - capturable. */
int sdeo_ddim_step_masked(sdeo_handle h, float* x, float* pred_x0, const float* orig, const float* noise, const float* mask, int mask_n,
                          int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row, float cfg_scale, float a_t, float a_prev,
                          float sqrt_one_minus_at, const float* host_control_scales, int only_mid_control, int flags, void* stream);
int sdeo_dpmpp_2m_step_masked(sdeo_handle h, float* x, float* d, const float* orig, const float* noise, const float* mask, int mask_n,
                              int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row, float cfg_scale, float a_t,
                              float sqrt_one_minus_at, float k_x, float k_d, float k_p, const float* host_control_scales,
                              int only_mid_control, int flags, void* stream);

/* The fused CFG-pair steps with the sampler's noise term (cldm/ddim_hacked.py:227-230, eta > 0; DPM-Solver++(2M) SDE), IN PLACE on x:
 *   sdeo_ddim_step_eta:      x <- x_prev + sigma_t * noise, with dir_coef = sqrt(1 - a_prev - sigma_t^2) inside x_prev
 *   sdeo_dpmpp_2m_sde_step:  x <- k_x x + k_d D + k_p d + k_n * noise,  d <- D
 * noise [n/2][4][h][w] fp32, read by address (a captured call reads whatever the row holds at replay); the fp16 staging of the next
 * forward is written from the noisy latent.  orig == NULL: the unmasked step (mask_noise and mask must then be NULL too); else the blend
 * of sdeo_ddim_step_masked runs in front, with mask_noise as its noise operand, and orig / mask_noise / mask / mask_n / mask_c / sqrt_a /
 * sqrt_one_minus_a mean what they mean there.  Every other argument as in sdeo_ddim_step / sdeo_dpmpp_2m_step.
 * Contract:
 *   - sdeo_ddim_step_eta is bit-identical to sdeo_apply_model on [x; x] followed by sdeo_cfg_ddim_step(_v) with the same noise and
 *     sigma_t (the noise product is one fused multiply-add in both); sdeo_dpmpp_2m_sde_step likewise to sdeo_cfg_dpmpp_2m_sde_step;
 *     with blend operands both are bit-identical to sdeo_mask_blend followed by the unmasked call;
 *   - noise == NULL is allowed only with sigma_t == 0 / k_n == 0 and then runs the launches of the plain (or masked) step; k_n == 0
 *     runs them whatever noise is;
 *   - unmasked, SDEO_STEP_LATENT_STAGED keeps its meaning (the previous fused step, stochastic or not, staged the latent);
 *     SDEO_STEP_HINT_SHARED and SDEO_STEP_V_PREDICTION keep theirs;
 *   - refused before the first device call, each with its own message, x / pred_x0 / d untouched: a null noise with sigma_t != 0 or
 *     k_n != 0; 1 - a_prev - sigma_t^2 < 0; a non-finite coefficient; a partial set of blend operands; SDEO_STEP_LATENT_STAGED together
 *     with a mask; and everything the unmasked and the masked steps refuse;
 *   - with SDEO_STEP_UNGUIDED noise, orig and mask_noise are [n][4][h][w] like x, cfg_scale is not among the coefficients checked, and the
 *     unfused calls of the first item are given eps_u / m_u == NULL after sdeo_apply_model on x;
 *   - capturable. */
int sdeo_ddim_step_eta(sdeo_handle h, float* x, float* pred_x0, const float* noise, float sigma_t,
                       const float* orig, const float* mask_noise, const float* mask, int mask_n, int mask_c, float sqrt_a,
                       float sqrt_one_minus_a, int table_row, float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at,
                       const float* host_control_scales, int only_mid_control, int flags, void* stream);
int sdeo_dpmpp_2m_sde_step(sdeo_handle h, float* x, float* d, const float* noise, const float* orig, const float* mask_noise,
                           const float* mask, int mask_n, int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row,
                           float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, float k_n,
                           const float* host_control_scales, int only_mid_control, int flags, void* stream);

/* decode_first_stage: z/scale_factor -> post_quant_conv -> Decoder (model.py:619-652).
 * z [n][4][h][w] fp32 NCHW -> images [n][3][8h][8w] fp32 NCHW in [-1,1]; images_u8 (optional, may be NULL)
 * additionally receives the NHWC uint8 post-process of canny2image_torch.py:68. n must be <= configured n. */
int sdeo_vae_decode(sdeo_handle h, const float* z, int n, float* images, uint8_t* images_u8, void* stream);

/* VAE encoder (opt-in).  Registers "first_stage_model.encoder.*" (the Encoder of ldm/modules/diffusionmodules/model.py:452-545 built
 * with the VAE fields of sdeo_config, attn_resolutions = [], double_z = True: conv_out has 2 * vae_z_channels outputs, vae_out_ch is
 * the image channel count) and "first_stage_model.quant_conv" as expected weights, and makes sdeo_configure build the encode program
 * for images of 8h x 8w.  Call it once, after sdeo_create and before the first sdeo_load_weight (the weight slab is sized at
 * registration).  The encoder stays fp16 whatever sdeo_set_weight_precision says.  Without this call nothing about the handle changes:
 * the expected weights, the device bytes and the programs are those of a handle without an encoder. */
int sdeo_enable_vae_encoder(sdeo_handle h);
/* encode_first_stage + get_first_stage_encoding (upstream AutoencoderKL.encode / LatentDiffusion.get_first_stage_encoding; both absent
 * from the reference tree): moments = quant_conv(Encoder(x)), DiagonalGaussianDistribution (ldm/modules/distributions/distributions.py:
 * 24-35), z = scale_factor * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise).
 *   images    fp32 NCHW [n][C][8h][8w] in [-1,1], OR
 *   images_u8 uint8 NHWC [n][8h][8w][C] (exactly one of the two non-NULL), mapped like upstream load_img: 2 * (u / 255) - 1 in fp32;
 *             both are rounded once to fp16, so a u8 image and its fp32 mapping give identical results;
 *   n <= configured n; C = vae_out_ch;
 *   noise     fp32 [n][zc][h][w] or NULL (= the posterior mode: z = scale_factor * mean); zc = vae_z_channels;
 *   z         fp32 [n][zc][h][w];
 *   moments   optional fp32 [n][2zc][h][w]: quant_conv output (mean, then logvar) before the clamp.
 * Images are encoded one at a time (results do not depend on n).  Fails when the handle has no encoder.  Capturable. */
int sdeo_vae_encode(sdeo_handle h, const float* images, const uint8_t* images_u8, int n, const float* noise, float* z, float* moments,
                    void* stream);

/* Multi-ControlNet (opt-in): K = 1 + count control networks on one UNet, their residuals summed,
 *   control[i] = sum_j scales_j[i] * ControlNet_j(x, hint_j, t, context)[i],  eps = ControlledUnetModel(x, t, context, control).
 * Net 0 is "control_model."; net j = 1..count registers the same tensor set under "control_model_<j>." behind everything registered
 * before (existing offsets do not move), fp8-eligible like net 0's.  count in 1..3.  Call it once, after sdeo_create[_ex] and before
 * the first sdeo_load_weight.  Without this call nothing about the handle changes.  With it, sdeo_apply_model and every sdeo_*_step
 * run all the nets (the extra ones on the side stream behind net 0; the fused decoder applies each extra net's 13 zero convs as one
 * more multi-problem launch, in place over the running sum), sdeo_set_timestep_table fills a table per net, the context K / V of every
 * net is recomputed whenever net 0's is, SDEO_STEP_HINT_SHARED vouches for the hints of every net, and only_mid_control /
 * SDEO_NO_CONTROL apply to all of them.  sdeo_unet_forward is untouched.  sdeo_finalize_weights refuses block-scaled fp8 activations
 * (sdeo_set_activation_precision 8) on such a handle. */
int sdeo_enable_extra_controlnets(sdeo_handle h, int count);
/* Net `net`'s (1..count) hint [n][hint_channels][8h][8w] fp32: copied in and run through that net's hint block into its own cached
 * features (what a new `hint` argument does for net 0; `hint` and SDEO_HINT_CACHED of the other entry points refer to net 0 only).
 * Capturable.  sdeo_configure invalidates the cache: a forward on a handle with an extra net whose hint was not set since is refused. */
int sdeo_set_control_hint(sdeo_handle h, int net, const float* hint, void* stream);
/* Net `net`'s (1..count) 13 control scales (NULL: all 1).  They persist until changed (sdeo_configure resets them to 1) and are read
 * at launch with only_mid_control folded in, like net 0's: a captured step bakes them in.  Net 0's scales stay an argument of each call. */
int sdeo_set_control_scales(sdeo_handle h, int net, const float* host_scales13);
/* sdeo_controlnet_forward for net `net` (0..count; net 0 is that function): the 13 unscaled controls of one net. */
int sdeo_controlnet_forward_net(sdeo_handle h, int net, const float* x_noisy, const float* hint, const int64_t* timesteps,
                                const float* context, float* const* controls, int flags, void* stream);

/* Control modes (opt-in): per call and per control network, apply the network to both halves of the CFG pair, to the conditional half
 * only, or not at all -- what a control window ("starting / ending control step") and guess mode (the unconditional half runs without
 * ControlNet, canny2image_torch.py:48) come down to -- with the work shrinking accordingly: a COND net runs on n / 2 images, an OFF
 * net does not run.
 * sdeo_enable_control_modes: after sdeo_create[_ex], before sdeo_configure.  Adds no weight and no device memory: sdeo_configure builds,
 *   per control network, one more program (the network on the first n / 2 images: every launch the batch prefix of its full-batch
 *   launch, in the same tensors) and the further forms of that net's zero-conv launch in the fused decoders.  A handle that never
 *   calls it is bit for bit what it was, sdeo_device_bytes included.  Refused by name: a handle with fp8 weights
 *   (sdeo_set_weight_precision 8) or block-scaled fp8 activations (sdeo_set_activation_precision 8) -- here or, when the precision is
 *   set later, by sdeo_configure; a call after sdeo_configure.
 * sdeo_set_control_mode: net 0..extra (0 = "control_model."), mode one of
 *     SDEO_CONTROL_BOTH  every image (what a handle without modes does);
 *     SDEO_CONTROL_COND  images [0, n/2) only: the conditional half of [cond; uncond];
 *     SDEO_CONTROL_OFF   no image.
 *   Host state like an extra net's scales: read when a call launches (a captured step bakes it in), kept until changed; sdeo_configure
 *   resets every net to BOTH.  It acts in sdeo_apply_model and in all six fused steps, their masked, noisy, staged and v-prediction
 *   forms included; sdeo_unet_forward, sdeo_controlnet_forward[_net] and the 13-tensor boundary ignore it.  Refused, before any device
 *   call and each with its own message: a handle without sdeo_enable_control_modes, a net outside 0..extra, a mode that is none of
 *   the three.  sdeo_apply_model with a COND net on an odd configured n is refused there, before its first device call.
 * What runs, for the modes (m_0 .. m_k) of a call:
 *   - all BOTH: exactly the programs of a handle without modes -- same launches, same bits;
 *   - all OFF: the no-control program (the SDEO_NO_CONTROL branch of sdeo_apply_model): no fork, no ControlNet launch;
 *   - anything else: an OFF net's programs do not run; a COND net's half-batch program does; the fused decoder applies, per active net,
 *     scale * zero_conv(block outputs) to the net's LIVE rows -- all of them, or those of the first n / 2 images.  The live-row rule: a
 *     row that is not live receives its residual unchanged (the skip, or the running sum of the nets in front); it is selected, never
 *     multiplied by a zero scale, because the block outputs of a COND net hold nothing meaningful beyond the first half.  The first
 *     ACTIVE net takes the skip as its residual, the later ones work in place over the running sum.  No mode adds a launch to the step
 *     where the zero convs run as one multi-problem launch per net (channel counts that are multiples of 64); the per-conv form passes
 *     the other half's skip rows through with one copy launch per zero conv of the first active net when that net is COND.
 *   - every live row of eps is bit-identical to the same call with that net in BOTH mode when every net is BOTH or COND alike; an
 *     image no net is live on is bit-identical to what the all-OFF decoder arithmetic gives it (the skip passes through unchanged).
 * SDEO_STEP_UNGUIDED: there is no second half, COND means BOTH and OFF means no control.  SDEO_STEP_HINT_SHARED stays accepted and has
 *   no effect for a net in COND or OFF mode.
 * The cache contract is untouched by the modes: a fused step still wants every net's hint cached and the context K / V of both sides,
 *   whatever the modes; a call that is given a hint (or a context) stages it and runs the hint block (the K / V projections of every
 *   net) whatever the modes, so the first active step of a window finds them cached.
 * Left for later: fp8 handles; per-half scales other than 1 / 0. */
#define SDEO_CONTROL_BOTH 0
#define SDEO_CONTROL_COND 1
#define SDEO_CONTROL_OFF 2
int sdeo_enable_control_modes(sdeo_handle h);
int sdeo_set_control_mode(sdeo_handle h, int net, int mode);

/* bytes of device memory the handle owns (weights + arena + the tensors saved under LoRA adapters) */
size_t sdeo_device_bytes(sdeo_handle h);

/* LoRA adapters, merged on the device IN PLACE into the stored weights (csrc/lora.hip):
 *   W[o][j] <- fp16( fp32(W[o][j]) + scale * sum_{r < rank} up[o][r] * down[r][j] ),   o < out, j < in * kh * kw
 * up [out][rank] and down [rank][in * kh * kw] are fp32 in the PyTorch layout of lora_up.weight / lora_down.weight (flattened) and stay
 * fp32; products and sums are fp32, the add is fp32, the store rounds once to nearest-even.  The update lands where sdeo_load_weight put
 * the tensor: inside a stacked matrix (to_q | to_k | to_v, attn2.to_k | to_v, the stacked emb_layers), in the row-interleaved GEGLU
 * projection, in a KRSC conv weight whose pad channels stay zero.  Programs and captured graphs read weights by address, so they stay
 * valid; what they computed with the earlier weights does not (below).
 *
 * sdeo_lora_apply: `name` is a registry name exactly as sdeo_weight_info returns it (any "model.diffusion_model.*", "control_model.*",
 *   "control_model_<j>.*" or "first_stage_model.*" matrix or conv weight).  down / up may be host or device pointers (copied with
 *   hipMemcpyDefault).  The first apply on a tensor saves its raw bytes (the copy counts in sdeo_device_bytes); several applies on one
 *   tensor stack, each rounding once.  Synchronises `stream`; not capturable.  Refused before any device call, each with its own message,
 *   the handle untouched: a null argument, an unknown name, a bias / norm vector (the GEGLU bias included), rank outside 1..1024, a
 *   non-finite scale, weights not finalized, and a handle with sdeo_set_weight_precision(h, 8): its fp16 copies hold the dequantised
 *   values, not the raw ones, so adapters on fp8-weight handles are out of scope.
 * sdeo_lora_commit: rebuilds what sdeo_finalize_weights derives from the raw tensors (the LayerNorm folds and the ff.net.2 x proj_out
 *   products) and marks every cache computed with the earlier weights stale, for every net: the hint features, the context K / V and the
 *   timestep table.  Until the uncached call (a forward given the hint / the context, sdeo_set_control_hint, sdeo_set_timestep_table)
 *   has run again, a call passing SDEO_HINT_CACHED, SDEO_CONTEXT_CACHED or SDEO_TIMESTEP_ROW and every fused sdeo_*_step is refused, each
 *   cache with its own message.  Call it once after the last sdeo_lora_apply of a set.
 * sdeo_lora_clear: copies every saved tensor back, frees the copies (sdeo_device_bytes returns to its earlier figure) and commits: the
 *   handle is then bit for bit the handle no adapter was applied to.
 * sdeo_lora_touched: the number of tensors currently modified (saved).
 * sdeo_read_weight: the current RAW tensor `name`, converted back to fp32 in PyTorch layout into `out` (host or device pointer, as many
 *   floats as sdeo_weight_info's dims multiply to): the inverse of sdeo_load_weight, the GEGLU de-interleave and KRSC -> OIHW without the
 *   pad included; vectors are returned as stored (the interleaved GEGLU bias is refused).  A loader / test aid. */
int sdeo_lora_apply(sdeo_handle h, const char* name, const float* down, const float* up, int rank, float scale, void* stream);
int sdeo_lora_commit(sdeo_handle h);
int sdeo_lora_clear(sdeo_handle h);
int sdeo_lora_touched(sdeo_handle h);
int sdeo_read_weight(sdeo_handle h, const char* name, float* out);

/* LoHa and LoKr adapters (LyCORIS algo=loha / algo=lokr), merged like sdeo_lora_apply: in place, the first write saved, the same
 * commit / clear / touched / read_weight.  The definitions below are this library's contract; they are not
 * pinned to upstream code.  The target weight is W with shape [O][I] or [O][I][kh][kw]; J = I*kh*kw and kk = kh*kw (kk = 1 for a
 * matrix).  The merged weight is W + scale * dW, rounded once to fp16; the caller folds the multiplier (alpha / r, or 1) into scale.
 *
 * LoHa (plain).  Leaves: hada_w1_a [O][r], hada_w1_b [r][J], hada_w2_a [O][r], hada_w2_b [r][J], optional alpha.
 *   dW = (w1_a @ w1_b) (.) (w2_a @ w2_b), viewed as W.  Multiplier: alpha / r, or 1 without alpha.
 * LoHa, Tucker form (convs with kk > 1 only).  Extra leaves: hada_t1, hada_t2, both [r][r][kh][kw].  The four factors are then
 *   transposed against the plain form: hada_wX_a [r][O] and hada_wX_b [r][I].
 *   PX[o][c][y][x] = sum_i sum_j tX[i][j][y][x] * wX_a[i][o] * wX_b[j][c];  dW = P1 (.) P2.
 * LoKr.  O = Ol*Ok and I = Im*In.  The factors are read from the tensor shapes (here: out_l = Ol, in_m = Im).
 *   w1 is [Ol][Im].  It comes either as the leaf lokr_w1, or as lokr_w1_a [Ol][r] @ lokr_w1_b [r][Im].
 *   w2 is [Ok][In*kk].  It comes in one of three forms: the leaf lokr_w2, shape [Ok][In] or [Ok][In][kh][kw];
 *     lokr_w2_a [Ok][r] @ lokr_w2_b [r][In*kk];  the Tucker form: lokr_t2 [r][r][kh][kw], lokr_w2_a [r][Ok], lokr_w2_b [r][In],
 *     contracted like LoHa's.
 *   dW[ol*Ok + ok][(im*In + in)*kk + s] = w1[ol][im] * w2[ok][in*kk + s].  For a matrix this is torch.kron(w1, w2).  For a conv it is
 *     torch.kron(w1[:, :, None, None], w2).
 *   Multiplier: alpha / r.  r is the row count of lokr_w2_b if present, else of lokr_w1_b.  Without alpha, or with both factors
 *     full, the multiplier is 1.
 * The key set decides the form.  A module is merged only when its leaves are exactly one complete form.
 *
 * Arithmetic: fp32 throughout.  LoHa: two fmaf chains in rank order and one multiply.  LoKr: one gathered w1 value times either a
 * loaded w2 value or one fmaf chain over w2's rank.  w1 = w1_a @ w1_b and a Tucker core folded into its b factor
 * (b_eff[i][(c,y,x)] = sum_j t[i][j][y][x] * b[j][c], chain in j order) are written as fp32 by a pre-pass.  Then fmaf(scale, dW, fp32(W)),
 * rounded once; an element whose update is exactly zero is not stored; pad channels are neither read nor written.
 *
 * Operands: fp32, host or device pointers, in the layout above; an absent operand is a null pointer.  sdeo_loha_apply: t1 and t2 both
 * null (plain) or both given (Tucker).  sdeo_lokr_apply: w1, or w1_a and w1_b with rank1; w2, or w2_a and w2_b with rank2, t2 given
 * for the Tucker form; rank1 / rank2 are ignored where the factor comes whole.  Refused before any device call, each with its own
 * message, the handle untouched: a null name or a missing / mixed operand set, an unknown name, a bias / norm vector, a rank outside
 * 1..1024, a non-finite scale, weights not finalized, an fp8-weight handle, a to_k_ip / to_v_ip matrix, and factor shapes that do not
 * fit the tensor (out_l / in_m not dividing out / in, a Tucker core on a matrix or a 1 x 1 conv). */
int sdeo_loha_apply(sdeo_handle h, const char* name, const float* w1_a, const float* w1_b, const float* w2_a, const float* w2_b,
                    const float* t1, const float* t2, int rank, float scale, void* stream);
int sdeo_lokr_apply(sdeo_handle h, const char* name, const float* w1, const float* w1_a, const float* w1_b, int rank1, const float* w2,
                    const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale, void* stream);

/* ------------------------------------------------------------------ text encoder
 * FrozenCLIPEmbedder.forward (ldm/modules/encoders/modules.py:123-141): token ids -> CLIPTextModel ->
 * last_hidden_state [batch][positions][width].  The tokenizer stays on the host (it needs the vocabulary
 * files the caller supplies by path).  Tensor names are those of the HuggingFace state dict below
 * "text_model." ("cond_stage_model.transformer.text_model.*" in an SD checkpoint: anything up to and including
 * "text_model." is stripped).  openai/clip-vit-large-patch14: vocab 49408, positions 77, width 768, 12 layers,
 * 12 heads, ffn 3072. */
typedef struct sdeo_clip_handle_s* sdeo_clip_handle;
typedef struct sdeo_clip_config {
  int vocab, positions, width, layers, heads, ffn;
} sdeo_clip_config;
int sdeo_clip_create(const sdeo_clip_config* cfg, sdeo_clip_handle* out);
int sdeo_clip_destroy(sdeo_clip_handle h);
int sdeo_clip_load_weight(sdeo_clip_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict);
int sdeo_clip_finalize_weights(sdeo_clip_handle h);
int sdeo_clip_num_weights(sdeo_clip_handle h);
int sdeo_clip_weight_info(sdeo_clip_handle h, int i, const char** name, int64_t dims[2], int* ndim);
/* fix the number of prompts per call and allocate the activation buffers */
/* The OpenCLIP text tower behind FrozenOpenCLIPEmbedder (ldm/modules/encoders/modules.py:147-206): the same transformer with two
 * differences.  Call before sdeo_clip_configure; hidden_act 0 = quick-GELU (default), 1 = erf GELU; skip_last_layers 0 (default) or
 * k < layers: the last k blocks are expected as weights (checkpoints hold them) but not run, final_layer_norm follows block
 * layers - k (layer = "penultimate" is k = 1).  (0, 0) leaves the handle exactly as it was created. */
int sdeo_clip_set_variant(sdeo_clip_handle h, int hidden_act, int skip_last_layers);
int sdeo_clip_configure(sdeo_clip_handle h, int batch);
/* tokens int32 [batch][positions] (device) -> out fp32 [batch][positions][width] (device); ids outside the
 * vocabulary are clamped */
int sdeo_clip_encode(sdeo_clip_handle h, const int32_t* tokens, int batch, float* out, void* stream);
size_t sdeo_clip_device_bytes(sdeo_clip_handle h);
/* LoRA / LoHa / LoKr adapters on the text tower: sdeo_lora_apply / sdeo_loha_apply / sdeo_lokr_apply / _commit / _clear / _touched and
 * sdeo_read_weight on the CLIP handle, names as in
 * sdeo_clip_weight_info (anything up to and including "text_model." is stripped); q_proj / k_proj / v_proj live inside the stacked qkv
 * matrix.  The tower runs on the raw tensors and caches nothing between encodes, so commit has nothing to rebuild or invalidate. */
int sdeo_clip_lora_apply(sdeo_clip_handle h, const char* name, const float* down, const float* up, int rank, float scale, void* stream);
int sdeo_clip_loha_apply(sdeo_clip_handle h, const char* name, const float* w1_a, const float* w1_b, const float* w2_a, const float* w2_b,
                         const float* t1, const float* t2, int rank, float scale, void* stream);
int sdeo_clip_lokr_apply(sdeo_clip_handle h, const char* name, const float* w1, const float* w1_a, const float* w1_b, int rank1,
                         const float* w2, const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale,
                         void* stream);
int sdeo_clip_lora_commit(sdeo_clip_handle h);
int sdeo_clip_lora_clear(sdeo_clip_handle h);
int sdeo_clip_lora_touched(sdeo_clip_handle h);
int sdeo_clip_read_weight(sdeo_clip_handle h, const char* name, float* out);

/* ------------------------------------------------------------------ image encoder (the image prompt of sdeo_set_ip_tokens, from a picture)
 * HuggingFace CLIPVisionModelWithProjection: pixel_values -> image_embeds [batch][proj], optionally hidden_states[-2].  The tower the
 * ip-adapter_sd15 files are trained against is OpenCLIP ViT-H/14: image 224, patch 14 (257 tokens), width 1280, 32 layers, 16 heads,
 * ffn 5120, erf GELU, proj 1024.  Tensor names are those of the HuggingFace state dict below "vision_model." (anything up to and
 * including "vision_model." is stripped) plus "visual_projection.weight":
 *   embeddings.class_embedding [W], embeddings.patch_embedding.weight [W][3][p][p], embeddings.position_embedding.weight [T][W],
 *   pre_layrnorm.* (the upstream spelling), encoder.layers.N.* as in the text tower, post_layernorm.*, visual_projection.weight [proj][W].
 *
 * sdeo_clip_image_preprocess_u8: CLIPImageProcessor for ONE 8-bit RGB HWC image of any size, on the device -- PIL's
 *   Image.resize(BICUBIC) of the shortest side to S (the long side is int(S * long / short)), the centre crop S x S
 *   (top = (nh - S) / 2, left = (nw - S) / 2, floor), v = fp32(u * (1.0 / 255)), (v - mean) / std in fp32 with CLIP's mean / std, and
 *   the result as fp16 patch rows [(S / patch)^2][Kp]: Kp = 3 patch^2 rounded up to a multiple of 8, column (py * patch + px) * 3 + c,
 *   columns >= 3 patch^2 zero.  PIL's resampler is integer arithmetic (ImagingResample, a = -0.5 bicubic, 22 fractional bits, the
 *   horizontal pass first, an 8-bit intermediate); the per-axis tables hold it and are built on the host from the sizes alone
 *   (stablediffusioneo_amd/annotator/util.py: clip_preprocess_tables), for the S columns / rows of the CROP only:
 *     x_first[S], x_count[S]: first source column and tap count of crop column j; x_coeffs[S][x_taps]: its int32 coefficients;
 *     y_*: the same for the crop's rows against source rows; src_row0, src_rows: the source rows the crop's rows tap (only those
 *     are resampled horizontally).  Table entries are clamped on the device: no table makes a launch read outside the image.
 *   Two launches: the horizontal pass into the 8-bit workspace, then vertical pass + normalise + patchify.  crop_u8 (optional,
 *   [S][S][3]) receives the resized-and-cropped 8-bit image.  workspace: >= sdeo_clip_image_preprocess_workspace_bytes(ih, iw, S) bytes
 *   (src_rows * S * 3 are used).  Only launches: capturable.
 *
 * The handle has the text handle's life cycle: create (refuses, before any device call and each with its own message, image % patch
 * != 0, a head dim sdeo_attention_f16 does not take, width / ffn / proj that are no multiples of 8), load_weight, finalize_weights,
 * configure(batch 1..16, want_hidden), then per encode: fill every slot's patch rows -- sdeo_clip_vision_set_pixels (pixel_values fp32
 * NCHW [batch][3][S][S], preprocessed elsewhere; fills all slots) or sdeo_clip_vision_set_image_u8 per slot (the op above into slot's
 * rows) -- and sdeo_clip_vision_encode: image_embeds fp32 [batch][proj]; hidden (optional; needs want_hidden = 1) fp32 [batch][T][W],
 * hidden_states[-2].  An encode whose slots were not all filled since the last encode is refused, as are a batch other than the
 * configured one and a non-NULL hidden without want_hidden.  image_embeds has the same bits with want_hidden 0 and 1. */
typedef struct sdeo_clip_vision_handle_s* sdeo_clip_vision_handle;
typedef struct sdeo_clip_vision_config {
  int image, patch, width, layers, heads, ffn, proj;
} sdeo_clip_vision_config;
size_t sdeo_clip_image_preprocess_workspace_bytes(int ih, int iw, int S);
int sdeo_clip_image_preprocess_u8(void* patch_rows, uint8_t* crop_u8, const uint8_t* img_hwc, int ih, int iw, int S, int patch,
                                  const int32_t* x_first, const int32_t* x_count, const int32_t* x_coeffs, int x_taps, const int32_t* y_first,
                                  const int32_t* y_count, const int32_t* y_coeffs, int y_taps, int src_row0, int src_rows, void* workspace,
                                  size_t workspace_bytes, void* stream);
int sdeo_clip_vision_create(const sdeo_clip_vision_config* cfg, sdeo_clip_vision_handle* out);
int sdeo_clip_vision_destroy(sdeo_clip_vision_handle h);
int sdeo_clip_vision_num_weights(sdeo_clip_vision_handle h);
int sdeo_clip_vision_weight_info(sdeo_clip_vision_handle h, int i, const char** name, int64_t dims[4], int* ndim);
int sdeo_clip_vision_load_weight(sdeo_clip_vision_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict);
int sdeo_clip_vision_finalize_weights(sdeo_clip_vision_handle h);
int sdeo_clip_vision_configure(sdeo_clip_vision_handle h, int batch, int want_hidden);
int sdeo_clip_vision_set_pixels(sdeo_clip_vision_handle h, const float* pixel_values, int batch, void* stream);
int sdeo_clip_vision_set_image_u8(sdeo_clip_vision_handle h, int slot, const uint8_t* img_hwc, int ih, int iw, const int32_t* x_first,
                                  const int32_t* x_count, const int32_t* x_coeffs, int x_taps, const int32_t* y_first, const int32_t* y_count,
                                  const int32_t* y_coeffs, int y_taps, int src_row0, int src_rows, void* workspace, size_t workspace_bytes,
                                  void* stream);
int sdeo_clip_vision_encode(sdeo_clip_vision_handle h, int batch, float* image_embeds, float* hidden, void* stream);
size_t sdeo_clip_vision_device_bytes(sdeo_clip_vision_handle h);

/* ------------------------------------------------------------------ IP-Adapter Plus image projection (the Resampler; csrc/resampler.hip)
 * hidden_states[-2] of the vision tower (what sdeo_clip_vision_encode writes as `hidden`) -> the num_queries image tokens
 * sdeo_set_ip_tokens reads, without touching the host.  The definition below is this library's statement of the published module; it is
 * UNPINNED to upstream code (neither the adapter's source nor a "plus" file was at hand).  ip-adapter-plus_sd15: tokens T 257, embed_dim
 * E 1280, dim D 768, depth 4, dim_head d 64, heads H 12 (inner = H d = 768), num_queries Q 16, ffn F 3072, out_dim O 768.
 *   x   = proj_in(hidden)                                  Linear E -> D with bias
 *   lat = latents, repeated per image                      parameter [1][Q][D]
 *   per layer l:  xn = norm1(x), ln = norm2(lat)           LayerNorm, eps 1e-5, affine
 *                 q = to_q(ln);  k | v = to_kv(cat(xn, ln) over the token axis)          no biases; T + Q keys
 *                 per head: w = softmax((q s)(k s)^T) in fp32, s = d^-1/4 (== scale d^-1/2), ONE softmax over all T + Q keys; o = w v
 *                 lat = to_out(o) + lat;  lat = W2 gelu_erf(W1 norm_ff(lat)) + lat       no biases
 *   tokens = norm_out(proj_out(lat))                       Linear D -> O with bias, LayerNorm(O)
 * Tensor names are the adapter file's keys below "image_proj." (anything up to and including "image_proj." is stripped): latents
 * [1][Q][D], proj_in.{weight,bias}, proj_out.{weight,bias}, norm_out.{weight,bias}, and per layer layers.<l>.0.{norm1,norm2}.{weight,bias},
 * layers.<l>.0.to_q.weight [inner][D], .to_kv.weight [2 inner][D], .to_out.weight [D][inner], layers.<l>.1.0.{weight,bias} (norm_ff),
 * layers.<l>.1.1.weight [F][D] (W1), layers.<l>.1.3.weight [D][F] (W2).  The latent stream is fp16 like both towers'; proj_out and
 * norm_out run in fp32.
 *
 * Life cycle of the other handles: create, load_weight, finalize_weights, configure(batch 1..16), project.  create refuses, before any
 * device call and each with its own message: widths that are no multiples of 8, dim or out_dim above 2048, heads * dim_head that is
 * no inner width the matrices can have, a head dim sdeo_attention_f16 does not take, num_queries outside 1..64.  project refuses an
 * unfinalised or unconfigured handle and a batch other than the configured one; hidden fp32 device [batch][tokens][embed_dim], tokens_out
 * fp32 device [batch][num_queries][out_dim], both 16-byte aligned.  It only launches: no allocation, no synchronisation, capturable.
 * sdeo_resampler_num_launches: the ops of the configured program, 5 + 8 depth (one kernel each; two for a GEMM whose plan splits K).
 *
 * Its two normalisation kernels as ops:
 * sdeo_layernorm_pair_f16: ONE launch normalises the b*t rows of x [b][t][c] with (gamma1, beta1) into rows 0..t-1 of kv_in[b][t + q][c]
 *   and the b*q rows of lat [b][q][c] with (gamma2, beta2) into rows t.. of kv_in and, the same bits, into the dense q_in [b * q][c].
 *   fp16 rows, fp32 gamma / beta, c a multiple of 8 up to 2048, operands 16-byte aligned.
 * sdeo_layernorm_f32: LayerNorm over the last dim of fp32 [rows][c], fp32 out (c a multiple of 4 up to 2048). */
int sdeo_layernorm_pair_f16(void* kv_in, void* q_in, const void* x, const void* lat, const float* gamma1, const float* beta1, const float* gamma2,
                            const float* beta2, int b, int t, int q, int c, float eps, void* stream);
int sdeo_layernorm_f32(float* y, const float* x, const float* gamma, const float* beta, int rows, int c, float eps, void* stream);
typedef struct sdeo_resampler_handle_s* sdeo_resampler_handle;
typedef struct sdeo_resampler_config {
  int tokens, embed_dim, dim, depth, dim_head, heads, num_queries, ffn, out_dim;
} sdeo_resampler_config;
int sdeo_resampler_create(const sdeo_resampler_config* cfg, sdeo_resampler_handle* out);
int sdeo_resampler_destroy(sdeo_resampler_handle h);
int sdeo_resampler_num_weights(sdeo_resampler_handle h);
int sdeo_resampler_weight_info(sdeo_resampler_handle h, int i, const char** name, int64_t dims[4], int* ndim);
int sdeo_resampler_load_weight(sdeo_resampler_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict);
int sdeo_resampler_finalize_weights(sdeo_resampler_handle h);
int sdeo_resampler_configure(sdeo_resampler_handle h, int batch);
int sdeo_resampler_num_launches(sdeo_resampler_handle h);
int sdeo_resampler_project(sdeo_resampler_handle h, const float* hidden, int batch, float* tokens_out, void* stream);
size_t sdeo_resampler_device_bytes(sdeo_resampler_handle h);

/* ------------------------------------------------------------------ HED soft-edge annotator
 * annotator/hed/__init__.py (ControlNetHED_Apache2 + HEDdetector.__call__): x - norm, five VGG blocks of 3x3 convs + ReLU (2, 2, 3, 3,
 * 3 convs; 64, 128, 256, 512, 512 channels) with a 2x2 / stride-2 max-pool in front of blocks 2..5 and a 1x1 projection to one
 * channel behind each block; the five projections resized bilinearly to H x W (cv2.resize INTER_LINEAR on float32 =
 * F.interpolate(mode="bilinear", align_corners=False)), averaged, passed through a sigmoid and stored as uint8 (truncated).
 * Tensor names are those of the reference state dict (= ControlNetHED.pth): "norm" (1,3,1,1), "block{1..5}.convs.{i}.weight/bias",
 * "block{1..5}.projection.weight/bias"; 37 tensors.  One image per call, any H, W >= 16 (floor pooling). */
typedef struct sdeo_hed_handle_s* sdeo_hed_handle;
int sdeo_hed_create(sdeo_hed_handle* out);
int sdeo_hed_destroy(sdeo_hed_handle h);
int sdeo_hed_num_weights(sdeo_hed_handle h);
int sdeo_hed_weight_info(sdeo_hed_handle h, int i, const char** name, int64_t dims[4], int* ndim);
/* host_data: fp32 in PyTorch layout, host or device pointer; unknown names are ignored unless strict */
int sdeo_hed_load_weight(sdeo_hed_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict);
int sdeo_hed_finalize_weights(sdeo_hed_handle h);
/* fix the image size (one image of height x width, both >= 16) and allocate the activation arena and split-K workspace once */
int sdeo_hed_configure(sdeo_hed_handle h, int height, int width);
/* img_hwc: device uint8 [H][W][3] RGB.  Outputs (each may be NULL, all device): edges uint8 [H][W]; control_chw fp32 [3][H][W] =
 * edges / 255 on three identical channels (as sdeo_canny_u8); side[5]: fp32 [h_k][w_k] projection maps of the five blocks (h_1 = H,
 * h_{k+1} = h_k / 2 rounded down), before the resize.  No allocation, no synchronisation: capturable. */
int sdeo_hed_detect_u8(sdeo_hed_handle h, const uint8_t* img_hwc, uint8_t* edges, float* control_chw, float* const* side, void* stream);
size_t sdeo_hed_device_bytes(sdeo_hed_handle h);

/* The scribble family (csrc/scribble.hip): `nms(x, t, s)` of annotator/hed/__init__.py and the hint preparation of upstream
 * gradio_fake_scribble2image / gradio_scribble2image.  All images are on the device; single planes are uint8 [h][w], any h, w >= 1.
 * Each call only launches: no allocation, no synchronisation, no copy, hipGraph-capturable.  Arguments are checked before the first
 * HIP call (null image, h or w < 1, sigma <= 0 or a Gaussian wider than 65 taps, workspace too small).
 *
 * sdeo_nms_u8: b = cv2.GaussianBlur(float32(x), (0, 0), sigma) (round(8 sigma + 1) | 1 taps, BORDER_REFLECT_101); y = b where b is
 * the maximum of one of the four 3-tap lines through the pixel (cv2.dilate(b, line) == b, neighbours outside the image ignored), else
 * 0; z = y > t ? 255 : 0.  z (optional) uint8 [h][w]; blurred (optional) fp32 [h][w] receives b.
 * workspace: >= sdeo_nms_workspace_bytes(h, w) bytes, 4-byte aligned. */
size_t sdeo_nms_workspace_bytes(int h, int w);
int sdeo_nms_u8(const uint8_t* x, int h, int w, float t, float sigma, uint8_t* z, float* blurred, void* workspace,
                    size_t workspace_bytes, void* stream);
/* edges -> nms(edges, 127, 3.0) -> cv2.GaussianBlur(uint8, (0, 0), 3.0) (OpenCV's 8-bit fixed-point path) -> > 4 ? 255 : 0.
 * scribble (optional): uint8 [h][w]; control_chw (optional): fp32 [3][h][w] = scribble / 255 on three identical channels (as
 * sdeo_canny_u8).  workspace: >= sdeo_fake_scribble_workspace_bytes(h, w) bytes, 4-byte aligned. */
size_t sdeo_fake_scribble_workspace_bytes(int h, int w);
int sdeo_fake_scribble_u8(const uint8_t* edges, int h, int w, uint8_t* scribble, float* control_chw, void* workspace,
                          size_t workspace_bytes, void* stream);
/* img_hwc: uint8 [h][w][c], c in 1..4.  map (optional): uint8 [h][w], 255 where the smallest channel is below 127, else 0;
 * control_chw (optional): fp32 [3][h][w] = map / 255. */
int sdeo_scribble_u8(const uint8_t* img_hwc, int h, int w, int c, uint8_t* map, float* control_chw, void* stream);

/* Per-kernel timing for bench.py's roofline: between begin and end every launch of the net-level calls is
 * bracketed by HIP events on the stream it runs on; end synchronises the device and returns a JSON array
 * [{"kernel", "launches", "total_ms", "flops", "bytes"}] (algorithmic flops / bytes summed over the launches).
 * Do not time whole steps while profiling is on (the events serialise nothing but add host overhead). */
int sdeo_profile_begin(sdeo_handle h);
const char* sdeo_profile_end(sdeo_handle h);

#ifdef __cplusplus
}
#endif
#endif /* SDEO_H */
