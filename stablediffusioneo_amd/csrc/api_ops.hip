// C ABI: error convention and the op-level entry points declared in include/sdeo.h.
#include <stdarg.h>

#include "../../include/sdeo.h"
#include "sdeo_internal.h"
#include "kernels.h"

namespace sdeo {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return 1;
}

}  // namespace sdeo

using namespace sdeo;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

const char* sdeo_last_error(void) { return g_last_error.c_str(); }
int sdeo_version(void) { return SDEO_ABI_VERSION; }
void sdeo_debug_force_gemm_plan(int tile, int splitk) { conv_gemm_debug_force(tile, splitk); }
void sdeo_debug_force_gemm_order(int order) { conv_gemm_debug_force_order(order); }
void sdeo_set_tuned_gemm_plan(const int* key10, int tile, int splitk) { conv_gemm_set_tuned(key10, tile, splitk); }
const char* sdeo_tuned_gemm_plans_json(void) {
  static std::string s;
  s = conv_gemm_tuned_json();
  return s.c_str();
}
int sdeo_debug_silu(void* y, const void* x, int64_t n, void* stream) { return silu((f16*)y, (const f16*)x, n, S(stream)); }

size_t sdeo_groupnorm_workspace_bytes(int n, int hw, int groups) {
  return (size_t)n * gn_chunks(hw) * groups * 2 * sizeof(float);
}

int sdeo_groupnorm_nhwc_f16(void* y, const void* x, const float* gamma, const float* beta, int n, int h, int w, int c,
                            int groups, float eps, int with_swish, void* workspace, void* stream) {
  return groupnorm_nhwc((f16*)y, c, (const f16*)x, c, gamma, beta, n, h * w, c, groups, eps, with_swish, (float*)workspace,
                        S(stream));
}

size_t sdeo_freeu_workspace_bytes(int n, int h, int w) { return freeu_workspace_bytes(n, h, w); }

int sdeo_freeu_nhwc_f16(void* buf, int ld, int n, int h, int w, int c_h, int c_skip, float b, float s, int version, void* workspace,
                        void* stream) {
  if (int rc = freeu_check("sdeo_freeu_nhwc_f16", (const f16*)buf, ld, n, h, w, c_h, c_skip, b, s, version, (const float*)workspace)) return rc;
  return freeu_nhwc_f16((f16*)buf, ld, n, h, w, c_h, c_skip, b, s, version, (float*)workspace, S(stream));
}

int sdeo_debug_groupnorm_path(int n, int hw, int c, int groups) {
  if (!(n > 0 && hw > 0 && c > 0 && c % 8 == 0 && groups > 0 && groups <= 64 && c % groups == 0)) {
    fail("groupnorm_path: n=%d hw=%d c=%d groups=%d", n, hw, c, groups);
    return -1;
  }
  GnArgs a{};
  a.B = n; a.HW = hw; a.C = c; a.groups = groups; a.ldx = a.ldy = c;
  return gn_fused_threads(a);
}

int sdeo_debug_groupnorm_ld_f16(void* y, int ldy, const void* x, int ldx, const float* gamma, const float* beta, int n, int hw, int c,
                                int groups, float eps, int with_silu, void* workspace, void* stream) {
  SDEO_CHECK(ldx >= c && ldy >= c, "groupnorm_ld: ldx=%d ldy=%d below c=%d", ldx, ldy, c);
  return groupnorm_nhwc((f16*)y, ldy, (const f16*)x, ldx, gamma, beta, n, hw, c, groups, eps, with_silu, (float*)workspace, S(stream));
}

static thread_local const void* g_next_q8 = nullptr;
static thread_local const float* g_next_q8_scale = nullptr;
// sdeo_debug_next_weights_fp8 is one-shot: every conv / GEMM entry point disarms it FIRST (before any validation can fail), so a
// rejected call can never leave it armed for an unrelated later one
struct Fp8Arm { const void* q; const float* s; };
static Fp8Arm disarm_fp8() {
  Fp8Arm a{g_next_q8, g_next_q8_scale};
  g_next_q8 = nullptr; g_next_q8_scale = nullptr;
  return a;
}
static void take_fp8(ConvGemm& p, const Fp8Arm& a) {
  if (!a.q) return;
  p.w = (const f16*)a.q; p.wscale = a.s; p.ldw = p.K;
}

// pad_before / pad_after < 0: ksize / 2 (the symmetric "same" padding of every conv of the networks)
static int fill_conv(ConvGemm& p, int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int pad_before = -1,
                     int pad_after = -1) {
  SDEO_CHECK(ksize == 1 || ksize == 3, "conv2d: ksize %d unsupported", ksize);
  SDEO_CHECK(stride == 1 || stride == 2, "conv2d: stride %d unsupported", stride);
  const int pad = pad_before < 0 ? ksize / 2 : pad_before;
  const int pa = pad_after < 0 ? ksize / 2 : pad_after;
  SDEO_CHECK(pad < ksize && pa < ksize, "conv2d: padding (%d, %d) out of range for ksize %d", pad, pa, ksize);
  const int hv = upsample2x ? 2 * h : h, wv = upsample2x ? 2 * w : w;
  p.B = n; p.Hi = h; p.Wi = w; p.Cin = cin;
  p.R = p.S = ksize; p.stride = stride; p.pad = pad; p.ups = upsample2x;
  if (pa != pad) p.pad_after = pa;
  p.Ho = (hv + pad + pa - ksize) / stride + 1;
  p.Wo = (wv + pad + pa - ksize) / stride + 1;
  SDEO_CHECK(p.Ho >= 1 && p.Wo >= 1, "conv2d: empty output (%dx%d, padding %d / %d)", h, w, pad, pa);
  p.M = n * p.Ho * p.Wo; p.N = cout; p.K = ksize * ksize * cin;
  p.ldx = cin; p.ldw = p.K; p.ldy = cout; p.ldres = cout; p.ld_bias2 = cout;
  return 0;
}

size_t sdeo_conv2d_workspace_bytes(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x) {
  ConvGemm p;
  if (fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x)) return 0;
  return conv_gemm_workspace_bytes(p);
}

size_t sdeo_canny_workspace_bytes(int h, int w) { return canny_workspace_bytes(h, w); }

int sdeo_canny_u8(const uint8_t* img_hwc, int h, int w, int c, float low_threshold, float high_threshold, uint8_t* edges,
                  float* control_chw, void* workspace, size_t workspace_bytes, void* stream) {
  return canny_u8(img_hwc, h, w, c, low_threshold, high_threshold, edges, control_chw, workspace, workspace_bytes, S(stream));
}

int sdeo_resize_lanczos4_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dst_h, int dst_w, const int32_t* x_first_tap,
                            const int16_t* x_coeffs, const int32_t* y_first_tap, const int16_t* y_coeffs, void* stream) {
  return resize_lanczos4_u8(dst, src, h, w, c, dst_h, dst_w, x_first_tap, x_coeffs, y_first_tap, y_coeffs, S(stream));
}

int sdeo_resize_area_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dst_h, int dst_w, const int32_t* x_start,
                        const int32_t* x_index, const float* x_weight, const int32_t* y_start, const int32_t* y_index,
                        const float* y_weight, void* stream) {
  return resize_area_u8(dst, src, h, w, c, dst_h, dst_w, x_start, x_index, x_weight, y_start, y_index, y_weight, S(stream));
}

int sdeo_resize_area_fast_u8(uint8_t* dst, const uint8_t* src, int h, int w, int c, int dst_h, int dst_w, void* stream) {
  return resize_area_fast_u8(dst, src, h, w, c, dst_h, dst_w, S(stream));
}

int sdeo_debug_read_stamps(int which, unsigned long long* out, int n) {
  return which ? conv_halo_read_stamps(out, n) : conv_gemm_read_stamps(out, n);
}

const char* sdeo_debug_conv2d_kernel_name(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x) {
  ConvGemm p;
  if (fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x)) return "";
  return conv_gemm_kernel_name(p);
}

const char* sdeo_debug_attention_kernel_name(int B, int H, int Tq, int Tk, int d, int causal) {
  return attention_kernel_name(B, H, Tq, Tk, d, causal);
}

const char* sdeo_debug_attention2_kernel_name(int B, int H, int Tq, int Tk, int Tk2, int d) {
  return attention2_kernel_name(B, H, Tq, Tk, Tk2, d);
}

// Plan query (tests): the ConvGemm of an sdeo_conv2d_nhwc_f16 / sdeo_gemm_f16 call, built by the same fill_conv / fill_gemm, with
// `act` and armed fp8 weights (fp8 != 0) as that call would see them; returns the tuned-table key it looks up (key10) and the
// (tile, split-K) the launcher picks.  Host only: no device call.
static const float g_query_scale = 1.f;
static const Fp8Arm kQueryFp8{&g_query_scale, &g_query_scale};

int sdeo_debug_conv2d_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int act, int fp8, int* key10,
                           int* tile, int* splitk) {
  SDEO_CHECK(key10 && tile && splitk, "conv2d_plan: null argument");
  ConvGemm p;
  if (int rc = fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x)) return rc;
  p.act = act;
  if (fp8) take_fp8(p, kQueryFp8);
  conv_gemm_query_plan(p, key10, tile, splitk);
  return 0;
}

int sdeo_conv2d_nhwc_f16(void* y, const void* x, const void* w_krsc, const float* bias, const float* bias2, const void* res,
                         int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int act, float scale,
                         void* workspace, size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  ConvGemm p;
  if (int rc = fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x)) return rc;
  p.x = (const f16*)x; p.w = (const f16*)w_krsc; p.y = (f16*)y; p.bias = bias; p.bias2 = bias2; p.res = (const f16*)res;
  p.act = act; p.scale = scale; p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  return conv_gemm(p, S(stream));
}

// sdeo_conv2d_nhwc_f16 with explicit padding: pad_before rows / columns of zeros at the top / left, pad_after at the bottom / right
size_t sdeo_conv2d_pad_workspace_bytes(int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int pad_before,
                                       int pad_after) {
  ConvGemm p;
  if (fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x, pad_before, pad_after)) return 0;
  return conv_gemm_workspace_bytes(p);
}

int sdeo_conv2d_pad_nhwc_f16(void* y, const void* x, const void* w_krsc, const float* bias, const float* bias2, const void* res,
                             int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, int pad_before, int pad_after,
                             int act, float scale, void* workspace, size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  SDEO_CHECK(pad_before >= 0 && pad_after >= 0, "conv2d_pad: negative padding (%d, %d)", pad_before, pad_after);
  ConvGemm p;
  if (int rc = fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x, pad_before, pad_after)) return rc;
  p.x = (const f16*)x; p.w = (const f16*)w_krsc; p.y = (f16*)y; p.bias = bias; p.bias2 = bias2; p.res = (const f16*)res;
  p.act = act; p.scale = scale; p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  return conv_gemm(p, S(stream));
}

// sdeo_conv2d_pad_nhwc_f16 on views: x a channel block of [pixels][ldx], y / res column blocks of [M][ldy] / [M][ldres] (the concat
// buffers of csrc/net_build.hip).  What a view may be is the launcher's to say (prepare): nothing about ldx / ldy / ldres is checked here.
int sdeo_debug_conv2d_view_f16(void* y, int ldy, const void* x, int ldx, const void* w_krsc, const float* bias, const float* bias2,
                               const void* res, int ldres, int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x,
                               int pad_before, int pad_after, int act, float scale, void* workspace, size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  SDEO_CHECK(pad_before >= 0 && pad_after >= 0, "conv2d_view: negative padding (%d, %d)", pad_before, pad_after);
  ConvGemm p;
  if (int rc = fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x, pad_before, pad_after)) return rc;
  p.x = (const f16*)x; p.w = (const f16*)w_krsc; p.y = (f16*)y; p.bias = bias; p.bias2 = bias2; p.res = (const f16*)res;
  p.ldx = ldx; p.ldy = ldy; p.ldres = ldres;
  p.act = act; p.scale = scale; p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  return conv_gemm(p, S(stream));
}

// conv2d whose epilogue emits the GroupNorm partials of its output, followed by the normalise-only GroupNorm that consumes them
// (the [conv -> GroupNorm] pairs of the networks, csrc/net_build.hip).  *slots = entries per image the plan writes; 0 = this shape's plan
// cannot emit them (nothing is launched then).  partials >= n * slots * groups * 2 floats (+ n * groups * 2 when slots > 128).
int sdeo_debug_conv2d_gn_f16(void* ynorm, void* y, const void* x, const void* w_krsc, const float* bias, const void* res, int n, int h,
                             int w, int cin, int cout, int ksize, int stride, int upsample2x, const float* gamma, const float* beta,
                             int groups, float eps, int with_silu, float* partials, size_t partial_floats, int* slots, void* stream) {
  return sdeo_debug_conv2d_gn_b2_f16(ynorm, y, x, w_krsc, bias, nullptr, res, n, h, w, cin, cout, ksize, stride, upsample2x, gamma, beta, groups, eps,
                                     with_silu, partials, partial_floats, slots, stream);
}

int sdeo_debug_conv2d_gn_b2_f16(void* ynorm, void* y, const void* x, const void* w_krsc, const float* bias, const float* bias2, const void* res,
                                int n, int h, int w, int cin, int cout, int ksize, int stride, int upsample2x, const float* gamma,
                                const float* beta, int groups, float eps, int with_silu, float* partials, size_t partial_floats, int* slots,
                                void* stream) {
  const Fp8Arm arm = disarm_fp8();
  SDEO_CHECK(slots && groups > 0 && cout % groups == 0, "conv2d_gn: bad arguments");
  ConvGemm p;
  if (int rc = fill_conv(p, n, h, w, cin, cout, ksize, stride, upsample2x)) return rc;
  p.x = (const f16*)x; p.w = (const f16*)w_krsc; p.y = (f16*)y; p.bias = bias; p.res = (const f16*)res;
  p.bias2 = bias2; p.ld_bias2 = cout;
  take_fp8(p, arm);
  const int cpg = cout / groups;
  *slots = conv_gemm_gn_slots(p, cpg);
  if (*slots <= 0) { *slots = 0; return 0; }
  const size_t need = (size_t)n * *slots * groups * 2, fold = *slots > 128 ? (size_t)n * groups * 2 : 0;
  SDEO_CHECK(partials && partial_floats >= need + fold, "conv2d_gn: partials buffer too small");
  p.gn_out = partials; p.gn_cpg = cpg; p.gn_slots = *slots; p.gn_groups = groups;
  if (int rc = conv_gemm(p, S(stream))) return rc;
  GnArgs g{(f16*)ynorm, (const f16*)y, gamma, beta, partials + need, cout, cout, n, p.Ho * p.Wo, cout, groups, eps, with_silu};
  g.ext_partials = partials; g.ext_nsc = *slots;
  return groupnorm_nhwc(g, S(stream));
}

static void fill_gemm(ConvGemm& p, int m, int n, int k) {
  p.B = m; p.Hi = p.Wi = p.Ho = p.Wo = 1; p.Cin = k; p.R = p.S = 1; p.stride = 1; p.pad = 0;
  p.M = m; p.N = n; p.K = k;
}

int sdeo_debug_gemm_plan(int m, int n, int k, int act, int fp8, int* key10, int* tile, int* splitk) {
  SDEO_CHECK(key10 && tile && splitk, "gemm_plan: null argument");
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.act = act;
  if (fp8) take_fp8(p, kQueryFp8);
  conv_gemm_query_plan(p, key10, tile, splitk);
  return 0;
}

// (tile, split-K) of the last conv / GEMM launch (host-side record; -1 / 0 before the first)
void sdeo_debug_last_gemm_plan(int* tile, int* splitk) { conv_gemm_last_plan(tile, splitk); }
int sdeo_debug_last_gemm_epilogue(void) { return conv_gemm_last_epilogue(); }
int sdeo_debug_last_gemm_epilogue_mode(void) { return conv_gemm_last_epilogue_mode(); }
void sdeo_debug_force_gemm_epilogue_mode(int mode) { conv_gemm_debug_force_epilogue_mode(mode); }
int sdeo_debug_tile_has_epilogue_mode(int tile, int mode) { return conv_gemm_tile_has_epilogue_mode(tile, mode); }
int sdeo_debug_gemm_epilogue_census(int* rows6, int cap, int clear) { return conv_gemm_epilogue_census(rows6, cap, clear); }

int sdeo_debug_tile_info(int tile, int* kind, int* bm, int* bn, int* stages, int* caps, const char** name) {
  return conv_gemm_tile_info(tile, kind, bm, bn, stages, caps, name);
}

size_t sdeo_gemm_workspace_bytes(int m, int n, int k) {
  ConvGemm p;
  fill_gemm(p, m, n, k);
  return conv_gemm_workspace_bytes(p);
}

int sdeo_gemm_f16(void* y, int ldy, const void* x, int ldx, const void* w, int ldw, const float* bias, const void* res,
                  int ldres, int m, int n, int k, int act, float scale, int out_f32, int bias_per_row, void* workspace,
                  size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.x = (const f16*)x; p.w = (const f16*)w; p.bias = bias; p.res = (const f16*)res;
  if (out_f32) p.y32 = (float*)y; else p.y = (f16*)y;
  p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.ldres = ldres;
  p.act = act; p.scale = scale; p.bias_per_row = bias_per_row;
  p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  return conv_gemm(p, S(stream));
}

// block-scaled fp8 ("MX") at op level: pack an fp16 matrix, and the GEMM on two packed operands (v_mfma_scale_f32_16x16x128_f8f6f4)
int sdeo_debug_quantize_mx(void* q_out, void* scales_out, const void* x, int rows, int cols, void* stream) {
  return quantize_mx((uint8_t*)q_out, (uint8_t*)scales_out, (const f16*)x, rows, cols, cols, cols, cols / 32, S(stream));
}
int sdeo_debug_gemm_mx_f16(void* y, int ldy, const void* xq, const void* xs, const void* wq, const void* ws, const float* bias, const void* res,
                           int ldres, int m, int n, int k, int act, void* workspace, size_t workspace_bytes, void* stream) {
  (void)disarm_fp8();
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.x = (const f16*)xq; p.w = (const f16*)wq; p.y = (f16*)y; p.bias = bias; p.res = (const f16*)res;
  p.ldx = k; p.ldw = k; p.ldy = ldy; p.ldres = ldres; p.act = act;
  p.mx_sx = (const uint8_t*)xs; p.mx_sw = (const uint8_t*)ws; p.mx_ldsx = k / 32; p.mx_ldsw = k / 32;
  p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  return conv_gemm(p, S(stream));
}

// sdeo_debug_gemm_mx_f16 with what csrc/net_build.hip hands a block-scaled launch besides bias / residual / act: an output scale, a
// residual of res_rows rows, row statistics out and a LayerNorm-folded input (act 3: the GEGLU pair, weights in geglu_interleave order)
int sdeo_debug_gemm_mx_ex_f16(void* y, int ldy, const void* xq, const void* xs, const void* wq, const void* ws, const float* bias, const void* res,
                              int ldres, int res_rows, int m, int n, int k, int act, float scale, float* stats, int stats_ld, int* strips_out,
                              const float* ln_stats, const float* ln_s, int ln_ld, int ln_strips, int ln_c, float eps, void* workspace,
                              size_t workspace_bytes, void* stream) {
  (void)disarm_fp8();
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.x = (const f16*)xq; p.w = (const f16*)wq; p.y = (f16*)y; p.bias = bias; p.res = (const f16*)res;
  p.ldx = k; p.ldw = k; p.ldy = ldy; p.ldres = ldres; p.res_rows = res_rows; p.act = act; p.scale = scale;
  p.mx_sx = (const uint8_t*)xs; p.mx_sw = (const uint8_t*)ws; p.mx_ldsx = k / 32; p.mx_ldsw = k / 32;
  p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  if (ln_stats) { p.ln_stats = ln_stats; p.ln_s = ln_s; p.ln_ld = ln_ld; p.ln_strips = ln_strips; p.ln_c = ln_c; p.ln_eps = eps; }
  if (stats) {       // as sdeo_debug_gemm_res_rows_f16: a split-K plan (*strips_out = 0) still runs and leaves the statistics to row_stats
    SDEO_CHECK(strips_out, "gemm_mx_ex: null argument");
    *strips_out = conv_gemm_stats_strips(p);
    SDEO_CHECK(*strips_out <= stats_ld, "gemm_mx_ex: %d strips do not fit stats_ld %d", *strips_out, stats_ld);
    if (*strips_out > 0) { p.stats_out = stats; p.stats_ld = stats_ld; }
  }
  return conv_gemm(p, S(stream));
}

int sdeo_debug_quantize_fp8_rows(void* w_f16_inout, void* q_out, float* scale_out, int rows, int cols, void* stream) {
  return quantize_fp8_rows((uint8_t*)q_out, scale_out, (f16*)w_f16_inout, rows, cols, cols, cols, S(stream));
}
void sdeo_debug_next_weights_fp8(const void* q, const float* scale) { g_next_q8 = q; g_next_q8_scale = scale; }

int sdeo_debug_fold_layernorm(void* w_out, float* s_out, float* b_out, const void* w, const float* gamma, const float* beta,
                              const float* bias, int rows, int c, void* stream) {
  return fold_layernorm((f16*)w_out, s_out, b_out, (const f16*)w, gamma, beta, bias, rows, c, S(stream));
}

int sdeo_debug_compose_proj(void* w_out, float* b_out, const void* wp, const float* bp, const void* w2, const float* b2, int c, int k2,
                            void* stream) {
  return compose_proj((f16*)w_out, b_out, (const f16*)wp, bp, (const f16*)w2, b2, c, k2, S(stream));
}

int sdeo_debug_gemm_stats_f16(void* y, int ldy, const void* x, int ldx, const void* w, int ldw, const float* bias, const void* res,
                              int ldres, int m, int n, int k, float* stats, int stats_ld, int* strips_out, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  SDEO_CHECK(stats && strips_out, "gemm_stats: null argument");
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.x = (const f16*)x; p.w = (const f16*)w; p.bias = bias; p.res = (const f16*)res; p.y = (f16*)y;
  p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.ldres = ldres;
  take_fp8(p, arm);
  *strips_out = conv_gemm_stats_strips(p);
  if (*strips_out == 0) return 0;
  SDEO_CHECK(*strips_out <= stats_ld, "gemm_stats: %d strips do not fit stats_ld %d", *strips_out, stats_ld);
  p.stats_out = stats; p.stats_ld = stats_ld;
  return conv_gemm(p, S(stream));
}

int sdeo_debug_gemm_res_rows_f16(void* y, int ldy, const void* x, int ldx, const void* w, int ldw, const float* bias, const void* res,
                                 int ldres, int res_rows, int m, int n, int k, float* stats, int stats_ld, int* strips_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.x = (const f16*)x; p.w = (const f16*)w; p.bias = bias; p.res = (const f16*)res; p.y = (f16*)y;
  p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.ldres = ldres; p.res_rows = res_rows;
  p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  if (stats) {
    SDEO_CHECK(strips_out, "gemm_res_rows: null argument");
    *strips_out = conv_gemm_stats_strips(p);
    SDEO_CHECK(*strips_out <= stats_ld, "gemm_res_rows: %d strips do not fit stats_ld %d", *strips_out, stats_ld);
    if (*strips_out > 0) { p.stats_out = stats; p.stats_ld = stats_ld; }
  }
  return conv_gemm(p, S(stream));
}

// sdeo_conv2d_nhwc_f16 (stride 1, no bias2) with what csrc/net_build.hip's conv() can add to a conv: a residual of res_rows rows
// (0 = one per output row), row statistics out, and (for the host check only: it is refused for filters larger than 1x1) a
// LayerNorm-folded input
int sdeo_debug_conv2d_ex_f16(void* y, const void* x, const void* w_krsc, const float* bias, const void* res, int res_rows, int n, int h,
                             int w, int cin, int cout, int ksize, float* stats, int stats_ld, int* strips_out, const float* ln_stats,
                             const float* ln_s, int ln_ld, int ln_strips, void* workspace, size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  ConvGemm p;
  if (int rc = fill_conv(p, n, h, w, cin, cout, ksize, 1, 0)) return rc;
  p.x = (const f16*)x; p.w = (const f16*)w_krsc; p.y = (f16*)y; p.bias = bias; p.res = (const f16*)res; p.res_rows = res_rows;
  p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  if (ln_stats) { p.ln_stats = ln_stats; p.ln_s = ln_s; p.ln_ld = ln_ld; p.ln_strips = ln_strips; p.ln_c = cin; p.ln_eps = 1e-5f; }
  if (stats) {
    SDEO_CHECK(strips_out, "conv2d_ex: null argument");
    *strips_out = conv_gemm_stats_strips(p);
    SDEO_CHECK(*strips_out > 0 && *strips_out <= stats_ld, "conv2d_ex: %d strips do not fit stats_ld %d", *strips_out, stats_ld);
    p.stats_out = stats; p.stats_ld = stats_ld;
  }
  return conv_gemm(p, S(stream));
}

int sdeo_debug_gemm_multi_f16(int count, const int* tile, const int* splitk, const int* m, const int* n, const int* k, void* const* y,
                              const int* ldy, const void* const* x, const int* ldx, const void* const* w, const int* ldw,
                              const void* const* bias, const void* const* res, const int* ldres, const float* scale, void* stream) {
  (void)disarm_fp8();       // multi-problem launches are fp16 only
  SDEO_CHECK(count >= 1 && tile && splitk && m && n && k && y && ldy && x && ldx && w && ldw && scale, "gemm_multi: null argument");
  std::vector<ConvGemm> ps((size_t)count);
  for (int i = 0; i < count; ++i) {
    ConvGemm& p = ps[i];
    fill_gemm(p, m[i], n[i], k[i]);
    p.x = (const f16*)x[i]; p.w = (const f16*)w[i]; p.y = (f16*)y[i];
    p.bias = bias ? (const float*)bias[i] : nullptr;
    p.res = res ? (const f16*)res[i] : nullptr;
    p.ldx = ldx[i]; p.ldw = ldw[i]; p.ldy = ldy[i]; p.ldres = (res && res[i] && ldres) ? ldres[i] : 0;
    p.scale = scale[i];
    p.force_tile = tile[i]; p.force_splitk = splitk[i];
  }
  ConvGemmMultiPlan pl;
  if (int rc = conv_gemm_multi_plan(ps, tile[0], &pl)) return rc;      // every refusal happens here, before any device call
  void* tab = nullptr;
  SDEO_HIP(hipMalloc(&tab, pl.table.size()));
  int rc = 0;
  if (hipMemcpy(tab, pl.table.data(), pl.table.size(), hipMemcpyHostToDevice) != hipSuccess) rc = fail("gemm_multi: cannot write the problem table");
  if (!rc) rc = conv_gemm_multi_launch(pl, tab, nullptr, S(stream));
  if (!rc && hipStreamSynchronize(S(stream)) != hipSuccess) rc = fail("gemm_multi: the launch failed");      // the table must outlive it
  (void)hipFree(tab);
  return rc;
}

int sdeo_debug_gemm_ln_f16(void* y, int ldy, const void* x, int ldx, const void* w_folded, int ldw, const float* ln_s,
                           const float* bias_folded, const float* stats, int stats_ld, int strips, int ln_c, int m, int n, int k, int act, float eps, void* workspace, size_t workspace_bytes, void* stream) {
  const Fp8Arm arm = disarm_fp8();
  ConvGemm p;
  fill_gemm(p, m, n, k);
  p.x = (const f16*)x; p.w = (const f16*)w_folded; p.bias = bias_folded; p.y = (f16*)y;
  p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.act = act;
  p.ln_stats = stats; p.ln_s = ln_s; p.ln_strips = strips; p.ln_ld = stats_ld; p.ln_c = ln_c; p.ln_eps = eps;
  p.workspace = (float*)workspace; p.workspace_bytes = workspace_bytes;
  take_fp8(p, arm);
  return conv_gemm(p, S(stream));
}

int sdeo_debug_row_stats_f16(float* stats, int stats_ld, const void* x, int ldx, int rows, int c, void* stream) {
  return row_stats(stats, stats_ld, (const f16*)x, ldx, rows, c, S(stream));
}

int sdeo_layernorm_f16(void* y, const void* x, const float* gamma, const float* beta, int rows, int c, float eps,
                       void* stream) {
  return layernorm((f16*)y, c, (const f16*)x, c, gamma, beta, rows, c, eps, S(stream));
}

int sdeo_debug_layernorm_ld_f16(void* y, int ldy, const void* x, int ldx, const float* gamma, const float* beta, int rows, int c,
                                float eps, void* stream) {
  SDEO_CHECK(ldx >= c && ldy >= c, "layernorm_ld: ldx=%d ldy=%d below c=%d", ldx, ldy, c);
  return layernorm((f16*)y, ldy, (const f16*)x, ldx, gamma, beta, rows, c, eps, S(stream));
}

int sdeo_debug_softmax_rows(void* p, int ldp, const float* s, int lds, int rows, int cols, float scale, void* stream) {
  SDEO_CHECK(ldp >= cols && lds >= cols, "softmax_rows: ldp=%d lds=%d below cols=%d", ldp, lds, cols);
  return softmax_rows((f16*)p, ldp, s, lds, rows, cols, scale, S(stream));
}

int sdeo_attention_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int b,
                       int heads, int tq, int tk, int tk_stride, int vt_batch_stride, int d, float scale, void* stream) {
  return attention((f16*)o, ldo, (const f16*)q, ldq, (const f16*)k, ldk, (const f16*)v, ldv, b, heads, tq, tk, tk_stride,
                   vt_batch_stride, d, scale, S(stream));
}

int sdeo_debug_attention_qb_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int b,
                                int q_batches, int heads, int tq, int tk, int tk_stride, int v_batch_stride, int d, float scale, void* stream) {
  AttnArgs a{(f16*)o, (const f16*)q, (const f16*)k, (const f16*)v, ldo, ldq, ldk, ldv, b, heads, tq, tk, tk_stride, v_batch_stride, d, scale, 0};
  a.qB = q_batches;
  return attention(a, S(stream));
}

// check_only: the refusals of the launch without the launch (sdeo_debug_attention2_check)
static int attention2_api(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int tk, int tk_stride,
                          int v_batch_stride, const void* k2, int ldk2, const void* v2, int ldv2, int tk2, int tk2_stride,
                          int v2_batch_stride, float weight2, int b, int q_batches, int heads, int tq, int d, float scale, void* stream,
                          bool check_only = false) {
  AttnArgs a{(f16*)o, (const f16*)q, (const f16*)k, (const f16*)v, ldo, ldq, ldk, ldv, b, heads, tq, tk, tk_stride, v_batch_stride, d, scale, 0};
  a.qB = q_batches;
  const Attn2Seg s2{(const f16*)k2, (const f16*)v2, ldk2, ldv2, tk2, tk2_stride, v2_batch_stride, weight2};
  return check_only ? attention2_check(a, s2) : attention2(a, s2, S(stream));
}

int sdeo_debug_attention2_check(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int tk, int tk_stride,
                                int v_batch_stride, const void* k2, int ldk2, const void* v2, int ldv2, int tk2, int tk2_stride,
                                int v2_batch_stride, float weight2, int b, int heads, int tq, int d, float scale) {
  return attention2_api(o, ldo, q, ldq, k, ldk, v, ldv, tk, tk_stride, v_batch_stride, k2, ldk2, v2, ldv2, tk2, tk2_stride, v2_batch_stride,
                        weight2, b, 0, heads, tq, d, scale, nullptr, true);
}

int sdeo_attention2_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int tk, int tk_stride,
                        int v_batch_stride, const void* k2, int ldk2, const void* v2, int ldv2, int tk2, int tk2_stride,
                        int v2_batch_stride, float weight2, int b, int heads, int tq, int d, float scale, void* stream) {
  return attention2_api(o, ldo, q, ldq, k, ldk, v, ldv, tk, tk_stride, v_batch_stride, k2, ldk2, v2, ldv2, tk2, tk2_stride, v2_batch_stride,
                        weight2, b, 0, heads, tq, d, scale, stream);
}

int sdeo_debug_attention2_qb_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int tk,
                                 int tk_stride, int v_batch_stride, const void* k2, int ldk2, const void* v2, int ldv2, int tk2,
                                 int tk2_stride, int v2_batch_stride, float weight2, int b, int q_batches, int heads, int tq, int d,
                                 float scale, void* stream) {
  return attention2_api(o, ldo, q, ldq, k, ldk, v, ldv, tk, tk_stride, v_batch_stride, k2, ldk2, v2, ldv2, tk2, tk2_stride, v2_batch_stride,
                        weight2, b, q_batches, heads, tq, d, scale, stream);
}

int sdeo_attention_causal_f16(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int b,
                              int heads, int tq, int tk, int tk_stride, int vt_batch_stride, int d, float scale, void* stream) {
  return attention((f16*)o, ldo, (const f16*)q, ldq, (const f16*)k, ldk, (const f16*)v, ldv, b, heads, tq, tk, tk_stride,
                   vt_batch_stride, d, scale, S(stream), 1);
}

int sdeo_geglu_f16(void* y, const void* a, int rows, int c, void* stream) {
  return geglu((f16*)y, c, (const f16*)a, 2 * c, rows, c, S(stream));
}

int sdeo_timestep_embedding_f16(void* out, const int64_t* t, int b, int dim, void* stream) {
  return timestep_embedding((f16*)out, t, b, dim, S(stream));
}

int sdeo_cfg_ddim_step(float* x_prev, float* pred_x0, const float* x, const float* eps_c, const float* eps_u,
                       const float* noise, float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at,
                       int64_t n, void* stream) {
  return cfg_ddim_step(x_prev, pred_x0, x, eps_c, eps_u, noise, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, n,
                       false, S(stream));
}

int sdeo_cfg_ddim_step_v(float* x_prev, float* pred_x0, const float* x, const float* v_c, const float* v_u,
                         const float* noise, float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at,
                         int64_t n, void* stream) {
  return cfg_ddim_step(x_prev, pred_x0, x, v_c, v_u, noise, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, n,
                       true, S(stream));
}

int sdeo_cfg_dpmpp_2m_step(float* x_next, float* d, const float* x, const float* m_c, const float* m_u, float cfg_scale, float a_t,
                           float sqrt_one_minus_at, float k_x, float k_d, float k_p, int flags, int64_t n, void* stream) {
  return cfg_lms_step("cfg_lms_step", x_next, d, x, m_c, m_u, nullptr, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p, 0.f, n,
                      (flags & SDEO_STEP_V_PREDICTION) != 0, S(stream));
}

int sdeo_cfg_dpmpp_2m_sde_step(float* x_next, float* d, const float* x, const float* m_c, const float* m_u, const float* noise,
                               float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, float k_n, int flags,
                               int64_t n, void* stream) {
  return cfg_lms_step("cfg_lms_noise_step", x_next, d, x, m_c, m_u, noise, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p, k_n, n,
                      (flags & SDEO_STEP_V_PREDICTION) != 0, S(stream));
}

int sdeo_mask_blend(float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c, float sqrt_a,
                    float sqrt_one_minus_a, int n, int c, int hw, void* stream) {
  return mask_blend(x, orig, noise, mask, mask_n, mask_c, sqrt_a, sqrt_one_minus_a, n, c, hw, S(stream));
}

int sdeo_composite_u8(uint8_t* dst, const uint8_t* gen, const uint8_t* orig, const uint8_t* mask, int h, int w, int c, void* stream) {
  return composite_u8(dst, gen, orig, mask, h, w, c, S(stream));
}

int sdeo_nchw_f32_to_nhwc_f16(void* y, int ldy, const float* x, int n, int c, int hw, void* stream) {
  return nchw_f32_to_nhwc_f16((f16*)y, ldy, x, n, c, hw, 1.0f, S(stream));
}

int sdeo_nhwc_f16_to_nchw_f32(float* y, const void* x, int ldx, int n, int c, int hw, float scale, void* stream) {
  return nhwc_f16_to_nchw_f32(y, (const f16*)x, ldx, n, c, hw, scale, S(stream));
}

int sdeo_oihw_f32_to_krsc_f16(void* y, const float* w, int o, int i, int r, int s, int i_pad, void* stream) {
  return oihw_f32_to_ohwi_f16((f16*)y, w, o, i, r, s, i_pad, S(stream));
}

}  // extern "C"
