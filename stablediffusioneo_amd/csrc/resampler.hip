// IP-Adapter Plus "Resampler" image projection: hidden_states[-2] of the CLIP vision tower -> the Q image tokens `sdeo_set_ip_tokens`
// reads.  The algorithm as include/sdeo.h states it (UNPINNED to upstream code: no adapter source or "plus" file was at hand):
//   x   = proj_in(hidden) + bias                                                   [B][T][D]
//   lat = latents, once per image                                                  [B][Q][D]
//   per layer:  xn = norm1(x), ln = norm2(lat);  q = to_q(ln);  k | v = to_kv(cat(xn, ln))          (T + Q keys, ONE softmax)
//               lat += to_out(softmax(q k^T d^-1/2) v);  lat += W2 gelu_erf(W1 norm_ff(lat))         (no biases)
//   tokens = norm_out(proj_out(lat) + bias)                                        [B][Q][O]
// It is the towers' program (clip.hip, clip_vision.hip) on the same conv_gemm / attention / layernorm kernels, with an fp16 latent
// stream.  New HIP, one wave per row with two-pass statistics in registers like norm.hip's layernorm_kernel:
//   * layernorm_pair_kernel: norm1 over the image rows and norm2 over the latent rows in ONE launch, written where the key / value GEMM
//     reads them (kv_in[b][T + Q][D]: image rows, then latent rows) and, for the latent rows, also densely for to_q (q_in[B Q][D]).
//     Two LayerNorm launches and a concatenation per layer become one launch, and attention() runs on one key buffer with a per-image
//     row stride of T + Q.
//   * layernorm_f32_kernel: norm_out on the fp32 rows proj_out writes (y32), fp32 out: the tokens are never rounded to fp16 after the
//     last GEMM.
//   * broadcast_rows_kernel: the latent parameter into every image's rows of the fp16 stream.
#include <stdint.h>

#include "../../include/sdeo.h"
#include "program_handle.h"

using namespace sdeo;

namespace {

// rows [0, B T): y = LN(x[row]; g1, b1) -> kv_in[b][t];  rows [B T, B T + B Q): y = LN(lat[r]; g2, b2) -> kv_in[b][T + q] and q_in[r].
// The row lives in registers (VPL vectors of 8 per lane => C <= 512 VPL); 4 rows per block.
template <int VPL>
__global__ __launch_bounds__(256) void layernorm_pair_kernel(f16* __restrict__ kv_in, f16* __restrict__ q_in, const f16* __restrict__ x,
                                                             const f16* __restrict__ lat, const float* __restrict__ g1,
                                                             const float* __restrict__ b1, const float* __restrict__ g2,
                                                             const float* __restrict__ b2, int B, int T, int Q, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int xrows = B * T;
  if (row >= xrows + B * Q) return;
  const bool is_lat = row >= xrows;
  const int r = is_lat ? row - xrows : row;                  // row of x / of lat
  const int per = is_lat ? Q : T;
  const int b = r / per, t = r - b * per;
  const f16* src = (is_lat ? lat : x) + (size_t)r * C;
  const float* gamma = is_lat ? g2 : g1;
  const float* beta = is_lat ? b2 : b1;
  f16* dst = kv_in + ((size_t)b * (T + Q) + (is_lat ? T : 0) + t) * C;
  f16* dst2 = is_lat ? q_in + (size_t)r * C : nullptr;
  const int nvec = C / 8;
  f16x8 v[VPL];
  f32x4 gv[VPL][2], bv[VPL][2];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      v[i] = *reinterpret_cast<const f16x8*>(src + vi * 8);
      gv[i][0] = *reinterpret_cast<const f32x4*>(gamma + vi * 8); gv[i][1] = *reinterpret_cast<const f32x4*>(gamma + vi * 8 + 4);
      bv[i][0] = *reinterpret_cast<const f32x4*>(beta + vi * 8); bv[i][1] = *reinterpret_cast<const f32x4*>(beta + vi * 8 + 4);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    if (lane + i * 64 < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)v[i][j];
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    if (lane + i * 64 < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = (float)v[i][j] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      f16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (f16)(((float)v[i][j] - mean) * rstd * gv[i][j >> 2][j & 3] + bv[i][j >> 2][j & 3]);
      *reinterpret_cast<f16x8*>(dst + vi * 8) = o;
      if (dst2) *reinterpret_cast<f16x8*>(dst2 + vi * 8) = o;
    }
  }
}

// y[row] = LN(x[row]) on fp32 rows, fp32 out; 8 vectors of 4 per lane => C <= 2048
__global__ __launch_bounds__(256) void layernorm_f32_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int rows, int C, float eps) {
  constexpr int VPL = 8;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = C / 4;
  f32x4 v[VPL];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      v[i] = *reinterpret_cast<const f32x4*>(x + (size_t)row * C + vi * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += v[i][j];
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    if (lane + i * 64 < nvec) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; q += d * d; }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gamma + vi * 4), bv = *reinterpret_cast<const f32x4*>(beta + vi * 4);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * gv[j] + bv[j];
      *reinterpret_cast<f32x4*>(y + (size_t)row * C + vi * 4) = o;
    }
  }
}

// dst[b][0 : n8] = src[0 : n8] for b < B, in vectors of 8 fp16
__global__ __launch_bounds__(256) void broadcast_rows_kernel(f16* __restrict__ dst, const f16* __restrict__ src, int B, int n8) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * n8) return;
  reinterpret_cast<f16x8*>(dst)[i] = reinterpret_cast<const f16x8*>(src)[i % n8];
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int layernorm_pair(f16* kv_in, f16* q_in, const f16* x, const f16* lat, const float* g1, const float* b1, const float* g2, const float* b2,
                          int B, int T, int Q, int C, float eps, hipStream_t stream) {
  SDEO_CHECK(kv_in && q_in && x && lat && g1 && b1 && g2 && b2, "layernorm_pair: null operand");
  SDEO_CHECK(B >= 1 && T >= 1 && Q >= 1 && C >= 8 && C % 8 == 0, "layernorm_pair: B=%d T=%d Q=%d C=%d (C a positive multiple of 8)", B, T, Q, C);
  SDEO_CHECK(C <= 2048, "layernorm_pair: C=%d > 2048 unsupported", C);
  SDEO_CHECK((int64_t)B * (T + Q) <= (int64_t)1 << 24, "layernorm_pair: %lld rows unsupported", (long long)B * (T + Q));
  SDEO_CHECK(aligned16(kv_in) && aligned16(q_in) && aligned16(x) && aligned16(lat) && aligned16(g1) && aligned16(b1) && aligned16(g2) && aligned16(b2),
             "layernorm_pair: operands must be 16-byte aligned");
  const int vpl = cdiv(C / 8, 64);
  const dim3 grid(cdiv(B * (T + Q), 4));
  if (vpl <= 1) hipLaunchKernelGGL(layernorm_pair_kernel<1>, grid, dim3(256), 0, stream, kv_in, q_in, x, lat, g1, b1, g2, b2, B, T, Q, C, eps);
  else if (vpl == 2) hipLaunchKernelGGL(layernorm_pair_kernel<2>, grid, dim3(256), 0, stream, kv_in, q_in, x, lat, g1, b1, g2, b2, B, T, Q, C, eps);
  else hipLaunchKernelGGL(layernorm_pair_kernel<4>, grid, dim3(256), 0, stream, kv_in, q_in, x, lat, g1, b1, g2, b2, B, T, Q, C, eps);
  SDEO_HIP(hipGetLastError());
  return 0;
}

static int layernorm_f32(float* y, const float* x, const float* gamma, const float* beta, int rows, int C, float eps, hipStream_t stream) {
  SDEO_CHECK(y && x && gamma && beta, "layernorm_f32: null operand");
  SDEO_CHECK(rows >= 1 && rows <= 1 << 24 && C >= 4 && C % 4 == 0, "layernorm_f32: rows=%d C=%d (C a positive multiple of 4)", rows, C);
  SDEO_CHECK(C <= 2048, "layernorm_f32: C=%d > 2048 unsupported", C);
  SDEO_CHECK(aligned16(y) && aligned16(x) && aligned16(gamma) && aligned16(beta), "layernorm_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(layernorm_f32_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, y, x, gamma, beta, rows, C, eps);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace

struct sdeo_resampler_handle_s : ProgramHandle {
  sdeo_resampler_config cfg{};
  // configured state
  int batch = 0;
  const float* in = nullptr;     // the caller's hidden / tokens_out of the project under way
  float* out = nullptr;

  void free_configured() {
    batch = 0;
    ProgramHandle::free_configured();
  }
};

namespace {

typedef sdeo_resampler_handle_s Res;

// names follow the adapter file's keys below "image_proj."
static void build_registry(Res* e) {
  const sdeo_resampler_config& c = e->cfg;
  WeightStore& r = e->ws;
  const int D = c.dim, I = c.heads * c.dim_head;
  auto mat = [&](const std::string& n, int rows, int cols) { r.add(n, W_LINEAR, {rows, cols}, r.take((size_t)rows * cols * 2)); };
  auto vec = [&](const std::string& n, int len) { r.add(n, W_VEC, {len}, r.take((size_t)len * 4)); };
  r.add("latents", W_LINEAR, {1, c.num_queries, D}, r.take((size_t)c.num_queries * D * 2));      // fp16, like the stream it starts
  mat("proj_in.weight", D, c.embed_dim);
  vec("proj_in.bias", D);
  mat("proj_out.weight", c.out_dim, D);
  vec("proj_out.bias", c.out_dim);
  vec("norm_out.weight", c.out_dim);
  vec("norm_out.bias", c.out_dim);
  for (int l = 0; l < c.depth; ++l) {
    const std::string a = "layers." + std::to_string(l) + ".0.", f = "layers." + std::to_string(l) + ".1.";
    vec(a + "norm1.weight", D);
    vec(a + "norm1.bias", D);
    vec(a + "norm2.weight", D);
    vec(a + "norm2.bias", D);
    mat(a + "to_q.weight", I, D);
    mat(a + "to_kv.weight", 2 * I, D);
    mat(a + "to_out.weight", D, I);
    vec(f + "0.weight", D);
    vec(f + "0.bias", D);
    mat(f + "1.weight", c.ffn, D);
    mat(f + "3.weight", D, c.ffn);
  }
}

// the body of sdeo_resampler_configure after its checks
static int configure_impl(Res* e, int B) {
  const sdeo_resampler_config& c = e->cfg;
  const int T = c.tokens, E = c.embed_dim, D = c.dim, H = c.heads, d = c.dim_head, I = H * d, Q = c.num_queries, F = c.ffn, O = c.out_dim;
  const int xrows = B * T, lrows = B * Q, krows = B * (T + Q);
  // activation buffers: hid [B T][E] fp16; x [B T][D]; la, lb [B Q][D] (the latent stream, ping-pong); kv_in [B (T + Q)][D]; q_in, a
  // [B Q][D]; q, o [B Q][I]; kv [B (T + Q)][2 I]; ff [B Q][F]; po [B Q][O] fp32
  const size_t o_hid = e->take((size_t)xrows * E * 2), o_x = e->take((size_t)xrows * D * 2), o_la = e->take((size_t)lrows * D * 2),
               o_lb = e->take((size_t)lrows * D * 2), o_kvin = e->take((size_t)krows * D * 2), o_qin = e->take((size_t)lrows * D * 2),
               o_a = e->take((size_t)lrows * D * 2), o_q = e->take((size_t)lrows * I * 2), o_o = e->take((size_t)lrows * I * 2),
               o_kv = e->take((size_t)krows * 2 * I * 2), o_ff = e->take((size_t)lrows * F * 2), o_po = e->take((size_t)lrows * O * 4);
  if (int rc = e->alloc_act()) return rc;
  auto P16 = [&](size_t o) { return e->at<f16>(o); };
  f16 *hid = P16(o_hid), *x = P16(o_x), *la = P16(o_la), *lb = P16(o_lb), *kv_in = P16(o_kvin), *q_in = P16(o_qin), *a = P16(o_a), *q = P16(o_q),
      *o = P16(o_o), *kv = P16(o_kv), *ff = P16(o_ff);
  float* po = e->at<float>(o_po);

  auto wp = [&](const std::string& n) { return e->ws.ptr<f16>(n); };
  auto vp = [&](const std::string& n) { return e->ws.ptr<float>(n); };
  // 1. the caller's fp32 hidden states -> fp16 rows; proj_in
  e->prog.push_back(Op([=](hipStream_t s) { return f32_to_f16(hid, e->in, (int64_t)xrows * E, s); }, "f32_to_f16", 0, 6.0 * xrows * E));
  e->gemm(hid, xrows, E, wp("proj_in.weight"), D, vp("proj_in.bias"), 0, nullptr, x);
  // 2. the latent parameter into every image's rows
  {
    const f16* src = wp("latents");
    const int n8 = Q * D / 8;
    e->prog.push_back(Op([=](hipStream_t s) {
      hipLaunchKernelGGL(broadcast_rows_kernel, dim3(cdiv(B * n8, 256)), dim3(256), 0, s, la, src, B, n8);
      SDEO_HIP(hipGetLastError());
      return 0;
    }, "broadcast_rows", 0, 2.0 * (B + 1) * Q * D));
  }
  // 3. the layers
  f16* lat = la;
  f16* nxt = lb;
  const float scale = 1.0f / sqrtf((float)d);
  for (int l = 0; l < c.depth; ++l) {
    const std::string pa = "layers." + std::to_string(l) + ".0.", pf = "layers." + std::to_string(l) + ".1.";
    {
      const float *g1 = vp(pa + "norm1.weight"), *b1 = vp(pa + "norm1.bias"), *g2 = vp(pa + "norm2.weight"), *b2 = vp(pa + "norm2.bias");
      const f16* li = lat;
      e->prog.push_back(Op([=](hipStream_t s) { return layernorm_pair(kv_in, q_in, x, li, g1, b1, g2, b2, B, T, Q, D, 1e-5f, s); }, "layernorm_pair", 0,
                           4.0 * krows * D + 2.0 * lrows * D));
    }
    e->gemm(q_in, lrows, D, wp(pa + "to_q.weight"), I, nullptr, 0, nullptr, q);
    e->gemm(kv_in, krows, D, wp(pa + "to_kv.weight"), 2 * I, nullptr, 0, nullptr, kv);
    e->prog.push_back(Op([=](hipStream_t s) {
      return attention(o, I, q, I, kv, 2 * I, kv + I, 2 * I, B, H, Q, T + Q, T + Q, T + Q, d, scale, s, /*causal=*/0);
    }, "attention", 4.0 * B * H * (double)Q * (T + Q) * d, 2.0 * B * H * d * (2.0 * Q + 2.0 * (T + Q))));
    e->gemm(o, lrows, I, wp(pa + "to_out.weight"), D, nullptr, 0, lat, nxt);
    std::swap(lat, nxt);
    e->ln(a, lat, D, vp(pf + "0.weight"), vp(pf + "0.bias"), lrows, D);
    e->gemm(a, lrows, D, wp(pf + "1.weight"), F, nullptr, 5, nullptr, ff);
    e->gemm(ff, lrows, F, wp(pf + "3.weight"), D, nullptr, 0, lat, nxt);
    std::swap(lat, nxt);
  }
  // 4. proj_out in fp32, norm_out fp32 -> the caller's tokens
  e->gemm(lat, lrows, D, wp("proj_out.weight"), O, vp("proj_out.bias"), 0, nullptr, nullptr, po);
  {
    const float *g = vp("norm_out.weight"), *b = vp("norm_out.bias");
    e->prog.push_back(Op([=](hipStream_t s) { return layernorm_f32(e->out, po, g, b, lrows, O, 1e-5f, s); }, "layernorm_f32", 0, 8.0 * lrows * O));
  }
  if (int rc = e->alloc_splitk()) return rc;
  e->batch = B;
  return 0;
}

}  // namespace

extern "C" {

int sdeo_layernorm_pair_f16(void* kv_in, void* q_in, const void* x, const void* lat, const float* gamma1, const float* beta1, const float* gamma2,
                            const float* beta2, int b, int t, int q, int c, float eps, void* stream) {
  return layernorm_pair((f16*)kv_in, (f16*)q_in, (const f16*)x, (const f16*)lat, gamma1, beta1, gamma2, beta2, b, t, q, c, eps,
                        reinterpret_cast<hipStream_t>(stream));
}

int sdeo_layernorm_f32(float* y, const float* x, const float* gamma, const float* beta, int rows, int c, float eps, void* stream) {
  return layernorm_f32(y, x, gamma, beta, rows, c, eps, reinterpret_cast<hipStream_t>(stream));
}

int sdeo_resampler_create(const sdeo_resampler_config* cfg, sdeo_resampler_handle* out) {
  const char* who = "sdeo_resampler_create";
  SDEO_CHECK(cfg && out, "%s: null argument", who);
  SDEO_CHECK(cfg->tokens > 0 && cfg->embed_dim > 0 && cfg->dim > 0 && cfg->depth > 0 && cfg->dim_head > 0 && cfg->heads > 0 && cfg->ffn > 0 &&
             cfg->out_dim > 0, "%s: empty config", who);
  SDEO_CHECK(cfg->tokens <= 4096 && cfg->depth <= 64, "%s: tokens %d / depth %d out of range (<= 4096, <= 64)", who, cfg->tokens, cfg->depth);
  SDEO_CHECK(cfg->embed_dim % 8 == 0 && cfg->dim % 8 == 0 && cfg->ffn % 8 == 0 && cfg->out_dim % 8 == 0,
             "%s: embed_dim %d / dim %d / ffn %d / out_dim %d must be multiples of 8", who, cfg->embed_dim, cfg->dim, cfg->ffn, cfg->out_dim);
  SDEO_CHECK(cfg->dim <= 2048 && cfg->out_dim <= 2048, "%s: dim %d / out_dim %d > 2048 unsupported (LayerNorm)", who, cfg->dim, cfg->out_dim);
  SDEO_CHECK(cfg->embed_dim <= 16384 && cfg->ffn <= 16384, "%s: embed_dim %d / ffn %d > 16384 unsupported", who, cfg->embed_dim, cfg->ffn);
  SDEO_CHECK(cfg->num_queries >= 1 && cfg->num_queries <= 64, "%s: num_queries %d out of range (1..64, what sdeo_enable_ip_adapter takes)", who,
             cfg->num_queries);
  const int64_t inner = (int64_t)cfg->heads * cfg->dim_head;
  SDEO_CHECK(inner % 8 == 0 && inner <= 8192 && cfg->heads <= 1024,
             "%s: heads %d * dim_head %d = %lld is not an inner width to_q / to_kv / to_out can have (a multiple of 8, <= 8192)", who, cfg->heads,
             cfg->dim_head, (long long)inner);
  const int d = cfg->dim_head, Tk = cfg->tokens + cfg->num_queries;
  SDEO_CHECK(d % 8 == 0 && d <= 160 && attention_kernel_name(1, cfg->heads, cfg->num_queries, Tk, d, 0) != nullptr,
             "%s: head dim %d unsupported (8..96 in steps of 8, 120, 128, 152, 160)", who, d);
  Res* e = new Res();
  e->cfg = *cfg;
  build_registry(e);
  return handle_created(who, e, out);
}

int sdeo_resampler_destroy(sdeo_resampler_handle h) { return handle_destroy(h); }

int sdeo_resampler_num_weights(sdeo_resampler_handle h) { return handle_num_weights(h); }

int sdeo_resampler_weight_info(sdeo_resampler_handle h, int i, const char** name, int64_t dims[4], int* ndim) {
  return handle_weight_info("sdeo_resampler_weight_info", h, i, name, dims, 4, 1, ndim);
}

int sdeo_resampler_load_weight(sdeo_resampler_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict) {
  const char* who = "sdeo_resampler_load_weight";
  SDEO_CHECK(h && name && host_data && dims, "%s: null argument", who);
  return h->ws.load(who, name, registry_key(name, "image_proj."), host_data, dims, ndim, strict);
}

int sdeo_resampler_finalize_weights(sdeo_resampler_handle h) { return handle_finalize_weights("sdeo_resampler_finalize_weights", h); }

int sdeo_resampler_configure(sdeo_resampler_handle h, int batch) {
  SDEO_CHECK(h && h->finalized, "sdeo_resampler_configure: weights not finalized");
  SDEO_CHECK(batch >= 1 && batch <= 16, "sdeo_resampler_configure: batch=%d out of range (1..16)", batch);
  return handle_configure(h, [&] { return configure_impl(h, batch); });
}

int sdeo_resampler_num_launches(sdeo_resampler_handle h) { return h ? (int)h->prog.size() : 0; }

int sdeo_resampler_project(sdeo_resampler_handle h, const float* hidden, int batch, float* tokens_out, void* stream) {
  const char* who = "sdeo_resampler_project";
  SDEO_CHECK(h && hidden && tokens_out, "%s: null argument", who);
  SDEO_CHECK(h->finalized, "%s: weights not finalized (call sdeo_resampler_finalize_weights)", who);
  SDEO_CHECK(h->batch > 0, "%s: the handle is not configured (call sdeo_resampler_configure)", who);
  SDEO_CHECK(batch == h->batch, "%s: batch %d != configured %d", who, batch, h->batch);
  SDEO_CHECK(aligned16(hidden) && aligned16(tokens_out), "%s: hidden and tokens_out must be 16-byte aligned", who);
  h->in = hidden;
  h->out = tokens_out;
  return run_program(h->prog, reinterpret_cast<hipStream_t>(stream));
}

size_t sdeo_resampler_device_bytes(sdeo_resampler_handle h) { return handle_device_bytes(h); }

}  // extern "C"
