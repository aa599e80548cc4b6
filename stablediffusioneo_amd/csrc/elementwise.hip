// Memory-bound elementwise / layout kernels of the CNSD path (gfx950): 16-byte vector accesses,
// grid-stride loops, fp32 math.
#include "kernels.h"

#include <cmath>
#include <type_traits>

namespace sdeo {

static inline dim3 grid_for(int64_t work_items) {
  int64_t b = cdiv64(work_items, 256);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// GEGLU (`attention.py:49-56`): y = a[:, :C] * gelu(a[:, C:]) with the exact erf GELU (F.gelu default).
__global__ __launch_bounds__(256) void geglu_kernel(f16* __restrict__ y, int ldy, const f16* __restrict__ a, int lda,
                                                    int64_t rows, int C) {
  const int nvec = C / 8;
  const int64_t total = rows * nvec;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / nvec;
    const int v = (int)(i - r * nvec);
    const f16x8 xv = *reinterpret_cast<const f16x8*>(a + r * lda + v * 8);
    const f16x8 gv = *reinterpret_cast<const f16x8*>(a + r * lda + C + v * 8);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = (float)gv[j];
      const float ge = 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f));
      o[j] = (f16)((float)xv[j] * ge);
    }
    *reinterpret_cast<f16x8*>(y + r * ldy + v * 8) = o;
  }
}

int geglu(f16* y, int ldy, const f16* a, int lda, int rows, int C, hipStream_t stream) {
  SDEO_CHECK(y && a && rows > 0 && C > 0 && C % 8 == 0 && ldy % 8 == 0 && lda % 8 == 0, "geglu: bad operand");
  hipLaunchKernelGGL(geglu_kernel, grid_for((int64_t)rows * (C / 8)), dim3(256), 0, stream, y, ldy, a, lda, (int64_t)rows, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void add_scaled_kernel(f16* y, int ldy, const f16* a, int lda,   // y may alias a
                                                         const f16* __restrict__ b, int ldb, float scale, int64_t rows,
                                                         int C) {
  const int nvec = C / 8;
  const int64_t total = rows * nvec;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / nvec;
    const int v = (int)(i - r * nvec);
    f16x8 av = *reinterpret_cast<const f16x8*>(a + r * lda + v * 8);
    if (b) {
      const f16x8 bv = *reinterpret_cast<const f16x8*>(b + r * ldb + v * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) av[j] = (f16)((float)av[j] + (float)bv[j] * scale);
    }
    *reinterpret_cast<f16x8*>(y + r * ldy + v * 8) = av;
  }
}

int add_scaled(f16* y, int ldy, const f16* a, int lda, const f16* b, int ldb, float scale, int rows, int C,
               hipStream_t stream) {
  SDEO_CHECK(y && a && rows > 0 && C > 0 && C % 8 == 0 && ldy % 8 == 0 && lda % 8 == 0 && (!b || ldb % 8 == 0),
             "add_scaled: bad operand");
  hipLaunchKernelGGL(add_scaled_kernel, grid_for((int64_t)rows * (C / 8)), dim3(256), 0, stream, y, ldy, a, lda, b, ldb,
                     scale, (int64_t)rows, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// timestep_embedding (`util.py:154-174`): [cos(t*f_i), sin(t*f_i)], f_i = exp(-ln(1e4) * i / half)
__global__ void timestep_embedding_kernel(f16* __restrict__ out, const int64_t* __restrict__ t, int B, int dim) {
  const int half = dim / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, k = i - b * half;
  const float freq = expf(-9.210340371976184f * (float)k / (float)half);
  const float arg = (float)t[b] * freq;
  out[(size_t)b * dim + k] = (f16)cosf(arg);
  out[(size_t)b * dim + half + k] = (f16)sinf(arg);
  if ((dim & 1) && k == 0) out[(size_t)b * dim + dim - 1] = (f16)0.f;
}

int timestep_embedding(f16* out, const int64_t* t, int B, int dim, hipStream_t stream) {
  SDEO_CHECK(out && t && B > 0 && dim > 1, "timestep_embedding: bad operand");
  const int n = B * (dim / 2);
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, out, t, B, dim);
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void silu_kernel(f16* __restrict__ y, const f16* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = (f16)silu_f((float)x[i]);
}

int silu(f16* y, const f16* x, int64_t n, hipStream_t stream) {
  SDEO_CHECK(y && x && n > 0, "silu: bad operand");
  hipLaunchKernelGGL(silu_kernel, grid_for(n), dim3(256), 0, stream, y, x, n);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// NCHW fp32 -> NHWC fp16 with channel padding to ldy (pad channels written as 0). One thread per pixel.
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(f16* __restrict__ y, int ldy, const float* __restrict__ x, int B,
                                                           int C, int HW, float scale) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW;
    const int64_t pix = i - b * HW;
    for (int c = 0; c < ldy; ++c)
      y[i * ldy + c] = c < C ? (f16)(x[(b * C + c) * HW + pix] * scale) : (f16)0.f;
  }
}

int nchw_f32_to_nhwc_f16(f16* y, int ldy, const float* x, int B, int C, int HW, float scale, hipStream_t stream) {
  SDEO_CHECK(y && x && B > 0 && C > 0 && HW > 0 && ldy >= C, "nchw_f32_to_nhwc_f16: bad operand");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid_for((int64_t)B * HW), dim3(256), 0, stream, y, ldy, x, B, C, HW, scale);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// NHWC fp16 -> NCHW fp32 (times scale). Thread per (b, c, pix) element, pix fastest => coalesced writes.
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(float* __restrict__ y, const f16* __restrict__ x, int ldx, int B,
                                                           int C, int HW, float scale) {
  const int64_t total = (int64_t)B * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t pix = i % HW;
    const int64_t bc = i / HW;
    const int64_t c = bc % C, b = bc / C;
    y[i] = (float)x[(b * HW + pix) * ldx + c] * scale;
  }
}

int nhwc_f16_to_nchw_f32(float* y, const f16* x, int ldx, int B, int C, int HW, float scale, hipStream_t stream) {
  SDEO_CHECK(y && x && B > 0 && C > 0 && HW > 0 && ldx >= C, "nhwc_f16_to_nchw_f32: bad operand");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid_for((int64_t)B * C * HW), dim3(256), 0, stream, y, x, ldx, B, C, HW, scale);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// post-process (`canny2image_torch.py:68`): (x*127.5+127.5).clip(0,255).astype(uint8), truncation like numpy
__global__ __launch_bounds__(256) void to_u8_kernel(uint8_t* __restrict__ y, const f16* __restrict__ x, int ldx,
                                                    int64_t pixels, int C) {
  const int64_t total = pixels * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t pix = i / C;
    const int c = (int)(i - pix * C);
    float v = (float)x[pix * ldx + c] * 127.5f + 127.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    y[i] = (uint8_t)v;
  }
}

int nhwc_f16_to_nhwc_u8(uint8_t* y, const f16* x, int ldx, int64_t pixels, int C, hipStream_t stream) {
  SDEO_CHECK(y && x && pixels > 0 && C > 0 && ldx >= C, "nhwc_f16_to_nhwc_u8: bad operand");
  hipLaunchKernelGGL(to_u8_kernel, grid_for(pixels * C), dim3(256), 0, stream, y, x, ldx, pixels, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// weights: fp32 OIHW -> fp16 O,R,S,Ipad (K-contiguous KRSC, zero-padded input channels)
__global__ __launch_bounds__(256) void oihw_to_ohwi_kernel(f16* __restrict__ y, const float* __restrict__ w, int O, int I,
                                                           int R, int S, int Ipad) {
  const int64_t total = (int64_t)O * R * S * Ipad;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % Ipad);
    const int64_t t = i / Ipad;
    const int s = (int)(t % S);
    const int64_t t2 = t / S;
    const int r = (int)(t2 % R);
    const int64_t o = t2 / R;
    y[i] = c < I ? (f16)w[((o * I + c) * R + r) * S + s] : (f16)0.f;
  }
}

int oihw_f32_to_ohwi_f16(f16* y, const float* w, int O, int I, int R, int S, int Ipad, hipStream_t stream) {
  SDEO_CHECK(y && w && O > 0 && I > 0 && R > 0 && S > 0 && Ipad >= I, "oihw_f32_to_ohwi_f16: bad operand");
  hipLaunchKernelGGL(oihw_to_ohwi_kernel, grid_for((int64_t)O * R * S * Ipad), dim3(256), 0, stream, y, w, O, I, R, S, Ipad);
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void pad_rows_kernel(f16* __restrict__ y, const float* __restrict__ x, int B, int T, int Tpad,
                                                       int C) {
  const int64_t total = (int64_t)B * Tpad * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int t = (int)(r % Tpad);
    const int64_t b = r / Tpad;
    y[i] = t < T ? (f16)x[(b * T + t) * C + c] : (f16)0.f;
  }
}

int pad_rows_f32_to_f16(f16* y, const float* x, int B, int T, int Tpad, int C, hipStream_t stream) {
  SDEO_CHECK(y && x && B > 0 && T > 0 && Tpad >= T && C > 0, "pad_rows_f32_to_f16: bad operand");
  hipLaunchKernelGGL(pad_rows_kernel, grid_for((int64_t)B * Tpad * C), dim3(256), 0, stream, y, x, B, T, Tpad, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void transpose_pad_kernel(f16* __restrict__ vt, int ldvt, const f16* __restrict__ v, int ldv, int B,
                                                            int T, int TkSv, int C) {
  const int64_t total = (int64_t)B * T * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int t = (int)(r % T);
    const int b = (int)(r / T);
    vt[(size_t)c * ldvt + (size_t)b * TkSv + t] = v[(size_t)r * ldv + c];
  }
}

int transpose_pad(f16* vt, int ldvt, const f16* v, int ldv, int B, int T, int TkSv, int C, hipStream_t stream) {
  SDEO_CHECK(vt && v && B > 0 && T > 0 && TkSv >= T && C > 0, "transpose_pad: bad operand");
  hipLaunchKernelGGL(transpose_pad_kernel, grid_for((int64_t)B * T * C), dim3(256), 0, stream, vt, ldvt, v, ldv, B, T, TkSv, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void zero_f16_kernel(f16* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = (f16)0.f;
}

int zero_f16(f16* y, int64_t n, hipStream_t stream) {
  SDEO_CHECK(y && n > 0, "zero_f16: bad operand");
  hipLaunchKernelGGL(zero_f16_kernel, grid_for(n), dim3(256), 0, stream, y, n);
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void f32_to_f16_kernel(f16* __restrict__ y, const float* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = (f16)x[i];
}

int f32_to_f16(f16* y, const float* x, int64_t n, hipStream_t stream) {
  SDEO_CHECK(y && x && n > 0, "f32_to_f16: bad operand");
  hipLaunchKernelGGL(f32_to_f16_kernel, grid_for(n), dim3(256), 0, stream, y, x, n);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// GEGLU weight interleave (load time): row j of the [2H][cols] projection (`attention.py:49-56`: rows 0..H-1 = values,
// H..2H-1 = gates) goes to row 32*(j'/16) + 16*is_gate + j'%16 with j' = j mod H, so that the GEMM epilogue finds a value
// and its gate in neighbouring 16-wide accumulator tiles of the same lane.  cols = 1 with OUT = float handles the bias.
template <typename OUT>
__global__ __launch_bounds__(256) void geglu_interleave_kernel(OUT* __restrict__ y, const float* __restrict__ x, int H, int64_t cols) {
  const int64_t n = (int64_t)2 * H * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i / cols);
    const int64_t c = i - (int64_t)j * cols;
    const int gate = j >= H, jj = gate ? j - H : j;
    const int dst = 32 * (jj >> 4) + 16 * gate + (jj & 15);
    y[(int64_t)dst * cols + c] = (OUT)x[i];
  }
}

int geglu_interleave_f32_to_f16(f16* y, const float* x, int H, int cols, hipStream_t stream) {
  SDEO_CHECK(y && x && H > 0 && H % 16 == 0 && cols > 0, "geglu_interleave: bad operand (H=%d must be a multiple of 16)", H);
  hipLaunchKernelGGL(geglu_interleave_kernel<f16>, grid_for((int64_t)2 * H * cols), dim3(256), 0, stream, y, x, H, (int64_t)cols);
  SDEO_HIP(hipGetLastError());
  return 0;
}

int geglu_interleave_f32(float* y, const float* x, int H, hipStream_t stream) {
  SDEO_CHECK(y && x && H > 0 && H % 16 == 0, "geglu_interleave: bad operand (H=%d must be a multiple of 16)", H);
  hipLaunchKernelGGL(geglu_interleave_kernel<float>, grid_for((int64_t)2 * H), dim3(256), 0, stream, y, x, H, (int64_t)1);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// CFG combine + DDIM update (`cldm/ddim_hacked.py:192,208-231`), eps-parameterisation, fp32 NCHW latents.
//   e = eps_u + s*(eps_c - eps_u);  pred_x0 = (x - sqrt(1-a_t) e)/sqrt(a_t)
//   x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) e + sigma * noise
// one element of the update; shared by both kernels below so that they round alike
__device__ __forceinline__ void cfg_ddim_elem(float x, float c, float u, bool guided, float s, float rsqrt_at, float sqrt_aprev, float dir_coef,
                                              float sqrt_1m_at, float& p0, float& xp) {
  // explicit fused multiply-adds: left to the compiler, the contraction of a * b + c * d differs from kernel to kernel
  const float e = guided ? fmaf(s, c - u, u) : c;
  p0 = fmaf(-sqrt_1m_at, e, x) * rsqrt_at;
  xp = fmaf(sqrt_aprev, p0, dir_coef * e);
}

// The v-parameterisation of the same step (SD-2.x 768-v; upstream LatentDiffusion.predict_eps_from_z_and_v / predict_start_from_z_and_v,
// called at `cldm/ddim_hacked.py:194-197,214-217`): the model outputs are combined first, v = v_u + s (v_c - v_u), then with
// a = sqrt(a_t), s1 = sqrt(1 - a_t):   e = a v + s1 x;   pred_x0 = a x - s1 v;   x_prev as above.  No division.
__device__ __forceinline__ void cfg_ddim_elem_v(float x, float c, float u, bool guided, float s, float sqrt_at, float sqrt_aprev, float dir_coef,
                                                float sqrt_1m_at, float& p0, float& xp) {
  const float v = guided ? fmaf(s, c - u, u) : c;
  const float e = fmaf(sqrt_at, v, sqrt_1m_at * x);
  p0 = fmaf(sqrt_at, x, -(sqrt_1m_at * v));
  xp = fmaf(sqrt_aprev, p0, dir_coef * e);
}

// VPRED: `at_coef` is sqrt(a_t) and the model output is v; else 1 / sqrt(a_t) and eps (both kernels below)
template <bool VPRED>
__device__ __forceinline__ void cfg_ddim_elem_sel(float x, float c, float u, bool guided, float s, float at_coef, float sqrt_aprev, float dir_coef,
                                                  float sqrt_1m_at, float& p0, float& xp) {
  if constexpr (VPRED) cfg_ddim_elem_v(x, c, u, guided, s, at_coef, sqrt_aprev, dir_coef, sqrt_1m_at, p0, xp);
  else cfg_ddim_elem(x, c, u, guided, s, at_coef, sqrt_aprev, dir_coef, sqrt_1m_at, p0, xp);
}

// The launch-time choice of a kernel's bool template parameters: f receives the two flags as std::bool_constant values, so that its body
// can name K<v.value, n.value>.  Every launcher of the sampler-step family below chooses its instantiation through it.
template <typename F>
static inline void with_flags(bool a, bool b, F&& f) {
  if (a) {
    if (b) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
  } else {
    if (b) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
  }
}

// a third flag in front of the two: f receives it first
template <typename F>
static inline void with_flags(bool p, bool a, bool b, F&& f) {
  if (p) with_flags(a, b, [&](auto x, auto y) { f(std::true_type{}, x, y); });
  else with_flags(a, b, [&](auto x, auto y) { f(std::false_type{}, x, y); });
}

// `noise` (fp32, laid out like x) adds the sampler's noise term (`cldm/ddim_hacked.py:227-230`, eta > 0): one fused multiply-add on the
// finished update, stated as fmaf here and in the pair kernel so that the two round alike whatever the compiler does.
template <bool VPRED>
__global__ __launch_bounds__(256) void cfg_ddim_kernel(float* __restrict__ x_prev, float* __restrict__ pred_x0,
                                                       const float* __restrict__ x, const float* __restrict__ ec,
                                                       const float* __restrict__ eu, const float* __restrict__ noise,
                                                       float s, float at_coef, float sqrt_aprev, float dir_coef, float sigma,
                                                       float sqrt_1m_at, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float p0, xp;
    cfg_ddim_elem_sel<VPRED>(x[i], ec[i], eu ? eu[i] : 0.f, eu != nullptr, s, at_coef, sqrt_aprev, dir_coef, sqrt_1m_at, p0, xp);
    if (noise) xp = fmaf(sigma, noise[i], xp);
    x_prev[i] = xp;
    if (pred_x0) pred_x0[i] = p0;
  }
}

// The loop of every kernel that leaves the fp16 NHWC latent of the next forward in x0: one thread per (image, pixel) of a latent
// [b][C][HW], and what elem(i, n, c, pix, j) returns for channel c (j: the element's index in the fp32 NCHW latent, i = n * HW + pix) goes
// to both halves of the CFG pair (images n and n + b), padding channels zero.  elem does its own fp32 loads and stores.
// PAIRED = false is the un-paired member of every kernel below (SDEO_STEP_UNGUIDED): b is then the whole batch, each image is staged
// once, and the model output of image n is used as it is (the `guided = false` leg of the element functions).
template <bool PAIRED, typename F>
__device__ __forceinline__ void stage_pair(f16* __restrict__ x0, int ld0, int b, int C, int HW, F elem) {
  const int64_t total = (int64_t)b * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / HW, pix = i - n * HW;
    for (int c = 0; c < ld0; ++c) {
      const f16 v = c < C ? (f16)elem(i, n, c, pix, (n * C + c) * HW + pix) : (f16)0.f;
      x0[i * ld0 + c] = v;
      if constexpr (PAIRED) x0[(i + total) * ld0 + c] = v;
    }
  }
}

// The same update for the fused CFG pair inside the library (the sdeo_ddim_step family): eps comes straight from the UNet's fp16 NHWC
// output (images 0..b-1 conditional, b..2b-1 unconditional), x [b][C][HW] fp32 is updated in place, and the latent of the NEXT forward is
// staged on the way out (from the noisy value when NOISE).
template <bool PAIRED, bool VPRED, bool NOISE>
__global__ __launch_bounds__(256) void cfg_ddim_pair_kernel(float* __restrict__ x, float* __restrict__ pred_x0, const f16* __restrict__ eps,
                                                            int lde, const float* __restrict__ noise, f16* __restrict__ x0, int ld0, int b,
                                                            int C, int HW, float s, float at_coef, float sqrt_aprev, float dir_coef,
                                                            float sigma, float sqrt_1m_at) {
  const int64_t total = (int64_t)b * HW;
  stage_pair<PAIRED>(x0, ld0, b, C, HW, [=](int64_t i, int64_t, int c, int64_t, int64_t j) {
    float p0, xp;
    cfg_ddim_elem_sel<VPRED>(x[j], (float)eps[i * lde + c], PAIRED ? (float)eps[(i + total) * lde + c] : 0.f, PAIRED, s, at_coef, sqrt_aprev,
                             dir_coef, sqrt_1m_at, p0, xp);
    if constexpr (NOISE) xp = fmaf(sigma, noise[j], xp);
    x[j] = xp;
    if (pred_x0) pred_x0[j] = p0;
    return xp;
  });
}

// What the DDIM update refuses, host only: callers that change x before it (the blend) or must leave x untouched refuse up front.
// sigma_t null: the deterministic update, which takes no noise.
int cfg_ddim_check(const char* who, float a_t, float a_prev, const float* noise, const float* sigma_t) {
  if (!sigma_t) {
    SDEO_CHECK(a_t > 0.f && (1.f - a_prev) >= 0.f, "%s: invalid schedule a_t=%g a_prev=%g", who, a_t, a_prev);
    return 0;
  }
  const float sg = *sigma_t;
  SDEO_CHECK(std::isfinite(a_t) && std::isfinite(a_prev) && std::isfinite(sg), "%s: non-finite coefficient a_t=%g a_prev=%g sigma_t=%g", who,
             a_t, a_prev, sg);
  SDEO_CHECK(noise || sg == 0.f, "%s: sigma_t=%g needs the step noise, but noise is null", who, sg);
  SDEO_CHECK(a_t > 0.f, "%s: invalid schedule a_t=%g", who, a_t);
  SDEO_CHECK((1.f - a_prev - sg * sg) >= 0.f, "%s: 1 - a_prev - sigma_t^2 < 0 (a_prev=%g sigma_t=%g)", who, a_prev, sg);
  return 0;
}

// noise set: the stochastic update, bit-equal to cfg_ddim_step with the same noise / sigma_t; null: sigma_t is not read
int cfg_ddim_pair(float* x, float* pred_x0, const f16* eps, int lde, const float* noise, float sigma_t, f16* x0, int ld0, int b, int C, int HW,
                  float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at, bool v_prediction, bool paired, hipStream_t stream) {
  SDEO_CHECK(x && eps && x0 && b > 0 && C > 0 && HW > 0 && lde >= C && ld0 >= C, "cfg_ddim_pair: bad operand");
  if (int rc = cfg_ddim_check("cfg_ddim_pair", a_t, a_prev, noise, noise ? &sigma_t : nullptr)) return rc;
  // the coefficients as cfg_ddim_step forms them, expression for expression
  const float sg = noise ? sigma_t : 0.f;
  with_flags(paired, v_prediction, noise != nullptr, [&](auto p, auto v, auto n) {
    hipLaunchKernelGGL((cfg_ddim_pair_kernel<p.value, v.value, n.value>), grid_for((int64_t)b * HW), dim3(256), 0, stream, x, pred_x0, eps, lde,
                       noise, x0, ld0, b, C, HW, cfg_scale, v.value ? sqrtf(a_t) : 1.0f / sqrtf(a_t), sqrtf(a_prev), sqrtf(1.f - a_prev - sg * sg), sg,
                       sqrt_one_minus_at);
  });
  SDEO_HIP(hipGetLastError());
  return 0;
}

// latent [b][C][HW] fp32 -> fp16 NHWC for BOTH halves of the CFG pair (un-paired: each image once)
template <bool PAIRED>
__global__ __launch_bounds__(256) void latent_pair_kernel(f16* __restrict__ x0, int ld0, const float* __restrict__ x, int b, int C, int HW) {
  stage_pair<PAIRED>(x0, ld0, b, C, HW, [=](int64_t, int64_t, int, int64_t, int64_t j) { return x[j]; });
}

int latent_pair_to_nhwc(f16* x0, int ld0, const float* x, int b, int C, int HW, bool paired, hipStream_t stream) {
  SDEO_CHECK(x0 && x && b > 0 && C > 0 && HW > 0 && ld0 >= C, "latent_pair_to_nhwc: bad operand");
  hipLaunchKernelGGL(paired ? latent_pair_kernel<true> : latent_pair_kernel<false>, grid_for((int64_t)b * HW), dim3(256), 0, stream, x0, ld0,
                     x, b, C, HW);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// The sampler's mask / x0 blend (cldm/ddim_hacked.py:154-157): x <- mask * q_sample(orig) + (1 - mask) * x with
// q_sample(orig) = sqrt_a * orig + sqrt_1ma * noise.  The eager loop evaluates this as seven separate torch kernels, each rounding once;
// hipcc's default (-ffp-contract=fast) fuses a product into the sum that follows it.  HIP's __fmul_rn / __fadd_rn state the intent but are
// plain operators to the compiler, and `#pragma clang fp contract(off)` does not reach the backend's combiner either: with both, q still
// came out as ONE v_pk_fma_f32 (product unrounded).  So every product passes through an empty asm statement: the compiler must hold the
// rounded fp32 value in a register there and cannot see through it to fuse.  It costs no instruction.  Checked in the ISA of both
// kernels: four multiplies, a subtract and two adds, no fma.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ float mask_blend_elem(float x, float orig, float noise, float m, float sqrt_a, float sqrt_1ma) {
  const float q = __fadd_rn(rounded(__fmul_rn(sqrt_a, orig)), rounded(__fmul_rn(sqrt_1ma, noise)));
  return __fadd_rn(rounded(__fmul_rn(q, m)), rounded(__fmul_rn(__fsub_rn(1.0f, m), x)));
}

// mask [mask_n][mask_c][HW], mask_n in {1, n}, mask_c in {1, C}: the element of image n, channel c, pixel pix
__device__ __forceinline__ int64_t mask_index(int64_t n, int64_t c, int64_t pix, int mask_n, int mask_c, int HW) {
  return ((mask_n == 1 ? 0 : n) * mask_c + (mask_c == 1 ? 0 : c)) * HW + pix;
}

// fp32 NCHW operands [n][C][HW], one thread per element; x is read and written by the same thread at the same index
__global__ __launch_bounds__(256) void mask_blend_kernel(float* x, const float* __restrict__ orig, const float* __restrict__ noise,
                                                         const float* __restrict__ mask, int mask_n, int mask_c, float sqrt_a,
                                                         float sqrt_1ma, int64_t total, int C, int HW) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t plane = i / HW, pix = i - plane * HW;
    const int64_t n = plane / C, c = plane - n * C;
    x[i] = mask_blend_elem(x[i], orig[i], noise[i], mask[mask_index(n, c, pix, mask_n, mask_c, HW)], sqrt_a, sqrt_1ma);
  }
}

// The blend as the front of a fused CFG-pair step: x [b][C][HW] is blended in place and the blended latent is staged.
template <bool PAIRED>
__global__ __launch_bounds__(256) void mask_blend_pair_kernel(float* x, const float* __restrict__ orig, const float* __restrict__ noise,
                                                              const float* __restrict__ mask, int mask_n, int mask_c, float sqrt_a,
                                                              float sqrt_1ma, f16* __restrict__ x0, int ld0, int b, int C, int HW) {
  stage_pair<PAIRED>(x0, ld0, b, C, HW, [=](int64_t, int64_t n, int c, int64_t pix, int64_t j) {
    const float xb = mask_blend_elem(x[j], orig[j], noise[j], mask[mask_index(n, c, pix, mask_n, mask_c, HW)], sqrt_a, sqrt_1ma);
    x[j] = xb;
    return xb;
  });
}

int mask_blend_check(const char* who, const float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c,
                     int n, int C, int HW) {
  SDEO_CHECK(x, "%s: null latent", who);
  SDEO_CHECK(orig, "%s: null orig (the known latent)", who);
  SDEO_CHECK(noise, "%s: null noise", who);
  SDEO_CHECK(mask, "%s: null mask", who);
  SDEO_CHECK(n > 0 && C > 0 && HW > 0, "%s: empty latent (n=%d c=%d hw=%d)", who, n, C, HW);
  SDEO_CHECK(mask_n == 1 || mask_n == n, "%s: mask_n=%d, but the mask holds 1 or n=%d images", who, mask_n, n);
  SDEO_CHECK(mask_c == 1 || mask_c == C, "%s: mask_c=%d, but the mask holds 1 or c=%d channels", who, mask_c, C);
  return 0;
}

int mask_blend(float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c, float sqrt_a, float sqrt_1ma,
               int n, int C, int HW, hipStream_t stream) {
  if (int rc = mask_blend_check("mask_blend", x, orig, noise, mask, mask_n, mask_c, n, C, HW)) return rc;
  const int64_t total = (int64_t)n * C * HW;
  hipLaunchKernelGGL(mask_blend_kernel, grid_for(total), dim3(256), 0, stream, x, orig, noise, mask, mask_n, mask_c, sqrt_a, sqrt_1ma, total,
                     C, HW);
  SDEO_HIP(hipGetLastError());
  return 0;
}

int mask_blend_pair(float* x, const float* orig, const float* noise, const float* mask, int mask_n, int mask_c, float sqrt_a,
                    float sqrt_1ma, f16* x0, int ld0, int b, int C, int HW, bool paired, hipStream_t stream) {
  if (int rc = mask_blend_check("mask_blend_pair", x, orig, noise, mask, mask_n, mask_c, b, C, HW)) return rc;
  SDEO_CHECK(x0 && ld0 >= C, "mask_blend_pair: bad staging operand");
  hipLaunchKernelGGL(paired ? mask_blend_pair_kernel<true> : mask_blend_pair_kernel<false>, grid_for((int64_t)b * HW), dim3(256), 0, stream,
                     x, orig, noise, mask, mask_n, mask_c, sqrt_a, sqrt_1ma, x0, ld0, b, C, HW);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// dst = (gen * m + orig * (255 - m) + 127) / 255 in integers: uint8 HWC images of C channels, uint8 [H][W] mask; one thread per pixel
__global__ __launch_bounds__(256) void composite_u8_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ gen,
                                                           const uint8_t* __restrict__ orig, const uint8_t* __restrict__ mask,
                                                           int64_t pixels, int C) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    const int m = mask[i];
    for (int c = 0; c < C; ++c) {
      const int64_t j = i * C + c;
      dst[j] = (uint8_t)(((int)gen[j] * m + (int)orig[j] * (255 - m) + 127) / 255);
    }
  }
}

int composite_u8(uint8_t* dst, const uint8_t* gen, const uint8_t* orig, const uint8_t* mask, int H, int W, int C, hipStream_t stream) {
  SDEO_CHECK(dst && gen && orig && mask, "composite_u8: null argument");
  SDEO_CHECK(H >= 1 && W >= 1 && C >= 1 && C <= 4, "composite_u8: h=%d w=%d c=%d (h, w >= 1, c in 1..4)", H, W, C);
  const int64_t pixels = (int64_t)H * W;
  hipLaunchKernelGGL(composite_u8_kernel, grid_for(pixels), dim3(256), 0, stream, dst, gen, orig, mask, pixels, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

int cfg_ddim_step(float* x_prev, float* pred_x0, const float* x, const float* eps_c, const float* eps_u, const float* noise,
                  float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, int64_t n, bool v_prediction,
                  hipStream_t stream) {
  SDEO_CHECK(x_prev && x && eps_c && n > 0, "cfg_ddim_step: bad operand");
  SDEO_CHECK(a_t > 0.f && (1.f - a_prev - sigma_t * sigma_t) >= 0.f, "cfg_ddim_step: invalid schedule a_t=%g a_prev=%g sigma=%g",
             a_t, a_prev, sigma_t);
  with_flags(v_prediction, false, [&](auto v, auto) {
    hipLaunchKernelGGL(cfg_ddim_kernel<v.value>, grid_for(n), dim3(256), 0, stream, x_prev, pred_x0, x, eps_c, eps_u, noise, cfg_scale,
                       v.value ? sqrtf(a_t) : 1.0f / sqrtf(a_t), sqrtf(a_prev), sqrtf(1.f - a_prev - sigma_t * sigma_t), sigma_t,
                       sqrt_one_minus_at, n);
  });
  SDEO_HIP(hipGetLastError());
  return 0;
}

// CFG combine + one linear-multistep update (DPM-Solver++(2M), Lu et al. 2022): D is the data prediction cfg_ddim_elem_sel forms as
// pred_x0 (so it is bit-equal to the DDIM kernels'), x_next = k_x x + k_d D + k_p D_prev.  The host folds the log-SNR arithmetic into the
// three coefficients; k_p == 0 is the first-order step (algebraically the eta = 0 DDIM step) and never reads D_prev.
// one element of the update; shared by both kernels below so that they round alike
template <bool VPRED>
__device__ __forceinline__ void cfg_lms_elem(float x, float c, float u, bool guided, float s, float at_coef, float sqrt_1m_at, float k_x, float k_d,
                                             float k_p, float d_prev, float& p0, float& xn) {
  float xp;                                   // the DDIM x_prev: not wanted here (its coefficients are passed as zero)
  cfg_ddim_elem_sel<VPRED>(x, c, u, guided, s, at_coef, 0.f, 0.f, sqrt_1m_at, p0, xp);
  xn = fmaf(k_d, p0, k_x * x);
  if (k_p != 0.f) xn = fmaf(k_p, d_prev, xn);
}

// fp32 NCHW operands.  d is read (when k_p != 0) and then written by the same thread at the same index, so it carries no __restrict__.
// NOISE is the stochastic member of the family (DPM-Solver++(2M) SDE): a fourth term, x_next = ... + k_n noise, one more fused
// multiply-add on what cfg_lms_elem returns (stated as fmaf in both kernels so that they round alike).  noise is fp32, laid out like x.
template <bool VPRED, bool NOISE>
__global__ __launch_bounds__(256) void cfg_lms_kernel(float* __restrict__ x_next, float* d, const float* __restrict__ x,
                                                      const float* __restrict__ mc, const float* __restrict__ mu,
                                                      const float* __restrict__ noise, float s, float at_coef, float sqrt_1m_at, float k_x,
                                                      float k_d, float k_p, float k_n, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float p0, xn;
    const float dp = k_p != 0.f ? d[i] : 0.f;
    cfg_lms_elem<VPRED>(x[i], mc[i], mu ? mu[i] : 0.f, mu != nullptr, s, at_coef, sqrt_1m_at, k_x, k_d, k_p, dp, p0, xn);
    if constexpr (NOISE) xn = fmaf(k_n, noise[i], xn);
    x_next[i] = xn;
    if (d) d[i] = p0;
  }
}

// The same update for the fused CFG pair (the sdeo_dpmpp_2m_step family), laid out as cfg_ddim_pair_kernel: fp16 NHWC model output
// (conditional images first), x [b][C][HW] fp32 updated in place, the latent of the next forward staged.
template <bool PAIRED, bool VPRED, bool NOISE>
__global__ __launch_bounds__(256) void cfg_lms_pair_kernel(float* __restrict__ x, float* d, const f16* __restrict__ eps, int lde,
                                                           const float* __restrict__ noise, f16* __restrict__ x0, int ld0, int b, int C, int HW,
                                                           float s, float at_coef, float sqrt_1m_at, float k_x, float k_d, float k_p,
                                                           float k_n) {
  const int64_t total = (int64_t)b * HW;
  stage_pair<PAIRED>(x0, ld0, b, C, HW, [=](int64_t i, int64_t, int c, int64_t, int64_t j) {
    float p0, xn;
    const float dp = k_p != 0.f ? d[j] : 0.f;
    cfg_lms_elem<VPRED>(x[j], (float)eps[i * lde + c], PAIRED ? (float)eps[(i + total) * lde + c] : 0.f, PAIRED, s, at_coef, sqrt_1m_at, k_x,
                        k_d, k_p, dp, p0, xn);
    if constexpr (NOISE) xn = fmaf(k_n, noise[j], xn);
    x[j] = xn;
    if (d) d[j] = p0;
    return xn;
  });
}

// what the multistep update refuses, host only (k_n = 0: the deterministic update, which takes no noise)
int cfg_lms_check(const char* who, const float* d, const float* noise, float a_t, float k_x, float k_d, float k_p, float k_n) {
  SDEO_CHECK(std::isfinite(k_n), "%s: non-finite coefficient k_n=%g", who, k_n);
  SDEO_CHECK(noise || k_n == 0.f, "%s: k_n=%g needs the step noise, but noise is null", who, k_n);
  SDEO_CHECK(a_t > 0.f, "%s: invalid schedule a_t=%g", who, a_t);
  SDEO_CHECK(std::isfinite(k_x) && std::isfinite(k_d) && std::isfinite(k_p), "%s: non-finite coefficient k_x=%g k_d=%g k_p=%g", who, k_x, k_d,
             k_p);
  SDEO_CHECK(d || k_p == 0.f, "%s: k_p=%g needs the previous data prediction, but d is null", who, k_p);
  return 0;
}

// k_n == 0: the deterministic kernel, whatever the noise pointer
int cfg_lms_pair(float* x, float* d, const f16* eps, int lde, const float* noise, float k_n, f16* x0, int ld0, int b, int C, int HW,
                 float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, bool v_prediction, bool paired,
                 hipStream_t stream) {
  SDEO_CHECK(x && eps && x0 && b > 0 && C > 0 && HW > 0 && lde >= C && ld0 >= C, "cfg_lms_pair: bad operand");
  if (int rc = cfg_lms_check("cfg_lms_pair", d, noise, a_t, k_x, k_d, k_p, k_n)) return rc;
  with_flags(paired, v_prediction, k_n != 0.f, [&](auto p, auto v, auto n) {
    hipLaunchKernelGGL((cfg_lms_pair_kernel<p.value, v.value, n.value>), grid_for((int64_t)b * HW), dim3(256), 0, stream, x, d, eps, lde, noise,
                       x0, ld0, b, C, HW, cfg_scale, v.value ? sqrtf(a_t) : 1.0f / sqrtf(a_t), sqrt_one_minus_at, k_x, k_d, k_p, k_n);
  });
  SDEO_HIP(hipGetLastError());
  return 0;
}

int cfg_lms_step(const char* who, float* x_next, float* d, const float* x, const float* m_c, const float* m_u, const float* noise,
                 float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, float k_n, int64_t n, bool v_prediction,
                 hipStream_t stream) {
  SDEO_CHECK(x_next && x && m_c && n > 0, "%s: bad operand", who);
  if (int rc = cfg_lms_check(who, d, noise, a_t, k_x, k_d, k_p, k_n)) return rc;
  with_flags(v_prediction, k_n != 0.f, [&](auto v, auto ns) {
    hipLaunchKernelGGL((cfg_lms_kernel<v.value, ns.value>), grid_for(n), dim3(256), 0, stream, x_next, d, x, m_c, m_u, noise, cfg_scale,
                       v.value ? sqrtf(a_t) : 1.0f / sqrtf(a_t), sqrt_one_minus_at, k_x, k_d, k_p, k_n, n);
  });
  SDEO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void f16_to_f32_kernel(float* __restrict__ y, const f16* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = (float)x[i];
}

int f16_to_f32(float* y, const f16* x, int64_t n, hipStream_t stream) {
  SDEO_CHECK(y && x && n > 0, "f16_to_f32: bad operand");
  hipLaunchKernelGGL(f16_to_f32_kernel, grid_for(n), dim3(256), 0, stream, y, x, n);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// one thread per 8 channels of one token
__global__ __launch_bounds__(256) void embed_tokens_kernel(f16* __restrict__ out, const int32_t* __restrict__ ids,
                                                           const f16* __restrict__ tok_emb, const f16* __restrict__ pos_emb, int B,
                                                           int T, int W, int vocab) {
  const int w8 = W / 8;
  const int64_t total = (int64_t)B * T * w8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % w8) * 8;
    const int64_t row = i / w8;
    const int t = (int)(row % T);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const f16x8 a = *reinterpret_cast<const f16x8*>(tok_emb + (size_t)id * W + c);
    const f16x8 b = *reinterpret_cast<const f16x8*>(pos_emb + (size_t)t * W + c);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)((float)a[j] + (float)b[j]);
    *reinterpret_cast<f16x8*>(out + (size_t)row * W + c) = o;
  }
}

int embed_tokens(f16* out, const int32_t* ids, const f16* tok_emb, const f16* pos_emb, int B, int T, int W, int vocab,
                 hipStream_t stream) {
  SDEO_CHECK(out && ids && tok_emb && pos_emb, "embed_tokens: null operand");
  SDEO_CHECK(B > 0 && T > 0 && W > 0 && W % 8 == 0 && vocab > 0, "embed_tokens: bad sizes B=%d T=%d W=%d vocab=%d", B, T, W, vocab);
  hipLaunchKernelGGL(embed_tokens_kernel, grid_for((int64_t)B * T * (W / 8)), dim3(256), 0, stream, out, ids, tok_emb, pos_emb, B, T, W,
                     vocab);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// ---- LayerNorm folded into the following Linear (conv_inl.h, KP::ln_stats): one wave per output row r
//      w_out[r][k] = fp16(w[r][k] * gamma[k]);  s[r] = sum_k w_out[r][k];  b_out[r] = bias[r] + sum_k beta[k] * w[r][k]
__global__ __launch_bounds__(256) void fold_layernorm_kernel(f16* __restrict__ w_out, float* __restrict__ s_out,
                                                             float* __restrict__ b_out, const f16* __restrict__ w,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ bias, int rows, int C) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float ss = 0.f, sb = 0.f;
  for (int k = lane * 8; k < C; k += 64 * 8) {
    const f16x8 wv = *reinterpret_cast<const f16x8*>(w + (size_t)r * C + k);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float wf = (float)wv[j];
      o[j] = (f16)(wf * gamma[k + j]);
      ss += (float)o[j];
      sb += wf * beta[k + j];
    }
    *reinterpret_cast<f16x8*>(w_out + (size_t)r * C + k) = o;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    ss += __shfl_xor(ss, off, 64);
    sb += __shfl_xor(sb, off, 64);
  }
  if (lane == 0) {
    s_out[r] = ss;
    b_out[r] = sb + (bias ? bias[r] : 0.f);
  }
}

int fold_layernorm(f16* w_out, float* s_out, float* b_out, const f16* w, const float* gamma, const float* beta,
                   const float* bias, int rows, int C, hipStream_t stream) {
  SDEO_CHECK(w_out && s_out && b_out && w && gamma && beta && rows > 0 && C > 0 && C % 8 == 0, "fold_layernorm: bad operand");
  hipLaunchKernelGGL(fold_layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, w_out, s_out, b_out, w, gamma, beta, bias,
                     rows, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// ---- ff.net.2 followed by the SpatialTransformer's proj_out (`attention.py:75-76,385`, `:431-450`): two Linear maps with nothing
//      but a residual add between them, so   proj_out(ff2(g) + t) = g (Wp W2)^T + t Wp^T + (Wp b2 + bp)
//      is ONE GEMM over the row-concatenated operand [g | t] against  w_out[n] = [ (Wp W2)[n][0..K2) | Wp[n][0..C) ]  (built once, at
//      weight finalisation, in fp32 from the fp16 matrices the network would otherwise stream; rounded to fp16 once).
//      grid (ceil((K2 + C) / 256), C): thread (k, n); the bias row is blockIdx.x == gridDim.x - 1's extra duty.
__global__ __launch_bounds__(256) void compose_proj_kernel(f16* __restrict__ w_out, float* __restrict__ b_out, const f16* __restrict__ wp,
                                                           const float* __restrict__ bp, const f16* __restrict__ w2,
                                                           const float* __restrict__ b2, int C, int K2) {
  const int n = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const f16* wrow = wp + (size_t)n * C;
  if (k < K2) {
    float acc = 0.f;
    for (int j = 0; j < C; ++j) acc = fmaf((float)wrow[j], (float)w2[(size_t)j * K2 + k], acc);
    w_out[(size_t)n * (K2 + C) + k] = (f16)acc;
  } else if (k < K2 + C) {
    w_out[(size_t)n * (K2 + C) + k] = wrow[k - K2];
  }
  if (blockIdx.x == gridDim.x - 1) {            // bias: one block-wide deterministic sum per output row
    __shared__ float red[256];
    float acc = 0.f;
    for (int j = threadIdx.x; j < C; j += 256) acc = fmaf((float)wrow[j], b2[j], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) b_out[n] = red[0] + bp[n];
  }
}

int compose_proj(f16* w_out, float* b_out, const f16* wp, const float* bp, const f16* w2, const float* b2, int C, int K2,
                 hipStream_t stream) {
  SDEO_CHECK(w_out && b_out && wp && bp && w2 && b2 && C > 0 && K2 > 0, "compose_proj: bad operand");
  hipLaunchKernelGGL(compose_proj_kernel, dim3(cdiv(K2 + C, 256), C), dim3(256), 0, stream, w_out, b_out, wp, bp, w2, b2, C, K2);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// per-row (sum, sum of squares) of [rows][C] fp16 as ONE partial per row: stats[r][ld][2] (fallback producer of the
// LayerNorm statistics when the GEMM that wrote x ran split-K)
__global__ __launch_bounds__(256) void row_stats_kernel(float* __restrict__ stats, int ld, const f16* __restrict__ x, int ldx,
                                                        int rows, int C) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float s = 0.f, q = 0.f;
  for (int k = lane * 8; k < C; k += 64 * 8) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(x + (size_t)r * ldx + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; s += f; q += f * f; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    q += __shfl_xor(q, off, 64);
  }
  if (lane == 0) reinterpret_cast<float2*>(stats)[(size_t)r * ld] = make_float2(s, q);
}

int row_stats(float* stats, int ld, const f16* x, int ldx, int rows, int C, hipStream_t stream) {
  SDEO_CHECK(stats && x && rows > 0 && C > 0 && C % 8 == 0 && ldx % 8 == 0 && ld >= 1, "row_stats: bad operand");
  hipLaunchKernelGGL(row_stats_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, stats, ld, x, ldx, rows, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// ---- fp8 weight pack (BASELINE configs[4]; the reference's precision switch is the TensorRT builder flag,
//      `onnx2trt_static_plugin.py:40-42`).  One wave per output row: scale = the smallest power of two with absmax / scale <= 448,
//      codes = OCP e4m3fn (round to nearest even, gfx950's native fp8; NOT MI300's fnuz), and the fp16 matrix is overwritten with
//      the dequantised values code * scale (exact in fp16), so kernels without an fp8 path compute with the same weights.
__device__ __forceinline__ unsigned e4m3fn_encode(float f) {           // |f| <= 448
  const unsigned sign = (__float_as_uint(f) >> 24) & 0x80u;
  const float a = fabsf(f);
  unsigned code;
  if (a < 0.015625f) {                                                  // below 2^-6: subnormal grid of 2^-9 (8 rounds up to the
    code = (unsigned)rintf(a * 512.0f);                                 // smallest normal, whose code is 8)
  } else {
    unsigned b = __float_as_uint(a);
    b += 0x7FFFFu + ((b >> 20) & 1u);                                   // round the 23-bit mantissa to 3 bits, ties to even
    code = (b >> 20) - ((127u - 7u) << 3);
    if (code > 0x7Eu) code = 0x7Eu;                                     // 448 = S.1111.110
  }
  return sign | code;
}
__device__ __forceinline__ float e4m3fn_decode(unsigned c) {
  const unsigned e = (c >> 3) & 15u, m = c & 7u;
  const float v = e == 0 ? (float)m * 0.001953125f : __uint_as_float(((e + 120u) << 23) | (m << 20));
  return (c & 0x80u) ? -v : v;
}

__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(uint8_t* __restrict__ q, float* __restrict__ scale, f16* w,
                                                                int rows, int cols, int ldw, int ldq) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  f16* wr = w + (size_t)r * ldw;
  float amax = 0.f;
  for (int k = lane * 8; k < cols; k += 64 * 8) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(wr + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)v[j]));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  float sc = 1.0f;
  if (amax > 0.f) {
    int x;
    const float m = frexpf(amax, &x);                                  // amax = m * 2^x, m in [0.5, 1);  448 = 0.875 * 2^9
    const int e = m <= 0.875f ? x - 9 : x - 8;
    sc = ldexpf(1.0f, e < -15 ? -15 : e);       // >= 2^-15: the smallest code (2^-9) times the scale stays on the fp16 grid (2^-24)
  }
  const float inv = 1.0f / sc;                                          // exact: a power of two
  for (int k = lane * 8; k < cols; k += 64 * 8) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(wr + k);
    f16x8 o;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned c = e4m3fn_encode((float)v[j] * inv);
      if (fabsf(e4m3fn_decode(c) * sc) > 65504.0f) c -= 1;            // |w| in fp16's top binade may round past fp16's maximum: next code down
      if (j < 4) lo |= c << (8 * j); else hi |= c << (8 * (j - 4));
      o[j] = (f16)(e4m3fn_decode(c) * sc);
    }
    *reinterpret_cast<uint2*>(q + (size_t)r * ldq + k) = make_uint2(lo, hi);
    *reinterpret_cast<f16x8*>(wr + k) = o;
  }
  if (lane == 0) scale[r] = sc;
}

int quantize_fp8_rows(uint8_t* q, float* scale, f16* w, int rows, int cols, int ldw, int ldq, hipStream_t stream) {
  SDEO_CHECK(q && scale && w && rows > 0 && cols > 0 && cols % 8 == 0 && ldw % 8 == 0 && ldq % 8 == 0, "quantize_fp8_rows: bad operand");
  hipLaunchKernelGGL(quantize_fp8_rows_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, q, scale, w, rows, cols, ldw, ldq);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// block-scaled fp8 pack (kernels.h quantize_mx): thread = 8 elements, four neighbouring lanes = one 32-element block
__global__ __launch_bounds__(256) void quantize_mx_kernel(uint8_t* __restrict__ q, uint8_t* __restrict__ scales, const f16* __restrict__ x,
                                                          int rows, int cols, int ldx, int ldq, int lds) {
  const int vpr = cols / 8;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = id < (int64_t)rows * vpr;
  const int r = live ? (int)(id / vpr) : 0, v = live ? (int)(id - (int64_t)r * vpr) : 0;
  f16x8 val = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (live) val = *reinterpret_cast<const f16x8*>(x + (size_t)r * ldx + v * 8);
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)val[j]));
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));       // cols % 32 == 0: the four lanes of a block are live or dead together
  amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  int e = 0;
  if (amax > 0.f) {
    int ex;
    const float m = frexpf(amax, &ex);                // amax = m * 2^ex, m in [0.5, 1);  448 = 0.875 * 2^9
    e = m <= 0.875f ? ex - 9 : ex - 8;
  }
  const float inv = ldexpf(1.0f, -e);
  unsigned lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned c = e4m3fn_encode((float)val[j] * inv);
    if (j < 4) lo |= c << (8 * j); else hi |= c << (8 * (j - 4));
  }
  if (live) {
    *reinterpret_cast<uint2*>(q + (size_t)r * ldq + v * 8) = make_uint2(lo, hi);
    if ((v & 3) == 0) scales[(size_t)r * lds + (v >> 2)] = (uint8_t)(e + 127);
  }
}

int quantize_mx(uint8_t* q, uint8_t* scales, const f16* x, int rows, int cols, int ldx, int ldq, int lds, hipStream_t stream) {
  SDEO_CHECK(q && scales && x && rows > 0 && cols > 0 && cols % 32 == 0 && ldx % 8 == 0 && ldq % 8 == 0 && lds >= cols / 32,
             "quantize_mx: bad operand (cols %d, ldx %d, ldq %d, lds %d)", cols, ldx, ldq, lds);
  const int64_t n = (int64_t)rows * (cols / 8);
  hipLaunchKernelGGL(quantize_mx_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, q, scales, x, rows, cols, ldx, ldq, lds);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// s[r] = sum_k w[r][k]  (row sums of a LayerNorm-folded matrix after it was re-quantised: KP::ln_s must match the streamed weights)
__global__ __launch_bounds__(256) void row_sums_kernel(float* __restrict__ s_out, const f16* __restrict__ w, int rows, int C) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float ss = 0.f;
  for (int k = lane * 8; k < C; k += 64 * 8) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(w + (size_t)r * C + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (float)v[j];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
  if (lane == 0) s_out[r] = ss;
}

int row_sums_f16(float* s_out, const f16* w, int rows, int C, hipStream_t stream) {
  SDEO_CHECK(s_out && w && rows > 0 && C > 0 && C % 8 == 0, "row_sums_f16: bad operand");
  hipLaunchKernelGGL(row_sums_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, s_out, w, rows, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace sdeo
