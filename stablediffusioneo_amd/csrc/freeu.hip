// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") on the UNet decoder's concat buffer, in place (include/sdeo.h defines it:
// sdeo_freeu_nhwc_f16).  The buffer is an fp16 NHWC view [n * H * W][ld] whose columns [0, c_h) are the backbone h and [c_h, c_h + c_skip)
// the skip that enters the concat.  Two kernels:
//   freeu_mean_kernel   version 2 only: m[i][p] = mean over the c_h channels of pixel p of image i, fp32, one wave per pixel
//   freeu_apply_kernel  one launch, two kinds of workgroup:
//     skip workgroups      own `cv` 8-channel vectors of one image's skip over all H * W pixels: seven fp32 sums per channel (the spectrum
//                          at the at most four frequencies the filter scales), then x + (s - 1) / (HW) * (their inverse transform)
//     backbone workgroups  own a pixel range of one image: version 2 redoes the min / max of that image's m (H * W floats, L2-resident),
//                          then h[:, :c_h / 2] *= (b - 1) * (m - min) / (max - min) + 1 (1 when max == min); version 1: *= b
// Every reduction runs in a fixed order (per-thread strided sums, xor butterflies, a fixed order over the four waves): results are
// reproducible.  Every global access is one 16-byte channel vector.  Sines and cosines come from the device library's double-precision
// sincospi, H + W of them per skip workgroup, kept in LDS as fp32.  b == 1 and s == 1 launch nothing for their half, so that half keeps
// its bits (signed zeros included).
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace sdeo {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCv = 8;                  // channel vectors of a skip workgroup
constexpr int kSums = 7;                   // S0 = sum x, then x against cos / sin of the row angle, of the column angle, of their sum

__device__ __forceinline__ f16x8 ld8(const f16* p) { return *reinterpret_cast<const f16x8*>(p); }
__device__ __forceinline__ void st8(f16* p, f16x8 v) { *reinterpret_cast<f16x8*>(p) = v; }

__global__ __launch_bounds__(kThreads) void freeu_mean_kernel(float* __restrict__ m, const f16* __restrict__ buf, int ld, int rows, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C >> 3;
  const float inv = 1.0f / (float)C;
  for (int r = blockIdx.x * (kThreads / 64) + wave; r < rows; r += gridDim.x * (kThreads / 64)) {      // (wave-uniform trip count)
    const f16* x = buf + (size_t)r * ld;
    float acc = 0.f;
    for (int v = lane; v < nvec; v += 64) {
      const f16x8 q = ld8(x + v * 8);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)q[j];
      acc += s;
    }
    acc = wave_sum(acc);
    if (lane == 0) m[r] = acc * inv;
  }
}

struct FreeuArgs {
  f16* buf;
  const float* m;            // version 2: the mean map [n][H * W]
  int ld, n, H, W, c_h, c_skip;
  float b, s;
  int version;
  int skip_blocks, cv, slices;        // skip workgroups: slices per image, cv channel vectors each
  int bb_per_image, bb_pixels;        // backbone workgroups per image and the pixels of each
};

__global__ __launch_bounds__(kThreads) void freeu_apply_kernel(FreeuArgs a) {
  __shared__ float tab[4][kFreeuMaxDim];                       // cos / sin of 2 pi u / H, cos / sin of 2 pi v / W
  __shared__ float red[kThreads / 64][kMaxCv][kSums * 8];
  __shared__ float mm[2][kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = a.H * a.W;
  if ((int)blockIdx.x < a.skip_blocks) {
    // ---- skip: the Fourier filter of one channel slice of one image
    const int img = blockIdx.x / a.slices, slice = blockIdx.x - img * a.slices;
    for (int i = tid; i < a.H; i += kThreads) {
      double sn, cs;
      sincospi(2.0 * i / a.H, &sn, &cs);
      tab[0][i] = (float)cs; tab[1][i] = (float)sn;
    }
    for (int i = tid; i < a.W; i += kThreads) {
      double sn, cs;
      sincospi(2.0 * i / a.W, &sn, &cs);
      tab[2][i] = (float)cs; tab[3][i] = (float)sn;
    }
    __syncthreads();
    const int cv = a.cv, ci = tid % cv, pl = tid / cv, npl = kThreads / cv;
    const int vi = slice * cv + ci;
    const bool active = vi < (a.c_skip >> 3);
    f16* x = a.buf + (size_t)img * HW * a.ld + a.c_h + vi * 8;
    float acc[kSums][8];
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    if (active) {
#pragma unroll 2
      for (int p = pl; p < HW; p += npl) {
        const int u = p / a.W, v = p - u * a.W;
        const float cu = tab[0][u], su = tab[1][u], cw = tab[2][v], sw = tab[3][v];
        const float cc = cu * cw - su * sw, ss = su * cw + cu * sw;
        const f16x8 q = ld8(x + (size_t)p * a.ld);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xf = (float)q[j];
          acc[0][j] += xf;
          acc[1][j] += xf * cu; acc[2][j] += xf * su;
          acc[3][j] += xf * cw; acc[4][j] += xf * sw;
          acc[5][j] += xf * cc; acc[6][j] += xf * ss;
        }
      }
    }
    // lanes of a wave that share ci: xor butterfly over the distances 32 .. cv (cv divides 64), then the four waves in order
    // (the distance outside, the 56 values inside: their exchanges are independent and overlap)
    for (int off = 32; off >= cv; off >>= 1) {
#pragma unroll
      for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] += __shfl_xor(acc[k][j], off);
    }
    if (lane < cv) {
#pragma unroll
      for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) red[wave][ci][k * 8 + j] = acc[k][j];
    }
    __syncthreads();
    const float kf = (a.s - 1.0f) / (float)HW;
    const float ka = a.H > 1 ? kf : 0.f, kb = a.W > 1 ? kf : 0.f, kab = (a.H > 1 && a.W > 1) ? kf : 0.f;      // K(1) = {0}
    const float scale[kSums] = {kf, ka, ka, kb, kb, kab, kab};
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = 0.f;
#pragma unroll
        for (int wv = 0; wv < kThreads / 64; ++wv) v += red[wv][ci][k * 8 + j];
        acc[k][j] = v * scale[k];
      }
    if (active) {
#pragma unroll 4
      for (int p = pl; p < HW; p += npl) {
        const int u = p / a.W, v = p - u * a.W;
        const float cu = tab[0][u], su = tab[1][u], cw = tab[2][v], sw = tab[3][v];
        const float cc = cu * cw - su * sw, ss = su * cw + cu * sw;
        f16x8 q = ld8(x + (size_t)p * a.ld);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = acc[0][j] + acc[1][j] * cu + acc[2][j] * su + acc[3][j] * cw + acc[4][j] * sw + acc[5][j] * cc + acc[6][j] * ss;
          q[j] = (f16)((float)q[j] + d);
        }
        st8(x + (size_t)p * a.ld, q);
      }
    }
    return;
  }
  // ---- backbone: the first c_h / 2 channels of a pixel range of one image
  const int bi = blockIdx.x - a.skip_blocks;
  const int img = bi / a.bb_per_image, chunk = bi - img * a.bb_per_image;
  const int p0 = chunk * a.bb_pixels, p1 = min(HW, p0 + a.bb_pixels);
  const float* m = a.m + (size_t)img * HW;
  float lo = 0.f, range = 0.f;
  if (a.version == 2) {
    float mn = INFINITY, mx = -INFINITY;
    for (int p = tid; p < HW; p += kThreads) { const float v = m[p]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    for (int off = 32; off >= 1; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off)); }
    if (lane == 0) { mm[0][wave] = mn; mm[1][wave] = mx; }
    __syncthreads();
    mn = mm[0][0]; mx = mm[1][0];
#pragma unroll
    for (int wv = 1; wv < kThreads / 64; ++wv) { mn = fminf(mn, mm[0][wv]); mx = fmaxf(mx, mm[1][wv]); }
    lo = mn; range = mx - mn;
  }
  const int nv = a.c_h >> 4;                // 8-channel vectors of the first half
  f16* h = a.buf + (size_t)img * HW * a.ld;
  const int work = (p1 - p0) * nv;
  for (int idx = tid; idx < work; idx += kThreads) {
    const int dp = idx / nv, v = idx - dp * nv, p = p0 + dp;
    float f = a.b;
    if (a.version == 2) f = range > 0.f ? (a.b - 1.0f) * ((m[p] - lo) / range) + 1.0f : 1.0f;
    f16* x = h + (size_t)p * a.ld + v * 8;
    f16x8 q = ld8(x);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = (f16)((float)q[j] * f);
    st8(x, q);
  }
}

}  // namespace

static int freeu_value_check(const char* who, const char* name, float v) {
  SDEO_CHECK(std::isfinite(v), "%s: %s is not finite", who, name);
  SDEO_CHECK(v >= 0.f, "%s: %s = %g is negative", who, name, v);
  SDEO_CHECK(v <= kFreeuMax, "%s: %s = %g is above the cap of %g", who, name, v, kFreeuMax);
  return 0;
}
static int freeu_version_check(const char* who, int version) {
  SDEO_CHECK(version == 1 || version == 2, "%s: version %d (1: constant backbone factor, 2: the mean-map factor)", who, version);
  return 0;
}

int freeu_params_check(const char* who, float b1, float b2, float s1, float s2, int version) {
  const float v[4] = {b1, b2, s1, s2};
  static const char* const nm[4] = {"b1", "b2", "s1", "s2"};
  for (int i = 0; i < 4; ++i)
    if (int rc = freeu_value_check(who, nm[i], v[i])) return rc;
  return freeu_version_check(who, version);
}

int freeu_check(const char* who, const f16* buf, int ld, int n, int h, int w, int c_h, int c_skip, float b, float s, int version,
                const float* workspace) {
  SDEO_CHECK(buf, "%s: null buffer", who);
  SDEO_CHECK(n >= 1 && h >= 1 && w >= 1 && h <= kFreeuMaxDim && w <= kFreeuMaxDim, "%s: n = %d maps of %d x %d (1..%d each way)", who, n, h, w,
             kFreeuMaxDim);
  SDEO_CHECK((int64_t)n * h * w <= INT32_MAX, "%s: %d maps of %d x %d are more rows than an int holds", who, n, h, w);
  SDEO_CHECK(c_h >= 16 && c_h % 16 == 0, "%s: c_h = %d must be a positive multiple of 16 (its first half is scaled in 8-channel vectors)", who, c_h);
  SDEO_CHECK(c_skip >= 8 && c_skip % 8 == 0, "%s: c_skip = %d must be a positive multiple of 8", who, c_skip);
  SDEO_CHECK(ld % 8 == 0 && ld >= c_h + c_skip, "%s: ld = %d must be a multiple of 8 and at least c_h + c_skip = %d", who, ld, c_h + c_skip);
  SDEO_CHECK(reinterpret_cast<uintptr_t>(buf) % 16 == 0, "%s: the buffer must be 16-byte aligned", who);
  if (int rc = freeu_value_check(who, "b", b)) return rc;
  if (int rc = freeu_value_check(who, "s", s)) return rc;
  if (int rc = freeu_version_check(who, version)) return rc;
  SDEO_CHECK(version == 1 || b == 1.0f || workspace, "%s: version 2 needs a workspace of n * h * w floats (sdeo_freeu_workspace_bytes)", who);
  return 0;
}

size_t freeu_workspace_bytes(int n, int h, int w) { return (size_t)n * h * w * sizeof(float); }

int freeu_nhwc_f16(f16* buf, int ld, int n, int h, int w, int c_h, int c_skip, float b, float s, int version, float* workspace,
                   hipStream_t stream) {
  if (int rc = freeu_check("freeu_nhwc_f16", buf, ld, n, h, w, c_h, c_skip, b, s, version, workspace)) return rc;
  const int HW = h * w;
  const bool backbone = b != 1.0f, skip = s != 1.0f;
  if (!backbone && !skip) return 0;
  if (backbone && version == 2) {
    const int rows = n * HW;
    hipLaunchKernelGGL(freeu_mean_kernel, dim3(std::min(cdiv(rows, kThreads / 64), 4096)), dim3(kThreads), 0, stream, workspace, buf, ld, rows, c_h);
  }
  FreeuArgs a{buf, workspace, ld, n, h, w, c_h, c_skip, b, s, version, 0, 1, 1, 0, 1};
  if (skip) {
    const int nvs = c_skip / 8;
    int cv = kMaxCv;
    while (cv > 1 && n * cdiv(nvs, cv) < 128) cv >>= 1;      // wider slices only while the grid still fills the chip
    a.cv = cv; a.slices = cdiv(nvs, cv); a.skip_blocks = n * a.slices;
  }
  int bb_blocks = 0;
  if (backbone) {
    const int64_t work = (int64_t)HW * (c_h / 16);
    const int g = (int)std::min<int64_t>(64, std::max<int64_t>(1, cdiv64(work, 2048)));
    a.bb_pixels = cdiv(HW, g); a.bb_per_image = cdiv(HW, a.bb_pixels);
    bb_blocks = n * a.bb_per_image;
  }
  hipLaunchKernelGGL(freeu_apply_kernel, dim3(a.skip_blocks + bb_blocks), dim3(kThreads), 0, stream, a);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace sdeo
