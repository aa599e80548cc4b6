// The two ends of the VAE encode path (gfx950): the image intake in front of encoder.conv_in and the Gaussian-posterior tail
// behind quant_conv.  Both are memory-bound, one thread per pixel, fp32 math.
#include "kernels.h"

namespace sdeo {

static inline dim3 grid_for_px(int64_t work_items) {
  int64_t b = cdiv64(work_items, 256);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// images -> fp16 NHWC with 8 stored channels (one 16-byte store per pixel).  fp32 input: NCHW, rounded once to fp16.  uint8 input:
// HWC, upstream load_img's 2 * (u / 255) - 1 evaluated in fp32 (IEEE division; 2 q is exact, so the subtraction rounds once), then
// rounded once to fp16 -- the same fp16 value the fp32 path produces from that fp32 pixel.
__global__ __launch_bounds__(256) void image_intake_kernel(f16* __restrict__ y, const float* __restrict__ x,
                                                           const uint8_t* __restrict__ xu, int B, int C, int HW) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW;
    const int64_t p = i - b * HW;
    f16x8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float v = 0.f;
      if (c < C) {
        if (x) {
          v = x[(b * C + c) * HW + p];
        } else {
          const float q = (float)xu[i * C + c] / 255.0f;
          v = 2.0f * q - 1.0f;
        }
      }
      o[c] = (f16)v;
    }
    *reinterpret_cast<f16x8*>(y + i * 8) = o;
  }
}

int image_to_nhwc8_f16(f16* y, const float* x, const uint8_t* x_u8, int B, int C, int HW, hipStream_t stream) {
  SDEO_CHECK(y && (x || x_u8) && B > 0 && HW > 0 && C >= 1 && C <= 8, "image_to_nhwc8_f16: bad operand (C=%d, at most 8)", C);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(y) & 15) == 0, "image_to_nhwc8_f16: output must be 16-byte aligned");
  hipLaunchKernelGGL(image_intake_kernel, grid_for_px((int64_t)B * HW), dim3(256), 0, stream, y, x, x ? nullptr : x_u8, B, C, HW);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// DiagonalGaussianDistribution (distributions.py:24-35): mean, logvar = chunk(moments, 2); logvar = clamp(logvar, -30, 20);
// std = exp(0.5 logvar); sample = mean + std * noise; get_first_stage_encoding: z = scale_factor * sample (mode(): noise = 0)
__global__ __launch_bounds__(256) void vae_posterior_kernel(float* __restrict__ z, float* __restrict__ moments, const f16* __restrict__ m,
                                                            int ldm, const float* __restrict__ noise, int zc, int HW, float scale) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const f16* row = m + (int64_t)p * ldm;
    for (int c = 0; c < zc; ++c) {
      const float mean = (float)row[c];
      const float lv_raw = (float)row[zc + c];
      if (moments) {
        moments[(int64_t)c * HW + p] = mean;
        moments[(int64_t)(zc + c) * HW + p] = lv_raw;
      }
      float s = mean;
      if (noise) {
        const float lv = fminf(fmaxf(lv_raw, -30.0f), 20.0f);
        s = mean + expf(0.5f * lv) * noise[(int64_t)c * HW + p];
      }
      z[(int64_t)c * HW + p] = scale * s;
    }
  }
}

int vae_posterior(float* z, float* moments, const f16* m, int ldm, const float* noise, int zc, int HW, float scale, hipStream_t stream) {
  SDEO_CHECK(z && m && zc >= 1 && ldm >= 2 * zc && HW > 0, "vae_posterior: bad operand (zc=%d ldm=%d)", zc, ldm);
  hipLaunchKernelGGL(vae_posterior_kernel, grid_for_px(HW), dim3(256), 0, stream, z, moments, m, ldm, noise, zc, HW, scale);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace sdeo
