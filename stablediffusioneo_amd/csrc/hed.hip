// HED soft-edge annotator (`annotator/hed/__init__.py`: ControlNetHED_Apache2 + HEDdetector.__call__) on gfx950:
//   h = x - norm;  block k: [2x2 / stride-2 max-pool for k >= 2] -> n_k x (conv3x3 + ReLU) -> projection conv1x1 C_k -> 1
//   edge = uint8(clip(255 sigmoid(mean_k resize_bilinear(projection_k, H x W)), 0, 255))      (truncated, like .astype(np.uint8))
// The thirteen 3x3 convs run on the implicit-GEMM / halo kernels of conv_gemm.hip with the ReLU epilogue (ConvGemm::act = 4).  The
// kernels of this file are the memory-bound pieces around them, one thread (or eight lanes) per pixel:
//   hed_intake_kernel    uint8 RGB HWC -> fp16 NHWC, 8 stored channels, v = (float)u - norm[c] rounded once (the first conv's zero
//                        padding pads x - norm, so the subtraction happens here)
//   maxpool2x2_kernel    F.max_pool2d(kernel 2, stride 2) on NHWC fp16, floor semantics (an odd last row / column is dropped); exact
//   side_proj_kernel     the 1x1 projection C -> 1 + bias into an fp32 map (eight lanes per pixel, 16-byte loads, one read of the
//                        block output)
//   hed_fuse_kernel      cv2.resize INTER_LINEAR on float32 (= F.interpolate bilinear, align_corners=False) of the five maps at each
//                        output pixel, fp32 mean in numpy's order, fp64 sigmoid, truncation to uint8 (+ optional control tensor)
#include "../../include/sdeo.h"
#include "program_handle.h"
#include "sdeo_internal.h"

using namespace sdeo;

namespace sdeo {

static inline dim3 grid_px(int64_t work_items) {
  int64_t b = cdiv64(work_items, 256);
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

__global__ __launch_bounds__(256) void hed_intake_kernel(f16* __restrict__ y, const uint8_t* __restrict__ img,
                                                         const float* __restrict__ norm, int64_t HW) {
  const float n0 = norm[0], n1 = norm[1], n2 = norm[2];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
    const uint8_t* px = img + i * 3;
    f16x8 o = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    o[0] = (f16)((float)px[0] - n0);
    o[1] = (f16)((float)px[1] - n1);
    o[2] = (f16)((float)px[2] - n2);
    *reinterpret_cast<f16x8*>(y + i * 8) = o;
  }
}

int hed_intake(f16* y, const uint8_t* img, const float* norm, int H, int W, hipStream_t stream) {
  SDEO_CHECK(y && img && norm && H > 0 && W > 0, "hed_intake: bad operand");
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(hed_intake_kernel, grid_px(HW), dim3(256), 0, stream, y, img, norm, HW);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// one thread per (output pixel, 8-channel group); the four source pixels exist for every output pixel (floor semantics)
__global__ __launch_bounds__(256) void maxpool2x2_kernel(f16* __restrict__ y, const f16* __restrict__ x, int Hi, int Wi, int C) {
  const int Ho = Hi / 2, Wo = Wi / 2, G = C / 8;
  const int64_t total = (int64_t)Ho * Wo * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t p = i / G;
    const int wo = (int)(p % Wo), ho = (int)(p / Wo);
    const f16* s = x + ((int64_t)(2 * ho) * Wi + 2 * wo) * C + g * 8;
    const f16x8 a = *reinterpret_cast<const f16x8*>(s), b = *reinterpret_cast<const f16x8*>(s + C);
    const f16x8 c = *reinterpret_cast<const f16x8*>(s + (int64_t)Wi * C), d = *reinterpret_cast<const f16x8*>(s + (int64_t)Wi * C + C);
    f16x8 o;
#pragma unroll
    for (int t = 0; t < 8; ++t) o[t] = (f16)fmaxf(fmaxf((float)a[t], (float)b[t]), fmaxf((float)c[t], (float)d[t]));
    *reinterpret_cast<f16x8*>(y + p * C + g * 8) = o;
  }
}

int maxpool2x2_nhwc(f16* y, const f16* x, int Hi, int Wi, int C, hipStream_t stream) {
  SDEO_CHECK(y && x && Hi >= 2 && Wi >= 2 && C > 0 && C % 8 == 0, "maxpool2x2: bad operand (%dx%d, C=%d: C %% 8 == 0)", Hi, Wi, C);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "maxpool2x2: operands must be 16-byte aligned");
  hipLaunchKernelGGL(maxpool2x2_kernel, grid_px((int64_t)(Hi / 2) * (Wi / 2) * (C / 8)), dim3(256), 0, stream, y, x, Hi, Wi, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// out[p] = bias + sum_c x[p][c] w[c]: eight lanes per pixel, lane j reads channels [8 j + 64 t, 8 j + 64 t + 8) (16 bytes; the eight
// lanes of a pixel read 128 contiguous bytes per step), fp32 products, then a fixed three-step butterfly over the eight lanes
__global__ __launch_bounds__(256) void side_proj_kernel(float* __restrict__ out, const f16* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int64_t HW, int C) {
  const int j = threadIdx.x & 7;
  const float b = bias[0];
  const int64_t stride = (int64_t)gridDim.x * 32;
  for (int64_t p0 = (int64_t)blockIdx.x * 32; p0 < HW; p0 += stride) {
    const int64_t p = p0 + (threadIdx.x >> 3);
    float s = 0.f;
    if (p < HW) {
      const f16* row = x + p * C;
      for (int c = j * 8; c < C; c += 64) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(row + c);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + c), w1 = *reinterpret_cast<const f32x4*>(w + c + 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) s = fmaf((float)v[t], w0[t], s);
#pragma unroll
        for (int t = 0; t < 4; ++t) s = fmaf((float)v[4 + t], w1[t], s);
      }
    }
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    if (p < HW && j == 0) out[p] = s + b;
  }
}

int side_proj(float* out, const f16* x, const float* w, const float* bias, int H, int W, int C, hipStream_t stream) {
  SDEO_CHECK(out && x && w && bias && H > 0 && W > 0 && C > 0 && C % 64 == 0, "side_proj: bad operand (C=%d: C %% 64 == 0)", C);
  const int64_t HW = (int64_t)H * W;
  int64_t blocks = cdiv64(HW, 32);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(side_proj_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, out, x, w, bias, HW, C);
  SDEO_HIP(hipGetLastError());
  return 0;
}

struct HedMaps {
  const float* m[5];
  int h[5], w[5];
};

// F.interpolate(bilinear, align_corners=False) index and weights along one axis (upsample_bilinear2d's CPU arithmetic in fp32):
// src = max(scale (d + 0.5) - 0.5, 0), i0 = min(floor(src), n - 1), l1 = clamp(src - i0, 0, 1), i1 = i0 + (i0 < n - 1)
__device__ __forceinline__ void lin_axis(int d, int n, float scale, int& i0, int& i1, float& l0, float& l1) {
  float src = __fsub_rn(__fmul_rn(scale, (float)d + 0.5f), 0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = (int)floorf(src);
  i0 = i0 < n - 1 ? i0 : n - 1;
  l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  l0 = __fsub_rn(1.f, l1);
}

__global__ __launch_bounds__(256) void hed_fuse_kernel(uint8_t* __restrict__ edges, float* __restrict__ control, const HedMaps maps, int H,
                                                       int W) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int h = maps.h[k], w = maps.w[k];
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      lin_axis(y, h, (float)h / (float)H, y0, y1, ly0, ly1);
      lin_axis(x, w, (float)w / (float)W, x0, x1, lx0, lx1);
      const float* m = maps.m[k];
      const float t0 = __fadd_rn(__fmul_rn(m[y0 * w + x0], lx0), __fmul_rn(m[y0 * w + x1], lx1));
      const float t1 = __fadd_rn(__fmul_rn(m[y1 * w + x0], lx0), __fmul_rn(m[y1 * w + x1], lx1));
      const float v = __fadd_rn(__fmul_rn(t0, ly0), __fmul_rn(t1, ly1));
      s = k ? __fadd_rn(s, v) : v;                 // ((((a + b) + c) + d) + e): numpy's order for five float32 elements
    }
    const float mean = s / 5.0f;                   // IEEE division (np.mean divides the float32 sum by the count)
    const double e = 1.0 / (1.0 + exp(-(double)mean));
    double v = e * 255.0;
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    const uint8_t u = (uint8_t)(int)v;             // truncation, as .astype(np.uint8)
    if (edges) edges[i] = u;
    if (control) {
      const float c = (float)u / 255.0f;           // HWC3(edge) / 255 in fp32
      control[i] = c;
      control[HW + i] = c;
      control[2 * HW + i] = c;
    }
  }
}

int hed_fuse(uint8_t* edges, float* control, const HedMaps& maps, int H, int W, hipStream_t stream) {
  SDEO_CHECK(H > 0 && W > 0, "hed_fuse: bad size");
  for (int k = 0; k < 5; ++k) SDEO_CHECK(maps.m[k] && maps.h[k] >= 1 && maps.w[k] >= 1, "hed_fuse: map %d missing", k);
  if (!edges && !control) return 0;
  hipLaunchKernelGGL(hed_fuse_kernel, grid_px((int64_t)H * W), dim3(256), 0, stream, edges, control, maps, H, W);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace sdeo

// ------------------------------------------------------------------------------------------------ handle
namespace {

const int kBlockConvs[5] = {2, 2, 3, 3, 3};
const int kBlockCh[5] = {64, 128, 256, 512, 512};

}  // namespace

struct sdeo_hed_handle_s : ProgramHandle {
  // configured state
  int H = 0, W = 0;
  const uint8_t* img = nullptr;      // the image of the current sdeo_hed_detect_u8 call (read by the intake op)
  uint8_t* edges = nullptr;
  float* control = nullptr;
  HedMaps maps{};
  Profiler prof;                     // sdeo_debug_hed_profile

  void free_configured() {
    maps = HedMaps{};
    H = W = 0;
    ProgramHandle::free_configured();
  }
};

namespace {

typedef sdeo_hed_handle_s Hed;

// reference state-dict order: norm, then per block convs.{i}.weight / bias and projection.weight / bias
static void build_registry(Hed* e) {
  WeightStore& r = e->ws;
  r.add("norm", W_VEC, {1, 3, 1, 1}, r.take(3 * 4));
  int cin = 3;
  for (int b = 0; b < 5; ++b) {
    const std::string p = "block" + std::to_string(b + 1) + ".";
    const int c = kBlockCh[b];
    for (int i = 0; i < kBlockConvs[b]; ++i) {
      const int cp = (cin + 7) / 8 * 8;
      r.add(p + "convs." + std::to_string(i) + ".weight", W_CONV, {c, cin, 3, 3}, r.take((size_t)c * 9 * cp * 2), cp);
      r.add(p + "convs." + std::to_string(i) + ".bias", W_VEC, {c}, r.take((size_t)c * 4));
      cin = c;
    }
    r.add(p + "projection.weight", W_VEC, {1, c, 1, 1}, r.take((size_t)c * 4));
    r.add(p + "projection.bias", W_VEC, {1}, r.take(4));
  }
}

// the body of sdeo_hed_configure after its checks
static int configure_impl(Hed* e, int H, int W) {
  int hk[5], wk[5];
  hk[0] = H; wk[0] = W;
  for (int k = 1; k < 5; ++k) { hk[k] = hk[k - 1] / 2; wk[k] = wk[k - 1] / 2; }
  // arena: intake [H W][8] fp16; two ping-pong activation buffers of max_k h_k w_k C_k fp16 (block 1 is the largest); five side maps
  size_t act_elems = 0;
  for (int k = 0; k < 5; ++k) act_elems = std::max(act_elems, (size_t)hk[k] * wk[k] * kBlockCh[k]);
  const size_t o_in = e->take((size_t)H * W * 8 * 2), o_a = e->take(act_elems * 2), o_b = e->take(act_elems * 2);
  size_t o_side[5];
  for (int k = 0; k < 5; ++k) o_side[k] = e->take((size_t)hk[k] * wk[k] * 4);
  if (int rc = e->alloc_act()) return rc;
  f16* xin = e->at<f16>(o_in);
  f16* buf[2] = {e->at<f16>(o_a), e->at<f16>(o_b)};
  for (int k = 0; k < 5; ++k) {
    e->maps.m[k] = e->at<float>(o_side[k]);
    e->maps.h[k] = hk[k];
    e->maps.w[k] = wk[k];
  }

  const float* norm = e->ws.ptr<float>("norm");
  e->prog.push_back(Op([e, xin, norm, H, W](hipStream_t s) { return hed_intake(xin, e->img, norm, H, W, s); }, "hed_intake"));
  const f16* cur = xin;
  int cur_buf = -1, cin = 8;
  for (int b = 0; b < 5; ++b) {
    const std::string p = "block" + std::to_string(b + 1) + ".";
    const int c = kBlockCh[b], h = hk[b], w = wk[b];
    if (b > 0) {
      f16* dst = buf[cur_buf ^ 1];
      const f16* src = cur;
      const int hi = hk[b - 1], wi = wk[b - 1], cc = cin;
      e->prog.push_back(Op([dst, src, hi, wi, cc](hipStream_t s) { return maxpool2x2_nhwc(dst, src, hi, wi, cc, s); }, "maxpool2x2_kernel"));
      cur = dst;
      cur_buf ^= 1;
    }
    for (int i = 0; i < kBlockConvs[b]; ++i) {
      const std::string n = p + "convs." + std::to_string(i) + ".";
      f16* dst = buf[cur_buf < 0 ? 0 : cur_buf ^ 1];
      ConvGemm q;
      q.x = cur; q.w = e->ws.ptr<f16>(n + "weight"); q.y = dst;
      q.bias = e->ws.ptr<float>(n + "bias");
      q.B = 1; q.Hi = h; q.Wi = w; q.Cin = cin; q.R = q.S = 3; q.stride = 1; q.pad = 1;
      q.Ho = h; q.Wo = w; q.M = h * w; q.N = c; q.K = 9 * cin;
      q.ldx = cin; q.ldw = q.K; q.ldy = c; q.ldres = c; q.ld_bias2 = c;
      q.act = 4;
      e->push(q, /*flop_k=*/9 * (b == 0 && i == 0 ? 3 : cin));
      cur = dst;
      cur_buf = cur_buf < 0 ? 0 : cur_buf ^ 1;
      cin = c;
    }
    {
      float* out = const_cast<float*>(e->maps.m[b]);
      const f16* src = cur;
      const float* pw = e->ws.ptr<float>(p + "projection.weight");
      const float* pb = e->ws.ptr<float>(p + "projection.bias");
      e->prog.push_back(Op([out, src, pw, pb, h, w, c](hipStream_t s) { return side_proj(out, src, pw, pb, h, w, c, s); }, "side_proj_kernel",
                           2.0 * h * w * c));
    }
  }
  e->prog.push_back(Op([e, H, W](hipStream_t s) { return hed_fuse(e->edges, e->control, e->maps, H, W, s); }, "hed_fuse_kernel"));
  if (int rc = e->alloc_splitk()) return rc;
  e->H = H;
  e->W = W;
  return 0;
}

}  // namespace

extern "C" {

int sdeo_hed_create(sdeo_hed_handle* out) {
  SDEO_CHECK(out, "sdeo_hed_create: null argument");
  Hed* e = new Hed();
  build_registry(e);
  return handle_created("sdeo_hed_create", e, out);
}

int sdeo_hed_destroy(sdeo_hed_handle h) { return handle_destroy(h); }

int sdeo_hed_num_weights(sdeo_hed_handle h) { return handle_num_weights(h); }

int sdeo_hed_weight_info(sdeo_hed_handle h, int i, const char** name, int64_t dims[4], int* ndim) {
  return handle_weight_info("sdeo_hed_weight_info", h, i, name, dims, 4, 0, ndim);
}

int sdeo_hed_load_weight(sdeo_hed_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict) {
  SDEO_CHECK(h && name && host_data && dims, "sdeo_hed_load_weight: null argument");
  if (int rc = h->ws.load("sdeo_hed_load_weight", name, name, host_data, dims, ndim, strict)) return rc;
  if (h->ws.find(name)) h->finalized = false;      // a tensor changed: finalize again before the next configure / detect
  return 0;
}

int sdeo_hed_finalize_weights(sdeo_hed_handle h) { return handle_finalize_weights("sdeo_hed_finalize_weights", h); }

int sdeo_hed_configure(sdeo_hed_handle h, int height, int width) {
  SDEO_CHECK(h, "sdeo_hed_configure: null handle");
  SDEO_CHECK(h->finalized, "sdeo_hed_configure: weights not finalized");
  SDEO_CHECK(height >= 16 && width >= 16 && height <= 8192 && width <= 8192, "sdeo_hed_configure: image %dx%d out of range (16..8192)",
             height, width);
  return handle_configure(h, [&] { return configure_impl(h, height, width); });
}

int sdeo_hed_detect_u8(sdeo_hed_handle h, const uint8_t* img_hwc, uint8_t* edges, float* control_chw, float* const* side, void* stream) {
  SDEO_CHECK(h, "sdeo_hed_detect_u8: null handle");
  SDEO_CHECK(h->finalized, "sdeo_hed_detect_u8: weights not finalized");
  SDEO_CHECK(h->H > 0, "sdeo_hed_detect_u8: handle not configured (sdeo_hed_configure)");
  SDEO_CHECK(img_hwc, "sdeo_hed_detect_u8: null image");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  h->img = img_hwc;
  h->edges = edges;
  h->control = control_chw;
  const int rc = run_program(h->prog, s);
  h->img = nullptr; h->edges = nullptr; h->control = nullptr;
  if (rc) return rc;
  if (side)
    for (int k = 0; k < 5; ++k)
      if (side[k])
        SDEO_HIP(hipMemcpyAsync(side[k], h->maps.m[k], (size_t)h->maps.h[k] * h->maps.w[k] * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}

size_t sdeo_hed_device_bytes(sdeo_hed_handle h) { return handle_device_bytes(h); }

// ---- not in sdeo.h: tests and tools

// F.max_pool2d(x, 2, 2) on NHWC fp16 [h][w][c] (one image), c % 8 == 0 -> y [h/2][w/2][c]
int sdeo_debug_maxpool2x2_f16(void* y, const void* x, int h, int w, int c, void* stream) {
  return maxpool2x2_nhwc((f16*)y, (const f16*)x, h, w, c, reinterpret_cast<hipStream_t>(stream));
}

// one detection with HIP events around every launch; synchronises and returns the JSON array
// [{"kernel", "launches", "total_ms", "flops", "bytes"}] aggregated by kernel name (tools/hed_time.py).  Not capturable.
const char* sdeo_debug_hed_profile(sdeo_hed_handle h, const uint8_t* img_hwc, void* stream) {
  if (!h || !h->finalized || h->H <= 0 || !img_hwc) return "[]";
  h->img = img_hwc;
  h->prof.begin();
  const int rc = run_program(h->prog, reinterpret_cast<hipStream_t>(stream), &h->prof);
  h->img = nullptr;
  const char* out = h->prof.end();
  return rc ? "[]" : out;
}

}  // extern "C"
