// The scribble family on gfx950: `nms(x, t, s)` of the reference's annotator/hed/__init__.py (cv2.GaussianBlur on float32, four
// cv2.dilate line tests, threshold), the cv2.GaussianBlur(uint8, (0, 0), 3.0) + threshold that upstream gradio_fake_scribble2image
// runs on its result, and the threshold of gradio_scribble2image.  OpenCV is not in the reference tree: its arithmetic is restated
// in tests/scribble_oracle.py (parity with OpenCV unpinned) and these kernels are bit-exact to that oracle.
//
//   gauss_f32_kernel        separable fp32 Gaussian of a uint8 plane.  One workgroup per 32 x 64 output tile: the tile plus an r-pixel
//                           halo (BORDER_REFLECT_101, iterated) is staged in LDS as bytes, the row pass writes (32 + 2r) x 64 floats
//                           into LDS, the column pass reads them back (lanes on consecutive columns: no bank conflict).  The weights
//                           travel by value in the kernel arguments.  OpenCV's symmetric summation order, every product and sum
//                           rounded on its own: no FMA contraction anywhere in this file.
//   nms_kernel              y = b where b is the maximum of one of the four 3-tap lines through the pixel (neighbours outside the
//                           image do not take part), else 0; z = y > t ? 255 : 0
//   gauss_u8_thresh_kernel  the same tiling in integers: OpenCV's 8-bit fixed-point Gaussian for sigma 3 (19 taps, 8 fractional bits
//                           per pass), then > 4 -> 255 / 0 and the optional fp32 control tensor
//   scribble_kernel         255 where the darkest channel of an HWC pixel is below 127
// No allocation, no synchronisation, no host-to-device copy: every entry point is hipGraph-capturable.
#include <math.h>

#include <string>

#include "../../include/sdeo.h"
#include "sdeo_internal.h"
#include "kernels.h"

// hipcc contracts a * b + c into an FMA by default, which would break bit-equality with the oracle's separately rounded products and
// sums.  The pragma governs the expressions written in this file (not inlined header functions such as __fmul_rn, whose results the
// compiler still fuses), so the Gaussian passes below use plain * and +.
#pragma clang fp contract(off)

namespace sdeo {

constexpr int kTH = 32, kTW = 64;      // output tile of the two Gaussians: 256 threads, 8 outputs each
constexpr int kMaxR = 32;              // at most 65 taps

struct GaussF32 {
  int r;
  float k[kMaxR + 1];                  // k[0] centre, k[i] the two taps at distance i
};

constexpr int kU8R = 8;                // sigma 3 on uint8: 19 taps, of which the two outermost round to 0

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

// rows [y0 - R, y0 + rows + R) x columns [x0 - R, x0 + cols + R) of src, reflected at the image border, into tile[.][kTW + 2R]:
// row-major, consecutive lanes on consecutive bytes of a row
__device__ __forceinline__ void stage_tile_u8(uint8_t* tile, const uint8_t* __restrict__ src, int H, int W, int y0, int x0, int rows,
                                              int cols, int R) {
  const int tw = kTW + 2 * R, cw = cols + 2 * R, n = (rows + 2 * R) * cw;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ty = i / cw, tx = i - ty * cw;
    tile[ty * tw + tx] = src[(size_t)reflect101(y0 - R + ty, H) * W + reflect101(x0 - R + tx, W)];
  }
}

__global__ __launch_bounds__(256) void gauss_f32_kernel(const uint8_t* __restrict__ x, int H, int W, GaussF32 g, float* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int R = g.r, tw = kTW + 2 * R;
  float* rowp = reinterpret_cast<float*>(smem);                              // [kTH + 2R][kTW]
  uint8_t* tile = smem + (size_t)(kTH + 2 * R) * kTW * sizeof(float);        // [kTH + 2R][kTW + 2R]
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int rows = min(kTH, H - y0), cols = min(kTW, W - x0);
  stage_tile_u8(tile, x, H, W, y0, x0, rows, cols, R);
  __syncthreads();
  for (int i = threadIdx.x; i < (rows + 2 * R) * kTW; i += 256) {
    const int ty = i / kTW, tx = i % kTW;
    if (tx >= cols) continue;
    const uint8_t* p = tile + ty * tw + tx + R;
    float acc = g.k[0] * (float)p[0];
    for (int j = 1; j <= R; ++j) acc = acc + g.k[j] * ((float)p[-j] + (float)p[j]);
    rowp[ty * kTW + tx] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows * kTW; i += 256) {
    const int ty = i / kTW, tx = i % kTW;
    if (tx >= cols) continue;
    const float* p = rowp + (ty + R) * kTW + tx;
    float acc = g.k[0] * p[0];
    for (int j = 1; j <= R; ++j) acc = acc + g.k[j] * (p[-j * kTW] + p[j * kTW]);
    out[(size_t)(y0 + ty) * W + x0 + tx] = acc;
  }
}

__global__ __launch_bounds__(256) void nms_kernel(const float* __restrict__ b, int H, int W, float t, uint8_t* __restrict__ z) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= W || y >= H) return;
  const size_t o = (size_t)y * W + x;
  const float c = b[o];
  // cv2.dilate(b, line) == b at this pixel: neither neighbour along the line exceeds it; a neighbour outside the image never does
  auto ge = [&](int dy, int dx) {
    const int yy = y + dy, xx = x + dx;
    return yy < 0 || yy >= H || xx < 0 || xx >= W || c >= b[(size_t)yy * W + xx];
  };
  const bool keep = (ge(0, -1) && ge(0, 1)) || (ge(-1, 0) && ge(1, 0)) || (ge(-1, -1) && ge(1, 1)) || (ge(-1, 1) && ge(1, -1));
  const float v = keep ? c : 0.0f;
  z[o] = v > t ? 255 : 0;
}

__global__ __launch_bounds__(256) void gauss_u8_thresh_kernel(const uint8_t* __restrict__ z, int H, int W, uint8_t* __restrict__ map,
                                                              float* __restrict__ control) {
  constexpr int R = kU8R, tw = kTW + 2 * R;
  // the integer weights from the centre outwards (tests/scribble_oracle.py gauss_weights_u8_sigma3); the taps at distance 9 are 0,
  // so a halo of 8 is all there is to stage
  constexpr int kU8W[R + 1] = {34, 32, 28, 20, 14, 9, 4, 3, 1};
  __shared__ int rowp[(kTH + 2 * R) * kTW];
  __shared__ uint8_t tile[(kTH + 2 * R) * tw];
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int rows = min(kTH, H - y0), cols = min(kTW, W - x0);
  stage_tile_u8(tile, z, H, W, y0, x0, rows, cols, R);
  __syncthreads();
  for (int i = threadIdx.x; i < (rows + 2 * R) * kTW; i += 256) {
    const int ty = i / kTW, tx = i % kTW;
    if (tx >= cols) continue;
    const uint8_t* p = tile + ty * tw + tx + R;
    int acc = kU8W[0] * p[0];
#pragma unroll
    for (int j = 1; j <= R; ++j) acc += kU8W[j] * ((int)p[-j] + (int)p[j]);      // <= 255 * 256
    rowp[ty * kTW + tx] = acc;
  }
  __syncthreads();
  const size_t n = (size_t)H * W;
  for (int i = threadIdx.x; i < rows * kTW; i += 256) {
    const int ty = i / kTW, tx = i % kTW;
    if (tx >= cols) continue;
    const int* p = rowp + (ty + R) * kTW + tx;
    int acc = kU8W[0] * p[0];
#pragma unroll
    for (int j = 1; j <= R; ++j) acc += kU8W[j] * (p[-j * kTW] + p[j * kTW]);    // <= 255 * 65536
    const bool e = ((acc + 32768) >> 16) > 4;
    const size_t o = (size_t)(y0 + ty) * W + x0 + tx;
    if (map) map[o] = e ? 255 : 0;
    if (control) {
      const float v = e ? 1.0f : 0.0f;             // 255 / 255
      control[o] = v; control[n + o] = v; control[2 * n + o] = v;
    }
  }
}

__global__ __launch_bounds__(256) void scribble_kernel(const uint8_t* __restrict__ img, int64_t n, int C, uint8_t* __restrict__ map,
                                                       float* __restrict__ control) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int m = 255;
    for (int k = 0; k < C; ++k) m = min(m, (int)img[i * C + k]);
    const bool e = m < 127;
    if (map) map[i] = e ? 255 : 0;
    if (control) {
      const float v = e ? 1.0f : 0.0f;
      control[i] = v; control[n + i] = v; control[2 * n + i] = v;
    }
  }
}

// cv2.getGaussianKernel(n, sigma, CV_32F) with n = round(sigma * 8 + 1) | 1: float64 weights, summed left to right, cast to float
static int make_gauss_f32(GaussF32& g, float sigma, const char* who) {
  SDEO_CHECK(sigma > 0.0f, "%s: sigma %g must be positive", who, (double)sigma);
  const double s = sigma, taps = nearbyint(s * 8 + 1);          // round half to even, as Python's round()
  SDEO_CHECK(taps <= 2 * kMaxR + 1, "%s: sigma %g needs a Gaussian kernel of more than %d taps", who, s, 2 * kMaxR + 1);
  const int n = (int)taps | 1, r = n / 2;
  double t[2 * kMaxR + 1], sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const int d = i - r;
    t[i] = exp(-(double)(d * d) / (2.0 * s * s));
    sum += t[i];
  }
  g.r = r;
  for (int j = 0; j <= kMaxR; ++j) g.k[j] = j <= r ? (float)(t[r + j] / sum) : 0.0f;
  return 0;
}

static int check_plane(const void* in, int H, int W, const char* who) {
  SDEO_CHECK(in, "%s: null image", who);
  SDEO_CHECK(H >= 1 && W >= 1, "%s: bad image %dx%d (h and w must be at least 1)", who, H, W);
  SDEO_CHECK((int64_t)H * W < (1ll << 31) && cdiv(H, 8) <= 65535, "%s: image %dx%d is too large", who, H, W);
  return 0;
}

static int check_workspace(const void* ws, size_t have, size_t need, const char* who) {
  SDEO_CHECK(ws && have >= need, "%s: workspace too small (%zu < %zu)", who, ws ? have : (size_t)0, need);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "%s: workspace must be 4-byte aligned", who);
  return 0;
}

static inline dim3 tile_grid(int H, int W) { return dim3(cdiv(W, kTW), cdiv(H, kTH)); }

static void launch_nms(const uint8_t* x, int H, int W, float t, const GaussF32& g, uint8_t* z, float* b, hipStream_t stream,
                       hipEvent_t* ev) {
  const size_t lds = (size_t)(kTH + 2 * g.r) * kTW * sizeof(float) + (size_t)(kTH + 2 * g.r) * (kTW + 2 * g.r);
  hipLaunchKernelGGL(gauss_f32_kernel, tile_grid(H, W), dim3(256), lds, stream, x, H, W, g, b);
  if (ev) (void)hipEventRecord(ev[1], stream);
  if (z) hipLaunchKernelGGL(nms_kernel, dim3(cdiv(W, 32), cdiv(H, 8)), dim3(256), 0, stream, b, H, W, t, z);
  if (ev) (void)hipEventRecord(ev[2], stream);
}

static size_t hed_nms_workspace_bytes(int H, int W) { return H >= 1 && W >= 1 ? (size_t)H * W * sizeof(float) : 0; }

static int hed_nms_u8(const uint8_t* x, int H, int W, float t, float sigma, uint8_t* z, float* blurred, void* workspace, size_t workspace_bytes,
               hipStream_t stream) {
  const char* who = "sdeo_nms_u8";
  if (int rc = check_plane(x, H, W, who)) return rc;
  GaussF32 g;
  if (int rc = make_gauss_f32(g, sigma, who)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, hed_nms_workspace_bytes(H, W), who)) return rc;
  launch_nms(x, H, W, t, g, z, blurred ? blurred : static_cast<float*>(workspace), stream, nullptr);
  SDEO_HIP(hipGetLastError());
  return 0;
}

static size_t fake_scribble_workspace_bytes(int H, int W) { return H >= 1 && W >= 1 ? (size_t)H * W * (sizeof(float) + 1) : 0; }

// ev (optional): four events recorded around the three launches (sdeo_debug_fake_scribble_profile)
static int fake_scribble_u8(const uint8_t* edges, int H, int W, uint8_t* scribble, float* control, void* workspace, size_t workspace_bytes,
                     hipStream_t stream, hipEvent_t* ev = nullptr) {
  const char* who = "sdeo_fake_scribble_u8";
  if (int rc = check_plane(edges, H, W, who)) return rc;
  GaussF32 g;
  if (int rc = make_gauss_f32(g, 3.0f, who)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, fake_scribble_workspace_bytes(H, W), who)) return rc;
  float* b = static_cast<float*>(workspace);                    // the fp32 plane first: 4-byte aligned
  uint8_t* z = reinterpret_cast<uint8_t*>(b + (size_t)H * W);
  if (ev) (void)hipEventRecord(ev[0], stream);
  launch_nms(edges, H, W, 127.0f, g, z, b, stream, ev);
  hipLaunchKernelGGL(gauss_u8_thresh_kernel, tile_grid(H, W), dim3(256), 0, stream, z, H, W, scribble, control);
  if (ev) (void)hipEventRecord(ev[3], stream);
  SDEO_HIP(hipGetLastError());
  return 0;
}

static int scribble_u8(const uint8_t* img, int H, int W, int C, uint8_t* map, float* control, hipStream_t stream) {
  const char* who = "sdeo_scribble_u8";
  if (int rc = check_plane(img, H, W, who)) return rc;
  SDEO_CHECK(C >= 1 && C <= 4, "%s: %d channels (1..4 expected)", who, C);
  const int64_t n = (int64_t)H * W;
  const int64_t blocks = cdiv64(n, 256);
  hipLaunchKernelGGL(scribble_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, stream, img, n, C, map, control);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace sdeo

using namespace sdeo;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

size_t sdeo_nms_workspace_bytes(int h, int w) { return hed_nms_workspace_bytes(h, w); }

int sdeo_nms_u8(const uint8_t* x, int h, int w, float t, float sigma, uint8_t* z, float* blurred, void* workspace,
                    size_t workspace_bytes, void* stream) {
  return hed_nms_u8(x, h, w, t, sigma, z, blurred, workspace, workspace_bytes, S(stream));
}

size_t sdeo_fake_scribble_workspace_bytes(int h, int w) { return fake_scribble_workspace_bytes(h, w); }

int sdeo_fake_scribble_u8(const uint8_t* edges, int h, int w, uint8_t* scribble, float* control_chw, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return fake_scribble_u8(edges, h, w, scribble, control_chw, workspace, workspace_bytes, S(stream));
}

int sdeo_scribble_u8(const uint8_t* img_hwc, int h, int w, int c, uint8_t* map, float* control_chw, void* stream) {
  return scribble_u8(img_hwc, h, w, c, map, control_chw, S(stream));
}

// one sdeo_fake_scribble_u8 call with HIP events between its launches; synchronises and returns the JSON array
// [{"kernel", "launches", "total_ms"}] (tools/scribble_time.py).  Not capturable.  "[]" when the call fails (sdeo_last_error).
const char* sdeo_debug_fake_scribble_profile(const uint8_t* edges, int h, int w, uint8_t* scribble, float* control_chw, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  static thread_local std::string report;
  static const char* names[3] = {"gauss_f32_kernel", "nms_kernel", "gauss_u8_thresh_kernel"};
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  for (auto& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  ok = ok && fake_scribble_u8(edges, h, w, scribble, control_chw, workspace, workspace_bytes, S(stream), ev) == 0;
  ok = ok && hipStreamSynchronize(S(stream)) == hipSuccess;
  report = "[";
  for (int i = 0; ok && i < 3; ++i) {
    float ms = 0.f;
    ok = hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess;
    char buf[160];
    snprintf(buf, sizeof(buf), "%s{\"kernel\": \"%s\", \"launches\": 1, \"total_ms\": %.6f}", i ? ", " : "", names[i], ms);
    report += buf;
  }
  report += "]";
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return ok ? report.c_str() : "[]";
}

}  // extern "C"
