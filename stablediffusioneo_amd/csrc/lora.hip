// LoRA merge into a stored weight tensor, and the read-back of a stored tensor.
//
//   W[o][j] <- fp16( fp32(W[o][j]) + scale * sum_{r < rank} up[o][r] * down[r][j] )        o < O, j < J = in * kh * kw
//
// up [O][rank] and down [rank][J] are fp32 in the PyTorch layout of lora_up.weight / lora_down.weight; W is the fp16 tensor as
// WeightStore::load stored it, so the epilogue writes (o, j) where load would have put it (handle_common.h, WKind):
//   W_LINEAR   [O][J]
//   W_CONV     [O][kh][kw][ipad]; j = (c * kh + r) * kw + s; the pad channels c in [in, ipad) are neither read nor written
//   W_GEGLU_W  row o of the [2H][J] projection lives at row 32 * (o' / 16) + 16 * is_gate + o' % 16, o' = o mod H
//
// The work is memory-bound (each element of W is read once and written once, rank is small), so the kernel is a plain fp32 FMA on an
// LDS-tiled block, not an MFMA: a 64 x 64 tile of W per 256-thread block, a 4 x 4 micro-tile per thread, rank walked in chunks of 32
// through LDS.  The tile is indexed in DESTINATION order (rows of the stored matrix, its contiguous columns), so the read-modify-write
// of W is coalesced in every layout and the layout only shows in how a column finds its entry of `down` (a strided gather of a matrix
// that is rank x J floats and stays in L2).  Arithmetic: the sum is one fp32 fmaf chain in rank order, the update one fmaf(scale, sum,
// fp32(W)) and one round-to-nearest-even to fp16; operands are never rounded to fp16.  An element whose update scale * sum is zero is
// not written at all, so scale = 0 (and a zero-initialised lora_up) leaves every bit, the sign of a zero included.
#include <cmath>

#include "handle_common.h"

namespace sdeo {

namespace {

constexpr int kTile = 64;        // rows and columns of W per block
constexpr int kRankChunk = 32;   // ranks per LDS pass
constexpr int kUpLd = kTile + 4; // row stride of the transposed `up` tile (keeps the float4 reads aligned, spreads the transposing stores)

struct LoraDst {
  int kind;          // WKind
  int O, J;          // logical rows and columns of the update
  int cols;          // stored columns of a row: J, or kh * kw * ipad
  int in, khw, ipad; // W_CONV
  int H;             // W_GEGLU_W: O / 2
};

// stored row of logical row o
__device__ __forceinline__ int64_t lora_dst_row(const LoraDst& d, int o) {
  if (d.kind != W_GEGLU_W) return o;
  const int gate = o >= d.H, oo = gate ? o - d.H : o;
  return 32 * (int64_t)(oo >> 4) + 16 * gate + (oo & 15);
}
// logical row of stored row `row` (the inverse; the interleave permutes the rows of a [2H][J] matrix, H % 16 == 0)
__device__ __forceinline__ int lora_src_row(const LoraDst& d, int row) {
  if (d.kind != W_GEGLU_W) return row;
  const int blk = row >> 5, gate = (row >> 4) & 1;
  return gate * d.H + blk * 16 + (row & 15);
}
// logical column of stored column c, or -1 for a pad channel
__device__ __forceinline__ int lora_src_col(const LoraDst& d, int c) {
  if (d.kind != W_CONV) return c;
  const int rs = c / d.ipad, ch = c - rs * d.ipad;
  return ch < d.in ? ch * d.khw + rs : -1;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(f16* __restrict__ w, const float* __restrict__ down, const float* __restrict__ up,
                                                         LoraDst d, int rank, float scale) {
  __shared__ __attribute__((aligned(16))) float up_s[kRankChunk][kUpLd];      // [r][row]
  __shared__ __attribute__((aligned(16))) float down_s[kRankChunk][kTile];    // [r][col]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * kTile, col0 = blockIdx.x * kTile;             // stored rows / columns of this tile
  float acc[4][4] = {};
  for (int r0 = 0; r0 < rank; r0 += kRankChunk) {
    // up tile: consecutive threads walk r (contiguous in up[o][:]); rows past O and ranks past `rank` are zero
    for (int e = tid; e < kTile * kRankChunk; e += 256) {
      const int r = e % kRankChunk, row = e / kRankChunk;
      float v = 0.f;
      if (row0 + row < d.O && r0 + r < rank) v = up[(int64_t)lora_src_row(d, row0 + row) * rank + r0 + r];
      up_s[r][row] = v;
    }
    // down tile: consecutive threads walk the stored columns
    for (int e = tid; e < kTile * kRankChunk; e += 256) {
      const int col = e % kTile, r = e / kTile;
      float v = 0.f;
      if (col0 + col < d.cols && r0 + r < rank) {
        const int j = lora_src_col(d, col0 + col);
        if (j >= 0) v = down[(int64_t)(r0 + r) * d.J + j];
      }
      down_s[r][col] = v;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < kRankChunk; ++r) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&up_s[r][ty * 4]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&down_s[r][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[i][k] = fmaf(a[i], b[k], acc[i][k]);
    }
    __syncthreads();
  }
  // epilogue: read-modify-write of the 4 x 4 micro-tile.  Rows of the logical matrix map to stored rows; (for W_GEGLU_W the tile walks
  // stored rows, all of which belong to the tensor)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + ty * 4 + i;
    if (row >= d.O) continue;
    f16* p = w + (int64_t)row * d.cols + col0 + tx * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = col0 + tx * 4 + k;
      if (c >= d.cols || lora_src_col(d, c) < 0) continue;
      if (scale * acc[i][k] == 0.f) continue;
      p[k] = (f16)fmaf(scale, acc[i][k], (float)p[k]);
    }
  }
}

__global__ __launch_bounds__(256) void lora_read_kernel(float* __restrict__ out, const f16* __restrict__ w, LoraDst d) {
  const int64_t total = (int64_t)d.O * d.J;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i / d.J), j = (int)(i - (int64_t)o * d.J);
    int64_t col = j;
    if (d.kind == W_CONV) {
      const int ch = j / d.khw, rs = j - ch * d.khw;
      col = (int64_t)rs * d.ipad + ch;
    }
    out[i] = (float)w[lora_dst_row(d, o) * d.cols + col];
  }
}

static int lora_dst(const char* who, LoraDst* d, int kind, int out, int in, int k, int ipad) {
  SDEO_CHECK(kind == W_LINEAR || kind == W_CONV || kind == W_GEGLU_W, "%s: tensor kind %d is not a matrix or a conv weight", who, kind);
  SDEO_CHECK(out > 0 && in > 0 && k > 0, "%s: bad shape out=%d in=%d k=%d", who, out, in, k);
  SDEO_CHECK(kind == W_CONV || k == 1, "%s: a matrix has k = 1 (got %d)", who, k);
  SDEO_CHECK(kind != W_CONV || ipad >= in, "%s: ipad=%d is below in=%d", who, ipad, in);
  SDEO_CHECK(kind != W_GEGLU_W || out % 32 == 0, "%s: a GEGLU projection has 2H rows with H a multiple of 16 (got %d rows)", who, out);
  SDEO_CHECK((int64_t)in * k * k < (1ll << 31) && (int64_t)k * k * (kind == W_CONV ? ipad : in) < (1ll << 31), "%s: row too long", who);
  d->kind = kind; d->O = out; d->J = in * k * k; d->in = in; d->khw = k * k; d->ipad = ipad; d->H = out / 2;
  d->cols = kind == W_CONV ? k * k * ipad : d->J;
  return 0;
}

}  // namespace

int lora_merge_f16(f16* w, int kind, int out, int in, int k, int ipad, const float* down, const float* up, int rank, float scale,
                   hipStream_t stream) {
  LoraDst d;
  SDEO_CHECK(w && down && up, "lora_merge_f16: null operand");
  if (int rc = lora_dst("lora_merge_f16", &d, kind, out, in, k, ipad)) return rc;
  SDEO_CHECK(rank >= 1 && rank <= 1024, "lora_merge_f16: rank %d out of range (1..1024)", rank);
  SDEO_CHECK(std::isfinite(scale), "lora_merge_f16: scale is not finite");
  const dim3 grid(cdiv(d.cols, kTile), cdiv(d.O, kTile));
  SDEO_CHECK(grid.y <= 65535, "lora_merge_f16: %d rows are more than one launch covers", out);
  hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), 0, stream, w, down, up, d, rank, scale);
  SDEO_HIP(hipGetLastError());
  return 0;
}

int lora_read_f32(float* out_f32, const f16* w, int kind, int out, int in, int k, int ipad, hipStream_t stream) {
  LoraDst d;
  SDEO_CHECK(w && out_f32, "lora_read_f32: null operand");
  if (int rc = lora_dst("lora_read_f32", &d, kind, out, in, k, ipad)) return rc;
  const int64_t total = (int64_t)d.O * d.J;
  hipLaunchKernelGGL(lora_read_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(total, 256), 65535)), dim3(256), 0, stream, out_f32, w, d);
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace sdeo

using namespace sdeo;

extern "C" {

// op-level entry (include/sdeo.h): down / up may be host or device pointers, so they are staged like WeightStore::load stages a
// tensor; the call allocates, synchronises and frees, and is therefore not capturable
int sdeo_lora_merge_f16(void* w, int kind, int out, int in, int k, int ipad, const float* down, const float* up, int rank, float scale,
                        void* stream) {
  SDEO_CHECK(w && down && up, "sdeo_lora_merge_f16: null argument");
  LoraDst d;
  if (int rc = lora_dst("sdeo_lora_merge_f16", &d, kind, out, in, k, ipad)) return rc;
  SDEO_CHECK(rank >= 1 && rank <= 1024, "sdeo_lora_merge_f16: rank %d out of range (1..1024)", rank);
  SDEO_CHECK(std::isfinite(scale), "sdeo_lora_merge_f16: scale is not finite");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t nd = (size_t)rank * in * k * k, nu = (size_t)out * rank;
  float* stage = nullptr;
  SDEO_HIP(hipMalloc((void**)&stage, (nd + nu) * sizeof(float)));
  int rc = 0;
  if (hipMemcpy(stage, down, nd * sizeof(float), hipMemcpyDefault) != hipSuccess ||
      hipMemcpy(stage + nd, up, nu * sizeof(float), hipMemcpyDefault) != hipSuccess)
    rc = fail("sdeo_lora_merge_f16: cannot copy down / up to the device");
  if (!rc) rc = lora_merge_f16((f16*)w, kind, out, in, k, ipad, stage, stage + nd, rank, scale, s);
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail("sdeo_lora_merge_f16: the merge launch failed");
  (void)hipFree(stage);
  return rc;
}

}  // extern "C"
