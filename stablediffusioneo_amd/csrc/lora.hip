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
//
// LoHa and LoKr (the forms are defined in include/sdeo.h) are siblings of that kernel over the same tile
// loaders, rank-chunk FMA and epilogue: only dW differs.  LoHa keeps two accumulator tiles and multiplies them; LoKr's loaders gather
// w2's low-rank pair through the Kronecker index map and its epilogue multiplies by the gathered w1 entry (a whole w2 is loaded there
// too, without the rank loop).  What has to be composed first -- w1 = w1_a @ w1_b, a Tucker core folded into its b factor -- is
// written as fp32 into the staging buffer by two small pre-pass kernels, after which a Tucker operand is an ordinary [rank][J] down
// whose up is read transposed.
#include <algorithm>
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

// LoKr: where a logical row / column of W finds its entry of the Kronecker factor w2 [Ok][J2], J2 = In * khw (LoRA and LoHa: unused)
struct KronMap {
  int Ok, In, J2;
  int Im;            // columns of w1 [O / Ok][Im]
};
__device__ __forceinline__ int kron_w2_col(const KronMap& m, const LoraDst& d, int j) {
  const int c = j / d.khw, s = j - c * d.khw;
  return (c % m.In) * d.khw + s;
}

// ---- the pieces the three merges share: two tile loaders, the rank-chunk FMA and the read-modify-write epilogue.  KRON: rows and
// columns go through the KronMap (the operand is w2's low-rank pair, not a pair as large as W).
//
// up tile, up_s[r][row]: entry (row, r) of an [rows][rank] matrix; with ld_t > 0 of its transpose [rank][ld_t] (the `a` factor of a
// Tucker form).  Consecutive threads walk whichever index is contiguous; rows past O and ranks past `rank` are zero.
template <bool KRON>
__device__ __forceinline__ void load_up_tile(float (*up_s)[kUpLd], const float* __restrict__ up, const LoraDst& d, const KronMap& m,
                                             int row0, int r0, int rank, int ld_t, int tid) {
  for (int e = tid; e < kTile * kRankChunk; e += 256) {
    const int r = ld_t ? e / kTile : e % kRankChunk, row = ld_t ? e % kTile : e / kRankChunk;
    float v = 0.f;
    if (row0 + row < d.O && r0 + r < rank) {
      int o = lora_src_row(d, row0 + row);
      if (KRON) o %= m.Ok;
      v = ld_t ? up[(int64_t)(r0 + r) * ld_t + o] : up[(int64_t)o * rank + r0 + r];
    }
    up_s[r][row] = v;
  }
}
// down tile, down_s[r][col]: consecutive threads walk the stored columns; pad channels and ranks past `rank` are zero
template <bool KRON>
__device__ __forceinline__ void load_down_tile(float (*down_s)[kTile], const float* __restrict__ down, const LoraDst& d, const KronMap& m,
                                               int col0, int r0, int rank, int tid) {
  for (int e = tid; e < kTile * kRankChunk; e += 256) {
    const int col = e % kTile, r = e / kTile;
    float v = 0.f;
    if (col0 + col < d.cols && r0 + r < rank) {
      const int j = lora_src_col(d, col0 + col);
      if (j >= 0) v = KRON ? down[(int64_t)(r0 + r) * m.J2 + kron_w2_col(m, d, j)] : down[(int64_t)(r0 + r) * d.J + j];
    }
    down_s[r][col] = v;
  }
}
__device__ __forceinline__ void tile_fma(float (&acc)[4][4], const float (*up_s)[kUpLd], const float (*down_s)[kTile], int ty, int tx) {
#pragma unroll 8
  for (int r = 0; r < kRankChunk; ++r) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(&up_s[r][ty * 4]);
    const f32x4 b = *reinterpret_cast<const f32x4*>(&down_s[r][tx * 4]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = fmaf(a[i], b[k], acc[i][k]);
  }
}
// epilogue: read-modify-write of the 4 x 4 micro-tile with dW = dw(i, k, stored row, stored column).  Rows of the logical matrix map
// to stored rows; (for W_GEGLU_W the tile walks stored rows, all of which belong to the tensor)
template <class F>
__device__ __forceinline__ void tile_store(f16* __restrict__ w, const LoraDst& d, int row0, int col0, int ty, int tx, float scale, F dw) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + ty * 4 + i;
    if (row >= d.O) continue;
    f16* p = w + (int64_t)row * d.cols + col0 + tx * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = col0 + tx * 4 + k;
      if (c >= d.cols || lora_src_col(d, c) < 0) continue;
      const float v = dw(i, k, row, c);
      if (scale * v == 0.f) continue;
      p[k] = (f16)fmaf(scale, v, (float)p[k]);
    }
  }
}

__global__ __launch_bounds__(256) void lora_merge_kernel(f16* __restrict__ w, const float* __restrict__ down, const float* __restrict__ up,
                                                         LoraDst d, int rank, float scale) {
  __shared__ __attribute__((aligned(16))) float up_s[kRankChunk][kUpLd];      // [r][row]
  __shared__ __attribute__((aligned(16))) float down_s[kRankChunk][kTile];    // [r][col]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * kTile, col0 = blockIdx.x * kTile;             // stored rows / columns of this tile
  const KronMap none{};
  float acc[4][4] = {};
  for (int r0 = 0; r0 < rank; r0 += kRankChunk) {
    load_up_tile<false>(up_s, up, d, none, row0, r0, rank, 0, tid);
    load_down_tile<false>(down_s, down, d, none, col0, r0, rank, tid);
    __syncthreads();
    tile_fma(acc, up_s, down_s, ty, tx);
    __syncthreads();
  }
  tile_store(w, d, row0, col0, ty, tx, scale, [&](int i, int k, int, int) { return acc[i][k]; });
}

// LoHa: dW = (a1 @ b1) (.) (a2 @ b2): two fmaf chains in rank order and one multiply.  b1 / b2 are [rank][J] (a Tucker core already
// folded in by lyco_fold_kernel), a1 / a2 [O][rank], or [rank][O] with ld_t = O (the Tucker form).
__global__ __launch_bounds__(256) void loha_merge_kernel(f16* __restrict__ w, const float* __restrict__ b1, const float* __restrict__ a1,
                                                         const float* __restrict__ b2, const float* __restrict__ a2, LoraDst d, int rank,
                                                         int ld_t, float scale) {
  __shared__ __attribute__((aligned(16))) float up_s[2][kRankChunk][kUpLd];
  __shared__ __attribute__((aligned(16))) float down_s[2][kRankChunk][kTile];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * kTile, col0 = blockIdx.x * kTile;
  const KronMap none{};
  float acc1[4][4] = {}, acc2[4][4] = {};
  for (int r0 = 0; r0 < rank; r0 += kRankChunk) {
    load_up_tile<false>(up_s[0], a1, d, none, row0, r0, rank, ld_t, tid);
    load_down_tile<false>(down_s[0], b1, d, none, col0, r0, rank, tid);
    load_up_tile<false>(up_s[1], a2, d, none, row0, r0, rank, ld_t, tid);
    load_down_tile<false>(down_s[1], b2, d, none, col0, r0, rank, tid);
    __syncthreads();
    tile_fma(acc1, up_s[0], down_s[0], ty, tx);
    tile_fma(acc2, up_s[1], down_s[1], ty, tx);
    __syncthreads();
  }
  tile_store(w, d, row0, col0, ty, tx, scale, [&](int i, int k, int, int) { return acc1[i][k] * acc2[i][k]; });
}

// LoKr: dW[ol * Ok + ok][(im * In + in) * khw + s] = w1[ol][im] * w2[ok][in * khw + s], with w2 either given whole (w2 != null: one
// loaded value) or as a2 @ b2 (one fmaf chain over its rank; a2 [Ok][rank], or [rank][Ok] with ld_t = Ok).  The logical row decides
// ol / ok (W_GEGLU_W), and a tile or a micro-tile may straddle any number of Kronecker blocks: every element finds its own entries.
__global__ __launch_bounds__(256) void lokr_merge_kernel(f16* __restrict__ w, const float* __restrict__ w1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, const float* __restrict__ a2, LoraDst d, KronMap m,
                                                         int rank, int ld_t, float scale) {
  __shared__ __attribute__((aligned(16))) float up_s[kRankChunk][kUpLd];
  __shared__ __attribute__((aligned(16))) float down_s[kRankChunk][kTile];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * kTile, col0 = blockIdx.x * kTile;
  float acc[4][4] = {};
  if (!w2)
    for (int r0 = 0; r0 < rank; r0 += kRankChunk) {
      load_up_tile<true>(up_s, a2, d, m, row0, r0, rank, ld_t, tid);
      load_down_tile<true>(down_s, b2, d, m, col0, r0, rank, tid);
      __syncthreads();
      tile_fma(acc, up_s, down_s, ty, tx);
      __syncthreads();
    }
  tile_store(w, d, row0, col0, ty, tx, scale, [&](int i, int k, int row, int c) {
    const int o = lora_src_row(d, row), ol = o / m.Ok, j = lora_src_col(d, c), im = j / d.khw / m.In;
    const float v = w2 ? w2[(int64_t)(o - ol * m.Ok) * m.J2 + kron_w2_col(m, d, j)] : acc[i][k];
    return w1[(int64_t)ol * m.Im + im] * v;
  });
}

// ---- the pre-pass: composed operands as fp32 into the staging buffer, each sum one fmaf chain in index order
// out[m][n] = sum_r a[m][r] * b[r][n]   (LoKr's w1 = w1_a @ w1_b)
__global__ __launch_bounds__(256) void lyco_compose_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                                                           int M, int N, int rank) {
  const int64_t total = (int64_t)M * N;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int mm = (int)(e / N), n = (int)(e - (int64_t)mm * N);
    float s = 0.f;
    for (int r = 0; r < rank; ++r) s = fmaf(a[(int64_t)mm * rank + r], b[(int64_t)r * N + n], s);
    out[e] = s;
  }
}
// a Tucker core t [rank][rank][khw] folded into its b factor [rank][I]:  out[i][c * khw + s] = sum_j t[i][j][s] * b[j][c]
__global__ __launch_bounds__(256) void lyco_fold_kernel(float* __restrict__ out, const float* __restrict__ t, const float* __restrict__ b,
                                                        int rank, int I, int khw) {
  const int J = I * khw;
  const int64_t total = (int64_t)rank * J;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / J), cs = (int)(e - (int64_t)i * J), c = cs / khw, s = cs - c * khw;
    float v = 0.f;
    for (int j = 0; j < rank; ++j) v = fmaf(t[((int64_t)i * rank + j) * khw + s], b[(int64_t)j * I + c], v);
    out[e] = v;
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

int lyco_check(const char* who, const LycoOps& p, int kind, int out, int in, int k) {
  const bool rank_ok1 = p.rank1 >= 1 && p.rank1 <= 1024, rank_ok2 = p.rank2 >= 1 && p.rank2 <= 1024;
  if (p.algo == LYCO_LOHA) {
    SDEO_CHECK(p.a1 && p.b1 && p.a2 && p.b2, "%s: null operand (hada_w1_a, hada_w1_b, hada_w2_a and hada_w2_b are all required)", who);
    SDEO_CHECK(!p.t1 == !p.t2, "%s: null operand (hada_t1 and hada_t2 come together)", who);
    SDEO_CHECK(rank_ok1, "%s: rank %d out of range (1..1024)", who, p.rank1);
    SDEO_CHECK(!p.t1 || (kind == W_CONV && k > 1), "%s: the factor shapes do not fit the tensor: a Tucker core (hada_t1 / hada_t2) needs a "
               "conv weight with a filter larger than 1 x 1, this one is %d x %d x %d x %d", who, out, in, k, k);
    return 0;
  }
  SDEO_CHECK(p.algo == LYCO_LOKR, "%s: unknown adapter form %d", who, p.algo);
  SDEO_CHECK(!p.a1 == !p.b1 && !p.w1 != !p.a1, "%s: null operand (w1 comes either whole or as lokr_w1_a and lokr_w1_b)", who);
  SDEO_CHECK(!p.a2 == !p.b2 && !p.w2 != !p.a2 && (!p.t2 || p.a2), "%s: null operand (w2 comes whole, as lokr_w2_a and lokr_w2_b, or as those two "
             "with lokr_t2)", who);
  SDEO_CHECK(!p.a1 || rank_ok1, "%s: rank %d of w1 out of range (1..1024)", who, p.rank1);
  SDEO_CHECK(!p.a2 || rank_ok2, "%s: rank %d of w2 out of range (1..1024)", who, p.rank2);
  SDEO_CHECK(p.out_l >= 1 && p.in_m >= 1 && out % p.out_l == 0 && in % p.in_m == 0, "%s: the factor shapes do not fit the tensor: w1 %d x %d "
             "does not divide the %d x %d of the weight", who, p.out_l, p.in_m, out, in);
  SDEO_CHECK(!p.t2 || (kind == W_CONV && k > 1), "%s: the factor shapes do not fit the tensor: a Tucker core (lokr_t2) needs a conv weight "
             "with a filter larger than 1 x 1, this one is %d x %d x %d x %d", who, out, in, k, k);
  return 0;
}

namespace {

// the staging buffer of one merge, filled front to back; base == null only counts
struct LycoStage {
  float* base;
  size_t used = 0;
  bool failed = false;
  float* room(size_t n) {
    float* p = base ? base + used : nullptr;
    used += n;
    return p;
  }
  const float* put(const float* src, size_t n) {
    float* p = room(n);
    if (p && hipMemcpy(p, src, n * sizeof(float), hipMemcpyDefault) != hipSuccess) failed = true;
    return p;
  }
};

inline unsigned prepass_grid(int64_t total) { return (unsigned)std::min<int64_t>(cdiv64(total, 256), 4096); }

// a Tucker triple (t [r][r][k][k], a [r][rows], b [r][cols]) as an ordinary pair: *b_eff [r][cols * k * k], `a` stays transposed
const float* stage_fold(LycoStage& st, const float* t, const float* b, int rank, int cols, int khw, hipStream_t stream) {
  const float* td = st.put(t, (size_t)rank * rank * khw);
  const float* bd = st.put(b, (size_t)rank * cols);
  float* eff = st.room((size_t)rank * cols * khw);
  if (eff && !st.failed)
    hipLaunchKernelGGL(lyco_fold_kernel, dim3(prepass_grid((int64_t)rank * cols * khw)), dim3(256), 0, stream, eff, td, bd, rank, cols, khw);
  return eff;
}

// stage == null: count the floats into *floats and touch nothing
int lyco_run(f16* w, int kind, int out, int in, int k, int ipad, const LycoOps& p, float* stage, size_t* floats, float scale, hipStream_t stream) {
  LoraDst d;
  if (int rc = lora_dst("lyco_merge_f16", &d, kind, out, in, k, ipad)) return rc;
  LycoStage st{stage};
  const dim3 grid(cdiv(d.cols, kTile), cdiv(d.O, kTile));
  SDEO_CHECK(grid.y <= 65535, "lyco_merge_f16: %d rows are more than one launch covers", out);
  if (p.algo == LYCO_LOHA) {
    const int r = p.rank1;
    const float *a1 = st.put(p.a1, (size_t)out * r), *a2 = st.put(p.a2, (size_t)out * r), *b1, *b2;
    if (p.t1) {
      b1 = stage_fold(st, p.t1, p.b1, r, in, d.khw, stream);
      b2 = stage_fold(st, p.t2, p.b2, r, in, d.khw, stream);
    } else {
      b1 = st.put(p.b1, (size_t)r * d.J);
      b2 = st.put(p.b2, (size_t)r * d.J);
    }
    if (floats) *floats = st.used;
    if (!stage) return 0;
    SDEO_CHECK(!st.failed, "lyco_merge_f16: cannot copy the LoHa operands to the device");
    hipLaunchKernelGGL(loha_merge_kernel, grid, dim3(256), 0, stream, w, b1, a1, b2, a2, d, r, p.t1 ? out : 0, scale);
  } else {
    KronMap m;
    m.Ok = out / p.out_l; m.In = in / p.in_m; m.J2 = m.In * d.khw; m.Im = p.in_m;
    const float* w1;
    if (p.w1) {
      w1 = st.put(p.w1, (size_t)p.out_l * p.in_m);
    } else {
      const float *a = st.put(p.a1, (size_t)p.out_l * p.rank1), *b = st.put(p.b1, (size_t)p.rank1 * p.in_m);
      float* c = st.room((size_t)p.out_l * p.in_m);
      if (c && !st.failed)
        hipLaunchKernelGGL(lyco_compose_kernel, dim3(prepass_grid((int64_t)p.out_l * p.in_m)), dim3(256), 0, stream, c, a, b, p.out_l, p.in_m, p.rank1);
      w1 = c;
    }
    const float *w2 = nullptr, *a2 = nullptr, *b2 = nullptr;
    if (p.w2) {
      w2 = st.put(p.w2, (size_t)m.Ok * m.J2);
    } else {
      a2 = st.put(p.a2, (size_t)m.Ok * p.rank2);
      b2 = p.t2 ? stage_fold(st, p.t2, p.b2, p.rank2, m.In, d.khw, stream) : st.put(p.b2, (size_t)p.rank2 * m.J2);
    }
    if (floats) *floats = st.used;
    if (!stage) return 0;
    SDEO_CHECK(!st.failed, "lyco_merge_f16: cannot copy the LoKr operands to the device");
    hipLaunchKernelGGL(lokr_merge_kernel, grid, dim3(256), 0, stream, w, w1, w2, b2, a2, d, m, p.w2 ? 0 : p.rank2, p.t2 ? m.Ok : 0, scale);
  }
  SDEO_HIP(hipGetLastError());
  return 0;
}

}  // namespace

size_t lyco_stage_floats(const LycoOps& ops, int out, int in, int k) {
  size_t n = 0;
  // (kind and ipad do not change the count; W_CONV with ipad = in passes lora_dst for every k)
  (void)lyco_run(nullptr, W_CONV, out, in, k, in, ops, nullptr, &n, 0.f, 0);
  return n;
}

int lyco_merge_f16(f16* w, int kind, int out, int in, int k, int ipad, const LycoOps& ops, float* stage, float scale, hipStream_t stream) {
  SDEO_CHECK(w && stage, "lyco_merge_f16: null operand");
  return lyco_run(w, kind, out, in, k, ipad, ops, stage, nullptr, scale, stream);
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

// the same for the LoHa / LoKr merges: every refusal first, then stage, pre-pass, merge, synchronise, free
static int lyco_merge_entry(const char* who, void* w, int kind, int out, int in, int k, int ipad, const LycoOps& ops, float scale, void* stream) {
  SDEO_CHECK(w, "%s: null operand (w)", who);
  LoraDst d;
  if (int rc = lora_dst(who, &d, kind, out, in, k, ipad)) return rc;
  if (int rc = lyco_check(who, ops, kind, out, in, k)) return rc;
  SDEO_CHECK(std::isfinite(scale), "%s: scale is not finite", who);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* stage = nullptr;
  SDEO_HIP(hipMalloc((void**)&stage, lyco_stage_floats(ops, out, in, k) * sizeof(float)));
  int rc = lyco_merge_f16((f16*)w, kind, out, in, k, ipad, ops, stage, scale, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("%s: the merge launch failed", who);
  (void)hipFree(stage);
  return rc;
}

int sdeo_loha_merge_f16(void* w, int kind, int out, int in, int k, int ipad, const float* w1_a, const float* w1_b, const float* w2_a,
                        const float* w2_b, const float* t1, const float* t2, int rank, float scale, void* stream) {
  LycoOps ops;
  ops.algo = LYCO_LOHA; ops.a1 = w1_a; ops.b1 = w1_b; ops.t1 = t1; ops.a2 = w2_a; ops.b2 = w2_b; ops.t2 = t2; ops.rank1 = ops.rank2 = rank;
  return lyco_merge_entry("sdeo_loha_merge_f16", w, kind, out, in, k, ipad, ops, scale, stream);
}

int sdeo_lokr_merge_f16(void* w, int kind, int out, int in, int k, int ipad, const float* w1, const float* w1_a, const float* w1_b, int rank1,
                        const float* w2, const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale,
                        void* stream) {
  LycoOps ops;
  ops.algo = LYCO_LOKR; ops.w1 = w1; ops.a1 = w1_a; ops.b1 = w1_b; ops.rank1 = rank1; ops.w2 = w2; ops.a2 = w2_a; ops.b2 = w2_b; ops.t2 = t2;
  ops.rank2 = rank2; ops.out_l = out_l; ops.in_m = in_m;
  return lyco_merge_entry("sdeo_lokr_merge_f16", w, kind, out, in, k, ipad, ops, scale, stream);
}

}  // extern "C"
