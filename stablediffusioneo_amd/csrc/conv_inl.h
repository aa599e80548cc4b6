// Device-side pieces shared by the implicit-GEMM kernels (conv_gemm.hip) and the halo-reuse 3x3 kernel (conv_halo.hip):
// kernel parameter block, epilogue, XCD-aware tile order, LDS-DMA / fragment-read helpers.
#pragma once
#include <type_traits>
#include <utility>

#include "kernels.h"

namespace sdeo {

struct KP {
  const f16* x;
  const f16* w;
  f16* y;
  float* y32;
  const float* bias;
  const float* bias2;
  const f16* res;
  float* ws;
  int M, N, K;
  int Hi, Wi, Cin, Ho, Wo, S, stride, pad, ups;
  int HoWo;
  int ldx, ldw, ldy, ldres, ld_bias2;
  int res_rows;      // rows of `res`: output row m adds residual row m - res_rows when m >= res_rows (= M: one residual row per output
                     // row; M / 2: the second half of the batch re-reads the first half's residual, see ConvGemm::res_rows)
  int act, bias_per_row;
  float scale;
  int nk, nk_per_split, splitk;
  int tiles_m, tiles_n;
  // measurement builds only (-DSDEO_DEBUG_KERNELS, `python -m stablediffusioneo_amd.build --debug` -> libsdeo_dbg.so; the
  // field is ignored by the production kernels): SDEO_DBG_GEMM bits, results are wrong under them: 1 = activation DMAs read
  // the zero page, 2 = weight DMAs do, 4 = no MFMAs, 8 = no DMAs after the prologue, 16 = no fragment reads, 32 = no epilogue,
  // 64 = phase stamps, 128 (with 64) = a second trip through the same epilogue instructions, resident by then (stamps 5 -> 6)
  int dbg;
  int n_fastest;     // tile order inside an XCD's contiguous run: 1 = all N tiles of an M tile are neighbours
  int coalesce;      // host-checked: the LDS-transposed 16-byte epilogue applies (see epilogue_rows)
  // ---- LayerNorm folded into this GEMM (the consumer of a pre-LN residual stream, `attention.py:381-385`):
  //      LN(x) W^T + b = rstd * (x W'^T - mean * s) + b'   with W' = W * gamma (fp16), s[n] = sum_k W'[n][k],
  //      b'[n] = b[n] + sum_k beta[k] W[n][k] (passed as `bias`).  The K loop runs on the RAW x; the epilogue applies the two
  //      per-row scalars.  (mean, rstd) come from per-row partial (sum, sum of squares) written by the PRODUCER of x.
  const float* ln_stats;   // [rows][ln_ld][2] partial (sum, sumsq) per row of x, ln_strips valid partials per row; null = off
  const float* ln_s;       // [N]
  int ln_strips, ln_ld;
  float ln_invc, ln_eps;
  // ---- fp8 weights (conv_gemm_dma_kernel<..., W8>): `w` points at bytes, ldw counts bytes, the accumulators are multiplied by the
  //      per-output-channel scale before anything else in the epilogue (or in the split-K reduce)
  const float* wscale;     // [N]; null = fp16 weights
  // ---- producer side: per-row partial (sum, sumsq) of the values this launch stores, one partial per TN-wide strip
  float* stats_out;        // [M][stats_ld][2]; null = off
  int stats_ld;
  // ---- producer side, GroupNorm (`util.py:217-219`): per-(image, M tile of the image, group) partial (sum, sumsq) of the values this
  //      launch stores, so that the GroupNorm that consumes y needs no statistics pass.  Every (image, tile, group) entry is written
  //      by exactly one workgroup (host-checked: strips cover whole groups, tiles do not straddle images, unsplit fp16 plan);
  //      the consumer sums the gn_slots entries of a group in a fixed order (deterministic, no atomics).
  float* gn_out;           // [B][gn_slots][gn_groups][2]; null = off
  int gn_cpg, gn_slots, gn_groups;
  // ---- block-scaled fp8 operands (conv_gemm_dma_kernel<..., MX>, GEMM only): x and w hold OCP e4m3fn codes (one byte per element,
  //      addressed through this block as fp16 arrays of half the length: K, Cin, ldx, ldw count PAIRS of codes), mx_sx / mx_sw one
  //      e8m0 scale byte per 32 codes of a row.  The MFMA is v_mfma_scale_f32_16x16x128_f8f6f4: 128 codes per K-step.
  const unsigned char* mx_sx;   // [M][mx_ldsx]; null = off
  const unsigned char* mx_sw;   // [N][mx_ldsw]
  int mx_ldsx, mx_ldsw;
};

// Multi-problem launch (conv_gemm_dma_kernel<..., MULTI>): several problems that run on the same tile, unsplit, as ONE grid.
// MPTable lives in device memory and is written when the launch is configured: the problems' parameter blocks and the inclusive
// prefix sums of their tile counts (entries past the last problem hold INT_MAX, so a scan needs no count).  MPArgs is the kernel
// argument: sixteen blocks would not fit the 4 KB argument segment, and `scale` must be the value of the moment of the launch.
struct MPTable {
  int prefix[kMultiMax];
  KP kp[kMultiMax];
};
struct MPArgs {
  const MPTable* tab;
  int count;
  float scale[kMultiMax];
};
// The argument of the live-row instantiation (conv_gemm_dma_kernel<..., MULTI, LIVE>): MPArgs plus, per problem, how many of its M rows
// are live.  Rows at or beyond m_live are not computed: they receive their `res` row as it is (nothing when res is the output itself).
// A type of its own, so that MPArgs -- the argument of the plain multi-problem kernel -- stays what it was.
struct MPArgsLive {
  const MPTable* tab;
  int count;
  float scale[kMultiMax];
  int m_live[kMultiMax];
};
// reads of the table go through the constant address space: it does not change under the launch, and loads from there at a uniform
// address are scalar ones (one s_load_dwordx16 for the prefix sums, a batch of them for a block)
__device__ __forceinline__ int mp_prefix(const MPTable* tab, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((const __attribute__((address_space(4))) MPTable*)tab)->prefix[i];
#else
  return tab->prefix[i];
#endif
}
__device__ __forceinline__ KP mp_block(const MPTable* tab, int prob) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((const __attribute__((address_space(4))) MPTable*)tab)->kp[prob];
#else
  return tab->kp[prob];
#endif
}
// a block read from device memory: its pointers are global ones (the compiler knows that of kernel arguments only, and every access
// through a generic pointer is a flat_ one, which also counts on lgkmcnt)
__device__ __forceinline__ void mp_globalize(KP& q) {
#define SDEO_GLOBAL_PTR(f) q.f = (decltype(q.f))(__attribute__((address_space(1))) std::remove_pointer_t<decltype(q.f)>*)q.f;
  SDEO_GLOBAL_PTR(x) SDEO_GLOBAL_PTR(w) SDEO_GLOBAL_PTR(y) SDEO_GLOBAL_PTR(y32) SDEO_GLOBAL_PTR(bias) SDEO_GLOBAL_PTR(bias2)
  SDEO_GLOBAL_PTR(res) SDEO_GLOBAL_PTR(ws) SDEO_GLOBAL_PTR(ln_stats) SDEO_GLOBAL_PTR(ln_s) SDEO_GLOBAL_PTR(wscale)
  SDEO_GLOBAL_PTR(stats_out) SDEO_GLOBAL_PTR(gn_out) SDEO_GLOBAL_PTR(mx_sx) SDEO_GLOBAL_PTR(mx_sw)
#undef SDEO_GLOBAL_PTR
}

// Ablation / stamp switches exist only in the measurement build: in the production library dbg_on() is the constant false and
// every branch on it (and the stamp code) is compiled out of the K loops.
#ifdef SDEO_DEBUG_KERNELS
__device__ __forceinline__ bool dbg_on(const KP& p, int bit) { return (p.dbg & bit) != 0; }
#else
__device__ __forceinline__ constexpr bool dbg_on(const KP&, int) { return false; }
#endif

// SDEO_DBG_GEMM bit 6 (64): per-workgroup phase stamps (s_memrealtime, 100 MHz, chip-wide) written by MFMA wave 0, lane 0:
// [0] kernel entry, [1] address set-up done, [2] first K-step visible, [3] K loop done, [4] epilogue stores issued,
// [5] stores complete.  One copy of the buffer per translation unit; read with sdeo_debug_read_stamps.
constexpr int kStampWGs = 4096, kStampSlots = 16;
static __device__ unsigned long long g_stamps[kStampWGs * kStampSlots];
__device__ __forceinline__ void stamp_cycles(const KP& p, int slot) {      // shader-clock counter (for the in-kernel clock rate)
  if (dbg_on(p, 64) && threadIdx.x == 0) {
    const int wg = blockIdx.x + gridDim.x * blockIdx.z;
    if (wg < kStampWGs) g_stamps[wg * kStampSlots + slot] = __builtin_amdgcn_s_memtime();
  }
}
__device__ __forceinline__ void stamp(const KP& p, int slot) {
  if (dbg_on(p, 64) && threadIdx.x == 0) {
    const int wg = blockIdx.x + gridDim.x * blockIdx.z;
    if (wg < kStampWGs) g_stamps[wg * kStampSlots + slot] = __builtin_amdgcn_s_memrealtime();
  }
}

// 256 bytes of zeros: DMA source for padded / out-of-range rows
static __device__ __attribute__((aligned(256))) const unsigned int g_zero_page[64] = {0};

template <int BK>
__device__ __forceinline__ int swz_chunk(int row, int chunk) {
  // conflict-free for the 16-lane groups of ds_read_b128 when lanes read rows r..r+15 at one k-chunk
  if (BK == 64) return chunk ^ ((row >> 1) & 7);
  return chunk ^ (((row >> 3) & 1) * 3);
}

// ---- epilogue shared by all kernels: lane holds n = nb + i*16 + fq*4 + {0..3} (4 consecutive channels) of output row
//      mrow[j] (-1: no such row) for accumulator tile (i, j); nb = first column of this wave's TN-wide strip
// `scratch` (optional): wave-private LDS, >= epilogue_scratch_bytes(TN) bytes, free of pending DMAs and of other waves'
// fragment reads.  With it (and p.coalesce set by the host: fp16 output, no split-K, N % 8 == 0, 16-byte aligned rows) the
// wave transposes each 16-row block of fp32 results through LDS so that every lane then moves 8 consecutive channels:
// 16-byte residual loads and 16-byte stores in runs of TN*2 contiguous bytes per row, instead of 8-byte pieces in 32-byte
// runs (measured: the 8-byte epilogue took ~4 us of a 24 us conv).  Same arithmetic, same single rounding.
constexpr int epilogue_scratch_bytes(int tn) { return 16 * (tn * 4 + 16) + 32 * tn; }   // + [16 rows][tn / 8] float2 row-statistics partials
                                                                                        //   or [16 rows][tn] fp16 copy of the stored block (GroupNorm partials)

// The epilogue reads ~25 scalar parameters.  Left to the compiler they are loaded from the kernel-argument segment where first
// used, one s_load + s_waitcnt lgkmcnt(0) after the other (the loads are invariant, so it prefers re-loading to keeping SGPRs
// live across the K loop): a serial chain of scalar-cache round trips at the start of every epilogue.  Kernels therefore copy the
// parameters right BEFORE the pre-epilogue barrier and pin the epilogue's fields in SGPRs here: one batch of wide loads whose
// latency hides behind the barrier.
__device__ __forceinline__ unsigned long long pin_u64(unsigned long long v) {
  unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  asm volatile("" : "+s"(lo), "+s"(hi));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int pin_i32(int v) {
  int r = __builtin_amdgcn_readfirstlane(v);
  asm volatile("" : "+s"(r));
  return r;
}
__device__ __forceinline__ float pin_f32(float v) { return __builtin_bit_cast(float, pin_i32(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ void pin_epilogue_scalars(KP& q) {
  // pointers travel through the asm as integers and come back as GLOBAL pointers: pinned as generic pointers they would lose
  // their address space and every access would become a flat_ one (which also counts on lgkmcnt and would serialise with the
  // epilogue's LDS traffic)
#define SDEO_PIN_PTR(f) q.f = (decltype(q.f))(__attribute__((address_space(1))) std::remove_pointer_t<decltype(q.f)>*)pin_u64((unsigned long long)q.f);
  SDEO_PIN_PTR(y) SDEO_PIN_PTR(y32) SDEO_PIN_PTR(bias) SDEO_PIN_PTR(bias2) SDEO_PIN_PTR(res) SDEO_PIN_PTR(ws)
  SDEO_PIN_PTR(wscale) SDEO_PIN_PTR(stats_out) SDEO_PIN_PTR(ln_stats) SDEO_PIN_PTR(ln_s) SDEO_PIN_PTR(gn_out)
#undef SDEO_PIN_PTR
  q.M = pin_i32(q.M); q.N = pin_i32(q.N); q.HoWo = pin_i32(q.HoWo); q.ldy = pin_i32(q.ldy); q.ldres = pin_i32(q.ldres);
  q.res_rows = pin_i32(q.res_rows);
  q.ld_bias2 = pin_i32(q.ld_bias2); q.act = pin_i32(q.act); q.bias_per_row = pin_i32(q.bias_per_row); q.scale = pin_f32(q.scale);
  q.splitk = pin_i32(q.splitk); q.coalesce = pin_i32(q.coalesce); q.stats_ld = pin_i32(q.stats_ld); q.ln_strips = pin_i32(q.ln_strips);
  q.ln_ld = pin_i32(q.ln_ld); q.ln_invc = pin_f32(q.ln_invc); q.ln_eps = pin_f32(q.ln_eps);
  q.gn_cpg = pin_i32(q.gn_cpg); q.gn_slots = pin_i32(q.gn_slots); q.gn_groups = pin_i32(q.gn_groups);
}

// row of `res` that output row m adds (KP::res_rows)
__device__ __forceinline__ int res_row(const KP& p, int m) { return m >= p.res_rows ? m - p.res_rows : m; }

// blocks staged per round: the largest divisor of MI whose scratch fits `budget` bytes per wave and whose residual registers
// (PASSES 16-byte vectors per block) stay within 8 vectors
constexpr int epilogue_blocks(int tn, int mi, int budget) {
  const int passes = (16 * (tn / 8) + 63) / 64;
  int best = 1;
  for (int nb = 1; nb <= mi; ++nb)
    if (mi % nb == 0 && nb * epilogue_scratch_bytes(tn) <= budget && nb * passes <= 8) best = nb;
  return best;
}

// one 16-row block of the coalesced epilogue, flags resolved at compile time (a scalar branch per flag per tile cost more
// than the arithmetic: ~60 taken branches per wave)
template <int NI, int TN, bool B2, int ACT>
__device__ __forceinline__ void stage_block(const KP& p, const f32x4 (&accj)[NI], const f32x4 (&bias)[NI], int m, int nb, int fq,
                                            int frow, char* scratch) {
  constexpr int ROWB = TN * 4 + 16;
  const float* b2p = nullptr;
  if (B2) b2p = p.bias2 + (size_t)(m >= 0 ? m / p.HoWo : 0) * p.ld_bias2 + nb + fq * 4;
  f32x4 b2[NI];
  if (B2) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      b2[i] = (nb + i * 16 + fq * 4 < p.N) ? *reinterpret_cast<const f32x4*>(b2p + i * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    f32x4 v = accj[i] + bias[i];
    if (B2) v += b2[i];
    if (ACT == 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = silu_f(v[t]);
    } else if (ACT == 2) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = quick_gelu_f(v[t]);
    } else if (ACT == 4) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
    } else if (ACT == 5) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = gelu_erf_f(v[t]);
    }
    v *= p.scale;
    *reinterpret_cast<f32x4*>(scratch + frow * ROWB + (i * 16 + fq * 4) * 4) = v;
  }
}

// (mean, rstd) of one row of the LayerNorm'ed operand from the producer's per-strip partials (fixed order: deterministic)
__device__ __forceinline__ void ln_row_scalars(const KP& p, int row, float& r, float& rm) {
  const float2* src = reinterpret_cast<const float2*>(p.ln_stats) + (size_t)row * p.ln_ld;
  float s = 0.f, q = 0.f;
  for (int t0 = 0; t0 < p.ln_strips; t0 += 8) {       // 8 independent loads in flight, summed in a fixed order
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = t0 + u < p.ln_strips ? src[t0 + u] : make_float2(0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 8; ++u) { s += v[u].x; q += v[u].y; }
  }
  const float mean = s * p.ln_invc;
  float var = q * p.ln_invc - mean * mean;
  var = var < 0.f ? 0.f : var;
  r = rsqrtf(var + p.ln_eps);
  rm = r * mean;
}

// ---- epilogue kind: a compile-time argument of the kernels, chosen per launch on the host (conv_gemm.hip: prepare / dispatch).
//      The tile table's rows and names do not know about it.
//  EPI_STAGED  everything epilogue_rows does (LDS-transposed stores, GEGLU pair, GroupNorm partials, split-K slabs, 8-byte fallback)
//  EPI_DIRECT  16-byte stores straight from the accumulators (epilogue_direct): the weight rows of a strip are dealt to the MFMA
//              rows in a permuted order, so that a lane holds 8 consecutive channels across accumulator tiles 2q and 2q + 1
// The kinds from EPI_SPLITK on are the staged family: epilogue_rows with the tests of one launch mode resolved at compile time
// (EpiMode below), so that a launch carries the one path it takes instead of all of them.  Same source text, same operations in
// the same order: every stored value, GroupNorm partial and split-K slab is bit-identical to EPI_STAGED, which stays the fallback
// of every launch without a specialised form.  The host picks the kind (conv_gemm.hip: epi_kind) and guarantees its mode.
//  EPI_SPLITK  splitk > 1: the fp32 slab stores of the per-row loop
//  EPI_GEGLU   act == 3 on the coalesced path: the pair path through the LDS transposition (LayerNorm fold still read at run time)
//  EPI_GN      coalesced, GroupNorm partials out, no bias2, no activation (residual read at run time)
//  EPI_GN_B2   the same with a per-image bias2
enum EpiKind { EPI_STAGED = 0, EPI_DIRECT = 1, EPI_SPLITK = 2, EPI_GEGLU = 3, EPI_GN = 4, EPI_GN_B2 = 5, EPI_KINDS = 6 };

// What a kind knows of its launch at compile time.  Each predicate reads the parameter block in EPI_STAGED and is a constant in a
// specialised kind, so the branches of epilogue_rows it guards exist in the instantiations that can take them only.
template <int EPI>
struct EpiMode {
  static_assert(EPI == EPI_STAGED || (EPI >= EPI_SPLITK && EPI < EPI_KINDS), "a kind of the staged family");
  static constexpr bool generic = EPI == EPI_STAGED;
  static constexpr bool k_gn = EPI == EPI_GN || EPI == EPI_GN_B2;
  static constexpr bool k_block = k_gn;                 // the kinds of the coalesced block path
  static constexpr bool k_b2 = EPI == EPI_GN_B2;        // stage_block<..., B2, ACT> of a block kind
  static constexpr int k_act = 0;
  static __device__ __forceinline__ bool split(const KP& p) { return generic ? p.splitk > 1 : EPI == EPI_SPLITK; }
  static __device__ __forceinline__ bool pair(const KP& p, const char* scratch) { return generic ? scratch && p.coalesce && p.act == 3 : EPI == EPI_GEGLU; }
  static __device__ __forceinline__ bool block(const KP& p, const char* scratch) { return generic ? scratch && p.coalesce && p.act != 3 : k_block; }
  static __device__ __forceinline__ bool gn(const KP& p) { return generic ? p.gn_out != nullptr : k_gn; }
  static __device__ __forceinline__ bool stats(const KP& p) { return generic && p.stats_out != nullptr; }
  static __device__ __forceinline__ bool wscale(const KP& p) { return generic && p.wscale != nullptr && p.splitk == 1; }
  static __device__ __forceinline__ bool ln(const KP& p) { return generic ? p.ln_stats != nullptr && p.splitk == 1 : EPI == EPI_GEGLU && p.ln_stats != nullptr; }
};

// EPI_DIRECT channel map of a strip of NI 16-row accumulator tiles.  Row rho of tile i carries channel
// 32 (i >> 1) + 8 (rho >> 2) + 4 (i & 1) + (rho & 3) of the strip: the accumulator rows of lane (frow, fq) are rho = 4 fq + t, so the
// lane holds channels 32 q + 8 fq + {0..3} in tile 2q and + {4..7} in tile 2q + 1, and the four fq lanes of a pixel cover 32
// consecutive channels.  An unpaired last tile (NI odd) keeps the plain order: 16 i + rho.
template <int NI>
__device__ __forceinline__ constexpr int direct_row_chan(int r) {          // channel held by row r (= 16 i + rho) of the strip
  const int i = r >> 4, rho = r & 15;
  return (NI % 2 == 1 && i == NI - 1) ? r : 32 * (i >> 1) + 8 * (rho >> 2) + 4 * (i & 1) + (rho & 3);
}
template <int NI, bool DIRECT>
__device__ __forceinline__ constexpr int lane_chan(int i, int fq) {        // first of the 4 channels lane quarter fq holds in tile i
  return DIRECT ? direct_row_chan<NI>(i * 16 + fq * 4) : i * 16 + fq * 4;
}

// acc <- rstd * acc - rstd * mean * s   (see KP::ln_stats).  `lnrow` (optional, LDS): the (rstd, rstd * mean) of this wave's
// rows, indexed j * 16 + frow, computed at kernel start while the first K-step was in flight (conv_gemm_dma_kernel); without it
// each lane sums its rows' partials here.
template <int NI, int MI, bool DIRECT = false>
__device__ __forceinline__ void ln_correct(const KP& p, f32x4 (&acc)[NI][MI], const int (&mrow)[MI], int nb, int fq,
                                           const float2* lnrow) {
  const int frow = threadIdx.x & 15;
  float r[MI], rm[MI];
#pragma unroll
  for (int j = 0; j < MI; ++j) {
    r[j] = 0.f; rm[j] = 0.f;
    if (lnrow) { const float2 v = lnrow[j * 16 + frow]; r[j] = v.x; rm[j] = v.y; }
    else if (mrow[j] >= 0) ln_row_scalars(p, mrow[j], r[j], rm[j]);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = nb + lane_chan<NI, DIRECT>(i, fq);
    const f32x4 sv = n < p.N ? *reinterpret_cast<const f32x4*>(p.ln_s + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = acc[i][j] * r[j] - sv * rm[j];
  }
}

// EPI_DIRECT epilogue: the plain modes (act 0 / 1 / 2 / 4 / 5, bias, control scale, residual, LayerNorm-folded
// input, row statistics out; not the per-image bias2: measured slower here than staged) of an unsplit fp16 launch whose rows are 16-byte aligned (the host's conditions for KP::coalesce),
// straight from the accumulators in the lane_chan<NI, true> layout.  No LDS, no wave barrier, one pass: per (pixel, 8 channels)
// one 16-byte residual load and one 16-byte store; the four fq lanes of a pixel write 64 contiguous bytes.  An unpaired last tile
// (NI odd) moves 8 bytes.  Same arithmetic and the same single rounding as the staged path, in the same order (bias,
// activation, scale, residual; the multiply by `scale` is kept apart from the residual add as it is there), so the stored values
// are bit-identical.  The row statistics keep the staged path's summation order as well (the 8 values of a group in channel order,
// then the groups of the strip in channel order: the partials of a row's groups are gathered into its fq = 0 lane by index
// shuffles), so they are bit-identical too and a network computes the same bits on either kind.
__device__ __forceinline__ float relu_f(float v) { return fmaxf(v, 0.f); }
template <int NI, int MI, int TN>
__device__ __forceinline__ void epilogue_direct(const KP& p, f32x4 (&acc)[NI][MI], const int (&mrow)[MI], int nb, int fq,
                                                const f32x4 (&bpre)[NI], bool use_bpre, const float2* lnrow = nullptr) {
#pragma clang fp contract(off)
  constexpr int NP = NI / 2;               // paired tiles: 8 channels per lane
  constexpr bool ODD = NI % 2 == 1;
  if (p.ln_stats) ln_correct<NI, MI, true>(p, acc, mrow, nb, fq, lnrow);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = nb + lane_chan<NI, true>(i, fq);
    const f32x4 bv = use_bpre ? bpre[i] : ((p.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] += bv;
  }
  // one uniform branch per launch, the loops inside each case
#define SDEO_ACT_ALL(f)                                       \
  _Pragma("unroll") for (int i = 0; i < NI; ++i)              \
  _Pragma("unroll") for (int j = 0; j < MI; ++j)              \
  _Pragma("unroll") for (int t = 0; t < 4; ++t) acc[i][j][t] = f(acc[i][j][t]);
  switch (p.act) {
    case 1: SDEO_ACT_ALL(silu_f) break;
    case 2: SDEO_ACT_ALL(quick_gelu_f) break;
    case 4: SDEO_ACT_ALL(relu_f) break;
    case 5: SDEO_ACT_ALL(gelu_erf_f) break;
    default: break;
  }
#undef SDEO_ACT_ALL
  const float scale = p.scale;
  // residual loads of every block first: they depend on nothing above
  f16x8 resv[MI][NP > 0 ? NP : 1];
  f16x4 reso[MI];
#pragma unroll
  for (int j = 0; j < MI; ++j) {
#pragma unroll
    for (int q = 0; q < NP; ++q) resv[j][q] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    reso[j] = f16x4{0, 0, 0, 0};
  }
  if (p.res) {
#pragma unroll
    for (int j = 0; j < MI; ++j) {
      if (mrow[j] < 0) continue;
      const f16* rp = p.res + (size_t)res_row(p, mrow[j]) * p.ldres + nb;
#pragma unroll
      for (int q = 0; q < NP; ++q)
        if (nb + 32 * q + 8 * fq < p.N) resv[j][q] = *reinterpret_cast<const f16x8*>(rp + 32 * q + 8 * fq);
      if (ODD && nb + 16 * (NI - 1) + 4 * fq < p.N) reso[j] = *reinterpret_cast<const f16x4*>(rp + 16 * (NI - 1) + 4 * fq);
    }
  }
#pragma unroll
  for (int j = 0; j < MI; ++j) {
    const int m = mrow[j];
    if (m < 0) continue;
    f16* yp = p.y + (size_t)m * p.ldy + nb;
    float gs[NP > 0 ? NP : 1], gq[NP > 0 ? NP : 1];      // (sum, sumsq) of this lane's 8-channel group of pair q: group 4 q + fq of the strip
    f16x4 oo = f16x4{0, 0, 0, 0};                         // this lane's stored values of the unpaired tile
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      gs[q] = 0.f; gq[q] = 0.f;
      const int c = 32 * q + 8 * fq;
      if (nb + c >= p.N) continue;
      const f32x4 lo = acc[2 * q][j] * scale, hi = acc[2 * q + 1][j] * scale;
      f16x8 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        o[u] = (f16)(lo[u] + (float)resv[j][q][u]);
        o[4 + u] = (f16)(hi[u] + (float)resv[j][q][4 + u]);
      }
      *reinterpret_cast<f16x8*>(yp + c) = o;
      if (p.stats_out) {
#pragma unroll
        for (int u = 0; u < 8; ++u) { const float f = (float)o[u]; gs[q] += f; gq[q] += f * f; }
      }
    }
    if (ODD) {
      const int c = 16 * (NI - 1) + 4 * fq;
      if (nb + c < p.N) {
        const f32x4 v = acc[NI - 1][j] * scale;
        f16x4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = (f16)(v[u] + (float)reso[j][u]);
        *reinterpret_cast<f16x4*>(yp + c) = o;
        oo = o;
      }
    }
    if (p.stats_out) {
      // The four lanes fq = 0..3 with this frow hold the strip's columns of row m between them (and share m: they take this branch
      // together).  Every lane runs the gather, lane fq = 0 has the use of it.  Groups past N hold zeros, as in the staged path.
      const int l0 = threadIdx.x & 15;
      float ts = 0.f, tq = 0.f;
#pragma unroll
      for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int f = 0; f < 4; ++f) { ts += __shfl(gs[q], l0 + 16 * f, 64); tq += __shfl(gq[q], l0 + 16 * f, 64); }
      if (ODD) {         // the unpaired tile: groups of 8 channels span the lane pairs fq = (0, 1) and (2, 3)
        const uint2 raw = __builtin_bit_cast(uint2, oo);
        float v[16];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const uint2 r = make_uint2(__shfl(raw.x, l0 + 16 * f, 64), __shfl(raw.y, l0 + 16 * f, 64));
          const f16x4 h = __builtin_bit_cast(f16x4, r);
#pragma unroll
          for (int u = 0; u < 4; ++u) v[f * 4 + u] = (float)h[u];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          float s8 = 0.f, q8 = 0.f;
#pragma unroll
          for (int u = 0; u < 8; ++u) { s8 += v[g * 8 + u]; q8 += v[g * 8 + u] * v[g * 8 + u]; }
          ts += s8; tq += q8;
        }
      }
      if (fq == 0 && nb < p.N) reinterpret_cast<float2*>(p.stats_out)[(size_t)m * p.stats_ld + nb / TN] = make_float2(ts, tq);
    }
  }
}

// NB = 16-row blocks staged per LDS round trip (scratch >= NB * epilogue_scratch_bytes(TN) per wave).  With NB = 1 a wave tile of
// MI blocks costs MI dependent write -> read -> store chains; staging several blocks first issues their residual loads, LDS
// reads and global stores back to back (measured with tools/gemm_ablate.py: the epilogue is ~40 % of a many-tile short-K GEMM
// and of the order of a third of every ~8 us conv / GEMM launch).
template <int NI, int MI, int TN, int NB = 1, int EPI = EPI_STAGED>
__device__ __forceinline__ void epilogue_rows(const KP& p, f32x4 (&acc)[NI][MI], const int (&mrow)[MI], int nb, int fq, int z,
                                              const f32x4 (&bpre)[NI], bool use_bpre, char* scratch = nullptr,
                                              const float2* lnrow = nullptr) {
  static_assert(NB >= 1 && MI % NB == 0, "blocks per staging round");
  using Mode = EpiMode<EPI>;
  static_assert(EPI != EPI_GEGLU || (NI % 2 == 0 && TN % 32 == 0), "the GEGLU pair needs an even number of accumulator tiles per strip");
  if (Mode::wscale(p)) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nb + i * 16 + fq * 4;
      const f32x4 sc = n < p.N ? *reinterpret_cast<const f32x4*>(p.wscale + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < MI; ++j) acc[i][j] *= sc;
    }
  }
  if (Mode::ln(p)) ln_correct<NI, MI>(p, acc, mrow, nb, fq, lnrow);
  if constexpr (NI % 2 == 0 && TN % 32 == 0) {
    if (Mode::pair(p, scratch)) {
      // GEGLU pair epilogue (see below) through the same LDS transposition: value * gelu(gate) is formed in the accumulator
      // layout, staged as fp32 [16 rows][TN / 2] and stored in 16-byte pieces, TN bytes contiguous per row
      constexpr int TNO = TN / 2, ROWB = TNO * 4 + 16, G = TNO / 8, PASSES = (16 * G + 63) / 64;
      constexpr int BLOCKB = epilogue_scratch_bytes(TN);
      const int lane = threadIdx.x & 63, frow = lane & 15;
      f32x4 bias[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int n = nb + i * 16 + fq * 4;
        bias[i] = use_bpre ? bpre[i] : ((p.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f});
      }
      const int nbo = nb >> 1, No = p.N >> 1;
#pragma unroll
      for (int j0 = 0; j0 < MI; j0 += NB) {
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
          char* sc = scratch + jb * BLOCKB;
#pragma unroll
          for (int i = 0; i < NI; i += 2) {
            const f32x4 v = acc[i][j0 + jb] + bias[i], g = acc[i + 1][j0 + jb] + bias[i + 1];
            f32x4 o;
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = v[t] * gelu_erf_f(g[t]);
            *reinterpret_cast<f32x4*>(sc + frow * ROWB + ((i >> 1) * 16 + fq * 4) * 4) = o;
          }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
          const char* sc = scratch + jb * BLOCKB;
          const int m = mrow[j0 + jb];
#pragma unroll
          for (int t = 0; t < PASSES; ++t) {
            const int id = t * 64 + lane;
            const int r = id / G, n = nbo + (id - r * G) * 8;
            const int msrc = __shfl(m, r & 15, 64);
            if (id < 16 * G && n < No && msrc >= 0) {
              const char* src = sc + r * ROWB + (n - nbo) * 4;
              const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 16);
              f16x8 o;
#pragma unroll
              for (int u = 0; u < 4; ++u) { o[u] = (f16)lo[u]; o[4 + u] = (f16)hi[u]; }
              *reinterpret_cast<f16x8*>(p.y + (size_t)msrc * p.ldy + n) = o;
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
      return;
    }
  }
  if (Mode::block(p, scratch)) {
    constexpr int ROWB = TN * 4 + 16;            // odd multiple of 16 bytes: the 16 rows of a block start in different banks
    constexpr int G = TN / 8;                    // 8-channel groups per row
    constexpr int PASSES = (16 * G + 63) / 64;
    constexpr int BLOCKB = epilogue_scratch_bytes(TN);
    const int lane = threadIdx.x & 63, frow = lane & 15;
    // per-channel bias of this lane's tiles (zeros when absent), second-phase coordinates: the same for every block
    f32x4 bias[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nb + i * 16 + fq * 4;
      bias[i] = use_bpre ? bpre[i] : ((p.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f});
    }
    int rr[PASSES], nn[PASSES];
    bool live[PASSES];
#pragma unroll
    for (int t = 0; t < PASSES; ++t) {
      const int id = t * 64 + lane;
      rr[t] = id / G;
      nn[t] = nb + (id - rr[t] * G) * 8;
      live[t] = id < 16 * G && nn[t] < p.N;
    }
    const int mode = (p.bias2 ? 8 : 0) | p.act;   // act is 0, 1, 2, 4 or 5 here (3 = GEGLU never takes this path; 5 never comes with bias2)
    // GroupNorm partials (KP::gn_out): lane c (and c + 64 ...) sums column c of every stored block, read back from an fp16 copy of
    // the block in LDS -- two registers per column instead of sixteen per (row, vector) slot
    constexpr int GCH = (TN + 63) / 64;
    float gsum[GCH], gsq[GCH];
#pragma unroll
    for (int c = 0; c < GCH; ++c) { gsum[c] = 0.f; gsq[c] = 0.f; }
    stamp(p, 8);
#pragma unroll
    for (int j0 = 0; j0 < MI; j0 += NB) {
      // residual loads of these blocks first: they are independent of the staging
      int mm[NB][PASSES];
      f16x8 resv[NB][PASSES];
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        const int m = mrow[j0 + jb];
#pragma unroll
        for (int t = 0; t < PASSES; ++t) {
          const int msrc = __shfl(m, rr[t] & 15, 64);          // lane r (fq == 0) holds the row index of block row r
          mm[jb][t] = live[t] ? msrc : -1;
          resv[jb][t] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
      if (p.res) {
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
          for (int t = 0; t < PASSES; ++t)
            if (mm[jb][t] >= 0) resv[jb][t] = *reinterpret_cast<const f16x8*>(p.res + (size_t)res_row(p, mm[jb][t]) * p.ldres + nn[t]);
      }
      if (j0 == 0) stamp(p, 9);
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        const int m = mrow[j0 + jb];
        char* sc = scratch + jb * BLOCKB;
        f32x4 accj[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) accj[i] = acc[i][j0 + jb];
        if (dbg_on(p, 2048)) continue;          // ablation: no staging writes
        if constexpr (!Mode::generic) {
          stage_block<NI, TN, Mode::k_b2, Mode::k_act>(p, accj, bias, m, nb, fq, frow, sc);
        } else switch (mode) {
          case 0: stage_block<NI, TN, false, 0>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 1: stage_block<NI, TN, false, 1>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 2: stage_block<NI, TN, false, 2>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 4: stage_block<NI, TN, false, 4>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 5: stage_block<NI, TN, false, 5>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 8: stage_block<NI, TN, true, 0>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 9: stage_block<NI, TN, true, 1>(p, accj, bias, m, nb, fq, frow, sc); break;
          case 10: stage_block<NI, TN, true, 2>(p, accj, bias, m, nb, fq, frow, sc); break;
          default: stage_block<NI, TN, true, 4>(p, accj, bias, m, nb, fq, frow, sc); break;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (j0 == 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); stamp(p, 10); }
      if (dbg_on(p, 1024)) continue;            // ablation: staging only
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        const char* sc = scratch + jb * BLOCKB;
        float2* spart = reinterpret_cast<float2*>(scratch + jb * BLOCKB + 16 * ROWB);     // [16 rows][G] partial (sum, sumsq) of the stored values
#pragma unroll
        for (int t = 0; t < PASSES; ++t) {
          float ssum = 0.f, ssq = 0.f;
          if (mm[jb][t] >= 0) {
            const char* src = sc + rr[t] * ROWB + (nn[t] - nb) * 4;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 16);
            f16x8 o;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              o[u] = (f16)(lo[u] + (float)resv[jb][t][u]);
              o[4 + u] = (f16)(hi[u] + (float)resv[jb][t][4 + u]);
            }
            if (!dbg_on(p, 512)) *reinterpret_cast<f16x8*>(p.y + (size_t)mm[jb][t] * p.ldy + nn[t]) = o;
            if (Mode::stats(p)) {
#pragma unroll
              for (int u = 0; u < 8; ++u) { const float f = (float)o[u]; ssum += f; ssq += f * f; }
            }
            if (Mode::gn(p)) *reinterpret_cast<f16x8*>(scratch + jb * BLOCKB + 16 * ROWB + (rr[t] * TN + (nn[t] - nb)) * 2) = o;
          } else if (Mode::gn(p) && t * 64 + lane < 16 * G) {     // rows / columns past the problem count as zeros
            *reinterpret_cast<f16x8*>(scratch + jb * BLOCKB + 16 * ROWB + (rr[t] * TN + (nn[t] - nb)) * 2) = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
          }
          if (Mode::stats(p) && t * 64 + lane < 16 * G) spart[t * 64 + lane] = make_float2(ssum, ssq);     // index = row * G + group
        }
      }
      if (Mode::gn(p)) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
          const f16* blk = reinterpret_cast<const f16*>(scratch + jb * BLOCKB + 16 * ROWB);
#pragma unroll
          for (int c = 0; c < GCH; ++c) {
            const int col = c * 64 + lane;
            if (col < TN) {
#pragma unroll
              for (int r = 0; r < 16; ++r) { const float f = (float)blk[r * TN + col]; gsum[c] += f; gsq[c] += f * f; }
            }
          }
        }
      }
      if (Mode::stats(p)) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
          const int m = mrow[j0 + jb];
          const float2* spart = reinterpret_cast<const float2*>(scratch + jb * BLOCKB + 16 * ROWB);
          if (lane < 16 && m >= 0 && nb < p.N) {   // lanes 0..15 have fq == 0 and frow == lane: `m` is the row index of block row `lane`;
                                                   // a strip wholly past N (tile padding) has no slot in the statistics row
            float ts = 0.f, tq = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) { const float2 v = spart[lane * G + g]; ts += v.x; tq += v.y; }
            reinterpret_cast<float2*>(p.stats_out)[(size_t)m * p.stats_ld + nb / TN] = make_float2(ts, tq);
          }
        }
      }
      if (j0 == 0) stamp(p, 11);
      __builtin_amdgcn_wave_barrier();        // the next round overwrites the scratch rows
    }
    if (Mode::gn(p)) {      // this wave's per-column (sum, sumsq) at the start of its scratch: gn_partials_finish combines the waves
#pragma unroll
      for (int c = 0; c < GCH; ++c)
        if (c * 64 + lane < TN) reinterpret_cast<float2*>(scratch)[c * 64 + lane] = make_float2(gsum[c], gsq[c]);
    }
    stamp(p, 12);
    return;
  }
#pragma unroll
  for (int j = 0; j < MI; ++j) {
    const int m = mrow[j];
    if (m < 0) continue;
    if constexpr (Mode::generic && NI % 2 == 0 && TN % 32 == 0) {
      if (p.act == 3) {
        // GEGLU (`attention.py:49-56`) fused into ff.net.0.proj: the weight rows were interleaved at load time in blocks of
        // 16 (block 2q = value channels 16q..16q+15, block 2q+1 = their gates), so accumulator tiles i and i+1 hold, in the
        // same lane and register, a value and its gate.  Output column = value channel; ldy counts N/2 columns.
#pragma unroll
        for (int i = 0; i < NI; i += 2) {
          const int n = nb + i * 16 + fq * 4;
          if (n >= p.N) continue;
          f32x4 v = acc[i][j], g = acc[i + 1][j];
          if (p.bias) {
            if (use_bpre) { v += bpre[i]; g += bpre[i + 1]; }
            else { v += *reinterpret_cast<const f32x4*>(p.bias + n); g += *reinterpret_cast<const f32x4*>(p.bias + n + 16); }
          }
          f16x4 o;
#pragma unroll
          for (int t = 0; t < 4; ++t) o[t] = (f16)(v[t] * gelu_erf_f(g[t]));
          *reinterpret_cast<f16x4*>(p.y + (size_t)m * p.ldy + ((nb + i * 16) >> 1) + fq * 4) = o;
        }
        continue;
      }
    }
    const int b = p.bias2 ? m / p.HoWo : 0;
    float ssum = 0.f, ssq = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nb + i * 16 + fq * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (Mode::split(p)) {
        *reinterpret_cast<f32x4*>(p.ws + ((size_t)z * p.M + m) * p.N + n) = v;
        continue;
      }
      if (p.bias) {
        if (p.bias_per_row) v += p.bias[m];
        else if (use_bpre) v += bpre[i];
        else v += *reinterpret_cast<const f32x4*>(p.bias + n);
      }
      if (p.bias2) v += *reinterpret_cast<const f32x4*>(p.bias2 + (size_t)b * p.ld_bias2 + n);
      if (p.act == 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = silu_f(v[t]);
      } else if (p.act == 2) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = quick_gelu_f(v[t]);
      } else if (p.act == 4) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
      } else if (p.act == 5) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = gelu_erf_f(v[t]);
      }
      v *= p.scale;
      if (p.res) {
        const f16x4 r = *reinterpret_cast<const f16x4*>(p.res + (size_t)res_row(p, m) * p.ldres + n);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] += (float)r[t];
      }
      if (p.y32) {
        *reinterpret_cast<f32x4*>(p.y32 + (size_t)m * p.ldy + n) = v;
      } else {
        f16x4 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = (f16)v[t];
        *reinterpret_cast<f16x4*>(p.y + (size_t)m * p.ldy + n) = o;
        if (p.stats_out) {
#pragma unroll
          for (int t = 0; t < 4; ++t) { const float f = (float)o[t]; ssum += f; ssq += f * f; }
        }
      }
    }
    if (Mode::stats(p) && !Mode::split(p)) {
      // the four lanes fq = 0..3 with this frow hold the strip's columns of row m between them
      ssum += __shfl_xor(ssum, 16, 64); ssq += __shfl_xor(ssq, 16, 64);
      ssum += __shfl_xor(ssum, 32, 64); ssq += __shfl_xor(ssq, 32, 64);
      if (fq == 0 && nb < p.N) reinterpret_cast<float2*>(p.stats_out)[(size_t)m * p.stats_ld + nb / TN] = make_float2(ssum, ssq);
    }
  }
}

// implicit-GEMM tiles: accumulator tile (i, j) of wave (wm, wn) is output row m0 + wm*TM + j*16 + frow
template <int NI, int MI, int TM, int TN, int NB = 1>
__device__ __forceinline__ void epilogue(const KP& p, f32x4 (&acc)[NI][MI], int m0, int n0, int wm, int wn, int frow, int fq, int z,
                                         const f32x4 (&bpre)[NI], bool use_bpre, char* scratch = nullptr,
                                         const float2* lnrow = nullptr) {
  int mrow[MI];
#pragma unroll
  for (int j = 0; j < MI; ++j) {
    const int m = m0 + wm * TM + j * 16 + frow;
    mrow[j] = m < p.M ? m : -1;
  }
  epilogue_rows<NI, MI, TN, NB>(p, acc, mrow, n0 + wn * TN, fq, z, bpre, use_bpre, scratch, lnrow);
}

// GroupNorm partials, second half (KP::gn_out).  After epilogue_rows every wave's scratch starts with the per-column (sum, sumsq)
// of the rows it stored.  Called by ONE wave per TN-wide strip after a workgroup barrier: sums the NW waves that share the strip
// (scratch bases `base + w * stride`), then the gn_cpg columns of each group, and writes entry (image b, tile slot, group).
template <int TN, int NW>
__device__ __forceinline__ void gn_partials_finish(const KP& p, char* base, int stride, int lane, int b, int slot, int nb) {
  constexpr int GCH = (TN + 63) / 64;
  float2* tot = reinterpret_cast<float2*>(base) + TN;          // behind wave 0's own column sums
#pragma unroll
  for (int c = 0; c < GCH; ++c) {
    const int col = c * 64 + lane;
    if (col < TN) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) { const float2 v = reinterpret_cast<const float2*>(base + w * stride)[col]; s += v.x; q += v.y; }
      tot[col] = make_float2(s, q);
    }
  }
  __builtin_amdgcn_wave_barrier();
  const int cpg = p.gn_cpg;
  const int g = (nb / cpg) + lane;                             // strips start on a group boundary (host-checked)
  if (lane * cpg < TN && nb + lane * cpg < p.N) {
    float s = 0.f, q = 0.f;
    for (int k = 0; k < cpg; ++k) { const float2 v = tot[lane * cpg + k]; s += v.x; q += v.y; }
    reinterpret_cast<float2*>(p.gn_out)[((size_t)b * p.gn_slots + slot) * p.gn_groups + g] = make_float2(s, q);
  }
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (observed, speed only), so give each
// XCD a contiguous run of tiles (bijective for any tile count): neighbouring tiles share a weight panel in L2.
__device__ __forceinline__ int xcd_remap(int wg, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = wg & 7, idx = wg >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// compile-time loop (the LDS offsets of the inline-asm fragment reads must be immediates)
template <int N, typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl<N>(f, std::make_integer_sequence<int, N>{});
}
template <int OFF>
__device__ __forceinline__ void lds_read128(f16x8& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

// a weight fragment as it sits in LDS: 16 bytes of fp16 or 8 bytes of fp8
template <int OFF>
__device__ __forceinline__ void lds_read_w(f16x8& dst, unsigned addr) { lds_read128<OFF>(dst, addr); }
template <int OFF>
__device__ __forceinline__ void lds_read_w(uint2& dst, unsigned addr) {
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}


// One row of the conv / GEMM tile table (conv_gemm.hip: kTiles), the only description of a tile: the planner, the launcher, the
// autotuner and sdeo_debug_tile_info all read it.  A tile's index in that table is public (tuned_plans_gfx950.json, the force hook).
enum TileKind { TK_DMA, TK_GENERIC, TK_HALO };
// CAP_LIGHT: four-wave workgroups (no loader waves); CAP_GROUPED: one barrier per group of `kpb` K-steps; CAP_W8 / CAP_MX: an
// fp8-weight / block-scaled-fp8 instantiation exists; CAP_HALO: kind == TK_HALO.  (the bit values are those of sdeo_debug_tile_info)
enum TileCap { CAP_LIGHT = 1, CAP_GROUPED = 2, CAP_W8 = 4, CAP_MX = 8, CAP_HALO = 16 };
typedef int (*TileLaunch)(const KP& kp, int tiles, hipStream_t stream);      // one launch of tiles x 1 x kp.splitk workgroups
struct TileCfg {
  int bm, bn, bk, stages;      // TK_HALO: bm = ph * pw pixels of one image, stages = weight ring slots
  TileKind kind;
  int caps, kpb;
  int ph, pw;                  // TK_HALO: the patch of output pixels a workgroup owns
  const char* name;            // the instantiation, as profiles and bench.py --full key on it
  TileLaunch plain, ups, w8, mx;    // fp16 / folded nearest-x2 upsample / fp8 weights / block-scaled fp8; null where none exists
  TileLaunch epi[EPI_KINDS];        // the plain fp16 instantiation per epilogue kind (EpiKind): [EPI_STAGED] = plain, the others null where
                                    // the row has no such kind
};
// the kinds a row instantiates besides EPI_STAGED, as a mask in the row's description (dma_tile / halo_tile)
constexpr int K_D = 1 << EPI_DIRECT, K_SK = 1 << EPI_SPLITK, K_GG = 1 << EPI_GEGLU, K_GN = 1 << EPI_GN, K_GNB = 1 << EPI_GN_B2;
// the halo-reuse 3x3 kernel's rows (conv_halo.hip: 17 variants), which kTiles takes in by position
const TileCfg& halo_row(int variant);

}  // namespace sdeo
