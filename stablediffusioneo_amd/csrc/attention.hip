// Fused attention for gfx950:  O = softmax(Q K^T * scale) V, scores never leave registers.
//
// Replaces CrossAttention.forward's einsum / softmax / einsum (`ldm/modules/attention.py:227-249`), which
// materialises a (B*heads, Tq, Tk) fp32 score tensor (1.07 GB at 512x512).  Numerics kept from
// the reference: q.k^T accumulated in fp32 and scaled in fp32 (`:230-233`), softmax in fp32.
//
// Structure (per workgroup: 4 waves x 32 query rows, one (batch, head); key tiles of 64 streamed through LDS):
//  * S^T = K Q^T on v_mfma_f32_32x32x16_f16 with K as the A operand: the accumulator then has the query on
//    the lane and 16 keys in registers, so the row max / row sum of the online softmax are in-lane
//    reductions plus ONE exchange with lane^32.
//  * P^T stays in registers: registers 8s..8s+7 of the score accumulator, packed to fp16, ARE the B operand
//    of the next MFMA (O^T += V^T P^T) with no LDS round trip.  The k-order inside a step is permuted
//    (element j of lane-half h is key 16s + 8(j>>2) + 4h + (j&3)); the V^T fragment is fetched with two
//    8-byte LDS reads at exactly those key offsets.
//  * V arrives row-major ([B*TkS][heads*d], i.e. a column block of the fused q/k/v projection) and is staged
//    row-major in LDS ([key][d]); the V^T fragments of the O^T += V^T P^T MFMA are fetched with the transposing
//    LDS read ds_read_b64_tr_b16 (four keys of one channel per lane), so no transposed copy of V exists anywhere.
//    The key-row stride of the LDS tile is 64 or 192 bytes mod 256: the four rows a 32-lane half reads then
//    cover all 64 banks once.
//  * head dims 40 / 80 / 160 (and 8..64 for the reduced test config): QK^T pads d to a multiple of 16 with
//    zero chunks in LDS, PV pads to a multiple of 32 rows.
//  * K / V tiles are register-staged and double-buffered: the next tile's global loads are issued before
//    the MFMA phase and written to the other LDS buffer after it.
#include <cmath>
#include <type_traits>

#include "kernels.h"

namespace sdeo {

typedef __fp16 h16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// bytes per key of the row-major V tile in LDS (see the file comment)
constexpr int attn_vrow(int dt) { return dt == 1 ? 64 : (dt <= 3 ? 192 : 320); }

struct AP {
  f16* o;
  const f16* q;
  const f16* k;
  const f16* v;
  int ldo, ldq, ldk, ldv;
  int H, Tq, Tk, TkS, TkSv, d;
  float scale_log2;
  int causal;        // 1: key j is visible to query t only when j <= t (CLIP text transformer)
  int qB;            // batches of Q: batch b reads the queries of batch b - qB when b >= qB (AttnArgs::qB)
};

struct AP2 { AP k[1]; };

// Second key segment of the two-segment kernels (attention2_kernel): one more tile of at most 64 keys with a softmax of its own,
// O = softmax(Q K^T s) V + w * softmax(Q K2^T s) V2  (the image-prompt term of a decoupled cross-attention)
struct APX {
  const f16* k;
  const f16* v;
  int ldk, ldv;
  int Tk, TkS, TkSv;  // 1 <= Tk <= 64
  float w;
};

struct AP3 { AP k[1]; APX x; };

// lane ^ 32 exchange on the VALU (gfx950 v_permlane32_swap): after the swap the pair (lo, hi) holds the value of lanes 0..31 and
// of lanes 32..63 in every lane, so a reduction over the two halves needs no LDS round trip (ds_bpermute) in the softmax chain.
// Inline asm, not __builtin_amdgcn_permlane32_swap: hipcc 7.2 maps both results of the builtin to ONE register for float users
// (r0 + r1 is emitted as v_add v1, v1, v1).  The s_nop covers the VALU-write -> permlane read hazard the compiler cannot see.
__device__ __forceinline__ void swap32(float v, float& lo, float& hi) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  lo = a;
  hi = b;
}
// v_max_f32 without the canonicalising v_max v, v, v the compiler puts in front of fmaxf on values it cannot prove quiet
// (results of inline asm, loop-carried state); the operands here are never signalling NaNs
__device__ __forceinline__ float max_raw(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float xor32_max(float v) {
  float lo, hi;
  swap32(v, lo, hi);
  return max_raw(lo, hi);
}
__device__ __forceinline__ float xor32_sum(float v) {
  float lo, hi;
  swap32(v, lo, hi);
  return lo + hi;
}

// The two roundings of the two-segment store (attention_body.h).  attention_kernel's store is `(f16)(o * inv)` on four neighbouring
// accumulator registers, and the compiler emits it, in every KS = 1 instantiation, as v_fma_mixlo_f16 for elements 0 and 3 of the quad
// (the product rounded ONCE, straight to fp16) and v_pk_mul_f32 + v_cvt_pk_f16_f32 for elements 1 and 2 (rounded to fp32, then to
// fp16).  The two-segment store forms o1 * inv1 + t per element and has to give those bits when t = 0 (weight 0 is the one-segment
// kernel, tests/test_attention2_gpu.py), so it asks for each rounding by name instead of leaving the choice to the compiler:
//   fma_f16_once   fp16(a * b + c), one fused multiply-add in fp32 precision rounded once
//   fma_f16_twice  fp16(fp32(a * b + c)); the empty asm keeps the two roundings apart
__device__ __forceinline__ f16 fma_f16_once(float a, float b, float c) {
  unsigned r;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return __builtin_bit_cast(f16, (unsigned short)r);
}
__device__ __forceinline__ f16 fma_f16_twice(float a, float b, float c) {
  float r = fmaf(a, b, c);
  asm("" : "+v"(r));
  return (f16)r;
}

// KS = 1: four waves, each owning 32 queries and walking all keys.  KS = 2 ("key split"): eight waves, the two waves of a
// pair own the same 32 queries and each takes one 32-key half of every staged tile, so the serial per-tile chain
// (QK^T -> max -> exp -> PV) per wave halves and twice as many waves hide it; the two partial (m, l, O) states are merged
// through LDS at the end.  Reduction order is fixed (half 0 then half 1), so results stay deterministic.
// MPAD (head dims with a free K-dim slot, d % 16 == 8: d = 40): the softmax's per-score fma moves into the QK^T MFMA.  Q is scaled
// by scale * log2 e once (fp16), the K tile's pad channel d holds 1, and Q's pad channel d holds -m, the row's running reference
// (kept as an fp16-exact value), so the MFMA delivers  s * scale * log2 e - m  and the inner loop is max / exp / cvt only.
// QB: 32-query blocks per workgroup (4: 128 queries; 2: 64 queries, twice the workgroups, each staging the K / V tiles for half as
// many queries but with only QB * KS waves behind one barrier).
template <int D16, int KS, bool MPAD, int QB = 4>
__global__ __launch_bounds__(64 * QB * KS, (KS == 2 ? (D16 <= 4 ? 4 : 2) : (D16 <= 2 ? 4 : (D16 <= 5 ? 2 : 1))))
void attention_kernel(const AP2 pp) {
  kernarg_warm<sizeof(AP2)>();
  // the whole parameter block in one batch, pinned in SGPRs (otherwise ~5 dependent s_load round trips before the first Q load);
  // blockIdx.y is always 0 (one problem per launch)
  AP pl = pp.k[0];
  // (integers / floats only: a pointer that has been through the asm loses its address space and its accesses become flat_ ones)
  asm volatile("" : "+s"(pl.ldo), "+s"(pl.ldq), "+s"(pl.ldk), "+s"(pl.ldv), "+s"(pl.H),
               "+s"(pl.Tq), "+s"(pl.Tk), "+s"(pl.TkS), "+s"(pl.TkSv), "+s"(pl.d), "+s"(pl.scale_log2), "+s"(pl.causal), "+s"(pl.qB));
  const AP& p = pl;
  // The body is shared with attention2_kernel below as TEXT (attention_body.h).  A shared __device__ function was tried first: inlined
  // into this kernel it moved the instruction schedule of all 27 instantiations of this kernel, and they (with the two wide kernels: 29) are to stay as they are, instruction for
  // instruction.  Here SEG2 is false and x a dummy: every `if constexpr (SEG2)` of the body is discarded.
  constexpr bool SEG2 = false;
  constexpr APX x{};
#include "attention_body.h"
}

// The two-segment form of attention_kernel<D16, 1, MPAD, 4> (SEG2 in attention_body.h):
//   O = softmax(Q K^T s) V + x.w * softmax(Q K2^T s) V2
// The keys are the Tk keys of k / v, tiles 0 .. ntiles - 1, followed by ONE tile of x.Tk <= 64 keys of x.k / x.v, tile `ntiles` of the
// same pipeline: prefetch, LDS stages and register sets alternate straight through, and the "deep" class again runs one fully masked
// tile when the count INCLUDING that tile is odd.  In front of that tile the first softmax is closed: O and 1 / l are parked in fp32
// registers and (m, l, O) start afresh; the output is fp16(O1 / l1 + x.w * O2 / l2), rounded once.
// The parked O1 costs 16 DT registers: D16 = 5 (224 VGPRs in one segment) no longer fits two workgroups per CU and is built for one,
// as D16 > 5 is.
template <int D16, bool MPAD>
__global__ __launch_bounds__(256, (D16 <= 2 ? 4 : (D16 <= 4 ? 2 : 1)))
void attention2_kernel(const AP3 pp) {
  kernarg_warm<sizeof(AP3)>();
  AP pl = pp.k[0];
  APX px = pp.x;
  asm volatile("" : "+s"(pl.ldo), "+s"(pl.ldq), "+s"(pl.ldk), "+s"(pl.ldv), "+s"(pl.H),
               "+s"(pl.Tq), "+s"(pl.Tk), "+s"(pl.TkS), "+s"(pl.TkSv), "+s"(pl.d), "+s"(pl.scale_log2), "+s"(pl.causal), "+s"(pl.qB));
  asm volatile("" : "+s"(px.ldk), "+s"(px.ldv), "+s"(px.Tk), "+s"(px.TkS), "+s"(px.TkSv), "+s"(px.w));
  const AP& p = pl;
  const APX& x = px;
  constexpr bool SEG2 = true;
  constexpr int KS = 1, QB = 4;
#include "attention_body.h"
}

// ------------------------------------------------------------------------------------------------
// Wide heads (d = 256 / 512: the VAE AttnBlock, `ldm/modules/diffusionmodules/model.py:179-203`, one head of 512 channels).
// 32 queries x d fp32 of O do not fit one wave's registers, so the four waves of a workgroup share ONE block of 32 queries and
// split the CHANNELS: wave w owns channels [w*DS, (w+1)*DS).  Per 32-key tile each wave forms the partial S^T = K[:, slice] Q[:, slice]^T
// of its slice, the four partials are summed through LDS in a fixed order (identical full scores in every wave, deterministic),
// every wave runs the same online softmax on them (redundant VALU work, but no second exchange), and multiplies P into ITS slice
// of V: O^T[slice] += V[:, slice]^T P^T.  MFMA layouts, the in-register P^T operand and the transposing V reads are those of
// attention_kernel above.  K / V tiles: 32 keys x d, register-staged, double-buffered in LDS.
// ------------------------------------------------------------------------------------------------
template <int DS>
__global__ __launch_bounds__(256, 1) void attention_wide_kernel(const AP p) {
  constexpr int D = 4 * DS;                                   // head dim
  constexpr int KS16 = DS / 16;                               // QK^T k-steps per wave (even)
  constexpr int DT = DS / 32;                                 // 32-row tiles of O^T per wave
  constexpr int KROW = D * 2 + 16;                            // K tile row bytes: odd multiple of 16
  constexpr int VROW = D * 2 + 64;                            // V tile row bytes: 64 (mod 256), see attn_vrow
  constexpr int KBYTES = 32 * KROW, VBYTES = 32 * VROW, STAGE = KBYTES + VBYTES;
  constexpr int CH = D / 8;                                   // 16-byte chunks per row
  constexpr int PASS = 32 * CH / 256;                         // chunks per thread per tile (K and V each)
  static_assert(KROW % 32 == 16 && VROW % 256 == 64 && (32 * CH) % 256 == 0, "tile geometry");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* xch = smem + 2 * STAGE;                               // partial-score exchange: [wave][4][lane] f32x4 (16 KB)

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 31, lh = lane >> 5;
  const int qtiles = (p.Tq + 31) >> 5;
  const int bh = blockIdx.x / qtiles;
  const int b = bh / p.H, h = bh - b * p.H;
  const int q0 = (blockIdx.x - bh * qtiles) * 32;
  const int qrow = q0 + lq;
  const bool qvalid = qrow < p.Tq;
  const int c0 = wave * DS;                                   // first channel of this wave's slice

  f16x8 qf[KS16];
  {
    const f16* qp = p.q + ((size_t)(b >= p.qB ? b - p.qB : b) * p.Tq + (qvalid ? qrow : 0)) * p.ldq + h * D + c0;
#pragma unroll
    for (int ks = 0; ks < KS16; ++ks)
      qf[ks] = *reinterpret_cast<const f16x8*>(qp + (ks * 2 + lh) * 8);       // row 0 for queries past Tq: never stored
  }

  const f16* kbase = p.k + (size_t)b * p.TkS * p.ldk + h * D;
  const f16* vbase = p.v + (size_t)b * p.TkSv * p.ldv + h * D;
  // loop-invariant scalars pinned in SGPRs (see attention_kernel)
  float sl2 = p.scale_log2;
  int Tk = p.Tk;
  unsigned ldk2 = (unsigned)p.ldk * 2u, ldv2 = (unsigned)p.ldv * 2u;
  asm volatile("" : "+s"(sl2), "+s"(Tk), "+s"(ldk2), "+s"(ldv2));
  const int ntiles = (Tk + 31) / 32;
  const int last_key = Tk - 1;
  // K / V tiles are register-staged two tiles ahead (two register sets): with one workgroup per CU and one wave per SIMD nothing
  // else hides a global round trip, and one tile of compute (~1 us) is shorter than it (measured: 2.7 us per tile with the
  // loads issued one tile ahead)
  f16x8 kr[2][PASS], vr[2][PASS];
  auto load_tile = [&](auto SET, int kt) {
    constexpr int rs = SET.value;
#pragma unroll
    for (int i = 0; i < PASS; ++i) {
      const int it = tid + i * 256;
      const int row = it / CH, c = it - row * CH;
      // unconditional, counted loads (see attention_kernel): rows >= Tk re-read row Tk - 1, their keys are masked (P = 0, V finite)
      const unsigned key = (unsigned)min(kt * 32 + row, last_key);
      kr[rs][i] = *reinterpret_cast<const f16x8*>(reinterpret_cast<const char*>(kbase) + (__umul24(key, ldk2) + (unsigned)c * 16u));
      vr[rs][i] = *reinterpret_cast<const f16x8*>(reinterpret_cast<const char*>(vbase) + (__umul24(key, ldv2) + (unsigned)c * 16u));
    }
  };
  auto store_tile = [&](auto SET, int stage) {
    constexpr int rs = SET.value;
    char* ks_ = smem + stage * STAGE;
    char* vs_ = ks_ + KBYTES;
#pragma unroll
    for (int i = 0; i < PASS; ++i) {
      const int it = tid + i * 256;
      const int row = it / CH, c = it - row * CH;
      *reinterpret_cast<f16x8*>(ks_ + row * KROW + c * 16) = kr[rs][i];
      *reinterpret_cast<f16x8*>(vs_ + row * VROW + c * 16) = vr[rs][i];
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  load_tile(S0{}, 0);
  load_tile(S1{}, 1);                                 // set 1 carries the odd tiles, set 0 the even ones
  store_tile(S0{}, 0);
#pragma unroll
  for (int ks = 0; ks < KS16; ++ks) asm volatile("" : "+v"(qf[ks]));     // Q's wait in front of the loop (see attention_kernel)
  load_tile(S0{}, 2);
  __syncthreads();

  auto compute = [&](int kt, int cur) __attribute__((always_inline)) {
    const char* ks_ = smem + cur * STAGE;
    const char* vs_ = ks_ + KBYTES;

    // ---- partial S^T over this wave's channel slice
    f32x16 s, s1;                                     // two accumulation chains: a 32x32x16 MFMA has 16 passes of latency
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < KS16; ks += 2) {
      const f16x8 kf0 = *reinterpret_cast<const f16x8*>(ks_ + lq * KROW + (c0 / 8 + ks * 2 + lh) * 16);
      const f16x8 kf1 = *reinterpret_cast<const f16x8*>(ks_ + lq * KROW + (c0 / 8 + ks * 2 + 2 + lh) * 16);
      s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf0, qf[ks], s, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf1, qf[ks + 1], s1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] += s1[r];
    {
      f32x4* dst = reinterpret_cast<f32x4*>(xch) + wave * 256 + lane;       // [wave][4 register groups][lane]: lane-contiguous
#pragma unroll
      for (int g = 0; g < 4; ++g) dst[g * 64] = f32x4{s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]};
    }
    __syncthreads();
    // ---- full scores: the four partials in a fixed order (every wave computes the same bits)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const f32x4* src = reinterpret_cast<const f32x4*>(xch) + w * 256 + lane;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = src[g * 64];
        s[4 * g] += v[0]; s[4 * g + 1] += v[1]; s[4 * g + 2] += v[2]; s[4 * g + 3] += v[3];
      }
    }
    // ---- online softmax (base 2); key of s[r] = kt*32 + (r&3) + 8*(r>>2) + 4*lh
    float mx = -INFINITY;
    if ((kt + 1) * 32 > Tk) {                         // one uniform branch per tile
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh >= Tk) s[r] = -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = xor32_max(mx) * sl2;
    // lazy rescale of the running reference (threshold 2^8, see attention_kernel): O is DT x 16 registers per wave here, and the
    // eager form multiplied all of them by alpha on every tile
    if (__any(mx > m_run + 8.0f)) {                   // tile 0 always holds key 0: m_run becomes finite there
      const float m_new = max_raw(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
      m_run = m_new;
    }
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], sl2, -m_run));
      s[r] = pv;
      rs += pv;
    }
    l_run += xor32_sum(rs);
    // ---- O^T[slice] += V[:, slice]^T P^T
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f16x8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (f16)s[8 * st + j];
      const char* vblk = vs_ + (16 * st + 4 * lh + ((lane & 15) >> 2)) * VROW + (c0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        typedef __attribute__((address_space(3))) h16x4* lds_h4;
        const h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4)(vblk + t * 64));
        const h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4)(vblk + t * 64 + 8 * VROW));
        const f16x8 vf = __builtin_shufflevector(__builtin_bit_cast(f16x4, lo), __builtin_bit_cast(f16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[t], 0, 0, 0);
      }
    }
  };
  // at the end of a tile the NEXT tile (loaded two iterations ago) goes from registers to the other LDS buffer and the freed
  // register set takes the loads of the tile after that; the closing barrier also frees the exchange area
  for (int kt = 0; kt < ntiles; kt += 2) {            // an odd tile count runs one fully masked tile (P = 0) at the end
    compute(kt, 0);
    store_tile(S1{}, 1);
    load_tile(S1{}, kt + 3);
    __syncthreads();
    compute(kt + 1, 1);
    store_tile(S0{}, 0);
    load_tile(S0{}, kt + 4);
    __syncthreads();
  }

  if (qvalid) {
    const float inv = 1.0f / l_run;
    f16* op = p.o + ((size_t)b * p.Tq + qrow) * p.ldo + h * D + c0;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f16x4 ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = (f16)(o[t][4 * g + j] * inv);
        *reinterpret_cast<f16x4*>(op + t * 32 + 8 * g + 4 * lh) = ov;
      }
  }
}

template <int DS>
static int launch_attn_wide(const AP& ap, int B, hipStream_t stream) {
  constexpr int D = 4 * DS;
  constexpr int smem = 2 * (32 * (D * 2 + 16) + 32 * (D * 2 + 64)) + 4 * 64 * 16 * 4;
  static_assert(smem <= 160 * 1024, "LDS");
  static DeviceOnce attr_done;
  if (attr_done.need()) {
    SDEO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_wide_kernel<DS>), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_done.mark();
  }
  hipLaunchKernelGGL((attention_wide_kernel<DS>), dim3(cdiv(ap.Tq, 32) * B * ap.H), dim3(256), smem, stream, ap);
  SDEO_HIP(hipGetLastError());
  return 0;
}

template <int D16, int KS, bool MPAD, int QB = 4>
static int launch_attn_ks(const AP2& ap2, int count, int B, hipStream_t stream) {
  const AP& ap = ap2.k[0];
  constexpr int DT = (D16 + 1) / 2;
  constexpr int KROW = D16 * 32 + ((D16 * 2) % 2 == 0 ? 16 : 0);
  constexpr int stage2 = 2 * (64 * KROW + 64 * attn_vrow(DT));
  constexpr int merge = KS == 2 ? QB * (2 + DT * 16) * 64 * 4 : 0;    // LDS of the key-half merge
  constexpr int smem = stage2 > merge ? stage2 : merge;
  static DeviceOnce attr_done;
  if (attr_done.need()) {
    SDEO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_kernel<D16, KS, MPAD, QB>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_done.mark();
  }
  dim3 grid(cdiv(ap.Tq, 32 * QB) * B * ap.H, count);
  hipLaunchKernelGGL((attention_kernel<D16, KS, MPAD, QB>), grid, dim3(64 * QB * KS), smem, stream, ap2);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// Which kernel a problem runs.  attn_select is the ONLY place that decides it: the launcher switches on the value it returns and
// attention_kernel_name (sdeo_debug_attention_kernel_name) formats it, so the name a test is told is the kernel a launch runs.
struct AttnForm {
  int wide;                  // DS of attention_wide_kernel<DS> (d = 4 DS), or 0: attention_kernel<d16, ks, mpad, qb>
  int d16, ks, mpad, qb;
};

// Host only (no device call).  Depends on nothing but the shape: operands and strides are attn_prepare's.
static int attn_select(AttnForm& f, int B, int H, int Tq, int Tk, int d, int causal) {
  SDEO_CHECK(B > 0 && H > 0 && Tq > 0 && Tk > 0, "attention: bad sizes B=%d H=%d Tq=%d Tk=%d", B, H, Tq, Tk);
  f = AttnForm{0, 0, 1, 0, 4};
  if (d == 256 || d == 512) {
    SDEO_CHECK(!causal, "attention: causal masking is not built for head dim %d", d);
    f.wide = d / 4;
    return 0;
  }
  const int d16 = cdiv(d, 16);
  // instantiated k-step counts: 1..6, 8, 10 (7 and 9, d = 104 / 112 / 136 / 144, are not)
  SDEO_CHECK(d % 8 == 0 && d >= 8 && d <= 160 && d16 != 7 && d16 != 9,
             "attention: head dim %d unsupported (8..96 in steps of 8, 120, 128, 152, 160, 256, 512)", d);
  SDEO_CHECK(!causal || Tq == Tk, "attention: causal needs Tq == Tk (got %d, %d)", Tq, Tk);
  f.d16 = d16;
  if (d16 > 5) return 0;
  // a free K-dim slot right after the head's channels (d = 8, 24, 40, 56, 72): the reference-in-the-pad form
  static const bool mpad_on = [] { const char* e = getenv("SDEO_ATTN_MPAD"); return !e || atoi(e) != 0; }();
  f.mpad = mpad_on && d % 16 == 8;
  // key split pays when there are enough keys for the serial chain to dominate and the head dim keeps the merge small
  static const int ks_forced = [] { const char* e = getenv("SDEO_ATTN_KS"); return e ? atoi(e) : 0; }();
  f.ks = (ks_forced ? ks_forced == 2 : Tk >= 128) ? 2 : 1;
  if (f.ks == 2 && (d16 == 3 || d16 == 5)) {
    // 64-query workgroups where 128-query ones leave CUs empty (T = 1024 on 16 (batch, head) pairs: 128 workgroups on 256 CUs;
    // measured 19.3 -> 17.2 us at d = 80); with the chip already full they lose (T = 4096: 71 -> 95 us: twice the staging per
    // query, one prefetch set).  SDEO_ATTN_QB = 2 / 4 forces one form (measurement).  Instantiated for d = 40 / 80.
    static const int qb_forced = [] { const char* e = getenv("SDEO_ATTN_QB"); return e ? atoi(e) : 0; }();
    const bool small_grid = cdiv(Tq, 128) * B * H < 256;
    if (qb_forced ? qb_forced == 2 : small_grid) f.qb = 2;
  }
  return 0;
}

const char* attention_kernel_name(int B, int H, int Tq, int Tk, int d, int causal) {
  static thread_local char name[48];
  AttnForm f;
  if (attn_select(f, B, H, Tq, Tk, d, causal)) return nullptr;
  if (f.wide) snprintf(name, sizeof(name), "attention_wide_kernel<%d>", f.wide);
  else snprintf(name, sizeof(name), "attention_kernel<%d,%d,%s,%d>", f.d16, f.ks, f.mpad ? "true" : "false", f.qb);
  return name;
}

template <int D16>
static int launch_attn(const AttnForm& f, const AP2& ap, int count, int B, hipStream_t stream) {
  if constexpr (D16 <= 5) {
    if (f.ks == 2) {
      if constexpr (D16 == 3 || D16 == 5) {
        if (f.qb == 2)
          return f.mpad ? launch_attn_ks<D16, 2, true, 2>(ap, count, B, stream) : launch_attn_ks<D16, 2, false, 2>(ap, count, B, stream);
      }
      return f.mpad ? launch_attn_ks<D16, 2, true>(ap, count, B, stream) : launch_attn_ks<D16, 2, false>(ap, count, B, stream);
    }
    return f.mpad ? launch_attn_ks<D16, 1, true>(ap, count, B, stream) : launch_attn_ks<D16, 1, false>(ap, count, B, stream);
  } else {
    return launch_attn_ks<D16, 1, false>(ap, count, B, stream);
  }
}

static int attn_prepare(AP& ap, const AttnArgs& a) {
  SDEO_CHECK(a.o && a.q && a.k && a.v, "attention: null operand");
  SDEO_CHECK(a.TkS >= a.Tk && a.TkSv >= a.Tk, "attention: bad sizes Tk=%d TkS=%d TkSv=%d", a.Tk, a.TkS, a.TkSv);
  SDEO_CHECK(a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 && a.ldo % 4 == 0,
             "attention: strides must keep 16-byte alignment (ldq=%d ldk=%d ldv=%d ldo=%d)", a.ldq, a.ldk, a.ldv, a.ldo);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(a.q) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.k) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(a.v) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.o) & 7) == 0,
             "attention: operands must be 16-byte aligned");
  SDEO_CHECK(a.qB == 0 || (a.qB <= a.B && 2 * a.qB >= a.B), "attention: qB=%d must lie in [B/2, B] (B=%d)", a.qB, a.B);
  SDEO_CHECK(a.plan_B == 0 || a.plan_B >= a.B, "attention: plan_B=%d is smaller than B=%d", a.plan_B, a.B);
  ap = AP{a.o, a.q, a.k, a.v, a.ldo, a.ldq, a.ldk, a.ldv, a.H, a.Tq, a.Tk, a.TkS, a.TkSv, a.d, a.scale * 1.4426950408889634f, a.causal ? 1 : 0,
          a.qB > 0 ? a.qB : a.B};
  return 0;
}

static int attn_dispatch(const AttnForm& f, const AP2& ap, int count, int B, hipStream_t stream) {
  if (f.wide == 128) return launch_attn_wide<128>(ap.k[0], B, stream);
  if (f.wide == 64) return launch_attn_wide<64>(ap.k[0], B, stream);
  switch (f.d16) {
    case 1: return launch_attn<1>(f, ap, count, B, stream);
    case 2: return launch_attn<2>(f, ap, count, B, stream);
    case 3: return launch_attn<3>(f, ap, count, B, stream);
    case 4: return launch_attn<4>(f, ap, count, B, stream);
    case 5: return launch_attn<5>(f, ap, count, B, stream);
    case 6: return launch_attn<6>(f, ap, count, B, stream);
    case 8: return launch_attn<8>(f, ap, count, B, stream);
    case 10: return launch_attn<10>(f, ap, count, B, stream);
    default: return fail("attention: no kernel for the selected form (d16 = %d)", f.d16);   // attn_select never returns one
  }
}

int attention(const AttnArgs& a, hipStream_t stream) {
  AP2 ap{};
  AttnForm f;
  if (int rc = attn_prepare(ap.k[0], a)) return rc;
  if (int rc = attn_select(f, a.plan_B > 0 ? a.plan_B : a.B, a.H, a.Tq, a.Tk, a.d, a.causal)) return rc;
  return attn_dispatch(f, ap, 1, a.B, stream);
}

int attention(f16* o, int ldo, const f16* q, int ldq, const f16* k, int ldk, const f16* v, int ldv, int B, int H,
              int Tq, int Tk, int TkS, int TkSv, int d, float scale, hipStream_t stream, int causal) {
  return attention(AttnArgs{o, q, k, v, ldo, ldq, ldk, ldv, B, H, Tq, Tk, TkS, TkSv, d, scale, causal}, stream);
}

// ---- two segments.  The selection depends on the head dim alone: always the KS = 1 form (the second segment is one tile handled by
// the wave that owns the query block; cross-attention, the caller, has 77 keys), MPAD as attn_select decides it.
static int attn2_select(AttnForm& f, int B, int H, int Tq, int Tk, int Tk2, int d) {
  SDEO_CHECK(Tk2 >= 1 && Tk2 <= 64, "attention2: the second segment holds 1..64 keys (got %d)", Tk2);
  SDEO_CHECK(d != 256 && d != 512, "attention2: head dim %d has no two-segment kernel (8..96 in steps of 8, 120, 128, 152, 160)", d);
  if (int rc = attn_select(f, B, H, Tq, Tk, d, 0)) return rc;
  f.ks = 1;
  f.qb = 4;
  return 0;
}

const char* attention2_kernel_name(int B, int H, int Tq, int Tk, int Tk2, int d) {
  static thread_local char name[48];
  AttnForm f;
  if (attn2_select(f, B, H, Tq, Tk, Tk2, d)) return nullptr;
  snprintf(name, sizeof(name), "attention2_kernel<%d,%s>", f.d16, f.mpad ? "true" : "false");
  return name;
}

template <int D16, bool MPAD>
static int launch_attn2(const AP3& ap, int B, hipStream_t stream) {
  constexpr int DT = (D16 + 1) / 2;
  constexpr int KROW = D16 * 32 + ((D16 * 2) % 2 == 0 ? 16 : 0);
  constexpr int smem = 2 * (64 * KROW + 64 * attn_vrow(DT));
  static DeviceOnce attr_done;
  if (attr_done.need()) {
    SDEO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&attention2_kernel<D16, MPAD>), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_done.mark();
  }
  hipLaunchKernelGGL((attention2_kernel<D16, MPAD>), dim3(cdiv(ap.k[0].Tq, 128) * B * ap.k[0].H), dim3(256), smem, stream, ap);
  SDEO_HIP(hipGetLastError());
  return 0;
}

// every refusal of attention2, on the host and before any device call; fills the kernel's parameter block and the selected form
static int attn2_prepare(AP3& ap, AttnForm& f, const AttnArgs& a, const Attn2Seg& s2) {
  SDEO_CHECK(a.o && a.q && a.k && a.v && s2.k && s2.v, "attention2: null operand");
  SDEO_CHECK(!a.causal, "attention2: no causal form");
  SDEO_CHECK(std::isfinite(s2.w), "attention2: the weight of the second segment is not finite");
  if (int rc = attn2_select(f, a.plan_B > 0 ? a.plan_B : a.B, a.H, a.Tq, a.Tk, s2.Tk, a.d)) return rc;
  if (int rc = attn_prepare(ap.k[0], a)) return rc;
  SDEO_CHECK(s2.TkS >= s2.Tk && s2.TkSv >= s2.Tk, "attention2: bad sizes Tk2=%d TkS2=%d TkSv2=%d", s2.Tk, s2.TkS, s2.TkSv);
  SDEO_CHECK(s2.ldk % 8 == 0 && s2.ldv % 8 == 0, "attention2: strides must keep 16-byte alignment (ldk2=%d ldv2=%d)", s2.ldk, s2.ldv);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(s2.k) & 15) == 0 && (reinterpret_cast<uintptr_t>(s2.v) & 15) == 0,
             "attention2: operands must be 16-byte aligned");
  ap.x = APX{s2.k, s2.v, s2.ldk, s2.ldv, s2.Tk, s2.TkS, s2.TkSv, s2.w};
  return 0;
}

int attention2_check(const AttnArgs& a, const Attn2Seg& s2) {
  AP3 ap{};
  AttnForm f;
  return attn2_prepare(ap, f, a, s2);
}

int attention2(const AttnArgs& a, const Attn2Seg& s2, hipStream_t stream) {
  AP3 ap{};
  AttnForm f;
  if (int rc = attn2_prepare(ap, f, a, s2)) return rc;
  switch (f.d16 * 2 + f.mpad) {
    case 2: return launch_attn2<1, false>(ap, a.B, stream);
    case 3: return launch_attn2<1, true>(ap, a.B, stream);
    case 4: return launch_attn2<2, false>(ap, a.B, stream);
    case 5: return launch_attn2<2, true>(ap, a.B, stream);
    case 6: return launch_attn2<3, false>(ap, a.B, stream);
    case 7: return launch_attn2<3, true>(ap, a.B, stream);
    case 8: return launch_attn2<4, false>(ap, a.B, stream);
    case 9: return launch_attn2<4, true>(ap, a.B, stream);
    case 10: return launch_attn2<5, false>(ap, a.B, stream);
    case 11: return launch_attn2<5, true>(ap, a.B, stream);
    case 12: return launch_attn2<6, false>(ap, a.B, stream);
    case 16: return launch_attn2<8, false>(ap, a.B, stream);
    case 20: return launch_attn2<10, false>(ap, a.B, stream);
    default: return fail("attention2: no kernel for the selected form (d16 = %d, mpad = %d)", f.d16, f.mpad);   // attn2_select never returns one
  }
}

}  // namespace sdeo
