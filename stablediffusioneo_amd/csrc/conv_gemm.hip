// Implicit-GEMM convolution / GEMM for gfx950 (CDNA4) on v_mfma_f32_16x16x32_f16.
//
// Replaces, for the CNSD hot path, every F.conv2d / F.linear the reference issues through ATen
// (ResBlock convs `openaimodel.py:200-240`, Down/Upsample `:90-159`, SpatialTransformer proj_in/out
// and the CrossAttention / GEGLU Linear layers `attention.py:49-76,154-179`, VAE convs `model.py`).
//
// Design (MI355X-first, not a cuDNN/cuBLAS shape):
//  * both operands are K-contiguous: activations NHWC (channel fastest), weights KRSC; every MFMA
//    fragment is one 16-byte LDS read, every global access a 16-byte vector.
//  * the im2col matrix is never materialised: the A tile is gathered straight from the NHWC tensor,
//    one filter tap x BK channels per K-step; zero padding, stride 2 and the nearest-x2 Upsample are
//    folded into the gather address.
//  * weights are the MFMA "A" operand (rows = output channel), activations the "B" operand (cols =
//    output pixel): each lane then ends up with 4 consecutive output channels of one pixel, i.e. an
//    8-byte NHWC store, and bias / time-embedding / residual / SiLU / scale are applied in registers.
//  * main kernel (`conv_gemm_dma_kernel`): global_load_lds (LDS-DMA, 16 B per lane) into a ring of LDS
//    stages, counted s_waitcnt vmcnt(N) + raw s_barrier so 1-3 K-steps of loads stay in flight across
//    the barrier; padding rows read a zero page so every lane issues the same number of DMAs; the XOR
//    swizzle that makes the ds_read_b128 fragment reads bank-conflict free is applied to the per-lane
//    SOURCE address (the DMA destination is lane-linear) and to the fragment reads.
//  * fallback kernel (`conv_gemm_kernel`): register-staged double buffering, used when Cin is not a
//    multiple of 64 (first convs, hint block, reduced test configs).
//  * split-K over blockIdx.z for the weight-bandwidth-bound deep levels (M = 128..512, K up to 23k) and to
//    fill 256 CUs when M x N is small.
#include <stdlib.h>

#include <array>
#include <map>

#include <type_traits>
#include <utility>

#include "conv_inl.h"

namespace sdeo {

// ------------------------------------------------------------------------------------------------
// main kernel: LDS-DMA ring, Cin % 64 == 0
// ------------------------------------------------------------------------------------------------
// WS ("wave-specialised"): 8 waves, waves 0-3 only read fragments and issue MFMAs, waves 4-7 only issue the LDS-DMAs.
// An LDS-DMA instruction stalls its wave for ~60-180 clocks at issue (measured); with one
// workgroup per CU that stall sat in front of every K-step's MFMAs.  Same ring protocol, one barrier per K-step for
// both roles: the loaders retire step `it` (counted vmcnt) BEFORE barrier `it`, the MFMA waves read it AFTER; the
// loaders refill slot (it-1) % STAGES after barrier `it`, which every MFMA wave only reaches once its reads of step
// it-1 have fed its MFMAs.
// W8: the weights are fp8 (OCP e4m3fn, one byte per element, per-output-channel power-of-two scale applied in the epilogue):
// a weight-tile row is 64 bytes per K-step instead of 128, one DMA pass of the 256 loading threads covers 64 rows, and the
// MFMA waves widen each 8-byte fragment to fp16 in registers (v_cvt_scalef32_pk_f16_fp8, exact) right before its MFMAs.
// The activations, the accumulation and the epilogue are those of the fp16 kernel; what changes is the bytes streamed.
// KPB (K-steps per barrier): the ring still holds STAGES 64-deep steps and every step is issued and retired as before, but loaders
// and MFMA waves meet only once per GROUP of KPB steps: the loaders make a whole group visible with one counted wait + barrier and
// then refill the KPB slots of the previous group.  A small tile has 10 - 20 MFMAs per wave per step (160 - 320 clocks) against a
// barrier / wait skeleton of ~240 clocks per step; the halo kernel gained 14 - 35 % from the same change
// (conv_halo.hip TPB).  Needs STAGES >= 2 KPB; STAGES - 2 KPB steps of loads stay in flight across a barrier.
// MX: both operands are block-scaled fp8 (KP::mx_sx): the loaders move the same 128-byte rows (128 codes instead of 64 halves: the
// address arithmetic is that of an fp16 problem of half the length), the MFMA waves read each lane's 32 consecutive codes as two
// 16-byte chunks and issue v_mfma_scale_f32_16x16x128_f8f6f4 with the two e8m0 block scales of the lane's row and 32-code block:
// 4x the K per MFMA at twice its cycles, half the operand bytes per FLOP.  GEMM (1x1) only, wave-specialised only.
// MULTI (multi-problem launch): the grid is the concatenation of the tiles of up to kMultiMax problems that share this tile.  The
// argument is an MPArgs: the problems' parameter blocks and the inclusive prefix sums of their tile counts sit in device memory
// (MPTable, written when the launch is configured), the per-problem `scale` comes by kernel argument (it is read when the launch runs).
// A workgroup finds (problem, tile in problem) by a branch-free scan of the prefix sums in SGPRs, copies that problem's block in one
// batch and from there on IS a workgroup of that problem's own launch: same K order, same epilogue, bit-identical output.  Unsplit
// fp16 plans only (host-checked).  With MULTI = false nothing of this is compiled and the kernel is the one it was.
// EPI (EpiKind, conv_inl.h): EPI_DIRECT deals the weight rows of each wave's strip to the LDS rows in the order of direct_row_chan
// (a change of the loaders' SOURCE rows only: the LDS image, the fragment reads and the K loop are those of EPI_STAGED, so the
// fragment reads stay bank-conflict free) and stores from the accumulators (epilogue_direct); the staged epilogue is not compiled in.
// LIVE (with MULTI; the argument is an MPArgsLive): problem i computes its first m_live[i] rows only.  An M tile wholly at or beyond
// m_live runs no K loop (nk = 0: the loaders issue nothing, the MFMA waves go straight to the pre-epilogue barrier) and copies its `res`
// rows to the output; the tile that straddles m_live computes, its epilogue stores the live rows only (mrow = -1 for the others, the
// state rows beyond M have in every launch) and the rows left over are copied.  A dead row is SELECTED, never scaled: what the
// activation rows beyond m_live hold does not reach the output.  res == y (an in-place problem): nothing is copied.  With LIVE = false
// none of this is compiled.
template <int BM, int BN, int STAGES, bool UPS, bool WS, bool W8 = false, int KPB = 1, bool MX = false, bool MULTI = false, int EPI = EPI_STAGED,
          bool LIVE = false>
__global__ __launch_bounds__(WS ? 512 : 256) void conv_gemm_dma_kernel(const std::conditional_t<LIVE, MPArgsLive, std::conditional_t<MULTI, MPArgs, KP>> pp) {
  kernarg_warm<sizeof(pp)>();
  static_assert(!MULTI || (!W8 && !MX), "multi-problem launches stream fp16 weights");
  static_assert(!LIVE || MULTI, "live-row counts come with the multi-problem argument");
  static_assert(!LIVE || !WS, "the pass-through of the dead rows strides by the 256 threads of a four-wave workgroup");
  static_assert(EPI == EPI_STAGED || (!W8 && !MX && !MULTI && !UPS), "the register-direct epilogue exists for the plain fp16 kernels");
  // The scalars both roles need before their first DMA / fragment read, fetched in ONE batch and pinned in SGPRs: left to the
  // compiler each is an s_load + s_waitcnt lgkmcnt(0) next to its first use, ten dependent scalar round trips in front of the
  // first DMA of a launch whose whole K loop lasts a few microseconds.
  KP pl;
  int wg = blockIdx.x;                     // position of this workgroup among the tiles of its problem
  [[maybe_unused]] int mp_prob = 0;
  if constexpr (MULTI) {
    int pre[kMultiMax];
#pragma unroll
    for (int i = 0; i < kMultiMax; ++i) pre[i] = mp_prefix(pp.tab, i);     // (entries past the count hold INT_MAX)
    int prob = 0, first = 0;
#pragma unroll
    for (int i = 0; i < kMultiMax - 1; ++i) {
      const bool past = (int)blockIdx.x >= pre[i];
      prob += past ? 1 : 0;
      first = past ? pre[i] : first;
    }
    mp_prob = __builtin_amdgcn_readfirstlane(min(prob, pp.count - 1));
    wg = __builtin_amdgcn_readfirstlane((int)blockIdx.x - first);
    pl = mp_block(pp.tab, mp_prob);
    pl.scale = pp.scale[mp_prob];
    mp_globalize(pl);
  } else {
    pl = pp;
  }
  // (integers only: a pointer that has been through the asm loses its address space and every access through it becomes a flat_ one)
  asm volatile("" : "+s"(pl.M), "+s"(pl.N), "+s"(pl.K), "+s"(pl.Hi), "+s"(pl.Wi), "+s"(pl.Cin), "+s"(pl.Wo),
               "+s"(pl.S), "+s"(pl.stride), "+s"(pl.pad), "+s"(pl.HoWo), "+s"(pl.ldx), "+s"(pl.ldw), "+s"(pl.nk),
               "+s"(pl.nk_per_split), "+s"(pl.tiles_m), "+s"(pl.tiles_n), "+s"(pl.n_fastest));
  const KP& p = pl;
  static_assert(!MX || (WS && !W8 && !UPS && KPB == 1), "the block-scaled fp8 path exists for the plain wave-specialised GEMM");
  constexpr int BK = 64, RPP = 32;
  constexpr int WRPP = W8 ? 64 : 32;                           // weight rows per DMA pass
  constexpr int XP = BM / RPP, WP = (BN + WRPP - 1) / WRPP, L = XP + WP;     // DMA instructions per loading thread per stage
  constexpr int TM = BM / 2, TN = BN / 2, MI = TM / 16, NI = TN / 16;
  constexpr int XBYTES = BM * BK * 2, WBYTES = WP * 4096, STAGE = XBYTES + WBYTES;
  constexpr int PF = STAGES - KPB;                              // K-steps of loads issued ahead of the compute (initial fill)
  constexpr int FLY = STAGES - 2 * KPB;                         // steps of loads that stay in flight across a barrier
  static_assert(KPB >= 1 && FLY >= 0 && PF >= 1 && STAGES <= 10, "ring depth");

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool do_load = !WS || wave_all >= 4;                   // wave-uniform roles
  const bool do_mma = !WS || wave_all < 4;
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;      // indices inside the role
  const int wm = wave & 1, wn = wave >> 1;
  int m0, n0;
  auto set_tile = [&](int t) {             // t: position in the (XCD-aware) tile order
    const int tile = xcd_remap(t, p.tiles_m * p.tiles_n);
    const int tm = p.n_fastest ? tile / p.tiles_n : tile % p.tiles_m;
    const int tn = p.n_fastest ? tile % p.tiles_n : tile / p.tiles_m;
    m0 = tm * BM; n0 = tn * BN;
  };
  set_tile(wg);
  const int z = blockIdx.z;
  const int kbeg = z * p.nk_per_split;
  const int kend = min(p.nk, kbeg + p.nk_per_split);
  [[maybe_unused]] int m_live = 0;
  if constexpr (LIVE) m_live = __builtin_amdgcn_readfirstlane(min(max(pp.m_live[mp_prob], 0), p.M));
  const int nk = (LIVE && m0 >= m_live) ? 0 : kend - kbeg;     // (m0 is uniform: every wave of a dead tile skips the K loop)

  stamp(p, 0);
  const int chunk = tid & 7, lrow = tid >> 3;
  const int cl = chunk ^ ((lrow >> 1) & 7);        // logical k-chunk this lane fetches into its (linear) LDS slot
  const char* zero = reinterpret_cast<const char*>(g_zero_page);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // provably uniform: the DMA's LDS base stays in SGPRs

  // Gather state, all hoisted out of the K loop (the loop body must stay MFMA-bound, not address-bound):
  //   xrow[i]  address of this row's tap (0,0) pixel at channel chunk cl (may lie outside the tensor for border
  //            rows: it is only dereferenced when the tap's bit in vmask[i] is set)
  //   vmask[i] bit r*S+s = tap (r,s) of row i reads inside the image (zero padding otherwise)
  const char* xrow[XP];
  unsigned vmask[XP];
  int pixbase[UPS ? XP : 1], hb[UPS ? XP : 1], wb[UPS ? XP : 1];
  const char* wptr[WP];
  int winc[WP];
  const int tapsteps = p.Cin >> 6;
  int st_c, st_r, st_s;                                                                         // next K-step to issue
  auto loader_setup = [&]() {              // gather state of tile (m0, n0)
    st_c = kbeg % tapsteps; st_r = (kbeg / tapsteps) / p.S; st_s = (kbeg / tapsteps) % p.S;
    const int Hv = UPS ? 2 * p.Hi : p.Hi, Wv = UPS ? 2 * p.Wi : p.Wi;
    const int R = p.K / (p.S * p.Cin);
    const bool linear = !UPS && p.K == p.Cin && p.stride == 1 && p.pad == 0;   // Linear / conv1x1: row m IS pixel m
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int m = m0 + lrow + i * RPP;
      const bool mv = m < p.M;
      if (linear) {
        vmask[i] = (mv && !dbg_on(p, 1)) ? 1u : 0u;
        xrow[i] = reinterpret_cast<const char*>(p.x) + ((long)m * p.ldx + cl * 8) * 2;
        continue;
      }
      const int mm = mv ? m : 0;
      const int b = mm / p.HoWo;
      const int rem = mm - b * p.HoWo;
      const int ho = rem / p.Wo;
      const int wo = rem - ho * p.Wo;
      const int h0 = ho * p.stride - p.pad, w0 = wo * p.stride - p.pad;
      // taps inside the image: rows rlo..rhi-1, columns slo..shi-1
      const int rlo = max(0, -h0), rhi = min(R, Hv - h0), slo = max(0, -w0), shi = min(p.S, Wv - w0);
      const unsigned sm = (mv && shi > slo && !dbg_on(p, 1)) ? (((1u << shi) - 1u) & ~((1u << slo) - 1u)) : 0u;
      unsigned vm = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r)          // R <= 4 (checked on the host): straight-line selects instead of a divergent loop
        if (r >= rlo && r < rhi) vm |= sm << (r * p.S);
      vmask[i] = vm;
      if (UPS) {
        pixbase[i] = b * p.Hi * p.Wi; hb[i] = h0; wb[i] = w0;
        xrow[i] = nullptr;
      } else {
        xrow[i] = reinterpret_cast<const char*>(p.x) + ((long)(b * p.Hi * p.Wi + h0 * p.Wi + w0) * p.ldx + cl * 8) * 2;
      }
    }
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      if constexpr (!W8) {
        const int lr = lrow + i * RPP;             // LDS row of the weight tile; the channel it holds:
        const int n = n0 + (EPI == EPI_DIRECT ? lr / TN * TN + direct_row_chan<NI>(lr % TN) : lr);
        const bool nv = n < p.N && !dbg_on(p, 2);
        wptr[i] = nv ? reinterpret_cast<const char*>(p.w + (size_t)n * p.ldw + (size_t)kbeg * BK + cl * 8) : zero;
        winc[i] = nv ? BK * 2 : 0;
      } else {
        // 64-byte rows: thread (row = tid >> 2, 16-byte chunk c = tid & 3) of each pass; the LDS image rotates the four chunks
        // of row r by (r >> 2) & 3 (source-side, the DMA destination is lane-linear) so that the 8-byte fragment reads of a
        // 32-lane half (16 rows x 2 k-groups) cover all 64 banks once
        const int r8 = (tid >> 2) + i * 64, c = tid & 3;
        const int n = n0 + r8;
        const bool nv = r8 < BN && n < p.N && !dbg_on(p, 2);
        const int csrc = (c - ((r8 >> 2) & 3)) & 3;
        wptr[i] = nv ? reinterpret_cast<const char*>(p.w) + (size_t)n * p.ldw + (size_t)kbeg * BK + csrc * 16 : zero;
        winc[i] = nv ? BK : 0;
      }
    }
  };
  if (do_load) loader_setup();

  // issue the DMAs of the NEXT K-step into ring slot `slot` (every loading lane issues exactly L of them)
  auto issue = [&](int slot) {
    const int tapbit = st_r * p.S + st_s;
    char* xs = smem + slot * STAGE + wave_u * 1024;
    char* wsm = xs + XBYTES;
    if (!UPS) {
      const long toff = ((long)(st_r * p.Wi + st_s) * p.ldx + (st_c << 6)) * 2;
#pragma unroll
      for (int i = 0; i < XP; ++i) {
        const char* src = ((vmask[i] >> tapbit) & 1) ? xrow[i] + toff : zero;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(xs + i * 4096), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < XP; ++i) {
        const int hi = (hb[i] + st_r) >> 1, wi = (wb[i] + st_s) >> 1;
        const char* src = ((vmask[i] >> tapbit) & 1)
                              ? reinterpret_cast<const char*>(p.x) + ((long)(pixbase[i] + hi * p.Wi + wi) * p.ldx + (st_c << 6) + cl * 8) * 2
                              : zero;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(xs + i * 4096), 16, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)wptr[i],
                                       (__attribute__((address_space(3))) void*)(wsm + i * 4096), 16, 0, 0);
      wptr[i] += winc[i];
    }
    if (++st_c == tapsteps) {
      st_c = 0;
      if (++st_s == p.S) { st_s = 0; ++st_r; }
    }
  };
  // retire the DMAs of group g (K-steps g KPB .. g KPB + KPB - 1): all but the (newer) steps still allowed in flight.  Steps are
  // issued in order: PF in the prologue, then KPB more after every barrier, so behind group g at most FLY steps are younger.
  auto retire = [&](int g) {
    const int ahead = max(0, min(FLY, nk - (g + 1) * KPB));
    static_for<FLY + 1>([&](auto A) {
      if (ahead == A.value) wait_vmcnt<A.value * L>();
    });
  };
  // after barrier g every MFMA wave holds group g - 1 in registers: refill its slots (group 0: the KPB slots not used yet)
  auto refill = [&](int g) {
#pragma unroll
    for (int j = 0; j < KPB; ++j) {
      const int step = PF + g * KPB + j;
      if (step < nk && !dbg_on(p, 8)) issue(step % STAGES);
    }
  };
  const int ngroups = (nk + KPB - 1) / KPB;

  if constexpr (WS) {
    if (!do_mma) {                         // ---- loader waves
      if (nk > 0) {
#pragma unroll
        for (int s = 0; s < PF; ++s)
          if (s < nk) issue(s);
        for (int g = 0; g < ngroups; ++g) {
          retire(g);
          __builtin_amdgcn_s_barrier();
          refill(g);
        }
      }
      __builtin_amdgcn_s_barrier();          // matches the MFMA waves' pre-epilogue barrier (LDS becomes epilogue scratch)
      return;
    }
  }

  const int frow = lane & 15, fq = lane >> 4;
  constexpr int g0 = 0;
  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // LayerNorm folded into this GEMM: (rstd, rstd * mean) of the tile's rows from the producer's per-strip partials, summed by
  // the MFMA waves of column 0 while the first K-step is in flight (they would wait on the first barrier otherwise) and parked
  // in LDS behind the ring; the epilogue reads two floats per row instead of re-summing up to N/32 partials per lane.
  float2* lnsm = reinterpret_cast<float2*>(smem + STAGES * STAGE);
  const bool ln_lds = p.ln_stats != nullptr && p.splitk == 1;
  if (ln_lds && wn == 0) {
    for (int rr = lane; rr < TM; rr += 64) {
      const int m = m0 + wm * TM + rr;
      float r = 0.f, rm = 0.f;
      if (m < p.M) ln_row_scalars(p, m, r, rm);
      lnsm[wm * TM + rr] = make_float2(r, rm);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // written before this wave's next barrier, read after the pre-epilogue one
  }

  // the bias is needed only by the epilogue: fetch it now (issued before, hence older than, every DMA) so the
  // epilogue does not start with a dependent global round trip
  f32x4 bpre[NI];
  const bool use_bpre = p.bias && !p.bias_per_row && p.splitk == 1;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = n0 + wn * TN + lane_chan<NI, EPI == EPI_DIRECT>(i, fq);
    bpre[i] = (use_bpre && n < p.N) ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // One K-step of MFMAs.  hipcc waits lgkmcnt(0) before the first MFMA after ANY group of LDS reads in this kernel (it
  // never emits a partial count here), and left alone it keeps a minimal fragment set: four full LDS round trips per
  // K-step in front of ~20 MFMAs (measured 700 clocks per step for 320 clocks of MFMA).  So on tiles with room for two
  // fragment sets the reads are inline asm (invisible to the compiler's wait insertion) with hand-counted waits: all reads
  // of the step are issued, lgkmcnt(NI+MI) releases the 32-deep half 0 (LDS returns in order), its MFMAs run while half 1
  // lands.  sched_barrier(0) after each wait keeps hipcc from hoisting MFMAs above it.
  constexpr bool DB = (NI + MI) * 8 + NI * MI * 4 <= 200;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int swl = (frow >> 1) & 7;                      // == (row >> 1) & 7: every fragment row is frow + multiple of 16
  const unsigned xa0 = lds0 + (wm * TM + frow) * 128 + ((fq ^ swl) << 4), xa1 = lds0 + (wm * TM + frow) * 128 + (((4 + fq) ^ swl) << 4);
  // weight fragment addresses: fp16 rows of 128 bytes (chunk swizzle as for the activations) or fp8 rows of 64 bytes, 8-byte
  // k-group g = kk * 4 + fq stored at group (g + 2 ((row >> 2) & 3)) & 7
  const int g8 = (fq + 2 * ((frow >> 2) & 3)) & 7;
  const unsigned wa0 = W8 ? lds0 + XBYTES + (wn * TN + frow) * 64 + g8 * 8 : xa0 + XBYTES + (wn * TN - wm * TM) * 128;
  const unsigned wa1 = W8 ? lds0 + XBYTES + (wn * TN + frow) * 64 + (g8 ^ 4) * 8 : xa1 + XBYTES + (wn * TN - wm * TM) * 128;
  constexpr int WSTEP = W8 ? 1024 : 2048;               // bytes between fragment rows i and i + 1 (16 tile rows)
  typedef std::conditional_t<W8, uint2, f16x8> wfrag;   // a weight fragment as it sits in LDS
  auto widen = [](const wfrag& w) -> f16x8 {
    if constexpr (W8) {
      const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.0f, true);
      const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.0f, true);
      return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    } else {
      return w;
    }
  };
  auto read_half = [&](const char* xs, const char* wsm, int kk, wfrag (&wf)[NI], f16x8 (&xf)[MI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = wn * TN + i * 16 + frow;
      if constexpr (W8) wf[i] = *reinterpret_cast<const uint2*>(wsm + row * 64 + ((kk * 4 + fq + 2 * ((row >> 2) & 3)) & 7) * 8);
      else wf[i] = *reinterpret_cast<const f16x8*>(wsm + row * 128 + swz_chunk<64>(row, kk * 4 + fq) * 16);
    }
#pragma unroll
    for (int j = 0; j < MI; ++j) {
      const int row = wm * TM + j * 16 + frow;
      xf[j] = *reinterpret_cast<const f16x8*>(xs + row * 128 + swz_chunk<64>(row, kk * 4 + fq) * 16);
    }
  };
  auto mma_half = [&](const wfrag (&wf)[NI], const f16x8 (&xf)[MI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const f16x8 w = widen(wf[i]);
#pragma unroll
      for (int j = 0; j < MI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, xf[j], acc[i][j], 0, 0, 0);
    }
  };
  auto compute = [&](int it) {
    if constexpr (DB) {
      const unsigned sb = ((g0 + it) % STAGES) * STAGE;
      wfrag wf0[NI], wf1[NI];
      f16x8 xf0[MI], xf1[MI];
      static_for<NI>([&](auto I) { lds_read_w<I.value * WSTEP>(wf0[I.value], wa0 + sb); });
      static_for<MI>([&](auto J) { lds_read128<J.value * 2048>(xf0[J.value], xa0 + sb); });
      static_for<NI>([&](auto I) { lds_read_w<I.value * WSTEP>(wf1[I.value], wa1 + sb); });
      static_for<MI>([&](auto J) { lds_read128<J.value * 2048>(xf1[J.value], xa1 + sb); });
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NI + MI) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma_half(wf0, xf0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma_half(wf1, xf1);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      const char* xs = smem + ((g0 + it) % STAGES) * STAGE;
      const char* wsm = xs + XBYTES;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        wfrag wf[NI];
        f16x8 xf[MI];
        read_half(xs, wsm, kk, wf, xf);
        __builtin_amdgcn_sched_barrier(0);
        mma_half(wf, xf);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  if (nk > 0) {
    if constexpr (WS) {                    // ---- MFMA waves
      // retire every scalar (kernel-argument) load here: while one may be pending the compiler's wait-count pass has to
      // assume out-of-order LGKM returns and turns each partial lgkmcnt(N) in the loop into lgkmcnt(0)
      __builtin_amdgcn_s_waitcnt(0xc07f);
      if constexpr (MX) {
        // Two fragment register sets by step parity.  Operand map of the instruction (found with exact integer data, tools/mx_probe*.py:
        // CK's "32 consecutive k per lane" does not describe it): the 128-deep step is two 64-deep halves, lane (r = l & 15, g = l >> 4)
        // holds k = 16 g .. 16 g + 15 of EACH half (bytes 0-15: first half, bytes 16-31: second half) -- chunks g and 4 + g of the 128-byte
        // LDS row, the very chunks of the fp16 fragments -- while the scale it supplies belongs to block g = k in [32 g, 32 g + 32).
        // The reads of step it + 1 are issued before the MFMAs of step it.
        typedef int v8i __attribute__((ext_vector_type(8)));
        typedef int v4i __attribute__((ext_vector_type(4)));
        const unsigned xm0 = lds0 + (wm * TM + frow) * 128 + ((fq ^ swl) << 4), xm1 = lds0 + (wm * TM + frow) * 128 + (((4 + fq) ^ swl) << 4);
        const unsigned wm0 = xm0 + XBYTES + (wn * TN - wm * TM) * 128, wm1 = xm1 + XBYTES + (wn * TN - wm * TM) * 128;
        f16x8 wlo[NI], whi[NI], xlo[MI], xhi[MI];
        int swv[NI], sxv[MI];
        // scale bytes of this lane's rows: block index = 4 * (K-step) + fq; rows past the problem read row 0 (their results are dropped)
        const unsigned char* swp[NI];
        const unsigned char* sxp[MI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int n = n0 + wn * TN + i * 16 + frow;
          swp[i] = p.mx_sw + (size_t)(n < p.N ? n : 0) * p.mx_ldsw + kbeg * 4 + fq;
        }
#pragma unroll
        for (int j = 0; j < MI; ++j) {
          const int m = m0 + wm * TM + j * 16 + frow;
          sxp[j] = p.mx_sx + (size_t)(m < p.M ? m : 0) * p.mx_ldsx + kbeg * 4 + fq;
        }
        auto rd = [&](unsigned sb) {
          static_for<NI>([&](auto I) { lds_read128<I.value * 2048>(wlo[I.value], wm0 + sb); lds_read128<I.value * 2048>(whi[I.value], wm1 + sb); });
          static_for<MI>([&](auto J) { lds_read128<J.value * 2048>(xlo[J.value], xm0 + sb); lds_read128<J.value * 2048>(xhi[J.value], xm1 + sb); });
        };
        auto cat = [](const f16x8& lo, const f16x8& hi) -> v8i {
          const v4i a = __builtin_bit_cast(v4i, lo), b = __builtin_bit_cast(v4i, hi);
          return v8i{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        };
        // ONE fragment set (two spilled at the 256-register cap of an 8-wave workgroup): an MFMA reads its operands at issue, so the
        // reads of step it + 1 are issued right behind the last MFMA of step it and land while the matrix pipe works through them
        __builtin_amdgcn_s_barrier();        // step 0 visible
        rd(0u);
        for (int it = 0; it < nk; ++it) {
          int swn[NI], sxn[MI];
#pragma unroll
          for (int i = 0; i < NI; ++i) swv[i] = swp[i][it * 4];
#pragma unroll
          for (int j = 0; j < MI; ++j) sxv[j] = sxp[j][it * 4];
          (void)swn; (void)sxn;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const v8i w = cat(wlo[i], whi[i]);
#pragma unroll
            for (int j = 0; j < MI; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, cat(xlo[j], xhi[j]), acc[i][j], 0, 0, 0, swv[i], 0, sxv[j]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (it + 1 < nk) {
            __builtin_amdgcn_s_barrier();    // step it+1 visible; every MFMA wave has issued (= read the operands of) step `it`
            rd(((it + 1) % STAGES) * STAGE);
          }
        }
      } else if constexpr (DB) {
        // Rotated loop: barrier `it+1` and the half-0 reads of step it+1 are issued BEFORE the half-1 MFMAs of step it,
        // the half-1 reads of step it+1 right after them, so every LDS round trip and the barrier hide under 32-deep
        // halves of MFMAs.  A wave reaches barrier it+1 only after lgkmcnt(0), i.e. with all its reads of step `it` in
        // registers, which is what allows the loaders to refill that slot.  Register sets are rewritten only after the
        // MFMAs reading them have issued (an LDS return is >60 clocks away, an MFMA reads its operands at issue).
        wfrag wf0[NI], wf1[NI];
        f16x8 xf0[MI], xf1[MI];
        auto reads0 = [&](unsigned sb) {
          if (dbg_on(p, 16)) return;
          static_for<NI>([&](auto I) { lds_read_w<I.value * WSTEP>(wf0[I.value], wa0 + sb); });
          static_for<MI>([&](auto J) { lds_read128<J.value * 2048>(xf0[J.value], xa0 + sb); });
        };
        auto reads1 = [&](unsigned sb) {
          if (dbg_on(p, 16)) return;
          static_for<NI>([&](auto I) { lds_read_w<I.value * WSTEP>(wf1[I.value], wa1 + sb); });
          static_for<MI>([&](auto J) { lds_read128<J.value * 2048>(xf1[J.value], xa1 + sb); });
        };
        stamp(p, 1);
        __builtin_amdgcn_s_barrier();        // step 0 visible
        stamp(p, 2);
        reads0((g0 % STAGES) * STAGE);
        reads1((g0 % STAGES) * STAGE);
        int ing = 1;                         // position of step it + 1 inside its group (KPB = 1: always 0 = opens a group)
        for (int it = 0; it < nk; ++it) {
          const bool more = it + 1 < nk;
          if (ing == KPB) ing = 0;
          const bool newgroup = KPB == 1 || ing == 0;      // step it + 1 opens a group: meet the loaders before reading it
          const unsigned sbn = ((g0 + it + 1) % STAGES) * STAGE;
          asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NI + MI) : "memory");
          __builtin_amdgcn_sched_barrier(0);
          if (!dbg_on(p, 4)) mma_half(wf0, xf0);
          __builtin_amdgcn_sched_barrier(0);
          if (newgroup || !more) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (more) {
              __builtin_amdgcn_s_barrier();  // group of step it+1 visible; every MFMA wave holds step `it` in registers
              reads0(sbn);
            }
          } else {
            reads0(sbn);                     // same group, already visible: the half-1 fragments of step `it` only have to be in
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NI + MI) : "memory");     // registers (older than the NI + MI reads just issued)
          }
          __builtin_amdgcn_sched_barrier(0);
          if (!dbg_on(p, 4)) mma_half(wf1, xf1);
          __builtin_amdgcn_sched_barrier(0);
          if (more) reads1(sbn);
          ++ing;
        }
      } else {
        for (int it = 0; it < nk; ++it) {
          if (it % KPB == 0) __builtin_amdgcn_s_barrier();      // group of step `it` visible (its loaders retired it before arriving here)
          if (!dbg_on(p, 4)) compute(it);
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < PF; ++s)
        if (s < nk) issue(s);
      for (int it = 0; it < nk; ++it) {
        if (it % KPB == 0) {
          retire(it / KPB);
          __builtin_amdgcn_s_barrier();    // group of step `it` visible to every wave; everyone is done reading the previous group's slots
          refill(it / KPB);
        }
        compute(it);
      }
    }
  }
  // every wave is done reading fragments and no DMA is pending (the last K-step was retired with vmcnt(0)): the ring becomes
  // the waves' private epilogue scratch
  KP pe = p;                               // the epilogue's scalars in one batch of loads, in flight across the barrier
  if constexpr (MULTI) { pe = mp_block(pp.tab, mp_prob); pe.scale = pp.scale[mp_prob]; }      // (the problem's block again, rather than ~60 SGPRs live across the K loop)
  pin_epilogue_scalars(pe);
  __builtin_amdgcn_s_barrier();
  stamp(p, 3);
  if (dbg_on(p, 32)) return;
  static_assert(4 * epilogue_scratch_bytes(TN) <= STAGES * STAGE, "epilogue scratch");
  constexpr int SCR = (STAGES * STAGE / 4) & ~15;        // LDS each wave may use as epilogue scratch
  [[maybe_unused]] constexpr int NBLK = epilogue_blocks(TN, MI, SCR);
  [[maybe_unused]] char* scratch = smem + wave * SCR;
  int mrow[MI];
#pragma unroll
  for (int j = 0; j < MI; ++j) {
    const int m = m0 + wm * TM + j * 16 + frow;
    mrow[j] = m < (LIVE ? m_live : pe.M) ? m : -1;
  }
  if constexpr (LIVE) {
    // the rows of this tile at or beyond m_live: out = res, 8 bytes per lane (N, ldy, ldres % 4 == 0 and 8-byte aligned bases: host-checked)
    if (pe.res && pe.res != pe.y) {
      const int r0 = max(m0, m_live), r1 = min(m0 + BM, pe.M);
      const int c4 = min(BN, pe.N - n0) >> 2;
      for (int idx = tid; idx < (r1 - r0) * c4; idx += 256) {
        const int r = r0 + idx / c4, c = n0 + (idx % c4) * 4;
        *reinterpret_cast<uint2*>(pe.y + (size_t)r * pe.ldy + c) = *reinterpret_cast<const uint2*>(pe.res + (size_t)r * pe.ldres + c);
      }
    }
    if (m0 >= m_live) return;              // a dead tile has nothing to store (uniform; no barrier follows for a multi-problem launch)
  }
  const float2* lnrow = ln_lds ? lnsm + wm * TM : nullptr;
  // One epilogue in the code.  SDEO_DBG_GEMM bit 128 takes a second trip through THE SAME instructions (a loop the compiler may not
  // unroll), so the second trip runs code the first one has just fetched: stamps 3 -> 4 against 5 -> 6 is cold fetch against work.
  // In the production build the loop condition is the constant false and there is no loop.
  int trip = 0;
#pragma nounroll
  do {
    if constexpr (EPI == EPI_DIRECT) {
      epilogue_direct<NI, MI, TN>(pe, acc, mrow, n0 + wn * TN, fq, bpre, use_bpre, lnrow);
    } else {
      epilogue_rows<NI, MI, TN, NBLK, EPI>(pe, acc, mrow, n0 + wn * TN, fq, z, bpre, use_bpre, scratch, lnrow);
      if (EpiMode<EPI>::gn(pe)) {          // GroupNorm partials of this tile (loader waves, if any, are gone: the barrier counts the rest)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wm == 0) {                     // waves 2 wn and 2 wn + 1 share strip wn
          const int bimg = m0 / pe.HoWo;
          gn_partials_finish<TN, 2>(pe, smem + 2 * wn * SCR, SCR, lane, bimg, (m0 - bimg * pe.HoWo) / BM, n0 + wn * TN);
        }
      }
    }
    if (dbg_on(p, 64)) {
      stamp(p, trip ? 6 : 4);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (!trip) stamp(p, 5);
    }
  } while (dbg_on(p, 128) && ++trip < 2);
}

// ------------------------------------------------------------------------------------------------
// fallback kernel: register-staged double buffer (any Cin % 8 == 0)
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int BK, bool GENERIC>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const KP pp) {
  kernarg_warm<sizeof(KP)>();
  const KP& p = pp;
  constexpr int CPR = BK / 8;         // 16-byte chunks per tile row
  constexpr int RPP = 256 / CPR;      // tile rows covered per pass of the 256 threads
  constexpr int XP = BM / RPP;        // passes for the activation tile
  constexpr int WP = BN / RPP;        // passes for the weight tile
  constexpr int TM = BM / 2, TN = BN / 2;   // wave tile (2x2 waves)
  constexpr int MI = TM / 16, NI = TN / 16;
  constexpr int XBYTES = BM * BK * 2, WBYTES = BN * BK * 2, STAGE = XBYTES + WBYTES;
  static_assert(XP >= 1 && WP >= 1, "tile too small for 256 threads");

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;

  const int tile = blockIdx.x;
  const int tm = tile % p.tiles_m, tn = tile / p.tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.z;
  const int kbeg = z * p.nk_per_split;
  const int kend = min(p.nk, kbeg + p.nk_per_split);

  const int chunk = tid % CPR;
  const int lrow = tid / CPR;

  int pixbase[XP], hb[XP], wb[XP];
  bool mvalid[XP];
  const int Hv = p.ups ? 2 * p.Hi : p.Hi, Wv = p.ups ? 2 * p.Wi : p.Wi;
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int m = m0 + lrow + i * RPP;
    mvalid[i] = m < p.M;
    const int mm = mvalid[i] ? m : 0;
    const int b = mm / p.HoWo;
    const int rem = mm - b * p.HoWo;
    const int ho = rem / p.Wo;
    const int wo = rem - ho * p.Wo;
    pixbase[i] = b * p.Hi * p.Wi;
    hb[i] = ho * p.stride - p.pad;
    wb[i] = wo * p.stride - p.pad;
  }
  const f16* wrow[WP];
  bool nvalid[WP];
#pragma unroll
  for (int i = 0; i < WP; ++i) {
    const int n = n0 + lrow + i * RPP;
    nvalid[i] = n < p.N;
    wrow[i] = p.w + (size_t)(nvalid[i] ? n : 0) * p.ldw + chunk * 8;
  }

  uint4 xr[XP], wr[WP];
  const uint4 zero4 = make_uint4(0, 0, 0, 0);

  auto load_tile = [&](int kt) {
    if (!GENERIC) {
      const int tapsteps = p.Cin / BK;
      const int tap = kt / tapsteps;
      const int c0 = (kt - tap * tapsteps) * BK + chunk * 8;
      const int r = tap / p.S, s = tap - r * p.S;
#pragma unroll
      for (int i = 0; i < XP; ++i) {
        int hi = hb[i] + r, wi = wb[i] + s;
        const bool ok = mvalid[i] && hi >= 0 && hi < Hv && wi >= 0 && wi < Wv;
        if (p.ups) { hi >>= 1; wi >>= 1; }
        const f16* src = p.x + (size_t)(pixbase[i] + hi * p.Wi + wi) * p.ldx + c0;
        xr[i] = ok ? *reinterpret_cast<const uint4*>(src) : zero4;
      }
#pragma unroll
      for (int i = 0; i < WP; ++i)
        wr[i] = nvalid[i] ? *reinterpret_cast<const uint4*>(wrow[i] + (size_t)kt * BK) : zero4;
    } else {
      const int kg = kt * BK + chunk * 8;
      const bool kok = kg < p.K;
      const int tap = kg / p.Cin;
      const int c0 = kg - tap * p.Cin;
      const int r = tap / p.S, s = tap - r * p.S;
#pragma unroll
      for (int i = 0; i < XP; ++i) {
        int hi = hb[i] + r, wi = wb[i] + s;
        const bool ok = kok && mvalid[i] && hi >= 0 && hi < Hv && wi >= 0 && wi < Wv;
        if (p.ups) { hi >>= 1; wi >>= 1; }
        const f16* src = p.x + (size_t)(pixbase[i] + hi * p.Wi + wi) * p.ldx + c0;
        xr[i] = ok ? *reinterpret_cast<const uint4*>(src) : zero4;
      }
#pragma unroll
      for (int i = 0; i < WP; ++i)
        wr[i] = (kok && nvalid[i]) ? *reinterpret_cast<const uint4*>(wrow[i] + (size_t)kt * BK) : zero4;
    }
  };
  auto store_tile = [&](int stage) {
    char* xs = smem + stage * STAGE;
    char* wsm = xs + XBYTES;
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int row = lrow + i * RPP;
      *reinterpret_cast<uint4*>(xs + row * (BK * 2) + swz_chunk<BK>(row, chunk) * 16) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      const int row = lrow + i * RPP;
      *reinterpret_cast<uint4*>(wsm + row * (BK * 2) + swz_chunk<BK>(row, chunk) * 16) = wr[i];
    }
  };

  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;

  if (kbeg < kend) {
    load_tile(kbeg);
    store_tile(0);
    __syncthreads();
    for (int kt = kbeg; kt < kend; ++kt) {
      const int cur = (kt - kbeg) & 1;
      const bool more = kt + 1 < kend;
      if (more) load_tile(kt + 1);
      const char* xs = smem + cur * STAGE;
      const char* wsm = xs + XBYTES;
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        f16x8 wf[NI], xf[MI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int row = wn * TN + i * 16 + frow;
          wf[i] = *reinterpret_cast<const f16x8*>(wsm + row * (BK * 2) + swz_chunk<BK>(row, kk * 4 + fq) * 16);
        }
#pragma unroll
        for (int j = 0; j < MI; ++j) {
          const int row = wm * TM + j * 16 + frow;
          xf[j] = *reinterpret_cast<const f16x8*>(xs + row * (BK * 2) + swz_chunk<BK>(row, kk * 4 + fq) * 16);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < MI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], xf[j], acc[i][j], 0, 0, 0);
      }
      if (more) store_tile(cur ^ 1);
      __syncthreads();
    }
  }
  f32x4 nob[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) nob[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  static_assert(4 * epilogue_scratch_bytes(TN) <= 2 * STAGE, "epilogue scratch");
  epilogue<NI, MI, TM, TN>(p, acc, m0, n0, wm, wn, frow, fq, z, nob, false, smem + wave * epilogue_scratch_bytes(TN));   // the K loop ends on a barrier
}

// split-K: sum the fp32 partial slabs and apply the epilogue. One thread per 4 output channels.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const KP pp) {
  kernarg_warm<sizeof(KP)>();
  // every scalar the loads below depend on, in one batch (see conv_gemm_dma_kernel)
  KP pl = pp;
  asm volatile("" : "+s"(pl.M), "+s"(pl.N), "+s"(pl.HoWo), "+s"(pl.ldy), "+s"(pl.ldres), "+s"(pl.ld_bias2), "+s"(pl.act),
               "+s"(pl.bias_per_row), "+s"(pl.splitk), "+s"(pl.res_rows));     // integers only: pinned pointers would turn their accesses into flat_ ones
  const KP& p = pl;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = p.N / 4;
  if (idx >= (int64_t)p.M * n4) return;
  const int m = (int)(idx / n4);
  const int n = (int)(idx - (int64_t)m * n4) * 4;
  // every load below is independent: issue them all before the first add (a dependent round trip costs ~0.5 us)
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* src = p.ws + (size_t)m * p.N + n;
  const size_t zs = (size_t)p.M * p.N;
  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f}, b2 = bv;
  f16x4 rv = f16x4{0, 0, 0, 0};
  if (p.bias) {
    if (p.bias_per_row) bv += p.bias[m];
    else bv = *reinterpret_cast<const f32x4*>(p.bias + n);
  }
  if (p.bias2) b2 = *reinterpret_cast<const f32x4*>(p.bias2 + (size_t)(m / p.HoWo) * p.ld_bias2 + n);
  if (p.res) rv = *reinterpret_cast<const f16x4*>(p.res + (size_t)res_row(p, m) * p.ldres + n);
  for (int z0 = 0; z0 < p.splitk; z0 += 8) {
    f32x4 t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      t[u] = (z0 + u < p.splitk) ? *reinterpret_cast<const f32x4*>(src + (size_t)(z0 + u) * zs) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  if (p.wscale) v *= *reinterpret_cast<const f32x4*>(p.wscale + n);       // fp8 weights: per-output-channel scale
  if (p.ln_stats) {                 // LayerNorm folded into the GEMM: see KP::ln_stats
    float r, rm;
    ln_row_scalars(p, m, r, rm);
    v = v * r - *reinterpret_cast<const f32x4*>(p.ln_s + n) * rm;
  }
  v += bv;
  v += b2;
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
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] += (float)rv[t];
  if (p.y32) {
    *reinterpret_cast<f32x4*>(p.y32 + (size_t)m * p.ldy + n) = v;
  } else {
    f16x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = (f16)v[t];
    *reinterpret_cast<f16x4*>(p.y + (size_t)m * p.ldy + n) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// host side: tile / split-K selection and launch
// ------------------------------------------------------------------------------------------------
// launch of one instantiation; the attribute call raises the dynamic-LDS limit once per device
template <typename K>
static int launch_k(K kernel, int smem, DeviceOnce* attr_done, const KP& kp, int tiles, hipStream_t stream, int threads = 256) {
  if (attr_done->need()) {
    SDEO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_done->mark();
  }
  hipLaunchKernelGGL(kernel, dim3(tiles, 1, kp.splitk), dim3(threads), smem, stream, kp);
  SDEO_HIP(hipGetLastError());
  return 0;
}

template <int BM, int BN, int ST, bool UPS, bool WS, bool W8 = false, int KPB = 1, bool MX = false, int EPI = EPI_STAGED>
static int launch_dma(const KP& kp, int tiles, hipStream_t stream) {
  static DeviceOnce done;
  // ring + the LayerNorm row scalars (conv_gemm_dma_kernel: lnsm); an fp8 weight row is 64 bytes, one DMA pass covers 64 rows
  constexpr int smem = ST * (W8 ? BM * 128 + (BN + 63) / 64 * 4096 : (BM + BN) * 128) + BM * 8;
  static_assert(smem <= 160 * 1024, "LDS");
  return launch_k(&conv_gemm_dma_kernel<BM, BN, ST, UPS, WS, W8, KPB, MX, false, EPI>, smem, &done, kp, tiles, stream, WS ? 512 : 256);
}

// multi-problem launch of one instantiation (conv_gemm_dma_kernel MULTI): `tiles` = the sum over the problems
typedef int (*MultiLaunch)(const MPArgs& a, int tiles, hipStream_t stream);
typedef int (*MultiLiveLaunch)(const MPArgsLive& a, int tiles, hipStream_t stream);
template <int BM, int BN, int ST, bool WS, bool LIVE = false>
static int launch_dma_multi(const std::conditional_t<LIVE, MPArgsLive, MPArgs>& a, int tiles, hipStream_t stream) {
  static DeviceOnce done;
  constexpr int smem = ST * (BM + BN) * 128 + BM * 8;
  static_assert(smem <= 160 * 1024, "LDS");
  auto kernel = &conv_gemm_dma_kernel<BM, BN, ST, false, WS, false, 1, false, true, EPI_STAGED, LIVE>;
  if (done.need()) {
    SDEO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    done.mark();
  }
  hipLaunchKernelGGL(kernel, dim3(tiles, 1, 1), dim3(WS ? 512 : 256), smem, stream, a);
  SDEO_HIP(hipGetLastError());
  return 0;
}

template <int BM, int BN>
static int launch_generic(const KP& kp, int tiles, hipStream_t stream) {
  static DeviceOnce done;
  return launch_k(&conv_gemm_kernel<BM, BN, 32, true>, 2 * (BM + BN) * 64, &done, kp, tiles, stream);
}

// The tile table (TileCfg: conv_inl.h).  Adding a tile = one row here (appended: indices are public) + its index in the tests' tile
// lists, which tests/test_tile_table_cpu.py holds against this table (a TK_GENERIC row: FALLBACK_TILES / TILE_BM of
// tests/fallback_cases.py, run by tests/test_fallback_kernel_cpu.py and tests/test_fallback_kernel_gpu.py).  CAPS: CAP_LIGHT makes the row the four-wave instantiation;
// CAP_W8 / CAP_MX add the fp8-weight / block-scaled-fp8 instantiation of the same shape (wave-specialised, no folded Upsample, KPB 1).
// Epilogue kinds (EpiKind; KINDS = the mask of K_* bits of a row): a row has the EPI_DIRECT form of its plain fp16 instantiation when
// the networks can plan it unsplit: the rows the heuristic may pick (no CAP_LIGHT / CAP_GROUPED / CAP_HALO) and the rows the
// committed plan table (tuned_plans_gfx950.json) runs at split-K 1.  The others say so here (KINDS = 0) and in conv_halo.hip (HALO
// against HALO_D): rows 29, 31, 33, 42 and the halo rows 13, 15 - 18, 22 - 25, 36, 38.  A row has a specialised kind of the staged
// family (K_SK split-K slabs, K_GG GEGLU pair, K_GN / K_GNB GroupNorm partials without / with bias2) where the flagship step
// launches that (tile, mode) pair under the committed plan table: the census of tools/epilogue_census.py, recorded in
// tests/golden/epilogue_census.json and held against this table by tests/test_epilogue_kinds_cpu.py.  A launch on a row without
// the kind of its mode (a forced tile, another network, a new plan table) runs the generic staged kernel: epi_kind() is the one
// place that decides.  The folded-Upsample, fp8, block-scaled and multi-problem instantiations and the register-staged fallback
// kernel exist as EPI_STAGED only.
template <int BM, int BN, int ST, int CAPS = 0, int KPB = 1, int KINDS = K_D>
static constexpr TileCfg dma_tile(const char* name) {
  constexpr bool WS = !(CAPS & CAP_LIGHT);
  TileCfg c{BM, BN, 64, ST, TK_DMA, CAPS | (KPB > 1 ? CAP_GROUPED : 0), KPB, 0, 0, name,
            &launch_dma<BM, BN, ST, false, WS, false, KPB>, &launch_dma<BM, BN, ST, true, WS, false, KPB>, nullptr, nullptr, {}};
  c.epi[EPI_STAGED] = c.plain;
  if constexpr ((KINDS & K_D) != 0) c.epi[EPI_DIRECT] = &launch_dma<BM, BN, ST, false, WS, false, KPB, false, EPI_DIRECT>;
  if constexpr ((KINDS & K_SK) != 0) c.epi[EPI_SPLITK] = &launch_dma<BM, BN, ST, false, WS, false, KPB, false, EPI_SPLITK>;
  if constexpr ((KINDS & K_GG) != 0) c.epi[EPI_GEGLU] = &launch_dma<BM, BN, ST, false, WS, false, KPB, false, EPI_GEGLU>;
  if constexpr ((KINDS & K_GN) != 0) c.epi[EPI_GN] = &launch_dma<BM, BN, ST, false, WS, false, KPB, false, EPI_GN>;
  if constexpr ((KINDS & K_GNB) != 0) c.epi[EPI_GN_B2] = &launch_dma<BM, BN, ST, false, WS, false, KPB, false, EPI_GN_B2>;
  if constexpr ((CAPS & CAP_W8) != 0) c.w8 = &launch_dma<BM, BN, ST, false, true, true>;
  if constexpr ((CAPS & CAP_MX) != 0) c.mx = &launch_dma<BM, BN, ST, false, true, false, 1, true>;
  return c;
}
template <int BM, int BN>
static constexpr TileCfg generic_tile(const char* name) {      // the kernel folds the Upsample at run time
  return {BM, BN, 32, 2, TK_GENERIC, 0, 1, 0, 0, name, &launch_generic<BM, BN>, &launch_generic<BM, BN>, nullptr, nullptr, {&launch_generic<BM, BN>}};
}
static const TileCfg kTiles[] = {
    dma_tile<128, 128, 3, CAP_MX>("conv_gemm_dma_kernel<128,128,3>"),
    dma_tile<128, 64, 3, CAP_W8 | CAP_MX>("conv_gemm_dma_kernel<128,64,3>"),
    dma_tile<64, 64, 4, CAP_W8, 1, K_D | K_SK | K_GG>("conv_gemm_dma_kernel<64,64,4>"),
    generic_tile<128, 64>("conv_gemm_kernel<128,64,32,true>"),
    generic_tile<64, 64>("conv_gemm_kernel<64,64,32,true>"),
    dma_tile<256, 128, 3>("conv_gemm_dma_kernel<256,128,3>"),
    // 160-wide weight panels: the channel counts of this model are multiples of 320, and what bounds these kernels is the
    // bytes a CU has to take in per K-step, so the tile menu is built to hit 256 equal workgroups
    dma_tile<64, 160, 3, CAP_W8 | CAP_MX, 1, K_D | K_SK | K_GN>("conv_gemm_dma_kernel<64,160,3>"),
    dma_tile<128, 160, 3>("conv_gemm_dma_kernel<128,160,3>"),      // (its block-scaled fp8 form spills at the 256-register cap)
    dma_tile<256, 160, 3>("conv_gemm_dma_kernel<256,160,3>"),
    dma_tile<32, 160, 4, CAP_W8>("conv_gemm_dma_kernel<32,160,4>"),
    dma_tile<64, 160, 5>("conv_gemm_dma_kernel<64,160,5>"),
    dma_tile<128, 160, 4>("conv_gemm_dma_kernel<128,160,4>"),
    dma_tile<128, 64, 5>("conv_gemm_dma_kernel<128,64,5>"),
    // halo-reuse 3x3 kernels (stride 1, pad 1, Cin % 64 == 0, image a multiple of the patch)
    halo_row(0), halo_row(1), halo_row(2), halo_row(3), halo_row(4), halo_row(5),
    // deep rings: a K-step is bound by bytes in flight per CU (a DMA lands ~1 us after issue under load), so small tiles get
    // as many stages as LDS holds
    dma_tile<64, 64, 8, CAP_W8>("conv_gemm_dma_kernel<64,64,8>"),
    dma_tile<32, 160, 6, CAP_W8>("conv_gemm_dma_kernel<32,160,6>"),
    dma_tile<128, 128, 4, CAP_MX>("conv_gemm_dma_kernel<128,128,4>"),
    // halo kernels with two MFMA waves per SIMD
    halo_row(6), halo_row(7), halo_row(8), halo_row(9),
    // many-tile, short-K problems (ff.net.0.proj, q|k|v: thousands of tiles of 5 - 10 K-steps): a tile's prologue, K loop and
    // epilogue are each ~2 us and serial inside a workgroup (tools/stamps.py), so what overlaps them is OTHER workgroups on the
    // same CU.  Four-wave workgroups (no loader waves: half the register footprint per workgroup) on a two-slot ring fit three
    // or four to a CU.
    dma_tile<128, 64, 2, CAP_LIGHT, 1, K_D | K_GG>("conv_gemm_dma_kernel<128,64,2>"),
    dma_tile<64, 64, 2, CAP_LIGHT>("conv_gemm_dma_kernel<64,64,2>"),
    dma_tile<128, 128, 2, CAP_LIGHT>("conv_gemm_dma_kernel<128,128,2>"),      // (its GEGLU kind measured no gain: DESIGN.md section 32)
    dma_tile<128, 160, 2, CAP_LIGHT, 1, 0>("conv_gemm_dma_kernel<128,160,2>"),
    dma_tile<64, 160, 2, CAP_LIGHT>("conv_gemm_dma_kernel<64,160,2>"),
    dma_tile<32, 160, 2, CAP_LIGHT, 1, 0>("conv_gemm_dma_kernel<32,160,2>"),
    dma_tile<64, 64, 3, CAP_LIGHT>("conv_gemm_dma_kernel<64,64,3>"),
    dma_tile<128, 64, 3, CAP_LIGHT, 1, 0>("conv_gemm_dma_kernel<128,64,3>/4w"),
    // halo kernels with one barrier per filter row (three taps)
    halo_row(10), halo_row(11), halo_row(12), halo_row(13), halo_row(14), halo_row(15), halo_row(16),
    // implicit-GEMM tiles with one barrier per GROUP of K-steps (conv_gemm_dma_kernel KPB): name<BM,BN,STAGES,KPB>
    dma_tile<32, 160, 6, 0, 2, K_D | K_GN>("conv_gemm_dma_kernel<32,160,6,k2>"),
    dma_tile<64, 64, 8, 0, 2, 0>("conv_gemm_dma_kernel<64,64,8,k2>"),
    dma_tile<64, 64, 9, 0, 3>("conv_gemm_dma_kernel<64,64,9,k3>"),
    dma_tile<64, 160, 5, 0, 2>("conv_gemm_dma_kernel<64,160,5,k2>"),
    dma_tile<128, 64, 6, 0, 2>("conv_gemm_dma_kernel<128,64,6,k2>"),
    dma_tile<64, 64, 6, 0, 2>("conv_gemm_dma_kernel<64,64,6,k2>"),
    dma_tile<128, 128, 4, 0, 2>("conv_gemm_dma_kernel<128,128,4,k2>"),
    dma_tile<32, 160, 5, 0, 2>("conv_gemm_dma_kernel<32,160,5,k2>"),
};
static const int kTileCount = (int)std::size(kTiles);
// halo, four-wave and grouped-barrier tiles enter through the measured plan table or a forced plan only
static bool by_plan_only(const TileCfg& c) { return (c.caps & (CAP_HALO | CAP_LIGHT | CAP_GROUPED)) != 0; }
static const int kNumCU = 256;

struct Plan { int tile; int splitk; int nk; int tiles_m, tiles_n; int epi; };      // epi: the EpiKind instantiation of the tile the launch runs (set by prepare)

static bool is_fast(const ConvGemm& p) { return p.Cin % 64 == 0; }
static bool halo_ok(const ConvGemm& p, const TileCfg& c) {
  if (c.kind != TK_HALO) return false;
  return p.R == 3 && p.S == 3 && p.stride == 1 && p.pad == 1 && conv_pad_after(p) == 1 && !p.ups && p.Cin % 64 == 0 && p.act != 3 && !p.bias_per_row &&
         p.Hi % c.ph == 0 && p.Wi % c.pw == 0 && p.Ho == p.Hi && p.Wo == p.Wi;
}
// tiles and K-steps of a plan: a halo tile is a patch of one image and steps through Cin in 64-channel slices (9 taps each)
static int plan_tiles_m(const ConvGemm& p, const TileCfg& c) {
  return c.kind == TK_HALO ? p.B * (p.Hi / c.ph) * (p.Wi / c.pw) : cdiv(p.M, c.bm);
}
static int plan_nk(const ConvGemm& p, const TileCfg& c) { return c.kind == TK_HALO ? p.Cin / 64 : cdiv(p.K, c.bk); }

// tuning hook (tools/tune_gemm.py): force the tile configuration / split-K factor of every following launch
static int g_force_tile = -1, g_force_splitk = 0, g_force_order = -1;
void conv_gemm_debug_force_order(int order) { g_force_order = order; }
void conv_gemm_debug_force(int tile, int splitk) { g_force_tile = tile; g_force_splitk = splitk; }

// plans measured on this device by conv_gemm_autotune (shape -> tile, split-K); consulted before the heuristic
typedef std::array<int, 10> ShapeKey;
static std::map<ShapeKey, std::pair<int, int>> g_tuned;
// (the `ups` slot doubles as the epilogue class: 2 = GEGLU pair epilogue, whose tile menu is restricted)
// (... and + 4 marks fp8 weights: a different kernel family with its own measurements)
static ShapeKey key_of(const ConvGemm& p) {
  return {p.M, p.N, p.K, p.Cin, p.R, p.stride, (p.act == 3 ? 2 : p.ups) + (p.wscale ? 4 : 0) + (p.mx_sx ? 8 : 0), p.Hi, p.Wi, p.B};
}
// the instantiations p's operands need exist for tile c: fp8 weights (the weight-bound shapes: few rows, long K) / block-scaled fp8
// operands (the MFMA-bound GEMMs: many rows)
static bool has_operand_form(const ConvGemm& p, const TileCfg& c) { return (!p.wscale || (c.caps & CAP_W8)) && (!p.mx_sx || (c.caps & CAP_MX)); }

static Plan make_plan(const ConvGemm& p) {
  if (p.plan_B > 0 && p.plan_B != p.B) {
    // a batch prefix of a larger problem (ConvGemm::plan_B) runs that problem's plan on fewer M tiles: tile, split-K factor and
    // K-steps decide the instruction sequence of every output row, the number of M tiles does not
    ConvGemm q = p;
    q.M = p.M / p.B * p.plan_B; q.B = p.plan_B; q.plan_B = 0;
    Plan pl = make_plan(q);
    pl.tiles_m = plan_tiles_m(p, kTiles[pl.tile]);
    return pl;
  }
  Plan best{};
  const bool fast = is_fast(p);
  const int force_tile = p.force_tile >= 0 ? p.force_tile : g_force_tile;
  const int force_sk = p.force_splitk > 0 ? p.force_splitk : g_force_splitk;
  const bool pair = p.act == 3;     // GEGLU epilogue: needs an even number of 16-wide accumulator tiles per wave, no split-K
  if (force_tile < 0 && force_sk <= 0 && fast) {
    auto it = g_tuned.find(key_of(p));
    if (it != g_tuned.end() && !(pair && ((kTiles[it->second.first].bn / 2) % 32 != 0 || it->second.second != 1))) {
      const TileCfg& c = kTiles[it->second.first];
      if ((c.kind != TK_HALO || halo_ok(p, c)) && has_operand_form(p, c))
        return Plan{it->second.first, it->second.second, plan_nk(p, c), plan_tiles_m(p, c), cdiv(p.N, c.bn)};
    }
  }
  float best_t = 1e30f;
  for (int t = 0; t < kTileCount; ++t) {
    const TileCfg& c = kTiles[t];
    auto usable = [&](int ti) {
      const TileCfg& cc = kTiles[ti];
      if (!has_operand_form(p, cc)) return false;
      if (cc.kind == TK_HALO) return halo_ok(p, cc);
      return (cc.kind == TK_DMA) == fast && !(pair && (cc.bn / 2) % 32 != 0);
    };
    if (!usable(t)) continue;
    if (by_plan_only(c) && force_tile != t) continue;
    if (force_tile >= 0 && usable(force_tile) && force_tile != t) continue;
    const int tmn = plan_tiles_m(p, c), tnn = cdiv(p.N, c.bn);
    const int tiles = tmn * tnn;
    const int nk = plan_nk(p, c);
    const bool halo = c.kind == TK_HALO;
    // candidate split-K factors: 1 and whatever gives every CU one or two workgroups
    int cands[3] = {1, 0, 0};
    int ncand = 1;
    if (tiles < kNumCU && (nk >= 8 || halo) && !pair) {
      for (int fill = 1; fill <= 2; ++fill) {
        int sk = fill * kNumCU / tiles;
        if (sk > nk / (halo ? 1 : 4)) sk = nk / (halo ? 1 : 4);
        if (sk > 16) sk = 16;
        if (sk >= 2 && sk != cands[ncand - 1]) cands[ncand++] = sk;
      }
    }
    if (force_sk > 0 && !pair) { cands[0] = force_sk > nk ? nk : force_sk; ncand = 1; }
    for (int ci = 0; ci < ncand; ++ci) {
      int sk = cands[ci];
      const int per = cdiv(nk, sk);
      sk = cdiv(nk, per);
      // time model in clocks: a CU takes in ~28 B/clk through the vector-memory path whatever
      // the source, so a K-step of a workgroup costs max((bm+bn) * 128 B / 28, MFMA time of the tile); the workgroups
      // are spread over 256 CUs; ~9k clocks of launch / prologue / epilogue per kernel
      const float rounds = (float)cdiv(tiles * sk, kNumCU);
      const float step_clk = halo ? fmaxf(((float)c.bm * 0.16f + c.bn) * 4.57f, (float)(c.bm * c.bn) / 31.8f)
                                  : fmaxf((float)(c.bm + c.bn) * 4.57f, (float)(c.bm * c.bn) / 31.8f);
      float tcost = 9000.f + rounds * ((float)per * (halo ? 9.f : 1.f) * step_clk + 1500.f);
      if (sk > 1) tcost += 8000.f + ((float)sk + 1.f) * p.M * p.N * 4.0f / 1700.f;   // reduce launch + fp32 slabs at ~4 TB/s
      if (tcost < best_t) { best_t = tcost; best = Plan{t, sk, nk, tmn, tnn}; }
    }
  }
  return best;
}

// block-scaled fp8 operands are addressed as an fp16 problem of half the length (KP::mx_sx): every plan query sees that view
static ConvGemm mx_view(const ConvGemm& p0) {
  ConvGemm p = p0;
  if (p.mx_sx) { p.K /= 2; p.Cin /= 2; p.ldx /= 2; p.ldw /= 2; }
  return p;
}

// columns per epilogue strip of a plan: the wave tile width of the implicit-GEMM kernels, the whole tile of the halo kernel
static int plan_tn(const Plan& pl) { return kTiles[pl.tile].kind == TK_HALO ? kTiles[pl.tile].bn : kTiles[pl.tile].bn / 2; }

int conv_gemm_stats_strips(const ConvGemm& p0) {
  const ConvGemm p = mx_view(p0);
  const Plan pl = make_plan(p);
  return pl.splitk == 1 ? cdiv(p.N, plan_tn(pl)) : 0;
}

bool conv_gemm_plan_is_halo(const ConvGemm& p) { return kTiles[make_plan(mx_view(p)).tile].kind == TK_HALO; }

// GroupNorm partials from the epilogue (KP::gn_out): entries per image the plan of p writes for groups of `cpg` channels, or 0 when it
// cannot (split-K, a strip that cuts a group, a tile that straddles two images, the register-staged fallback kernel, an epilogue
// that is not the LDS-transposed one)
static int gn_slots_of(const ConvGemm& p, int cpg);
int conv_gemm_gn_slots(const ConvGemm& p0, int cpg) { return gn_slots_of(mx_view(p0), cpg); }
static int gn_slots_of(const ConvGemm& p, int cpg) {       // p: the view the kernels see (mx_view)
  if (cpg <= 0 || p.N % cpg || p.act == 3 || p.y32 || !p.y || p.bias_per_row || p.stats_out) return 0;
  const Plan pl = make_plan(p);
  const TileCfg& c = kTiles[pl.tile];
  if (pl.splitk != 1 || c.kind == TK_GENERIC || plan_tn(pl) % cpg) return 0;
  if (p.N % 8 || p.ldy % 8 || (reinterpret_cast<uintptr_t>(p.y) & 15) || (p.res && (p.ldres % 8 || (reinterpret_cast<uintptr_t>(p.res) & 15)))) return 0;
  if (c.kind == TK_HALO) return (p.Hi / c.ph) * (p.Wi / c.pw);
  const int hw = p.Ho * p.Wo;
  return hw % c.bm == 0 ? hw / c.bm : 0;
}

size_t conv_gemm_workspace_bytes(const ConvGemm& p0) {
  const ConvGemm p = mx_view(p0);
  const Plan pl = make_plan(p);
  return pl.splitk > 1 ? (size_t)pl.splitk * p.M * p.N * sizeof(float) : 0;
}

const char* conv_gemm_kernel_name(const ConvGemm& p) { return kTiles[make_plan(mx_view(p)).tile].name; }
int conv_gemm_plan_splitk(const ConvGemm& p) { return make_plan(mx_view(p)).splitk; }

void conv_gemm_query_plan(const ConvGemm& p0, int key[10], int* tile, int* splitk) {
  const ConvGemm p = mx_view(p0);
  const ShapeKey k = key_of(p);
  for (int i = 0; i < 10; ++i) key[i] = k[i];
  const Plan pl = make_plan(p);
  *tile = pl.tile;
  *splitk = pl.splitk;
}

// (tile, split-K) of the last problem conv_gemm() launched: host-side only, read by the tests through sdeo_debug_last_gemm_plan
static int g_last_tile = -1, g_last_splitk = 0, g_last_epilogue = -1;
void conv_gemm_last_plan(int* tile, int* splitk) { *tile = g_last_tile; *splitk = g_last_splitk; }
int conv_gemm_last_epilogue() { return g_last_epilogue < 0 ? -1 : g_last_epilogue == EPI_DIRECT ? EPI_DIRECT : EPI_STAGED; }       // the family of that launch
int conv_gemm_last_epilogue_mode() { return g_last_epilogue >= EPI_SPLITK ? g_last_epilogue : 0; }      // its kind within the staged family (0 = generic)
static int g_force_epi_mode = -1;
void conv_gemm_debug_force_epilogue_mode(int mode) { g_force_epi_mode = mode; }
int conv_gemm_tile_has_epilogue_mode(int tile, int mode) {
  return tile >= 0 && tile < kTileCount && mode >= 0 && mode < EPI_KINDS && mode != EPI_DIRECT && kTiles[tile].epi[mode] != nullptr;
}

// Census of the launches dispatch() made: (tile, split-K, operand form, EpiKind run, mode flags of the problem) -> count.  Host
// side, plain integers; tools/epilogue_census.py reads and clears it.  form: 0 plain, 1 folded Upsample, 2 fp8 weights,
// 3 block-scaled fp8, 4 multi-problem.  flags: act | 8 bias2 | 16 GroupNorm partials | 32 row statistics | 64 LayerNorm fold |
// 128 residual | 256 coalesced.
static std::map<std::array<int, 5>, int> g_census;
static int census_flags(const KP& kp) {
  return kp.act | (kp.bias2 ? 8 : 0) | (kp.gn_out ? 16 : 0) | (kp.stats_out ? 32 : 0) | (kp.ln_stats ? 64 : 0) | (kp.res ? 128 : 0) | (kp.coalesce ? 256 : 0);
}
int conv_gemm_epilogue_census(int* rows6, int cap, int clear) {       // rows of (tile, split-K, form, kind, flags, count); returns their number
  int n = 0;
  for (auto& kv : g_census) {
    if (n < cap) { for (int i = 0; i < 5; ++i) rows6[n * 6 + i] = kv.first[i]; rows6[n * 6 + 5] = kv.second; }
    ++n;
  }
  if (clear) g_census.clear();
  return n;
}

// Which launches run the EPI_DIRECT instantiation of their tile (epilogue_direct): those the LDS-transposed epilogue would serve
// (kp.coalesce: unsplit, fp16 output, N % 8 == 0, 16-byte aligned output and residual rows) in a plain mode.  The GEGLU pair
// epilogue, the GroupNorm partials and the per-image bias2 (slower direct than staged when measured) stay staged, split-K launches keep the plain channel order (their slabs and
// splitk_reduce_kernel are untouched), and the folded Upsample, fp8 and block-scaled kernels have no direct form.
// SDEO_EPI_DIRECT=0 (measurement) keeps every launch on the staged epilogue.
static int direct_ok(const ConvGemm& p, const KP& kp, const TileCfg& c) {
  static const int on = [] { const char* e = getenv("SDEO_EPI_DIRECT"); return e ? atoi(e) : 1; }();
  return on && c.epi[EPI_DIRECT] && kp.coalesce && p.act != 3 && !p.gn_out && !p.bias2 && !p.ups && !p.wscale && !p.mx_sx;
}
// The kind of the staged family whose mode the problem in kp has (EpiMode, conv_inl.h), EPI_STAGED when it has none: what a
// specialised kernel may assume is exactly what is tested here.  The fp8, block-scaled and folded-Upsample instantiations exist
// as EPI_STAGED only.
static int staged_mode(const KP& kp) {
  if (kp.wscale || kp.mx_sx || kp.ups) return EPI_STAGED;
  if (kp.splitk > 1) return EPI_SPLITK;
  if (!kp.coalesce || kp.stats_out) return EPI_STAGED;
  if (kp.act == 3) return EPI_GEGLU;
  if (kp.ln_stats || kp.act != 0 || !kp.gn_out) return EPI_STAGED;
  return kp.bias2 ? EPI_GN_B2 : EPI_GN;
}
// The EpiKind a launch runs: the one place that decides.  A row without the instantiation of the problem's mode runs the generic
// kernel.  SDEO_EPI_KINDS=0 (measurement) and conv_gemm_debug_force_epilogue_mode(0) keep every non-direct launch on it.
static int epi_kind(const ConvGemm& p, const KP& kp, const Plan& pl) {
  static const int kinds_on = [] { const char* e = getenv("SDEO_EPI_KINDS"); return e ? atoi(e) : 1; }();
  const TileCfg& c = kTiles[pl.tile];
  if (direct_ok(p, kp, c)) return EPI_DIRECT;
  if (!kinds_on || g_force_epi_mode == 0) return EPI_STAGED;
  const int k = staged_mode(kp);
  return c.epi[k] ? k : EPI_STAGED;
}

// argument checks + plan + kernel parameters of one problem
static int prepare(const ConvGemm& p, Plan& pl, KP& kp) {
  SDEO_CHECK(p.x && p.w && (p.y || p.y32), "conv_gemm: null operand");
  SDEO_CHECK(p.M > 0 && p.N > 0 && p.K > 0, "conv_gemm: empty problem M=%d N=%d K=%d", p.M, p.N, p.K);
  SDEO_CHECK(p.act >= 0 && p.act <= 5, "conv_gemm: act=%d unsupported (0 none, 1 SiLU, 2 quick-GELU, 3 GEGLU pair, 4 ReLU, 5 erf GELU)", p.act);
  SDEO_CHECK(p.act != 5 || !p.bias2, "conv_gemm: act 5 (erf GELU) is not built with a per-image bias2");
  SDEO_CHECK(p.N % 4 == 0, "conv_gemm: N=%d must be a multiple of 4", p.N);
  SDEO_CHECK(p.Cin % 8 == 0 && p.ldx % 8 == 0 && p.ldw % 8 == 0, "conv_gemm: Cin=%d ldx=%d ldw=%d must be multiples of 8",
             p.Cin, p.ldx, p.ldw);
  SDEO_CHECK(p.K == p.R * p.S * p.Cin, "conv_gemm: K=%d != R*S*Cin=%d", p.K, p.R * p.S * p.Cin);
  SDEO_CHECK(p.R >= 1 && p.R <= 4 && p.S >= 1 && p.S <= 4, "conv_gemm: filter %dx%d unsupported (1..4)", p.R, p.S);
  SDEO_CHECK(p.ldw >= p.K, "conv_gemm: ldw=%d < K=%d", p.ldw, p.K);
  SDEO_CHECK(p.M == p.B * p.Ho * p.Wo, "conv_gemm: M=%d != B*Ho*Wo=%d", p.M, p.B * p.Ho * p.Wo);
  SDEO_CHECK(p.ldy % 4 == 0 && p.ldy >= (p.act == 3 ? p.N / 2 : p.N), "conv_gemm: ldy=%d", p.ldy);
  SDEO_CHECK(!p.res || p.ldres % 4 == 0, "conv_gemm: ldres=%d", p.ldres);
  SDEO_CHECK(p.res_rows == 0 || (p.res && p.res_rows <= p.M && 2 * p.res_rows >= p.M),
             "conv_gemm: res_rows=%d must lie in [M/2, M] (M=%d) and needs a residual", p.res_rows, p.M);
  SDEO_CHECK(p.plan_B == 0 || (p.plan_B >= p.B && p.M % p.B == 0), "conv_gemm: plan_B=%d is smaller than B=%d", p.plan_B, p.B);
  SDEO_CHECK((reinterpret_cast<uintptr_t>(p.x) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0,
             "conv_gemm: operands must be 16-byte aligned");
  {
    const int Hv = p.ups ? 2 * p.Hi : p.Hi, Wv = p.ups ? 2 * p.Wi : p.Wi;
    // pad = top / left, pad_after = bottom / right: the kernels place tap (0, 0) of output (ho, wo) at (ho stride - pad, wo stride - pad)
    // and read every tap outside [0, Hv) x [0, Wv) as zero, so the bottom / right padding only enters through Ho / Wo
    const int pa = conv_pad_after(p);
    SDEO_CHECK(p.pad >= 0 && pa >= 0 && p.pad < p.R && pa < p.R && p.pad < p.S && pa < p.S,
               "conv_gemm: padding (%d, %d) out of range for a %dx%d filter", p.pad, pa, p.R, p.S);
    SDEO_CHECK(pa == p.pad || p.K != p.Cin, "conv_gemm: asymmetric padding needs a filter larger than 1x1");
    SDEO_CHECK((Hv + p.pad + pa - p.R) / p.stride + 1 == p.Ho && (Wv + p.pad + pa - p.S) / p.stride + 1 == p.Wo,
               "conv_gemm: geometry mismatch Hi=%d Wi=%d -> Ho=%d Wo=%d (R=%d S=%d stride=%d pad=%d/%d ups=%d)", p.Hi, p.Wi,
               p.Ho, p.Wo, p.R, p.S, p.stride, p.pad, pa, p.ups);
  }
  if (p.act == 3)
    SDEO_CHECK(p.N % 32 == 0 && p.y && !p.y32 && !p.res && !p.bias2 && !p.bias_per_row && p.ldy >= p.N / 2 && p.scale == 1.0f,
               "conv_gemm: GEGLU epilogue needs N %% 32 == 0 (N=%d), fp16 output with ldy >= N/2 and no residual / bias2", p.N);
  if (p.wscale)
    SDEO_CHECK(p.Cin % 64 == 0 && !p.ups && p.ldw % 16 == 0 && !p.bias_per_row,
               "conv_gemm: fp8 weights need Cin %% 64 == 0 (Cin=%d), no folded upsample and 16-byte aligned rows (ldw=%d bytes)", p.Cin, p.ldw);
  pl = make_plan(p);
  SDEO_CHECK(!p.wscale || (kTiles[pl.tile].caps & CAP_W8), "conv_gemm: no fp8-weight plan for this shape");
  SDEO_CHECK(!p.mx_sx || (kTiles[pl.tile].caps & CAP_MX), "conv_gemm: no block-scaled fp8 plan for this shape");
  SDEO_CHECK(p.act != 3 || (pl.splitk == 1 && (kTiles[pl.tile].bn / 2) % 32 == 0), "conv_gemm: no GEGLU-capable plan");
  kp = KP{};
  kp.x = p.x; kp.w = p.w; kp.y = p.y; kp.y32 = p.y32; kp.bias = p.bias; kp.bias2 = p.bias2; kp.res = p.res;
  kp.ws = p.workspace;
  kp.M = p.M; kp.N = p.N; kp.K = p.K;
  kp.Hi = p.Hi; kp.Wi = p.Wi; kp.Cin = p.Cin; kp.Ho = p.Ho; kp.Wo = p.Wo; kp.S = p.S; kp.stride = p.stride; kp.pad = p.pad;
  kp.ups = p.ups; kp.HoWo = p.Ho * p.Wo;
  kp.ldx = p.ldx; kp.ldw = p.ldw; kp.ldy = p.ldy; kp.ldres = p.ldres; kp.ld_bias2 = p.ld_bias2;
  kp.res_rows = p.res_rows > 0 ? p.res_rows : p.M;
  kp.act = p.act; kp.bias_per_row = p.bias_per_row; kp.scale = p.scale;
  kp.wscale = p.wscale;
  if (p.mx_sx) {       // (p arrives with K, Cin, ldx, ldw already halved: conv_gemm())
    SDEO_CHECK(p.mx_sw && p.R == 1 && p.S == 1 && p.stride == 1 && !p.ups && !p.wscale && p.Cin % 64 == 0 && !p.bias_per_row,
               "conv_gemm: block-scaled fp8 operands go with a plain GEMM whose K is a multiple of 128");
    SDEO_CHECK(p.mx_ldsx >= p.K / 16 && p.mx_ldsw >= p.K / 16, "conv_gemm: scale rows too short (%d, %d < %d)", p.mx_ldsx, p.mx_ldsw, p.K / 16);
    kp.mx_sx = p.mx_sx; kp.mx_sw = p.mx_sw; kp.mx_ldsx = p.mx_ldsx; kp.mx_ldsw = p.mx_ldsw;
  }
  if (p.ln_stats) {
    SDEO_CHECK(p.ln_s && p.ln_strips >= 1 && p.ln_ld >= p.ln_strips && p.ln_c > 0, "conv_gemm: incomplete LayerNorm-fold arguments");
    SDEO_CHECK(!p.bias_per_row && !p.y32, "conv_gemm: the LayerNorm fold applies to row-major fp16 products only");
    SDEO_CHECK(p.K == p.Cin && p.stride == 1 && !p.ups, "conv_gemm: the LayerNorm fold needs one input row per output row (a %dx%d filter mixes rows with different statistics)", p.R, p.S);
    kp.ln_stats = p.ln_stats; kp.ln_s = p.ln_s; kp.ln_strips = p.ln_strips; kp.ln_ld = p.ln_ld;
    kp.ln_invc = 1.0f / (float)p.ln_c; kp.ln_eps = p.ln_eps;
  }
  if (p.stats_out) {
    const int strips = pl.splitk == 1 ? cdiv(p.N, plan_tn(pl)) : 0;
    SDEO_CHECK(strips >= 1 && p.stats_ld >= strips && p.y && !p.y32 && p.act != 3,
               "conv_gemm: row statistics need an unsplit fp16 plan (strips %d, stats_ld %d)", strips, p.stats_ld);
    kp.stats_out = p.stats_out; kp.stats_ld = p.stats_ld;
  }
  if (p.gn_out) {
    const int slots = gn_slots_of(p, p.gn_cpg);
    SDEO_CHECK(slots > 0 && slots == p.gn_slots && p.gn_groups * p.gn_cpg == p.N,
               "conv_gemm: GroupNorm partials need an unsplit fp16 plan whose strips cover whole groups (slots %d, expected %d)", slots, p.gn_slots);
    kp.gn_out = p.gn_out; kp.gn_cpg = p.gn_cpg; kp.gn_slots = p.gn_slots; kp.gn_groups = p.gn_groups;
  }
  kp.nk = pl.nk; kp.splitk = pl.splitk; kp.nk_per_split = cdiv(pl.nk, pl.splitk);
  kp.tiles_m = pl.tiles_m; kp.tiles_n = pl.tiles_n;
  pl.epi = EPI_STAGED;
  {
    // Each of the 8 XCDs has a private L2 and gets a contiguous run of tiles.  With N fastest every activation row is
    // fetched by one XCD but every XCD streams all the weights; with M fastest it is the other way round (each XCD
    // sees about tiles_n/8 weight panels and every activation row min(8, tiles_n) times).  Pick the cheaper fetch.
    const double xb = (double)p.M * p.Cin * 2.0 * (p.R * p.S > 1 ? 1.3 : 1.0), wb = (double)p.N * p.K * 2.0;
    const double cost_n_fast = xb + 8.0 * wb;
    const double cost_m_fast = (pl.tiles_n < 8 ? pl.tiles_n : 8) * xb + wb * (pl.tiles_n < 8 ? 1.6 : 1.0);
#ifdef SDEO_DEBUG_KERNELS
    { static const int dbg = [] { const char* e = getenv("SDEO_DBG_GEMM"); return e ? atoi(e) : 0; }(); kp.dbg = dbg; }
#endif
    kp.n_fastest = g_force_order >= 0 ? g_force_order : (cost_n_fast < cost_m_fast ? 1 : 0);
    static const int epi = [] { const char* e = getenv("SDEO_EPI_COALESCE"); return e ? atoi(e) : 1; }();
    kp.coalesce = epi && p.y && !p.y32 && pl.splitk == 1 && !p.bias_per_row && p.N % (p.act == 3 ? 16 : 8) == 0 && p.ldy % 8 == 0 &&
                  (reinterpret_cast<uintptr_t>(p.y) & 15) == 0 &&
                  (!p.res || (p.ldres % 8 == 0 && (reinterpret_cast<uintptr_t>(p.res) & 15) == 0));
    SDEO_CHECK(!p.gn_out || kp.coalesce, "conv_gemm: GroupNorm partials need the LDS-transposed epilogue");
  }
  if (pl.splitk > 1) {
    const size_t need = (size_t)pl.splitk * p.M * p.N * sizeof(float);
    SDEO_CHECK(p.workspace && p.workspace_bytes >= need, "conv_gemm: split-K workspace too small (%zu < %zu)",
               p.workspace_bytes, need);
  }
  if (kTiles[pl.tile].kind == TK_HALO) SDEO_CHECK(halo_ok(p, kTiles[pl.tile]), "conv_gemm: halo plan on an ineligible problem");
  pl.epi = epi_kind(p, kp, pl);
  return 0;
}

// launch the problem in kp at plan `pl`: the row's instantiation for these operands, then the split-K reduce
static int dispatch(const Plan& pl, int ups, bool w8, const KP& kp, hipStream_t stream) {
  if (pl.tile < 0 || pl.tile >= kTileCount) return fail("conv_gemm: bad tile %d", pl.tile);
  const TileCfg& c = kTiles[pl.tile];
  if (pl.epi < 0 || pl.epi >= EPI_KINDS) return fail("conv_gemm: bad epilogue kind %d", pl.epi);
  if (pl.epi != EPI_STAGED && (kp.mx_sx || w8 || ups || !c.epi[pl.epi]))
    return fail("conv_gemm: tile %d has no %s instantiation for this launch", pl.tile, pl.epi == EPI_DIRECT ? "register-direct" : "specialised staged");
  if (pl.epi >= EPI_SPLITK && pl.epi != staged_mode(kp)) return fail("conv_gemm: epilogue kind %d does not match the problem's mode (%d)", pl.epi, staged_mode(kp));
  const TileLaunch launch = pl.epi != EPI_STAGED ? c.epi[pl.epi] : kp.mx_sx ? c.mx : w8 ? c.w8 : ups ? c.ups : c.plain;
  if (!launch) return fail("conv_gemm: tile %d has no %s instantiation", pl.tile, kp.mx_sx ? "block-scaled fp8" : w8 ? "fp8-weight" : "folded-upsample");
  ++g_census[{pl.tile, pl.splitk, kp.mx_sx ? 3 : w8 ? 2 : ups ? 1 : 0, pl.epi, census_flags(kp)}];
  if (int rc = launch(kp, pl.tiles_m * pl.tiles_n, stream)) return rc;
  if (pl.splitk > 1) {
    const int64_t n = (int64_t)kp.M * (kp.N / 4);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, kp);
    SDEO_HIP(hipGetLastError());
  }
  return 0;
}

int conv_gemm(const ConvGemm& p0, hipStream_t stream) {
  if (p0.mx_sx)        // fp8 codes addressed as an fp16 problem of half the length (KP::mx_sx)
    SDEO_CHECK(p0.K % 128 == 0 && p0.ldx % 16 == 0 && p0.ldw % 16 == 0 && p0.K == p0.Cin, "conv_gemm: block-scaled fp8 GEMM needs K %% 128 == 0 (K=%d, ldx=%d, ldw=%d)", p0.K, p0.ldx, p0.ldw);
  const ConvGemm p = mx_view(p0);
  Plan pl;
  KP kp{};
  if (int rc = prepare(p, pl, kp)) return rc;
  g_last_tile = pl.tile; g_last_splitk = pl.splitk; g_last_epilogue = pl.epi;
  return dispatch(pl, p.ups, p.wscale != nullptr, kp, stream);
}

// The rows of kTiles that have a multi-problem instantiation (the table itself is untouched: a multi-problem launch is asked for by
// name, never planned).  Each costs one more kernel, so there are as many as there are users.
// launch_live: the live-row instantiation (conv_gemm_multi_launch_live), where a user exists: the zero convs' tile.
struct MultiTile { int tile, bm, bn, stages; bool light; MultiLaunch launch; const char* name; MultiLiveLaunch launch_live; };
static const MultiTile kMultiTiles[] = {
    {2, 64, 64, 4, false, &launch_dma_multi<64, 64, 4, true>, "conv_gemm_dma_kernel<64,64,4> multi", nullptr},
    {6, 64, 160, 3, false, &launch_dma_multi<64, 160, 3, true>, "conv_gemm_dma_kernel<64,160,3> multi", nullptr},
    {26, 128, 64, 2, true, &launch_dma_multi<128, 64, 2, false>, "conv_gemm_dma_kernel<128,64,2> multi", &launch_dma_multi<128, 64, 2, false, true>},
};
static const MultiTile* multi_tile(int tile) {
  for (const MultiTile& m : kMultiTiles) {
    const TileCfg& c = kTiles[m.tile];
    if (m.tile == tile && c.kind == TK_DMA && c.bm == m.bm && c.bn == m.bn && c.stages == m.stages && c.kpb == 1 &&
        ((c.caps & CAP_LIGHT) != 0) == m.light)
      return &m;
  }
  return nullptr;
}

int conv_gemm_multi_plan(const std::vector<ConvGemm>& ps, int tile, ConvGemmMultiPlan* out) {
  *out = ConvGemmMultiPlan{};
  // refusals that need no look at the operands come first
  SDEO_CHECK(!ps.empty() && (int)ps.size() <= kMultiMax, "conv_gemm_multi: %d problems in one launch (1..%d)", (int)ps.size(), kMultiMax);
  for (const ConvGemm& p : ps) {
    if (tile < 0) tile = p.force_tile;
    SDEO_CHECK(p.force_tile < 0 || p.force_tile == tile, "conv_gemm_multi: mixed tiles (%d and %d): one tile serves all problems of a launch", tile, p.force_tile);
    SDEO_CHECK(p.force_splitk <= 1, "conv_gemm_multi: a split-K plan (factor %d) cannot be part of a multi-problem launch", p.force_splitk);
  }
  const MultiTile* mt = multi_tile(tile);
  SDEO_CHECK(mt, "conv_gemm_multi: tile %d has no multi-problem instantiation", tile);
  MPTable tab{};
  int total = 0;
  for (size_t i = 0; i < ps.size(); ++i) {
    ConvGemm p = ps[i];
    SDEO_CHECK(!p.mx_sx && !p.wscale, "conv_gemm_multi: problem %d: fp16 weights only", (int)i);
    SDEO_CHECK(!p.gn_out && !p.stats_out && !p.ln_stats, "conv_gemm_multi: problem %d: no GroupNorm-partial, row-statistics or LayerNorm-fold epilogue", (int)i);
    SDEO_CHECK(p.act != 3 && !p.ups && p.plan_B == 0, "conv_gemm_multi: problem %d: no GEGLU pair, folded upsample or batch-prefix plan", (int)i);
    SDEO_CHECK(is_fast(p), "conv_gemm_multi: problem %d: Cin=%d must be a multiple of 64", (int)i, p.Cin);
    p.force_tile = tile; p.force_splitk = 1;
    Plan pl;
    if (int rc = prepare(p, pl, tab.kp[i])) return rc;
    SDEO_CHECK(pl.tile == tile && pl.splitk == 1, "conv_gemm_multi: problem %d cannot run unsplit on tile %d", (int)i, tile);
    total += pl.tiles_m * pl.tiles_n;
    tab.prefix[i] = total;
    out->scale[i] = p.scale;
    out->flops += 2.0 * p.M * p.N * (double)p.K;
    out->bytes += 2.0 * ((double)p.M * p.Cin + (double)p.N * p.K + (double)p.M * p.N);
  }
  for (int i = (int)ps.size(); i < kMultiMax; ++i) tab.prefix[i] = 0x7fffffff;
  out->tile = tile; out->count = (int)ps.size(); out->tiles = total; out->name = mt->name;
  out->table.assign(reinterpret_cast<const char*>(&tab), reinterpret_cast<const char*>(&tab) + sizeof(tab));
  return 0;
}

int conv_gemm_multi_launch(const ConvGemmMultiPlan& pl, const void* table_dev, const float* scales, hipStream_t stream) {
  const MultiTile* mt = multi_tile(pl.tile);
  SDEO_CHECK(mt && pl.count >= 1 && pl.count <= kMultiMax && pl.tiles > 0 && pl.table.size() == sizeof(MPTable), "conv_gemm_multi: launch of an unplanned table");
  SDEO_CHECK(table_dev && (reinterpret_cast<uintptr_t>(table_dev) & 15) == 0, "conv_gemm_multi: the device table must be 16-byte aligned");
  MPArgs a{};
  a.tab = static_cast<const MPTable*>(table_dev);
  a.count = pl.count;
  for (int i = 0; i < pl.count; ++i) a.scale[i] = scales ? scales[i] : pl.scale[i];
  g_last_tile = pl.tile; g_last_splitk = 1; g_last_epilogue = EPI_STAGED;
  ++g_census[{pl.tile, 1, 4, EPI_STAGED, 0}];
  return mt->launch(a, pl.tiles, stream);
}

int conv_gemm_multi_launch_live(const ConvGemmMultiPlan& pl, const void* table_dev, const float* scales, const int* m_live, hipStream_t stream) {
  const MultiTile* mt = multi_tile(pl.tile);
  SDEO_CHECK(mt && pl.count >= 1 && pl.count <= kMultiMax && pl.tiles > 0 && pl.table.size() == sizeof(MPTable), "conv_gemm_multi: launch of an unplanned table");
  SDEO_CHECK(mt->launch_live, "conv_gemm_multi: tile %d has no live-row instantiation", pl.tile);
  SDEO_CHECK(table_dev && (reinterpret_cast<uintptr_t>(table_dev) & 15) == 0, "conv_gemm_multi: the device table must be 16-byte aligned");
  SDEO_CHECK(m_live, "conv_gemm_multi: live-row counts required");
  const MPTable* tab = reinterpret_cast<const MPTable*>(pl.table.data());
  MPArgsLive a{};
  a.tab = static_cast<const MPTable*>(table_dev);
  a.count = pl.count;
  for (int i = 0; i < pl.count; ++i) {
    const KP& kp = tab->kp[i];
    SDEO_CHECK(m_live[i] >= 0 && m_live[i] <= kp.M, "conv_gemm_multi: problem %d: %d live rows of %d", i, m_live[i], kp.M);
    // the pass-through of the dead rows moves 8 bytes per lane
    SDEO_CHECK(kp.y && !kp.y32 && kp.res_rows == kp.M && kp.N % 4 == 0 && kp.ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(kp.y) & 7) == 0 &&
                   (!kp.res || (kp.ldres % 4 == 0 && (reinterpret_cast<uintptr_t>(kp.res) & 7) == 0)),
               "conv_gemm_multi: problem %d: the live-row form needs an fp16 output and a one-to-one residual, 8-byte aligned, N / ldy / ldres multiples of 4", i);
    a.scale[i] = scales ? scales[i] : pl.scale[i];
    a.m_live[i] = m_live[i];
  }
  g_last_tile = pl.tile; g_last_splitk = 1; g_last_epilogue = EPI_STAGED;
  return mt->launch_live(a, pl.tiles, stream);
}

int conv_gemm_tile_info(int tile, int* kind, int* bm, int* bn, int* stages, int* caps, const char** name) {
  if (tile < 0 || tile >= kTileCount) return 1;
  const TileCfg& c = kTiles[tile];
  *kind = c.kind; *bm = c.bm; *bn = c.bn; *stages = c.stages; *caps = c.caps; *name = c.name;
  return 0;
}

int conv_gemm_read_stamps(unsigned long long* out, int n) {
  SDEO_HIP(hipDeviceSynchronize());
  SDEO_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * (size_t)(n < kStampWGs * kStampSlots ? n : kStampWGs * kStampSlots)));
  return 0;
}

// tuned-plan table I/O (stablediffusioneo_amd/tuned_plans_gfx950.json is produced by tools/tune_plans.py on an MI355X and
// loaded at start-up, so production runs neither re-measure nor vary their plans from run to run)
void conv_gemm_set_tuned(const int key[10], int tile, int splitk) {
  ShapeKey k;
  for (int i = 0; i < 10; ++i) k[i] = key[i];
  if (tile >= 0 && tile < kTileCount && kTiles[tile].kind != TK_GENERIC && splitk >= 1) g_tuned[k] = {tile, splitk};
}

std::string conv_gemm_tuned_json() {
  std::string out = "[";
  char buf[256];
  bool first = true;
  for (auto& kv : g_tuned) {
    snprintf(buf, sizeof(buf), "%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", first ? "" : ",", kv.first[0], kv.first[1], kv.first[2],
             kv.first[3], kv.first[4], kv.first[5], kv.first[6], kv.first[7], kv.first[8], kv.first[9], kv.second.first,
             kv.second.second);
    out += buf;
    first = false;
  }
  return out + "]";
}

// ------------------------------------------------------------------------------------------------
// autotune: measure every (tile, split-K) candidate for one problem on the device and remember the fastest.
// Called once per distinct shape from sdeo_configure (never on the hot path, never under graph capture).
// ------------------------------------------------------------------------------------------------
static const size_t kTuneWorkspaceCap = (size_t)256 << 20;

size_t conv_gemm_autotune_workspace_bytes(const ConvGemm& p) {
  if (!is_fast(p)) return conv_gemm_workspace_bytes(p);
  const size_t per = (size_t)p.M * p.N * sizeof(float);
  size_t want = per * 16;
  if (want > kTuneWorkspaceCap) want = kTuneWorkspaceCap / per * per;
  const size_t heur = conv_gemm_workspace_bytes(p);
  return want > heur ? want : heur;
}

int conv_gemm_autotune(const ConvGemm& p, hipStream_t stream) {
  if (p.mx_sx) return 0;                                   // block-scaled fp8 GEMMs run on the heuristic plan among their few tiles
  if (!is_fast(p) || g_force_tile >= 0 || g_force_splitk > 0) return 0;
  const ShapeKey key = key_of(p);
  if (g_tuned.count(key)) return 0;
  static const int sks[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20};
  hipEvent_t a, b;
  SDEO_HIP(hipEventCreate(&a));
  SDEO_HIP(hipEventCreate(&b));
  float best = 1e30f;
  std::pair<int, int> pick(-1, 1);
  for (int t = 0; t < kTileCount; ++t) {
    if (kTiles[t].kind == TK_GENERIC) continue;
    const bool halo = kTiles[t].kind == TK_HALO;
    if (halo && !halo_ok(p, kTiles[t])) continue;
    if (p.wscale && !(kTiles[t].caps & CAP_W8)) continue;
    const int nk = plan_nk(p, kTiles[t]);
    const int wgs1 = plan_tiles_m(p, kTiles[t]) * cdiv(p.N, kTiles[t].bn);
    if (p.act == 3 && (kTiles[t].bn / 2) % 32 != 0) continue;
    for (int sk : sks) {
      if (sk > 1 && p.act == 3) continue;
      if (sk > 1 && (nk / sk < (halo ? 1 : 4) || (size_t)sk * p.M * p.N * sizeof(float) > p.workspace_bytes || !p.workspace)) continue;
      if (sk > 1 && make_plan([&] { ConvGemm q = p; q.force_tile = t; q.force_splitk = sk; return q; }()).splitk != sk) continue;   // duplicate of a smaller factor
      if (sk > 1 && wgs1 >= 4 * kNumCU) continue;      // already several rounds of workgroups: splitting K only adds traffic
      ConvGemm q = p;
      q.force_tile = t;
      q.force_splitk = sk;
      q.gn_out = nullptr;                              // candidates are timed without the GroupNorm partials (not every plan can emit them)
      if (int rc = conv_gemm(q, stream)) return rc;    // warm-up (also sets the function attributes)
      // best of two rounds of 8 back-to-back launches: single short rounds flipped plans from run to run
      const int reps = 8;
      float ms = 1e30f;
      for (int round = 0; round < 2; ++round) {
        SDEO_HIP(hipEventRecord(a, stream));
        for (int r = 0; r < reps; ++r)
          if (int rc = conv_gemm(q, stream)) return rc;
        SDEO_HIP(hipEventRecord(b, stream));
        SDEO_HIP(hipEventSynchronize(b));
        float t = 0.f;
        SDEO_HIP(hipEventElapsedTime(&t, a, b));
        ms = fminf(ms, t / reps);
      }
      // a 3x3 conv of a ResBlock feeds a GroupNorm: a plan whose epilogue cannot emit the GroupNorm partials (split-K, strips that
      // cut a group) costs that GroupNorm a statistics launch (~4 us, tools/plan_ab.py) where it runs as two launches (HW >= 1024)
      if (p.R == 3 && p.N % 32 == 0 && p.Ho * p.Wo >= 1024 && p.y && conv_gemm_gn_slots(q, p.N / 32) == 0) ms += 0.004f;
      if (ms < best) { best = ms; pick = {t, make_plan(q).splitk}; }
    }
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (pick.first >= 0) g_tuned[key] = pick;
  return 0;
}

}  // namespace sdeo
