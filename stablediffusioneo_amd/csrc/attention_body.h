  // The body of attention_kernel<D16, KS, MPAD, QB> and attention2_kernel<D16, MPAD> (csrc/attention.hip), included as text INSIDE both
  // kernels, after the parameter block has been pinned.  It expects: D16, KS, MPAD, QB, SEG2 (compile-time), `const AP& p`, and
  // `x` (APX: the second key segment, read only under SEG2).  No include guard on purpose.
  static_assert(!SEG2 || (KS == 1 && QB == 4), "the two-segment form exists for the KS = 1 kernels");
  constexpr int NT = 64 * QB * KS;                           // threads per workgroup
  constexpr int NKB = 2 / KS;                                // 32-key blocks of a tile each wave handles
  constexpr int DT = (D16 + 1) / 2;                          // 32-row tiles of O^T
  constexpr int KROW = D16 * 32 + ((D16 * 2) % 2 == 0 ? 16 : 0);  // K tile row bytes (odd multiple of 16)
  constexpr int VROW = attn_vrow(DT);                        // V tile bytes per key: >= DT*64, == 64 or 192 (mod 256)
  constexpr int KBYTES = 64 * KROW;
  constexpr int VBYTES = 64 * VROW;
  constexpr int STAGE = KBYTES + VBYTES;
  constexpr int KCH = D16 * 2;                               // 16-byte chunk slots per K / V row
  constexpr int KITEMS = 64 * KCH, KPASS = (KITEMS + NT - 1) / NT;
  // Row sum for free (odd D16 only): P V pads d to DT*32 = 16 (D16 + 1) rows of O^T, QK^T only to 16 D16, so column R1 = 16 D16 of
  // the V tile is never a real channel.  Filled with ones, the MFMA leaves sum_k P[k][q] in that row of O^T (register 8 of the
  // last tile, lanes 0..31): no per-score add, no cross-half exchange per tile, and the running sum is rescaled with O.
  constexpr bool ONES = (D16 % 2) == 1;
  constexpr int R1 = 16 * D16;

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int qb = KS == 2 ? (wave >> 1) : wave;               // 32-query block of this wave
  const int kh = KS == 2 ? (wave & 1) : 0;                   // key half of this wave (KS == 2)
  // XCD-aware placement (speed only): workgroups are dealt round-robin over the 8 XCDs; give each XCD a contiguous
  // run of (batch, head) pairs so the K / V^T of a head stay in ONE private L2 instead of being streamed by all eight
  const int qtiles = (p.Tq + 32 * QB - 1) / (32 * QB);
  int wg = blockIdx.x, nwg = gridDim.x;
  {
    const int q_ = nwg >> 3, r_ = nwg & 7, xcd = wg & 7, idx = wg >> 3;
    wg = (xcd < r_ ? xcd * (q_ + 1) : r_ * (q_ + 1) + (xcd - r_) * q_) + idx;
  }
  const int bh = wg / qtiles;
  const int b = bh / p.H, h = bh - b * p.H;
  const int q0 = (wg - bh * qtiles) * (32 * QB) + qb * 32;
  const int qrow = q0 + lq;
  const bool qvalid = qrow < p.Tq;
  const int d = p.d;
  // loop-invariant scalars pinned in SGPRs (otherwise re-read from the kernel-argument segment inside the key loop, an
  // s_load + lgkmcnt(0) in the softmax chain of every tile)
  float sl2 = p.scale_log2;
  int Tk = p.Tk;
  int causal = p.causal;
  asm volatile("" : "+s"(sl2), "+s"(Tk), "+s"(causal));

  // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[qrow][ks*16 + 8*lh + 0..7]
  f16x8 qf[D16];
  {
    const f16* qp = p.q + ((size_t)(b >= p.qB ? b - p.qB : b) * p.Tq + (qvalid ? qrow : 0)) * p.ldq + h * d;
    // unconditional loads (rows past Tq read row 0, chunks past d read chunk 0; zeroed at their first use below): a load under an
    // exec mask cannot be counted by the compiler's wait pass, and every later wait of the prologue would become vmcnt(0)
#pragma unroll
    for (int ks = 0; ks < D16; ++ks) {
      const int c = (ks * 2 + lh) * 8;
      qf[ks] = *reinterpret_cast<const f16x8*>(qp + (c < d ? c : 0));
    }
  }

  const f16* kbase = p.k + (size_t)b * p.TkS * p.ldk + h * d;
  const f16* vbase = p.v + (size_t)b * p.TkSv * p.ldv + h * d;
  const int ntiles = (p.Tk + 63) / 64;
  const f16x8 zero8 = f16x8{0, 0, 0, 0, 0, 0, 0, 0};

  // per-thread staging state, hoisted out of the key loop: source column and LDS destinations of the 16-byte chunks this thread moves.
  // DEEP: two register sets, the loads of a tile are issued TWO tiles ahead (small head dims, where a tile's compute is
  // shorter than a global round trip); otherwise one set, loads issued at the top of the previous tile.
  // Every load is UNCONDITIONAL (rows past Tk read row Tk - 1 again: those keys are masked to -inf, so P is 0 against a finite
  // V; threads without a chunk read chunk 0 and never store): with loads under exec masks or uniform branches the compiler
  // cannot count them and turns every wait into vmcnt(0), which serialises the prefetch with the compute it should hide behind.
  constexpr bool DEEP = D16 <= 5 && QB == 4;      // 64-query workgroups: one set (two passes per thread already fill the registers)
  f16x8 kr[DEEP ? 2 : 1][KPASS], vr[DEEP ? 2 : 1][KPASS];
  int krow[KPASS], kcol[KPASS], kdst[KPASS], vdst[KPASS];
#pragma unroll
  for (int i = 0; i < KPASS; ++i) {
    const int it = tid + i * NT;
    const int row = it / KCH, c = it - row * KCH;
    const bool use = it < KITEMS && c * 8 < d;
    krow[i] = row;
    kcol[i] = use ? c * 16 : 0;                      // bytes
    kdst[i] = use ? row * KROW + c * 16 : -1;        // chunk slots past d keep their zeros (K) / zeros and the ones column (V)
    vdst[i] = use ? row * VROW + c * 16 : -1;
  }
  const int last_key = Tk - 1;
  // byte offsets from the (wave-uniform) head bases stay below 2^32 and their factors below 2^24: one v_mad_u32_u24 per
  // address and the scalar-base form of global_load instead of a 64-bit multiply-add chain per load
  unsigned ldk2 = (unsigned)p.ldk * 2u, ldv2 = (unsigned)p.ldv * 2u;
  asm volatile("" : "+s"(ldk2), "+s"(ldv2));
  // SEG2: the same for the second segment.  A tile index >= ntiles addresses it (rows past x.Tk read row x.Tk - 1 again, so does every
  // tile the prefetch requests past the last one); bases, strides and the row limit are chosen by scalar selects, the loads stay
  // unconditional.
  const f16* kbase_x = SEG2 ? x.k + (size_t)b * x.TkS * x.ldk + h * d : nullptr;
  const f16* vbase_x = SEG2 ? x.v + (size_t)b * x.TkSv * x.ldv + h * d : nullptr;
  unsigned ldk2_x = SEG2 ? (unsigned)x.ldk * 2u : 0u, ldv2_x = SEG2 ? (unsigned)x.ldv * 2u : 0u;
  int last_key_x = SEG2 ? x.Tk - 1 : 0;
  if constexpr (SEG2) asm volatile("" : "+s"(ldk2_x), "+s"(ldv2_x), "+s"(last_key_x));
  auto load_tile = [&](auto SET, int kt) {
    constexpr int rs = SET.value;
    if constexpr (SEG2) {
      const bool second = kt >= ntiles;
      const int key0 = (second ? kt - ntiles : kt) * 64;
      const int last = second ? last_key_x : last_key;
      const char* kb = reinterpret_cast<const char*>(second ? kbase_x : kbase);
      const char* vb = reinterpret_cast<const char*>(second ? vbase_x : vbase);
      const unsigned lk = second ? ldk2_x : ldk2, lv = second ? ldv2_x : ldv2;
#pragma unroll
      for (int i = 0; i < KPASS; ++i) {
        const unsigned row = (unsigned)min(key0 + krow[i], last);
        kr[rs][i] = *reinterpret_cast<const f16x8*>(kb + (__umul24(row, lk) + (unsigned)kcol[i]));
        vr[rs][i] = *reinterpret_cast<const f16x8*>(vb + (__umul24(row, lv) + (unsigned)kcol[i]));
      }
    } else {
      const int key0 = kt * 64;
#pragma unroll
      for (int i = 0; i < KPASS; ++i) {
        const unsigned row = (unsigned)min(key0 + krow[i], last_key);
        kr[rs][i] = *reinterpret_cast<const f16x8*>(reinterpret_cast<const char*>(kbase) + (__umul24(row, ldk2) + (unsigned)kcol[i]));
        vr[rs][i] = *reinterpret_cast<const f16x8*>(reinterpret_cast<const char*>(vbase) + (__umul24(row, ldv2) + (unsigned)kcol[i]));
      }
    }
  };
  auto store_tile = [&](auto SET, int stage) {
    constexpr int rs = SET.value;
    char* ks_ = smem + stage * STAGE;
    char* vs_ = ks_ + KBYTES;
#pragma unroll
    for (int i = 0; i < KPASS; ++i) {
      if (kdst[i] >= 0) *reinterpret_cast<f16x8*>(ks_ + kdst[i]) = kr[rs][i];
      if (vdst[i] >= 0) *reinterpret_cast<f16x8*>(vs_ + vdst[i]) = vr[rs][i];
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  // Prologue order: EVERY global load of the prologue (Q above, tile 0, tile 1) is in flight before the LDS is initialised, so the
  // zero fill and its barrier pass under one memory round trip instead of standing between two of them.
  load_tile(S0{}, 0);
  if constexpr (DEEP) load_tile(S1{}, 1);           // set 1 carries the odd tiles, set 0 the even ones
  // both stages start as zeros (+ the ones column of V): staging only ever writes the chunk slots below d
  for (int off = tid * 16; off < 2 * STAGE; off += NT * 16) *reinterpret_cast<f16x8*>(smem + off) = zero8;
  __syncthreads();
  if (ONES && tid < 128) *reinterpret_cast<f16*>(smem + (tid >> 6) * STAGE + KBYTES + (tid & 63) * VROW + R1 * 2) = (f16)1.f;
  if (MPAD && tid < 128) *reinterpret_cast<f16*>(smem + (tid >> 6) * STAGE + (tid & 63) * KROW + d * 2) = (f16)1.f;   // K[key][d] = 1

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // the first real use of the Q fragments HERE (MPAD: scaled by scale * log2 e), before the later prefetch loads are issued: their
  // wait is then placed in front of the loop.  Left to the first MFMA of the loop the compiler must assume Q still in flight on
  // every iteration and waits vmcnt(0) at the top of each tile, which serialises the prefetched K / V loads with the compute they
  // were meant to hide behind.
#pragma unroll
  for (int ks = 0; ks < D16; ++ks) {
    const bool live = qvalid && (ks * 2 + lh) * 8 < d;
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[ks][j] = live ? (MPAD ? (f16)((float)qf[ks][j] * sl2) : qf[ks][j]) : (f16)0.f;
  }
#pragma unroll
  for (int ks = 0; ks < D16; ++ks) asm volatile("" : "+v"(qf[ks]));
  store_tile(S0{}, 0);
  if constexpr (DEEP) load_tile(S0{}, 2);
  __syncthreads();

  // one 64-key tile; at its end the NEXT tile (loaded two iterations ago) goes from registers to the other LDS buffer and the
  // freed register set takes the loads of the tile after that: a global round trip has two tiles of compute to hide behind
  // the compute of one 64-key tile (QK^T, online softmax, P V) out of LDS buffer `cur`
  // SEG2: tile `ntiles` is the second segment's.  In front of it the first softmax is closed: O and 1 / l go to registers of their own
  // (fp32: parked in the output rows O / l would pass through fp16 and the sum would be rounded twice), the state starts afresh (MPAD:
  // Q's pad channel holds no reference again) and masking switches to the second key count.  The branches are wave-uniform.
  // What is parked is the UNNORMALISED O: the store forms O * (1 / l) + t as one fused multiply-add per element, which for t = 0
  // (x.w = 0) can be rounded exactly as the one-segment store rounds O * (1 / l); a normalised fp32 copy would add a rounding.
  std::conditional_t<SEG2, f32x16[DT], char> o1;
  float inv1 = 0.f;
  auto compute = [&](int kt, int cur) __attribute__((always_inline)) {
    if constexpr (SEG2) {
      if (kt == ntiles) {
        if constexpr (ONES) l_run = __shfl(o[DT - 1][8], lq, 64);
        inv1 = 1.0f / l_run;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            o1[t][r] = o[t][r];
            o[t][r] = 0.f;
          }
        m_run = -INFINITY;
        l_run = 0.f;
        if (MPAD && lh == 1) qf[D16 - 1][0] = (f16)0.f;
        Tk = x.Tk;
      }
      if (kt >= ntiles) kt -= ntiles;             // key indices of the second segment count from 0 again
    }
    const char* ks_ = smem + cur * STAGE;
    const char* vs_ = ks_ + KBYTES;

    // ---- S^T = K Q^T for the two 32-key blocks of this tile
    f32x16 s[NKB];
#pragma unroll
    for (int ki = 0; ki < NKB; ++ki) {
      const int kb = KS == 2 ? kh : ki;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[ki][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < D16; ++ks) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(ks_ + (kb * 32 + lq) * KROW + (ks * 2 + lh) * 16);
        s[ki] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[ki], 0, 0, 0);
      }
    }
    // ---- V^T fragments of this tile, fetched NOW (transposing LDS reads): their latency passes under the softmax below
    //      instead of in front of every P V MFMA.  Lane (q = (lane & 15) >> 2, pp = lane & 3) of each 16-lane group addresses key
    //      row q, channels 4pp..4pp+3 of the group's 4-key x 16-channel block and receives its own channel for the four keys.
    f16x8 vf[NKB][2][DT];
#pragma unroll
    for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const int kb = KS == 2 ? kh : ki;
        const char* vblk = vs_ + (kb * 32 + 16 * st + 4 * lh + ((lane & 15) >> 2)) * VROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          typedef __attribute__((address_space(3))) h16x4* lds_h4;
          const h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4)(vblk + t * 64));
          const h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4)(vblk + t * 64 + 8 * VROW));
          vf[ki][st][t] = __builtin_shufflevector(__builtin_bit_cast(f16x4, lo), __builtin_bit_cast(f16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
        }
      }
    // ---- online softmax (base-2), key index of s[kb][r] = kt*64 + kb*32 + (r&3) + 8*(r>>2) + 4*lh
    //      the running max is kept in scaled units (score * scale * log2 e); the scale itself is folded into one fma
    // masking only on a tile that needs it: ONE uniform branch per tile (inside the register loop it became a branch per score register)
    if ((kt + 1) * 64 > Tk || causal) {
#pragma unroll
      for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kb = KS == 2 ? kh : ki;
          const int key = kt * 64 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (key >= Tk || (causal && key > qrow)) s[ki][r] = -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[ki][r]);
    float rs = 0.f;
    if constexpr (MPAD) {
      // the scores arrive as s * scale * log2 e - m_run (0 instead of m_run while the row has no reference yet)
      mx = xor32_max(mx);
      const bool unset = m_run == -INFINITY;
      if (__any(mx > 8.0f || (unset && mx > -INFINITY))) {       // wave-uniform, rare (see the lazy rescale below)
        const float m_abs = unset ? mx : m_run + fmaxf(mx, 0.f);  // the row's reference in absolute units: only ever raised
        const float m_q = (float)(f16)m_abs;                       // ... as the fp16 value Q's pad channel can hold
        const bool valid = m_abs > -INFINITY;                      // false: no visible key so far, the row stays unset
        const float delta = valid ? m_q - (unset ? 0.f : m_run) : 0.f;
        const float alpha = unset ? 0.f : __builtin_amdgcn_exp2f(-delta);
#pragma unroll
        for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[ki][r] -= delta;          // this tile was formed against the old reference
        l_run *= alpha;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
        if (valid) {
          m_run = m_q;
          if (lh == 1) qf[D16 - 1][0] = (f16)(-m_q);               // channel d of this row's Q: lanes lh = 1, last k-step, element 0
        }
      }
#pragma unroll
      for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = __builtin_amdgcn_exp2f(s[ki][r]);
          s[ki][r] = pv;
          if (!ONES) rs += pv;
        }
    } else {
    mx = xor32_max(mx) * sl2;
    // Lazy rescale: the running reference m_run moves only when some row's new maximum exceeds it by more than 8 (base-2 units),
    // i.e. P = 2^(s - m_run) stays below 2^8 -- exact in the fp32 accumulators and far inside fp16 for the P V operand.  The
    // result is the same softmax (any common reference per row cancels in O / l); with the eager form ~70 % of the tiles of a
    // 32-query block took the 19-instruction rescale of O on random scores, with this one only the first few do.
    if (__any(mx > m_run + 8.0f)) {    // wave-uniform; -inf + 8 = -inf, so the first valid tile always takes it
      const float m_new = max_raw(m_run, mx);
      // a row that has not seen a valid key yet (m_new = -inf; its O and l are still 0) must not form -inf - -inf
      const float alpha = m_new == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
      m_run = m_new;
    }
    // a key half that has not seen a single valid key yet (KS == 2, Tk <= 32) keeps m = -inf: exponentiate against 0
    const float m_use = (KS == 2 && m_run == -INFINITY) ? 0.f : m_run;
#pragma unroll
    for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[ki][r], sl2, -m_use));
        s[ki][r] = pv;
        if (!ONES) rs += pv;
      }
    }
    if (!ONES) rs = xor32_sum(rs);
    l_run += rs;

    // ---- O^T += V^T P^T : P^T fragments straight from the score registers
#pragma unroll
    for (int ki = 0; ki < NKB; ++ki)
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        f16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (f16)s[ki][8 * st + j];
#pragma unroll
        for (int t = 0; t < DT; ++t) o[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[ki][st][t], pf, o[t], 0, 0, 0);
      }
  };
  const int nloop = SEG2 ? ntiles + 1 : ntiles;   // SEG2: the second segment's tile included
  if constexpr (DEEP) {
    // at the end of a tile the NEXT tile (loaded two iterations ago) goes from registers to the other LDS buffer and the freed
    // register set takes the loads of the tile after that: a global round trip has two tiles of compute to hide behind
    for (int kt = 0; kt < nloop; kt += 2) {       // an odd tile count runs one fully masked tile (P = 0) at the end
      compute(kt, 0);
      store_tile(S1{}, 1);
      load_tile(S1{}, kt + 3);
      __syncthreads();
      compute(kt + 1, 1);
      store_tile(S0{}, 0);
      load_tile(S0{}, kt + 4);
      __syncthreads();
    }
  } else {
    for (int kt = 0; kt < nloop; ++kt) {
      const int cur = kt & 1;
      load_tile(S0{}, kt + 1);
      compute(kt, cur);
      store_tile(S0{}, cur ^ 1);
      __syncthreads();
    }
  }

  if constexpr (KS == 2) {
    // ---- merge the two key halves of each query block through LDS (field-major, lane-contiguous: conflict-free).
    //      The loop's last __syncthreads() already separates the final tile reads from these writes.
    // A tile of a half that lies entirely past Tk leaves m = -inf, l = 0 there; exp2(-inf - m) = 0 handles it, and half 0
    // always sees key 0, so m below is finite.
    constexpr int NF = 2 + DT * 16;
    float* mg = reinterpret_cast<float*>(smem) + qb * NF * 64 + lane;
    if (kh == 1) {
      mg[0] = m_run;
      mg[64] = l_run;
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mg[(2 + t * 16 + r) * 64] = o[t][r];
    }
    __syncthreads();
    if (kh == 1) return;
    const float m1 = mg[0], l1 = mg[64];
    const float m = fmaxf(m_run, m1);
    const float a0 = __builtin_amdgcn_exp2f(m_run - m), a1 = __builtin_amdgcn_exp2f(m1 - m);
    l_run = l_run * a0 + l1 * a1;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][r] = o[t][r] * a0 + mg[(2 + t * 16 + r) * 64] * a1;
  }

  if constexpr (ONES) l_run = __shfl(o[DT - 1][8], lq, 64);     // row R1 of O^T: register 8 of the last tile in lanes 0..31
  // ---- normalise and store: o[t][4g..4g+3] = O[qrow][t*32 + 8g + 4lh + 0..3]
  if (qvalid) {
    const float inv = SEG2 ? x.w / l_run : 1.0f / l_run;
    f16* op = p.o + ((size_t)b * p.Tq + qrow) * p.ldo + h * d;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dc = t * 32 + 8 * g + 4 * lh;
        if (dc < d) {
          if constexpr (SEG2) {
            // O1 / l1 + w O2 / l2 in fp32, each element rounded the way the one-segment store below rounds it (fma_f16_once)
            f16x4 ov;
            ov[0] = fma_f16_once(o1[t][4 * g], inv1, o[t][4 * g] * inv);
            ov[1] = fma_f16_twice(o1[t][4 * g + 1], inv1, o[t][4 * g + 1] * inv);
            ov[2] = fma_f16_twice(o1[t][4 * g + 2], inv1, o[t][4 * g + 2] * inv);
            ov[3] = fma_f16_once(o1[t][4 * g + 3], inv1, o[t][4 * g + 3] * inv);
            *reinterpret_cast<f16x4*>(op + dc) = ov;
          } else {
            f16x4 ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = (f16)(o[t][4 * g + j] * inv);
            *reinterpret_cast<f16x4*>(op + dc) = ov;
          }
        }
      }
  }
