// Network executor of libsdeo, program construction: the static launch schedules ("programs") of ControlNet, ControlledUnetModel and
// the VAE that sdeo_configure builds (the weight registry is net_weights.hip, the entry points that run the programs net.hip).
//
// This is what stands where the reference's opaque TensorRT engines stood (ControlNet.plan /
// ControlledUnet.plan / Decoder.plan driven by Engine.infer, Engine.py:131-161): the module structure of
// `cldm/cldm.py:22-45,284-305`, `openaimodel.py:255-275` (ResBlock), `attention.py:381-385,431-450`
// (BasicTransformerBlock / SpatialTransformer) and `model.py:619-652` (Decoder) is unrolled ONCE at
// sdeo_configure time into a flat list of kernel launches over a planned activation arena (fp16 NHWC);
// a forward pass then only walks that list: no allocation, no synchronisation, no shape logic, so the
// whole step is hipGraph-capturable.
//
// Fusions decided here (each is arithmetic the reference performs as separate ATen calls):
//   * conv/linear bias, the ResBlock time-embedding add, the residual add, SiLU of the hint block and the
//     control scale are epilogues of the producing conv/GEMM;
//   * nearest-x2 Upsample is folded into the following conv's gather; channel concat is a write into place;
//   * every ResBlock's emb_layers Linear is one stacked GEMM per forward (same input SiLU(emb));
//   * q, k and v projections of self-attention are ONE GEMM (the attention kernel reads V row-major through transposing
//     LDS reads), cross-attention K and V likewise;
//   * every LayerNorm of a BasicTransformerBlock is folded into the GEMM that consumes it (gamma into the weights at load
//     time, mean / rstd as two per-row scalars in the epilogue); the per-row statistics are written by the epilogue of the
//     GEMM that produced the residual stream, so no LayerNorm kernel and no normalised copy of the tokens exists;
//   * cross-attention K / V^T depend only on the text context and the hint block only on the hint: both are
//     computed once per image and cached across the DDIM steps;
//   * the two halves of sdeo_ddim_step's CFG batch [x; x] differ only in their text context, so what a network computes before its
//     first cross-attention (input_blocks.1: ResBlock, proj_in, self-attention, attn2.to_q) runs on the first half only and the
//     full-batch launches behind it read the half-batch tensors twice (P_UNET_ENC_SH / P_CN_SH, build_shared_prefix).
//   * several control networks (sdeo_enable_extra_controlnets) share the UNet: the extra ones run behind net 0 on its stream and the fused
//     decoder adds scale_j * zero_conv_j(cn_h[j][i]) to the running sum of control i in place, one multi-problem launch per extra net.
#include "net_handle.h"

// ------------------------------------------------------------------------------------------------
// program builder
// ------------------------------------------------------------------------------------------------
namespace sdeo {      // (Fp8State, declared with the handle, names the Builder)

struct RowStats {                     // per-row (sum, sumsq) partials of a [rows][c] tensor: fp32 [rows][ld][2]
  float* p = nullptr;
  int ld = 0, strips = 0, c = 0;
};

struct ConvOpts {                     // conv / gemm options
  const float* bias2 = nullptr; int ld_bias2 = 0;
  const float* const* bias2_cur = nullptr; const int* ld_bias2_cur = nullptr; int bias2_off = 0;    // read at launch time (time embedding)
  const T* res = nullptr;
  bool res_half = false;         // a full-batch launch whose residual was computed for the first half of the batch only (Builder::share)
  int act = 0;
  int plan_rows = 0;             // gemm(): run the plan of the same GEMM at this many rows (ConvGemm::plan_B); 0: its own
  const float* scale_host = nullptr;   // read at launch time (control scales)
  const T* out = nullptr;        // write into this view instead of allocating
  int cout_store = -1;           // stored output channels (>= logical, padded rows of W are zero)
  RowStats* stats = nullptr;     // producer: emit per-row (sum, sumsq) partials of the stored values into this buffer
  const RowStats* ln = nullptr;  // consumer: LayerNorm folded into this GEMM, statistics of x from *ln, row sums ln_s
  const float* ln_s = nullptr;
  bool gn_next = false;          // the output feeds a GroupNorm(32): let the epilogue emit its partial statistics when the plan can
  // conv(): stream this [cout][k*k*x.c] matrix / bias instead of the tensors registered under `name` (a composed Linear)
  const f16* w_ovr = nullptr; const float* b_ovr = nullptr;
  // conv(): zero padding top / left and bottom / right; -1 = k / 2 (the VAE encoder's Downsample: 0 and 1)
  int pad_before = -1, pad_after = -1;
};

struct Builder {
  typedef ConvOpts CO;
  Engine* e;
  const Lane* lane;          // arena and workspaces of the stream the program built now runs on
  bool dry;
  // Shared prefix of the CFG pair (build_shared_prefix).  `share`: the block built now is the variant whose ops in front of the first
  // cross-attention run on the first N / 2 images; build_res / build_attn raise `half` around those ops.  A half-batch launch keeps the
  // full-batch tensors (same arena plan, it writes a prefix of them) and the full-batch problem's kernel plan (ConvGemm::plan_B,
  // AttnArgs::plan_B), so every row it writes is bit-identical to the full-batch launch's.
  // half_all: the program built now runs EVERY launch on the first N / 2 images (a control net in SDEO_CONTROL_COND: build_controlnet);
  // `half` then stays raised, under the same two promises.
  bool share = false, half = false, half_all = false;
  bool borrowed_plan = false;      // gemm() -> launch_conv(): plan_B comes from ConvOpts::plan_rows
  Program* prog = nullptr;
  size_t max_splitk = 0, max_gn = 0;
  std::string err;

  T alloc(int n, int h, int w, int c) {
    T t;
    t.n = n; t.h = h; t.w = w; t.c = c; t.ld = c;
    t.off = lane->arena->alloc((size_t)n * h * w * c * 2);
    t.p = reinterpret_cast<f16*>(lane->base + t.off);
    return t;
  }
  T alloc2d(int rows, int c) { return alloc(1, 1, rows, c); }
  void release(T& t) { t.release(*lane->arena); }
  void advance(T& cur, T next) { release(cur); cur = next; }      // cur = f(cur): the input is released once its successor exists
  template <class F>
  void on_lane(const Lane* l, F build) { const Lane* saved = lane; lane = l; build(); lane = saved; }      // what `build` builds runs on l
  // producer side of the GroupNorm fusion: when the plan of p can, give it a partials buffer and record it on the output tensor
  static bool gn_from_producer() { static const bool on = [] { const char* v = getenv("SDEO_GN_PRODUCER_STATS"); return !v || atoi(v) != 0; }(); return on; }
  // The buffer is reserved whatever the plan (sized for the smallest tile: 32 rows per entry), so that the arena plan does not depend
  // on plans measured between the planning pass and the build pass (SDEO_AUTOTUNE); whether the launch emits is decided in
  // launch_conv, after the plan of the shape is final.
  void reserve_gn_partials(const ConvGemm& p, T& y) {
    if (!gn_from_producer() || p.N % 32) return;
    const int hw = p.Ho * p.Wo;
    y.gnp_off = lane->arena->alloc((size_t)(p.plan_B ? p.plan_B : p.B) * ((hw + 31) / 32) * 32 * 2 * sizeof(float));
    y.gnp = nullptr;                       // set by launch_conv when the plan emits
    y.gn_slots = 0;
  }
  void push(Op op, const char* key = "elementwise", double flops = 0, double bytes = 0, const std::string& tag = std::string()) {
    op.key = key; op.flops = flops; op.bytes = bytes; op.tag = tag;
    if (!dry) prog->push_back(std::move(op));
  }

  const WEntry* W(const std::string& name) {
    const WEntry* w = e->ws.find(name);
    if (!w && err.empty()) err = "unknown weight " + name;
    return w;
  }
  const f16* wptr(const std::string& name) { return W(name) ? e->ws.ptr<f16>(name) : nullptr; }
  const float* vptr(const std::string& name) { return W(name) ? e->ws.ptr<float>(name) : nullptr; }
  const f16* named_w(const std::string& name) { return reinterpret_cast<const f16*>(e->ws.slab + e->named_off.at(name)); }
  const float* named_v(const std::string& name) { return reinterpret_cast<const float*>(e->ws.slab + e->named_off.at(name)); }

  void launch_conv(ConvGemm p, const float* scale_host, RowStats* stats = nullptr, T* gn_y = nullptr, const ConvOpts* lo = nullptr) {
    // precision and scratch sizes follow the problem whose plan the launch takes (a half-batch launch: the full-batch one); a GEMM
    // that only borrows the plan of more rows (ConvOpts::plan_rows) keeps the operand form of its own
    const int Mplan = p.plan_B && !borrowed_plan ? p.M / p.B * p.plan_B : p.M;
    e->fp8.use_mx(p, Mplan, *this);
    e->fp8.use_fp8_weights(p, Mplan, e->ws.slab);
    const size_t tune_ws = e->autotune ? conv_gemm_autotune_workspace_bytes(p) : 0;
    if (!dry && e->autotune && !share && !half_all) {       // (the shared variant of a block runs the plans its full-batch build measured)
      ConvGemm q = p;
      q.workspace = lane->splitk_ws;
      q.workspace_bytes = lane->splitk_ws_bytes;
      if (conv_gemm_autotune(q, 0) && err.empty()) err = std::string("autotune failed: ") + sdeo_last_error();
    }
    if (gn_y && gn_y->gn_reserved()) {      // the plan of this shape is final now: emit the GroupNorm partials if it can
      const int cpg = p.N / 32, slots = conv_gemm_gn_slots(p, cpg);
      if (slots > 0) {
        gn_y->gnp = reinterpret_cast<float*>(lane->base + gn_y->gnp_off);
        gn_y->gn_slots = slots;
        p.gn_out = gn_y->gnp; p.gn_cpg = cpg; p.gn_slots = slots; p.gn_groups = 32;
      }
    }
    if (!dry && !share && !half_all && getenv("SDEO_DUMP_GEMM"))   // shape census for tools/tune_gemm.py
      fprintf(stderr, "SDEO_GEMM %d %d %d %d %d %d %d %d %d %d %s\n", p.M, p.N, p.K, p.Cin, p.R, p.stride, p.ups, p.B, p.Hi, p.Wi,
              conv_gemm_kernel_name(p));
    bool stats_by_kernel = false;
    if (stats) {
      // the epilogue of an unsplit plan writes one partial per strip; a split-K plan leaves them to a row_stats launch
      stats->c = p.N;
      stats->strips = conv_gemm_stats_strips(p);
      if (stats->strips > 0 && stats->strips <= stats->ld) { p.stats_out = stats->p; p.stats_ld = stats->ld; }
      else { stats->strips = 1; stats_by_kernel = true; }
    }
    const float* const* b2cur = lo ? lo->bias2_cur : nullptr; const int* b2ld = lo ? lo->ld_bias2_cur : nullptr; const int b2off = lo ? lo->bias2_off : 0;
    size_t need = 0;
    Op op = conv_gemm_op(p, lane->splitk(), &need, true, 0, [scale_host, b2cur, b2ld, b2off](ConvGemm& q) {      // read when the launch runs
      if (scale_host) q.scale = *scale_host;
      if (b2cur) { q.bias2 = *b2cur + b2off; q.ld_bias2 = *b2ld; }
    });
    if (!dry) prog->push_back(std::move(op));
    max_splitk = std::max(max_splitk, e->autotune ? tune_ws : need);      // (autotune: sized before it could change the plan)
    for (auto& t : mx_tmp) release(t);       // the packed activations live for this one launch
    mx_tmp.clear();
    if (stats_by_kernel) {
      float* sp = stats->p; const int ld = stats->ld, rows = p.M, C = p.N, ldy = p.ldy; const f16* y = p.y;
      push([=](hipStream_t s) { return row_stats(sp, ld, y, ldy, rows, C, s); }, "row_stats", 0, 2.0 * rows * C,
           "rows" + std::to_string(rows) + " C" + std::to_string(C));
    }
  }

  std::vector<T> mx_tmp;
  RowStats alloc_stats(int rows, int c) {
    RowStats st;
    st.ld = std::max(1, (c + 31) / 32);          // narrowest epilogue strip is 32 columns
    st.c = c;
    T raw = alloc2d(rows, st.ld * 4);            // rows * ld * 2 floats in an fp16-typed arena block
    st.p = reinterpret_cast<float*>(raw.p);
    stats_blocks.push_back(raw);
    return st;
  }
  void release_stats() {                         // statistics buffers live until the end of their transformer block
    for (auto& t : stats_blocks) release(t);
    stats_blocks.clear();
  }
  std::vector<T> stats_blocks;

  static void set_ln(ConvGemm& p, const ConvOpts& o) {
    if (!o.ln) return;
    p.ln_stats = o.ln->p; p.ln_s = o.ln_s; p.ln_strips = o.ln->strips; p.ln_ld = o.ln->ld; p.ln_c = o.ln->c; p.ln_eps = 1e-5f;
  }

  // conv on an image view; weights by name (".weight"/".bias" appended)
  T conv(const T& x, const std::string& name, int cout, int k, int stride, int ups, const CO& o = CO()) {
    const WEntry* w = o.w_ovr ? nullptr : W(name + ".weight");
    ConvGemm p;
    const int pad = o.pad_before >= 0 ? o.pad_before : k / 2;
    const int pad_after = o.pad_after >= 0 ? o.pad_after : k / 2;
    const int hv = ups ? 2 * x.h : x.h, wv = ups ? 2 * x.w : x.w;
    const int ho = (hv + pad + pad_after - k) / stride + 1, wo = (wv + pad + pad_after - k) / stride + 1;
    const int cs = o.cout_store > 0 ? o.cout_store : cout;
    T y = o.out ? o.out->view() : alloc(x.n, ho, wo, cs);
    const int n = half ? x.n / 2 : x.n;
    if (w && w->ipad != x.c && err.empty()) err = "conv " + name + ": input has " + std::to_string(x.c) + " channels, weight expects " + std::to_string(w->ipad);
    p.x = x.p; p.y = y.p;
    if (o.w_ovr) { p.w = o.w_ovr; p.bias = o.b_ovr; } else { p.w = wptr(name + ".weight"); p.bias = vptr(name + ".bias"); }
    p.bias2 = o.bias2; p.ld_bias2 = o.ld_bias2;
    if (o.res) { p.res = o.res->p; p.ldres = o.res->ld; }
    p.B = n; p.Hi = x.h; p.Wi = x.w; p.Cin = x.c; p.Ho = ho; p.Wo = wo; p.R = p.S = k; p.stride = stride; p.pad = pad; p.ups = ups;
    if (pad_after != pad) p.pad_after = pad_after;
    p.M = n * ho * wo; p.N = cs; p.K = k * k * x.c;
    if (half) p.plan_B = x.n;
    if (o.res_half) p.res_rows = p.M / 2;
    p.ldx = x.ld; p.ldw = p.K; p.ldy = y.ld; p.act = o.act;
    const bool want_gn = o.gn_next && !o.out && !o.scale_host && cs == y.c;
    if (want_gn) reserve_gn_partials(p, y);
    launch_conv(p, o.scale_host, o.stats, want_gn ? &y : nullptr, &o);
    return y;
  }

  // y[rows][n] = x[rows][k] . w[n][k]^T (+bias)(+res)
  T gemm(const T& x, const f16* w, int ldw, int n, const float* bias, const CO& o = CO(), float* out32 = nullptr, int ld32 = 0) {
    ConvGemm p;
    const int rows = half ? x.rows() / 2 : x.rows();
    T y;
    if (!out32) y = o.out ? o.out->view() : alloc(x.n, x.h, x.w, n);
    p.x = x.p; p.w = w; p.bias = bias;
    if (out32) { p.y32 = out32; p.ldy = ld32; } else { p.y = y.p; p.ldy = y.ld; }
    if (o.res) { p.res = o.res->p; p.ldres = o.res->ld; }
    p.B = rows; p.Cin = x.c; p.M = rows; p.N = n; p.K = x.c;
    p.ldx = x.ld; p.ldw = ldw; p.act = o.act;
    if (half) p.plan_B = x.rows();
    else if (o.plan_rows > rows) { p.plan_B = o.plan_rows; borrowed_plan = true; }
    if (o.res_half) p.res_rows = rows / 2;
    set_ln(p, o);
    if (o.ln && o.ln->c != x.c && err.empty()) err = "LayerNorm statistics of a " + std::to_string(o.ln->c) + "-channel tensor fed to K = " + std::to_string(x.c);
    launch_conv(p, o.scale_host, o.stats);
    borrowed_plan = false;
    return y;
  }

  // yt[c][rows] = w[c][k] . x[rows][k]^T (+bias per row): the transposed projection (V^T)
  T gemm_t(const T& x, const f16* w, int ldw, int c, const float* bias_rows) {
    ConvGemm p;
    const int rows = x.rows();
    T y = alloc2d(c, rows);
    p.x = w; p.w = x.p; p.y = y.p; p.bias = bias_rows; p.bias_per_row = bias_rows ? 1 : 0;
    p.B = c; p.Cin = x.c; p.M = c; p.N = rows; p.K = x.c;
    p.ldx = ldw; p.ldw = x.ld; p.ldy = rows;
    launch_conv(p, nullptr);
    return y;
  }

  T gn(const T& x, const std::string& name, float eps, int silu_, const T* out = nullptr) {
    T y = out ? out->view() : alloc(x.n, x.h, x.w, x.c);
    const float* g = vptr(name + ".weight");
    const float* b = vptr(name + ".bias");
    const int B = half ? x.n / 2 : x.n, HW = x.h * x.w, C = x.c;      // (no plan to inherit: the GroupNorm kernels work image by image)
    max_gn = std::max(max_gn, (size_t)B * gn_chunks(HW) * 32 * 2 * sizeof(float));
    const Lane* ws = lane;                 // its GroupNorm workspace exists when the launch runs
    const f16* xp = x.p; f16* yp = y.p; const int ldx = x.ld, ldy = y.ld;
    GnArgs ga{yp, xp, g, b, nullptr, ldy, ldx, B, HW, C, 32, eps, silu_};
    // statistics that came out of the producer's epilogue: one launch (normalise) instead of two
    const bool apply_only = x.gnp && !groupnorm_is_single_launch(ga);
    if (apply_only) {
      ga.ext_partials = x.gnp; ga.ext_nsc = x.gn_slots;
      max_gn = std::max(max_gn, (size_t)B * 32 * 2 * sizeof(float));
    }
    push([=](hipStream_t s) mutable { ga.partials = ws->gn_ws; return groupnorm_nhwc(ga, s); }, "groupnorm", 0,
         (apply_only ? 2.0 : 3.0) * 2.0 * B * HW * C, "C" + std::to_string(C) + " HW" + std::to_string(HW) + (apply_only ? " apply" : ""));
    return y;
  }

  // FreeU on a decoder concat buffer whose two halves are written (include/sdeo.h: sdeo_set_freeu): in place, flagged launches that
  // only the handle's FreeU programs keep (build_all).  cat's first c_h columns are h; the stage rule picks (b, s), read at launch with
  // the version.  The version-2 mean map lives in the lane's GroupNorm workspace: the launches sit between the producers of the buffer
  // and the first GroupNorm that reads it, on one stream, so nothing else holds it.
  // The GroupNorm behind the concat must not take statistics from a producer's epilogue, which an in-place change would leave stale: a
  // concat buffer never carries any (conv() reserves partials only for a tensor it allocates, a concat half is written through
  // ConvOpts::out), and a buffer that did is refused here.
  void freeu(const T& cat, int c_h) {
    const int mc = e->cfg.model_channels;
    const int stage = c_h == 4 * mc ? 0 : c_h == 2 * mc ? 1 : -1;
    if (stage < 0) return;
    const int c_skip = cat.c - c_h;
    if (cat.gnp && err.empty()) err = "FreeU on a concat buffer that carries GroupNorm statistics of its producer";
    if (cat.h > kFreeuMaxDim || cat.w > kFreeuMaxDim || c_h % 16 || c_skip % 8 || cat.ld % 8) {      // (sdeo_set_freeu refuses; the plain programs are unaffected)
      if (e->freeu_refusal.empty())
        e->freeu_refusal = "a " + std::to_string(cat.h) + " x " + std::to_string(cat.w) + " concat of " + std::to_string(c_h) + " + " +
                           std::to_string(c_skip) + " channels is outside what the FreeU kernels take";
      return;
    }
    max_gn = std::max(max_gn, freeu_workspace_bytes(cat.n, cat.h, cat.w));
    const Lane* ws = lane;
    f16* p = cat.p; const int ld = cat.ld, n = cat.n, h = cat.h, w = cat.w;
    const float* bp = &e->freeu_b[stage]; const float* sp = &e->freeu_s[stage]; const int* vp = &e->freeu_version;
    Op op([=](hipStream_t s) { return freeu_nhwc_f16(p, ld, n, h, w, c_h, c_skip, *bp, *sp, *vp, ws->gn_ws, s); }, "freeu", 0,
          2.0 * n * h * w * (2.0 * c_h + 3.0 * c_skip), "C" + std::to_string(c_h) + "+" + std::to_string(c_skip) + " HW" + std::to_string(h * w));
    op.freeu = true;
    if (!dry) prog->push_back(std::move(op));
  }

  // conv3x3(act(GroupNorm(x))) (`openaimodel.py:255-275`, `model.py:129-149`): GroupNorm launch(es) + conv
  T gn_conv(const T& x, const std::string& gn_name, float eps, int silu_, const std::string& conv_name, int cout, CO o) {
    T t = gn(x, gn_name, eps, silu_);
    T y = conv(t, conv_name, cout, 3, 1, 0, o);
    release(t);
    return y;
  }

  // qB: batches of q when the full-batch launch reads the queries of the first half twice (0: B).  Under `half` the first B / 2 batches run.
  // k2: a second key segment (the image-prompt K_ip | V_ip of a handle with sdeo_enable_ip_adapter), [B * Tk2S][ldk2] with V_ip at v2:
  // the SAME launch becomes the two-segment one (attention2), weighted by e->ip_scale as it is when the launch runs.
  void attn(const T& o, const f16* q, int ldq, const f16* k, int ldk, const f16* v, int ldv, int B, int H, int Tq, int Tk, int TkS, int TkSv, int d,
            int qB = 0, const f16* k2 = nullptr, const f16* v2 = nullptr, int ldk2 = 0, int Tk2 = 0, int Tk2S = 0) {
    AttnArgs a{o.p, q, k, v, o.ld, ldq, ldk, ldv, B, H, Tq, Tk, TkS, TkSv, d, 1.0f / sqrtf((float)d), 0};
    a.qB = qB;
    if (half) { a.plan_B = B; a.B = B / 2; }
    B = a.B;
    const std::string tag = "Tq" + std::to_string(Tq) + " Tk" + std::to_string(Tk) + (k2 ? "+" + std::to_string(Tk2) : "") + " d" + std::to_string(d);
    if (k2) {
      if (!attention2_kernel_name(a.plan_B ? a.plan_B : a.B, H, Tq, Tk, Tk2, d) && err.empty()) err = std::string("image-prompt cross-attention: ") + sdeo_last_error();
      const Attn2Seg s2{k2, v2, ldk2, ldk2, Tk2, Tk2S, Tk2S, 0.f};
      const float* w = &e->ip_scale;
      push([=](hipStream_t s) { Attn2Seg x = s2; x.w = *w; return attention2(a, x, s); }, "attention",
           4.0 * B * H * (double)Tq * (Tk + Tk2) * d, 2.0 * B * H * d * (2.0 * Tq + 2.0 * (Tk + Tk2)), tag);
      return;
    }
    push([=](hipStream_t s) { return attention(a, s); }, "attention",
         4.0 * B * H * (double)Tq * Tk * d, 2.0 * B * H * d * (2.0 * Tq + 2.0 * Tk), tag);
  }
};

// block-scaled fp8 on both sides: pack the activations (one launch), run the GEMM on the fp8 MFMA.
// Not with the LayerNorm fold: the fold multiplies the RAW rows and subtracts mean * s afterwards, so the pack would round the rows
// with their mean still in them.  e4m3 rounds relative to the element, i.e. to the mean of a row that sits far off zero, and that error
// does not cancel in acc - mean * s: at 16 standard deviations off zero the folded block-scaled launch measured 0.37 of the output
// scale against 0.037 for LayerNorm first, pack second (profiles/mx_ln_fold_error.json).  Those GEMMs keep fp16 activations.
void Fp8State::use_mx(ConvGemm& p, int Mplan, Builder& b) {
  if (!(act_bits == 8 && mxslab && Mplan >= mx_min_rows && p.R == 1 && p.S == 1 && p.stride == 1 && !p.ups && p.K % 128 == 0 &&
        p.K == p.Cin && p.ldx % 16 == 0 && !p.bias_per_row && p.y && !p.y32 && !p.ln_stats))
    return;
  auto it = mxindex.find((size_t)(reinterpret_cast<const char*>(p.w) - b.e->ws.slab));
  if (it == mxindex.end() || it->second.cols != p.ldw || p.N > it->second.rows) return;
  T xq = b.alloc2d(Mplan, p.K / 2), xs = b.alloc2d(Mplan, (p.K / 32 + 15) / 16 * 8);      // bytes: M x K codes, M x roundup(K/32, 16) scales
  uint8_t* q = reinterpret_cast<uint8_t*>(xq.p);
  uint8_t* sc = reinterpret_cast<uint8_t*>(xs.p);
  const int lds = (p.K / 32 + 15) / 16 * 16;
  const f16* xp = p.x; const int M_ = p.M, K_ = p.K, ldx_ = p.ldx;
  b.push([=](hipStream_t s) { return quantize_mx(q, sc, xp, M_, K_, ldx_, K_, lds, s); }, "quantize_mx", 0, 3.0 * M_ * K_,
         "rows" + std::to_string(M_) + " C" + std::to_string(K_));
  p.x = reinterpret_cast<const f16*>(q); p.ldx = p.K;
  p.w = reinterpret_cast<const f16*>(mxslab + it->second.q_off); p.ldw = it->second.cols;
  p.mx_sx = sc; p.mx_ldsx = lds;
  p.mx_sw = reinterpret_cast<const uint8_t*>(mxslab + it->second.s_off); p.mx_ldsw = it->second.cols / 32;
  if (!b.dry && !b.share) ++mx_launches;
  b.mx_tmp.push_back(xq); b.mx_tmp.push_back(xs);
}

// weight-bound shapes stream the fp8 copy of their matrix (same numbers: the fp16 copy holds the dequantised values); where
// the measured fp16 plan is a halo-reuse 3x3 kernel (activation-bound: M = 512 at long K) that kernel keeps the job
void Fp8State::use_fp8_weights(ConvGemm& p, int Mplan, const char* slab) const {
  if (p.mx_sx || weight_bits != 8 || Mplan > 512 || p.Cin % 64 != 0 || p.ups || p.bias_per_row || conv_gemm_plan_is_halo(p)) return;
  auto it = qindex.find((size_t)(reinterpret_cast<const char*>(p.w) - slab));
  if (it == qindex.end()) return;
  const QRegion& q = qregions[it->second];
  if (q.cols != p.ldw || p.N > q.rows) return;
  p.w = reinterpret_cast<const f16*>(q8slab + q.q_off);
  p.wscale = reinterpret_cast<const float*>(q8slab + q.s_off);
}

}  // namespace sdeo

namespace {

// GroupNorm + SiLU -> conv3x3 -> GroupNorm + SiLU -> conv3x3, plus x (through a conv1x1 when the channel count changes); every conv
// feeds a GroupNorm.  The UNet's ResBlock (`openaimodel.py:255-275`; o1 adds the time embedding) and, under the VAE's names and eps,
// its ResnetBlock (`model.py:82-128`, no time embedding, dropout 0)
static T build_resblock(Builder& b, const std::string& p, bool vae, const T& x, int cin, int cout, Builder::CO o1, const T* out = nullptr) {
  static const char* const nm[2][5] = {{".in_layers.0", ".in_layers.2", ".out_layers.0", ".out_layers.3", ".skip_connection"},
                                       {".norm1", ".conv1", ".norm2", ".conv2", ".nin_shortcut"}};
  const float eps = vae ? 1e-6f : 1e-5f;
  o1.gn_next = true;
  T h1 = b.gn_conv(x, p + nm[vae][0], eps, 1, p + nm[vae][1], cout, o1);
  T skip;
  if (cin != cout) skip = b.conv(x, p + nm[vae][4], cout, 1, 1, 0);
  Builder::CO o2;
  o2.res = cin != cout ? &skip : &x;
  o2.out = out;
  o2.gn_next = true;
  T y = b.gn_conv(h1, p + nm[vae][2], eps, 1, p + nm[vae][3], cout, o2);
  b.release(h1);
  if (cin != cout) b.release(skip);
  return y;
}
static T build_vae_res(Builder& b, const std::string& p, const T& x, int cin, int cout) { return build_resblock(b, p, true, x, cin, cout, Builder::CO()); }

static T build_res(Builder& b, const std::string& ns, const Blk& blk, const T& x, int net, const T* out = nullptr) {
  const std::string p = ns + blk.name;
  b.half = b.share || b.half_all;      // the ResBlock in front of the first transformer: both halves of the CFG pair are the same images
  Builder::CO o1;
  o1.bias2_off = b.e->emb_row.at(p);
  o1.bias2 = b.e->emb_all[net] + o1.bias2_off;     // what planning / autotune see; the launch reads emb_cur / emb_ld_cur
  o1.ld_bias2 = b.e->emb_total[net];
  o1.bias2_cur = &b.e->emb_cur[net];
  o1.ld_bias2_cur = &b.e->emb_ld_cur[net];
  T y = build_resblock(b, p, false, x, blk.cin, blk.cout, o1, out);
  b.half = b.half_all;
  return y;
}

// SpatialTransformer.forward + BasicTransformerBlock._forward (`attention.py:381-385,431-450`).  Each pre-LN sub-block
// x + f(LN(x)) runs as: [GEMM that writes x also writes x's per-row statistics] -> [GEMM of f's first Linear on the RAW x with
// LN folded in] -> ... ; see the file comment.
// kv: cross-attention K | V of this block, computed from the context: [N*TkS][2C] (K in columns 0..C-1, V in C..2C-1)
// kv_ip: K_ip | V_ip of the same block from the image tokens, [N*round8(ip_tokens)][2C] (UNet blocks of an adapter handle), or null
static T build_attn(Builder& b, const std::string& ns, const Blk& blk, const T& x, const T& kv, const T* kv_ip, const T* out = nullptr) {
  const sdeo_config& c = b.e->cfg;
  const std::string p = ns + blk.name;
  const std::string t = p + ".transformer_blocks.0";
  const int C = blk.cin, H = blk.heads, d = C / H, N = x.n, Tq = x.h * x.w;
  const int TkS = round8(c.context_len);
  // b.share: x holds the first N / 2 images only and everything up to attn2.to_q runs on them; the cross-attention (per-image K / V),
  // attn2.to_out and the last GEMM run at full batch and read q2 / tok1 / x of image i - N / 2 for the second half
  b.half = b.share || b.half_all;
  T g = b.gn(x, p + ".norm", 1e-6f, 0);
  RowStats st0 = b.alloc_stats(x.rows(), C), st1 = b.alloc_stats(x.rows(), C), st2 = b.alloc_stats(x.rows(), C);
  Builder::CO pi; pi.stats = &st0;
  T tok = b.conv(g, p + ".proj_in", C, 1, 1, 0, pi);
  b.release(g);
  // attn1 (self): q | k | v = LN1(tok) [Wq; Wk; Wv]^T in one GEMM
  Builder::CO l1; l1.ln = &st0; l1.ln_s = b.named_v(t + ".attn1.qkv_ln.s");
  T qkv = b.gemm(tok, b.named_w(t + ".attn1.qkv_ln.w"), C, 3 * C, b.named_v(t + ".attn1.qkv_ln.b"), l1);
  T o1 = b.alloc(x.n, x.h, x.w, C);
  b.attn(o1, qkv.p, 3 * C, qkv.p + C, 3 * C, qkv.p + 2 * C, 3 * C, N, H, Tq, Tq, Tq, Tq, d);
  b.release(qkv);
  Builder::CO r1; r1.res = &tok; r1.stats = &st1;
  T tok1 = b.gemm(o1, b.wptr(t + ".attn1.to_out.0.weight"), C, C, b.vptr(t + ".attn1.to_out.0.bias"), r1);
  b.release(o1);
  b.release(tok);
  // attn2 (cross, K | V precomputed from the context)
  Builder::CO l2; l2.ln = &st1; l2.ln_s = b.named_v(t + ".attn2.q_ln.s");
  T q2 = b.gemm(tok1, b.named_w(t + ".attn2.q_ln.w"), C, C, b.named_v(t + ".attn2.q_ln.b"), l2);
  b.half = b.half_all;
  T o2 = b.alloc(x.n, x.h, x.w, C);
  // (+ the image-prompt segment: softmax(q K^T) V + ip_scale softmax(q K_ip^T) V_ip, still one launch)
  if (kv_ip) b.attn(o2, q2.p, C, kv.p, 2 * C, kv.p + C, 2 * C, N, H, Tq, c.context_len, TkS, TkS, d, b.share ? N / 2 : 0,
                    kv_ip->p, kv_ip->p + C, 2 * C, b.e->ip_tokens, round8(b.e->ip_tokens));
  else b.attn(o2, q2.p, C, kv.p, 2 * C, kv.p + C, 2 * C, N, H, Tq, c.context_len, TkS, TkS, d, b.share ? N / 2 : 0);
  b.release(q2);
  // ff.net.2 and proj_out are two Linear maps with only the residual add between them: composed at finalisation into ONE [C][5C]
  // matrix over the row-concatenated operand [GEGLU output (4C) | tok2 (C)] (ComposeJob), so attn2.to_out writes tok2 into the last C
  // columns of that operand, the GEGLU GEMM writes the first 4C, and one GEMM replaces two launches
  T cat = b.alloc(x.n, x.h, x.w, 5 * C);
  const T gg = cat.view(0, 4 * C), tok2v = cat.view(4 * C, C);
  Builder::CO r2; r2.res = &tok1; r2.res_half = b.share; r2.stats = &st2; r2.out = &tok2v;
  T tok2 = b.gemm(o2, b.wptr(t + ".attn2.to_out.0.weight"), C, C, b.vptr(t + ".attn2.to_out.0.bias"), r2);
  b.release(o2);
  b.release(tok1);
  // GEGLU feed-forward: LN3 + ff.net.0.proj + GEGLU in one launch (act 3: value * gelu(gate) in the GEMM epilogue, 4C columns out)
  {
    Builder::CO og; og.act = 3; og.out = &gg; og.ln = &st2; og.ln_s = b.named_v(t + ".ff1_ln.s");
    b.gemm(tok2, b.named_w(t + ".ff1_ln.w"), C, 8 * C, b.named_v(t + ".ff1_ln.b"), og);
  }
  b.release_stats();
  Builder::CO ro; ro.res = &x; ro.res_half = b.share; ro.out = out; ro.gn_next = true;
  ro.w_ovr = b.named_w(t + ".ffproj.w"); ro.b_ovr = b.named_v(t + ".ffproj.b");
  T y = b.conv(cat, p + ".proj_out", C, 1, 1, 0, ro);
  b.release(cat);
  return y;
}

// time_embed MLP + stacked emb_layers projection: int64 t[rows] -> fp32 out[rows][emb_total[net]]
static void build_time_embed(Builder& b, const std::string& ns, int net, int rows, const int64_t* tp, float* out) {
  const sdeo_config& c = b.e->cfg;
  const int mc = c.model_channels, emb = 4 * mc, total = b.e->emb_total[net];
  T te = b.alloc2d(rows, mc);
  {
    f16* o = te.p;
    b.push([=](hipStream_t s) { return timestep_embedding(o, tp, rows, mc, s); });
  }
  // The per-forward embedding (rows = N) runs the plans of the schedule's table (kTabRows rows): a row of the table and the same
  // timestep passed as t are then the same instruction sequence, which is what SDEO_TIMESTEP_ROW promises (include/sdeo.h: a cached
  // read is bit-identical).  Planned on their own rows the two part at full width: time_embed.2 (1280 x 1280) splits K at N rows
  // and does not at 128, and the sums come out in another order.  (The operand form stays that of the launch's own rows: with
  // block-scaled activations asked for from 128 rows down, a test setting, the table is packed to fp8 and these are not, as before.)
  Builder::CO a; a.act = 1; a.plan_rows = Engine::kTabRows;
  Builder::CO last; last.plan_rows = Engine::kTabRows;
  b.advance(te, b.gemm(te, b.wptr(ns + "time_embed.0.weight"), mc, emb, b.vptr(ns + "time_embed.0.bias"), a));
  // every consumer of emb applies SiLU first (emb_layers = SiLU -> Linear), so store SiLU(emb)
  b.advance(te, b.gemm(te, b.wptr(ns + "time_embed.2.weight"), emb, emb, b.vptr(ns + "time_embed.2.bias"), a));
  b.gemm(te, b.named_w(ns + "emb_all.weight"), emb, total, b.named_v(ns + "emb_all.bias"), last, out, total);
  b.release(te);
}

static std::vector<const Blk*> attn_blocks(const UPlan& p) {
  std::vector<const Blk*> v;
  for_each_block(p, [&](const Blk& b) { if (b.kind == B_ATTN) v.push_back(&b); });
  return v;
}

// AttnBlock (`model.py:179-203`) of the VAE decoder and encoder: single head of x.c channels over the x.h * x.w tokens of one image;
// consumes (releases) hcur, returns x + proj_out(attention)
static T build_vae_attn(Builder& b, const std::string& p, T hcur) {
  const int bin = hcur.c, h = hcur.h, w = hcur.w;
  const int Tn = h * w;
  T g = b.gn(hcur, p + ".norm", 1e-6f, 0);
  T q = b.conv(g, p + ".q", bin, 1, 1, 0);
  T k = b.conv(g, p + ".k", bin, 1, 1, 0);
  T o;
  if ((bin % 8 == 0 && bin <= 160) || bin == 256 || bin == 512) {
    // flash attention (d = 512 on the wide-head kernel: the four waves of a workgroup split the channels)
    T v = b.conv(g, p + ".v", bin, 1, 1, 0);
    b.release(g);
    o = b.alloc(1, h, w, bin);
    b.attn(o, q.p, q.ld, k.p, k.ld, v.p, v.ld, 1, 1, Tn, Tn, Tn, Tn, bin);
    b.release(q);
    b.release(k);
    b.release(v);
  } else {
    // other widths: scores materialised in fp32, row softmax, second GEMM
    T vt = b.gemm_t(g, b.wptr(p + ".v.weight"), bin, bin, b.vptr(p + ".v.bias"));
    b.release(g);
    T s32 = b.alloc2d(Tn, Tn * 2);
    float* sp = reinterpret_cast<float*>(s32.p);
    b.gemm(q, k.p, k.ld, Tn, nullptr, Builder::CO(), sp, Tn);
    b.release(q);
    b.release(k);
    T pr = b.alloc2d(Tn, Tn);
    {
      f16* pp = pr.p; const float sc = 1.0f / sqrtf((float)bin);
      b.push([=](hipStream_t s) { return softmax_rows(pp, Tn, sp, Tn, Tn, Tn, sc, s); });
    }
    b.release(s32);
    o = b.gemm(pr, vt.p, vt.ld, bin, nullptr);
    o.n = 1; o.h = h; o.w = w;
    b.release(pr);
    b.release(vt);
  }
  Builder::CO ro; ro.res = &hcur; ro.gn_next = true;
  T yo = b.conv(o, p + ".proj_out", bin, 1, 1, 0, ro);
  b.release(o);
  b.release(hcur);
  return yo;
}

struct BuildCtx {      // state of one build_all pass
  Builder b;
  int N, h, w, TkS, nctrl;
  std::unordered_map<std::string, T> kv[kNets];   // per net: attn block name -> cached K | V
  T ctx16, hint_feat[kMaxControlNets];            // per control net: the cached output of its hint block
  // image-prompt adapter: the padded fp16 tokens and, per UNet attn block, the cached K_ip | V_ip
  T ip16;
  std::unordered_map<std::string, T> kv_ip;
};

// persistent tensors first (never released): controls, context, cached K/V^T, hint features
static void build_persistent(BuildCtx& c) {
  Builder& b = c.b; Engine* e = b.e;
  const UPlan& cp = e->cplan;
  for (int i = 0; i < c.nctrl; ++i) {
    const size_t j = std::min((size_t)i, cp.in_ch.size() - 1);       // the middle block's control is shaped like the last input block's
    e->ctrl[i] = b.alloc(c.N, c.h / cp.in_ds[j], c.w / cp.in_ds[j], cp.in_ch[j]);
  }
  c.ctx16 = b.alloc2d(c.N * c.TkS, e->cfg.context_dim);
  c.hint_feat[0] = b.alloc(c.N, c.h, c.w, e->cfg.model_channels);
  e->x0 = b.alloc(c.N, c.h, c.w, round8(e->cfg.in_channels));
  e->eps16 = b.alloc(c.N, c.h, c.w, 4 * ((e->cfg.out_channels + 3) / 4));
  for (int net = 0; net < 2 + e->extra; ++net) {        // (the extra nets' tensors behind everything a plain handle places)
    if (net >= 2) c.hint_feat[net - 1] = b.alloc(c.N, c.h, c.w, e->cfg.model_channels);
    for (const Blk* ab : attn_blocks(net ? e->cplan : e->uplan)) c.kv[net][net_ns(net) + ab->name] = b.alloc2d(c.N * c.TkS, 2 * ab->cin);
  }
  if (e->ip_tokens) {                                   // (the adapter's tensors behind those again)
    const int TS = round8(e->ip_tokens);
    c.ip16 = b.alloc2d(c.N * TS, e->cfg.context_dim);
    for (const Blk* ab : attn_blocks(e->uplan)) c.kv_ip[net_ns(0) + ab->name] = b.alloc2d(c.N * TS, 2 * ab->cin);
  }
}

// latent in: NCHW fp32 -> NHWC fp16, once for both networks; eps out: the reverse
static void build_latent_io(BuildCtx& c) {
  Builder& b = c.b; Engine* e = b.e;
  const int N = c.N, HW = c.h * c.w;
  b.prog = &e->prog[P_X0];
  f16* o = e->x0.p; const float* in = e->in_x; const int Cc = e->cfg.in_channels, ld = e->x0.ld;
  b.push([=](hipStream_t s) { return nchw_f32_to_nhwc_f16(o, ld, in, N, Cc, HW, 1.0f, s); });
  b.prog = &e->prog[P_EPS_EXPORT];
  float* eo = e->out_eps; const f16* ein = e->eps16.p; const int eld = e->eps16.ld, Ce = e->cfg.out_channels;
  b.push([=](hipStream_t s) { return nhwc_f16_to_nchw_f32(eo, ein, eld, N, Ce, HW, 1.0f, s); });
}

// time embedding: per forward (rows = N, t from in_t) and per schedule (rows = kTabRows, t from tab_t), every network
// (a ControlNet's runs on the side stream beside the UNet encoder: its temporaries and split-K workspace are the side stream's)
static void build_time_embeds(BuildCtx& c) {
  Builder& b = c.b; Engine* e = b.e;
  for (int net = 0; net < 2 + e->extra; ++net) {
    b.prog = net == 0 ? &e->prog[P_TEMB] : &cn_prog(e, net - 1, CP_TEMB);
    b.on_lane(&e->lanes[net >= 1 ? L_SIDE : L_MAIN], [&] { build_time_embed(b, net_ns(net), net, c.N, e->in_t, e->emb_all[net]); });
  }
  b.prog = &e->prog[P_TEMB_TAB];
  for (int net = 0; net < 2 + e->extra; ++net) build_time_embed(b, net_ns(net), net, Engine::kTabRows, e->tab_t, e->temb_tab[net]);
}

// context programs: fp32 [N][77][768] -> fp16 padded; K | V = ctx [Wk; Wv]^T per attn block, one GEMM each
static void build_context(BuildCtx& c, int net) {
  Builder& b = c.b; Engine* e = b.e;
  b.prog = net == 0 ? &e->prog[P_CTX_UNET] : &cn_prog(e, net - 1, CP_CTX);
  f16* o = c.ctx16.p; const float* in = e->in_ctx; const int N = c.N, T_ = e->cfg.context_len, TkS = c.TkS, Cd = e->cfg.context_dim;
  b.push([=](hipStream_t s) { return pad_rows_f32_to_f16(o, in, N, T_, TkS, Cd, s); });
  for (const Blk* ab : attn_blocks(net ? e->cplan : e->uplan)) {
    const std::string name = net_ns(net) + ab->name;
    Builder::CO kvo; kvo.out = &c.kv[net][name];
    b.gemm(c.ctx16, b.named_w(name + ".transformer_blocks.0.attn2.to_kv"), e->cfg.context_dim, 2 * ab->cin, nullptr, kvo);
  }
}

// image-prompt program (sdeo_set_ip_tokens): fp32 [N][T][ctx] -> fp16 rows padded to round8(T); K_ip | V_ip = tokens [Wk_ip; Wv_ip]^T
// per UNet attn block, one GEMM each
static void build_context_ip(BuildCtx& c) {
  Builder& b = c.b; Engine* e = b.e;
  b.prog = &e->prog[P_CTX_IP];
  f16* o = c.ip16.p; const float* in = e->in_ip; const int N = c.N, T_ = e->ip_tokens, TS = round8(T_), Cd = e->cfg.context_dim;
  b.push([=](hipStream_t s) { return pad_rows_f32_to_f16(o, in, N, T_, TS, Cd, s); });
  for (const Blk* ab : attn_blocks(e->uplan)) {
    const std::string name = net_ns(0) + ab->name;
    Builder::CO kvo; kvo.out = &c.kv_ip[name];
    b.gemm(c.ip16, b.named_w(name + ".transformer_blocks.0.attn2.to_kv_ip"), Cd, 2 * ab->cin, nullptr, kvo);
  }
}

// hint program of control net j (`cldm/cldm.py:147-163,288`): 8 conv3x3, SiLU between, cached across steps
static void build_hint(BuildCtx& c, int j) {
  Builder& b = c.b; Engine* e = b.e;
  b.prog = &cn_prog(e, j, CP_HINT);
  const std::string ns = net_ns(1 + j);
  T x = b.alloc(c.N, 8 * c.h, 8 * c.w, round8(e->cfg.hint_channels));
  f16* xp = x.p; const float* in = e->in_hint[j]; const int N = c.N, Cc = e->cfg.hint_channels, ld = x.ld, HW = 64 * c.h * c.w;
  b.push([=](hipStream_t s) { return nchw_f32_to_nhwc_f16(xp, ld, in, N, Cc, HW, 1.0f, s); });
  for (size_t i = 0; i < e->hconvs.size(); ++i) {
    const HintConv& hc = e->hconvs[i];
    Builder::CO o;
    o.act = i + 1 < e->hconvs.size() ? 1 : 0;
    o.cout_store = round8(hc.cout);
    if (i + 1 == e->hconvs.size()) o.out = &c.hint_feat[j];
    b.advance(x, b.conv(x, ns + hc.name, hc.cout, 3, hc.stride, 0, o));
  }
}

static T run_blocks(BuildCtx& c, const std::string& ns, const std::vector<Blk>& blocks, T x, bool release_in, int net, const T* final_out) {
  Builder& b = c.b;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const Blk& blk = blocks[i];
    const T* out = (i + 1 == blocks.size()) ? final_out : nullptr;
    T y;
    switch (blk.kind) {
      case B_RES: y = build_res(b, ns, blk, x, net, out); break;
      case B_ATTN: y = build_attn(b, ns, blk, x, c.kv[net].at(ns + blk.name), net == 0 && b.e->ip_tokens ? &c.kv_ip.at(ns + blk.name) : nullptr, out); break;
      default: {   // B_CONV_IN / B_DOWN / B_UP: one conv3x3, stride 2 (Downsample) or over the nearest-x2 source (Upsample)
        Builder::CO o; o.out = out; o.gn_next = true;
        y = b.conv(x, ns + blk.name + conv_suffix(blk.kind), blk.cout, 3, blk.kind == B_DOWN ? 2 : 1, blk.kind == B_UP ? 1 : 0, o);
      }
    }
    if (release_in || i > 0) b.release(x);
    x = y;
  }
  return x;
}

// input_blocks.1 built twice from the same arena state: as it is, into the current program, and as the variant whose ops in front of
// the first cross-attention run on the first N / 2 images (Builder::share), into sp.var.  Both place every tensor at the same address,
// so the rest of the program, the zero convs and the decoder serve either; splice() puts the variant program together.
struct Splice { size_t first = 0, last = 0; Program var; bool on = false; };
static T build_shared_prefix(BuildCtx& c, const std::string& ns, const std::vector<Blk>& blocks, const T& x, int net, Splice& sp) {
  Builder& b = c.b;
  Arena& arena = *b.lane->arena;
  const Arena before = arena;
  sp.first = b.prog->size();
  T y = run_blocks(c, ns, blocks, x, false, net, nullptr);
  sp.last = b.prog->size();
  if (c.N % 2 || blocks.size() != 2 || blocks[0].kind != B_RES || blocks[1].kind != B_ATTN) return y;
  Arena after = arena;
  arena = before;
  Program* prog = b.prog;
  b.prog = &sp.var; b.share = true;
  T ys = run_blocks(c, ns, blocks, x, false, net, nullptr);
  b.prog = prog; b.share = false;
  if ((ys.p != y.p || ys.gnp != y.gnp || ys.gn_slots != y.gn_slots || arena.end != after.end) && b.err.empty())
    b.err = "the shared-prefix variant of " + ns + blocks[0].name + " plans another arena";
  after.peak = std::max(after.peak, arena.peak);
  arena = after;
  sp.on = true;
  return y;
}
static void splice(const BuildCtx& c, Program& out, const Program& full, const Splice& sp) {
  if (c.b.dry || !sp.on) return;
  out.assign(full.begin(), full.begin() + sp.first);
  out.insert(out.end(), sp.var.begin(), sp.var.end());
  out.insert(out.end(), full.begin() + sp.last, full.end());
}

// ControlNet program of control net j (`cldm/cldm.py:284-305`).  Every net writes its 13 controls into the same e->ctrl: only
// sdeo_controlnet_forward[_net] runs the zero convs here, one net per call.
// half_prog: the same network on the first N / 2 images into e->cn_half[j], for a net in SDEO_CONTROL_COND: no zero convs (the fused
// decoder applies them), every launch a batch prefix of its full-batch one, from the arena state the full program was built from and
// therefore in the same tensors (checked).
static void build_controlnet(BuildCtx& c, int j, bool half_prog = false) {
  Builder& b = c.b; Engine* e = b.e;
  Splice sp;
  Program& p_cn = half_prog ? e->cn_half[j] : cn_prog(e, j, CP_CN);
  b.prog = &p_cn;
  b.half_all = b.half = half_prog;
  const int net = 1 + j;
  const std::string ns = net_ns(net);
  // The block outputs stay allocated (cn_h): sdeo_apply_model / sdeo_ddim_step skip the zero convs here and let the UNet decoder apply
  // them with the skip connection as the residual operand (P_UNET_DEC_FUSED); sdeo_controlnet_forward runs them here (13 controls out).
  auto zero_conv = [&](const T& x, const std::string& name, int cout, const T* out) {
    if (half_prog) return;
    const size_t first = p_cn.size();
    Builder::CO zo; zo.out = out;
    b.conv(x, name, cout, 1, 1, 0, zo);
    for (size_t k = first; k < p_cn.size(); ++k) p_cn[k].zero_conv = true;
  };
  T hcur = e->x0;
  for (size_t i = 0; i < e->cplan.in.size(); ++i) {
    if (i == 0) {
      // input_blocks.0 conv, then h += guided_hint (residual epilogue)
      Builder::CO o; o.res = &c.hint_feat[j]; o.gn_next = true;
      hcur = b.conv(hcur, ns + e->cplan.in[0][0].name, e->cfg.model_channels, 3, 1, 0, o);
    } else if (i == 1 && !half_prog) {
      hcur = build_shared_prefix(c, ns, e->cplan.in[i], hcur, net, sp);
    } else {
      hcur = run_blocks(c, ns, e->cplan.in[i], hcur, false, net, nullptr);
    }
    if (half_prog && hcur.p != e->cn_h[j][i].p && b.err.empty()) b.err = "the half-batch program of " + ns + " plans another arena";
    e->cn_h[j][i] = hcur;
    zero_conv(hcur, ns + "zero_convs." + std::to_string(i) + ".0", e->cplan.in_ch[i], &e->ctrl[i]);
  }
  T m = run_blocks(c, ns, e->cplan.mid, hcur, false, net, nullptr);
  if (half_prog && m.p != e->cn_h[j][c.nctrl - 1].p && b.err.empty()) b.err = "the half-batch program of " + ns + " plans another arena";
  e->cn_h[j][c.nctrl - 1] = m;
  zero_conv(m, ns + "middle_block_out.0", e->cplan.in_ch.back(), &e->ctrl[c.nctrl - 1]);
  b.half_all = b.half = false;
  if (!half_prog) splice(c, cn_prog(e, j, CP_CN_SH), p_cn, sp);
}

// control net j's programs: the full-batch one (with its shared-prefix variant) and, on a handle with sdeo_enable_control_modes and an
// even N, the half-batch one, built from the same arena state
static void build_controlnet_programs(BuildCtx& c, int j) {
  Builder& b = c.b; Engine* e = b.e;
  Arena& arena = *b.lane->arena;
  const Arena before = arena;
  build_controlnet(c, j);
  if (!e->control_modes || c.N % 2) return;
  Arena after = arena;
  arena = before;
  build_controlnet(c, j, true);
  if (arena.end != after.end && b.err.empty()) b.err = "the half-batch program of " + net_ns(1 + j) + " plans another arena";
  after.peak = std::max(after.peak, arena.peak);
  arena = after;
}

// control export (fp16 NHWC -> fp32 NCHW boundary buffers) and import
static void build_control_io(BuildCtx& c) {
  Engine* e = c.b.e;
  e->ctrl_elems.clear();
  for (int i = 0; i < c.nctrl; ++i) {
    const T& t = e->ctrl[i];
    e->ctrl_elems.push_back((size_t)t.n * t.c * t.h * t.w);
    if (c.b.dry) continue;
    float* o = e->out_ctrl[i]; const f16* in = t.p; const int N = c.N, ld = t.ld, Cc = t.c, HW = t.h * t.w;
    e->prog[P_CN_EXPORT].push_back([=](hipStream_t s) { return nhwc_f16_to_nchw_f32(o, in, ld, N, Cc, HW, 1.0f, s); });
    const float* ci = e->in_ctrl[i]; f16* co = t.p;
    e->prog[P_CTRL_IMPORT].push_back([=](hipStream_t s) { return nchw_f32_to_nhwc_f16(co, ld, ci, N, Cc, HW, 1.0f, s); });
  }
}

// The decoder (`openaimodel.py:797-801` with `cldm/cldm.py:33-41`): h = cat([h, hs.pop() + control.pop()]).  Three forms of the same
// program: no control; controls given as tensors (the 13-tensor boundary: one add per control); controls applied as the ControlNet's
// zero convs themselves, out = scale * zero_conv(cn_h) + skip written straight into the concat buffer (no add launches, no fp16
// round trip of the control).
enum DecoderMode { D_NOCTRL, D_ADD, D_FUSED };
// D_FUSED: every operand of the zero convs exists at the join (the ControlNet block outputs, the skips, the middle block's output), so
// all of them run as ONE multi-problem launch (kernels.h: conv_gemm_multi_plan) in front of the decoder, each writing its half of its
// stage's concat buffer -- which therefore all exist from the start.  A function of the configuration only: the fp16 LDS-DMA kernel
// takes every problem (channels in multiples of 64, at most kMultiMax of them) and no GEMM of the handle runs block-scaled fp8 (those
// zero convs keep their own packed launches).
static const int kZeroConvTile = 26;     // conv_gemm_dma_kernel<128,64,2>, four waves: measured against <64,64,4> and <64,160,3>
static bool zero_convs_as_one(const BuildCtx& c) {
  const Engine* e = c.b.e;
  if (c.nctrl > kMultiMax || e->fp8.act_bits == 8 || e->uplan.out.size() + 1 != (size_t)c.nctrl) return false;
  for (int i = 0; i < c.nctrl; ++i)
    if (e->cn_h[0][i].c % 64) return false;
  return true;
}
// The forms (Op::zc_form) net j's zero-conv launch exists in.  A plain handle: the one it always ran -- net 0 takes the skip as its
// residual (ZC_FIRST), every later net works in place over the running sum.  A handle with sdeo_enable_control_modes: either role (an
// OFF net in front makes a later net the first active one; net 0 can only be first), each on all rows and, for an even N, on the
// first half of the batch (ZC_COND), where the rows of the other half are passed through from the residual.
enum { ZC_COND = 1, ZC_FIRST = 2 };
static std::vector<int> zero_conv_forms(const BuildCtx& c, int j) {
  if (!c.b.e->control_modes) return {j == 0 ? ZC_FIRST : 0};
  std::vector<int> f = j == 0 ? std::vector<int>{ZC_FIRST} : std::vector<int>{0, ZC_FIRST};
  if (c.N % 2 == 0) for (size_t i = 0, n = f.size(); i < n; ++i) f.push_back(f[i] | ZC_COND);
  return f;
}
// The per-conv form of net j's zero conv `leaf` of control ci: out = scale * zero_conv(cn_h[j][ci]) + res in each form of the net, res
// being `skip` for the first active net and the running sum `out` behind it.  ZC_COND: the launch is the batch prefix of the full one
// (Builder::half) and, where the residual is not the output itself, one pass-through launch copies the other half's skip rows.
static void zero_conv_per_conv(BuildCtx& c, int j, int ci, const std::string& leaf, const T& out, const T& skip) {
  Builder& b = c.b; Engine* e = b.e;
  for (int form : zero_conv_forms(c, j)) {
    const size_t first = b.prog->size();
    const T& res = (form & ZC_FIRST) ? skip : out;
    Builder::CO zo; zo.out = &out; zo.res = &res; zo.scale_host = &e->eff_scales[j][ci];
    b.half = (form & ZC_COND) != 0;
    b.conv(e->cn_h[j][ci], net_ns(1 + j) + leaf, out.c, 1, 1, 0, zo);
    b.half = false;
    if ((form & ZC_COND) && res.p != out.p) {
      const int rows = out.rows() / 2, Cc = out.c, ldy = out.ld, lda = res.ld;
      f16* yp = out.p + (size_t)rows * ldy; const f16* ap = res.p + (size_t)rows * lda;
      b.push([=](hipStream_t s) { return add_scaled(yp, ldy, ap, lda, nullptr, 0, 1.0f, rows, Cc, s); }, "elementwise", 0, 4.0 * rows * Cc);
    }
    if (!b.dry) for (size_t k = first; k < b.prog->size(); ++k) { (*b.prog)[k].zc_net = (signed char)j; (*b.prog)[k].zc_form = (signed char)form; }
  }
}
static void build_unet_decoder_multi(BuildCtx& c, std::vector<T> hs, T cat0, T view0);
static void build_unet_decoder(BuildCtx& c, DecoderMode mode, std::vector<T> hs, T cat, T view) {
  Builder& b = c.b; Engine* e = b.e;
  const std::string ns = NS_UNET;
  if (mode == D_FUSED && zero_convs_as_one(c)) return build_unet_decoder_multi(c, hs, cat, view);
  int ci = c.nctrl - 1;
  if (mode == D_ADD) {   // h += control.pop()
    f16* yp = view.p; const int ld = view.ld, rows = view.rows(), Cc = view.c;
    const f16* cp = e->ctrl[ci].p; const int ldc = e->ctrl[ci].ld; const float* sc = &e->scales[ci];
    b.push([=](hipStream_t s) { return add_scaled(yp, ld, yp, ld, cp, ldc, *sc, rows, Cc, s); });
  } else if (mode == D_FUSED) {
    // every extra net chains behind net 0's conv, in place over the running sum (res == out), like the middle block's own
    for (int j = 0; j <= e->extra; ++j) zero_conv_per_conv(c, j, ci, "middle_block_out.0", view, view);
  }
  --ci;
  for (size_t oi = 0; oi < e->uplan.out.size(); ++oi) {
    // second half of the concat buffer: hs.pop() (+ control.pop() unless only_mid_control)
    T skip = hs.back();
    hs.pop_back();
    const int c_h = cat.c - skip.c;
    if (mode == D_FUSED) {
      const T half = cat.view(c_h, skip.c);
      for (int j = 0; j <= e->extra; ++j) zero_conv_per_conv(c, j, ci, "zero_convs." + std::to_string(ci) + ".0", half, skip);
    } else {
      f16* yp = cat.p + c_h; const int ld = cat.ld, rows = cat.rows(), Cc = skip.c;
      const f16* ap = skip.p; const int lda = skip.ld;
      const f16* cp = mode == D_ADD ? e->ctrl[ci].p : nullptr; const int ldc = mode == D_ADD ? e->ctrl[ci].ld : 0;
      const float* sc = &e->scales[ci]; const int* om = &e->only_mid;
      b.push([=](hipStream_t s) { return add_scaled(yp, ld, ap, lda, (*om) ? nullptr : cp, ldc, *sc, rows, Cc, s); });
    }
    b.freeu(cat, c_h);           // both halves of the concat are in place
    --ci;
    b.release(skip);
    const std::vector<Blk>& blocks = e->uplan.out[oi];
    if (oi + 1 < e->uplan.out.size()) {
      const T& nskip = hs.back();
      const int c_hn = blocks.back().cout;
      const int up = blocks.back().kind == B_UP ? 2 : 1;
      T ncat = b.alloc(cat.n, cat.h * up, cat.w * up, c_hn + nskip.c);
      const T nview = ncat.view(0, c_hn);
      run_blocks(c, ns, blocks, cat, true, 0, &nview);
      cat = ncat;
    } else {
      T y = run_blocks(c, ns, blocks, cat, true, 0, nullptr);
      Builder::CO oo; oo.cout_store = 4 * ((e->cfg.out_channels + 3) / 4);
      oo.out = &e->eps16;
      b.gn_conv(y, ns + "out.0", 1e-5f, 1, ns + "out.2", e->cfg.out_channels, oo);
      b.release(y);
    }
  }
}

static void build_unet_decoder_multi(BuildCtx& c, std::vector<T> hs, T cat0, T view0) {
  Builder& b = c.b; Engine* e = b.e;
  const std::string ns = NS_UNET;
  const size_t stages = e->uplan.out.size(), nh = hs.size();      // one skip per stage
  // the concat buffer of every stage; [0, c_h) of stage oi + 1 is written by stage oi's last block
  std::vector<T> cats{cat0};
  for (size_t oi = 0; oi + 1 < stages; ++oi) {
    const std::vector<Blk>& blocks = e->uplan.out[oi];
    const T& prev = cats.back();
    const int up = blocks.back().kind == B_UP ? 2 : 1;
    cats.push_back(b.alloc(prev.n, prev.h * up, prev.w * up, blocks.back().cout + hs[nh - 2 - oi].c));
  }
  // out = scale * zero_conv(cn_h[ci]) + skip into the second half of its stage's buffer (the middle block's: in place over view0)
  // Net 0's 13 problems are one launch; each extra net adds one more launch of the same tile whose 13 problems work in place on what
  // the launch before left (res == out, the form the middle block's problem has in every launch) under that net's scales.
  // (zc[j]: net j's problems with the running sum as the residual; zc_first[j]: with the skips, the form of the first active net)
  std::vector<ConvGemm> zc[kMaxControlNets], zc_first[kMaxControlNets];
  std::vector<const float*> zs[kMaxControlNets];
  auto zero_conv_net = [&](int j, int ci, const std::string& name, const T& out, const T& res) {
    const T& x = e->cn_h[j][ci];
    const WEntry* w = b.W(name + ".weight");
    if (w && w->ipad != x.c && b.err.empty()) b.err = "conv " + name + ": input has " + std::to_string(x.c) + " channels, weight expects " + std::to_string(w->ipad);
    ConvGemm p;
    p.x = x.p; p.w = b.wptr(name + ".weight"); p.bias = b.vptr(name + ".bias"); p.y = out.p; p.res = res.p;
    p.B = x.n; p.Hi = p.Ho = x.h; p.Wi = p.Wo = x.w; p.Cin = x.c;
    p.M = x.rows(); p.N = out.c; p.K = x.c;
    p.ldx = x.ld; p.ldw = p.K; p.ldy = out.ld; p.ldres = res.ld;
    zc_first[j].push_back(p);
    p.res = out.p; p.ldres = out.ld;
    zc[j].push_back(p);
    zs[j].push_back(&e->eff_scales[j][ci]);
  };
  auto zero_conv = [&](int ci, const std::string& leaf, const T& out, const T& res) {
    for (int j = 0; j <= e->extra; ++j) zero_conv_net(j, ci, net_ns(1 + j) + leaf, out, res);
  };
  int ci = c.nctrl - 1;
  zero_conv(ci--, "middle_block_out.0", view0, view0);
  for (size_t oi = 0; oi < stages; ++oi, --ci) {
    const T& skip = hs[nh - 1 - oi];
    zero_conv(ci, "zero_convs." + std::to_string(ci) + ".0", cats[oi].view(cats[oi].c - skip.c, skip.c), skip);
  }
  if (!b.dry)
    for (int j = 0; j <= e->extra; ++j)
      for (int form : zero_conv_forms(c, j)) {
        const std::vector<ConvGemm>& ps = (form & ZC_FIRST) ? zc_first[j] : zc[j];
        std::vector<int> live;               // ZC_COND: the rows of the first half of the batch
        if (form & ZC_COND) for (const ConvGemm& p : ps) live.push_back(p.M / 2);
        Op op = conv_gemm_multi_op(ps, kZeroConvTile, zs[j], live);
        op.zc_net = (signed char)j; op.zc_form = (signed char)form;
        b.prog->push_back(std::move(op));
      }
  for (T& skip : hs) b.release(skip);
  for (size_t oi = 0; oi < stages; ++oi) {
    const std::vector<Blk>& blocks = e->uplan.out[oi];
    b.freeu(cats[oi], cats[oi].c - hs[nh - 1 - oi].c);      // h from the stage before (the middle block), the skip from the launch above
    if (oi + 1 < stages) {
      const T nview = cats[oi + 1].view(0, blocks.back().cout);
      run_blocks(c, ns, blocks, cats[oi], true, 0, &nview);
    } else {
      T y = run_blocks(c, ns, blocks, cats[oi], true, 0, nullptr);
      Builder::CO oo; oo.cout_store = 4 * ((e->cfg.out_channels + 3) / 4);
      oo.out = &e->eps16;
      b.gn_conv(y, ns + "out.0", 1e-5f, 1, ns + "out.2", e->cfg.out_channels, oo);
      b.release(y);
    }
  }
}

// UNet programs (`cldm/cldm.py:22-45`): encoder + middle block into P_UNET_ENC (and its shared-prefix variant) with the two decoders that
// take controls, or everything into P_UNET_NOCTRL.  The middle block's output goes straight into the first concat buffer of the decoder
// (cat0, of which view0 is the middle block's part).  The two decoders start from the same encoder state: the arena is rewound between them
static void build_unet(BuildCtx& c, bool with_ctrl) {
  Builder& b = c.b; Engine* e = b.e;
  b.prog = &e->prog[with_ctrl ? P_UNET_ENC : P_UNET_NOCTRL];
  const std::string ns = NS_UNET;
  std::vector<T> hs;
  T hcur = e->x0;
  Splice sp;
  for (size_t i = 0; i < e->uplan.in.size(); ++i) {
    hcur = (i == 1 && with_ctrl) ? build_shared_prefix(c, ns, e->uplan.in[i], hcur, 0, sp) : run_blocks(c, ns, e->uplan.in[i], hcur, false, 0, nullptr);
    hs.push_back(hcur);
  }
  const int c_mid = e->uplan.mid.back().cout;
  const T cat0 = b.alloc(hcur.n, hcur.h, hcur.w, c_mid + hcur.c), view0 = cat0.view(0, c_mid);
  run_blocks(c, ns, e->uplan.mid, hcur, false, 0, &view0);
  if (!with_ctrl) return build_unet_decoder(c, D_NOCTRL, hs, cat0, view0);
  splice(c, e->prog[P_UNET_ENC_SH], e->prog[P_UNET_ENC], sp);
  Arena& arena = *b.lane->arena;
  const Arena after_encoder = arena;          // everything below needs the controls: runs after the join
  b.prog = &e->prog[P_UNET_DEC];
  build_unet_decoder(c, D_ADD, hs, cat0, view0);
  const size_t peak_add = arena.peak;
  arena = after_encoder;
  arena.peak = std::max(arena.peak, peak_add);
  b.prog = &e->prog[P_UNET_DEC_FUSED];
  build_unet_decoder(c, D_FUSED, hs, cat0, view0);
}

// VAE decode program, batch 1 (`model.py:619-652`; decode_first_stage wrapper: z/scale_factor -> post_quant_conv -> Decoder; the
// wrapper itself is absent from the reference tree)
static void build_vae_decoder(BuildCtx& c) {
  Builder& b = c.b; Engine* e = b.e;
  const sdeo_config& cfg = e->cfg;
  b.prog = &e->prog[P_VAE];
  const std::string d = std::string(NS_VAE) + "decoder";
  T z = b.alloc(1, c.h, c.w, round8(cfg.vae_z_channels));
  f16* zp = z.p; const float* zin = e->vae_in; const int zc = cfg.vae_z_channels, zld = z.ld, zHW = c.h * c.w;
  const float sc = 1.0f / cfg.vae_scale_factor;
  b.push([=](hipStream_t s) { return nchw_f32_to_nhwc_f16(zp, zld, zin, 1, zc, zHW, sc, s); });
  Builder::CO pq; pq.cout_store = round8(cfg.vae_z_channels);
  T hcur = z;
  b.advance(hcur, b.conv(hcur, std::string(NS_VAE) + "post_quant_conv", cfg.vae_z_channels, 1, 1, 0, pq));
  int bin = 0;
  auto levels = vae_levels(cfg, &bin);
  Builder::CO gnx; gnx.gn_next = true;       // every conv of the decoder below feeds a GroupNorm
  b.advance(hcur, b.conv(hcur, d + ".conv_in", bin, 3, 1, 0, gnx));
  b.advance(hcur, build_vae_res(b, d + ".mid.block_1", hcur, bin, bin));
  hcur = build_vae_attn(b, d + ".mid.attn_1", hcur);
  b.advance(hcur, build_vae_res(b, d + ".mid.block_2", hcur, bin, bin));
  int last = bin;
  for (auto& L : levels) {
    const std::string up = d + ".up." + std::to_string(L.level);
    for (size_t j = 0; j < L.blocks.size(); ++j) {
      b.advance(hcur, build_vae_res(b, up + ".block." + std::to_string(j), hcur, L.blocks[j].first, L.blocks[j].second));
      last = L.blocks[j].second;
    }
    if (L.up) b.advance(hcur, b.conv(hcur, up + ".upsample.conv", last, 3, 1, 1, gnx));
  }
  Builder::CO oo; oo.cout_store = 4 * ((cfg.vae_out_ch + 3) / 4);
  b.advance(hcur, b.gn_conv(hcur, d + ".norm_out", 1e-6f, 1, d + ".conv_out", cfg.vae_out_ch, oo));
  float* o = e->vae_out; uint8_t* u8 = e->vae_u8; const f16* in = hcur.p; const int ld = hcur.ld, Cc = cfg.vae_out_ch, HW = 64 * c.h * c.w;
  b.push([=](hipStream_t s) {
    if (int rc = nhwc_f16_to_nchw_f32(o, in, ld, 1, Cc, HW, 1.0f, s)) return rc;
    return nhwc_f16_to_nhwc_u8(u8, in, ld, HW, Cc, s);
  });
  b.release(hcur);
}

// VAE encode program, batch 1 (sdeo_enable_vae_encoder only): image intake -> Encoder (`model.py:452-545`) -> quant_conv -> posterior
// tail (encode_first_stage + get_first_stage_encoding; AutoencoderKL itself is absent from the reference tree)
static void build_vae_encoder(BuildCtx& c) {
  Builder& b = c.b; Engine* e = b.e;
  const sdeo_config& cfg = e->cfg;
  b.prog = &e->prog[P_VAE_ENC];
  const std::string d = std::string(NS_VAE) + "encoder";
  const int h = c.h, w = c.w, H = 8 * h, W = 8 * w, zc = cfg.vae_z_channels;
  T hcur = b.alloc(1, H, W, round8(cfg.vae_out_ch));
  f16* ip = hcur.p; const float* in = e->enc_img; const uint8_t* in8 = e->enc_img_u8; const int Cc = cfg.vae_out_ch, iHW = H * W;
  const int* from_u8 = &e->enc_from_u8;
  b.push([=](hipStream_t s) { return image_to_nhwc8_f16(ip, *from_u8 ? nullptr : in, in8, 1, Cc, iHW, s); }, "image_intake", 0,
         (4.0 + 16.0) * iHW);
  Builder::CO gnx; gnx.gn_next = true;       // every conv of the encoder up to norm_out feeds a GroupNorm
  b.advance(hcur, b.conv(hcur, d + ".conv_in", cfg.vae_ch, 3, 1, 0, gnx));
  int bi = cfg.vae_ch;
  for (int l = 0; l < cfg.vae_num_levels; ++l) {
    const std::string down = d + ".down." + std::to_string(l);
    const int bo = cfg.vae_ch * cfg.vae_ch_mult[l];
    for (int j = 0; j < cfg.vae_num_res_blocks; ++j) {
      b.advance(hcur, build_vae_res(b, down + ".block." + std::to_string(j), hcur, bi, bo));
      bi = bo;
    }
    if (l != cfg.vae_num_levels - 1) {        // Downsample: F.pad(x, (0,1,0,1)) + conv3x3 stride 2 pad 0 (`model.py:78-86`)
      Builder::CO o = gnx; o.pad_before = 0; o.pad_after = 1;
      b.advance(hcur, b.conv(hcur, down + ".downsample.conv", bi, 3, 2, 0, o));
    }
  }
  if ((hcur.h != h || hcur.w != w) && b.err.empty())
    b.err = "VAE encoder: " + std::to_string(H) + "x" + std::to_string(W) + " images encode to " + std::to_string(hcur.h) + "x" +
            std::to_string(hcur.w) + ", not the configured latent " + std::to_string(h) + "x" + std::to_string(w);
  b.advance(hcur, build_vae_res(b, d + ".mid.block_1", hcur, bi, bi));
  hcur = build_vae_attn(b, d + ".mid.attn_1", hcur);
  b.advance(hcur, build_vae_res(b, d + ".mid.block_2", hcur, bi, bi));
  Builder::CO oo; oo.cout_store = round8(2 * zc);
  b.advance(hcur, b.gn_conv(hcur, d + ".norm_out", 1e-6f, 1, d + ".conv_out", 2 * zc, oo));
  b.advance(hcur, b.conv(hcur, std::string(NS_VAE) + "quant_conv", 2 * zc, 1, 1, 0, oo));
  float* zp = e->enc_z; float* mp = e->enc_moments; const float* np_ = e->enc_noise; const int* with_noise = &e->enc_with_noise;
  const f16* qp = hcur.p; const int ld = hcur.ld, HW = h * w; const float sf = cfg.vae_scale_factor;
  b.push([=](hipStream_t s) { return vae_posterior(zp, mp, qp, ld, *with_noise ? np_ : nullptr, zc, HW, sf, s); }, "vae_posterior", 0,
         (2.0 * 2 * zc + 4.0 * 4 * zc) * HW);
  b.release(hcur);
}

}  // namespace

// One pass over every program of the handle, on fresh arenas and in a fixed order: the arena plan is a function of the order of alloc /
// release.  Out: the workspaces the launches need and what each lane's arena has to hold
int sdeo::build_all(Engine* e, bool dry, size_t* max_splitk, size_t* max_gn, size_t peaks[L_COUNT]) {
  Arena arenas[L_COUNT];
  for (int i = 0; i < L_COUNT; ++i) e->lanes[i].arena = &arenas[i];
  BuildCtx c{Builder{e, &e->lanes[L_MAIN], dry}, e->N, e->lh, e->lw, round8(e->cfg.context_len), (int)e->cplan.in.size() + 1};
  build_persistent(c);
  // small programs (their temporaries come and go: only after every persistent tensor has its place)
  build_latent_io(c);
  build_time_embeds(c);
  for (int net = 0; net < 2 + e->extra; ++net) build_context(c, net);
  if (e->ip_tokens) build_context_ip(c);
  for (int j = 0; j <= e->extra; ++j) build_hint(c, j);
  // the extra nets run on the side stream behind net 0; every net's block outputs stay allocated there until the decoder has run
  c.b.on_lane(&e->lanes[L_SIDE], [&] { for (int j = 0; j <= e->extra; ++j) build_controlnet_programs(c, j); });
  build_control_io(c);
  for (int variant = 0; variant < 2; ++variant) build_unet(c, variant == 0);
  // the three programs that hold a decoder, as built, are the FreeU programs; without their flagged launches, the ones a handle runs
  // with FreeU off: launch for launch what this pass builds when Builder::freeu pushes nothing
  static const ProgId kWithDecoder[3] = {P_UNET_DEC, P_UNET_DEC_FUSED, P_UNET_NOCTRL};
  for (int i = 0; i < 3; ++i) {
    Program& p = e->prog[kWithDecoder[i]];
    e->prog_freeu[i] = p;
    p.erase(std::remove_if(p.begin(), p.end(), [](const Op& op) { return op.freeu; }), p.end());
  }
  build_vae_decoder(c);
  if (e->vae_encoder) build_vae_encoder(c);
  for (int i = 0; i < L_COUNT; ++i) {
    e->lanes[i].arena = nullptr;
    peaks[i] = align_up(arenas[i].peak, 256);
  }
  *max_splitk = c.b.max_splitk; *max_gn = c.b.max_gn;
  SDEO_CHECK(c.b.err.empty(), "sdeo_configure: %s", c.b.err.c_str());
  return 0;
}
