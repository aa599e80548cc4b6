// Network executor of libsdeo: weight registry, static launch schedules ("programs") for ControlNet,
// ControlledUnetModel and the VAE decoder, and the net-level C entry points of include/sdeo.h.
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
#include <cmath>
#include <functional>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include/sdeo.h"
#include "handle_common.h"
#include "net_plan.h"

using namespace sdeo;

namespace {

static inline int round8(int c) { return (c + 7) / 8 * 8; }

// LayerNorm folded into a Linear at weight-finalisation time (fold_layernorm): offsets into the weight slab
struct FoldJob { size_t w_out, s_out, b_out, w_in; std::string gamma, beta, bias; int rows, C; };
// ff.net.2 and proj_out of one SpatialTransformer composed into one [C][5C] Linear at weight-finalisation time (compose_proj)
struct ComposeJob { size_t w_out, b_out; std::string wp, bp, w2, b2; int C; };
// a [rows][cols] fp16 matrix of the UNet / ControlNet that a conv / GEMM streams as its weight operand: with fp8 weights
// (sdeo_set_weight_precision) it gets an e4m3fn copy + per-row scales and its fp16 copy is replaced by the dequantised values
struct QRegion { size_t off; int rows, cols; size_t q_off, s_off; };

struct Builder;

// fp8 state of a handle: the per-row-scaled fp8 weight copies (sdeo_set_weight_precision) and the block-scaled packs
// (sdeo_set_activation_precision), with the two operand substitutions Builder::launch_conv applies, in this order
struct Fp8State {
  std::vector<QRegion> qregions;
  std::unordered_map<size_t, int> qindex;              // fp16 slab offset -> qregions index
  int weight_bits = 16;                                // 8: fp8 e4m3fn weights for the UNet / ControlNet matrices
  char* q8slab = nullptr;                              // fp8 codes + scales (allocated at the first fp8 finalize)
  size_t q8_bytes = 0;
  int act_bits = 16, mx_min_rows = 2048;               // 8: block-scaled fp8 activations x weights for GEMMs of >= mx_min_rows rows
  char* mxslab = nullptr;                              // block-scaled packs of the matrices (codes + e8m0 scales)
  size_t mx_bytes = 0;
  struct MxRegion { size_t q_off, s_off; int rows, cols; };
  std::unordered_map<size_t, MxRegion> mxindex;        // fp16 slab offset of a matrix -> its block-scaled pack
  int mx_launches = 0;                                 // GEMMs of the current programs that run on the block-scaled fp8 MFMA
  void use_mx(ConvGemm& p, int Mplan, Builder& b);
  void use_fp8_weights(ConvGemm& p, int Mplan, const char* slab) const;
};

// What the launches of one stream work in: an arena and the two workspaces.  The workspaces are sized by the programs, so they are
// allocated between the planning pass and the build pass: a launch reads them through the Lane* it captured.
struct Lane {
  Arena* arena = nullptr;        // planner of the build pass under way
  char* base = nullptr;          // device allocation the offsets of `arena` index, and its size
  size_t bytes = 0;
  float* splitk_ws = nullptr; size_t splitk_ws_bytes = 0;
  float* gn_ws = nullptr;
  WorkspaceRef splitk() const { return WorkspaceRef{&splitk_ws, &splitk_ws_bytes}; }
};
// L_SIDE: ControlNet runs concurrently with the UNet encoder on a stream of its own (both depend only on x, t, context), joined
// before the decoder consumes the controls
enum { L_MAIN, L_SIDE, L_COUNT };

constexpr int kMaxControls = 13;
// Control networks of one handle: net 0 is `control_model.`, nets 1.. the ones sdeo_enable_extra_controlnets registered under
// `control_model_<j>.`.  Per-network state is indexed by `net`: 0 = the UNet, 1 + j = control network j.
constexpr int kMaxControlNets = 4;
constexpr int kNets = 1 + kMaxControlNets;
// programs every control network has: net 0's are P_HINT / P_CTX_CN / P_CN / P_CN_SH / P_TEMB_CN, an extra net's live in Engine::xprog
enum CnProg { CP_HINT, CP_CTX, CP_CN, CP_CN_SH, CP_TEMB, CP_COUNT };

// Programs of a configured handle.  P_TEMB + net: the time embedding of the UNet (0) and of control net 0 (1).  P_UNET_ENC_SH / P_CN_SH: P_UNET_ENC / P_CN with
// input_blocks.1 up to its cross-attention run on the first N / 2 images only (build_shared_prefix); empty when N is odd or the block
// has no transformer
enum ProgId {
  P_HINT, P_CTX_CN, P_CTX_UNET, P_CN, P_CN_SH, P_CN_EXPORT, P_CTRL_IMPORT, P_UNET_ENC, P_UNET_ENC_SH, P_UNET_DEC, P_UNET_DEC_FUSED,
  P_UNET_NOCTRL, P_VAE, P_VAE_ENC, P_TEMB, P_TEMB_CN, P_TEMB_TAB, P_X0, P_EPS_EXPORT, P_COUNT
};

}  // namespace

struct sdeo_handle_s {
  sdeo_config cfg;
  int num_head_channels = 0;  // sdeo_config_ext: > 0 = heads of a block = C / num_head_channels (Blk::heads holds the result)
  bool use_linear = false;    // sdeo_config_ext: proj_in / proj_out of every SpatialTransformer are nn.Linear, weights (C, C)
  UPlan uplan, cplan;
  std::vector<HintConv> hconvs;
  WeightStore ws;                                      // registry, slab and loader of the checkpoint tensors
  std::unordered_map<std::string, size_t> named_off;   // extra named regions (stacked parents, LayerNorm-folded copies)
  std::vector<FoldJob> folds;
  std::vector<ComposeJob> composes;
  Fp8State fp8;
  bool finalized = false;
  // per-net stacked time-embedding projection
  int emb_total[kNets] = {0};
  std::unordered_map<std::string, int> emb_row;        // "<ns><resblock>" -> row offset
  // problem size, arenas + workspaces (lanes[L_MAIN].base != nullptr: configured), side stream
  int N = 0, lh = 0, lw = 0;
  Lane lanes[L_COUNT];
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool overlap = true;       // SDEO_OVERLAP=0 runs ControlNet and UNet back to back on one stream
  // boundary buffers (device, owned)
  float* in_x = nullptr; float* in_hint[kMaxControlNets] = {nullptr}; float* in_ctx = nullptr; int64_t* in_t = nullptr;
  float* in_ctrl[kMaxControls] = {nullptr};
  float* out_eps = nullptr;
  float* out_ctrl[kMaxControls] = {nullptr};
  float* vae_in = nullptr; float* vae_out = nullptr; uint8_t* vae_u8 = nullptr;
  // VAE encoder (sdeo_enable_vae_encoder): boundary buffers of one image, and what the next run of P_VAE_ENC reads (set by
  // sdeo_vae_encode, read at launch): the uint8 image instead of the fp32 one, the noise instead of the posterior mode
  bool vae_encoder = false;
  float* enc_img = nullptr; uint8_t* enc_img_u8 = nullptr; float* enc_noise = nullptr; float* enc_z = nullptr; float* enc_moments = nullptr;
  int enc_from_u8 = 0, enc_with_noise = 0;
  std::vector<void*> extra_allocs;
  // persistent activations
  T ctrl[kMaxControls];  // fp16 NHWC controls (ControlNet output / UNet input), unscaled
  T cn_h[kMaxControlNets][kMaxControls];  // per control net: the block outputs the zero convs read (kept until the UNet decoder has run)
  float scales[kMaxControls];
  // per control net: scales with only_mid_control folded in (0 for the twelve skip controls), read at launch by P_UNET_DEC_FUSED
  float eff_scales[kMaxControlNets][kMaxControls];
  int only_mid = 0;
  // extra control networks (sdeo_enable_extra_controlnets): how many, their programs, the scales sdeo_set_control_scales left
  // (extra_scales[j - 1], kept until changed)
  int extra = 0;
  Program xprog[kMaxControlNets - 1][CP_COUNT];
  float extra_scales[kMaxControlNets - 1][kMaxControls];
  // The cache contract (include/sdeo.h, "State a handle keeps between calls"): host-side record of what the caches hold, checked before
  // the first device call of every entry point that reads one on the caller's word.  A captured call is checked at capture.
  //   hint_set[j]:     net j's hint block ran since the last sdeo_configure (net 0: a forward given the hint; j >= 1: sdeo_set_control_hint)
  //   ctx_set:         whose context K / V were computed since the last sdeo_configure (bit 0 the UNet, bit 1 the control networks)
  //   ctx_epoch:       advances every time a new context is staged; ctx_epoch_of[side] is the epoch side's K / V were computed from
  //   x0_staged_for:   the caller's latent whose updated fp16 copy the last fused step left in x0; null once anything else wrote x0
  //   x0_staged_paired: that step was a CFG-pair step (b = N / 2 latents, each staged twice), not an unguided one (N latents, once)
  bool hint_set[kMaxControlNets] = {false};
  int ctx_set = 0;
  unsigned long long ctx_epoch = 0, ctx_epoch_of[2] = {0, 0};
  const float* x0_staged_for = nullptr;
  bool x0_staged_paired = true;
  // sdeo_lora_commit changed the weights under the caches: net j's hint features, the context K / V of the UNet (bit 0) and of the
  // control networks (bit 1), the timestep table.  Each stays stale until the call that fills it runs again; a call that asks for a
  // stale cache is refused.  A handle that never commits an adapter never sets them.
  bool hint_stale[kMaxControlNets] = {false};
  int ctx_stale = 0;
  bool tab_stale = false;
  // time embedding (`openaimodel.py:777-781` + every ResBlock's emb_layers): fp32 [N][emb_total] per net, written by P_TEMB + net from
  // in_t -- or, for a sampler that announced its schedule (sdeo_set_timestep_table), one row of a table computed once per schedule.
  // The ResBlock convs read their pointer / row stride at LAUNCH time (emb_cur / emb_ld_cur), like the control scales.
  static constexpr int kTabRows = 128;
  float* emb_all[kNets] = {nullptr};
  float* temb_tab[kNets] = {nullptr};          // [kTabRows][emb_total[net]]
  int64_t* tab_t = nullptr;                    // device int64 [kTabRows]
  int tab_count = 0;
  const float* emb_cur[kNets] = {nullptr};
  int emb_ld_cur[kNets] = {0};
  T x0;                  // fp16 NHWC copy of the latent input, shared by ControlNet and UNet (P_X0 writes it from in_x)
  T eps16;               // the UNet's eps before the NCHW fp32 export (P_EPS_EXPORT), read directly by sdeo_ddim_step
  Program prog[P_COUNT]; // free_configured clears them all
  std::vector<size_t> ctrl_elems;
  size_t device_bytes = 0;
  // profiling (sdeo_profile_*): HIP events around every launch of the next programs
  bool autotune = false;    // SDEO_AUTOTUNE=1: measure GEMM plans of untabled shapes at configure time (tuning aid; tools/tune_plans.py)
  Profiler prof;
};

namespace {

typedef sdeo_handle_s Engine;
// ------------------------------------------------------------------------------------------------
// registry construction
// ------------------------------------------------------------------------------------------------
struct Registry {
  Engine* e;
  bool quant = true;          // matrices registered now belong to the UNet / ControlNet (fp8-eligible), not the VAE
  void region(size_t off, int rows, int cols) {
    if (!quant) return;
    e->fp8.qindex[off] = (int)e->fp8.qregions.size();
    e->fp8.qregions.push_back(QRegion{off, rows, cols, 0, 0});
  }
  size_t take(size_t bytes) { return e->ws.take(bytes); }
  void add(const std::string& name, WKind kind, std::initializer_list<int64_t> dims, size_t off, int ipad = 0) {
    e->ws.add(name, kind, dims, off, ipad);
  }
  // conv: weight [cout][cin][k][k] -> fp16 [opad][k][k][ipad]; bias -> fp32 [opad]
  void conv(const std::string& name, int cin, int cout, int k, int opad = -1) {
    const int ip = round8(cin);
    const int op = opad < 0 ? cout : opad;
    const size_t off = take((size_t)op * k * k * ip * 2);
    add(name + ".weight", W_CONV, {cout, cin, k, k}, off, ip);
    region(off, op, k * k * ip);
    add(name + ".bias", W_VEC, {cout}, take((size_t)op * 4));
  }
  void lin(const std::string& name, int cin, int cout, bool bias) {
    const size_t off = take((size_t)cout * cin * 2);
    add(name + ".weight", W_LINEAR, {cout, cin}, off);
    region(off, cout, cin);
    if (bias) add(name + ".bias", W_VEC, {cout}, take((size_t)cout * 4));
  }
  // proj_in / proj_out of a SpatialTransformer: conv1x1 weights (c, c, 1, 1), or nn.Linear weights (c, c) when the handle was created with
  // use_linear_in_transformer.  c % 8 == 0, so both are stored as the same fp16 [c][c] matrix and run as the same row GEMM on NHWC
  void proj(const std::string& name, int c) {
    if (!e->use_linear) return conv(name, c, c, 1);
    const size_t off = take((size_t)c * c * 2);
    add(name + ".weight", W_LINEAR, {c, c}, off, c);
    region(off, c, c);
    add(name + ".bias", W_VEC, {c}, take((size_t)c * 4));
  }
  void vec(const std::string& name, int c) { add(name, W_VEC, {c}, take((size_t)c * 4)); }
  void norm(const std::string& name, int c) { vec(name + ".weight", c); vec(name + ".bias", c); }
};

static void reg_res(Registry& r, const std::string& ns, const Blk& b, int emb_dim, size_t emb_w_off, size_t emb_b_off, int& emb_row) {
  const std::string p = ns + b.name;
  r.norm(p + ".in_layers.0", b.cin);
  r.conv(p + ".in_layers.2", b.cin, b.cout, 3);
  // emb_layers.1 lives inside the stacked [sum(cout)][emb_dim] matrix of its network
  r.add(p + ".emb_layers.1.weight", W_LINEAR, {b.cout, emb_dim}, emb_w_off + (size_t)emb_row * emb_dim * 2);
  r.add(p + ".emb_layers.1.bias", W_VEC, {b.cout}, emb_b_off + (size_t)emb_row * 4);
  r.e->emb_row[p] = emb_row;
  emb_row += b.cout;
  r.norm(p + ".out_layers.0", b.cout);
  r.conv(p + ".out_layers.3", b.cout, b.cout, 3);
  if (b.cin != b.cout) r.conv(p + ".skip_connection", b.cin, b.cout, 1);
}

static void reg_attn(Registry& r, const std::string& ns, const Blk& b, int ctx) {
  const std::string p = ns + b.name;
  const int c = b.cin;
  r.norm(p + ".norm", c);
  r.proj(p + ".proj_in", c);
  const std::string t = p + ".transformer_blocks.0";
  // attn1: to_q, to_k, to_v stacked as one [3c][c] matrix (raw); the copy the network runs on has norm1 folded in
  const size_t qkv = r.take((size_t)3 * c * c * 2);
  r.add(t + ".attn1.to_q.weight", W_LINEAR, {c, c}, qkv);
  r.add(t + ".attn1.to_k.weight", W_LINEAR, {c, c}, qkv + (size_t)c * c * 2);
  r.add(t + ".attn1.to_v.weight", W_LINEAR, {c, c}, qkv + (size_t)2 * c * c * 2);
  r.lin(t + ".attn1.to_out.0", c, c, true);
  r.add(t + ".attn2.to_q.weight", W_LINEAR, {c, c}, r.take((size_t)c * c * 2));      // raw: only the input of its LayerNorm fold
  // attn2: to_k and to_v stacked as one [2c][ctx] matrix (one GEMM per context)
  const size_t kv = r.take((size_t)2 * c * ctx * 2);
  r.e->named_off[t + ".attn2.to_kv"] = kv;
  r.region(kv, 2 * c, ctx);
  r.add(t + ".attn2.to_k.weight", W_LINEAR, {c, ctx}, kv);
  r.add(t + ".attn2.to_v.weight", W_LINEAR, {c, ctx}, kv + (size_t)c * ctx * 2);
  r.lin(t + ".attn2.to_out.0", c, c, true);
  const size_t ff1 = r.take((size_t)8 * c * c * 2);
  r.add(t + ".ff.net.0.proj.weight", W_GEGLU_W, {8 * c, c}, ff1);
  r.add(t + ".ff.net.0.proj.bias", W_GEGLU_B, {8 * c}, r.take((size_t)8 * c * 4));
  r.lin(t + ".ff.net.2", 4 * c, c, true);
  // LayerNorm-folded copies (built by sdeo_finalize_weights): weights, row sums s, bias'
  auto fold = [&](const std::string& name, size_t w_in, int rows, const std::string& norm, const std::string& bias) {
    FoldJob f;
    f.w_out = r.take((size_t)rows * c * 2);
    f.s_out = r.take((size_t)rows * 4);
    f.b_out = r.take((size_t)rows * 4);
    f.w_in = w_in; f.gamma = norm + ".weight"; f.beta = norm + ".bias"; f.bias = bias; f.rows = rows; f.C = c;
    r.e->named_off[name + ".w"] = f.w_out;
    r.e->named_off[name + ".s"] = f.s_out;
    r.e->named_off[name + ".b"] = f.b_out;
    r.e->folds.push_back(f);
    r.region(f.w_out, rows, c);        // the folded copy is what the network streams (the raw one is only the fold's input)
  };
  fold(t + ".attn1.qkv_ln", qkv, 3 * c, t + ".norm1", "");
  fold(t + ".attn2.q_ln", r.e->ws.find(t + ".attn2.to_q.weight")->off, c, t + ".norm2", "");
  fold(t + ".ff1_ln", ff1, 8 * c, t + ".norm3", t + ".ff.net.0.proj.bias");
  r.norm(t + ".norm1", c);
  r.norm(t + ".norm2", c);
  r.norm(t + ".norm3", c);
  r.proj(p + ".proj_out", c);
  // ff.net.2 + proj_out as one Linear over [GEGLU output | tok2] (build_attn); no fp8 / block-scaled copy: the reference modules the
  // fp8 goldens come from round ff.net.2 and proj_out separately, and this product is formed from exactly those rounded values
  ComposeJob cj;
  cj.w_out = r.take((size_t)c * 5 * c * 2);
  cj.b_out = r.take((size_t)c * 4);
  cj.wp = p + ".proj_out.weight"; cj.bp = p + ".proj_out.bias"; cj.w2 = t + ".ff.net.2.weight"; cj.b2 = t + ".ff.net.2.bias"; cj.C = c;
  r.e->named_off[t + ".ffproj.w"] = cj.w_out;
  r.e->named_off[t + ".ffproj.b"] = cj.b_out;
  r.e->composes.push_back(cj);
}

// where the one conv3x3 of a conv-only block (B_CONV_IN / B_DOWN / B_UP) keeps its parameters below the block's name
static const char* conv_suffix(BlkKind k) { return k == B_DOWN ? ".op" : k == B_UP ? ".conv" : ""; }

static int plan_emb_total(const UPlan& p) {
  int t = 0;
  for_each_block(p, [&](const Blk& b) { if (b.kind == B_RES) t += b.cout; });
  return t;
}

static void reg_unet_like(Registry& r, const std::string& ns, const UPlan& p, const sdeo_config& c, int net) {
  const int emb = 4 * c.model_channels;
  r.lin(ns + "time_embed.0", c.model_channels, emb, true);
  r.lin(ns + "time_embed.2", emb, emb, true);
  const int total = plan_emb_total(p);
  r.e->emb_total[net] = total;
  const size_t ew = r.take((size_t)total * emb * 2);
  const size_t eb = r.take((size_t)total * 4);
  r.e->named_off[ns + "emb_all.weight"] = ew;
  r.region(ew, total, emb);
  r.e->named_off[ns + "emb_all.bias"] = eb;
  int row = 0;
  for_each_block(p, [&](const Blk& b) {
    switch (b.kind) {
      case B_RES: reg_res(r, ns, b, emb, ew, eb, row); break;
      case B_ATTN: reg_attn(r, ns, b, c.context_dim); break;
      default: r.conv(ns + b.name + conv_suffix(b.kind), b.cin, b.cout, 3);
    }
  });
}

static void reg_vae_res(Registry& r, const std::string& p, int cin, int cout) {
  r.norm(p + ".norm1", cin);
  r.conv(p + ".conv1", cin, cout, 3);
  r.norm(p + ".norm2", cout);
  r.conv(p + ".conv2", cout, cout, 3);
  if (cin != cout) r.conv(p + ".nin_shortcut", cin, cout, 1);
}

// namespace of network `net`'s tensors: the UNet, `control_model.`, `control_model_<j>.` for the extra control net j = net - 1
static std::string net_ns(int net) { return net == 0 ? NS_UNET : net == 1 ? NS_CN : "control_model_" + std::to_string(net - 1) + "."; }

// the full tensor set of one control network under its namespace
static void reg_controlnet(Registry& r, int net) {
  Engine* e = r.e;
  const std::string ns = net_ns(net);
  reg_unet_like(r, ns, e->cplan, e->cfg, net);
  for (size_t i = 0; i < e->cplan.in_ch.size(); ++i)
    r.conv(ns + "zero_convs." + std::to_string(i) + ".0", e->cplan.in_ch[i], e->cplan.in_ch[i], 1);
  for (auto& hc : e->hconvs) r.conv(ns + hc.name, hc.cin, hc.cout, 3, round8(hc.cout));
  r.conv(ns + "middle_block_out.0", e->cplan.in_ch.back(), e->cplan.in_ch.back(), 1);
}

static void build_registry(Engine* e) {
  Registry r{e};
  const sdeo_config& c = e->cfg;
  // UNet
  reg_unet_like(r, NS_UNET, e->uplan, c, 0);
  r.norm(std::string(NS_UNET) + "out.0", c.model_channels);
  r.conv(std::string(NS_UNET) + "out.2", c.model_channels, c.out_channels, 3, (c.out_channels + 3) / 4 * 4);
  reg_controlnet(r, 1);
  // VAE decode path
  r.quant = false;                   // the VAE stays fp16 (BASELINE configs[4])
  const std::string d = std::string(NS_VAE) + "decoder";
  r.conv(std::string(NS_VAE) + "post_quant_conv", c.vae_z_channels, c.vae_z_channels, 1, round8(c.vae_z_channels));
  int bin = 0;
  auto levels = vae_levels(c, &bin);
  r.conv(d + ".conv_in", c.vae_z_channels, bin, 3);
  reg_vae_res(r, d + ".mid.block_1", bin, bin);
  r.norm(d + ".mid.attn_1.norm", bin);
  for (const char* n : {"q", "k", "v", "proj_out"}) r.conv(d + ".mid.attn_1." + n, bin, bin, 1);
  reg_vae_res(r, d + ".mid.block_2", bin, bin);
  int last = bin;
  for (auto& L : levels) {
    for (size_t j = 0; j < L.blocks.size(); ++j) {
      reg_vae_res(r, d + ".up." + std::to_string(L.level) + ".block." + std::to_string(j), L.blocks[j].first, L.blocks[j].second);
      last = L.blocks[j].second;
    }
    if (L.up) r.conv(d + ".up." + std::to_string(L.level) + ".upsample.conv", last, last, 3);
  }
  r.norm(d + ".norm_out", last);
  r.conv(d + ".conv_out", last, c.vae_out_ch, 3, (c.vae_out_ch + 3) / 4 * 4);
}

// VAE encoder (`model.py:452-545`, attn_resolutions = [], double_z) + quant_conv, appended behind everything build_registry placed
// (sdeo_enable_vae_encoder): the offsets of the existing tensors do not move
static void reg_vae_encoder(Engine* e) {
  Registry r{e};
  r.quant = false;                   // fp16 like the decoder
  const sdeo_config& c = e->cfg;
  const std::string d = std::string(NS_VAE) + "encoder";
  const int zc2 = 2 * c.vae_z_channels;
  r.conv(d + ".conv_in", c.vae_out_ch, c.vae_ch, 3);
  int bi = c.vae_ch;
  for (int l = 0; l < c.vae_num_levels; ++l) {
    const int bo = c.vae_ch * c.vae_ch_mult[l];
    for (int j = 0; j < c.vae_num_res_blocks; ++j) {
      reg_vae_res(r, d + ".down." + std::to_string(l) + ".block." + std::to_string(j), bi, bo);
      bi = bo;
    }
    if (l != c.vae_num_levels - 1) r.conv(d + ".down." + std::to_string(l) + ".downsample.conv", bi, bi, 3);
  }
  reg_vae_res(r, d + ".mid.block_1", bi, bi);
  r.norm(d + ".mid.attn_1.norm", bi);
  for (const char* n : {"q", "k", "v", "proj_out"}) r.conv(d + ".mid.attn_1." + n, bi, bi, 1);
  reg_vae_res(r, d + ".mid.block_2", bi, bi);
  r.norm(d + ".norm_out", bi);
  r.conv(d + ".conv_out", bi, zc2, 3, round8(zc2));
  r.conv(std::string(NS_VAE) + "quant_conv", zc2, zc2, 1, round8(zc2));
}

// ------------------------------------------------------------------------------------------------
// program builder
// ------------------------------------------------------------------------------------------------
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
  bool share = false, half = false;
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
    // precision and scratch sizes follow the problem whose plan the launch takes (a half-batch launch: the full-batch one)
    const int Mplan = p.plan_B ? p.M / p.B * p.plan_B : p.M;
    e->fp8.use_mx(p, Mplan, *this);
    e->fp8.use_fp8_weights(p, Mplan, e->ws.slab);
    const size_t tune_ws = e->autotune ? conv_gemm_autotune_workspace_bytes(p) : 0;
    if (!dry && e->autotune && !share) {       // (the shared variant of a block runs the plans its full-batch build measured)
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
    if (!dry && !share && getenv("SDEO_DUMP_GEMM"))   // shape census for tools/tune_gemm.py
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
    if (o.res_half) p.res_rows = rows / 2;
    set_ln(p, o);
    if (o.ln && o.ln->c != x.c && err.empty()) err = "LayerNorm statistics of a " + std::to_string(o.ln->c) + "-channel tensor fed to K = " + std::to_string(x.c);
    launch_conv(p, o.scale_host, o.stats);
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

  // conv3x3(act(GroupNorm(x))) (`openaimodel.py:255-275`, `model.py:129-149`): GroupNorm launch(es) + conv
  T gn_conv(const T& x, const std::string& gn_name, float eps, int silu_, const std::string& conv_name, int cout, CO o) {
    T t = gn(x, gn_name, eps, silu_);
    T y = conv(t, conv_name, cout, 3, 1, 0, o);
    release(t);
    return y;
  }

  // qB: batches of q when the full-batch launch reads the queries of the first half twice (0: B).  Under `half` the first B / 2 batches run.
  void attn(const T& o, const f16* q, int ldq, const f16* k, int ldk, const f16* v, int ldv, int B, int H, int Tq, int Tk, int TkS, int TkSv, int d,
            int qB = 0) {
    AttnArgs a{o.p, q, k, v, o.ld, ldq, ldk, ldv, B, H, Tq, Tk, TkS, TkSv, d, 1.0f / sqrtf((float)d), 0};
    a.qB = qB;
    if (half) { a.plan_B = B; a.B = B / 2; }
    B = a.B;
    push([=](hipStream_t s) { return attention(a, s); }, "attention",
         4.0 * B * H * (double)Tq * Tk * d, 2.0 * B * H * d * (2.0 * Tq + 2.0 * Tk),
         "Tq" + std::to_string(Tq) + " Tk" + std::to_string(Tk) + " d" + std::to_string(d));
  }
};

// block-scaled fp8 on both sides: pack the activations (one launch), run the GEMM on the fp8 MFMA
void Fp8State::use_mx(ConvGemm& p, int Mplan, Builder& b) {
  if (!(act_bits == 8 && mxslab && Mplan >= mx_min_rows && p.R == 1 && p.S == 1 && p.stride == 1 && !p.ups && p.K % 128 == 0 &&
        p.K == p.Cin && p.ldx % 16 == 0 && !p.bias_per_row && p.y && !p.y32))
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
  b.half = b.share;              // the ResBlock in front of the first transformer: both halves of the CFG pair are the same images
  Builder::CO o1;
  o1.bias2_off = b.e->emb_row.at(p);
  o1.bias2 = b.e->emb_all[net] + o1.bias2_off;     // what planning / autotune see; the launch reads emb_cur / emb_ld_cur
  o1.ld_bias2 = b.e->emb_total[net];
  o1.bias2_cur = &b.e->emb_cur[net];
  o1.ld_bias2_cur = &b.e->emb_ld_cur[net];
  T y = build_resblock(b, p, false, x, blk.cin, blk.cout, o1, out);
  b.half = false;
  return y;
}

// SpatialTransformer.forward + BasicTransformerBlock._forward (`attention.py:381-385,431-450`).  Each pre-LN sub-block
// x + f(LN(x)) runs as: [GEMM that writes x also writes x's per-row statistics] -> [GEMM of f's first Linear on the RAW x with
// LN folded in] -> ... ; see the file comment.
// kv: cross-attention K | V of this block, computed from the context: [N*TkS][2C] (K in columns 0..C-1, V in C..2C-1)
static T build_attn(Builder& b, const std::string& ns, const Blk& blk, const T& x, const T& kv, const T* out = nullptr) {
  const sdeo_config& c = b.e->cfg;
  const std::string p = ns + blk.name;
  const std::string t = p + ".transformer_blocks.0";
  const int C = blk.cin, H = blk.heads, d = C / H, N = x.n, Tq = x.h * x.w;
  const int TkS = round8(c.context_len);
  // b.share: x holds the first N / 2 images only and everything up to attn2.to_q runs on them; the cross-attention (per-image K / V),
  // attn2.to_out and the last GEMM run at full batch and read q2 / tok1 / x of image i - N / 2 for the second half
  b.half = b.share;
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
  b.half = false;
  T o2 = b.alloc(x.n, x.h, x.w, C);
  b.attn(o2, q2.p, C, kv.p, 2 * C, kv.p + C, 2 * C, N, H, Tq, c.context_len, TkS, TkS, d, b.share ? N / 2 : 0);
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
  Builder::CO a; a.act = 1;
  b.advance(te, b.gemm(te, b.wptr(ns + "time_embed.0.weight"), mc, emb, b.vptr(ns + "time_embed.0.bias"), a));
  // every consumer of emb applies SiLU first (emb_layers = SiLU -> Linear), so store SiLU(emb)
  b.advance(te, b.gemm(te, b.wptr(ns + "time_embed.2.weight"), emb, emb, b.vptr(ns + "time_embed.2.bias"), a));
  b.gemm(te, b.named_w(ns + "emb_all.weight"), emb, total, b.named_v(ns + "emb_all.bias"), Builder::CO(), out, total);
  b.release(te);
}

static std::vector<const Blk*> attn_blocks(const UPlan& p) {
  std::vector<const Blk*> v;
  for_each_block(p, [&](const Blk& b) { if (b.kind == B_ATTN) v.push_back(&b); });
  return v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// configure: plan the arena and build all programs
// ------------------------------------------------------------------------------------------------
namespace {

static int run(Engine* e, const Program& p, hipStream_t s, bool skip_zero_convs = false) {
  if (!skip_zero_convs) return run_program(p, s, &e->prof);
  for (auto& op : p) {       // the ControlNet program without its zero convs
    if (op.zero_conv) continue;
    if (int rc = e->prof.on ? e->prof.record(op, s) : op(s)) return rc;
  }
  return 0;
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
};
static const ProgId kCnProg0[CP_COUNT] = {P_HINT, P_CTX_CN, P_CN, P_CN_SH, P_TEMB_CN};
static Program& cn_prog(Engine* e, int j, CnProg k) { return j == 0 ? e->prog[kCnProg0[k]] : e->xprog[j - 1][k]; }

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
      case B_ATTN: y = build_attn(b, ns, blk, x, c.kv[net].at(ns + blk.name), out); break;
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
static void build_controlnet(BuildCtx& c, int j) {
  Builder& b = c.b; Engine* e = b.e;
  Splice sp;
  Program& p_cn = cn_prog(e, j, CP_CN);
  b.prog = &p_cn;
  const int net = 1 + j;
  const std::string ns = net_ns(net);
  // The block outputs stay allocated (cn_h): sdeo_apply_model / sdeo_ddim_step skip the zero convs here and let the UNet decoder apply
  // them with the skip connection as the residual operand (P_UNET_DEC_FUSED); sdeo_controlnet_forward runs them here (13 controls out).
  auto zero_conv = [&](const T& x, const std::string& name, int cout, const T* out) {
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
    } else if (i == 1) {
      hcur = build_shared_prefix(c, ns, e->cplan.in[i], hcur, net, sp);
    } else {
      hcur = run_blocks(c, ns, e->cplan.in[i], hcur, false, net, nullptr);
    }
    e->cn_h[j][i] = hcur;
    zero_conv(hcur, ns + "zero_convs." + std::to_string(i) + ".0", e->cplan.in_ch[i], &e->ctrl[i]);
  }
  T m = run_blocks(c, ns, e->cplan.mid, hcur, false, net, nullptr);
  e->cn_h[j][c.nctrl - 1] = m;
  zero_conv(m, ns + "middle_block_out.0", e->cplan.in_ch.back(), &e->ctrl[c.nctrl - 1]);
  splice(c, cn_prog(e, j, CP_CN_SH), p_cn, sp);
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
    for (int j = 0; j <= e->extra; ++j) {
      Builder::CO zo; zo.out = &view; zo.res = &view; zo.scale_host = &e->eff_scales[j][ci];
      b.conv(e->cn_h[j][ci], net_ns(1 + j) + "middle_block_out.0", view.c, 1, 1, 0, zo);
    }
  }
  --ci;
  for (size_t oi = 0; oi < e->uplan.out.size(); ++oi) {
    // second half of the concat buffer: hs.pop() (+ control.pop() unless only_mid_control)
    T skip = hs.back();
    hs.pop_back();
    const int c_h = cat.c - skip.c;
    if (mode == D_FUSED) {
      const T half = cat.view(c_h, skip.c);
      for (int j = 0; j <= e->extra; ++j) {
        Builder::CO zo; zo.out = &half; zo.res = j ? &half : &skip; zo.scale_host = &e->eff_scales[j][ci];
        b.conv(e->cn_h[j][ci], net_ns(1 + j) + "zero_convs." + std::to_string(ci) + ".0", skip.c, 1, 1, 0, zo);
      }
    } else {
      f16* yp = cat.p + c_h; const int ld = cat.ld, rows = cat.rows(), Cc = skip.c;
      const f16* ap = skip.p; const int lda = skip.ld;
      const f16* cp = mode == D_ADD ? e->ctrl[ci].p : nullptr; const int ldc = mode == D_ADD ? e->ctrl[ci].ld : 0;
      const float* sc = &e->scales[ci]; const int* om = &e->only_mid;
      b.push([=](hipStream_t s) { return add_scaled(yp, ld, ap, lda, (*om) ? nullptr : cp, ldc, *sc, rows, Cc, s); });
    }
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
  std::vector<ConvGemm> zc[kMaxControlNets];
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
    zc[j].push_back(p);
    zs[j].push_back(&e->eff_scales[j][ci]);
  };
  auto zero_conv = [&](int ci, const std::string& leaf, const T& out, const T& res) {
    for (int j = 0; j <= e->extra; ++j) zero_conv_net(j, ci, net_ns(1 + j) + leaf, out, j ? out : res);
  };
  int ci = c.nctrl - 1;
  zero_conv(ci--, "middle_block_out.0", view0, view0);
  for (size_t oi = 0; oi < stages; ++oi, --ci) {
    const T& skip = hs[nh - 1 - oi];
    zero_conv(ci, "zero_convs." + std::to_string(ci) + ".0", cats[oi].view(cats[oi].c - skip.c, skip.c), skip);
  }
  if (!b.dry)
    for (int j = 0; j <= e->extra; ++j) b.prog->push_back(conv_gemm_multi_op(zc[j], kZeroConvTile, zs[j]));
  for (T& skip : hs) b.release(skip);
  for (size_t oi = 0; oi < stages; ++oi) {
    const std::vector<Blk>& blocks = e->uplan.out[oi];
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

// One pass over every program of the handle, on fresh arenas and in a fixed order: the arena plan is a function of the order of alloc /
// release.  Out: the workspaces the launches need and what each lane's arena has to hold
static int build_all(Engine* e, bool dry, size_t* max_splitk, size_t* max_gn, size_t peaks[L_COUNT]) {
  Arena arenas[L_COUNT];
  for (int i = 0; i < L_COUNT; ++i) e->lanes[i].arena = &arenas[i];
  BuildCtx c{Builder{e, &e->lanes[L_MAIN], dry}, e->N, e->lh, e->lw, round8(e->cfg.context_len), (int)e->cplan.in.size() + 1};
  build_persistent(c);
  // small programs (their temporaries come and go: only after every persistent tensor has its place)
  build_latent_io(c);
  build_time_embeds(c);
  for (int net = 0; net < 2 + e->extra; ++net) build_context(c, net);
  for (int j = 0; j <= e->extra; ++j) build_hint(c, j);
  // the extra nets run on the side stream behind net 0; every net's block outputs stay allocated there until the decoder has run
  c.b.on_lane(&e->lanes[L_SIDE], [&] { for (int j = 0; j <= e->extra; ++j) build_controlnet(c, j); });
  build_control_io(c);
  for (int variant = 0; variant < 2; ++variant) build_unet(c, variant == 0);
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

template <typename Tp>
static int dev_alloc(Engine* e, Tp** p, size_t bytes) {
  void* v = nullptr;
  SDEO_HIP(hipMalloc(&v, bytes < 256 ? 256 : bytes));
  e->extra_allocs.push_back(v);
  e->device_bytes += bytes;
  *p = reinterpret_cast<Tp*>(v);
  return 0;
}

static bool configured(const Engine* e) { return e->lanes[L_MAIN].base != nullptr; }

static void free_configured(Engine* e) {
  for (void* v : e->extra_allocs) (void)hipFree(v);      // (the lanes' workspaces among them)
  e->extra_allocs.clear();
  for (Lane& l : e->lanes) {
    if (l.base) (void)hipFree(l.base);
    l = Lane();
  }
  for (Program& p : e->prog) p.clear();
  for (auto& px : e->xprog) for (Program& p : px) p.clear();
  for (int j = 0; j < kMaxControlNets - 1; ++j) {        // the hint caches are gone with the arenas, the scales return to 1
    for (float& v : e->extra_scales[j]) v = 1.0f;
  }
  for (bool& b : e->hint_set) b = false;                 // ... and so are the context K / V and the staged latent
  e->ctx_set = 0;
  e->x0_staged_for = nullptr;
  e->tab_count = e->fp8.mx_launches = 0;
  e->device_bytes = e->ws.slab_bytes + e->fp8.q8_bytes + e->fp8.mx_bytes + e->ws.lora_backup_bytes;      // what stays: the weights, their fp8 packs, the tensors saved under adapters
}

// control scales of the next forward (null: all 1) and what P_UNET_DEC_FUSED applies of them: with only_mid_control
// (`cldm/cldm.py:35-41`) the twelve skip controls are dropped, the middle one stays
static void set_scales(Engine* h, const float* host_scales, int only_mid) {
  const int mid = (int)h->cplan.in.size();
  h->only_mid = only_mid;
  for (int i = 0; i < kMaxControls; ++i) {
    h->scales[i] = host_scales ? host_scales[i] : 1.0f;
    h->eff_scales[0][i] = (only_mid && i != mid) ? 0.0f : h->scales[i];
    for (int j = 1; j <= h->extra; ++j) h->eff_scales[j][i] = (only_mid && i != mid) ? 0.0f : h->extra_scales[j - 1][i];
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C entry points
// ------------------------------------------------------------------------------------------------
static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

int sdeo_create(const sdeo_config* cfg, sdeo_handle* out) { return sdeo_create_ex(cfg, nullptr, out); }

int sdeo_create_ex(const sdeo_config* cfg, const sdeo_config_ext* ext, sdeo_handle* out) {
  SDEO_CHECK(cfg && out, "sdeo_create: null argument");
  SDEO_CHECK(!ext || ext->size == (int)sizeof(sdeo_config_ext), "sdeo_create_ex: sdeo_config_ext.size is %d, this library's struct has %d bytes",
             ext ? ext->size : 0, (int)sizeof(sdeo_config_ext));
  SDEO_CHECK(cfg->num_levels >= 1 && cfg->num_levels <= 8 && cfg->vae_num_levels >= 1 && cfg->vae_num_levels <= 8,
             "sdeo_create: bad level count");
  SDEO_CHECK(cfg->model_channels % 32 == 0 && cfg->vae_ch % 32 == 0, "sdeo_create: channels must be multiples of 32 (GroupNorm)");
  SDEO_CHECK(cfg->context_dim % 8 == 0, "sdeo_create: context_dim must be a multiple of 8");
  const int nhc = ext && ext->num_head_channels > 0 ? ext->num_head_channels : 0;
  if (!nhc) SDEO_CHECK((cfg->model_channels / cfg->num_heads) % 8 == 0, "sdeo_create: head dim must be a multiple of 8");
  std::unique_ptr<Engine> e(new Engine());
  e->cfg = *cfg;
  e->num_head_channels = nhc;
  e->use_linear = ext && ext->use_linear_in_transformer != 0;
  if (nhc) {
    // host-only checks, before any device call: Blk::heads = C / nhc must be exact, and the head dim one the attention launcher has
    const UPlan probe = make_uplan(*cfg, true, 0);
    int bad_c = 0;
    for_each_block(probe, [&](const Blk& b) { if (b.kind == B_ATTN && b.cin % nhc != 0 && !bad_c) bad_c = b.cin; });
    SDEO_CHECK(!bad_c, "sdeo_create_ex: num_head_channels %d does not divide the %d channels of an attention block", nhc, bad_c);
    if (!attention_kernel_name(1, 1, 1, 1, nhc, 0)) {
      const std::string why = sdeo_last_error();
      return fail("sdeo_create_ex: num_head_channels %d is not a head dim the attention kernels are built for (%s)", nhc, why.c_str());
    }
  }
  e->uplan = make_uplan(*cfg, true, nhc);
  e->cplan = make_uplan(*cfg, false, nhc);
  SDEO_CHECK(e->cplan.in.size() + 1 <= kMaxControls, "sdeo_create: more than %d control tensors", kMaxControls);
  e->hconvs = hint_convs(*cfg);
  if (const char* at = getenv("SDEO_AUTOTUNE")) e->autotune = atoi(at) != 0;
  if (const char* ov = getenv("SDEO_OVERLAP")) e->overlap = atoi(ov) != 0;
  SDEO_HIP(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
  SDEO_HIP(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  SDEO_HIP(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
  set_scales(e.get(), nullptr, 0);
  build_registry(e.get());
  if (int rc = e->ws.alloc("sdeo_create", /*zero_fill=*/true)) return rc;
  e->device_bytes = e->ws.slab_bytes;
  *out = e.release();
  return 0;
}

int sdeo_destroy(sdeo_handle h) {
  if (!h) return 0;
  free_configured(h);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  h->ws.destroy();
  if (h->fp8.q8slab) (void)hipFree(h->fp8.q8slab);
  if (h->fp8.mxslab) (void)hipFree(h->fp8.mxslab);
  delete h;
  return 0;
}

int sdeo_enable_vae_encoder(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_enable_vae_encoder: null handle");
  if (h->vae_encoder) return 0;
  for (const auto& w : h->ws.entries)
    SDEO_CHECK(!w.loaded, "sdeo_enable_vae_encoder: call it before the first sdeo_load_weight (%s is loaded)", w.name.c_str());
  SDEO_CHECK(!h->finalized && !configured(h), "sdeo_enable_vae_encoder: call it before sdeo_finalize_weights / sdeo_configure");
  SDEO_CHECK(h->cfg.vae_num_levels == 4, "sdeo_enable_vae_encoder: %d VAE levels downsample by %d, the 8h x 8w image boundary needs 8",
             h->cfg.vae_num_levels, 1 << (h->cfg.vae_num_levels - 1));
  SDEO_CHECK(h->cfg.vae_out_ch <= 8, "sdeo_enable_vae_encoder: %d image channels (at most 8)", h->cfg.vae_out_ch);
  reg_vae_encoder(h);
  // nothing is loaded yet: the larger slab starts from zeros like the first one
  if (int rc = h->ws.alloc("sdeo_enable_vae_encoder", /*zero_fill=*/true)) return rc;
  h->device_bytes = h->ws.slab_bytes;
  h->vae_encoder = true;
  return 0;
}

int sdeo_enable_extra_controlnets(sdeo_handle h, int count) {
  SDEO_CHECK(count >= 1 && count <= kMaxControlNets - 1, "sdeo_enable_extra_controlnets: count %d out of range (1..%d extra control networks)",
             count, kMaxControlNets - 1);
  SDEO_CHECK(h, "sdeo_enable_extra_controlnets: null handle");
  SDEO_CHECK(!h->extra, "sdeo_enable_extra_controlnets: already called (this handle has %d extra control networks)", h->extra);
  for (const auto& w : h->ws.entries)
    SDEO_CHECK(!w.loaded, "sdeo_enable_extra_controlnets: call it before the first sdeo_load_weight (%s is loaded)", w.name.c_str());
  SDEO_CHECK(!h->finalized && !configured(h), "sdeo_enable_extra_controlnets: call it before sdeo_finalize_weights / sdeo_configure");
  // behind everything registered so far: the offsets of the existing tensors do not move
  Registry r{h};
  for (int j = 1; j <= count; ++j) reg_controlnet(r, 1 + j);
  if (int rc = h->ws.alloc("sdeo_enable_extra_controlnets", /*zero_fill=*/true)) return rc;
  h->device_bytes = h->ws.slab_bytes;
  h->extra = count;
  return 0;
}

int sdeo_num_weights(sdeo_handle h) { return h ? (int)h->ws.entries.size() : 0; }

int sdeo_weight_info(sdeo_handle h, int i, const char** name, int64_t dims[4], int* ndim) {
  SDEO_CHECK(h && i >= 0 && i < (int)h->ws.entries.size(), "sdeo_weight_info: bad index");
  h->ws.info(i, name, dims, 4, 1, ndim);
  return 0;
}

int sdeo_load_weight(sdeo_handle h, const char* name, const float* host_data, const int64_t* dims, int ndim, int strict) {
  SDEO_CHECK(h && name && host_data && dims, "sdeo_load_weight: null argument");
  return h->ws.load("sdeo_load_weight", name, name, host_data, dims, ndim, strict);
}

static int derive_weights(sdeo_handle h);

int sdeo_finalize_weights(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_finalize_weights: null handle");
  SDEO_CHECK(!(h->extra && h->fp8.act_bits == 8),
             "sdeo_finalize_weights: block-scaled fp8 activations (sdeo_set_activation_precision 8) are not supported together with extra "
             "control networks (%d enabled)", h->extra);
  if (int rc = h->ws.require_all("sdeo_finalize_weights")) return rc;
  if (int rc = derive_weights(h)) return rc;
  h->finalized = true;
  return 0;
}

// Everything a handle derives from its raw tensors, on the null stream, synchronised: sdeo_finalize_weights runs it once, sdeo_lora_commit
// and sdeo_lora_clear again after the raw tensors changed.
static int derive_weights(sdeo_handle h) {
  // LayerNorm-folded copies of the Linear layers that consume a LayerNorm (rebuilt on every finalize, from the raw tensors)
  for (const FoldJob& f : h->folds) {
    auto vec = [&](const std::string& n) { return n.empty() ? nullptr : h->ws.ptr<float>(n); };
    if (int rc = fold_layernorm(reinterpret_cast<f16*>(h->ws.slab + f.w_out), reinterpret_cast<float*>(h->ws.slab + f.s_out),
                                reinterpret_cast<float*>(h->ws.slab + f.b_out), reinterpret_cast<const f16*>(h->ws.slab + f.w_in),
                                vec(f.gamma), vec(f.beta), vec(f.bias), f.rows, f.C, 0))
      return rc;
  }
  if (h->fp8.weight_bits == 8) {
    // fp8 pack: codes + per-row scales in a slab of their own; the fp16 copies become the dequantised values
    if (!h->fp8.q8slab) {
      size_t sz = 0;
      for (QRegion& q : h->fp8.qregions) {
        q.q_off = align_up(sz, 256); sz = q.q_off + (size_t)q.rows * q.cols;
        q.s_off = align_up(sz, 256); sz = q.s_off + (size_t)q.rows * 4;
      }
      h->fp8.q8_bytes = align_up(sz, 256);
      SDEO_HIP(hipMalloc((void**)&h->fp8.q8slab, h->fp8.q8_bytes));
      h->device_bytes += h->fp8.q8_bytes;
    }
    for (const QRegion& q : h->fp8.qregions)
      if (int rc = quantize_fp8_rows(reinterpret_cast<uint8_t*>(h->fp8.q8slab + q.q_off), reinterpret_cast<float*>(h->fp8.q8slab + q.s_off),
                                     reinterpret_cast<f16*>(h->ws.slab + q.off), q.rows, q.cols, q.cols, q.cols, 0))
        return rc;
    for (const FoldJob& f : h->folds)          // the row sums of the LayerNorm fold must be those of the re-quantised matrix
      if (int rc = row_sums_f16(reinterpret_cast<float*>(h->ws.slab + f.s_out), reinterpret_cast<const f16*>(h->ws.slab + f.w_out), f.rows, f.C, 0))
        return rc;
  }
  // ff.net.2 x proj_out products, from the values the fp16 copies hold NOW (the dequantised ones when weight_bits == 8)
  for (const ComposeJob& cj : h->composes) {
    if (int rc = compose_proj(reinterpret_cast<f16*>(h->ws.slab + cj.w_out), reinterpret_cast<float*>(h->ws.slab + cj.b_out),
                              h->ws.ptr<f16>(cj.wp), h->ws.ptr<float>(cj.bp), h->ws.ptr<f16>(cj.w2), h->ws.ptr<float>(cj.b2), cj.C, 4 * cj.C, 0))
      return rc;
  }
  if (h->fp8.act_bits == 8) {
    // block-scaled packs of every Linear / conv1x1 matrix whose K is a multiple of 128 (from the values the fp16 copies hold now,
    // i.e. after the per-row fp8 rounding when weight_bits == 8)
    if (!h->fp8.mxslab) {
      size_t sz = 0;
      for (const QRegion& q : h->fp8.qregions) {
        if (q.cols % 128) continue;
        Fp8State::MxRegion m{};
        m.rows = q.rows; m.cols = q.cols;
        m.q_off = align_up(sz, 256); sz = m.q_off + (size_t)q.rows * q.cols;
        m.s_off = align_up(sz, 256); sz = m.s_off + (size_t)q.rows * (q.cols / 32);
        h->fp8.mxindex[q.off] = m;
      }
      h->fp8.mx_bytes = align_up(sz, 256);
      SDEO_HIP(hipMalloc((void**)&h->fp8.mxslab, h->fp8.mx_bytes < 256 ? 256 : h->fp8.mx_bytes));
      h->device_bytes += h->fp8.mx_bytes;
    }
    for (auto& kv : h->fp8.mxindex)
      if (int rc = quantize_mx(reinterpret_cast<uint8_t*>(h->fp8.mxslab + kv.second.q_off), reinterpret_cast<uint8_t*>(h->fp8.mxslab + kv.second.s_off),
                               reinterpret_cast<const f16*>(h->ws.slab + kv.first), kv.second.rows, kv.second.cols, kv.second.cols, kv.second.cols,
                               kv.second.cols / 32, 0))
        return rc;
  }
  SDEO_HIP(hipDeviceSynchronize());
  return 0;
}

int sdeo_set_activation_precision(sdeo_handle h, int bits, int min_rows) {
  SDEO_CHECK(h, "sdeo_set_activation_precision: null handle");
  SDEO_CHECK(bits == 16 || bits == 8, "sdeo_set_activation_precision: %d bits unsupported (16 or 8)", bits);
  SDEO_CHECK(!h->finalized && !configured(h), "sdeo_set_activation_precision: call it before sdeo_finalize_weights / sdeo_configure");
  h->fp8.act_bits = bits;
  h->fp8.mx_min_rows = min_rows > 0 ? min_rows : 2048;
  return 0;
}
int sdeo_debug_mx_launches(sdeo_handle h) { return h ? h->fp8.mx_launches : -1; }

int sdeo_set_weight_precision(sdeo_handle h, int bits) {
  SDEO_CHECK(h, "sdeo_set_weight_precision: null handle");
  SDEO_CHECK(bits == 16 || bits == 8, "sdeo_set_weight_precision: %d bits unsupported (16 or 8)", bits);
  SDEO_CHECK(!h->finalized && !configured(h), "sdeo_set_weight_precision: call it before sdeo_finalize_weights / sdeo_configure");
  h->fp8.weight_bits = bits;
  return 0;
}

static int configure_impl(sdeo_handle h, int n, int latent_h, int latent_w) {
  free_configured(h);
  h->N = n; h->lh = latent_h; h->lw = latent_w;
  const sdeo_config& c = h->cfg;
  const size_t px = (size_t)latent_h * latent_w;
  // boundary buffers
  if (int rc = dev_alloc(h, &h->in_x, (size_t)n * c.in_channels * px * 4)) return rc;
  for (int j = 0; j <= h->extra; ++j)
    if (int rc = dev_alloc(h, &h->in_hint[j], (size_t)n * c.hint_channels * px * 64 * 4)) return rc;
  if (int rc = dev_alloc(h, &h->in_ctx, (size_t)n * c.context_len * c.context_dim * 4)) return rc;
  if (int rc = dev_alloc(h, &h->in_t, (size_t)n * 8)) return rc;
  if (int rc = dev_alloc(h, &h->tab_t, (size_t)sdeo_handle_s::kTabRows * 8)) return rc;
  SDEO_HIP(hipMemset(h->tab_t, 0, (size_t)sdeo_handle_s::kTabRows * 8));
  for (int net = 0; net < 2 + h->extra; ++net) {
    if (int rc = dev_alloc(h, &h->emb_all[net], (size_t)n * h->emb_total[net] * 4)) return rc;
    if (int rc = dev_alloc(h, &h->temb_tab[net], (size_t)sdeo_handle_s::kTabRows * h->emb_total[net] * 4)) return rc;
  }
  if (int rc = dev_alloc(h, &h->out_eps, (size_t)n * c.out_channels * px * 4)) return rc;
  if (int rc = dev_alloc(h, &h->vae_in, (size_t)c.vae_z_channels * px * 4)) return rc;
  if (int rc = dev_alloc(h, &h->vae_out, (size_t)c.vae_out_ch * px * 64 * 4)) return rc;
  if (int rc = dev_alloc(h, &h->vae_u8, (size_t)c.vae_out_ch * px * 64)) return rc;
  if (h->vae_encoder) {
    if (int rc = dev_alloc(h, &h->enc_img, (size_t)c.vae_out_ch * px * 64 * 4)) return rc;
    if (int rc = dev_alloc(h, &h->enc_img_u8, (size_t)c.vae_out_ch * px * 64)) return rc;
    if (int rc = dev_alloc(h, &h->enc_noise, (size_t)c.vae_z_channels * px * 4)) return rc;
    if (int rc = dev_alloc(h, &h->enc_z, (size_t)c.vae_z_channels * px * 4)) return rc;
    if (int rc = dev_alloc(h, &h->enc_moments, (size_t)2 * c.vae_z_channels * px * 4)) return rc;
  }
  const int nctrl = (int)h->cplan.in.size() + 1;
  for (int i = 0; i < nctrl; ++i) {
    const int idx = i < (int)h->cplan.in.size() ? i : (int)h->cplan.in.size() - 1;
    const int ds = h->cplan.in_ds[idx];
    const size_t elems = (size_t)n * h->cplan.in_ch[idx] * (latent_h / ds) * (latent_w / ds);
    if (int rc = dev_alloc(h, &h->in_ctrl[i], elems * 4)) return rc;
    if (int rc = dev_alloc(h, &h->out_ctrl[i], elems * 4)) return rc;
  }
  // pass 1: plan the arenas (no launches recorded), pass 2: build for real
  size_t ms = 0, mg = 0, peaks[L_COUNT];
  if (int rc = build_all(h, true, &ms, &mg, peaks)) return rc;
  for (int i = 0; i < L_COUNT; ++i) {
    Lane& l = h->lanes[i];
    l.bytes = peaks[i];
    SDEO_HIP(hipMalloc((void**)&l.base, l.bytes));
    SDEO_HIP(hipMemset(l.base, 0, l.bytes));
    h->device_bytes += l.bytes;
    if (int rc = dev_alloc(h, &l.splitk_ws, l.splitk_ws_bytes = ms)) return rc;
    if (int rc = dev_alloc(h, &l.gn_ws, mg)) return rc;
  }
  if (int rc = build_all(h, false, &ms, &mg, peaks)) return rc;
  SDEO_CHECK(peaks[L_MAIN] == h->lanes[L_MAIN].bytes && peaks[L_SIDE] == h->lanes[L_SIDE].bytes, "sdeo_configure: arena plan not reproducible");
  SDEO_HIP(hipDeviceSynchronize());      // autotune launches are done before the first real forward
  return 0;
}

// A configure that fails part-way leaves the handle unconfigured (never half-built programs); one whose arguments are rejected leaves
// the previous configuration in place
int sdeo_configure(sdeo_handle h, int n, int latent_h, int latent_w) {
  SDEO_CHECK(h, "sdeo_configure: null handle");
  SDEO_CHECK(n >= 1 && n <= 64, "sdeo_configure: n=%d out of range", n);
  const int maxds = 1 << (h->cfg.num_levels - 1);
  SDEO_CHECK(latent_h >= maxds && latent_w >= maxds && latent_h % maxds == 0 && latent_w % maxds == 0,
             "sdeo_configure: latent %dx%d must be a positive multiple of %d", latent_h, latent_w, maxds);
  SDEO_CHECK(h->fp8.weight_bits != 8 || h->fp8.q8slab, "sdeo_configure: fp8 weights are packed by sdeo_finalize_weights: call it first");
  const int rc = configure_impl(h, n, latent_h, latent_w);
  if (rc) free_configured(h);
  return rc;
}

static int copy_in(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (dst == src) return 0;
  SDEO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  return 0;
}

static int stage_inputs(sdeo_handle h, const float* x, const float* hint, const int64_t* t, const float* ctx, int hint_is_new,
                        int ctx_for_net, hipStream_t s) {
  const sdeo_config& c = h->cfg;
  const size_t px = (size_t)h->lh * h->lw;
  if (x) if (int rc = copy_in(h->in_x, x, (size_t)h->N * c.in_channels * px * 4, s)) return rc;
  if (t) if (int rc = copy_in(h->in_t, t, (size_t)h->N * 8, s)) return rc;
  if (hint && hint_is_new) {
    if (int rc = copy_in(h->in_hint[0], hint, (size_t)h->N * c.hint_channels * px * 64 * 4, s)) return rc;
    if (int rc = run(h, h->prog[P_HINT], s)) return rc;
    h->hint_stale[0] = false;
    h->hint_set[0] = true;
  }
  if (ctx) {
    h->ctx_set &= ~ctx_for_net;                   // (a failed launch leaves the side unset, not half written and trusted)
    ++h->ctx_epoch;
    if (int rc = copy_in(h->in_ctx, ctx, (size_t)h->N * c.context_len * c.context_dim * 4, s)) return rc;
    if (ctx_for_net & 1) if (int rc = run(h, h->prog[P_CTX_UNET], s)) return rc;
    if (ctx_for_net & 2)
      for (int j = 0; j <= h->extra; ++j) if (int rc = run(h, cn_prog(h, j, CP_CTX), s)) return rc;
    h->ctx_stale &= ~ctx_for_net;
    h->ctx_set |= ctx_for_net;
    for (int side = 0; side < 2; ++side) if (ctx_for_net >> side & 1) h->ctx_epoch_of[side] = h->ctx_epoch;
  }
  return 0;
}

// P_X0: the fp16 copy of in_x.  Whatever a fused step staged in x0 is gone.
static int run_x0(sdeo_handle h, hipStream_t s) {
  h->x0_staged_for = nullptr;
  return run(h, h->prog[P_X0], s);
}

// A call that asks for a cache sdeo_lora_commit made stale, or one nothing filled since the last sdeo_configure, is refused (before any
// device call), each cache with its own message; so is a call that reads the context K / V of both sides when the two were computed
// from different contexts.
// hint_net: the control network whose SDEO_HINT_CACHED features the call reads (-1: none); ctx_nets: whose context K / V it reads from
// the cache (bit 0 the UNet, bit 1 the control networks; 0: none)
static int caches_fresh(sdeo_handle h, const char* who, int hint_net, int ctx_nets) {
  SDEO_CHECK(hint_net < 0 || !h->hint_stale[hint_net],
             "%s: SDEO_HINT_CACHED, but sdeo_lora_commit changed the weights the cached hint features of control network %d were computed "
             "with (pass the hint again)", who, hint_net);
  SDEO_CHECK(!(h->ctx_stale & ctx_nets),
             "%s: SDEO_CONTEXT_CACHED, but sdeo_lora_commit changed the weights the cached context K / V were computed with (pass the "
             "context again)", who);
  SDEO_CHECK(hint_net < 0 || h->hint_set[hint_net],
             "%s: SDEO_HINT_CACHED, but control network %d has no hint since the last sdeo_configure (%s)", who, hint_net,
             hint_net == 0 ? "pass the hint to sdeo_apply_model or sdeo_controlnet_forward" : "call sdeo_set_control_hint");
  SDEO_CHECK(!(ctx_nets & 1 & ~h->ctx_set),
             "%s: SDEO_CONTEXT_CACHED, but the UNet has no context K / V since the last sdeo_configure (pass the context to "
             "sdeo_apply_model or sdeo_unet_forward)", who);
  SDEO_CHECK(!(ctx_nets & 2 & ~h->ctx_set),
             "%s: SDEO_CONTEXT_CACHED, but the control networks have no context K / V since the last sdeo_configure (pass the context to "
             "sdeo_apply_model or sdeo_controlnet_forward)", who);
  SDEO_CHECK(ctx_nets != 3 || h->ctx_epoch_of[0] == h->ctx_epoch_of[1],
             "%s: SDEO_CONTEXT_CACHED, but the cached context K / V of the UNet and of the control networks were computed from different "
             "contexts (a call that refreshes one side only ran since: sdeo_unet_forward, sdeo_controlnet_forward or SDEO_NO_CONTROL; pass "
             "the context to sdeo_apply_model again)", who);
  return 0;
}

#define REQUIRE_READY(h)                                                                     \
  SDEO_CHECK(h, "null handle");                                                              \
  SDEO_CHECK(h->finalized, "weights not finalized (call sdeo_finalize_weights)");            \
  SDEO_CHECK(configured(h), "not configured (call sdeo_configure)")

// time embedding of this forward: row `row` of the schedule table (>= 0; every image of the batch at that timestep), or in_t via P_TEMB + net
static int select_time(sdeo_handle h, int flags, const int64_t* timesteps, const char* who, int* row_out) {
  const int row = (flags & 8) ? (flags >> 8) : -1;
  SDEO_CHECK(row >= 0 || timesteps, "%s: timesteps required", who);
  SDEO_CHECK(row < h->tab_count, "%s: timestep row %d, but the table holds %d (sdeo_set_timestep_table)", who, row, h->tab_count);
  SDEO_CHECK(row < 0 || !h->tab_stale, "%s: SDEO_TIMESTEP_ROW, but sdeo_lora_commit changed the weights the timestep table was computed with "
             "(call sdeo_set_timestep_table again)", who);
  for (int net = 0; net < 2 + h->extra; ++net) {
    h->emb_cur[net] = row >= 0 ? h->temb_tab[net] + (size_t)row * h->emb_total[net] : h->emb_all[net];
    h->emb_ld_cur[net] = row >= 0 ? 0 : h->emb_total[net];
  }
  *row_out = row;
  return 0;
}

// The time embeddings of the extra control networks.  They run in FRONT of net 0's ControlNet: their temporaries were planned on the
// empty side arena, where net 0's block outputs (kept until the decoder has run) live afterwards.
static int run_extra_time_embeds(sdeo_handle h, hipStream_t s) {
  for (int j = 1; j <= h->extra; ++j) if (int rc = run(h, cn_prog(h, j, CP_TEMB), s)) return rc;
  return 0;
}

// the extra control networks, one behind the other on the stream net 0's ControlNet ran on, without their zero convs
static int run_extra_controlnets(sdeo_handle h, bool shared_cn, hipStream_t s) {
  for (int j = 1; j <= h->extra; ++j) {
    const Program& sh = cn_prog(h, j, CP_CN_SH);
    if (int rc = run(h, shared_cn && !sh.empty() ? sh : cn_prog(h, j, CP_CN), s, true)) return rc;
  }
  return 0;
}

// a forward that runs the control networks needs every extra net's hint cache filled (sdeo_set_control_hint)
static int extra_hints_ready(sdeo_handle h, const char* who) {
  for (int j = 1; j <= h->extra; ++j)
    SDEO_CHECK(h->hint_set[j], "%s: control network %d has no hint since the last sdeo_configure (call sdeo_set_control_hint(h, %d, ...))",
               who, j, j);
  for (int j = 1; j <= h->extra; ++j)
    SDEO_CHECK(!h->hint_stale[j], "%s: sdeo_lora_commit changed the weights the cached hint features of control network %d were computed with "
               "(call sdeo_set_control_hint(h, %d, ...) again)", who, j, j);
  return 0;
}

// ControlNet || UNet encoder, join, UNet decoder: eps16 holds the result.  The latent is already in x0.
// shared_unet / shared_cn: the two halves of the batch are the same images at the same timestep (and, for the ControlNet, under the same
// hint): run the programs whose shared prefix is computed once, where configure built them
static int run_step_programs(sdeo_handle h, bool no_control, bool time_from_table, hipStream_t s, bool shared_unet = false,
                             bool shared_cn = false) {
  const Program& p_unet_enc = shared_unet && !h->prog[P_UNET_ENC_SH].empty() ? h->prog[P_UNET_ENC_SH] : h->prog[P_UNET_ENC];
  const Program& p_cn = shared_cn && !h->prog[P_CN_SH].empty() ? h->prog[P_CN_SH] : h->prog[P_CN];
  if (no_control) {
    if (!time_from_table) if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
    return run(h, h->prog[P_UNET_NOCTRL], s);
  }
  if (h->overlap && !h->prof.on) {
    // fork: ControlNet on the side stream, UNet encoder + middle block on the caller's stream (capturable)
    SDEO_HIP(hipEventRecord(h->ev_fork, s));
    SDEO_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    if (!time_from_table) {
      if (int rc = run(h, h->prog[P_TEMB + 1], h->side)) return rc;
      if (int rc = run_extra_time_embeds(h, h->side)) return rc;
    }
    if (int rc = run(h, p_cn, h->side, true)) return rc;
    if (int rc = run_extra_controlnets(h, shared_cn, h->side)) return rc;
    SDEO_HIP(hipEventRecord(h->ev_join, h->side));
    if (!time_from_table) if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
    if (int rc = run(h, p_unet_enc, s)) return rc;
    SDEO_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
  } else {
    if (!time_from_table) {
      if (int rc = run(h, h->prog[P_TEMB + 1], s)) return rc;
      if (int rc = run_extra_time_embeds(h, s)) return rc;
      if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
    }
    if (int rc = run(h, p_cn, s, true)) return rc;
    if (int rc = run_extra_controlnets(h, shared_cn, s)) return rc;
    if (int rc = run(h, p_unet_enc, s)) return rc;
  }
  return run(h, h->prog[P_UNET_DEC_FUSED], s);      // applies the zero convs itself (skipped above)
}

// copy net j's hint in and run its hint block into its cached features (j >= 1; net 0's goes through stage_inputs)
static int set_extra_hint(sdeo_handle h, int j, const float* hint, hipStream_t s) {
  const size_t bytes = (size_t)h->N * h->cfg.hint_channels * h->lh * h->lw * 64 * 4;
  if (int rc = copy_in(h->in_hint[j], hint, bytes, s)) return rc;
  if (int rc = run(h, cn_prog(h, j, CP_HINT), s)) return rc;
  h->hint_set[j] = true;
  h->hint_stale[j] = false;
  return 0;
}

static int controlnet_forward_impl(sdeo_handle h, int j, const float* x_noisy, const float* hint, const int64_t* timesteps,
                                   const float* context, float* const* controls, int flags, const char* who, hipStream_t s) {
  SDEO_CHECK(x_noisy && controls, "%s: null argument", who);
  const int hint_new = !(flags & 1), ctx_new = !(flags & 2);
  SDEO_CHECK(!hint_new || hint, "%s: hint required", who);
  SDEO_CHECK(!ctx_new || context, "%s: context required", who);
  SDEO_CHECK(j == 0 || hint_new || h->hint_set[j], "%s: control network %d has no hint since the last sdeo_configure", who, j);
  if (int rc = caches_fresh(h, who, hint_new ? -1 : j, ctx_new ? 0 : 2)) return rc;
  int trow = -1;
  if (int rc = select_time(h, flags, timesteps, who, &trow)) return rc;
  if (int rc = stage_inputs(h, x_noisy, j == 0 ? hint : nullptr, trow < 0 ? timesteps : nullptr, ctx_new ? context : nullptr, hint_new, 2, s)) return rc;
  if (j > 0 && hint_new) if (int rc = set_extra_hint(h, j, hint, s)) return rc;
  if (int rc = run_x0(h, s)) return rc;
  if (trow < 0) if (int rc = run(h, cn_prog(h, j, CP_TEMB), s)) return rc;
  if (int rc = run(h, cn_prog(h, j, CP_CN), s)) return rc;
  if (int rc = run(h, h->prog[P_CN_EXPORT], s)) return rc;
  for (size_t i = 0; i < h->ctrl_elems.size(); ++i)
    if (controls[i]) if (int rc = copy_in(controls[i], h->out_ctrl[i], h->ctrl_elems[i] * 4, s)) return rc;
  return 0;
}

int sdeo_controlnet_forward(sdeo_handle h, const float* x_noisy, const float* hint, const int64_t* timesteps,
                            const float* context, float* const* controls, int flags, void* stream) {
  REQUIRE_READY(h);
  return controlnet_forward_impl(h, 0, x_noisy, hint, timesteps, context, controls, flags, "sdeo_controlnet_forward", S(stream));
}

int sdeo_controlnet_forward_net(sdeo_handle h, int net, const float* x_noisy, const float* hint, const int64_t* timesteps,
                                const float* context, float* const* controls, int flags, void* stream) {
  SDEO_CHECK(h, "sdeo_controlnet_forward_net: null handle");
  SDEO_CHECK(net >= 0 && net <= h->extra, "sdeo_controlnet_forward_net: net %d out of range (0..%d)", net, h->extra);
  REQUIRE_READY(h);
  return controlnet_forward_impl(h, net, x_noisy, hint, timesteps, context, controls, flags,
                                 net ? "sdeo_controlnet_forward_net" : "sdeo_controlnet_forward", S(stream));
}

// what the two setters of an extra net's state check first
static int extra_net_ok(sdeo_handle h, int net, const char* who) {
  SDEO_CHECK(h, "%s: null handle", who);
  SDEO_CHECK(h->extra > 0, "%s: this handle has no extra control networks (call sdeo_enable_extra_controlnets before loading weights)", who);
  SDEO_CHECK(net >= 1 && net <= h->extra, "%s: net %d out of range (1..%d)", who, net, h->extra);
  SDEO_CHECK(configured(h), "%s: not configured (call sdeo_configure)", who);
  return 0;
}

int sdeo_set_control_hint(sdeo_handle h, int net, const float* hint, void* stream) {
  if (int rc = extra_net_ok(h, net, "sdeo_set_control_hint")) return rc;
  SDEO_CHECK(h->finalized, "sdeo_set_control_hint: weights not finalized (call sdeo_finalize_weights)");
  SDEO_CHECK(hint, "sdeo_set_control_hint: null hint");
  return set_extra_hint(h, net, hint, S(stream));
}

int sdeo_set_control_scales(sdeo_handle h, int net, const float* host_scales13) {
  if (int rc = extra_net_ok(h, net, "sdeo_set_control_scales")) return rc;
  for (int i = 0; i < kMaxControls; ++i) h->extra_scales[net - 1][i] = host_scales13 ? host_scales13[i] : 1.0f;
  return 0;
}

int sdeo_unet_forward(sdeo_handle h, const float* x_noisy, const int64_t* timesteps, const float* context,
                      const float* const* controls, const float* host_control_scales, int only_mid_control, float* eps,
                      int flags, void* stream) {
  REQUIRE_READY(h);
  SDEO_CHECK(x_noisy && eps, "sdeo_unet_forward: null argument");
  hipStream_t s = S(stream);
  const int ctx_new = !(flags & 2);
  SDEO_CHECK(!ctx_new || context, "sdeo_unet_forward: context required");
  if (int rc = caches_fresh(h, "sdeo_unet_forward", -1, ctx_new ? 0 : 1)) return rc;
  int trow = -1;
  if (int rc = select_time(h, flags, timesteps, "sdeo_unet_forward", &trow)) return rc;
  if (int rc = stage_inputs(h, x_noisy, nullptr, trow < 0 ? timesteps : nullptr, ctx_new ? context : nullptr, 0, 1, s)) return rc;
  set_scales(h, host_control_scales, only_mid_control);
  if (int rc = run_x0(h, s)) return rc;
  if (trow < 0) if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
  if (controls) {
    for (size_t i = 0; i < h->ctrl_elems.size(); ++i) {
      SDEO_CHECK(controls[i], "sdeo_unet_forward: control %zu is null", i);
      if (int rc = copy_in(h->in_ctrl[i], controls[i], h->ctrl_elems[i] * 4, s)) return rc;
    }
    if (int rc = run(h, h->prog[P_CTRL_IMPORT], s)) return rc;
    if (int rc = run(h, h->prog[P_UNET_ENC], s)) return rc;
    if (int rc = run(h, h->prog[P_UNET_DEC], s)) return rc;
  } else {
    if (int rc = run(h, h->prog[P_UNET_NOCTRL], s)) return rc;
  }
  if (int rc = run(h, h->prog[P_EPS_EXPORT], s)) return rc;
  return copy_in(eps, h->out_eps, (size_t)h->N * h->cfg.out_channels * h->lh * h->lw * 4, s);
}

int sdeo_apply_model(sdeo_handle h, const float* x_noisy, const float* hint, const int64_t* timesteps, const float* context,
                     const float* host_control_scales, int only_mid_control, int flags, float* eps, void* stream) {
  REQUIRE_READY(h);
  SDEO_CHECK(x_noisy && eps, "sdeo_apply_model: null argument");
  hipStream_t s = S(stream);
  const int hint_new = !(flags & 1), ctx_new = !(flags & 2), no_control = (flags & 4) != 0;
  SDEO_CHECK(!ctx_new || context, "sdeo_apply_model: context required");
  SDEO_CHECK(no_control || !hint_new || hint, "sdeo_apply_model: hint required");
  if (!no_control) if (int rc = extra_hints_ready(h, "sdeo_apply_model")) return rc;
  if (int rc = caches_fresh(h, "sdeo_apply_model", no_control || hint_new ? -1 : 0, ctx_new ? 0 : no_control ? 1 : 3)) return rc;
  int trow = -1;
  if (int rc = select_time(h, flags, timesteps, "sdeo_apply_model", &trow)) return rc;
  if (int rc = stage_inputs(h, x_noisy, no_control ? nullptr : hint, trow < 0 ? timesteps : nullptr, ctx_new ? context : nullptr, hint_new,
                            no_control ? 1 : 3, s))
    return rc;
  set_scales(h, host_control_scales, only_mid_control);
  if (int rc = run_x0(h, s)) return rc;
  if (int rc = run_step_programs(h, no_control, trow >= 0, s)) return rc;
  if (int rc = run(h, h->prog[P_EPS_EXPORT], s)) return rc;
  return copy_in(eps, h->out_eps, (size_t)h->N * h->cfg.out_channels * h->lh * h->lw * 4, s);
}

int sdeo_set_timestep_table(sdeo_handle h, const int64_t* host_timesteps, int count, void* stream) {
  REQUIRE_READY(h);
  SDEO_CHECK(host_timesteps && count >= 1 && count <= sdeo_handle_s::kTabRows, "sdeo_set_timestep_table: 1..%d timesteps (got %d)",
             sdeo_handle_s::kTabRows, count);
  hipStream_t s = S(stream);
  int64_t padded[sdeo_handle_s::kTabRows] = {0};
  for (int i = 0; i < count; ++i) padded[i] = host_timesteps[i];
  h->tab_count = 0;
  SDEO_HIP(hipMemcpyAsync(h->tab_t, padded, sizeof(padded), hipMemcpyHostToDevice, s));
  SDEO_HIP(hipStreamSynchronize(s));          // `padded` is a stack array; this call is made once per schedule, outside any capture
  if (int rc = run(h, h->prog[P_TEMB_TAB], s)) return rc;
  h->tab_count = count;
  h->tab_stale = false;
  return 0;
}

// The mask / x0 blend a masked step puts in front of its forward (mask_blend_pair); null for an unmasked step.
struct StepBlend {
  const float* orig; const float* noise; const float* mask;
  int mask_n, mask_c;
  float sqrt_a, sqrt_1ma;
};

// What every fused CFG-pair step does before its update kernel: the checks, the time-embedding row, the control scales, the fp16 copy of
// [x; x] unless the previous step staged it, and the networks.  Leaves the model output in h->eps16.  With a blend, x is first replaced
// by the blended latent, in the launch that stages its fp16 copy.  Every check precedes the first device call.
// SDEO_STEP_UNGUIDED: the un-paired member.  x holds the configured N latents (any N >= 1), each is staged and run once, and the programs
// are the plain ones: no two images of the batch are the same, so no shared prefix holds.
static int cfg_pair_forward(sdeo_handle h, float* x, int table_row, const float* host_control_scales, int only_mid_control, int flags,
                            const StepBlend* blend, const char* who, hipStream_t s) {
  REQUIRE_READY(h);
  SDEO_CHECK(x, "%s: null latent", who);
  SDEO_CHECK(h->cfg.in_channels == h->cfg.out_channels, "%s: eps and latent must have the same channel count", who);
  const bool paired = !(flags & SDEO_STEP_UNGUIDED);
  const int b = paired ? h->N / 2 : h->N;         // latents in x
  SDEO_CHECK(!paired || h->N % 2 == 0, "%s: configured for %d images; the CFG pair needs an even count (n = 2 x latents)", who, h->N);
  SDEO_CHECK(paired || !(flags & SDEO_STEP_HINT_SHARED), "%s: SDEO_STEP_HINT_SHARED together with SDEO_STEP_UNGUIDED (an unguided step has no "
             "second half whose hints could be those of the first)", who);
  SDEO_CHECK(table_row >= 0 && table_row < h->tab_count, "%s: timestep row %d, but the table holds %d (sdeo_set_timestep_table)", who,
             table_row, h->tab_count);
  SDEO_CHECK(!h->tab_stale, "%s: sdeo_lora_commit changed the weights the timestep table was computed with (call sdeo_set_timestep_table again)", who);
  if (int rc = extra_hints_ready(h, who)) return rc;
  if (int rc = caches_fresh(h, who, 0, 3)) return rc;
  if (!blend && (flags & SDEO_STEP_LATENT_STAGED)) {
    SDEO_CHECK(h->x0_staged_for, "%s: SDEO_STEP_LATENT_STAGED, but no fused step staged a latent since the last sdeo_configure, or another "
               "forward (sdeo_apply_model, sdeo_unet_forward, sdeo_controlnet_forward) overwrote it since (drop the flag)", who);
    SDEO_CHECK(h->x0_staged_for == x, "%s: SDEO_STEP_LATENT_STAGED, but the previous fused step ran on another latent (%p; this one is %p; "
               "drop the flag)", who, (const void*)h->x0_staged_for, (const void*)x);
    SDEO_CHECK(h->x0_staged_paired == paired, "%s: SDEO_STEP_LATENT_STAGED, but the previous fused step was %s and staged its latent as such "
               "(drop the flag)", who, h->x0_staged_paired ? "a CFG-pair step" : "an unguided step (SDEO_STEP_UNGUIDED)");
  }
  if (blend) {
    SDEO_CHECK(!(flags & SDEO_STEP_LATENT_STAGED), "%s: SDEO_STEP_LATENT_STAGED has no meaning here (the blend changes the latent and always restages it)", who);
    if (int rc = mask_blend_check(who, x, blend->orig, blend->noise, blend->mask, blend->mask_n, blend->mask_c, b, h->cfg.in_channels,
                                  h->lh * h->lw))
      return rc;
  }
  int trow = -1;
  if (int rc = select_time(h, 8 | (table_row << 8), nullptr, who, &trow)) return rc;
  set_scales(h, host_control_scales, only_mid_control);
  h->x0_staged_for = nullptr;                     // until the update kernel has left the new latent in x0 (fused_step)
  if (blend) {
    if (int rc = mask_blend_pair(x, blend->orig, blend->noise, blend->mask, blend->mask_n, blend->mask_c, blend->sqrt_a, blend->sqrt_1ma,
                                 h->x0.p, h->x0.ld, b, h->cfg.in_channels, h->lh * h->lw, paired, s))
      return rc;
  } else if (!(flags & SDEO_STEP_LATENT_STAGED)) {
    if (int rc = latent_pair_to_nhwc(h->x0.p, h->x0.ld, x, b, h->cfg.in_channels, h->lh * h->lw, paired, s)) return rc;
  }
  // x0 = [x; x] at one timestep: the UNet's shared prefix always holds, the ControlNet's when the caller vouches for the hints
  return run_step_programs(h, false, true, s, paired, paired && (flags & SDEO_STEP_HINT_SHARED) != 0);
}

// One fused CFG-pair step as its entry point describes it: which update, its coefficients, the optional noise term and the optional blend.
struct Step {
  const char* who;                  // the entry point
  const char* coef_who;             // who refuses a coefficient: the entry point; for the two plain steps the update's launcher, as ever
  bool multistep = false;           // x_next = k_x x + k_d D + k_p D_prev (+ k_n noise); else the DDIM update
  bool stochastic = false;          // an _eta / _sde entry point: cfg_scale and the noise term are checked too, the blend is optional
  float* aux = nullptr;             // pred_x0 of the DDIM update, d of the multistep update
  float cfg_scale = 0.f, a_t = 0.f, sqrt_one_minus_at = 0.f;
  float a_prev = 0.f;               // DDIM
  float k_x = 0.f, k_d = 0.f, k_p = 0.f;   // multistep
  const float* noise = nullptr;     // the noise term and its coefficient: sigma_t of the DDIM step, k_n of the SDE solver's
  float noise_coef = 0.f;
  bool blended = false;             // the mask / x0 blend in front of the forward
  StepBlend blend{};
};

// a stochastic step takes the blend's operands all or none
static int step_blend_operands(const char* who, const StepBlend& b, int flags) {
  if (!b.orig) {
    SDEO_CHECK(!b.noise && !b.mask, "%s: partial blend operands: orig is null, so mask_noise and mask must be null too (the unmasked step)", who);
    return 0;
  }
  SDEO_CHECK(b.noise && b.mask, "%s: partial blend operands: orig is given, so mask_noise and mask are needed too", who);
  SDEO_CHECK(!(flags & SDEO_STEP_LATENT_STAGED), "%s: SDEO_STEP_LATENT_STAGED together with a mask (the blend changes the latent and always restages it)", who);
  return 0;
}

// Every fused step: what the update kernel would refuse after the networks ran is refused here, up front, with what cfg_pair_forward
// checks before its first launch; then the forward, the update, and the record that x's fp16 copy is staged for the next step on x
// (the next step may then pass SDEO_STEP_LATENT_STAGED).  A refused step has launched nothing and leaves that record alone.
static int fused_step(sdeo_handle h, float* x, const Step& st, int table_row, const float* host_control_scales, int only_mid_control,
                      int flags, hipStream_t s) {
  const bool paired = !(flags & SDEO_STEP_UNGUIDED);
  const float cfg_scale = paired ? st.cfg_scale : 0.f;        // an unguided step neither reads nor checks it
  if (st.stochastic && st.multistep)
    SDEO_CHECK(std::isfinite(cfg_scale) && std::isfinite(st.a_t) && std::isfinite(st.sqrt_one_minus_at),
               "%s: non-finite coefficient cfg_scale=%g a_t=%g sqrt_one_minus_at=%g", st.who, st.cfg_scale, st.a_t, st.sqrt_one_minus_at);
  else if (st.stochastic)
    SDEO_CHECK(std::isfinite(cfg_scale) && std::isfinite(st.sqrt_one_minus_at), "%s: non-finite coefficient cfg_scale=%g sqrt_one_minus_at=%g",
               st.who, st.cfg_scale, st.sqrt_one_minus_at);
  if (int rc = st.multistep ? cfg_lms_check(st.coef_who, st.aux, st.noise, st.a_t, st.k_x, st.k_d, st.k_p, st.noise_coef)
                            : cfg_ddim_check(st.coef_who, st.a_t, st.a_prev, st.noise, st.stochastic ? &st.noise_coef : nullptr))
    return rc;
  if (st.stochastic) if (int rc = step_blend_operands(st.who, st.blend, flags)) return rc;
  if (int rc = cfg_pair_forward(h, x, table_row, host_control_scales, only_mid_control, flags, st.blended ? &st.blend : nullptr, st.who, s))
    return rc;
  const bool v_prediction = (flags & SDEO_STEP_V_PREDICTION) != 0;
  const int b = paired ? h->N / 2 : h->N, C = h->cfg.out_channels, HW = h->lh * h->lw;
  const int rc = st.multistep ? cfg_lms_pair(x, st.aux, h->eps16.p, h->eps16.ld, st.noise, st.noise_coef, h->x0.p, h->x0.ld, b, C, HW, cfg_scale,
                                             st.a_t, st.sqrt_one_minus_at, st.k_x, st.k_d, st.k_p, v_prediction, paired, s)
                              : cfg_ddim_pair(x, st.aux, h->eps16.p, h->eps16.ld, st.noise, st.noise_coef, h->x0.p, h->x0.ld, b, C, HW, cfg_scale,
                                              st.a_t, st.a_prev, st.sqrt_one_minus_at, v_prediction, paired, s);
  if (!rc) h->x0_staged_for = x, h->x0_staged_paired = paired;
  return rc;
}

static Step ddim_update(const char* who, float* pred_x0, float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at) {
  Step st{who, who};
  st.aux = pred_x0, st.cfg_scale = cfg_scale, st.a_t = a_t, st.a_prev = a_prev, st.sqrt_one_minus_at = sqrt_one_minus_at;
  return st;
}

static Step multistep_update(const char* who, float* d, float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p) {
  Step st{who, who};
  st.multistep = true;
  st.aux = d, st.cfg_scale = cfg_scale, st.a_t = a_t, st.sqrt_one_minus_at = sqrt_one_minus_at, st.k_x = k_x, st.k_d = k_d, st.k_p = k_p;
  return st;
}

int sdeo_ddim_step(sdeo_handle h, float* x, float* pred_x0, int table_row, float cfg_scale, float a_t, float a_prev,
                   float sqrt_one_minus_at, const float* host_control_scales, int only_mid_control, int flags, void* stream) {
  Step st = ddim_update("sdeo_ddim_step", pred_x0, cfg_scale, a_t, a_prev, sqrt_one_minus_at);
  st.coef_who = "cfg_ddim_pair";
  return fused_step(h, x, st, table_row, host_control_scales, only_mid_control, flags, S(stream));
}

int sdeo_dpmpp_2m_step(sdeo_handle h, float* x, float* d, int table_row, float cfg_scale, float a_t, float sqrt_one_minus_at, float k_x,
                       float k_d, float k_p, const float* host_control_scales, int only_mid_control, int flags, void* stream) {
  Step st = multistep_update("sdeo_dpmpp_2m_step", d, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p);
  SDEO_CHECK(d || k_p == 0.f, "%s: k_p=%g needs the previous data prediction, but d is null", st.who, k_p);   // this one in its own name
  st.coef_who = "cfg_lms_pair";
  return fused_step(h, x, st, table_row, host_control_scales, only_mid_control, flags, S(stream));
}

int sdeo_ddim_step_masked(sdeo_handle h, float* x, float* pred_x0, const float* orig, const float* noise, const float* mask, int mask_n,
                          int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row, float cfg_scale, float a_t, float a_prev,
                          float sqrt_one_minus_at, const float* host_control_scales, int only_mid_control, int flags, void* stream) {
  Step st = ddim_update("sdeo_ddim_step_masked", pred_x0, cfg_scale, a_t, a_prev, sqrt_one_minus_at);
  st.blended = true, st.blend = {orig, noise, mask, mask_n, mask_c, sqrt_a, sqrt_one_minus_a};
  return fused_step(h, x, st, table_row, host_control_scales, only_mid_control, flags, S(stream));
}

int sdeo_dpmpp_2m_step_masked(sdeo_handle h, float* x, float* d, const float* orig, const float* noise, const float* mask, int mask_n,
                              int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row, float cfg_scale, float a_t,
                              float sqrt_one_minus_at, float k_x, float k_d, float k_p, const float* host_control_scales,
                              int only_mid_control, int flags, void* stream) {
  Step st = multistep_update("sdeo_dpmpp_2m_step_masked", d, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p);
  st.blended = true, st.blend = {orig, noise, mask, mask_n, mask_c, sqrt_a, sqrt_one_minus_a};
  return fused_step(h, x, st, table_row, host_control_scales, only_mid_control, flags, S(stream));
}

// The stochastic steps also refuse what is theirs alone: a coefficient without its noise row, a partial set of blend operands, the
// staged flag together with a blend.
int sdeo_ddim_step_eta(sdeo_handle h, float* x, float* pred_x0, const float* noise, float sigma_t, const float* orig,
                       const float* mask_noise, const float* mask, int mask_n, int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row,
                       float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at, const float* host_control_scales,
                       int only_mid_control, int flags, void* stream) {
  Step st = ddim_update("sdeo_ddim_step_eta", pred_x0, cfg_scale, a_t, a_prev, sqrt_one_minus_at);
  st.stochastic = true, st.noise = noise, st.noise_coef = sigma_t;
  st.blended = orig != nullptr, st.blend = {orig, mask_noise, mask, mask_n, mask_c, sqrt_a, sqrt_one_minus_a};
  return fused_step(h, x, st, table_row, host_control_scales, only_mid_control, flags, S(stream));
}

int sdeo_dpmpp_2m_sde_step(sdeo_handle h, float* x, float* d, const float* noise, const float* orig, const float* mask_noise,
                           const float* mask, int mask_n, int mask_c, float sqrt_a, float sqrt_one_minus_a, int table_row, float cfg_scale,
                           float a_t, float sqrt_one_minus_at, float k_x, float k_d, float k_p, float k_n, const float* host_control_scales,
                           int only_mid_control, int flags, void* stream) {
  Step st = multistep_update("sdeo_dpmpp_2m_sde_step", d, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p);
  st.stochastic = true, st.noise = noise, st.noise_coef = k_n;
  st.blended = orig != nullptr, st.blend = {orig, mask_noise, mask, mask_n, mask_c, sqrt_a, sqrt_one_minus_a};
  return fused_step(h, x, st, table_row, host_control_scales, only_mid_control, flags, S(stream));
}

int sdeo_vae_decode(sdeo_handle h, const float* z, int n, float* images, uint8_t* images_u8, void* stream) {
  REQUIRE_READY(h);
  SDEO_CHECK(z && n >= 1 && (images || images_u8), "sdeo_vae_decode: bad argument");
  hipStream_t s = S(stream);
  const sdeo_config& c = h->cfg;
  const size_t px = (size_t)h->lh * h->lw;
  for (int i = 0; i < n; ++i) {
    if (int rc = copy_in(h->vae_in, z + (size_t)i * c.vae_z_channels * px, (size_t)c.vae_z_channels * px * 4, s)) return rc;
    if (int rc = run(h, h->prog[P_VAE], s)) return rc;
    if (images)
      if (int rc = copy_in(images + (size_t)i * c.vae_out_ch * px * 64, h->vae_out, (size_t)c.vae_out_ch * px * 64 * 4, s)) return rc;
    if (images_u8)
      if (int rc = copy_in(images_u8 + (size_t)i * c.vae_out_ch * px * 64, h->vae_u8, (size_t)c.vae_out_ch * px * 64, s)) return rc;
  }
  return 0;
}

int sdeo_vae_encode(sdeo_handle h, const float* images, const uint8_t* images_u8, int n, const float* noise, float* z, float* moments,
                    void* stream) {
  SDEO_CHECK(h, "sdeo_vae_encode: null handle");
  SDEO_CHECK(h->vae_encoder, "sdeo_vae_encode: this handle has no VAE encoder (call sdeo_enable_vae_encoder before loading weights)");
  REQUIRE_READY(h);
  SDEO_CHECK(!images != !images_u8, "sdeo_vae_encode: pass exactly one of images (fp32) and images_u8");
  SDEO_CHECK(z && n >= 1 && n <= h->N, "sdeo_vae_encode: bad argument (z %s, n = %d, configured %d)", z ? "set" : "NULL", n, h->N);
  hipStream_t s = S(stream);
  const sdeo_config& c = h->cfg;
  const size_t px = (size_t)h->lh * h->lw, ipx = px * 64, zc = (size_t)c.vae_z_channels;
  h->enc_from_u8 = images ? 0 : 1;
  h->enc_with_noise = noise ? 1 : 0;
  for (int i = 0; i < n; ++i) {
    if (images) {
      if (int rc = copy_in(h->enc_img, images + (size_t)i * c.vae_out_ch * ipx, (size_t)c.vae_out_ch * ipx * 4, s)) return rc;
    } else {
      if (int rc = copy_in(h->enc_img_u8, images_u8 + (size_t)i * c.vae_out_ch * ipx, (size_t)c.vae_out_ch * ipx, s)) return rc;
    }
    if (noise) if (int rc = copy_in(h->enc_noise, noise + (size_t)i * zc * px, zc * px * 4, s)) return rc;
    if (int rc = run(h, h->prog[P_VAE_ENC], s)) return rc;
    if (int rc = copy_in(z + (size_t)i * zc * px, h->enc_z, zc * px * 4, s)) return rc;
    if (moments) if (int rc = copy_in(moments + (size_t)i * 2 * zc * px, h->enc_moments, 2 * zc * px * 4, s)) return rc;
  }
  return 0;
}

size_t sdeo_device_bytes(sdeo_handle h) { return h ? h->device_bytes : 0; }

// ---- LoRA adapters: WeightStore does the work, the handle adds what it derives from the raw tensors and its caches
int sdeo_lora_apply(sdeo_handle h, const char* name, const float* down, const float* up, int rank, float scale, void* stream) {
  SDEO_CHECK(h, "sdeo_lora_apply: null handle");
  const char* not_ready = !h->finalized ? "weights not finalized (call sdeo_finalize_weights)"
                          : h->fp8.weight_bits == 8 ? "this handle holds fp8 weights (sdeo_set_weight_precision 8): its fp16 copies are the dequantised values, "
                                                      "not the raw ones, and adapters on it are not supported"
                                                    : nullptr;
  const size_t before = h->ws.lora_backup_bytes;
  const int rc = h->ws.lora_apply("sdeo_lora_apply", name, name ? name : "", down, up, rank, scale, not_ready, S(stream));
  h->device_bytes += h->ws.lora_backup_bytes - before;
  return rc;
}

int sdeo_lora_commit(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_lora_commit: null handle");
  SDEO_CHECK(h->finalized, "sdeo_lora_commit: weights not finalized (call sdeo_finalize_weights)");
  h->ws.lora_release_stage();
  if (int rc = derive_weights(h)) return rc;
  for (bool& b : h->hint_stale) b = true;
  h->ctx_stale = 3;
  h->tab_stale = true;
  return 0;
}

int sdeo_lora_clear(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_lora_clear: null handle");
  SDEO_CHECK(h->finalized, "sdeo_lora_clear: weights not finalized (call sdeo_finalize_weights)");
  const size_t before = h->ws.lora_backup_bytes;
  const int rc = h->ws.lora_restore();
  h->device_bytes -= before - h->ws.lora_backup_bytes;
  if (rc) return rc;
  return sdeo_lora_commit(h);
}

int sdeo_lora_touched(sdeo_handle h) { return h ? h->ws.lora_touched() : 0; }

int sdeo_read_weight(sdeo_handle h, const char* name, float* out) {
  SDEO_CHECK(h, "sdeo_read_weight: null handle");
  return h->ws.read("sdeo_read_weight", name, name ? name : "", out);
}

int sdeo_profile_begin(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_profile_begin: null handle");
  h->prof.begin();
  return 0;
}

const char* sdeo_profile_end(sdeo_handle h) { return h ? h->prof.end() : ""; }

}  // extern "C"
