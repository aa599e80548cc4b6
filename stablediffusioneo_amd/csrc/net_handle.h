// The SD handle (sdeo_handle_s) and the types it is made of, shared by the three units of the network executor:
//   net_weights.hip  the weight registry, what a handle derives from its raw tensors (LayerNorm folds, composed matrices, fp8 packs)
//                    and the entry points that only touch weights (load / finalize / precision / LoRA / read)
//   net_build.hip    the program builder, the block builders and the per-program builders of sdeo_configure (build_all)
//   net.hip          the handle's life (create, destroy, enable, configure) and every forward, fused step and VAE door
// plus the few helpers more than one of them needs and the functions that cross from one unit to another.
#pragma once
#include <cmath>
#include <functional>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include/sdeo.h"
#include "cache_record.h"
#include "handle_common.h"
#include "net_plan.h"

namespace sdeo {

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
  P_UNET_NOCTRL, P_VAE, P_VAE_ENC, P_TEMB, P_TEMB_CN, P_TEMB_TAB, P_X0, P_EPS_EXPORT,
  P_CTX_IP,      // sdeo_set_ip_tokens: image tokens -> K_ip | V_ip of every UNet cross-attention (empty without sdeo_enable_ip_adapter)
  P_COUNT
};

}  // namespace sdeo

using namespace sdeo;      // (an internal header: the three units that include it work in this namespace, as clip.hip and hed.hip do)

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
  // image-prompt adapter (sdeo_enable_ip_adapter): tokens per image (0: none), the boundary buffer of sdeo_set_ip_tokens
  // ([N][ip_tokens][context_dim] fp32) and the weight of the image term, read at LAUNCH by every cross-attention of the UNet
  int ip_tokens = 0;
  float* in_ip = nullptr;
  float ip_scale = 1.0f;
  // FreeU (sdeo_set_freeu): whether the decoder programs with the FreeU launches run, and what those launches read at LAUNCH -- (b, s) of
  // the 4 mc-channel stage and of the 2 mc-channel stage, and the version.  prog_freeu: P_UNET_DEC, P_UNET_DEC_FUSED and P_UNET_NOCTRL
  // as built, FreeU launches included; prog[] holds them without (build_all).  freeu_refusal: why these programs cannot run FreeU (a map
  // beyond the kernel's size limit), empty when they can
  bool freeu_on = false;
  float freeu_b[2] = {1.0f, 1.0f}, freeu_s[2] = {1.0f, 1.0f};
  int freeu_version = 2;
  Program prog_freeu[3];
  std::string freeu_refusal;
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
  // control modes (sdeo_enable_control_modes): per control net SDEO_CONTROL_BOTH / _COND / _OFF, host state read when a call launches
  // (sdeo_set_control_mode; sdeo_configure resets them to BOTH).  cn_half[j]: net j's ControlNet program on the first N / 2 images
  // (build_controlnet: every launch a batch prefix of the full-batch one, in the same tensors; empty when N is odd).  The fused decoders
  // of such a handle hold every form of each net's zero-conv launch (Op::zc_form); run_decoder picks.
  bool control_modes = false;
  int cmode[kMaxControlNets] = {0};
  Program cn_half[kMaxControlNets];
  // The cache contract (include/sdeo.h, "State a handle keeps between calls"): host-side record of what the caches hold, checked before
  // the first device call of every entry point that reads one on the caller's word.  A captured call is checked at capture.
  CacheRecord cache;
  // time embedding (`openaimodel.py:777-781` + every ResBlock's emb_layers): fp32 [N][emb_total] per net, written by P_TEMB + net from
  // in_t -- or, for a sampler that announced its schedule (sdeo_set_timestep_table), one row of a table computed once per schedule.
  // The ResBlock convs read their pointer / row stride at LAUNCH time (emb_cur / emb_ld_cur), like the control scales.
  static constexpr int kTabRows = SDEO_MAX_TABLE_STEPS;
  float* emb_all[kNets] = {nullptr};
  float* temb_tab[kNets] = {nullptr};          // [kTabRows][emb_total[net]]
  int64_t* tab_t = nullptr;                    // device int64 [kTabRows]
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

static_assert(kMaxControlNets == CacheRecord::kMaxNets, "the cache record keeps one hint entry per control network");

namespace sdeo {

typedef sdeo_handle_s Engine;

// where the one conv3x3 of a conv-only block (B_CONV_IN / B_DOWN / B_UP) keeps its parameters below the block's name
static const char* conv_suffix(BlkKind k) { return k == B_DOWN ? ".op" : k == B_UP ? ".conv" : ""; }

// namespace of network `net`'s tensors: the UNet, `control_model.`, `control_model_<j>.` for the extra control net j = net - 1
static std::string net_ns(int net) { return net == 0 ? NS_UNET : net == 1 ? NS_CN : "control_model_" + std::to_string(net - 1) + "."; }

static Program& cn_prog(Engine* e, int j, CnProg k) {
  static const ProgId kCnProg0[CP_COUNT] = {P_HINT, P_CTX_CN, P_CN, P_CN_SH, P_TEMB_CN};
  return j == 0 ? e->prog[kCnProg0[k]] : e->xprog[j - 1][k];
}

static bool configured(const Engine* e) { return e->lanes[L_MAIN].base != nullptr; }

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- what crosses from one unit to another
// net_weights.hip: register the tensors of a new handle (the UNet, control network 0, the VAE decoder), of `count` extra control
// networks and of the VAE encoder, each behind everything registered before it
void build_registry(Engine* e);
void reg_extra_controlnets(Engine* e, int count);
void reg_vae_encoder(Engine* e);
void reg_ip_adapter(Engine* e);
// net_build.hip: one pass over every program of the handle (dry: plan the arenas only)
int build_all(Engine* e, bool dry, size_t* max_splitk, size_t* max_gn, size_t peaks[L_COUNT]);

}  // namespace sdeo
