// Network executor of libsdeo, the handle's life and its forwards: create / destroy / enable / configure, and the net-level C entry
// points of include/sdeo.h that run the programs net_build.hip built over the weights net_weights.hip registered -- the forwards, the
// timestep table, the six fused steps, VAE decode and encode, the profile calls.  Each reads as: checks of the cache record
// (cache_record.h), device work, transitions of the record.
#include "net_handle.h"

namespace {

static int run(Engine* e, const Program& p, hipStream_t s, bool skip_zero_convs = false) {
  if (!skip_zero_convs) return run_program(p, s, &e->prof);
  for (auto& op : p) {       // the ControlNet program without its zero convs
    if (op.zero_conv) continue;
    if (int rc = e->prof.on ? e->prof.record(op, s) : op(s)) return rc;
  }
  return 0;
}

// a program that holds a UNet decoder: with sdeo_set_freeu on, the one that kept its FreeU launches
static const Program& decoder_program(const Engine* e, ProgId id) {
  if (!e->freeu_on) return e->prog[id];
  return e->prog_freeu[id == P_UNET_DEC ? 0 : id == P_UNET_DEC_FUSED ? 1 : 2];
}

// Control modes of one call (sdeo_set_control_mode), as the call sees them: without a second half (an unguided step) COND means BOTH.
struct CallModes {
  int m[kMaxControlNets] = {0};
  bool any_cond = false, all_off = false, all_both = true;
};
static CallModes call_modes(const Engine* e, bool has_second_half) {
  CallModes cm;
  if (!e->control_modes) return cm;
  cm.all_off = true;
  for (int j = 0; j <= e->extra; ++j) {
    cm.m[j] = e->cmode[j] == SDEO_CONTROL_COND && !has_second_half ? SDEO_CONTROL_BOTH : e->cmode[j];
    cm.any_cond |= cm.m[j] == SDEO_CONTROL_COND;
    cm.all_off &= cm.m[j] == SDEO_CONTROL_OFF;
    cm.all_both &= cm.m[j] == SDEO_CONTROL_BOTH;
  }
  return cm;
}

// The fused decoder under the modes of this call: of each net's zero-conv launches the one form its mode asks for -- none for an OFF
// net; for the others all rows or the first half, with the skip as the residual for the first active net and in place behind it.
// All BOTH picks exactly the launches a plain handle's program holds.
static int run_decoder(Engine* e, const Program& p, const CallModes& cm, hipStream_t s) {
  if (!e->control_modes) return run(e, p, s);
  int want[kMaxControlNets];
  bool seen = false;
  for (int j = 0; j < kMaxControlNets; ++j) {
    want[j] = -1;
    if (j > e->extra || cm.m[j] == SDEO_CONTROL_OFF) continue;
    want[j] = (cm.m[j] == SDEO_CONTROL_COND ? 1 : 0) | (seen ? 0 : 2);      // (ZC_COND | ZC_FIRST of net_build.hip)
    seen = true;
  }
  for (auto& op : p) {
    if (op.zc_net >= 0 && op.zc_form != want[(int)op.zc_net]) continue;
    if (int rc = e->prof.on ? e->prof.record(op, s) : op(s)) return rc;
  }
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

static void free_configured(Engine* e) {
  for (void* v : e->extra_allocs) (void)hipFree(v);      // (the lanes' workspaces among them)
  e->extra_allocs.clear();
  for (Lane& l : e->lanes) {
    if (l.base) (void)hipFree(l.base);
    l = Lane();
  }
  for (Program& p : e->prog) p.clear();
  for (Program& p : e->prog_freeu) p.clear();
  for (auto& px : e->xprog) for (Program& p : px) p.clear();
  for (Program& p : e->cn_half) p.clear();
  for (int& m : e->cmode) m = SDEO_CONTROL_BOTH;          // the control modes return to BOTH
  for (int j = 0; j < kMaxControlNets - 1; ++j) {        // the hint caches are gone with the arenas, the scales return to 1
    for (float& v : e->extra_scales[j]) v = 1.0f;
  }
  e->cache.configured_anew();                            // ... and so are the context K / V, the staged latent and the table
  e->fp8.mx_launches = 0;
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
  reg_extra_controlnets(h, count);
  if (int rc = h->ws.alloc("sdeo_enable_extra_controlnets", /*zero_fill=*/true)) return rc;
  h->device_bytes = h->ws.slab_bytes;
  h->extra = count;
  return 0;
}

int sdeo_enable_ip_adapter(sdeo_handle h, int num_tokens) {
  SDEO_CHECK(num_tokens >= 1 && num_tokens <= 64, "sdeo_enable_ip_adapter: num_tokens %d out of range (1..64 image tokens)", num_tokens);
  SDEO_CHECK(h, "sdeo_enable_ip_adapter: null handle");
  SDEO_CHECK(!h->ip_tokens, "sdeo_enable_ip_adapter: already called (this handle has an adapter of %d tokens)", h->ip_tokens);
  for (const auto& w : h->ws.entries)
    SDEO_CHECK(!w.loaded, "sdeo_enable_ip_adapter: call it before the first sdeo_load_weight (%s is loaded)", w.name.c_str());
  SDEO_CHECK(!h->finalized && !configured(h), "sdeo_enable_ip_adapter: call it before sdeo_finalize_weights / sdeo_configure");
  // the two-segment cross-attention exists for the head dims of the one-wave-per-query-block kernels: refuse the others here, on the host
  int bad_d = 0;
  for_each_block(h->uplan, [&](const Blk& b) {
    if (b.kind == B_ATTN && !bad_d && !attention2_kernel_name(1, b.heads, 1, h->cfg.context_len, num_tokens, b.cin / b.heads)) bad_d = b.cin / b.heads;
  });
  if (bad_d) {
    const std::string why = sdeo_last_error();
    return fail("sdeo_enable_ip_adapter: head dim %d has no two-segment attention kernel (%s)", bad_d, why.c_str());
  }
  // behind everything registered so far: the offsets of the existing tensors do not move
  reg_ip_adapter(h);
  if (int rc = h->ws.alloc("sdeo_enable_ip_adapter", /*zero_fill=*/true)) return rc;
  h->device_bytes = h->ws.slab_bytes;
  h->ip_tokens = num_tokens;
  return 0;
}

int sdeo_enable_control_modes(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_enable_control_modes: null handle");
  SDEO_CHECK(!configured(h), "sdeo_enable_control_modes: call it before sdeo_configure");
  SDEO_CHECK(h->fp8.weight_bits != 8, "sdeo_enable_control_modes: fp8 weights (sdeo_set_weight_precision 8) are not supported with control modes");
  SDEO_CHECK(h->fp8.act_bits != 8, "sdeo_enable_control_modes: block-scaled fp8 activations (sdeo_set_activation_precision 8) are not supported with control modes");
  h->control_modes = true;
  return 0;
}

int sdeo_set_control_mode(sdeo_handle h, int net, int mode) {
  SDEO_CHECK(h, "sdeo_set_control_mode: null handle");
  SDEO_CHECK(h->control_modes, "sdeo_set_control_mode: this handle has no control modes (call sdeo_enable_control_modes before sdeo_configure)");
  SDEO_CHECK(net >= 0 && net <= h->extra, "sdeo_set_control_mode: net %d out of range (0..%d)", net, h->extra);
  SDEO_CHECK(mode == SDEO_CONTROL_BOTH || mode == SDEO_CONTROL_COND || mode == SDEO_CONTROL_OFF,
             "sdeo_set_control_mode: mode %d is none of SDEO_CONTROL_BOTH, SDEO_CONTROL_COND, SDEO_CONTROL_OFF", mode);
  h->cmode[net] = mode;
  return 0;
}

static int configure_impl(sdeo_handle h, int n, int latent_h, int latent_w) {
  free_configured(h);
  h->ip_scale = 1.0f;
  h->freeu_on = false;           // FreeU off and its values back to the identity, as ip_scale returns to 1
  h->freeu_b[0] = h->freeu_b[1] = h->freeu_s[0] = h->freeu_s[1] = 1.0f;
  h->freeu_version = 2;
  h->freeu_refusal.clear();
  h->N = n; h->lh = latent_h; h->lw = latent_w;
  const sdeo_config& c = h->cfg;
  const size_t px = (size_t)latent_h * latent_w;
  // boundary buffers
  if (int rc = dev_alloc(h, &h->in_x, (size_t)n * c.in_channels * px * 4)) return rc;
  for (int j = 0; j <= h->extra; ++j)
    if (int rc = dev_alloc(h, &h->in_hint[j], (size_t)n * c.hint_channels * px * 64 * 4)) return rc;
  if (int rc = dev_alloc(h, &h->in_ctx, (size_t)n * c.context_len * c.context_dim * 4)) return rc;
  if (int rc = dev_alloc(h, &h->in_t, (size_t)n * 8)) return rc;
  if (h->ip_tokens) if (int rc = dev_alloc(h, &h->in_ip, (size_t)n * h->ip_tokens * c.context_dim * 4)) return rc;
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
  SDEO_CHECK(!h->control_modes || (h->fp8.weight_bits != 8 && h->fp8.act_bits != 8),
             "sdeo_configure: control modes (sdeo_enable_control_modes) are not supported with fp8 weights or block-scaled fp8 activations");
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
    h->cache.hint_filled(0);
  }
  if (ctx) {
    h->cache.context_staging(ctx_for_net);
    if (int rc = copy_in(h->in_ctx, ctx, (size_t)h->N * c.context_len * c.context_dim * 4, s)) return rc;
    if (ctx_for_net & CacheRecord::UNET) if (int rc = run(h, h->prog[P_CTX_UNET], s)) return rc;
    if (ctx_for_net & CacheRecord::CONTROL)
      for (int j = 0; j <= h->extra; ++j) if (int rc = run(h, cn_prog(h, j, CP_CTX), s)) return rc;
    h->cache.context_filled(ctx_for_net);
  }
  return 0;
}

// P_X0: the fp16 copy of in_x.  Whatever a fused step staged in x0 is gone.
static int run_x0(sdeo_handle h, hipStream_t s) {
  h->cache.latent_overwritten();
  return run(h, h->prog[P_X0], s);
}

#define REQUIRE_READY(h)                                                                     \
  SDEO_CHECK(h, "null handle");                                                              \
  SDEO_CHECK(h->finalized, "weights not finalized (call sdeo_finalize_weights)");            \
  SDEO_CHECK(configured(h), "not configured (call sdeo_configure)")

// SDEO_TIMESTEP_ROW(i) taken apart: whether the flags carry a row, and which
static bool has_timestep_row(int flags) { return (flags & SDEO_TIMESTEP_ROW(0)) != 0; }
static int timestep_row(int flags) { return flags >> __builtin_ctz(SDEO_TIMESTEP_ROW(1) ^ SDEO_TIMESTEP_ROW(0)); }

// time embedding of this forward: row `row` of the schedule table (>= 0; every image of the batch at that timestep), or in_t via P_TEMB + net
static int select_time(sdeo_handle h, int flags, const int64_t* timesteps, const char* who, int* row_out) {
  const int row = has_timestep_row(flags) ? timestep_row(flags) : -1;
  SDEO_CHECK(row >= 0 || timesteps, "%s: timesteps required", who);
  if (int rc = h->cache.table_row(who, row)) return rc;
  for (int net = 0; net < 2 + h->extra; ++net) {
    h->emb_cur[net] = row >= 0 ? h->temb_tab[net] + (size_t)row * h->emb_total[net] : h->emb_all[net];
    h->emb_ld_cur[net] = row >= 0 ? 0 : h->emb_total[net];
  }
  *row_out = row;
  return 0;
}

// The time embeddings of the extra control networks.  They run in FRONT of net 0's ControlNet: their temporaries were planned on the
// empty side arena, where net 0's block outputs (kept until the decoder has run) live afterwards.
static int run_extra_time_embeds(sdeo_handle h, const CallModes& cm, hipStream_t s) {
  for (int j = 1; j <= h->extra; ++j)
    if (cm.m[j] != SDEO_CONTROL_OFF) if (int rc = run(h, cn_prog(h, j, CP_TEMB), s)) return rc;
  return 0;
}

// control net j's program of this call, without its zero convs: none for an OFF net, the half-batch one for a COND net, else the
// full-batch one or, where the caller vouches for the hints and configure built it, its shared-prefix variant
static int run_controlnet(sdeo_handle h, int j, const CallModes& cm, bool shared_cn, hipStream_t s) {
  if (cm.m[j] == SDEO_CONTROL_OFF) return 0;
  if (cm.m[j] == SDEO_CONTROL_COND) return run(h, h->cn_half[j], s);
  const Program& sh = cn_prog(h, j, CP_CN_SH);
  return run(h, shared_cn && !sh.empty() ? sh : cn_prog(h, j, CP_CN), s, true);
}

// the extra control networks, one behind the other on the stream net 0's ControlNet ran on, without their zero convs
static int run_extra_controlnets(sdeo_handle h, const CallModes& cm, bool shared_cn, hipStream_t s) {
  for (int j = 1; j <= h->extra; ++j) if (int rc = run_controlnet(h, j, cm, shared_cn, s)) return rc;
  return 0;
}

// ControlNet || UNet encoder, join, UNet decoder: eps16 holds the result.  The latent is already in x0.
// shared_unet / shared_cn: the two halves of the batch are the same images at the same timestep (and, for the ControlNet, under the same
// hint): run the programs whose shared prefix is computed once, where configure built them
// cm: the control modes of this call (call_modes).  Every net OFF is the no-control program: no fork, no ControlNet launch.
static int run_step_programs(sdeo_handle h, bool no_control, bool time_from_table, hipStream_t s, const CallModes& cm, bool shared_unet = false,
                             bool shared_cn = false) {
  const Program& p_unet_enc = shared_unet && !h->prog[P_UNET_ENC_SH].empty() ? h->prog[P_UNET_ENC_SH] : h->prog[P_UNET_ENC];
  if (no_control || cm.all_off) {
    if (!time_from_table) if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
    return run(h, decoder_program(h, P_UNET_NOCTRL), s);
  }
  if (h->overlap && !h->prof.on) {
    // fork: ControlNet on the side stream, UNet encoder + middle block on the caller's stream (capturable)
    SDEO_HIP(hipEventRecord(h->ev_fork, s));
    SDEO_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    if (!time_from_table) {
      if (cm.m[0] != SDEO_CONTROL_OFF) if (int rc = run(h, h->prog[P_TEMB + 1], h->side)) return rc;
      if (int rc = run_extra_time_embeds(h, cm, h->side)) return rc;
    }
    if (int rc = run_controlnet(h, 0, cm, shared_cn, h->side)) return rc;
    if (int rc = run_extra_controlnets(h, cm, shared_cn, h->side)) return rc;
    SDEO_HIP(hipEventRecord(h->ev_join, h->side));
    if (!time_from_table) if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
    if (int rc = run(h, p_unet_enc, s)) return rc;
    SDEO_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
  } else {
    if (!time_from_table) {
      if (cm.m[0] != SDEO_CONTROL_OFF) if (int rc = run(h, h->prog[P_TEMB + 1], s)) return rc;
      if (int rc = run_extra_time_embeds(h, cm, s)) return rc;
      if (int rc = run(h, h->prog[P_TEMB + 0], s)) return rc;
    }
    if (int rc = run_controlnet(h, 0, cm, shared_cn, s)) return rc;
    if (int rc = run_extra_controlnets(h, cm, shared_cn, s)) return rc;
    if (int rc = run(h, p_unet_enc, s)) return rc;
  }
  return run_decoder(h, decoder_program(h, P_UNET_DEC_FUSED), cm, s);      // applies the zero convs itself (skipped above)
}

// copy net j's hint in and run its hint block into its cached features (j >= 1; net 0's goes through stage_inputs)
static int set_extra_hint(sdeo_handle h, int j, const float* hint, hipStream_t s) {
  const size_t bytes = (size_t)h->N * h->cfg.hint_channels * h->lh * h->lw * 64 * 4;
  if (int rc = copy_in(h->in_hint[j], hint, bytes, s)) return rc;
  if (int rc = run(h, cn_prog(h, j, CP_HINT), s)) return rc;
  h->cache.hint_filled(j);
  return 0;
}

static int controlnet_forward_impl(sdeo_handle h, int j, const float* x_noisy, const float* hint, const int64_t* timesteps,
                                   const float* context, float* const* controls, int flags, const char* who, hipStream_t s) {
  SDEO_CHECK(x_noisy && controls, "%s: null argument", who);
  const int hint_new = !(flags & SDEO_HINT_CACHED), ctx_new = !(flags & SDEO_CONTEXT_CACHED);
  SDEO_CHECK(!hint_new || hint, "%s: hint required", who);
  SDEO_CHECK(!ctx_new || context, "%s: context required", who);
  if (j != 0 && !hint_new) if (int rc = h->cache.net_has_hint(who, j)) return rc;
  if (int rc = h->cache.cached_reads(who, hint_new ? -1 : j, ctx_new ? 0 : CacheRecord::CONTROL)) return rc;
  int trow = -1;
  if (int rc = select_time(h, flags, timesteps, who, &trow)) return rc;
  if (int rc = stage_inputs(h, x_noisy, j == 0 ? hint : nullptr, trow < 0 ? timesteps : nullptr, ctx_new ? context : nullptr, hint_new,
                            CacheRecord::CONTROL, s))
    return rc;
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

// What sdeo_enable_ip_adapter adds to a handle's life: the tokens of the image prompt, projected once into the K_ip | V_ip every UNet
// cross-attention reads by address (P_CTX_IP), and the weight of the image term.
int sdeo_set_ip_tokens(sdeo_handle h, const float* tokens, void* stream) {
  SDEO_CHECK(h, "sdeo_set_ip_tokens: null handle");
  SDEO_CHECK(h->ip_tokens, "sdeo_set_ip_tokens: this handle has no image-prompt adapter (call sdeo_enable_ip_adapter before loading weights)");
  SDEO_CHECK(h->finalized, "sdeo_set_ip_tokens: weights not finalized (call sdeo_finalize_weights)");
  SDEO_CHECK(configured(h), "sdeo_set_ip_tokens: not configured (call sdeo_configure)");
  SDEO_CHECK(tokens, "sdeo_set_ip_tokens: null tokens");
  hipStream_t s = S(stream);
  h->cache.ip_staging();
  if (int rc = copy_in(h->in_ip, tokens, (size_t)h->N * h->ip_tokens * h->cfg.context_dim * 4, s)) return rc;
  if (int rc = run(h, h->prog[P_CTX_IP], s)) return rc;
  h->cache.ip_filled();
  return 0;
}

int sdeo_set_ip_scale(sdeo_handle h, float scale) {
  SDEO_CHECK(h, "sdeo_set_ip_scale: null handle");
  SDEO_CHECK(h->ip_tokens, "sdeo_set_ip_scale: this handle has no image-prompt adapter (call sdeo_enable_ip_adapter before loading weights)");
  SDEO_CHECK(std::isfinite(scale), "sdeo_set_ip_scale: the scale is not finite");
  h->ip_scale = scale;
  return 0;
}

// FreeU: which decoder programs the following forwards and steps run, and the values their FreeU launches read when they run.  Host
// state only: every refusal precedes it, and there is no device call to precede.
int sdeo_set_freeu(sdeo_handle h, float b1, float b2, float s1, float s2, int version) {
  if (int rc = freeu_params_check("sdeo_set_freeu", b1, b2, s1, s2, version)) return rc;
  SDEO_CHECK(h, "sdeo_set_freeu: null handle");
  SDEO_CHECK(h->freeu_refusal.empty(), "sdeo_set_freeu: %s", h->freeu_refusal.c_str());
  h->freeu_b[0] = b1; h->freeu_b[1] = b2; h->freeu_s[0] = s1; h->freeu_s[1] = s2;
  h->freeu_version = version;
  h->freeu_on = true;
  return 0;
}

int sdeo_clear_freeu(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_clear_freeu: null handle");
  h->freeu_on = false;
  return 0;
}

int sdeo_unet_forward(sdeo_handle h, const float* x_noisy, const int64_t* timesteps, const float* context,
                      const float* const* controls, const float* host_control_scales, int only_mid_control, float* eps,
                      int flags, void* stream) {
  REQUIRE_READY(h);
  SDEO_CHECK(x_noisy && eps, "sdeo_unet_forward: null argument");
  hipStream_t s = S(stream);
  const int ctx_new = !(flags & SDEO_CONTEXT_CACHED);
  SDEO_CHECK(!ctx_new || context, "sdeo_unet_forward: context required");
  if (int rc = h->cache.cached_reads("sdeo_unet_forward", -1, ctx_new ? 0 : CacheRecord::UNET)) return rc;
  if (h->ip_tokens) if (int rc = h->cache.ip_tokens("sdeo_unet_forward")) return rc;
  int trow = -1;
  if (int rc = select_time(h, flags, timesteps, "sdeo_unet_forward", &trow)) return rc;
  if (int rc = stage_inputs(h, x_noisy, nullptr, trow < 0 ? timesteps : nullptr, ctx_new ? context : nullptr, 0, CacheRecord::UNET, s)) return rc;
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
    if (int rc = run(h, decoder_program(h, P_UNET_DEC), s)) return rc;
  } else {
    if (int rc = run(h, decoder_program(h, P_UNET_NOCTRL), s)) return rc;
  }
  if (int rc = run(h, h->prog[P_EPS_EXPORT], s)) return rc;
  return copy_in(eps, h->out_eps, (size_t)h->N * h->cfg.out_channels * h->lh * h->lw * 4, s);
}

int sdeo_apply_model(sdeo_handle h, const float* x_noisy, const float* hint, const int64_t* timesteps, const float* context,
                     const float* host_control_scales, int only_mid_control, int flags, float* eps, void* stream) {
  REQUIRE_READY(h);
  SDEO_CHECK(x_noisy && eps, "sdeo_apply_model: null argument");
  hipStream_t s = S(stream);
  const int hint_new = !(flags & SDEO_HINT_CACHED), ctx_new = !(flags & SDEO_CONTEXT_CACHED), no_control = (flags & SDEO_NO_CONTROL) != 0;
  SDEO_CHECK(!ctx_new || context, "sdeo_apply_model: context required");
  SDEO_CHECK(no_control || !hint_new || hint, "sdeo_apply_model: hint required");
  const CallModes cm = call_modes(h, true);
  SDEO_CHECK(no_control || !cm.any_cond || h->N % 2 == 0, "sdeo_apply_model: SDEO_CONTROL_COND runs the control network on the first n / 2 images, "
             "the conditional half of [cond; uncond]: configured for %d images, an odd count", h->N);
  const int sides = no_control ? CacheRecord::UNET : CacheRecord::BOTH;      // whose context K / V this call runs on
  if (!no_control) if (int rc = h->cache.extra_hints("sdeo_apply_model", h->extra)) return rc;
  if (int rc = h->cache.cached_reads("sdeo_apply_model", no_control || hint_new ? -1 : 0, ctx_new ? 0 : sides)) return rc;
  if (h->ip_tokens) if (int rc = h->cache.ip_tokens("sdeo_apply_model")) return rc;
  int trow = -1;
  if (int rc = select_time(h, flags, timesteps, "sdeo_apply_model", &trow)) return rc;
  if (int rc = stage_inputs(h, x_noisy, no_control ? nullptr : hint, trow < 0 ? timesteps : nullptr, ctx_new ? context : nullptr, hint_new,
                            sides, s))
    return rc;
  set_scales(h, host_control_scales, only_mid_control);
  if (int rc = run_x0(h, s)) return rc;
  if (int rc = run_step_programs(h, no_control, trow >= 0, s, cm)) return rc;
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
  h->cache.table_refilling();
  SDEO_HIP(hipMemcpyAsync(h->tab_t, padded, sizeof(padded), hipMemcpyHostToDevice, s));
  SDEO_HIP(hipStreamSynchronize(s));          // `padded` is a stack array; this call is made once per schedule, outside any capture
  if (int rc = run(h, h->prog[P_TEMB_TAB], s)) return rc;
  h->cache.table_filled(count);
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
  if (int rc = h->cache.step_table_row(who, table_row)) return rc;
  if (int rc = h->cache.extra_hints(who, h->extra)) return rc;
  if (int rc = h->cache.cached_reads(who, 0, CacheRecord::BOTH)) return rc;
  if (h->ip_tokens) if (int rc = h->cache.ip_tokens(who)) return rc;
  if (!blend && (flags & SDEO_STEP_LATENT_STAGED)) if (int rc = h->cache.staged_latent(who, x, paired)) return rc;
  if (blend) {
    SDEO_CHECK(!(flags & SDEO_STEP_LATENT_STAGED), "%s: SDEO_STEP_LATENT_STAGED has no meaning here (the blend changes the latent and always restages it)", who);
    if (int rc = mask_blend_check(who, x, blend->orig, blend->noise, blend->mask, blend->mask_n, blend->mask_c, b, h->cfg.in_channels,
                                  h->lh * h->lw))
      return rc;
  }
  int trow = -1;
  if (int rc = select_time(h, SDEO_TIMESTEP_ROW(table_row), nullptr, who, &trow)) return rc;
  set_scales(h, host_control_scales, only_mid_control);
  h->cache.step_launching();                      // until the update kernel has left the new latent in x0 (fused_step)
  if (blend) {
    if (int rc = mask_blend_pair(x, blend->orig, blend->noise, blend->mask, blend->mask_n, blend->mask_c, blend->sqrt_a, blend->sqrt_1ma,
                                 h->x0.p, h->x0.ld, b, h->cfg.in_channels, h->lh * h->lw, paired, s))
      return rc;
  } else if (!(flags & SDEO_STEP_LATENT_STAGED)) {
    if (int rc = latent_pair_to_nhwc(h->x0.p, h->x0.ld, x, b, h->cfg.in_channels, h->lh * h->lw, paired, s)) return rc;
  }
  // x0 = [x; x] at one timestep: the UNet's shared prefix always holds, the ControlNet's when the caller vouches for the hints
  return run_step_programs(h, false, true, s, call_modes(h, paired), paired, paired && (flags & SDEO_STEP_HINT_SHARED) != 0);
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
  if (!rc) h->cache.step_succeeded(x, paired);
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

int sdeo_profile_begin(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_profile_begin: null handle");
  h->prof.begin();
  return 0;
}

const char* sdeo_profile_end(sdeo_handle h) { return h ? h->prof.end() : ""; }

}  // extern "C"
