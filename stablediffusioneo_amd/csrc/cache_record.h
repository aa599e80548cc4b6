// The cache contract of a handle (include/sdeo.h, "State a handle keeps between calls") as one host-only type:
// what the five items that outlive a call hold, one transition per "filled by" / "cleared by" row of that table, and the checks the
// entry points make before their first device call.  This header is the contract's only implementation: the entry points of net.hip
// and net_weights.hip read as record checks, device work and record transitions, and nothing outside this file touches a field.
// Standard C++ only (no HIP include): tests/cache_record_check.cpp builds it with the host compiler and supplies its own sdeo::fail.
//
// What a change here must keep (tests/test_cache_contract_gpu.py matches the messages by regex; README and DESIGN quote some):
//   * every message byte for byte, format arguments included;
//   * cached_reads checks in this order: hint stale, context stale, hint unset, UNet context unset, control-net context unset, epoch
//     mismatch -- so a cache that is both stale and unset (sdeo_lora_commit, then sdeo_configure) is reported stale;
//   * extra_hints checks every "no hint" over j first, then every "stale";
//   * controlnet_forward's own net_has_hint check for j >= 1 runs in front of cached_reads;
//   * configured_anew clears the set flags, the staged latent and the table count, not the stale bits and not the context epochs;
//   * context_staging drops the sides and advances the epoch BEFORE the context programs run, context_filled sets the sides, clears
//     their stale bits and stamps their epochs AFTER: a failed launch leaves the side unset;
//   * table_refilling zeroes the count before the copy, table_filled sets it after the program ran;
//   * a fused step makes every check before its first launch, calls step_launching just before it and step_succeeded only if the
//     update launcher returned 0: a refused step leaves the record equal (==) to what it was;
//   * every check runs on the host when the call is made (a captured call: at capture), none at replay.  No check changes the record.
#pragma once

namespace sdeo {

int fail(const char* fmt, ...);      // the declaration of common.h: sets the thread's last error, returns nonzero

class CacheRecord {
 public:
  static constexpr int kMaxNets = 4;      // control networks of one handle (net_handle.h: kMaxControlNets)
  enum Side { UNET = 1, CONTROL = 2, BOTH = 3 };      // whose context K / V: a bit set

  // ---- transitions
  // sdeo_configure (and what undoes a failed one): the caches are gone with the arenas
  void configured_anew() {
    for (bool& b : hint_set) b = false;
    ctx_set = 0;
    x0_staged_for = nullptr;
    tab_count = 0;
    ip_set = false;
  }
  // sdeo_set_ip_tokens projected the image tokens of an adapter handle into every cross-attention's K_ip | V_ip.  No sdeo_lora_commit
  // makes them stale: no adapter can touch the ip matrices (sdeo_lora_apply refuses their names), so weights_changed leaves this alone.
  void ip_staging() { ip_set = false; }                  // (a failed launch leaves the item unset)
  void ip_filled() { ip_set = true; }
  // the hint block of control network j ran on a hint given now
  void hint_filled(int j) {
    hint_stale[j] = false;
    hint_set[j] = true;
  }
  // a new context is about to be projected for `sides`, and has been
  void context_staging(int sides) {
    ctx_set &= ~sides;                   // (a failed launch leaves the side unset, not half written and trusted)
    ++ctx_epoch;
  }
  void context_filled(int sides) {
    ctx_stale &= ~sides;
    ctx_set |= sides;
    for (int side = 0; side < 2; ++side) if (sides >> side & 1) ctx_epoch_of[side] = ctx_epoch;
  }
  // a plain forward writes the fp16 copy of its own latent over whatever a fused step staged
  void latent_overwritten() { x0_staged_for = nullptr; }
  // a fused step: nothing is staged from its first launch until its update kernel has left the new latent of x behind
  void step_launching() { x0_staged_for = nullptr; }
  void step_succeeded(const float* x, bool paired) { x0_staged_for = x, x0_staged_paired = paired; }
  // sdeo_set_timestep_table: no row is valid while the table is rewritten
  void table_refilling() { tab_count = 0; }
  void table_filled(int count) {
    tab_count = count;
    tab_stale = false;
  }
  // sdeo_lora_commit changed the weights under the caches: each stays stale until the call that fills it runs again.  A handle that
  // never commits an adapter never sets these.
  void weights_changed() {
    for (bool& b : hint_stale) b = true;
    ctx_stale = BOTH;
    tab_stale = true;
  }

  // ---- checks: `who` is the entry point; 0, or the failure (sdeo::fail)
  // the *_CACHED reads.  hint_net: the control network whose SDEO_HINT_CACHED features the call reads (-1: none); ctx_sides: whose
  // context K / V it reads from the cache (0: none)
  int cached_reads(const char* who, int hint_net, int ctx_sides) const {
    if (hint_net >= 0 && hint_stale[hint_net])
      return fail("%s: SDEO_HINT_CACHED, but sdeo_lora_commit changed the weights the cached hint features of control network %d were computed "
                  "with (pass the hint again)", who, hint_net);
    if (ctx_stale & ctx_sides)
      return fail("%s: SDEO_CONTEXT_CACHED, but sdeo_lora_commit changed the weights the cached context K / V were computed with (pass the "
                  "context again)", who);
    if (hint_net >= 0 && !hint_set[hint_net])
      return fail("%s: SDEO_HINT_CACHED, but control network %d has no hint since the last sdeo_configure (%s)", who, hint_net,
                  hint_net == 0 ? "pass the hint to sdeo_apply_model or sdeo_controlnet_forward" : "call sdeo_set_control_hint");
    if (ctx_sides & UNET & ~ctx_set)
      return fail("%s: SDEO_CONTEXT_CACHED, but the UNet has no context K / V since the last sdeo_configure (pass the context to "
                  "sdeo_apply_model or sdeo_unet_forward)", who);
    if (ctx_sides & CONTROL & ~ctx_set)
      return fail("%s: SDEO_CONTEXT_CACHED, but the control networks have no context K / V since the last sdeo_configure (pass the context to "
                  "sdeo_apply_model or sdeo_controlnet_forward)", who);
    if (ctx_sides == BOTH && ctx_epoch_of[0] != ctx_epoch_of[1])
      return fail("%s: SDEO_CONTEXT_CACHED, but the cached context K / V of the UNet and of the control networks were computed from different "
                  "contexts (a call that refreshes one side only ran since: sdeo_unet_forward, sdeo_controlnet_forward or SDEO_NO_CONTROL; pass "
                  "the context to sdeo_apply_model again)", who);
    return 0;
  }
  // sdeo_controlnet_forward_net on net j >= 1 without a hint of its own
  int net_has_hint(const char* who, int j) const {
    if (!hint_set[j]) return fail("%s: control network %d has no hint since the last sdeo_configure", who, j);
    return 0;
  }
  // a forward that runs the control networks needs the hint cache of every extra net 1..extra filled (sdeo_set_control_hint)
  int extra_hints(const char* who, int extra) const {
    for (int j = 1; j <= extra; ++j)
      if (!hint_set[j])
        return fail("%s: control network %d has no hint since the last sdeo_configure (call sdeo_set_control_hint(h, %d, ...))", who, j, j);
    for (int j = 1; j <= extra; ++j)
      if (hint_stale[j])
        return fail("%s: sdeo_lora_commit changed the weights the cached hint features of control network %d were computed with "
                    "(call sdeo_set_control_hint(h, %d, ...) again)", who, j, j);
    return 0;
  }
  // SDEO_TIMESTEP_ROW(row) of a forward; row < 0: the call brought its timesteps and reads no table
  int table_row(const char* who, int row) const {
    if (row >= tab_count) return fail("%s: timestep row %d, but the table holds %d (sdeo_set_timestep_table)", who, row, tab_count);
    if (row >= 0 && tab_stale)
      return fail("%s: SDEO_TIMESTEP_ROW, but sdeo_lora_commit changed the weights the timestep table was computed with "
                  "(call sdeo_set_timestep_table again)", who);
    return 0;
  }
  // table_row of a fused step
  int step_table_row(const char* who, int row) const {
    if (row < 0 || row >= tab_count) return fail("%s: timestep row %d, but the table holds %d (sdeo_set_timestep_table)", who, row, tab_count);
    if (tab_stale)
      return fail("%s: sdeo_lora_commit changed the weights the timestep table was computed with (call sdeo_set_timestep_table again)", who);
    return 0;
  }
  // SDEO_STEP_LATENT_STAGED of a fused step on x, a CFG-pair step or an unguided one
  int staged_latent(const char* who, const float* x, bool paired) const {
    if (!x0_staged_for)
      return fail("%s: SDEO_STEP_LATENT_STAGED, but no fused step staged a latent since the last sdeo_configure, or another "
                  "forward (sdeo_apply_model, sdeo_unet_forward, sdeo_controlnet_forward) overwrote it since (drop the flag)", who);
    if (x0_staged_for != x)
      return fail("%s: SDEO_STEP_LATENT_STAGED, but the previous fused step ran on another latent (%p; this one is %p; "
                  "drop the flag)", who, (const void*)x0_staged_for, (const void*)x);
    if (x0_staged_paired != paired)
      return fail("%s: SDEO_STEP_LATENT_STAGED, but the previous fused step was %s and staged its latent as such "
                  "(drop the flag)", who, x0_staged_paired ? "a CFG-pair step" : "an unguided step (SDEO_STEP_UNGUIDED)");
    return 0;
  }

  // a call that runs the UNet on a handle with the image-prompt adapter enabled (the caller asks only on such a handle)
  int ip_tokens(const char* who) const {
    if (!ip_set)
      return fail("%s: this handle has an image-prompt adapter (sdeo_enable_ip_adapter), but no image-prompt K / V since the last "
                  "sdeo_configure (call sdeo_set_ip_tokens)", who);
    return 0;
  }

  friend bool operator==(const CacheRecord& a, const CacheRecord& b) {
    for (int j = 0; j < kMaxNets; ++j)
      if (a.hint_set[j] != b.hint_set[j] || a.hint_stale[j] != b.hint_stale[j]) return false;
    return a.ctx_set == b.ctx_set && a.ctx_stale == b.ctx_stale && a.ctx_epoch == b.ctx_epoch && a.ctx_epoch_of[0] == b.ctx_epoch_of[0] &&
           a.ctx_epoch_of[1] == b.ctx_epoch_of[1] && a.x0_staged_for == b.x0_staged_for && a.x0_staged_paired == b.x0_staged_paired &&
           a.tab_count == b.tab_count && a.tab_stale == b.tab_stale && a.ip_set == b.ip_set;
  }
  friend bool operator!=(const CacheRecord& a, const CacheRecord& b) { return !(a == b); }

 private:
  //   hint_set[j]:      net j's hint block ran since the last sdeo_configure (net 0: a forward given the hint; j >= 1: sdeo_set_control_hint)
  //   ctx_set:          whose context K / V were computed since the last sdeo_configure (a set of Side)
  //   ctx_epoch:        advances every time a new context is staged; ctx_epoch_of[side] is the epoch side's K / V were computed from
  //   x0_staged_for:    the caller's latent whose updated fp16 copy the last fused step left in x0; null once anything else wrote x0
  //   x0_staged_paired: that step was a CFG-pair step (b = N / 2 latents, each staged twice), not an unguided one (N latents, once)
  //   tab_count:        rows of the timestep table sdeo_set_timestep_table filled since the last sdeo_configure
  //   *_stale:          sdeo_lora_commit changed the weights the item was computed with
  //   ip_set:           sdeo_set_ip_tokens filled the image-prompt K / V since the last sdeo_configure (adapter handles only)
  bool hint_set[kMaxNets] = {false};
  bool hint_stale[kMaxNets] = {false};
  int ctx_set = 0, ctx_stale = 0;
  unsigned long long ctx_epoch = 0, ctx_epoch_of[2] = {0, 0};
  const float* x0_staged_for = nullptr;
  bool x0_staged_paired = true;
  int tab_count = 0;
  bool tab_stale = false;
  bool ip_set = false;
};

}  // namespace sdeo
