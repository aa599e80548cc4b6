// Host-only checks of csrc/cache_record.h, the cache contract of a handle (include/sdeo.h, "State a handle keeps between calls").
// tests/test_cache_record_cpu.py builds this with -fsanitize=address,undefined and runs it.  The messages below are restated from the
// library, whole, so that a change of one of them shows here as well as in tests/test_cache_contract_gpu.py.
// Prints one line per failed check and exits 1; exits 0 when every check holds.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

#include "../stablediffusioneo_amd/csrc/cache_record.h"

using sdeo::CacheRecord;

static std::string g_msg;      // what the last failed check reported
int sdeo::fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_msg = buf;
  return 1;
}

__attribute__((format(printf, 1, 2))) static std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

static int g_failed = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      if (++g_failed <= 20) {              \
        printf("FAILED %s: ", #cond);      \
        printf(__VA_ARGS__);               \
        printf("\n");                      \
      }                                    \
    }                                      \
  } while (0)

// ---- the library's messages
#define M_HINT_STALE "%s: SDEO_HINT_CACHED, but sdeo_lora_commit changed the weights the cached hint features of control network %d were computed with (pass the hint again)"
#define M_CTX_STALE "%s: SDEO_CONTEXT_CACHED, but sdeo_lora_commit changed the weights the cached context K / V were computed with (pass the context again)"
#define M_HINT_UNSET "%s: SDEO_HINT_CACHED, but control network %d has no hint since the last sdeo_configure (%s)"
#define M_HINT_UNSET_0 "pass the hint to sdeo_apply_model or sdeo_controlnet_forward"
#define M_HINT_UNSET_J "call sdeo_set_control_hint"
#define M_CTX_UNSET_U "%s: SDEO_CONTEXT_CACHED, but the UNet has no context K / V since the last sdeo_configure (pass the context to sdeo_apply_model or sdeo_unet_forward)"
#define M_CTX_UNSET_C "%s: SDEO_CONTEXT_CACHED, but the control networks have no context K / V since the last sdeo_configure (pass the context to sdeo_apply_model or sdeo_controlnet_forward)"
#define M_CTX_EPOCH "%s: SDEO_CONTEXT_CACHED, but the cached context K / V of the UNet and of the control networks were computed from different contexts (a call that refreshes one side only ran since: sdeo_unet_forward, sdeo_controlnet_forward or SDEO_NO_CONTROL; pass the context to sdeo_apply_model again)"
#define M_NET_NO_HINT "%s: control network %d has no hint since the last sdeo_configure"
#define M_EXTRA_UNSET "%s: control network %d has no hint since the last sdeo_configure (call sdeo_set_control_hint(h, %d, ...))"
#define M_EXTRA_STALE "%s: sdeo_lora_commit changed the weights the cached hint features of control network %d were computed with (call sdeo_set_control_hint(h, %d, ...) again)"
#define M_ROW "%s: timestep row %d, but the table holds %d (sdeo_set_timestep_table)"
#define M_ROW_STALE "%s: SDEO_TIMESTEP_ROW, but sdeo_lora_commit changed the weights the timestep table was computed with (call sdeo_set_timestep_table again)"
#define M_STEP_ROW_STALE "%s: sdeo_lora_commit changed the weights the timestep table was computed with (call sdeo_set_timestep_table again)"
#define M_STAGED_NONE "%s: SDEO_STEP_LATENT_STAGED, but no fused step staged a latent since the last sdeo_configure, or another forward (sdeo_apply_model, sdeo_unet_forward, sdeo_controlnet_forward) overwrote it since (drop the flag)"
#define M_STAGED_OTHER "%s: SDEO_STEP_LATENT_STAGED, but the previous fused step ran on another latent (%p; this one is %p; drop the flag)"
#define M_STAGED_KIND "%s: SDEO_STEP_LATENT_STAGED, but the previous fused step was %s and staged its latent as such (drop the flag)"

typedef std::function<int(const CacheRecord&)> Check;

// a check on r is accepted; or refused with exactly `want`, leaving r equal to its copy taken before
static void accepted(const CacheRecord& r, const Check& c, const char* what) {
  const CacheRecord before = r;
  g_msg.clear();
  const int rc = c(r);
  CHECK(rc == 0, "%s: refused with '%s'", what, g_msg.c_str());
  CHECK(r == before, "%s: an accepted check changed the record", what);
}
static void refused(const CacheRecord& r, const Check& c, const std::string& want, const char* what) {
  const CacheRecord before = r;
  g_msg.clear();
  const int rc = c(r);
  CHECK(rc != 0, "%s: accepted, expected '%s'", what, want.c_str());
  CHECK(g_msg == want, "%s: refused with\n  '%s', expected\n  '%s'", what, g_msg.c_str(), want.c_str());
  CHECK(r == before, "%s: a refused check changed the record", what);
}

static float g_latents[3];
static const float* const X = &g_latents[0];
static const float* const Y = &g_latents[1];
static const int kExtra = 2, kRows = 20, kRow = 5;
static const int U = CacheRecord::UNET, C = CacheRecord::CONTROL, B = CacheRecord::BOTH;

static void fill_context(CacheRecord& r, int sides) { r.context_staging(sides); r.context_filled(sides); }
static void fill_table(CacheRecord& r, int rows) { r.table_refilling(); r.table_filled(rows); }
static void run_step(CacheRecord& r, const float* x, bool paired) { r.step_launching(); r.step_succeeded(x, paired); }

// every item filled: a configured handle with kExtra extra control networks after sdeo_set_control_hint, one sdeo_apply_model with
// control, sdeo_set_timestep_table and one fused CFG-pair step on X
static CacheRecord filled() {
  CacheRecord r;
  r.configured_anew();
  for (int j = 0; j <= kExtra; ++j) r.hint_filled(j);
  fill_context(r, B);
  fill_table(r, kRows);
  run_step(r, X, true);
  return r;
}

// ---- the table of include/sdeo.h, row by row
enum Item { HINT0, HINT1, CTX_U, CTX_C, TAB, STAGED, ITEMS };
enum Effect { KEEP, UNSET, STALE };
struct Reader { Item item; const char* name; Check check; std::string unset, stale; };      // stale empty: the reader does not look
struct Transition { const char* name; std::function<void(CacheRecord&)> apply; Effect on[ITEMS]; };

static void check_table() {
  const char* who = "sdeo_apply_model";
  const char* step = "sdeo_ddim_step";
  const std::vector<Reader> readers = {
      {HINT0, "SDEO_HINT_CACHED, net 0", [=](const CacheRecord& r) { return r.cached_reads(who, 0, 0); },
       fmt(M_HINT_UNSET, who, 0, M_HINT_UNSET_0), fmt(M_HINT_STALE, who, 0)},
      {HINT1, "SDEO_HINT_CACHED, net 1", [=](const CacheRecord& r) { return r.cached_reads("sdeo_controlnet_forward_net", 1, 0); },
       fmt(M_HINT_UNSET, "sdeo_controlnet_forward_net", 1, M_HINT_UNSET_J), fmt(M_HINT_STALE, "sdeo_controlnet_forward_net", 1)},
      {HINT1, "net 1 has a hint", [=](const CacheRecord& r) { return r.net_has_hint("sdeo_controlnet_forward_net", 1); },
       fmt(M_NET_NO_HINT, "sdeo_controlnet_forward_net", 1), ""},
      {HINT1, "every extra net has a hint", [=](const CacheRecord& r) { return r.extra_hints(step, kExtra); },
       fmt(M_EXTRA_UNSET, step, 1, 1), fmt(M_EXTRA_STALE, step, 1, 1)},
      {CTX_U, "SDEO_CONTEXT_CACHED, the UNet", [=](const CacheRecord& r) { return r.cached_reads("sdeo_unet_forward", -1, U); },
       fmt(M_CTX_UNSET_U, "sdeo_unet_forward"), fmt(M_CTX_STALE, "sdeo_unet_forward")},
      {CTX_C, "SDEO_CONTEXT_CACHED, the control networks", [=](const CacheRecord& r) { return r.cached_reads("sdeo_controlnet_forward", -1, C); },
       fmt(M_CTX_UNSET_C, "sdeo_controlnet_forward"), fmt(M_CTX_STALE, "sdeo_controlnet_forward")},
      {TAB, "SDEO_TIMESTEP_ROW", [=](const CacheRecord& r) { return r.table_row(who, kRow); }, fmt(M_ROW, who, kRow, 0), fmt(M_ROW_STALE, who)},
      {TAB, "table_row of a step", [=](const CacheRecord& r) { return r.step_table_row(step, kRow); }, fmt(M_ROW, step, kRow, 0),
       fmt(M_STEP_ROW_STALE, step)},
      {STAGED, "SDEO_STEP_LATENT_STAGED", [=](const CacheRecord& r) { return r.staged_latent(step, X, true); }, fmt(M_STAGED_NONE, step), ""},
  };
  const std::vector<Transition> transitions = {
      //                                                                           HINT0  HINT1  CTX_U  CTX_C  TAB    STAGED
      {"sdeo_configure", [](CacheRecord& r) { r.configured_anew(); },             {UNSET, UNSET, UNSET, UNSET, UNSET, UNSET}},
      {"sdeo_lora_commit", [](CacheRecord& r) { r.weights_changed(); },           {STALE, STALE, STALE, STALE, STALE, KEEP}},
      {"hint of net 0", [](CacheRecord& r) { r.hint_filled(0); },                 {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"hint of net 1", [](CacheRecord& r) { r.hint_filled(1); },                 {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"hint of net 2", [](CacheRecord& r) { r.hint_filled(2); },                 {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"context, both sides", [](CacheRecord& r) { fill_context(r, B); },         {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"context, the UNet", [](CacheRecord& r) { fill_context(r, U); },           {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"context, the control networks", [](CacheRecord& r) { fill_context(r, C); }, {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"context of the UNet, failed launch", [](CacheRecord& r) { r.context_staging(U); }, {KEEP, KEEP, UNSET, KEEP, KEEP, KEEP}},
      {"context of the control networks, failed launch", [](CacheRecord& r) { r.context_staging(C); }, {KEEP, KEEP, KEEP, UNSET, KEEP, KEEP}},
      {"a plain forward's latent", [](CacheRecord& r) { r.latent_overwritten(); }, {KEEP, KEEP, KEEP, KEEP, KEEP, UNSET}},
      {"a fused step that failed", [](CacheRecord& r) { r.step_launching(); },    {KEEP, KEEP, KEEP, KEEP, KEEP, UNSET}},
      {"a fused step on X", [](CacheRecord& r) { run_step(r, X, true); },         {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"sdeo_set_timestep_table", [](CacheRecord& r) { fill_table(r, kRows); },   {KEEP, KEEP, KEEP, KEEP, KEEP, KEEP}},
      {"sdeo_set_timestep_table, failed launch", [](CacheRecord& r) { r.table_refilling(); }, {KEEP, KEEP, KEEP, KEEP, UNSET, KEEP}},
  };
  const CacheRecord full = filled();
  for (const Reader& rd : readers) accepted(full, rd.check, rd.name);
  for (const Transition& t : transitions) {
    CacheRecord r = full;
    t.apply(r);
    for (const Reader& rd : readers) {
      const std::string what = std::string(rd.name) + " after " + t.name;
      const Effect e = t.on[rd.item];
      if (e == KEEP || (e == STALE && rd.stale.empty())) accepted(r, rd.check, what.c_str());
      else refused(r, rd.check, e == UNSET ? rd.unset : rd.stale, what.c_str());
    }
    // ... and the transition that fills the item makes its readers accepted again
    CacheRecord again = r;
    for (int j = 0; j <= kExtra; ++j) again.hint_filled(j);
    fill_context(again, B);
    fill_table(again, kRows);
    run_step(again, X, true);
    for (const Reader& rd : readers) accepted(again, rd.check, (std::string(rd.name) + " refilled after " + t.name).c_str());
  }
  // a fresh record holds nothing; the readers of a forward that brought its own inputs are accepted all the same
  CacheRecord fresh;
  for (const Reader& rd : readers) refused(fresh, rd.check, rd.unset, (std::string(rd.name) + " on a fresh record").c_str());
  accepted(fresh, [=](const CacheRecord& r) { return r.cached_reads(who, -1, 0); }, "no cached read on a fresh record");
  accepted(fresh, [=](const CacheRecord& r) { return r.table_row(who, -1); }, "timesteps given on a fresh record");
  accepted(fresh, [=](const CacheRecord& r) { return r.extra_hints(who, 0); }, "no extra nets on a fresh record");
  CacheRecord stale = full;
  stale.weights_changed();
  accepted(stale, [=](const CacheRecord& r) { return r.table_row(who, -1); }, "timesteps given under a stale table");
  // the rows of the table: [0, count) of the last fill
  refused(full, [=](const CacheRecord& r) { return r.table_row(who, kRows); }, fmt(M_ROW, who, kRows, kRows), "row == count");
  refused(full, [=](const CacheRecord& r) { return r.step_table_row(step, kRows); }, fmt(M_ROW, step, kRows, kRows), "step row == count");
  refused(full, [=](const CacheRecord& r) { return r.step_table_row(step, -1); }, fmt(M_ROW, step, -1, kRows), "step row -1");
  accepted(full, [=](const CacheRecord& r) { return r.step_table_row(step, kRows - 1); }, "step row count - 1");
  CacheRecord shorter = full;
  fill_table(shorter, 3);
  refused(shorter, [=](const CacheRecord& r) { return r.table_row(who, kRow); }, fmt(M_ROW, who, kRow, 3), "a shorter table");
  // filling net 1's hint does not fill net 2's, and the order of extra_hints: every "no hint" before any "stale"
  CacheRecord one = full;
  one.configured_anew();
  one.hint_filled(1);
  refused(one, [=](const CacheRecord& r) { return r.extra_hints(step, kExtra); }, fmt(M_EXTRA_UNSET, step, 2, 2), "net 2 unset");
  accepted(one, [=](const CacheRecord& r) { return r.extra_hints(step, 1); }, "one extra net");
  one.weights_changed();      // net 1 set and stale, net 2 unset and stale
  refused(one, [=](const CacheRecord& r) { return r.extra_hints(step, kExtra); }, fmt(M_EXTRA_UNSET, step, 2, 2), "unset before stale over j");
  one.hint_filled(2);
  refused(one, [=](const CacheRecord& r) { return r.extra_hints(step, kExtra); }, fmt(M_EXTRA_STALE, step, 1, 1), "net 1 stale");
  one.hint_filled(1);
  accepted(one, [=](const CacheRecord& r) { return r.extra_hints(step, kExtra); }, "both extra nets refilled");
  // the order inside cached_reads, from the last check to the first
  CacheRecord o = full;
  const Check all = [=](const CacheRecord& r) { return r.cached_reads(who, 0, B); };
  fill_context(o, U);
  refused(o, all, fmt(M_CTX_EPOCH, who), "epoch mismatch alone");
  o.configured_anew();
  o.hint_filled(0);
  fill_context(o, U);
  refused(o, all, fmt(M_CTX_UNSET_C, who), "control-net context unset before the epochs");
  o.configured_anew();
  o.hint_filled(0);
  refused(o, all, fmt(M_CTX_UNSET_U, who), "UNet context unset before the control networks'");
  o.configured_anew();
  refused(o, all, fmt(M_HINT_UNSET, who, 0, M_HINT_UNSET_0), "hint unset before the contexts");
  o.weights_changed();
  refused(o, all, fmt(M_HINT_STALE, who, 0), "hint stale first");
  o.hint_filled(0);
  refused(o, all, fmt(M_CTX_STALE, who), "context stale before anything unset");
  fill_context(o, U);
  refused(o, all, fmt(M_CTX_STALE, who), "one side still stale");
  accepted(o, [=](const CacheRecord& r) { return r.cached_reads(who, -1, U); }, "the refilled side alone");
  fill_context(o, B);
  accepted(o, all, "everything refilled");
}

// ---- the epoch rule
static void check_epochs() {
  const char* who = "sdeo_ddim_step";
  const Check both = [=](const CacheRecord& r) { return r.cached_reads(who, -1, B); };
  const Check unet = [=](const CacheRecord& r) { return r.cached_reads(who, -1, U); };
  const Check cn = [=](const CacheRecord& r) { return r.cached_reads(who, -1, C); };
  CacheRecord r;
  r.configured_anew();
  fill_context(r, B);
  accepted(r, both, "both sides from one staging");
  for (int side : {U, C}) {
    fill_context(r, side);
    refused(r, both, fmt(M_CTX_EPOCH, who), "one side refilled alone");
    accepted(r, unet, "the UNet's side after a one-sided refill");
    accepted(r, cn, "the control networks' side after a one-sided refill");
    // refilling the other side alone gives it yet another context
    fill_context(r, B & ~side);
    refused(r, both, fmt(M_CTX_EPOCH, who), "the other side refilled alone");
    fill_context(r, B);
    accepted(r, both, "a both-sides refill");
  }
  // the epochs outlive a new configuration (the set flags refuse first)
  fill_context(r, U);
  r.configured_anew();
  refused(r, both, fmt(M_CTX_UNSET_U, who), "new configuration");
  fill_context(r, B);
  accepted(r, both, "both sides staged anew");
}

// ---- the staged latent
static void check_staged() {
  const char* who = "sdeo_dpmpp_2m_step";
  const auto staged = [=](const float* x, bool paired) { return Check([=](const CacheRecord& r) { return r.staged_latent(who, x, paired); }); };
  for (bool paired : {true, false}) {
    CacheRecord r;
    r.configured_anew();
    refused(r, staged(X, paired), fmt(M_STAGED_NONE, who), "nothing staged yet");
    run_step(r, X, paired);
    accepted(r, staged(X, paired), "the recorded pointer and kind");
    refused(r, staged(Y, paired), fmt(M_STAGED_OTHER, who, (const void*)X, (const void*)Y), "another pointer");
    refused(r, staged(X, !paired), fmt(M_STAGED_KIND, who, paired ? "a CFG-pair step" : "an unguided step (SDEO_STEP_UNGUIDED)"), "the other kind");
    refused(r, staged(Y, !paired), fmt(M_STAGED_OTHER, who, (const void*)X, (const void*)Y), "another pointer before the other kind");
    run_step(r, Y, !paired);
    accepted(r, staged(Y, !paired), "the next step's pointer and kind");
    refused(r, staged(X, paired), fmt(M_STAGED_OTHER, who, (const void*)Y, (const void*)X), "the step before the last");
    CacheRecord a = r, b = r, c = r;
    a.latent_overwritten();
    refused(a, staged(Y, !paired), fmt(M_STAGED_NONE, who), "latent overwritten");
    b.step_launching();
    refused(b, staged(Y, !paired), fmt(M_STAGED_NONE, who), "about to launch without succeeded");
    c.configured_anew();
    refused(c, staged(Y, !paired), fmt(M_STAGED_NONE, who), "a new configuration");
  }
}

// ---- stale against unset: sdeo_lora_commit, then sdeo_configure
static void check_stale_then_unset() {
  const char* who = "sdeo_apply_model";
  CacheRecord r = filled();
  r.weights_changed();
  r.configured_anew();
  refused(r, [=](const CacheRecord& q) { return q.cached_reads(who, 0, 0); }, fmt(M_HINT_STALE, who, 0), "hint: stale, not unset");
  refused(r, [=](const CacheRecord& q) { return q.cached_reads(who, 1, 0); }, fmt(M_HINT_STALE, who, 1), "hint of net 1: stale, not unset");
  refused(r, [=](const CacheRecord& q) { return q.cached_reads(who, -1, U); }, fmt(M_CTX_STALE, who), "UNet context: stale, not unset");
  refused(r, [=](const CacheRecord& q) { return q.cached_reads(who, -1, C); }, fmt(M_CTX_STALE, who), "control-net context: stale, not unset");
  // (extra_hints and the table report what they look at first: the missing hint, the empty table)
  refused(r, [=](const CacheRecord& q) { return q.extra_hints(who, kExtra); }, fmt(M_EXTRA_UNSET, who, 1, 1), "extra hints: unset first");
  refused(r, [=](const CacheRecord& q) { return q.table_row(who, kRow); }, fmt(M_ROW, who, kRow, 0), "table: empty first");
  CacheRecord same = r;
  same.configured_anew();
  CHECK(same == r, "a second configuration changes nothing more");
  CHECK(r != filled() && CacheRecord() == CacheRecord(), "operator==");
}

// ---- a long random walk against a model of what each cache holds
struct Lcg {
  uint64_t s = 0x5DE0CAC4EC0DEull;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

struct Model {       // what each cache holds: the number of the input it was last filled from (0: nothing), and whether it is stale
  int hint[CacheRecord::kMaxNets] = {0};
  bool hint_stale[CacheRecord::kMaxNets] = {false};
  int ctx[2] = {0, 0};
  bool ctx_stale[2] = {false, false};
  int staging = 0;                 // the number of the context staged last
  int tab = 0;                     // rows
  bool tab_stale = false;
  const float* staged = nullptr;
  bool staged_paired = true;
  int inputs = 0;

  bool hint_ok(int j) const { return hint[j] && !hint_stale[j]; }
  bool reads_ok(int hint_net, int sides) const {
    if (hint_net >= 0 && !hint_ok(hint_net)) return false;
    for (int s = 0; s < 2; ++s) if ((sides >> s & 1) && (!ctx[s] || ctx_stale[s])) return false;
    return sides != 3 || ctx[0] == ctx[1];
  }
  bool extra_ok(int extra) const {
    for (int j = 1; j <= extra; ++j) if (!hint_ok(j)) return false;
    return true;
  }
};

static std::vector<int> walk(CacheRecord& r, int steps) {
  Lcg g;
  Model m;
  std::vector<int> outcomes;
  const auto expect = [&](int rc, bool ok, const char* what, int i) {
    CHECK((rc == 0) == ok, "step %d: %s %s, the model says %s ('%s')", i, what, rc ? "refused" : "accepted", ok ? "accepted" : "refused",
          g_msg.c_str());
    outcomes.push_back(rc);
  };
  for (int i = 0; i < steps; ++i) {
    const uint32_t v = g.next() % 100, a = g.next(), b = g.next();
    const CacheRecord before = r;
    bool is_check = true;
    if (v < 12) expect(r.cached_reads("w", (int)(a % 5) - 1, (int)(b % 4)), m.reads_ok((int)(a % 5) - 1, (int)(b % 4)), "cached_reads", i);
    else if (v < 18) expect(r.extra_hints("w", (int)(a % 4)), m.extra_ok((int)(a % 4)), "extra_hints", i);
    else if (v < 22) expect(r.net_has_hint("w", 1 + (int)(a % 3)), m.hint[1 + a % 3] != 0, "net_has_hint", i);
    else if (v < 30) { const int row = (int)(a % 12) - 1; expect(r.table_row("w", row), row < m.tab && (row < 0 || !m.tab_stale), "table_row", i); }
    else if (v < 38) { const int row = (int)(a % 12) - 1; expect(r.step_table_row("w", row), row >= 0 && row < m.tab && !m.tab_stale, "step_table_row", i); }
    else if (v < 48) {
      const float* x = &g_latents[a % 3]; const bool paired = b & 1;
      expect(r.staged_latent("w", x, paired), m.staged == x && m.staged_paired == paired, "staged_latent", i);
    } else {
      is_check = false;
      if (v < 52) {
        r.configured_anew();
        for (int& h : m.hint) h = 0;
        m.ctx[0] = m.ctx[1] = 0; m.tab = 0; m.staged = nullptr;
      } else if (v < 62) {
        const int j = a % 4;
        r.hint_filled(j);
        m.hint[j] = ++m.inputs; m.hint_stale[j] = false;
      } else if (v < 74) {
        const int sides = 1 + a % 3;
        r.context_staging(sides);
        m.staging = ++m.inputs;
        for (int s = 0; s < 2; ++s) if (sides >> s & 1) m.ctx[s] = 0;
        if (b % 8) {             // (else: a context program failed)
          r.context_filled(sides);
          for (int s = 0; s < 2; ++s) if (sides >> s & 1) { m.ctx[s] = m.staging; m.ctx_stale[s] = false; }
        }
      } else if (v < 78) {
        r.latent_overwritten();
        m.staged = nullptr;
      } else if (v < 88) {
        r.step_launching();
        m.staged = nullptr;
        if (b % 8) {             // (else: a launch of the step failed)
          const float* x = &g_latents[a % 3];
          r.step_succeeded(x, (a >> 8) & 1);
          m.staged = x; m.staged_paired = (a >> 8) & 1;
        }
      } else if (v < 96) {
        r.table_refilling();
        m.tab = 0;
        if (b % 8) {
          const int rows = 1 + a % 10;
          r.table_filled(rows);
          m.tab = rows; m.tab_stale = false;
        }
      } else {
        r.weights_changed();
        for (bool& s : m.hint_stale) s = true;
        m.ctx_stale[0] = m.ctx_stale[1] = m.tab_stale = true;
      }
    }
    if (is_check) CHECK(r == before, "step %d: a check changed the record", i);
  }
  return outcomes;
}

static void check_walk() {
  const int kSteps = 20000;
  CacheRecord a, b;
  const std::vector<int> oa = walk(a, kSteps), ob = walk(b, kSteps);
  CHECK(oa == ob && a == b, "the same walk twice ends in another state or gives other outcomes");
  size_t refusals = 0;
  for (int rc : oa) refusals += rc != 0;
  CHECK(oa.size() > 5000 && refusals > 1000 && oa.size() - refusals > 1000, "the walk is too tame: %zu checks, %zu refused", oa.size(), refusals);
}

int main() {
  check_table();
  check_epochs();
  check_staged();
  check_stale_then_unset();
  check_walk();
  if (g_failed) printf("%d checks failed\n", g_failed);
  else printf("cache_record_check: ok\n");
  return g_failed ? 1 : 0;
}
