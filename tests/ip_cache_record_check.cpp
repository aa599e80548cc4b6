// Host-only checks of the fifth item of the cache contract, the image-prompt K / V of a handle with sdeo_enable_ip_adapter
// (csrc/cache_record.h; include/sdeo.h, "State a handle keeps between calls").  tests/test_ip_cache_record_cpu.py builds this with
// -fsanitize=address,undefined and runs it, like tests/cache_record_check.cpp, which checks the four other items and stays as it is.
// The message below is restated from the library, whole.  Prints one line per failed check and exits 1; exits 0 when every check holds.
#include <stdarg.h>
#include <stdio.h>

#include <functional>
#include <string>

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

#define M_IP_UNSET "%s: this handle has an image-prompt adapter (sdeo_enable_ip_adapter), but no image-prompt K / V since the last sdeo_configure (call sdeo_set_ip_tokens)"

// the readers of the item: every entry point that runs the UNet
static const char* const kReaders[] = {"sdeo_unet_forward", "sdeo_apply_model", "sdeo_ddim_step", "sdeo_dpmpp_2m_step", "sdeo_ddim_step_masked",
                                       "sdeo_dpmpp_2m_step_masked", "sdeo_ddim_step_eta", "sdeo_dpmpp_2m_sde_step"};

static std::string unset_message(const char* who) {
  char buf[1024];
  snprintf(buf, sizeof(buf), M_IP_UNSET, who);
  return buf;
}

static void all_accepted(const CacheRecord& r, const char* what) {
  for (const char* who : kReaders) {
    const CacheRecord before = r;
    g_msg.clear();
    CHECK(r.ip_tokens(who) == 0, "%s: %s refused with '%s'", what, who, g_msg.c_str());
    CHECK(r == before, "%s: an accepted check changed the record", what);
  }
}
static void all_refused(const CacheRecord& r, const char* what) {
  for (const char* who : kReaders) {
    const CacheRecord before = r;
    g_msg.clear();
    CHECK(r.ip_tokens(who) != 0, "%s: %s accepted", what, who);
    CHECK(g_msg == unset_message(who), "%s: refused with\n  '%s', expected\n  '%s'", what, g_msg.c_str(), unset_message(who).c_str());
    CHECK(r == before, "%s: a refused check changed the record", what);
  }
}

static float g_latent;
static const int B = CacheRecord::BOTH;

// the four other items filled, as tests/cache_record_check.cpp fills them
static CacheRecord others_filled() {
  CacheRecord r;
  r.configured_anew();
  for (int j = 0; j <= 2; ++j) r.hint_filled(j);
  r.context_staging(B);
  r.context_filled(B);
  r.table_refilling();
  r.table_filled(20);
  r.step_launching();
  r.step_succeeded(&g_latent, true);
  return r;
}
// what the readers of the four other items say
static void others_accepted(const CacheRecord& r, const char* what) {
  g_msg.clear();
  CHECK(r.cached_reads("who", 0, B) == 0 && r.extra_hints("who", 2) == 0 && r.step_table_row("who", 5) == 0 && r.table_row("who", 5) == 0 &&
            r.staged_latent("who", &g_latent, true) == 0 && r.net_has_hint("who", 1) == 0,
        "%s: a reader of another item is refused with '%s'", what, g_msg.c_str());
}

int main() {
  // a fresh record, and a configured one: nothing filled
  all_refused(CacheRecord(), "fresh record");
  {
    CacheRecord r;
    r.configured_anew();
    all_refused(r, "after sdeo_configure");
  }
  // filled by sdeo_set_ip_tokens: every reader accepted; cleared by sdeo_configure: refused with the whole message
  {
    CacheRecord r = others_filled();
    all_refused(r, "the other items filled, this one not");
    const CacheRecord without = r;
    r.ip_staging();
    CHECK(r == without, "ip_staging on an unset item changed the record");
    all_refused(r, "staged, the program has not run yet");
    r.ip_filled();
    CHECK(r != without, "operator== does not see the image-prompt item");
    all_accepted(r, "after sdeo_set_ip_tokens");
    others_accepted(r, "after sdeo_set_ip_tokens");
    // a refill passes through unset (a failed launch leaves it there)
    r.ip_staging();
    all_refused(r, "refill under way");
    CHECK(r == without, "ip_staging did not return the record to the unfilled one");
    r.ip_filled();
    all_accepted(r, "refilled");
    // sdeo_lora_commit / sdeo_lora_clear: the item stays as it was, the others go stale
    const CacheRecord filled = r;
    r.weights_changed();
    all_accepted(r, "after sdeo_lora_commit");
    CHECK(r != filled, "weights_changed left the other items alone");
    CHECK(r.cached_reads("who", 0, B) != 0, "weights_changed: the cached context is still accepted");
    // ... and an unset item stays unset under it
    CacheRecord u = without;
    u.weights_changed();
    all_refused(u, "unset, after sdeo_lora_commit");
    // every other transition leaves it as it was
    r = filled;
    r.hint_filled(1);
    r.context_staging(B);
    r.context_filled(B);
    r.latent_overwritten();
    r.step_launching();
    r.step_succeeded(&g_latent, false);
    r.table_refilling();
    r.table_filled(7);
    all_accepted(r, "after the transitions of the other items");
    r.configured_anew();
    all_refused(r, "after sdeo_configure (was filled)");
    CHECK(r.cached_reads("who", 0, B) != 0 && r.step_table_row("who", 0) != 0, "configured_anew kept another item");
  }
  // the new transitions leave the four other items as they were: equal records stay equal in everything but this item
  {
    CacheRecord a = others_filled(), b = others_filled();
    CHECK(a == b, "two records filled alike differ");
    a.ip_staging();
    a.ip_filled();
    others_accepted(a, "ip_filled");
    CHECK(a != b, "ip_filled is invisible to operator==");
    a.ip_staging();
    CHECK(a == b, "ip_staging / ip_filled touched another item");
    others_accepted(a, "ip_staging");
    // stale items stay stale, unset ones unset
    CacheRecord s = others_filled();
    s.weights_changed();
    const CacheRecord stale = s;
    s.ip_staging();
    s.ip_filled();
    s.ip_staging();
    CHECK(s == stale, "the image-prompt transitions changed a stale bit");
    CHECK(s.cached_reads("who", 0, B) != 0 && s.extra_hints("who", 2) != 0 && s.step_table_row("who", 5) != 0,
          "the image-prompt transitions refreshed a stale item");
  }
  if (g_failed) {
    printf("ip_cache_record_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("ip_cache_record_check: ok\n");
  return 0;
}
