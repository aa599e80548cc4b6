// Host-only checks of csrc/arena.h and csrc/net_plan.h (tests/test_arena_cpu.py builds this with -fsanitize=address,undefined and
// runs it):   arena_check <in_ch,...> <in_ds,...>     the two lists are spec.unet_plan(UNET_SD15)'s input_block_chans / input_block_ds.
// Prints one line per failed check and exits 1; exits 0 when every check holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../stablediffusioneo_amd/csrc/arena.h"
#include "../stablediffusioneo_amd/csrc/net_plan.h"

using namespace sdeo;

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

struct Lcg {      // the fixed pseudo-random sequence of every arena check
  uint64_t s = 0x5DE0A7E4A5EEDull;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

static bool same(const Arena& a, const Arena& b) {
  if (a.end != b.end || a.peak != b.peak || a.blocks.size() != b.blocks.size()) return false;
  for (size_t i = 0; i < a.blocks.size(); ++i)
    if (a.blocks[i].off != b.blocks[i].off || a.blocks[i].size != b.blocks[i].size || a.blocks[i].free != b.blocks[i].free) return false;
  return true;
}

// One step of the sequence on `a`: an alloc (sizes from 1 byte to ~1 MB, small ones more often) or the release of a live block.
// live: (offset, bytes asked for).  Returns the offset handed out, or the one released.
static size_t step(Arena& a, Lcg& r, std::vector<std::pair<size_t, size_t>>& live) {
  const uint32_t v = r.next();
  if (live.empty() || (v % 100 < 55 && live.size() < 200)) {
    const uint32_t bits = 4 + r.next() % 17;
    const size_t bytes = 1 + r.next() % (1u << bits);
    const size_t off = a.alloc(bytes);
    live.push_back({off, bytes});
    return off;
  }
  const size_t i = r.next() % live.size();
  const size_t off = live[i].first;
  a.release(off);
  live.erase(live.begin() + i);
  return off;
}

static void check_live(const Arena& a, std::vector<std::pair<size_t, size_t>> live, int call) {
  std::sort(live.begin(), live.end());
  for (size_t i = 0; i < live.size(); ++i) {
    CHECK(live[i].first % 256 == 0, "call %d: offset %zu is not a multiple of 256", call, live[i].first);
    CHECK(live[i].first + live[i].second <= a.end && a.end <= a.peak, "call %d: block %zu+%zu past end %zu / peak %zu", call,
          live[i].first, live[i].second, a.end, a.peak);
    if (i) CHECK(live[i - 1].first + live[i - 1].second <= live[i].first, "call %d: blocks %zu+%zu and %zu overlap", call,
                 live[i - 1].first, live[i - 1].second, live[i].first);
  }
}

static void check_arena() {
  const int kCalls = 10000, kMid = 5000;
  // (a) overlap / alignment after every call, (b) a second arena fed the same sequence, (c) a copy taken at kMid and replayed
  Arena a, twin, snap;
  Lcg ra, rt, rsnap;
  std::vector<std::pair<size_t, size_t>> la, lt, lsnap;
  std::vector<size_t> offs;
  for (int i = 0; i < kCalls; ++i) {
    if (i == kMid) { snap = a; rsnap = ra; lsnap = la; }
    offs.push_back(step(a, ra, la));
    check_live(a, la, i);
    const size_t ot = step(twin, rt, lt);
    CHECK(ot == offs.back() && twin.peak == a.peak, "call %d: the twin arena gives offset %zu peak %zu, the first %zu peak %zu", i, ot,
          twin.peak, offs.back(), a.peak);
  }
  CHECK(same(a, twin), "the twin arena ends in another state");
  CHECK(a.peak > (1u << 20) && la.size() > 10, "the sequence is too tame: peak %zu, %zu live blocks at the end", a.peak, la.size());
  for (int i = kMid; i < kCalls; ++i) {
    const size_t o = step(snap, rsnap, lsnap);
    CHECK(o == offs[i], "call %d replayed from the copy of call %d: offset %zu, originally %zu", i, kMid, o, offs[i]);
  }
  CHECK(same(a, snap), "the replayed copy ends in another state");
}

static void check_views() {
  // (d) a view is never owned, and the release path of the builder (T::release) gives nothing of it back
  Arena a;
  static f16 mem[4096];
  T t;
  t.n = 2; t.h = 3; t.w = 4; t.c = 40; t.ld = 40;
  t.off = a.alloc((size_t)t.rows() * t.c * 2);
  t.p = mem + t.off / 2;
  t.gnp_off = a.alloc(1024);
  float partials[1];
  t.gnp = partials; t.gn_slots = 3;
  const size_t other = a.alloc(512);
  CHECK(t.owned() && t.gn_reserved(), "an allocated tensor must own its blocks");
  T v = t.view(8, 16), whole = t.view();
  CHECK(!v.owned() && !whole.owned() && !v.gn_reserved() && !whole.gn_reserved(), "a view owns nothing");
  CHECK(v.p == t.p + 8 && v.c == 16 && v.ld == t.ld && v.n == t.n && v.h == t.h && v.w == t.w && v.rows() == t.rows(), "view(8, 16) geometry");
  CHECK(whole.p == t.p && whole.c == t.c && whole.ld == t.ld, "view() geometry");
  CHECK(v.gnp == nullptr && v.gn_slots == 0, "a view carries no GroupNorm partials");
  CHECK(!v.view(2, 4).owned() && v.view(2, 4).p == t.p + 10, "a view of a view");
  const Arena before = a;
  v.release(a);
  whole.release(a);
  CHECK(same(a, before), "releasing a view changed the arena");
  CHECK(!T().owned(), "a default tensor owns nothing");
  t.release(a);
  CHECK(!t.owned() && !t.gn_reserved() && t.gnp == nullptr, "a released tensor owns nothing");
  CHECK(a.blocks.size() == 2 && a.blocks[0].free && a.blocks[0].size == before.blocks[0].size + before.blocks[1].size && !a.blocks[1].free,
        "releasing the tensor frees and merges its two blocks");
  const Arena freed = a;
  t.release(a);
  CHECK(same(a, freed), "a second release changed the arena");
  a.release(other);
  CHECK(a.blocks.size() == 1 && a.blocks[0].free, "everything released: one free block");
}

static std::vector<int> int_list(const char* s) {
  std::vector<int> v;
  for (const char* p = s; *p;) {
    char* e = nullptr;
    v.push_back((int)strtol(p, &e, 10));
    p = *e == ',' ? e + 1 : e;
    if (e == p && *e) break;
  }
  return v;
}

static void check_plans(const std::vector<int>& want_ch, const std::vector<int>& want_ds) {
  // (e) SD-1.5 (cldm_v15.yaml): the block lists of the UNet and the ControlNet
  sdeo_config c = {};
  c.in_channels = 4; c.out_channels = 4; c.hint_channels = 3; c.model_channels = 320; c.num_res_blocks = 2;
  const int mult[4] = {1, 2, 4, 4}, ar[3] = {4, 2, 1};
  for (int i = 0; i < 4; ++i) c.channel_mult[i] = c.vae_ch_mult[i] = mult[i];
  for (int i = 0; i < 3; ++i) c.attention_resolutions[i] = ar[i];
  c.num_levels = 4; c.num_attention_resolutions = 3; c.num_heads = 8; c.context_dim = 768; c.context_len = 77;
  c.vae_ch = 128; c.vae_out_ch = 3; c.vae_num_levels = 4; c.vae_num_res_blocks = 2; c.vae_z_channels = 4; c.vae_scale_factor = 0.18215f;
  const UPlan u = make_uplan(c, true), cn = make_uplan(c, false);
  CHECK(u.in.size() == 12 && u.out.size() == 12 && u.mid.size() == 3, "UNet: %zu input, %zu output, %zu middle block lists", u.in.size(),
        u.out.size(), u.mid.size());
  CHECK(cn.in.size() == 12 && cn.out.empty(), "ControlNet: %zu input, %zu output block lists", cn.in.size(), cn.out.size());
  std::vector<int> controls = cn.in_ch;      // one zero conv per input block + middle_block_out
  controls.push_back(cn.in_ch.back());
  CHECK(controls.size() == 13, "%zu control channel counts", controls.size());
  CHECK(u.in_ch == want_ch && cn.in_ch == want_ch, "in_ch differs from input_block_chans (%zu vs %zu entries)", u.in_ch.size(), want_ch.size());
  CHECK(u.in_ds == want_ds && cn.in_ds == want_ds, "in_ds differs from input_block_ds (%zu vs %zu entries)", u.in_ds.size(), want_ds.size());
  for (size_t i = 0; i < cn.in.size() && i < u.in.size(); ++i)
    CHECK(u.in[i].back().cout == u.in_ch[i] && cn.in[i].size() == u.in[i].size(), "input block %zu: %d channels out, list says %d", i,
          u.in[i].back().cout, u.in_ch[i]);
  CHECK(u.out.back().back().cout == c.model_channels, "the decoder ends at %d channels", u.out.back().back().cout);
  int bin = 0;
  const std::vector<VLevel> lv = vae_levels(c, &bin);
  CHECK(bin == 512 && lv.size() == 4 && lv[0].up && !lv[3].up && lv[3].blocks.back().second == 128, "VAE levels");
  const std::vector<HintConv> hc = hint_convs(c);
  CHECK(hc.size() == 8 && hc[0].cin == 3 && hc[7].cout == 320 && hc[7].name == "input_hint_block.14", "hint convs");
}

int main(int argc, char** argv) {
  if (argc != 3) {
    printf("usage: arena_check <in_ch,...> <in_ds,...>\n");
    return 2;
  }
  check_arena();
  check_views();
  check_plans(int_list(argv[1]), int_list(argv[2]));
  if (g_failed) printf("%d checks failed\n", g_failed);
  else printf("arena_check: ok\n");
  return g_failed ? 1 : 0;
}
