// Architecture plans of the network executor (net_weights.hip, net_build.hip): the block lists of the UNet / ControlNet, the hint block and the VAE levels,
// mirror of stablediffusioneo_amd/spec.py (itself pinned to the reference constructors by tests/golden/manifest_sd15.json).
// Standard C++ only (no HIP include): tests/arena_check.cpp compares make_uplan with spec.unet_plan on the host.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/sdeo.h"

namespace sdeo {

static const char* const NS_UNET = "model.diffusion_model.";
static const char* const NS_CN = "control_model.";
static const char* const NS_VAE = "first_stage_model.";

enum BlkKind { B_CONV_IN, B_RES, B_ATTN, B_DOWN, B_UP };
struct Blk { BlkKind kind; std::string name; int cin, cout; int heads = 0; };      // heads: B_ATTN only (spec.Block.heads)
struct UPlan {
  std::vector<std::vector<Blk>> in, out;
  std::vector<Blk> mid;
  std::vector<int> in_ch, in_ds;
};

static inline bool in_list(const int* v, int n, int x) {
  for (int i = 0; i < n; ++i) if (v[i] == x) return true;
  return false;
}

// num_head_channels > 0: every attention block has ch / num_head_channels heads (`cldm/cldm.py:184-191`); else c.num_heads
static inline UPlan make_uplan(const sdeo_config& c, bool with_decoder, int num_head_channels = 0) {
  UPlan p;
  const int mc = c.model_channels;
  auto heads = [&](int ch) { return num_head_channels > 0 ? ch / num_head_channels : c.num_heads; };
  auto nm = [](const char* pre, int i, int j) { return std::string(pre) + "." + std::to_string(i) + "." + std::to_string(j); };
  p.in.push_back({{B_CONV_IN, "input_blocks.0.0", c.in_channels, mc}});
  p.in_ch.push_back(mc);
  p.in_ds.push_back(1);
  int ch = mc, ds = 1, idx = 1;
  for (int level = 0; level < c.num_levels; ++level) {
    const int mult = c.channel_mult[level];
    for (int r = 0; r < c.num_res_blocks; ++r) {
      std::vector<Blk> layers;
      layers.push_back({B_RES, nm("input_blocks", idx, 0), ch, mult * mc});
      ch = mult * mc;
      if (in_list(c.attention_resolutions, c.num_attention_resolutions, ds))
        layers.push_back({B_ATTN, nm("input_blocks", idx, 1), ch, ch, heads(ch)});
      p.in.push_back(layers);
      p.in_ch.push_back(ch);
      p.in_ds.push_back(ds);
      ++idx;
    }
    if (level != c.num_levels - 1) {
      p.in.push_back({{B_DOWN, nm("input_blocks", idx, 0), ch, ch}});
      p.in_ch.push_back(ch);
      ds *= 2;
      p.in_ds.push_back(ds);
      ++idx;
    }
  }
  p.mid = {{B_RES, "middle_block.0", ch, ch}, {B_ATTN, "middle_block.1", ch, ch, heads(ch)}, {B_RES, "middle_block.2", ch, ch}};
  if (!with_decoder) return p;
  std::vector<int> stack = p.in_ch;
  int oidx = 0;
  for (int level = c.num_levels - 1; level >= 0; --level) {
    const int mult = c.channel_mult[level];
    for (int i = 0; i <= c.num_res_blocks; ++i) {
      const int ich = stack.back();
      stack.pop_back();
      std::vector<Blk> layers;
      layers.push_back({B_RES, nm("output_blocks", oidx, 0), ch + ich, mc * mult});
      ch = mc * mult;
      if (in_list(c.attention_resolutions, c.num_attention_resolutions, ds))
        layers.push_back({B_ATTN, nm("output_blocks", oidx, 1), ch, ch, heads(ch)});
      if (level && i == c.num_res_blocks) {
        layers.push_back({B_UP, nm("output_blocks", oidx, (int)layers.size()), ch, ch});
        ds /= 2;
      }
      p.out.push_back(layers);
      ++oidx;
    }
  }
  return p;
}

template <class F>
static inline void for_each_block(const UPlan& p, F f) {      // in the order of a forward pass: input blocks, middle, output blocks
  for (auto& v : p.in) for (auto& b : v) f(b);
  for (auto& b : p.mid) f(b);
  for (auto& v : p.out) for (auto& b : v) f(b);
}

struct HintConv { std::string name; int cin, cout, stride; };
static inline std::vector<HintConv> hint_convs(const sdeo_config& c) {
  const int chans[8][3] = {{-1, 16, 1}, {16, 16, 1}, {16, 32, 2}, {32, 32, 1}, {32, 96, 2}, {96, 96, 1}, {96, 256, 2}, {256, -2, 1}};
  std::vector<HintConv> v;
  for (int i = 0; i < 8; ++i) {
    const int ci = chans[i][0] == -1 ? c.hint_channels : chans[i][0];
    const int co = chans[i][1] == -2 ? c.model_channels : chans[i][1];
    v.push_back({"input_hint_block." + std::to_string(2 * i), ci, co, chans[i][2]});
  }
  return v;
}

struct VLevel { int level; std::vector<std::pair<int, int>> blocks; bool up; };
static inline std::vector<VLevel> vae_levels(const sdeo_config& c, int* block_in_out) {
  const int nl = c.vae_num_levels;
  int bi = c.vae_ch * c.vae_ch_mult[nl - 1];
  *block_in_out = bi;
  std::vector<VLevel> v;
  for (int l = nl - 1; l >= 0; --l) {
    const int bo = c.vae_ch * c.vae_ch_mult[l];
    VLevel L{l, {}, l != 0};
    for (int j = 0; j <= c.vae_num_res_blocks; ++j) { L.blocks.push_back({bi, bo}); bi = bo; }
    v.push_back(L);
  }
  return v;
}

}  // namespace sdeo
