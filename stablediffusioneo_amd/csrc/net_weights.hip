// Network executor of libsdeo, weights: the registry of the checkpoint tensors a handle expects, what it derives from the raw tensors
// at finalisation (LayerNorm folds, composed matrices, the fp8 and block-scaled packs) and the entry points that only touch weights.
#include "net_handle.h"

namespace {

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

}  // namespace

void sdeo::build_registry(Engine* e) {
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

// the extra control networks 1..count (sdeo_enable_extra_controlnets)
void sdeo::reg_extra_controlnets(Engine* e, int count) {
  Registry r{e};
  for (int j = 1; j <= count; ++j) reg_controlnet(r, 1 + j);
}

// VAE encoder (`model.py:452-545`, attn_resolutions = [], double_z) + quant_conv, appended behind everything build_registry placed
// (sdeo_enable_vae_encoder): the offsets of the existing tensors do not move
void sdeo::reg_vae_encoder(Engine* e) {
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

// Image-prompt adapter (sdeo_enable_ip_adapter): to_k_ip | to_v_ip of every UNet cross-attention, stacked as one [2c][ctx] matrix the
// way to_kv is, behind everything registered so far.  No fp8 region: fp8 handles refuse the adapter (sdeo_finalize_weights).
void sdeo::reg_ip_adapter(Engine* e) {
  Registry r{e};
  r.quant = false;
  const int ctx = e->cfg.context_dim;
  for_each_block(e->uplan, [&](const Blk& b) {
    if (b.kind != B_ATTN) return;
    const std::string t = std::string(NS_UNET) + b.name + ".transformer_blocks.0";
    const int c = b.cin;
    const size_t kv = r.take((size_t)2 * c * ctx * 2);
    e->named_off[t + ".attn2.to_kv_ip"] = kv;
    r.add(t + ".attn2.to_k_ip.weight", W_LINEAR, {c, ctx}, kv);
    r.add(t + ".attn2.to_v_ip.weight", W_LINEAR, {c, ctx}, kv + (size_t)c * ctx * 2);
  });
}

// the two tensors per cross-attention reg_ip_adapter registers
static bool is_ip_weight(const char* name) {
  const std::string n = name ? name : "";
  return n.find(".attn2.to_k_ip.") != std::string::npos || n.find(".attn2.to_v_ip.") != std::string::npos;
}

// what the three apply entry points share: the handle-level refusals, then `apply(not_ready)` on the store, then the byte count
template <class F>
static int adapter_apply(const char* who, sdeo_handle h, const char* name, F apply) {
  SDEO_CHECK(h, "%s: null handle", who);
  SDEO_CHECK(!is_ip_weight(name), "%s: %s belongs to the image-prompt adapter: adapters on the ip matrices are not supported "
             "(the cached image-prompt K / V rely on them never changing)", who, name);
  const char* not_ready = !h->finalized ? "weights not finalized (call sdeo_finalize_weights)"
                          : h->fp8.weight_bits == 8 ? "this handle holds fp8 weights (sdeo_set_weight_precision 8): its fp16 copies are the dequantised values, "
                                                      "not the raw ones, and adapters on it are not supported"
                                                    : nullptr;
  const size_t before = h->ws.lora_backup_bytes;
  const int rc = apply(not_ready);
  h->device_bytes += h->ws.lora_backup_bytes - before;
  return rc;
}

extern "C" {

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
  SDEO_CHECK(!(h->ip_tokens && h->fp8.weight_bits == 8),
             "sdeo_finalize_weights: fp8 weights (sdeo_set_weight_precision 8) are not supported together with the image-prompt adapter "
             "(sdeo_enable_ip_adapter)");
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

// ---- LoRA adapters: WeightStore does the work, the handle adds what it derives from the raw tensors and its caches
int sdeo_lora_apply(sdeo_handle h, const char* name, const float* down, const float* up, int rank, float scale, void* stream) {
  return adapter_apply("sdeo_lora_apply", h, name, [&](const char* not_ready) {
    return h->ws.lora_apply("sdeo_lora_apply", name, name ? name : "", down, up, rank, scale, not_ready, S(stream));
  });
}

int sdeo_loha_apply(sdeo_handle h, const char* name, const float* w1_a, const float* w1_b, const float* w2_a, const float* w2_b,
                    const float* t1, const float* t2, int rank, float scale, void* stream) {
  return adapter_apply("sdeo_loha_apply", h, name, [&](const char* not_ready) {
    return h->ws.loha_apply("sdeo_loha_apply", name, name ? name : "", w1_a, w1_b, w2_a, w2_b, t1, t2, rank, scale, not_ready, S(stream));
  });
}

int sdeo_lokr_apply(sdeo_handle h, const char* name, const float* w1, const float* w1_a, const float* w1_b, int rank1, const float* w2,
                    const float* w2_a, const float* w2_b, const float* t2, int rank2, int out_l, int in_m, float scale, void* stream) {
  return adapter_apply("sdeo_lokr_apply", h, name, [&](const char* not_ready) {
    return h->ws.lokr_apply("sdeo_lokr_apply", name, name ? name : "", w1, w1_a, w1_b, rank1, w2, w2_a, w2_b, t2, rank2, out_l, in_m, scale,
                            not_ready, S(stream));
  });
}

int sdeo_lora_commit(sdeo_handle h) {
  SDEO_CHECK(h, "sdeo_lora_commit: null handle");
  SDEO_CHECK(h->finalized, "sdeo_lora_commit: weights not finalized (call sdeo_finalize_weights)");
  h->ws.lora_release_stage();
  if (int rc = derive_weights(h)) return rc;
  h->cache.weights_changed();
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

}  // extern "C"
