"""Architecture restatement of the CNSD hot path: configuration, parameter inventory and
seeded synthetic weights.

The reference builds its networks by running nn.Module constructors; the checkpoint key names
and tensor shapes that fall out of those constructors are the on-disk contract
(`cldm/model.py:12-21` loads a flat state dict).  This module restates that contract as data:

* `UNET_SD15` / `VAE_SD15`  -- the SD-1.5 + ControlNet-1.0 configuration.  `models/cldm_v15.yaml`
  is absent from the reference tree; the values are the ones the in-repo
  evidence requires (`export_onnx_all.py:242-256`, `Engine.py:55-91`).
* `unet_plan` / `controlnet_plan` / `vae_plan` -- block lists mirroring the constructor loops of
  `ldm/modules/diffusionmodules/openaimodel.py:544-732`, `cldm/cldm.py:131-279` and
  `ldm/modules/diffusionmodules/model.py:546-616`.
* `param_spec_*`  -- ordered `{name: shape}` for each network, same names as the reference modules.
* `synth_state_dict` -- deterministic synthetic weights from the torch CPU generator; every
  tensor is drawn from its own seed derived from (seed, name) so the oracle, the HIP path and
  the golden-fixture generator regenerate identical weights without shipping them.
"""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch

# ----------------------------------------------------------------------------------------
# configuration
# ----------------------------------------------------------------------------------------


@dataclass(frozen=True)
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    hint_channels: int = 3
    model_channels: int = 320
    num_res_blocks: int = 2
    attention_resolutions: Tuple[int, ...] = (4, 2, 1)
    channel_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_heads: int = 8
    context_dim: int = 768
    context_len: int = 77
    # the cldm_v21.yaml layout (`cldm/cldm.py:64,77,184-207`): a fixed head width instead of a fixed head count (-1: num_heads
    # holds), and nn.Linear instead of conv1x1 as the SpatialTransformer's proj_in / proj_out (`ldm/modules/attention.py:409-429`)
    num_head_channels: int = -1
    use_linear_in_transformer: bool = False

    @property
    def time_embed_dim(self) -> int:
        return self.model_channels * 4

    def heads_for(self, ch: int) -> int:
        """Heads of an attention block of `ch` channels (`cldm/cldm.py:184-191`)."""
        return self.num_heads if self.num_head_channels in (-1, 0) else ch // self.num_head_channels


@dataclass(frozen=True)
class VAEConfig:
    ch: int = 128
    out_ch: int = 3
    ch_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    z_channels: int = 4
    embed_dim: int = 4
    scale_factor: float = 0.18215


@dataclass(frozen=True)
class ScheduleConfig:
    """LatentDiffusion schedule values (upstream SD-v1; not present in the reference tree)."""
    timesteps: int = 1000
    linear_start: float = 0.00085
    linear_end: float = 0.012
    parameterization: str = "eps"


UNET_SD15 = UNetConfig()
VAE_SD15 = VAEConfig()
SCHEDULE_SD15 = ScheduleConfig()
# SD-2.x + its ControlNet (the cldm_v21.yaml layout): head width 64 (5 / 10 / 20 / 20 heads), Linear projections, OpenCLIP-H context;
# the 768-v checkpoints predict v instead of eps
UNET_SD21 = UNetConfig(num_head_channels=64, use_linear_in_transformer=True, context_dim=1024)
SCHEDULE_SD21V = ScheduleConfig(parameterization="v")

# reduced configuration with the same topology, for fast numeric tests
UNET_TINY = UNetConfig(model_channels=64, context_dim=96, num_heads=4)  # context_dim must differ from every query dim (attention.py:168-173 quirk)
VAE_TINY = VAEConfig(ch=32)
# the 2.x layout reduced: heads 2 / 4 / 8 / 8 at width 32
UNET_TINY21 = UNetConfig(model_channels=64, num_head_channels=32, use_linear_in_transformer=True, context_dim=96)


# ----------------------------------------------------------------------------------------
# block plans
# ----------------------------------------------------------------------------------------


@dataclass
class Block:
    """One entry of a TimestepEmbedSequential (`openaimodel.py:73-87`)."""
    kind: str                 # 'conv_in' | 'res' | 'attn' | 'down' | 'up'
    name: str                 # parameter prefix, e.g. 'input_blocks.1.0'
    cin: int
    cout: int
    heads: int = 0


@dataclass
class UNetPlan:
    cfg: UNetConfig
    input_blocks: List[List[Block]] = field(default_factory=list)
    middle_block: List[Block] = field(default_factory=list)
    output_blocks: List[List[Block]] = field(default_factory=list)
    input_block_chans: List[int] = field(default_factory=list)
    # spatial downsample factor at which each input block's output lives (1,2,4,8)
    input_block_ds: List[int] = field(default_factory=list)


def unet_plan(cfg: UNetConfig, with_decoder: bool = True) -> UNetPlan:
    """Mirror of the constructor loops in `openaimodel.py:544-732` (UNetModel) and
    `cldm/cldm.py:138-279` (ControlNet encoder copy; `with_decoder=False`)."""
    mc = cfg.model_channels
    plan = UNetPlan(cfg)
    plan.input_blocks.append([Block("conv_in", "input_blocks.0.0", cfg.in_channels, mc)])
    chans = [mc]
    dss = [1]
    ch, ds = mc, 1
    idx = 1
    for level, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            layers = [Block("res", f"input_blocks.{idx}.0", ch, mult * mc)]
            ch = mult * mc
            if ds in cfg.attention_resolutions:
                layers.append(Block("attn", f"input_blocks.{idx}.1", ch, ch, cfg.heads_for(ch)))
            plan.input_blocks.append(layers)
            chans.append(ch)
            dss.append(ds)
            idx += 1
        if level != len(cfg.channel_mult) - 1:
            plan.input_blocks.append([Block("down", f"input_blocks.{idx}.0", ch, ch)])
            chans.append(ch)
            ds *= 2
            dss.append(ds)
            idx += 1
    plan.input_block_chans = list(chans)
    plan.input_block_ds = list(dss)
    plan.middle_block = [
        Block("res", "middle_block.0", ch, ch),
        Block("attn", "middle_block.1", ch, ch, cfg.heads_for(ch)),
        Block("res", "middle_block.2", ch, ch),
    ]
    if not with_decoder:
        return plan
    stack = list(chans)
    oidx = 0
    for level, mult in list(enumerate(cfg.channel_mult))[::-1]:
        for i in range(cfg.num_res_blocks + 1):
            ich = stack.pop()
            layers = [Block("res", f"output_blocks.{oidx}.0", ch + ich, mc * mult)]
            ch = mc * mult
            if ds in cfg.attention_resolutions:
                layers.append(Block("attn", f"output_blocks.{oidx}.1", ch, ch, cfg.heads_for(ch)))
            if level and i == cfg.num_res_blocks:
                layers.append(Block("up", f"output_blocks.{oidx}.{len(layers)}", ch, ch))
                ds //= 2
            plan.output_blocks.append(layers)
            oidx += 1
    return plan


HINT_BLOCK_CHANNELS = [(None, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1),
                       (96, 256, 2), (256, None, 1)]  # (cin, cout, stride); `cldm/cldm.py:147-163`


def hint_block_convs(cfg: UNetConfig) -> List[Tuple[str, int, int, int]]:
    out = []
    for i, (ci, co, s) in enumerate(HINT_BLOCK_CHANNELS):
        ci = cfg.hint_channels if ci is None else ci
        co = cfg.model_channels if co is None else co
        out.append((f"input_hint_block.{2 * i}", ci, co, s))
    return out


# ----------------------------------------------------------------------------------------
# parameter inventory
# ----------------------------------------------------------------------------------------

Spec = "OrderedDict[str, Tuple[int, ...]]"


def _conv(spec, name, cin, cout, k):
    spec[f"{name}.weight"] = (cout, cin, k, k)
    spec[f"{name}.bias"] = (cout,)


def _lin(spec, name, cin, cout, bias=True):
    spec[f"{name}.weight"] = (cout, cin)
    if bias:
        spec[f"{name}.bias"] = (cout,)


def _norm(spec, name, c):
    spec[f"{name}.weight"] = (c,)
    spec[f"{name}.bias"] = (c,)


def _res(spec, b: Block, emb: int):
    """ResBlock parameters (`openaimodel.py:200-240`)."""
    _norm(spec, f"{b.name}.in_layers.0", b.cin)
    _conv(spec, f"{b.name}.in_layers.2", b.cin, b.cout, 3)
    _lin(spec, f"{b.name}.emb_layers.1", emb, b.cout)
    _norm(spec, f"{b.name}.out_layers.0", b.cout)
    _conv(spec, f"{b.name}.out_layers.3", b.cout, b.cout, 3)
    if b.cin != b.cout:
        _conv(spec, f"{b.name}.skip_connection", b.cin, b.cout, 1)


def _attn(spec, b: Block, ctx: int, linear: bool = False):
    """SpatialTransformer parameters (`ldm/modules/attention.py:397-429`, depth 1,
    BasicTransformerBlock `:360-375`, CrossAttention `:154-179`, GEGLU FeedForward `:49-76`).
    linear: proj_in / proj_out are nn.Linear, weights (C, C) (`use_linear`, `:409-429`)."""
    c = b.cin
    proj = (lambda n: _lin(spec, n, c, c)) if linear else (lambda n: _conv(spec, n, c, c, 1))
    _norm(spec, f"{b.name}.norm", c)
    proj(f"{b.name}.proj_in")
    t = f"{b.name}.transformer_blocks.0"
    for a, kd in (("attn1", c), ("attn2", ctx)):
        _lin(spec, f"{t}.{a}.to_q", c, c, bias=False)
        _lin(spec, f"{t}.{a}.to_k", kd, c, bias=False)
        _lin(spec, f"{t}.{a}.to_v", kd, c, bias=False)
        _lin(spec, f"{t}.{a}.to_out.0", c, c)
    _lin(spec, f"{t}.ff.net.0.proj", c, 8 * c)
    _lin(spec, f"{t}.ff.net.2", 4 * c, c)
    for n in ("norm1", "norm2", "norm3"):
        _norm(spec, f"{t}.{n}", c)
    proj(f"{b.name}.proj_out")


def _blocks(spec, blocks: List[Block], cfg: UNetConfig):
    for b in blocks:
        if b.kind == "conv_in":
            _conv(spec, b.name, b.cin, b.cout, 3)
        elif b.kind == "res":
            _res(spec, b, cfg.time_embed_dim)
        elif b.kind == "attn":
            _attn(spec, b, cfg.context_dim, cfg.use_linear_in_transformer)
        elif b.kind == "down":
            _conv(spec, f"{b.name}.op", b.cin, b.cout, 3)
        elif b.kind == "up":
            _conv(spec, f"{b.name}.conv", b.cin, b.cout, 3)
        else:
            raise ValueError(b.kind)


def param_spec_unet(cfg: UNetConfig = UNET_SD15):
    """ControlledUnetModel/UNetModel parameters, reference naming (`openaimodel.py:528-732`)."""
    spec = OrderedDict()
    plan = unet_plan(cfg)
    _lin(spec, "time_embed.0", cfg.model_channels, cfg.time_embed_dim)
    _lin(spec, "time_embed.2", cfg.time_embed_dim, cfg.time_embed_dim)
    for blocks in plan.input_blocks:
        _blocks(spec, blocks, cfg)
    _blocks(spec, plan.middle_block, cfg)
    for blocks in plan.output_blocks:
        _blocks(spec, blocks, cfg)
    _norm(spec, "out.0", cfg.model_channels)
    _conv(spec, "out.2", cfg.model_channels, cfg.out_channels, 3)
    return spec


def param_spec_ip_adapter(cfg: UNetConfig = UNET_SD15):
    """What an image-prompt adapter (IP-Adapter) adds to the UNet: `<block>.transformer_blocks.0.attn2.to_k_ip.weight` and
    `...to_v_ip.weight`, (C, context_dim) each and no bias, for every UNet attention block, in the order of a forward pass (input blocks,
    middle block, output blocks): the order in which `sdeo_enable_ip_adapter` registers them.  Names without the `model.diffusion_model.`
    prefix, like `param_spec_unet`."""
    spec = OrderedDict()
    plan = unet_plan(cfg)
    for blocks in list(plan.input_blocks) + [plan.middle_block] + list(plan.output_blocks):
        for b in blocks:
            if b.kind == "attn":
                for leaf in ("to_k_ip", "to_v_ip"):
                    _lin(spec, f"{b.name}.transformer_blocks.0.attn2.{leaf}", cfg.context_dim, b.cin, bias=False)
    return spec


def param_spec_controlnet(cfg: UNetConfig = UNET_SD15):
    """ControlNet parameters, reference naming (`cldm/cldm.py:131-282`)."""
    spec = OrderedDict()
    plan = unet_plan(cfg, with_decoder=False)
    _lin(spec, "time_embed.0", cfg.model_channels, cfg.time_embed_dim)
    _lin(spec, "time_embed.2", cfg.time_embed_dim, cfg.time_embed_dim)
    for blocks in plan.input_blocks:
        _blocks(spec, blocks, cfg)
    for i, ch in enumerate(plan.input_block_chans):
        _conv(spec, f"zero_convs.{i}.0", ch, ch, 1)
    for name, ci, co, _ in hint_block_convs(cfg):
        _conv(spec, name, ci, co, 3)
    _blocks(spec, plan.middle_block, cfg)
    ch = plan.input_block_chans[-1]
    _conv(spec, "middle_block_out.0", ch, ch, 1)
    return spec


def vae_plan(cfg: VAEConfig = VAE_SD15):
    """Decoder structure (`ldm/modules/diffusionmodules/model.py:546-616`): returns
    (block_in, [(level, [(cin,cout)...], has_upsample)]) in execution order (highest level first)."""
    nres = len(cfg.ch_mult)
    block_in = cfg.ch * cfg.ch_mult[nres - 1]
    levels = []
    bi = block_in
    for i_level in reversed(range(nres)):
        bo = cfg.ch * cfg.ch_mult[i_level]
        blocks = []
        for _ in range(cfg.num_res_blocks + 1):
            blocks.append((bi, bo))
            bi = bo
        levels.append((i_level, blocks, i_level != 0))
    return block_in, levels


def _vae_res(spec, name, cin, cout):
    _norm(spec, f"{name}.norm1", cin)
    _conv(spec, f"{name}.conv1", cin, cout, 3)
    _norm(spec, f"{name}.norm2", cout)
    _conv(spec, f"{name}.conv2", cout, cout, 3)
    if cin != cout:
        _conv(spec, f"{name}.nin_shortcut", cin, cout, 1)


def param_spec_vae(cfg: VAEConfig = VAE_SD15):
    """`first_stage_model.*` parameters on the decode path: post_quant_conv + decoder.*
    (AutoencoderKL itself is absent from the reference tree; naming follows upstream)."""
    spec = OrderedDict()
    _conv(spec, "post_quant_conv", cfg.embed_dim, cfg.z_channels, 1)
    block_in, levels = vae_plan(cfg)
    d = "decoder"
    _conv(spec, f"{d}.conv_in", cfg.z_channels, block_in, 3)
    _vae_res(spec, f"{d}.mid.block_1", block_in, block_in)
    _norm(spec, f"{d}.mid.attn_1.norm", block_in)
    for n in ("q", "k", "v", "proj_out"):
        _conv(spec, f"{d}.mid.attn_1.{n}", block_in, block_in, 1)
    _vae_res(spec, f"{d}.mid.block_2", block_in, block_in)
    last = block_in
    for i_level, blocks, has_up in levels:
        for j, (ci, co) in enumerate(blocks):
            _vae_res(spec, f"{d}.up.{i_level}.block.{j}", ci, co)
            last = co
        if has_up:
            _conv(spec, f"{d}.up.{i_level}.upsample.conv", last, last, 3)
    _norm(spec, f"{d}.norm_out", last)
    _conv(spec, f"{d}.conv_out", last, cfg.out_ch, 3)
    return spec


def param_spec_vae_encoder(cfg: VAEConfig = VAE_SD15):
    """`first_stage_model.*` parameters on the encode path: encoder.* + quant_conv (`model.py:452-545` with attn_resolutions = [],
    double_z = True, in_channels = out_ch; quant_conv = upstream AutoencoderKL's 2 z_channels -> 2 embed_dim conv1x1).  Not part of
    param_spec_vae / param_spec_full: a runtime expects these only when built with vae_encoder=True."""
    spec = OrderedDict()
    d = "encoder"
    _conv(spec, f"{d}.conv_in", cfg.out_ch, cfg.ch, 3)
    bi = cfg.ch
    for i_level, m in enumerate(cfg.ch_mult):
        bo = cfg.ch * m
        for j in range(cfg.num_res_blocks):
            _vae_res(spec, f"{d}.down.{i_level}.block.{j}", bi, bo)
            bi = bo
        if i_level != len(cfg.ch_mult) - 1:
            _conv(spec, f"{d}.down.{i_level}.downsample.conv", bi, bi, 3)
    _vae_res(spec, f"{d}.mid.block_1", bi, bi)
    _norm(spec, f"{d}.mid.attn_1.norm", bi)
    for n in ("q", "k", "v", "proj_out"):
        _conv(spec, f"{d}.mid.attn_1.{n}", bi, bi, 1)
    _vae_res(spec, f"{d}.mid.block_2", bi, bi)
    _norm(spec, f"{d}.norm_out", bi)
    _conv(spec, f"{d}.conv_out", bi, 2 * cfg.z_channels, 3)
    _conv(spec, "quant_conv", 2 * cfg.z_channels, 2 * cfg.embed_dim, 1)
    return spec


# checkpoint namespaces of `control_sd15_canny.pth`
NS_UNET = "model.diffusion_model."
NS_CONTROL = "control_model."
NS_VAE = "first_stage_model."


def param_spec_full(ucfg: UNetConfig = UNET_SD15, vcfg: VAEConfig = VAE_SD15):
    spec = OrderedDict()
    for ns, s in ((NS_UNET, param_spec_unet(ucfg)), (NS_CONTROL, param_spec_controlnet(ucfg)),
                  (NS_VAE, param_spec_vae(vcfg))):
        for k, v in s.items():
            spec[ns + k] = v
    return spec


# ----------------------------------------------------------------------------------------
# synthetic weights
# ----------------------------------------------------------------------------------------


def _seed_for(seed: int, name: str) -> int:
    h = hashlib.sha256(f"{seed}:{name}".encode()).digest()
    return int.from_bytes(h[:7], "little")


@dataclass(frozen=True)
class ClipConfig:
    """CLIP text transformer behind `FrozenCLIPEmbedder` (`ldm/modules/encoders/modules.py:90-141`):
    openai/clip-vit-large-patch14 text tower (HuggingFace `CLIPTextConfig` of that checkpoint)."""
    vocab: int = 49408
    positions: int = 77
    width: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072


CLIP_SD15 = ClipConfig()
CLIP_TINY = ClipConfig(vocab=1000, positions=77, width=64, layers=2, heads=4, ffn=128)
# the OpenCLIP ViT-H/14 text tower behind `FrozenOpenCLIPEmbedder` (`ldm/modules/encoders/modules.py:147-206`): erf-GELU, and the
# SD-2.x configs read the penultimate block's output through ln_final; same tensor inventory as the CLIP-L tower
CLIP_SD21 = ClipConfig(vocab=49408, positions=77, width=1024, layers=24, heads=16, ffn=4096)
CLIP_TINY21 = ClipConfig(vocab=1000, positions=77, width=128, layers=3, heads=4, ffn=256)
NS_CLIP = "cond_stage_model.transformer.text_model."


def _clip_layers(spec, cfg):
    """`encoder.layers.{i}.*` of a CLIP tower (text or vision: cfg has layers, width and ffn), weight then bias per projection"""
    w, f = cfg.width, cfg.ffn
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            spec[p + f"self_attn.{n}.weight"] = (w, w)
            spec[p + f"self_attn.{n}.bias"] = (w,)
        spec[p + "layer_norm1.weight"] = (w,)
        spec[p + "layer_norm1.bias"] = (w,)
        spec[p + "mlp.fc1.weight"] = (f, w)
        spec[p + "mlp.fc1.bias"] = (f,)
        spec[p + "mlp.fc2.weight"] = (w, f)
        spec[p + "mlp.fc2.bias"] = (w,)
        spec[p + "layer_norm2.weight"] = (w,)
        spec[p + "layer_norm2.bias"] = (w,)


def param_spec_clip(cfg: ClipConfig = CLIP_SD15) -> "OrderedDict[str, tuple]":
    """Tensor names below `text_model.` and shapes of the HuggingFace CLIPTextModel state dict."""
    w = cfg.width
    spec = OrderedDict()
    spec["embeddings.token_embedding.weight"] = (cfg.vocab, w)
    spec["embeddings.position_embedding.weight"] = (cfg.positions, w)
    _clip_layers(spec, cfg)
    spec["final_layer_norm.weight"] = (w,)
    spec["final_layer_norm.bias"] = (w,)
    return spec


@dataclass(frozen=True)
class ClipVisionConfig:
    """CLIP vision tower with projection (HuggingFace `CLIPVisionModelWithProjection`); the defaults are OpenCLIP ViT-H/14, the image
    encoder the ip-adapter_sd15 files are trained against (`image_encoder/config.json` of that repository)."""
    image: int = 224
    patch: int = 14
    width: int = 1280
    layers: int = 32
    heads: int = 16
    ffn: int = 5120
    proj: int = 1024

    @property
    def tokens(self) -> int:
        return (self.image // self.patch) ** 2 + 1


CLIP_VISION_H14 = ClipVisionConfig()
# everything inside one tile: T = 17
CLIP_VISION_TINY = ClipVisionConfig(image=56, patch=14, width=64, layers=3, heads=4, ffn=128, proj=48)
# the real T = 257, P = 256, Kp = 592 and d = 80 at toy widths: the ragged key tile, the K tail, the strided class-row LayerNorm
CLIP_VISION_TINY80 = ClipVisionConfig(image=224, patch=14, width=160, layers=2, heads=2, ffn=320, proj=64)
NS_CLIP_VISION = "image_encoder.vision_model."      # seed namespace of the synthetic draw


def param_spec_clip_vision(cfg: ClipVisionConfig = CLIP_VISION_H14) -> "OrderedDict[str, tuple]":
    """Tensor names below `vision_model.` (plus `visual_projection.weight`) and shapes of the HuggingFace
    CLIPVisionModelWithProjection state dict.  `sdeo_clip_vision_weight_info` lists the same tensors, with the stacked q | k | v
    weights of a layer in front of their biases (as the text tower's registry does)."""
    w = cfg.width
    spec = OrderedDict()
    spec["embeddings.class_embedding"] = (w,)
    spec["embeddings.patch_embedding.weight"] = (w, 3, cfg.patch, cfg.patch)
    spec["embeddings.position_embedding.weight"] = (cfg.tokens, w)
    spec["pre_layrnorm.weight"] = (w,)
    spec["pre_layrnorm.bias"] = (w,)
    _clip_layers(spec, cfg)
    spec["post_layernorm.weight"] = (w,)
    spec["post_layernorm.bias"] = (w,)
    spec["visual_projection.weight"] = (cfg.proj, w)
    return spec


def synth_clip_vision_state_dict(cfg: ClipVisionConfig = CLIP_VISION_H14, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded vision-tower weights (fp32, CPU) under the names of `param_spec_clip_vision`, as `ClipVisionRuntime.load_synthetic` draws
    them; pre_layrnorm / post_layernorm scales are drawn around 1 like every other norm."""
    out = OrderedDict()
    for k, shp in param_spec_clip_vision(cfg).items():
        t = synth_tensor(NS_CLIP_VISION + k, shp, seed)
        if k in ("pre_layrnorm.weight", "post_layernorm.weight"):
            t = 1.0 + 5.0 * t          # (synth_tensor knows "layer_norm" only: 0.02 N -> 1 + 0.1 N)
        out[k] = t
    return out


@dataclass(frozen=True)
class ResamplerConfig:
    """The Resampler image projection of the IP-Adapter "plus" files (csrc/resampler.hip; include/sdeo.h states the algorithm); the
    defaults are ip-adapter-plus_sd15 / ip-adapter-plus-face_sd15 behind the ViT-H/14 tower's hidden_states[-2]."""
    tokens: int = 257
    embed_dim: int = 1280
    dim: int = 768
    depth: int = 4
    dim_head: int = 64
    heads: int = 12
    num_queries: int = 16
    ffn: int = 3072
    out_dim: int = 768

    @property
    def inner(self) -> int:
        return self.heads * self.dim_head


RESAMPLER_PLUS_SD15 = ResamplerConfig()
# inner 64 != dim; dim = 12 vectors of 8, less than a wave; every key in one tile; fits CLIP_VISION_TINY (T 17, W 64) + UNET_TINY (96)
RESAMPLER_TINY = ResamplerConfig(tokens=17, embed_dim=64, dim=96, depth=2, dim_head=32, heads=2, num_queries=4, ffn=384, out_dim=96)
# the real T + Q = 273 ragged key tile, the real head dim and token count; fits CLIP_VISION_TINY80 (T 257, W 160)
RESAMPLER_TINY273 = ResamplerConfig(tokens=257, embed_dim=160, dim=128, depth=2, dim_head=64, heads=2, num_queries=16, ffn=512, out_dim=96)
NS_RESAMPLER = "image_proj."                        # the file's group; also the seed namespace of the synthetic draw
RESAMPLER_DIM_HEAD = 64                             # the file does not state it; 64 in every published file


def param_spec_resampler(cfg: ResamplerConfig = RESAMPLER_PLUS_SD15) -> "OrderedDict[str, tuple]":
    """Tensor names below `image_proj.` and shapes of a "plus" adapter file's Resampler, in the order `sdeo_resampler_weight_info`
    lists them.  The key names are stated from the published files and are UNPINNED: no plus file was at hand."""
    d, i, f = cfg.dim, cfg.inner, cfg.ffn
    spec = OrderedDict()
    spec["latents"] = (1, cfg.num_queries, d)
    spec["proj_in.weight"] = (d, cfg.embed_dim)
    spec["proj_in.bias"] = (d,)
    spec["proj_out.weight"] = (cfg.out_dim, d)
    spec["proj_out.bias"] = (cfg.out_dim,)
    spec["norm_out.weight"] = (cfg.out_dim,)
    spec["norm_out.bias"] = (cfg.out_dim,)
    for l in range(cfg.depth):
        a, ff = f"layers.{l}.0.", f"layers.{l}.1."
        for n in ("norm1", "norm2"):
            spec[a + n + ".weight"] = (d,)
            spec[a + n + ".bias"] = (d,)
        spec[a + "to_q.weight"] = (i, d)
        spec[a + "to_kv.weight"] = (2 * i, d)
        spec[a + "to_out.weight"] = (d, i)
        spec[ff + "0.weight"] = (d,)
        spec[ff + "0.bias"] = (d,)
        spec[ff + "1.weight"] = (f, d)
        spec[ff + "3.weight"] = (d, f)
    return spec


def synth_resampler_state_dict(cfg: ResamplerConfig = RESAMPLER_PLUS_SD15, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded Resampler weights (fp32, CPU) under the names of `param_spec_resampler`, as `ResamplerRuntime.load_synthetic` draws them.
    Two tensors `synth_tensor` would get wrong: `latents` is randn / sqrt(dim) as the module initialises it (its fan-in rule would give
    1 / sqrt(num_queries * dim)), and `layers.<l>.1.0.weight`, the FF LayerNorm's scale, has no "norm" in its name."""
    out = OrderedDict()
    for k, shp in param_spec_resampler(cfg).items():
        if k == "latents":
            g = torch.Generator(device="cpu")
            g.manual_seed(_seed_for(seed, NS_RESAMPLER + k))
            t = torch.randn(shp, generator=g) / cfg.dim ** 0.5
        else:
            t = synth_tensor(NS_RESAMPLER + k, shp, seed)
            if k.endswith(".1.0.weight"):
                t = 1.0 + 5.0 * t          # 0.02 N -> 1 + 0.1 N, like every other norm scale
        out[k] = t
    return out


def synth_tensor(name: str, shape, seed: int = 0) -> torch.Tensor:
    """Deterministic stand-in for one checkpoint tensor (fp32, CPU).

    Norm scales ~ 1 + 0.1 N(0,1), biases ~ 0.02 N(0,1), matrices ~ N(0, 1/fan_in) * gain.  The
    reference's `zero_module` tensors are drawn like every other tensor (with all-zero
    zero-convs every network output is exactly 0)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(_seed_for(seed, name))
    shape = tuple(shape)
    leaf = name.rsplit(".", 1)[-1]
    if len(shape) == 1:
        is_norm = any(t in name for t in (".norm", "in_layers.0", "out_layers.0", "out.0", "norm_out", "layer_norm"))
        if leaf == "weight" and is_norm:
            return 1.0 + 0.1 * torch.randn(shape, generator=g)
        return 0.02 * torch.randn(shape, generator=g)
    if "_embedding.weight" in name:          # CLIP token / position tables: entries of order 0.02-ish like the real ones
        return 0.05 * torch.randn(shape, generator=g)
    fan_in = 1
    for d in shape[1:]:
        fan_in *= d
    return torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5


def synth_state_dict(spec, seed: int = 0, prefix: str = "") -> Dict[str, torch.Tensor]:
    return OrderedDict((k, synth_tensor(prefix + k, shp, seed)) for k, shp in spec.items())


def synth_vae_encoder_state_dict(cfg: VAEConfig = VAE_SD15, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic `first_stage_model.encoder.*` / `quant_conv.*` tensors, drawn exactly as SdeoRuntime(vae_encoder=True).load_synthetic
    draws them (full checkpoint names)."""
    return OrderedDict((NS_VAE + k, v) for k, v in synth_state_dict(param_spec_vae_encoder(cfg), seed, NS_VAE).items())


def count_params(spec) -> int:
    n = 0
    for shp in spec.values():
        p = 1
        for d in shp:
            p *= d
        n += p
    return n


# ----------------------------------------------------------------------------------------
# HED soft-edge annotator (`annotator/hed/__init__.py`: ControlNetHED_Apache2)
# ----------------------------------------------------------------------------------------
HED_BLOCKS = [(2, 64), (2, 128), (3, 256), (3, 512), (3, 512)]    # (3x3 convs, channels) of block1..block5
NS_HED = "hed."                                                  # seed namespace of the synthetic draw (not part of the names)
# projection gain per block: with He-gain convs every block output sits on the 0-255 input scale, so each side map is scaled down to
# logits of a few units; the five maps then average to values mostly inside the sigmoid's sensitive range (tests/test_hed_cpu.py)
HED_PROJ_GAIN = (0.05, 0.02, 0.03, 0.03, 0.02)


def param_spec_hed() -> "OrderedDict[str, tuple]":
    """The reference state dict of ControlNetHED_Apache2 (= the public ControlNetHED.pth): 37 tensors, in module order."""
    spec = OrderedDict()
    spec["norm"] = (1, 3, 1, 1)
    cin = 3
    for b, (n, c) in enumerate(HED_BLOCKS):
        for i in range(n):
            spec[f"block{b + 1}.convs.{i}.weight"] = (c, cin, 3, 3)
            spec[f"block{b + 1}.convs.{i}.bias"] = (c,)
            cin = c
        spec[f"block{b + 1}.projection.weight"] = (1, c, 1, 1)
        spec[f"block{b + 1}.projection.bias"] = (1,)
    return spec


def synth_hed_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic HED weights (fp32, CPU), drawn for a ReLU stack rather than with `synth_tensor` (whose N(0, 1/fan_in) shrinks
    the activations about 90x over 13 layers): 3x3 convs N(0, 2/fan_in) (He gain: activations stay on the 0-255 input scale, so the
    fp16 range is exercised), conv biases 0.5 N(0,1), norm = 100 + 40 U(0,1) (plausible pixel means), projections
    N(0,1) HED_PROJ_GAIN[b] / sqrt(C) with bias 0.1 N(0,1)."""
    out = OrderedDict()
    for name, shape in param_spec_hed().items():
        g = torch.Generator(device="cpu")
        g.manual_seed(_seed_for(seed, NS_HED + name))
        b = int(name[5]) - 1 if name.startswith("block") else -1
        if name == "norm":
            t = 100.0 + 40.0 * torch.rand(shape, generator=g)
        elif ".projection.weight" in name:
            t = torch.randn(shape, generator=g) * (HED_PROJ_GAIN[b] / shape[1] ** 0.5)
        elif ".projection.bias" in name:
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".weight"):
            t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * 9)) ** 0.5
        else:
            t = 0.5 * torch.randn(shape, generator=g)
        out[name] = t
    return out
