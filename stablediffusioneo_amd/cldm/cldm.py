"""Host-side mirror of the reference's model surface (`cldm/cldm.py`): ControlNet, ControlledUnetModel and
ControlLDM with the same names, call signatures and semantics, but every forward is ONE call into libsdeo
(the seam where the TensorRT variant calls `Engine.infer`, `cldm_trt/cldm.py:321-341,368-384`).

Also restates the attributes of the absent `LatentDiffusion` base class that the sampler and the pipeline
read: `num_timesteps`, `betas`, `alphas_cumprod`, `alphas_cumprod_prev`, `device`,
`parameterization`, `predict_eps_from_z_and_v`, `predict_start_from_z_and_v`, `get_learned_conditioning`, `decode_first_stage`, `first_stage_model`, `model.diffusion_model`.
"""
from __future__ import annotations

import types
from typing import Callable, List, Optional

import numpy as np
import torch

from .. import spec as S
from ..runtime import CONTEXT_CACHED, HINT_CACHED, SdeoRuntime


def make_beta_schedule_linear(n_timestep, linear_start, linear_end):
    """`ldm/modules/diffusionmodules/util.py:21-25` ("linear": linspace in sqrt space, float64)."""
    return (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2).numpy()


class ControlNet:
    """`cldm/cldm.py:48-305`.  forward(x, hint, timesteps, context) -> list of 13 NCHW fp32 tensors."""

    def __init__(self, runtime: SdeoRuntime):
        self.rt = runtime

    def forward(self, x, hint, timesteps, context, **kwargs):
        self.rt.configure(x.shape[0], x.shape[2], x.shape[3])
        return self.rt.controlnet(x, hint, timesteps, context)

    __call__ = forward


class ControlledUnetModel:
    """`cldm/cldm.py:22-45`.  Like the reference, `control` (a list) is CONSUMED by the call (`:35,41` pop())."""

    def __init__(self, runtime: SdeoRuntime):
        self.rt = runtime

    def forward(self, x, timesteps=None, context=None, control=None, only_mid_control=False, **kwargs):
        self.rt.configure(x.shape[0], x.shape[2], x.shape[3])
        ctrl = None
        if control is not None:
            ctrl = list(control)
            del control[:]
        return self.rt.unet(x, timesteps, context, control=ctrl, only_mid_control=only_mid_control)

    __call__ = forward


class DiagonalGaussianDistribution:
    """`ldm/modules/distributions/distributions.py:24-35,61-62` over the moments the HIP encoder returned: mean / logvar are the two
    halves of quant_conv's output, logvar clamped to [-30, 20].  `sample(noise)` takes the noise from the caller (None draws it with
    torch.randn, like the reference).  The library's own z (`SdeoRuntime.vae_encode`) applies the same formula on the device."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self, noise=None):
        if noise is None:
            noise = torch.randn(self.mean.shape).to(device=self.parameters.device)
        return self.mean + self.std * noise.to(device=self.parameters.device, dtype=self.mean.dtype)

    def mode(self):
        return self.mean


class AutoencoderKLDecoder:
    """`ldm.models.autoencoder.AutoencoderKL` (absent from the reference tree): decode always, encode when the runtime was built with
    the VAE encoder (create_model(..., vae_encoder=True))."""

    def __init__(self, runtime: SdeoRuntime):
        self.rt = runtime

    def decode(self, z):
        """z is ALREADY divided by scale_factor (upstream AutoencoderKL.decode contract)."""
        return self.rt.vae_decode(z * self.rt.vcfg.scale_factor)

    def encode(self, x):
        """upstream AutoencoderKL.encode: x (b,3,8h,8w) in [-1,1] -> DiagonalGaussianDistribution(quant_conv(encoder(x)))."""
        if not self.rt.vae_encoder:
            raise RuntimeError("first_stage_model.encode: the runtime was built without the VAE encoder "
                               "(create_model(..., vae_encoder=True) / SdeoRuntime(..., vae_encoder=True))")
        x = x.to(device=self.rt.device, dtype=torch.float32)
        self.rt.configure(max(self.rt.n, x.shape[0]), x.shape[2] // 8, x.shape[3] // 8)
        _, moments = self.rt.vae_encode(images=x, want_moments=True)
        return DiagonalGaussianDistribution(moments)


class ControlLDM:
    """`cldm/cldm.py:308-435` on top of a libsdeo runtime."""

    def __init__(self, runtime: SdeoRuntime, schedule: S.ScheduleConfig = S.SCHEDULE_SD15,
                 cond_stage_model: Optional[Callable[[List[str]], torch.Tensor]] = None, only_mid_control: bool = False):
        self.rt = runtime
        self.device = runtime.device
        self.control_model = ControlNet(runtime)
        self.model = types.SimpleNamespace(diffusion_model=ControlledUnetModel(runtime))
        self.first_stage_model = AutoencoderKLDecoder(runtime)
        self.cond_stage_model = cond_stage_model
        self.only_mid_control = only_mid_control
        self.control_scales = [1.0] * 13
        self.control_key = "hint"
        self.channels = runtime.ucfg.in_channels
        self.scale_factor = runtime.vcfg.scale_factor
        # LatentDiffusion.register_schedule (upstream semantics; file absent from the reference)
        self.parameterization = schedule.parameterization
        self.num_timesteps = schedule.timesteps
        betas = make_beta_schedule_linear(schedule.timesteps, schedule.linear_start, schedule.linear_end)
        ac = np.cumprod(1.0 - betas, axis=0)
        to_t = lambda a: torch.tensor(a, dtype=torch.float32, device=self.device)
        self.betas = to_t(betas)
        self.alphas_cumprod = to_t(ac)
        self.alphas_cumprod_prev = to_t(np.append(1.0, ac[:-1]))
        self.sqrt_alphas_cumprod = to_t(np.sqrt(ac))
        self.sqrt_one_minus_alphas_cumprod = to_t(np.sqrt(1.0 - ac))

    # -- nn.Module-ish conveniences the pipeline scripts call
    def cuda(self):
        return self

    def cpu(self):
        return self

    def eval(self):
        return self

    def load_state_dict(self, sd, strict=False, extra_control=None):
        """extra_control: one state dict per extra control network (`SdeoRuntime.load_state_dict`)"""
        self.rt.load_state_dict(sd, strict=strict, extra_control=extra_control)
        if hasattr(self.cond_stage_model, "load_state_dict"):      # FrozenCLIPEmbedder mirror: cond_stage_model.transformer.*;
            # FrozenOpenCLIPEmbedder mirror: cond_stage_model.model.*
            self.cond_stage_model.load_state_dict({k: v for k, v in sd.items() if "text_model." in k or k.startswith("cond_stage_model.model.")},
                                                  strict=False)
        return self

    def load_lora(self, lora, unet_scale=1.0, te_scale=None, strict=False, commit=True):
        """Merge a kohya-ss LoRA / LoCon or LyCORIS LoHa / LoKr adapter (a path or a dict) into the weights on the device (`stablediffusioneo_amd.lora.apply_lora`);
        returns the keys it did not understand."""
        from ..lora import apply_lora
        return apply_lora(self, lora, unet_scale=unet_scale, te_scale=te_scale, strict=strict, commit=commit)

    def clear_loras(self):
        """Back to the base weights, bit for bit (`stablediffusioneo_amd.lora.clear_loras`)."""
        from ..lora import clear_loras
        clear_loras(self)
        return self

    def low_vram_shift(self, is_diffusing):
        """`cldm/cldm.py:425-435` moves sub-models between host and device to fit small GPUs; with 288 GB of
        HBM everything stays resident."""
        return None

    # -- conditioning
    def get_learned_conditioning(self, prompts):
        if self.cond_stage_model is None:
            raise RuntimeError("no cond_stage_model: pass the FrozenCLIPEmbedder / FrozenOpenCLIPEmbedder mirror "
                               "(stablediffusioneo_amd.ldm.modules.encoders.modules) or any callable(prompts)->(B,77,context_dim) tensor")
        return self.cond_stage_model(prompts).to(self.device)

    def get_unconditional_conditioning(self, N):
        return self.get_learned_conditioning([""] * N)

    # -- the hot call
    def q_sample(self, x_start, t, noise=None):
        """Forward diffusion x_t = sqrt(abar_t) x_0 + sqrt(1 - abar_t) eps, called by the sampler's mask / x0 branch
        (`cldm/ddim_hacked.py:154-157`).  `LatentDiffusion.q_sample` itself is absent from the reference tree: upstream
        SD-v1 semantics, parity unpinned."""
        if noise is None:
            noise = torch.randn_like(x_start)
        ext = lambda a: a.to(x_start.device)[t].reshape(-1, *([1] * (x_start.dim() - 1)))
        return ext(self.sqrt_alphas_cumprod) * x_start + ext(self.sqrt_one_minus_alphas_cumprod) * noise

    def predict_start_from_z_and_v(self, x_t, t, v):
        """upstream LatentDiffusion.predict_start_from_z_and_v (absent from the reference tree; called by the sampler at
        `cldm/ddim_hacked.py:214-215` for a v-prediction model): x0 = sqrt(abar_t) x_t - sqrt(1 - abar_t) v."""
        ext = lambda a: a.to(x_t.device)[t].reshape(-1, *([1] * (x_t.dim() - 1)))
        return ext(self.sqrt_alphas_cumprod) * x_t - ext(self.sqrt_one_minus_alphas_cumprod) * v

    def predict_eps_from_z_and_v(self, x_t, t, v):
        """upstream LatentDiffusion.predict_eps_from_z_and_v (`cldm/ddim_hacked.py:194-197`): eps = sqrt(abar_t) v + sqrt(1 - abar_t) x_t."""
        ext = lambda a: a.to(x_t.device)[t].reshape(-1, *([1] * (x_t.dim() - 1)))
        return ext(self.sqrt_alphas_cumprod) * v + ext(self.sqrt_one_minus_alphas_cumprod) * x_t

    # -- several control networks: `control_scales` is the reference's one attribute, a flat list of 13 applied to every net, or a list
    # of one list of 13 per net
    def per_net_scales(self):
        k = 1 + self.rt.extra_controlnets
        cs = list(self.control_scales)
        if cs and isinstance(cs[0], (list, tuple)):
            if len(cs) != k:
                raise ValueError(f"control_scales holds {len(cs)} lists, the model has {k} control networks")
            return [[float(v) for v in row] for row in cs]
        return [[float(v) for v in cs] for _ in range(k)]

    def net0_scales(self):
        """net 0's scales, the argument of every runtime call; the extra nets' are handed to the runtime here when they changed"""
        per = self.per_net_scales()
        for j in range(1, len(per)):
            if self.rt._extra_scales[j - 1] != tuple(per[j]):
                self.rt.set_control_scales(j, per[j])
        return per[0]

    def scales_key(self):
        """every net's scales: part of the key of every captured graph"""
        return tuple(v for row in self.per_net_scales() for v in row)

    # -- image prompts (IP-Adapter; the runtime was created with ip_adapter_tokens = T).  The image tokens are conditioning like the
    # text context: the conditional request carries the image's tokens, the unconditional one the projection of a zero embedding, as in
    # the adapter's own pipeline.  They are kept here per role and travel in the conditioning dicts as "c_ip" (`with_ip`).
    def load_ip_adapter(self, adapter, image_tokens=None):
        """Load an IP-Adapter file (a path or its state dict) into a model created with ip_adapter_tokens: the to_k_ip / to_v_ip matrices
        go to the runtime, the image projection stays here (`stablediffusioneo_amd.ip_adapter`: an ImageProjModel, or the Resampler of a
        "plus" file, fed by a vision tower of image_tokens tokens).  Call it before the base weights are finalised (`load_state_dict`),
        like the extra control networks' weights."""
        from ..ip_adapter import load_ip_adapter
        self.ip_proj = load_ip_adapter(self.rt, adapter, image_tokens)
        return self

    def set_ip_tokens(self, cond, uncond=None):
        """Raw image tokens (b or 1, T, context_dim) for the conditional requests; uncond: for the unconditional ones (None: zeros)."""
        t_, cd = self.rt.ip_adapter_tokens, self.rt.ucfg.context_dim
        if not t_:
            raise RuntimeError("set_ip_tokens: the model was created without an image-prompt adapter (create_model(..., ip_adapter_tokens=T))")
        prep = lambda x: x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        cond = prep(cond)
        uncond = torch.zeros_like(cond) if uncond is None else prep(uncond)
        for name, x in (("cond", cond), ("uncond", uncond)):
            if x.dim() != 3 or tuple(x.shape[1:]) != (t_, cd):
                raise ValueError(f"set_ip_tokens: {name} tokens of shape {tuple(x.shape)}, the adapter takes (b, {t_}, {cd})")
        # The samplers key their conditioning caches on the identity of the tensors they are given (storage, in-place version, shape):
        # tokens of the same shape are copied INTO the kept tensors, which bumps their version; fresh tensors could land on the
        # address the previous ones had and look unchanged.
        old = getattr(self, "_ip", None)
        if old is not None and old["cond"].shape == cond.shape and old["uncond"].shape == uncond.shape:
            old["cond"].copy_(cond)
            old["uncond"].copy_(uncond)
        else:
            self._ip = {"cond": cond.clone(), "uncond": uncond.clone()}
        return self

    def set_ip_image_embeds(self, cond_embeds, uncond_embeds=None, scale=1.0):
        """CLIP image embeddings (b or 1, embed_dim) -> tokens through the loaded adapter's ImageProjModel (torch fp32 on the device, once
        per image).  uncond_embeds None: the projection of zeros.
        With the Resampler of a "plus" file the embeddings are the tower's hidden_states[-2] (b or 1, tokens, embed_dim), projected on
        the HIP path; the adapter's own rule for the unconditional half is the hidden states of an all-zero pixel_values, which the
        caller computes with the tower and passes as uncond_embeds (None here is still zeros)."""
        if getattr(self, "ip_proj", None) is None:
            raise RuntimeError("set_ip_image_embeds: no image projection (load_ip_adapter first, or give tokens to set_ip_tokens)")
        cond_embeds = cond_embeds.detach().to(device=self.device, dtype=torch.float32)
        uncond_embeds = torch.zeros_like(cond_embeds) if uncond_embeds is None else uncond_embeds.detach().to(device=self.device, dtype=torch.float32)
        self.set_ip_tokens(self.ip_proj(cond_embeds), self.ip_proj(uncond_embeds))
        self.ip_scale = float(scale)
        return self

    ip_scale = 1.0

    def with_ip(self, cond, role, b):
        """`cond` with the image tokens of `role` ("cond" / "uncond") for b images under "c_ip", unless it carries some already or the
        model has no adapter.  Stored tokens of one image serve any b (a view: its identity is the stored tensor's)."""
        if not self.rt.ip_adapter_tokens or not isinstance(cond, dict) or cond.get("c_ip") is not None:
            return cond
        if getattr(self, "_ip", None) is None:
            raise RuntimeError("this model has an image-prompt adapter but no image tokens: call set_ip_image_embeds or set_ip_tokens first")
        t = self._ip[role]
        if t.shape[0] not in (1, b):
            raise ValueError(f"{t.shape[0]} sets of image tokens for {b} images")
        return {**cond, "c_ip": [t if t.shape[0] == b else t.expand(b, -1, -1)]}

    def sync_ip_scale(self):
        """hand `ip_scale` to the runtime when it differs (sdeo_configure resets the library's to 1)"""
        if self.rt.ip_adapter_tokens and self.rt.ip_scale != float(self.ip_scale):
            self.rt.set_ip_scale(self.ip_scale)

    # -- FreeU (include/sdeo.h: sdeo_set_freeu): backbone scaling and the skip's Fourier filter in the UNet decoder, no weights
    def set_freeu(self, b1=None, b2=None, s1=None, s2=None, version: int = 2):
        """FreeU in every following forward and sampler run (`SdeoRuntime.set_freeu`); `set_freeu(None)` turns it off.  The samplers'
        captured loops are keyed on it: new values capture anew, the same values replay."""
        self.rt.set_freeu(b1, b2, s1, s2, version)
        return self

    def freeu_key(self):
        return self.rt.freeu_key()

    # -- control schedule (`cldm/control_schedule.py`): per step and per net, both halves / the conditional half / off.  None: nothing
    # changes anywhere.  The samplers read the attribute; the setter checks it against the model first.
    control_schedule = None

    def set_control_schedule(self, schedule=None):
        """one ControlSchedule (every net), a list with one per net, or None (off).  Needs create_model(..., control_modes=True).  The
        samplers' captured loops are keyed on it: the same schedule replays, another one captures anew, None replays what ran before."""
        from .control_schedule import normalize
        normalize(schedule, 1 + self.rt.extra_controlnets)
        if schedule is not None and not getattr(self.rt, "control_modes", False):
            raise RuntimeError("set_control_schedule: the model was created without control modes (create_model(..., control_modes=True))")
        self.control_schedule = schedule
        return self

    def apply_model(self, x_noisy, t, cond, *args, flags: int = 0, out=None, **kwargs):
        """`cldm/cldm.py:328-341`.  With K control networks the channel concatenation of c_concat holds K hints: chunk j is net j's.
        With an image-prompt adapter cond["c_ip"] holds the image tokens of the n images (absent: the stored conditional ones)."""
        assert isinstance(cond, dict)
        cond_txt = torch.cat(cond["c_crossattn"], 1) if cond["c_crossattn"] is not None else None
        self.rt.configure(x_noisy.shape[0], x_noisy.shape[2], x_noisy.shape[3])
        if self.rt.ip_adapter_tokens:
            self.sync_ip_scale()
            if not (flags & CONTEXT_CACHED):      # the image tokens are conditioning: cached with the context K / V
                self.rt.set_ip_tokens(torch.cat(self.with_ip(cond, "cond", x_noisy.shape[0])["c_ip"], 0))
        if cond["c_concat"] is None:
            return self.rt.apply_model(x_noisy, None, t, cond_txt, None, self.only_mid_control, flags & CONTEXT_CACHED, out)
        hint = torch.cat(cond["c_concat"], 1)
        k, hc = 1 + self.rt.extra_controlnets, self.rt.ucfg.hint_channels
        if hint.shape[1] != k * hc:
            raise ValueError(f"c_concat has {hint.shape[1]} channels: {k} control networks of {hc} hint channels each need {k * hc}")
        scales0 = self.net0_scales()
        if k > 1:
            chunks = torch.split(hint, hc, dim=1)
            hint = chunks[0]
            for j in range(1, k):
                if not (flags & HINT_CACHED) or not self.rt.extra_hint_is_set(j):
                    self.rt.set_control_hint(j, chunks[j])
        return self.rt.apply_model(x_noisy, hint, t, cond_txt, scales0, self.only_mid_control, flags, out)

    def encode_first_stage(self, x):
        """upstream LatentDiffusion.encode_first_stage: first_stage_model.encode(x) (a DiagonalGaussianDistribution)."""
        return self.first_stage_model.encode(x)

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """upstream LatentDiffusion.get_first_stage_encoding: scale_factor * encoder_posterior.sample() (a tensor is taken as is).
        `noise` fixes the posterior sample (None: torch.randn, as upstream)."""
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample(noise)
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    def decode_first_stage(self, z):
        """`canny2image_torch.py:63-67`: z = 1/scale_factor * z; first_stage_model.decode(z)."""
        return self.rt.vae_decode(z)

    def decode_first_stage_uint8(self, z):
        """decode + the post-process of `canny2image_torch.py:68`, fused on the device: (B,H,W,3) uint8."""
        return self.rt.vae_decode(z, want_u8=True)[1]
