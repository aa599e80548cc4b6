"""Generate the SD-2.x golden fixtures under tests/golden/ by running the REFERENCE's own modules with the cldm_v21.yaml layout
(`num_head_channels`, `use_linear_in_transformer`, context_dim 1024), its DDIMSampler on a v-prediction model, and HuggingFace's
CLIPTextModel with erf-GELU as the OpenCLIP text tower.  Same recipe and stubs as make_golden.py (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sd21.py [--only manifest,tiny,full,sampler,openclip,shapes]

Outputs (arrays, names and shapes only; inputs and weights are regenerated from seeds by the tests):
    manifest_sd21.json    parameter names + shapes of the reference ControlledUnetModel / ControlNet with the UNET_SD21 values (meta device)
    tiny21_nets.npz       ControlNet(13) / UNet eps / eps without control on UNET_TINY21, the cases of tiny_nets.npz
    sd21_lat8.npz         full UNET_SD21 (866 M + its ControlNet) at latent 8x8, N = 2, t = [801, 1]: 13 controls + eps (~10 GB host RAM)
    sampler_v.npz         DDIMSampler.sample with parameterization = "v": analytic model (S = 10; scale 1 / 9; eta 0 / 0.5) with every
                          model output and noise draw recorded, and one run over the reference tiny21 nets (S = 4, 8x8, scale 7.5)
    sd21_shapes.npz       full UNET_SD21 at the untuned shapes of tests/shape_cases.py SD21_SHAPES: eps, every 40th control channel, statistics
    openclip_tiny.npz     CLIPTextModel(hidden_act="gelu") on CLIP_TINY21: token ids, "last" and "penultimate" outputs
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as G                                # noqa: E402  (stubs + helpers; puts the repository and the reference on sys.path)
from stablediffusioneo_amd import spec as S            # noqa: E402
from tests.common import X_T_SEED, make_hint, make_inputs, randn           # noqa: E402


def ref_cfg(c: S.UNetConfig):
    d = G.ref_cfg(c)
    if c.num_head_channels not in (-1, 0):
        d.update(num_heads=-1, num_head_channels=c.num_head_channels)
    d["use_linear_in_transformer"] = c.use_linear_in_transformer
    return d


def build_ref(ucfg, device="cpu"):
    from cldm.cldm import ControlNet, ControlledUnetModel
    with G.quiet(), torch.device(device):
        unet = ControlledUnetModel(out_channels=ucfg.out_channels, **ref_cfg(ucfg))
        cn = ControlNet(hint_channels=ucfg.hint_channels, **ref_cfg(ucfg))
    return unet.eval(), cn.eval()


def loaded_ref(ucfg, seed=0):
    unet, cn = build_ref(ucfg)
    su, sc = S.param_spec_unet(ucfg), S.param_spec_controlnet(ucfg)
    G.check_spec(unet, su, "unet")
    G.check_spec(cn, sc, "controlnet")
    unet.load_state_dict(S.synth_state_dict(su, seed, S.NS_UNET))
    cn.load_state_dict(S.synth_state_dict(sc, seed, S.NS_CONTROL))
    return unet, cn


def gen_manifest():
    unet, cn = build_ref(S.UNET_SD21, device="meta")
    G.check_spec(unet, S.param_spec_unet(S.UNET_SD21), "sd21 unet")
    G.check_spec(cn, S.param_spec_controlnet(S.UNET_SD21), "sd21 controlnet")
    tu, tc = build_ref(S.UNET_TINY21, device="meta")
    G.check_spec(tu, S.param_spec_unet(S.UNET_TINY21), "tiny21 unet")
    G.check_spec(tc, S.param_spec_controlnet(S.UNET_TINY21), "tiny21 controlnet")
    man = {"unet": {k: list(v.shape) for k, v in unet.state_dict().items()},
           "controlnet": {k: list(v.shape) for k, v in cn.state_dict().items()}}
    with open(os.path.join(HERE, "manifest_sd21.json"), "w") as f:
        json.dump(man, f, indent=0, sort_keys=True)
    print("manifest_sd21:", {k: len(v) for k, v in man.items()}, "unet parameters",
          sum(int(np.prod(v)) for v in man["unet"].values()) / 1e6, "M")


def gen_tiny_nets():
    ucfg = S.UNET_TINY21
    unet, cn = loaded_ref(ucfg)
    out = {}
    for (n, h, w) in ((2, 16, 16), (1, 8, 24)):
        x, ctx, hint = make_inputs(n, h, w, ctx_dim=ucfg.context_dim)
        t = torch.tensor([801, 1][:n] if n == 2 else [401], dtype=torch.long)
        with torch.no_grad(), G.quiet():
            ctrl = cn(x=x, hint=hint, timesteps=t, context=ctx)
            eps = unet(x=x, timesteps=t, context=ctx, control=[c.clone() for c in ctrl], only_mid_control=False)
            eps_nc = unet(x=x, timesteps=t, context=ctx, control=None, only_mid_control=False)
        tag = f"n{n}_{h}x{w}"
        for i, c in enumerate(ctrl):
            out[f"{tag}.control{i}"] = c.numpy()
        out[f"{tag}.eps"] = eps.numpy()
        out[f"{tag}.eps_nocontrol"] = eps_nc.numpy()
    np.savez_compressed(os.path.join(HERE, "tiny21_nets.npz"), **out)
    print("tiny21_nets:", len(out), "arrays", sum(v.nbytes for v in out.values()) / 1e6, "MB")


def gen_full():
    ucfg = S.UNET_SD21
    unet, cn = loaded_ref(ucfg)
    x, ctx, hint = make_inputs(2, 8, 8, ctx_dim=ucfg.context_dim)
    t = torch.tensor([801, 1], dtype=torch.long)
    with torch.no_grad(), G.quiet():
        ctrl = cn(x=x, hint=hint, timesteps=t, context=ctx)
        eps = unet(x=x, timesteps=t, context=ctx, control=[c.clone() for c in ctrl], only_mid_control=False)
    out = {f"control{i}": c.numpy() for i, c in enumerate(ctrl)}
    out["eps"] = eps.numpy()
    np.savez_compressed(os.path.join(HERE, "sd21_lat8.npz"), **out)
    print("sd21_lat8:", len(out), "arrays", sum(v.nbytes for v in out.values()) / 1e6, "MB")


def gen_shapes():
    """tests/shape_cases.py SD21_SHAPES on the full UNET_SD21 nets (every row its own x / context / hint / t), stored like
    make_golden_full.py --only shapes; the project's oracle runs on the same inputs and must agree to 1e-4 of max|eps|."""
    from make_golden_full import store_pass
    from oracle import sd_oracle as O
    from tests import shape_cases as SC
    ucfg = S.UNET_SD21
    unet, cn = loaded_ref(ucfg)
    up, cp, hc = S.unet_plan(ucfg), S.unet_plan(ucfg, False), S.hint_block_convs(ucfg)
    su, sc = unet.state_dict(), cn.state_dict()
    out = {}
    for c in SC.SD21_SHAPES:
        x, ctx, hint, t = SC.case_inputs(c, ctx_dim=ucfg.context_dim)
        with torch.no_grad(), G.quiet():
            ctrl = cn(x=x, hint=hint, timesteps=t, context=ctx)
            eps = unet(x=x, timesteps=t, context=ctx, control=[k.clone() for k in ctrl], only_mid_control=False)
            eps_o = O.apply_model(su, sc, up, cp, hc, x, t, ctx, hint, [1.0] * 13)
        d = float((eps_o - eps).abs().max() / eps.abs().max())
        print(f"sd21_shapes {c.tag}: |eps|max {float(eps.abs().max()):.3f}, oracle vs reference max|diff|/max|eps| = {d:.2e}", flush=True)
        assert d <= 1e-4, f"{c.tag}: the oracle is {d:.2e} of max|eps| away from the reference"
        store_pass(out, c.tag, ctrl, eps)
    p = os.path.join(HERE, "sd21_shapes.npz")
    np.savez_compressed(p, **out)
    print("sd21_shapes:", len(out), "arrays", f"{os.path.getsize(p) / 2**20:.3f} MiB")
    assert os.path.getsize(p) < 2**20


def gen_sampler():
    """The reference DDIMSampler on a stub model with parameterization = "v".  LatentDiffusion's predict_eps_from_z_and_v /
    predict_start_from_z_and_v are absent from the reference tree: the stub carries the upstream restatements."""
    from cldm.ddim_hacked import DDIMSampler
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    class Harness(DDIMSampler):
        def register_buffer(self, name, attr):   # the reference forces .to("cuda") (`ddim_hacked.py:17-21`)
            setattr(self, name, attr)

    betas_np = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    ac = np.cumprod(1.0 - betas_np, axis=0)

    class VModel:
        num_timesteps = 1000
        parameterization = "v"
        device = torch.device("cpu")
        betas = torch.tensor(betas_np, dtype=torch.float32)
        alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
        alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32)
        sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)
        sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32)

        def __init__(self):
            self.calls = []

        def predict_start_from_z_and_v(self, x_t, t, v):
            return (self.sqrt_alphas_cumprod[t].reshape(-1, 1, 1, 1) * x_t
                    - self.sqrt_one_minus_alphas_cumprod[t].reshape(-1, 1, 1, 1) * v)

        def predict_eps_from_z_and_v(self, x_t, t, v):
            return (self.sqrt_alphas_cumprod[t].reshape(-1, 1, 1, 1) * v
                    + self.sqrt_one_minus_alphas_cumprod[t].reshape(-1, 1, 1, 1) * x_t)

    class Analytic(VModel):
        def apply_model(self, x, t, c):          # the analytic model of make_golden.gen_sampler
            k = c["c_crossattn"][0]
            out = torch.tanh(x * k) * 0.7 + 0.1 * torch.sin(t.float() / 100.0)[:, None, None, None] * x.roll(1, -1)
            self.calls.append(out.numpy().copy())
            return out

    out = {}
    cond = {"c_crossattn": [torch.full((2, 1, 1, 1), 0.9)], "c_concat": None}
    unc = {"c_crossattn": [torch.full((2, 1, 1, 1), -0.4)], "c_concat": None}
    Sn = 10
    for scale in (1.0, 9.0):
        for eta in (0.0, 0.5):
            model = Analytic()
            sampler = Harness(model)
            x_T = randn((2, 4, 8, 8), X_T_SEED)
            torch.manual_seed(G.ETA_SEED)
            with G.quiet():
                x0, inter = sampler.sample(Sn, 2, (4, 8, 8), cond, verbose=False, eta=eta, x_T=x_T, log_every_t=1,
                                           unconditional_guidance_scale=scale, unconditional_conditioning=unc)
            tag = f"S{Sn}_scale{scale:g}_eta{eta:g}"
            out[f"{tag}.x0"] = x0.numpy()
            out[f"{tag}.x_inter"] = torch.stack(inter["x_inter"]).numpy()
            out[f"{tag}.pred_x0"] = torch.stack(inter["pred_x0"]).numpy()
            calls = np.stack(model.calls)                    # scale 1: one call per step; else (cond, uncond) per step
            if scale == 1.0:
                out[f"{tag}.v_c"] = calls
            else:
                out[f"{tag}.v_c"], out[f"{tag}.v_u"] = calls[0::2], calls[1::2]
            # the per-step noise is torch.randn(shape) from the global CPU generator, drawn at every step whatever sigma is
            # (`ddim_hacked.py:227`): replay the draws
            torch.manual_seed(G.ETA_SEED)
            out[f"{tag}.noise"] = torch.stack([torch.randn((2, 4, 8, 8)) for _ in range(Sn)]).numpy()
            out[f"{tag}.sigmas"] = np.asarray(sampler.ddim_sigmas, dtype=np.float64)
    out[f"S{Sn}.timesteps"] = np.asarray(sampler.ddim_timesteps)
    out[f"S{Sn}.alphas"] = np.asarray(sampler.ddim_alphas, dtype=np.float64)
    out[f"S{Sn}.alphas_prev"] = np.asarray(sampler.ddim_alphas_prev, dtype=np.float64)
    out[f"S{Sn}.sqrt_one_minus_alphas"] = np.asarray(sampler.ddim_sqrt_one_minus_alphas, dtype=np.float64)

    # the reference sampler over the reference tiny21 nets (ControlLDM.apply_model, `cldm/cldm.py:328-341`, control scales 1)
    ucfg = S.UNET_TINY21
    unet, cn = loaded_ref(ucfg)

    class Nets(VModel):
        def apply_model(self, x, t, c):
            ctx = torch.cat(c["c_crossattn"], 1)
            with G.quiet():
                control = cn(x=x, hint=torch.cat(c["c_concat"], 1), timesteps=t, context=ctx)
                return unet(x=x, timesteps=t, context=ctx, control=control, only_mid_control=False)

    b, h, w = 1, 8, 8
    x_T = randn((b, 4, h, w), X_T_SEED)
    ctx_c, ctx_u = randn((b, 77, ucfg.context_dim), 1), randn((b, 77, ucfg.context_dim), 2)
    hint = make_hint(b, 8 * h, 8 * w)
    sampler = Harness(Nets())
    with G.quiet():
        x0, inter = sampler.sample(4, b, (4, h, w), {"c_concat": [hint], "c_crossattn": [ctx_c]}, verbose=False, eta=0.0, x_T=x_T,
                                   log_every_t=1, unconditional_guidance_scale=7.5,
                                   unconditional_conditioning={"c_concat": [hint], "c_crossattn": [ctx_u]})
    out["tiny21v_S4.x0"] = x0.numpy()
    out["tiny21v_S4.x_inter"] = torch.stack(inter["x_inter"]).numpy()
    out["tiny21v_S4.pred_x0"] = torch.stack(inter["pred_x0"]).numpy()
    np.savez_compressed(os.path.join(HERE, "sampler_v.npz"), **out)
    print("sampler_v:", len(out), "arrays", sum(v.nbytes for v in out.values()) / 1e6, "MB")


OPENCLIP_PROMPTS = ("a photograph of a bird on a branch, best quality", "lowres")


def openclip_tokens(cfg: S.ClipConfig):
    """Seeded token ids of two prompts of 11 and 3 tokens: BOS, words, EOS, then the pad tail = 0 (as open_clip.tokenize pads)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    ids = torch.zeros((2, cfg.positions), dtype=torch.long)
    for i, n in enumerate((11, 3)):
        ids[i, 0] = cfg.vocab - 2
        ids[i, 1:n - 1] = torch.randint(1, cfg.vocab - 2, (n - 2,), generator=g)
        ids[i, n - 1] = cfg.vocab - 1
    return ids


def gen_openclip():
    stubs = {k: sys.modules.pop(k) for k in ("torchvision", "torchvision.utils") if k in sys.modules}      # transformers probes the real one
    from transformers import CLIPTextConfig, CLIPTextModel
    sys.modules.update(stubs)
    cfg = S.CLIP_TINY21
    hf = CLIPTextConfig(vocab_size=cfg.vocab, max_position_embeddings=cfg.positions, hidden_size=cfg.width, num_hidden_layers=cfg.layers,
                        num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, hidden_act="gelu", layer_norm_eps=1e-5,
                        bos_token_id=cfg.vocab - 2, eos_token_id=cfg.vocab - 1, pad_token_id=0, projection_dim=cfg.width)
    model = CLIPTextModel(hf).eval()
    sd = S.synth_state_dict(S.param_spec_clip(cfg), 0, S.NS_CLIP)
    prefixed = any(n.startswith("text_model.") for n in model.state_dict())       # depends on the transformers version
    model.load_state_dict({("text_model." + k if prefixed else k): v for k, v in sd.items()}, strict=False)
    for k, v in model.state_dict().items():          # strict=False must not have skipped a tensor
        if torch.is_floating_point(v):
            assert torch.equal(v, sd[k.split("text_model.")[-1]]), k
    ids = openclip_tokens(cfg)
    final_ln = (model.text_model if prefixed else model).final_layer_norm
    with torch.no_grad():
        o = model(input_ids=ids, output_hidden_states=True)
        pen = final_ln(o.hidden_states[-2])
        assert torch.equal(final_ln(o.hidden_states[-1]), o.last_hidden_state)
    out = {"tokens": ids.numpy().astype(np.int32), "last": o.last_hidden_state.numpy(), "penultimate": pen.numpy()}
    np.savez_compressed(os.path.join(HERE, "openclip_tiny.npz"), **out)
    print("openclip_tiny:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    G.install_stubs()
    torch.set_grad_enabled(False)
    steps = {"manifest": gen_manifest, "tiny": gen_tiny_nets, "sampler": gen_sampler, "openclip": gen_openclip, "full": gen_full,
             "shapes": gen_shapes}
    for k, fn in steps.items():
        if a.only and k not in a.only.split(","):
            continue
        fn()
