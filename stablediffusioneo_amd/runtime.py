"""Python owner of one libsdeo handle (one per process / GPU): configuration, weight upload and the
net-level calls.  Device memory for inputs/outputs is borrowed from torch; all arithmetic is in libsdeo."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence

import torch

from . import _lib, spec as S
from ._lib import SdeoConfig, check, cur_stream, ptr

# the flags of include/sdeo.h, read from it like every other constant
HINT_CACHED, CONTEXT_CACHED, NO_CONTROL = (_lib.header_constant("SDEO_" + n) for n in ("HINT_CACHED", "CONTEXT_CACHED", "NO_CONTROL"))
STEP_LATENT_STAGED, STEP_HINT_SHARED, STEP_V_PREDICTION, STEP_UNGUIDED = (
    _lib.header_constant("SDEO_STEP_" + n) for n in ("LATENT_STAGED", "HINT_SHARED", "V_PREDICTION", "UNGUIDED"))


def TIMESTEP_ROW(i: int) -> int:
    """SDEO_TIMESTEP_ROW(i) of include/sdeo.h (a function-like macro, so restated): run at row i of the table set with `set_timestep_table`"""
    return 8 | (int(i) << 8)


# rows of the library's timestep table (SDEO_MAX_TABLE_STEPS of include/sdeo.h): `set_timestep_table` refuses a longer schedule, so the
# samplers keep the per-step loop, which needs no table, for one
MAX_TABLE_STEPS = _lib.header_constant("SDEO_MAX_TABLE_STEPS")


# control modes of `SdeoRuntime.set_control_mode` (SDEO_CONTROL_* of include/sdeo.h)
CONTROL_BOTH, CONTROL_COND, CONTROL_OFF = (_lib.header_constant("SDEO_CONTROL_" + n) for n in ("BOTH", "COND", "OFF"))


# cap of the four FreeU values (SDEO_FREEU_MAX of include/sdeo.h)
FREEU_MAX = _lib.header_constant("SDEO_FREEU_MAX")


def freeu_args(b1, b2, s1, s2, version=2):
    """(b1, b2, s1, s2, version) as floats and an int after the checks `sdeo_set_freeu` makes, made here first so that a refusal names
    the argument as a ValueError whether or not a device is there; also takes one sequence of four or five as `b1`."""
    if isinstance(b1, (tuple, list)) and b2 is None and s1 is None and s2 is None:
        if len(b1) not in (4, 5):
            raise ValueError(f"freeu: expected (b1, b2, s1, s2[, version]), got {len(b1)} values")
        seq = tuple(b1)
        b1, b2, s1, s2 = seq[:4]
        version = seq[4] if len(seq) == 5 else version
    vals = []
    for name, v in (("b1", b1), ("b2", b2), ("s1", s1), ("s2", s2)):
        if v is None or isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"freeu: {name} must be a number, got {v!r} (there are no default values)")
        v = float(v)
        if v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"freeu: {name} = {v} is not finite")
        if v < 0:
            raise ValueError(f"freeu: {name} = {v} is negative")
        if v > FREEU_MAX:
            raise ValueError(f"freeu: {name} = {v} is above the cap of {FREEU_MAX}")
        vals.append(v)
    if isinstance(version, bool) or not isinstance(version, int) or version not in (1, 2):
        raise ValueError(f"freeu: version must be 1 (constant backbone factor) or 2 (mean-map factor), got {version!r}")
    return (*vals, int(version))


def make_config(ucfg: S.UNetConfig = S.UNET_SD15, vcfg: S.VAEConfig = S.VAE_SD15) -> SdeoConfig:
    c = SdeoConfig()
    c.in_channels, c.out_channels, c.hint_channels = ucfg.in_channels, ucfg.out_channels, ucfg.hint_channels
    c.model_channels, c.num_res_blocks = ucfg.model_channels, ucfg.num_res_blocks
    for i, m in enumerate(ucfg.channel_mult):
        c.channel_mult[i] = m
    c.num_levels = len(ucfg.channel_mult)
    for i, a in enumerate(ucfg.attention_resolutions):
        c.attention_resolutions[i] = a
    c.num_attention_resolutions = len(ucfg.attention_resolutions)
    c.num_heads, c.context_dim, c.context_len = ucfg.num_heads, ucfg.context_dim, ucfg.context_len
    c.vae_ch, c.vae_out_ch = vcfg.ch, vcfg.out_ch
    for i, m in enumerate(vcfg.ch_mult):
        c.vae_ch_mult[i] = m
    c.vae_num_levels, c.vae_num_res_blocks, c.vae_z_channels = len(vcfg.ch_mult), vcfg.num_res_blocks, vcfg.z_channels
    c.vae_scale_factor = vcfg.scale_factor
    return c


def make_config_ext(ucfg: S.UNetConfig) -> Optional[_lib.SdeoConfigExt]:
    """sdeo_config_ext for a config of the 2.x layout; None when plain sdeo_create describes it (every 1.5 config)"""
    if ucfg.num_head_channels in (-1, 0) and not ucfg.use_linear_in_transformer:
        return None
    return _lib.SdeoConfigExt(C.sizeof(_lib.SdeoConfigExt), max(0, ucfg.num_head_channels), int(ucfg.use_linear_in_transformer))


class _HandleRuntime:
    """What the owners of a libsdeo handle share: the device, the handle's lifetime and the weight calls.  A subclass names its
    symbol prefix and the length of the dims array its `<prefix>weight_info` fills, and creates the handle in its __init__."""
    _prefix = "sdeo_"
    _ndims = 4

    def __init__(self, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise _lib.SdeoError(f"{type(self).__name__} needs a HIP device (there is no CPU fallback)")
        self.lib = _lib.load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.handle = C.c_void_p()

    def _sym(self, fn: str):
        return getattr(self.lib, self._prefix + fn)

    def _call(self, fn: str, *args, detail: str = ""):
        """check(<prefix><fn>(handle, *args)); a failure is reported as "load_weight", "clip_load_weight", ... + detail"""
        check(self._sym(fn)(self.handle, *args), self._prefix[len("sdeo_"):] + fn + detail)

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self._sym("destroy")(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    def expected_weights(self) -> Dict[str, tuple]:
        out = {}
        name = C.c_char_p()
        dims = (C.c_int64 * self._ndims)()
        nd = C.c_int()
        for i in range(self._sym("num_weights")(self.handle)):
            self._call("weight_info", i, C.byref(name), dims, C.byref(nd))
            out[name.value.decode()] = tuple(int(dims[k]) for k in range(nd.value))
        return out

    def _load_ptr(self, name: str, data_ptr: int, shape, strict: bool = True):
        """fp32 contiguous data of `shape` at `data_ptr`, on the host or on this device"""
        dims = (C.c_int64 * max(len(shape), 1))(*shape)
        self._call("load_weight", name.encode(), C.c_void_p(data_ptr), dims, len(shape), int(strict), detail=f"({name})")

    def load_tensor(self, name: str, t: torch.Tensor, strict: bool = True):
        t = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
        self._load_ptr(name, t.data_ptr(), tuple(t.shape), strict)

    def _finalize(self):
        self._call("finalize_weights")

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """Every floating-point tensor of `sd` through `<prefix>load_weight` (which ignores a name it does not know unless strict), then
        finalize.  The subclasses say which names their door takes."""
        for k, v in sd.items():
            if not torch.is_floating_point(v):
                continue
            self.load_tensor(k, v, strict)
        self._finalize()
        return self

    def device_bytes(self) -> int:
        return int(self._sym("device_bytes")(self.handle))

    # ---------------------------------------------------------------- LoRA adapters (include/sdeo.h: sdeo_lora_*, sdeo_clip_lora_*)
    def _weight_shape(self, name: str):
        if getattr(self, "_expected", None) is None:
            self._expected = self.expected_weights()
        return self._expected.get(name)

    def lora_apply(self, name: str, down: torch.Tensor, up: torch.Tensor, scale: float = 1.0):
        """Merge scale * up @ down into the stored tensor `name` (a registry name of `expected_weights`), on the device and in place.
        down: (rank, in[, kh, kw]) as lora_down.weight; up: (out, rank[, 1, 1]) as lora_up.weight; host or device tensors.  Call
        `lora_commit` after the last apply of a set."""
        shape = self._weight_shape(name)
        if shape is not None and len(shape) >= 2:
            rank = int(down.shape[0]) if down.dim() >= 2 else 0
            fan = 1
            for d in shape[1:]:
                fan *= d
            ok_down = rank >= 1 and down.numel() == rank * fan and (down.dim() == 2 or tuple(down.shape[1:]) == tuple(shape[1:]))
            ok_up = up.dim() >= 2 and up.numel() == shape[0] * rank and tuple(up.shape[:2]) == (shape[0], rank)
            if not (ok_down and ok_up):
                raise ValueError(f"lora_apply({name}): down {tuple(down.shape)} / up {tuple(up.shape)} do not fit the weight {tuple(shape)}: "
                                 f"expected down (rank, {', '.join(str(d) for d in shape[1:])}) and up ({shape[0]}, rank)")
        # (an unknown name or a vector goes through: the library refuses it with its own message)
        down, up = self._keep(down), self._keep(up)
        self._call("lora_apply", name.encode(), ptr(down), ptr(up), int(down.shape[0]) if down.dim() else 0, C.c_float(float(scale)), cur_stream(),
                   detail=f"({name})")

    def _keep(self, t: Optional[torch.Tensor]):
        """an adapter operand as contiguous fp32 where it is (this device) or on the host; None stays None (an absent operand)"""
        if t is None:
            return None
        return t.detach().to(dtype=torch.float32).contiguous() if t.device == self.device else t.detach().to(device="cpu", dtype=torch.float32).contiguous()

    def _adapter_shape(self, name: str):
        """(out, in, kh * kw, the weight's shape) of a matrix / conv weight of this handle, or None (the library refuses the name)"""
        shape = self._weight_shape(name)
        if shape is None or len(shape) < 2:
            return None
        kk = 1
        for d in shape[2:]:
            kk *= d
        return shape[0], shape[1], kk, tuple(shape)

    def loha_apply(self, name: str, w1_a, w1_b, w2_a, w2_b, t1=None, t2=None, scale: float = 1.0):
        """Merge scale * (w1_a @ w1_b) (.) (w2_a @ w2_b) into the stored tensor `name`, on the device and in place (include/sdeo.h:
        sdeo_loha_apply defines the forms).  Plain: w?_a (out, r), w?_b (r, in * kh * kw).  Tucker (t1 and t2 (r, r, kh, kw) given, convs
        with kh * kw > 1): w?_a (r, out), w?_b (r, in).  Host or device tensors.  Call `lora_commit` after the last apply of a set."""
        ops = {"w1_a": w1_a, "w1_b": w1_b, "w2_a": w2_a, "w2_b": w2_b, "t1": t1, "t2": t2}
        info = self._adapter_shape(name)
        tucker = t1 is not None or t2 is not None
        rank = int(w1_b.shape[0]) if w1_b is not None and w1_b.dim() >= 1 else 0
        if info is not None and all(ops[k] is not None for k in ("w1_a", "w1_b", "w2_a", "w2_b")):
            o, i, kk, shape = info
            if tucker:
                want = {"w1_a": (rank, o), "w1_b": (rank, i), "w2_a": (rank, o), "w2_b": (rank, i), "t1": (rank, rank) + shape[2:], "t2": (rank, rank) + shape[2:]}
                ok = kk > 1 and all(ops[k] is not None and tuple(ops[k].shape) == want[k] for k in want)
            else:
                want = {"w1_a": (o, rank), "w1_b": (rank, i * kk), "w2_a": (o, rank), "w2_b": (rank, i * kk)}
                ok = all(tuple(ops[k].shape) == want[k] for k in want)
            if not (ok and rank >= 1):
                raise ValueError(f"loha_apply({name}): the factors {({k: tuple(v.shape) for k, v in ops.items() if v is not None})} do not fit the weight "
                                 f"{shape}: expected {want}" + (" (a Tucker core needs a conv with a filter larger than 1 x 1)" if tucker and kk == 1 else ""))
        kept = {k: self._keep(v) for k, v in ops.items()}
        self._call("loha_apply", name.encode(), *(None if kept[k] is None else ptr(kept[k]) for k in ("w1_a", "w1_b", "w2_a", "w2_b", "t1", "t2")),
                   rank, C.c_float(float(scale)), cur_stream(), detail=f"({name})")

    def lokr_apply(self, name: str, w1=None, w1_a=None, w1_b=None, w2=None, w2_a=None, w2_b=None, t2=None, scale: float = 1.0):
        """Merge scale * kron(w1, w2) into the stored tensor `name` (include/sdeo.h: sdeo_lokr_apply defines the forms).  w1 (Ol, Im)
        whole or as w1_a (Ol, r) @ w1_b (r, Im); w2 (Ok, In[, kh, kw]) whole, as w2_a (Ok, r) @ w2_b (r, In * kh * kw), or in the Tucker
        form t2 (r, r, kh, kw), w2_a (r, Ok), w2_b (r, In); out = Ol * Ok and in = Im * In are read from the shapes.  Host or device
        tensors.  Call `lora_commit` after the last apply of a set."""
        ops = {"w1": w1, "w1_a": w1_a, "w1_b": w1_b, "w2": w2, "w2_a": w2_a, "w2_b": w2_b, "t2": t2}
        info = self._adapter_shape(name)
        dims = lambda t, n: t is not None and t.dim() == n
        rank1 = int(w1_b.shape[0]) if dims(w1_b, 2) else 0
        rank2 = int(w2_b.shape[0]) if dims(w2_b, 2) else 0
        ol = int(w1.shape[0]) if dims(w1, 2) else int(w1_a.shape[0]) if dims(w1_a, 2) else 0
        im = int(w1.shape[1]) if dims(w1, 2) else int(w1_b.shape[1]) if dims(w1_b, 2) else 0
        if info is not None:
            o, i, kk, shape = info
            fits = ol >= 1 and im >= 1 and o % ol == 0 and i % im == 0
            ok_, in_ = (o // ol, i // im) if fits else (0, 0)
            want = {}
            if w1 is not None:
                want["w1"] = (ol, im)
            else:
                want.update({"w1_a": (ol, rank1), "w1_b": (rank1, im)})
            if w2 is not None:
                want["w2"] = (ok_, in_) if kk == 1 and w2.dim() == 2 else (ok_, in_) + shape[2:]
            elif t2 is not None:
                want.update({"w2_a": (rank2, ok_), "w2_b": (rank2, in_), "t2": (rank2, rank2) + shape[2:]})
            else:
                want.update({"w2_a": (ok_, rank2), "w2_b": (rank2, in_ * kk)})
            ok = fits and set(want) == {k for k, v in ops.items() if v is not None} and all(tuple(ops[k].shape) == want[k] for k in want)
            ok = ok and (t2 is None or kk > 1) and ("w1_a" not in want or rank1 >= 1) and ("w2_a" not in want or rank2 >= 1)
            if not ok:
                raise ValueError(f"lokr_apply({name}): the factors {({k: tuple(v.shape) for k, v in ops.items() if v is not None})} do not fit the weight "
                                 f"{shape}: expected one complete form with w1 (Ol, Im) and w2 ({shape[0]} / Ol, {shape[1]} / Im" +
                                 (", " + ", ".join(str(d) for d in shape[2:]) if len(shape) > 2 else "") + ")")
        kept = {k: self._keep(v) for k, v in ops.items()}
        p = lambda k: None if kept[k] is None else ptr(kept[k])
        self._call("lokr_apply", name.encode(), p("w1"), p("w1_a"), p("w1_b"), rank1, p("w2"), p("w2_a"), p("w2_b"), p("t2"), rank2, ol, im,
                   C.c_float(float(scale)), cur_stream(), detail=f"({name})")

    def lora_commit(self):
        """Rebuild what the library derives from the raw weights and invalidate everything computed with the earlier ones: bumps
        `generation`, the key of the samplers' hint / context caches, the timestep table and every captured graph."""
        self._call("lora_commit")
        self.generation += 1

    def lora_clear(self):
        """Restore every tensor an adapter touched (bit for bit), free the saved copies, commit."""
        self._call("lora_clear")
        self.generation += 1

    def lora_touched(self) -> int:
        return int(self._sym("lora_touched")(self.handle))

    def read_weight(self, name: str) -> torch.Tensor:
        """The stored tensor `name` as fp32 in PyTorch layout (the fp16 values the library holds now), on the host."""
        shape = self._weight_shape(name)
        out = torch.empty(shape if shape is not None else (1,), dtype=torch.float32)
        self._call("read_weight", name.encode(), ptr(out), detail=f"({name})")
        return out


class SdeoRuntime(_HandleRuntime):
    """create -> load_state_dict -> configure(n, h, w) -> controlnet / unet / apply_model / vae_decode."""

    def __init__(self, ucfg: S.UNetConfig = S.UNET_SD15, vcfg: S.VAEConfig = S.VAE_SD15, device: Optional[torch.device] = None,
                 weight_bits: int = 16, act_bits: int = 16, mx_min_rows: int = 0, vae_encoder: bool = False,
                 extra_controlnets: int = 0, ip_adapter_tokens: int = 0, control_modes: bool = False):
        """weight_bits = 8: the UNet / ControlNet matrices are packed to fp8 (OCP e4m3fn, per-output-channel power-of-two scale) when
        the weights are finalised (BASELINE configs[4]; the reference's precision switch is `onnx2trt_static_plugin.py:40-42`).
        vae_encoder = True: the handle also expects `first_stage_model.encoder.*` / `quant_conv.*` and runs `vae_encode`.
        extra_controlnets = k (1..3): the handle also expects `control_model_<j>.*` for j = 1..k and every forward sums the residuals
        of all 1 + k control networks (`set_control_hint`, `set_control_scales`).
        ip_adapter_tokens = T (1..64): the handle also expects `...attn2.to_k_ip.weight` / `to_v_ip.weight` of every UNet cross-attention
        (spec.param_spec_ip_adapter) and every forward adds the image term of `set_ip_tokens`, weighted by `set_ip_scale`.
        control_modes = True: `sdeo_enable_control_modes` -- `set_control_mode` may then run each control network on both halves of the
        CFG pair, on the conditional half only, or not at all."""
        super().__init__(device)
        self.ucfg, self.vcfg = ucfg, vcfg
        self._cfg = make_config(ucfg, vcfg)
        self._ext = make_config_ext(ucfg)
        if self._ext is None:
            check(self.lib.sdeo_create(C.byref(self._cfg), C.byref(self.handle)), "sdeo_create")
        else:
            check(self.lib.sdeo_create_ex(C.byref(self._cfg), C.byref(self._ext), C.byref(self.handle)), "sdeo_create_ex")
        self.vae_encoder = bool(vae_encoder)
        if self.vae_encoder:        # before any weight: the weight slab is sized when the encoder registers its tensors
            check(self.lib.sdeo_enable_vae_encoder(self.handle), "enable_vae_encoder")
        self.extra_controlnets = int(extra_controlnets)
        if self.extra_controlnets:  # before any weight, like the encoder
            check(self.lib.sdeo_enable_extra_controlnets(self.handle, self.extra_controlnets), "enable_extra_controlnets")
        # what the library holds for the extra nets: the scales last set, and the generation each hint was set in (0: never)
        self._extra_scales = [None] * self.extra_controlnets
        self._extra_hint_gen = [0] * self.extra_controlnets
        self.ip_adapter_tokens = int(ip_adapter_tokens)
        if self.ip_adapter_tokens:  # before any weight, like the encoder
            check(self.lib.sdeo_enable_ip_adapter(self.handle, self.ip_adapter_tokens), "enable_ip_adapter")
        self.ip_scale = 1.0         # as the library holds it (sdeo_configure resets it to 1): part of every key of a captured graph
        self._freeu = None          # (b1, b2, s1, s2, version) or None = off, as asked of `set_freeu`: kept across `configure`
        self.weight_bits = int(weight_bits)
        if self.weight_bits != 16:
            check(self.lib.sdeo_set_weight_precision(self.handle, self.weight_bits), "set_weight_precision")
        # act_bits = 8: the GEMMs of >= mx_min_rows rows (default 2048) run block-scaled fp8 x fp8 on the fp8 MFMA (sdeo.h)
        self.act_bits = int(act_bits)
        if self.act_bits != 16:
            check(self.lib.sdeo_set_activation_precision(self.handle, self.act_bits, int(mx_min_rows)), "set_activation_precision")
        self.control_modes = bool(control_modes)
        if self.control_modes:      # after the precisions: the library refuses the feature on an fp8 handle by name
            check(self.lib.sdeo_enable_control_modes(self.handle), "enable_control_modes")
        self._modes = [CONTROL_BOTH] * (1 + self.extra_controlnets)    # as the library holds them (sdeo_configure resets them to BOTH)
        self.n = self.h = self.w = 0
        self.n_controls = 13
        # bumped by every sdeo_configure: the library frees and re-plans its arenas / boundary buffers there, so a hipGraph
        # captured under an older generation points into freed memory and must be re-captured, never replayed
        self.generation = 0

    # ---------------------------------------------------------------- weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False, extra_control: Optional[Sequence[Dict[str, torch.Tensor]]] = None):
        """`sd` uses the reference checkpoint names (model.diffusion_model.*, control_model.*, first_stage_model.*).
        Tensors the hot path does not use (CLIP, VAE encoder, EMA ...) are ignored unless strict.
        extra_control: one state dict per extra control network; the tensors named `control_model.*` of dict j - 1 are loaded under
        `control_model_<j>.*` (a whole control_sd15_*.pth dict is accepted: its other tensors are ignored)."""
        extra_control = list(extra_control or [])
        if len(extra_control) != self.extra_controlnets and (extra_control or strict):
            raise _lib.SdeoError(f"load_state_dict: {len(extra_control)} extra control state dicts for {self.extra_controlnets} extra control networks")
        for k, v in sd.items():
            self.load_tensor(k, v, strict)
        for j, esd in enumerate(extra_control, 1):
            for k, v in esd.items():
                if k.startswith(S.NS_CONTROL):
                    self.load_tensor(f"control_model_{j}." + k[len(S.NS_CONTROL):], v, strict)
        self._finalize()

    def load_synthetic(self, seed: int = 0):
        """Seeded synthetic weights, generated tensor by tensor (never holds the full fp32 model on the host)."""
        for name, shape in self.expected_weights().items():
            self.load_tensor(name, S.synth_tensor(name, shape, seed))
        self._finalize()

    def load_synthetic_device(self, seed: int = 0):
        """Synthetic weights drawn on the GPU (device generator) -- fast path for bench.py; NOT reproducible on the
        CPU, so parity tests use load_synthetic instead.  Same distributions as spec.synth_tensor."""
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        for name, shape in self.expected_weights().items():
            leaf = name.rsplit(".", 1)[-1]
            if len(shape) == 1:
                is_norm = any(t in name for t in (".norm", "in_layers.0", "out_layers.0", "out.0", "norm_out"))
                t = torch.randn(shape, generator=g, device=self.device)
                t = 1.0 + 0.1 * t if (leaf == "weight" and is_norm) else 0.02 * t
            else:
                fan_in = 1
                for d in shape[1:]:
                    fan_in *= d
                t = torch.randn(shape, generator=g, device=self.device) * (1.0 / fan_in) ** 0.5
            self._load_ptr(name, t.contiguous().data_ptr(), shape)
        self._finalize()

    # ---------------------------------------------------------------- profiling
    def profile_begin(self):
        check(self.lib.sdeo_profile_begin(self.handle), "profile_begin")

    def profile_end(self):
        import json
        return json.loads(self.lib.sdeo_profile_end(self.handle).decode())

    # ---------------------------------------------------------------- shapes
    def configure(self, n: int, h: int, w: int):
        if (n, h, w) != (self.n, self.h, self.w):
            self._graph_key = None
            self._graphs = None
            self.generation += 1
            self.n = self.h = self.w = 0            # a failed configure leaves the handle unconfigured
            check(self.lib.sdeo_configure(self.handle, n, h, w), "configure")
            self.n, self.h, self.w = n, h, w
            self._extra_scales = [None] * self.extra_controlnets       # the library reset them to 1
            self.ip_scale = 1.0                                        # ... and the weight of the image term
            modes, self._modes = self._modes, [CONTROL_BOTH] * (1 + self.extra_controlnets)   # ... and every control mode to BOTH:
            self.set_control_modes(modes)                              # the runtime keeps them across `configure`, like FreeU
            if self._freeu is not None:                                # ... and turned FreeU off: hand it over again
                self._call("set_freeu", *(C.c_float(v) for v in self._freeu[:4]), self._freeu[4])
        return self

    # ---------------------------------------------------------------- FreeU
    def set_freeu(self, b1=None, b2=None, s1=None, s2=None, version: int = 2):
        """`sdeo_set_freeu`: FreeU (include/sdeo.h defines it) in every following UNet forward and fused step: backbone factors b1 / b2
        and skip filter scales s1 / s2 of the 4 mc / 2 mc-channel decoder stages, version 1 (constant factor) or 2 (mean-map factor, what
        diffusers ships).  `set_freeu(None)`: off (`sdeo_clear_freeu`).  There are no default values.  The values are read at launch, so
        a captured graph bakes them in: `freeu_key` is part of every graph key.  Unlike the library, the runtime keeps the setting across
        `configure`.  Refused (ValueError, nothing changes): a value that is missing, not finite, negative or above FREEU_MAX, a version
        other than 1 or 2."""
        if b1 is None and b2 is None and s1 is None and s2 is None:
            self._call("clear_freeu")
            self._freeu = None
            return self
        key = freeu_args(b1, b2, s1, s2, version)
        self._call("set_freeu", *(C.c_float(v) for v in key[:4]), key[4])
        self._freeu = key
        return self

    def freeu_key(self):
        """what a captured graph bakes in of FreeU: None when off, else (b1, b2, s1, s2, version)"""
        return self._freeu

    # ---------------------------------------------------------------- control modes
    def set_control_mode(self, net: int, mode: int):
        """`sdeo_set_control_mode`: control network `net` (0..extra_controlnets) on every image (CONTROL_BOTH), on the first n / 2 --
        the conditional half of [cond; uncond] -- only (CONTROL_COND), or not at all (CONTROL_OFF), in the following `apply_model` calls
        and fused steps.  Read at launch (a captured step bakes it in: `modes_key` is part of the key of `apply_model_graphed` and of the samplers' captured loops), kept until changed;
        unlike the library, the runtime keeps them across `configure`.  Needs SdeoRuntime(..., control_modes=True)."""
        check(self.lib.sdeo_set_control_mode(self.handle, int(net), int(mode)), "set_control_mode")
        self._modes[int(net)] = int(mode)
        return self

    def set_control_modes(self, modes):
        """one mode per control network (None: all BOTH); only the nets whose mode changes are told"""
        modes = [CONTROL_BOTH] * len(self._modes) if modes is None else [int(m) for m in modes]
        if len(modes) != len(self._modes):
            raise ValueError(f"set_control_modes: {len(modes)} modes for {len(self._modes)} control networks")
        for net, m in enumerate(modes):
            if m != self._modes[net]:
                self.set_control_mode(net, m)
        return self

    def modes_key(self):
        """the control modes as the library holds them: part of every key of a captured graph"""
        return tuple(self._modes)

    # ---------------------------------------------------------------- image-prompt adapter
    def set_ip_tokens(self, tokens):
        """`sdeo_set_ip_tokens`: the image tokens (n, ip_adapter_tokens, context_dim) into the K_ip | V_ip every UNet cross-attention reads.
        Once per image prompt; the result is read by address, so a captured step sees new tokens without re-capture."""
        tokens = self._f32(tokens, (self.n, self.ip_adapter_tokens, self.ucfg.context_dim))
        check(self.lib.sdeo_set_ip_tokens(self.handle, ptr(tokens), cur_stream()), "set_ip_tokens")

    def set_ip_scale(self, scale: float = 1.0):
        """`sdeo_set_ip_scale`: weight of the image term in the following forwards (read at launch: a captured step bakes it in)"""
        check(self.lib.sdeo_set_ip_scale(self.handle, C.c_float(float(scale))), "set_ip_scale")
        self.ip_scale = float(scale)

    def ip_key(self):
        """what a captured graph bakes in of the adapter: whether it is on, and the scale"""
        return (self.ip_adapter_tokens, self.ip_scale)

    # ---------------------------------------------------------------- extra control networks
    def set_control_hint(self, net: int, hint):
        """`sdeo_set_control_hint`: net (1..extra_controlnets)'s hint (n, hint_channels, 8h, 8w) into that net's cached hint features"""
        u = self.ucfg
        hint = self._f32(hint, (self.n, u.hint_channels, 8 * self.h, 8 * self.w))
        check(self.lib.sdeo_set_control_hint(self.handle, int(net), ptr(hint), cur_stream()), "set_control_hint")
        if 1 <= net <= self.extra_controlnets:
            self._extra_hint_gen[net - 1] = self.generation

    def extra_hint_is_set(self, net: int) -> bool:
        """whether net's hint was set under the current configuration"""
        return self._extra_hint_gen[net - 1] == self.generation and self.generation > 0

    def set_control_scales(self, net: int, scales=None):
        """`sdeo_set_control_scales`: net (1..extra_controlnets)'s 13 scales (None: all 1), kept until changed or reconfigured"""
        check(self.lib.sdeo_set_control_scales(self.handle, int(net), self._scales(scales)), "set_control_scales")
        if 1 <= net <= self.extra_controlnets:
            self._extra_scales[net - 1] = tuple(float(s) for s in scales) if scales is not None else None

    def extra_scales_key(self):
        """the extra nets' scales as the library holds them: part of every key of a captured graph (a capture bakes them in)"""
        return tuple(self._extra_scales)

    def control_shapes(self) -> List[tuple]:
        plan = S.unet_plan(self.ucfg, with_decoder=False)
        shp = [(self.n, c, self.h // ds, self.w // ds) for c, ds in zip(plan.input_block_chans, plan.input_block_ds)]
        shp.append(shp[-1])
        return shp

    # ---------------------------------------------------------------- forward calls
    def _f32(self, t, shape=None):
        if t is None:
            return None
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise _lib.SdeoError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _t64(self, t):
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(t.shape) != (self.n,):
            raise _lib.SdeoError(f"timesteps must have shape ({self.n},)")
        return t

    def _scales(self, scales):
        if scales is None:
            return None
        return (C.c_float * 13)(*[float(s) for s in list(scales) + [1.0] * (13 - len(scales))])

    def controlnet(self, x, hint, t, ctx, flags: int = 0, outs: Optional[Sequence[torch.Tensor]] = None, net: int = 0):
        u = self.ucfg
        x = self._f32(x, (self.n, u.in_channels, self.h, self.w))
        hint = self._f32(hint, (self.n, u.hint_channels, 8 * self.h, 8 * self.w)) if hint is not None else None
        ctx = self._f32(ctx, (self.n, u.context_len, u.context_dim)) if ctx is not None else None
        t = self._t64(t)
        if outs is None:
            outs = [torch.empty(s, dtype=torch.float32, device=self.device) for s in self.control_shapes()]
        arr = (C.c_void_p * 13)(*[o.data_ptr() for o in outs])
        if net == 0:
            check(self.lib.sdeo_controlnet_forward(self.handle, ptr(x), ptr(hint), ptr(t), ptr(ctx), arr, flags, cur_stream()),
                  "controlnet_forward")
        else:
            check(self.lib.sdeo_controlnet_forward_net(self.handle, int(net), ptr(x), ptr(hint), ptr(t), ptr(ctx), arr, flags,
                                                       cur_stream()), "controlnet_forward_net")
            if hint is not None and not (flags & HINT_CACHED) and 1 <= net <= self.extra_controlnets:
                self._extra_hint_gen[net - 1] = self.generation
        return list(outs)

    def unet(self, x, t, ctx, control=None, scales=None, only_mid_control=False, flags: int = 0, out=None):
        u = self.ucfg
        x = self._f32(x, (self.n, u.in_channels, self.h, self.w))
        ctx = self._f32(ctx, (self.n, u.context_len, u.context_dim)) if ctx is not None else None
        t = self._t64(t)
        arr = None
        keep = None
        if control is not None:
            keep = [self._f32(c, s) for c, s in zip(control, self.control_shapes())]
            arr = (C.c_void_p * 13)(*[c.data_ptr() for c in keep])
        eps = out if out is not None else torch.empty((self.n, u.out_channels, self.h, self.w), dtype=torch.float32,
                                                      device=self.device)
        check(self.lib.sdeo_unet_forward(self.handle, ptr(x), ptr(t), ptr(ctx), arr, self._scales(scales),
                                         int(only_mid_control), ptr(eps), flags, cur_stream()), "unet_forward")
        return eps

    def apply_model(self, x, hint, t, ctx, scales=None, only_mid_control=False, flags: int = 0, out=None):
        u = self.ucfg
        x = self._f32(x, (self.n, u.in_channels, self.h, self.w))
        hint = self._f32(hint, (self.n, u.hint_channels, 8 * self.h, 8 * self.w)) if hint is not None else None
        ctx = self._f32(ctx, (self.n, u.context_len, u.context_dim)) if ctx is not None else None
        t = self._t64(t) if t is not None else None          # None: flags carry TIMESTEP_ROW(i)
        if hint is None and not (flags & HINT_CACHED):
            flags |= NO_CONTROL
        eps = out if out is not None else torch.empty((self.n, u.out_channels, self.h, self.w), dtype=torch.float32,
                                                      device=self.device)
        check(self.lib.sdeo_apply_model(self.handle, ptr(x), ptr(hint), ptr(t), ptr(ctx), self._scales(scales),
                                        int(only_mid_control), flags, ptr(eps), cur_stream()), "apply_model")
        return eps

    def apply_model_graphed(self, x, t, scales=None, only_mid_control=False):
        """apply_model with the hint block and context K/V cached, replayed from a hipGraph (the reference captures its
        TensorRT engines the same way, `Engine.py:139-152`).  The graph holds both streams of the step (ControlNet on the
        side stream, UNet encoder on the main one), so the GPU sees the whole fork/join at once.  Inputs are copied into
        fixed device buffers; the returned eps tensor is owned by the runtime (valid until the next call)."""
        key = (self.generation, self.n, self.h, self.w, tuple(float(s) for s in (scales or [])), bool(only_mid_control),
               self.extra_scales_key(), self.ip_key(), self.freeu_key(), self.modes_key())
        if getattr(self, "_graph_key", None) != key:
            u = self.ucfg
            self._gx = torch.zeros((self.n, u.in_channels, self.h, self.w), dtype=torch.float32, device=self.device)
            self._gt = torch.zeros((self.n,), dtype=torch.int64, device=self.device)
            self._geps = torch.zeros((self.n, u.out_channels, self.h, self.w), dtype=torch.float32, device=self.device)
            self._gx.copy_(x)
            self._gt.copy_(t)
            flags = HINT_CACHED | CONTEXT_CACHED
            self.apply_model(self._gx, None, self._gt, None, scales, only_mid_control, flags, self._geps)   # warm-up, eager
            torch.cuda.synchronize(self.device)
            # (measured, tools/step_replay.py: two instances of the capture replayed alternately are SLOWER, 6.91 vs 6.78 ms per
            # step; the host enqueues a replay in 1.6 ms, so the step is GPU-bound and one instance is enough)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.apply_model(self._gx, None, self._gt, None, scales, only_mid_control, flags, self._geps)
            self._graphs, self._graph_key = [g], key
        self._gx.copy_(x)
        self._gt.copy_(t)
        self._graphs[0].replay()
        return self._geps

    def set_timestep_table(self, timesteps) -> int:
        """Hand the sampler's schedule (a host sequence of ints, in the order the loop visits them) to the library: the time
        embeddings of both networks for every step are computed once (`sdeo_set_timestep_table`).  Returns the number of rows."""
        ts = [int(t) for t in timesteps]
        arr = (C.c_int64 * len(ts))(*ts)
        check(self.lib.sdeo_set_timestep_table(self.handle, arr, len(ts), cur_stream()), "set_timestep_table")
        self._table_key = (self.generation, tuple(ts))      # whose schedule the table holds (captured graphs read it by address)
        return len(ts)

    def _step_tensors(self, x, aux, unguided=False):
        """what the six fused steps ask of the latent and of their second state tensor (pred_x0 / d, optional): half the configured
        count of latents for the CFG pair, all of it for an unguided step"""
        assert x.is_contiguous() and x.dtype == torch.float32 and (1 if unguided else 2) * x.shape[0] == self.n
        assert aux is None or (aux.is_contiguous() and aux.dtype == torch.float32 and aux.shape == x.shape)

    @staticmethod
    def _step_flags(staged, hint_shared, v_prediction, flags=0, unguided=False):
        """the SDEO_STEP_* word of a fused step (flags: extra bits as they are)"""
        return (flags | (STEP_LATENT_STAGED if staged else 0) | (STEP_HINT_SHARED if hint_shared else 0)
                | (STEP_V_PREDICTION if v_prediction else 0) | (STEP_UNGUIDED if unguided else 0))

    def ddim_step(self, x, pred_x0, row: int, cfg_scale: float, a_t: float, a_prev: float, sqrt_one_minus_at: float, scales=None,
                  only_mid_control: bool = False, staged: bool = False, hint_shared: bool = False, v_prediction: bool = False,
                  unguided: bool = False, flags: int = 0):
        """`sdeo_ddim_step`: one eta = 0 DDIM step of the CFG pair; x (b,4,h,w) fp32 contiguous is updated in place.
        hint_shared: the cached hints of the unconditional half are those of the conditional half (SDEO_STEP_HINT_SHARED), so the
        ControlNet too computes what precedes its first cross-attention once.  v_prediction: the model predicts v
        (SDEO_STEP_V_PREDICTION).  unguided (here and on the other five steps): SDEO_STEP_UNGUIDED, no guidance -- x holds the configured
        n latents, each runs once and its model output is used as it is; cfg_scale is not read and hint_shared must be off."""
        self._step_tensors(x, pred_x0, unguided)
        flags = self._step_flags(staged, hint_shared, v_prediction, flags, unguided)
        check(self.lib.sdeo_ddim_step(self.handle, ptr(x), ptr(pred_x0), int(row), cfg_scale, a_t, a_prev, sqrt_one_minus_at,
                                      self._scales(scales), int(only_mid_control), flags, cur_stream()), "ddim_step")
        return x

    def dpmpp_2m_step(self, x, d, row: int, cfg_scale: float, a_t: float, sqrt_one_minus_at: float, k_x: float, k_d: float, k_p: float,
                      scales=None, only_mid_control: bool = False, staged: bool = False, hint_shared: bool = False,
                      v_prediction: bool = False, unguided: bool = False, flags: int = 0):
        """`sdeo_dpmpp_2m_step`: one DPM-Solver++(2M) step of the CFG pair, as `ddim_step` with the linear-multistep update
        x <- k_x x + k_d D + k_p d, d <- D; x and d (b,4,h,w) fp32 contiguous are updated in place (d may be None when k_p == 0)."""
        self._step_tensors(x, d, unguided)
        flags = self._step_flags(staged, hint_shared, v_prediction, flags, unguided)
        check(self.lib.sdeo_dpmpp_2m_step(self.handle, ptr(x), ptr(d), int(row), cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p,
                                          self._scales(scales), int(only_mid_control), flags, cur_stream()), "dpmpp_2m_step")
        return x

    def _blend_args(self, x, orig, noise, mask):
        """the operand block the two masked steps share: pointers and the mask's broadcast dims, after the checks ctypes cannot make"""
        from .ops import mask_dims
        for t in (orig, noise):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.shape == x.shape
        assert mask.is_contiguous() and mask.dtype == torch.float32
        mn, mc = mask_dims(mask, x)
        return ptr(orig), ptr(noise), ptr(mask), mn, mc

    def ddim_step_masked(self, x, pred_x0, orig, noise, mask, sqrt_a: float, sqrt_one_minus_a: float, row: int, cfg_scale: float, a_t: float,
                         a_prev: float, sqrt_one_minus_at: float, scales=None, only_mid_control: bool = False, hint_shared: bool = False,
                         v_prediction: bool = False, flags: int = 0, unguided: bool = False):
        """`sdeo_ddim_step_masked`: x <- mask * (sqrt_a orig + sqrt_one_minus_a noise) + (1 - mask) x, then `ddim_step` on it, both in
        place; bit-identical to `ops.mask_blend` followed by the unstaged `ddim_step`.  There is no `staged`: the blend always restages
        (flags: extra SDEO_STEP_* bits as they are, for the tests of what the library refuses)."""
        self._step_tensors(x, pred_x0, unguided)
        flags = self._step_flags(False, hint_shared, v_prediction, flags, unguided)
        check(self.lib.sdeo_ddim_step_masked(self.handle, ptr(x), ptr(pred_x0), *self._blend_args(x, orig, noise, mask), sqrt_a,
                                             sqrt_one_minus_a, int(row), cfg_scale, a_t, a_prev, sqrt_one_minus_at, self._scales(scales),
                                             int(only_mid_control), flags, cur_stream()), "ddim_step_masked")
        return x

    def dpmpp_2m_step_masked(self, x, d, orig, noise, mask, sqrt_a: float, sqrt_one_minus_a: float, row: int, cfg_scale: float, a_t: float,
                             sqrt_one_minus_at: float, k_x: float, k_d: float, k_p: float, scales=None, only_mid_control: bool = False,
                             hint_shared: bool = False, v_prediction: bool = False, flags: int = 0, unguided: bool = False):
        """`sdeo_dpmpp_2m_step_masked`: the blend of `ddim_step_masked`, then `dpmpp_2m_step` on the blended latent"""
        self._step_tensors(x, d, unguided)
        flags = self._step_flags(False, hint_shared, v_prediction, flags, unguided)
        check(self.lib.sdeo_dpmpp_2m_step_masked(self.handle, ptr(x), ptr(d), *self._blend_args(x, orig, noise, mask), sqrt_a,
                                                 sqrt_one_minus_a, int(row), cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p,
                                                 self._scales(scales), int(only_mid_control), flags, cur_stream()), "dpmpp_2m_step_masked")
        return x

    def _eta_args(self, x, noise, orig, mask_noise, mask):
        """the operand block the two stochastic steps share: the step noise row, then the blend operands (all null without a mask).  What
        the library refuses (a missing row, a partial set) is passed through as it is."""
        from .ops import mask_dims
        for t in (noise, orig, mask_noise):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.shape == x.shape)
        mn = mc = 0
        if mask is not None:
            assert mask.is_contiguous() and mask.dtype == torch.float32
            mn, mc = mask_dims(mask, x)
        return ptr(noise), ptr(orig), ptr(mask_noise), ptr(mask), mn, mc

    def ddim_step_eta(self, x, pred_x0, noise, sigma_t: float, row: int, cfg_scale: float, a_t: float, a_prev: float,
                      sqrt_one_minus_at: float, scales=None, only_mid_control: bool = False, staged: bool = False, hint_shared: bool = False,
                      v_prediction: bool = False, orig=None, mask_noise=None, mask=None, sqrt_a: float = 0.0, sqrt_one_minus_a: float = 0.0,
                      flags: int = 0, unguided: bool = False):
        """`sdeo_ddim_step_eta`: `ddim_step` with the sampler's noise term, x <- x_prev + sigma_t * noise (dir_coef = sqrt(1 - a_prev -
        sigma_t^2)), in place; noise (b,4,h,w) fp32 is read by address, so a captured call sees what the row holds at replay.  With orig /
        mask_noise / mask / sqrt_a / sqrt_one_minus_a the blend of `ddim_step_masked` runs in front (no `staged` then).  Bit-identical to
        `apply_model` on [x; x] + `ops.cfg_ddim_step` with the same noise and sigma_t."""
        self._step_tensors(x, pred_x0, unguided)
        pn, po, pm, pk, mn, mc = self._eta_args(x, noise, orig, mask_noise, mask)
        flags = self._step_flags(staged, hint_shared, v_prediction, flags, unguided)
        check(self.lib.sdeo_ddim_step_eta(self.handle, ptr(x), ptr(pred_x0), pn, sigma_t, po, pm, pk, mn, mc, sqrt_a, sqrt_one_minus_a,
                                          int(row), cfg_scale, a_t, a_prev, sqrt_one_minus_at, self._scales(scales), int(only_mid_control),
                                          flags, cur_stream()), "ddim_step_eta")
        return x

    def dpmpp_2m_sde_step(self, x, d, noise, row: int, cfg_scale: float, a_t: float, sqrt_one_minus_at: float, k_x: float, k_d: float,
                          k_p: float, k_n: float, scales=None, only_mid_control: bool = False, staged: bool = False,
                          hint_shared: bool = False, v_prediction: bool = False, orig=None, mask_noise=None, mask=None, sqrt_a: float = 0.0,
                          sqrt_one_minus_a: float = 0.0, flags: int = 0, unguided: bool = False):
        """`sdeo_dpmpp_2m_sde_step`: `dpmpp_2m_step` with the SDE solver's fourth term, x <- k_x x + k_d D + k_p d + k_n noise, d <- D;
        the blend operands as in `ddim_step_eta`"""
        self._step_tensors(x, d, unguided)
        pn, po, pm, pk, mn, mc = self._eta_args(x, noise, orig, mask_noise, mask)
        flags = self._step_flags(staged, hint_shared, v_prediction, flags, unguided)
        check(self.lib.sdeo_dpmpp_2m_sde_step(self.handle, ptr(x), ptr(d), pn, po, pm, pk, mn, mc, sqrt_a, sqrt_one_minus_a, int(row),
                                              cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p, k_n, self._scales(scales),
                                              int(only_mid_control), flags, cur_stream()), "dpmpp_2m_sde_step")
        return x

    def vae_decode(self, z, want_u8: bool = False):
        """z (b,4,h,w) latents (sampler output) -> images (b,3,8h,8w) fp32 in [-1,1] (+ optional NHWC uint8)."""
        v = self.vcfg
        z = self._f32(z)
        b = z.shape[0]
        if tuple(z.shape[1:]) != (v.z_channels, self.h, self.w):
            raise _lib.SdeoError(f"latent shape {tuple(z.shape)} does not match the configured {self.h}x{self.w}")
        img = torch.empty((b, v.out_ch, 8 * self.h, 8 * self.w), dtype=torch.float32, device=self.device)
        u8 = torch.empty((b, 8 * self.h, 8 * self.w, v.out_ch), dtype=torch.uint8, device=self.device) if want_u8 else None
        check(self.lib.sdeo_vae_decode(self.handle, ptr(z), b, ptr(img), ptr(u8), cur_stream()), "vae_decode")
        return (img, u8) if want_u8 else img

    def vae_encode(self, images=None, images_u8=None, noise=None, want_moments: bool = False):
        """encode_first_stage + get_first_stage_encoding: images (b,3,8h,8w) fp32 in [-1,1] OR images_u8 (b,8h,8w,3) uint8 (mapped as
        2 * (u / 255) - 1) -> z (b,4,h,w) fp32 = scale_factor * (mean + std * noise), or scale_factor * mean when noise is None.
        want_moments: also return the quant_conv output (b,8,h,w) fp32 (mean, then logvar, before the clamp)."""
        if not self.vae_encoder:
            raise _lib.SdeoError("vae_encode: this runtime was created without the VAE encoder (SdeoRuntime(..., vae_encoder=True))")
        if (images is None) == (images_u8 is None):
            raise _lib.SdeoError("vae_encode: pass exactly one of images (fp32 NCHW) and images_u8 (uint8 NHWC)")
        v = self.vcfg
        if images is not None:
            images = self._f32(images)
            b = images.shape[0]
            if tuple(images.shape[1:]) != (v.out_ch, 8 * self.h, 8 * self.w):
                raise _lib.SdeoError(f"image shape {tuple(images.shape)} does not match the configured latent {self.h}x{self.w}")
        else:
            images_u8 = images_u8.to(device=self.device, dtype=torch.uint8).contiguous()
            b = images_u8.shape[0]
            if tuple(images_u8.shape[1:]) != (8 * self.h, 8 * self.w, v.out_ch):
                raise _lib.SdeoError(f"image shape {tuple(images_u8.shape)} does not match the configured latent {self.h}x{self.w}")
        if b > self.n:
            raise _lib.SdeoError(f"vae_encode: {b} images, the runtime is configured for {self.n}")
        if noise is not None:
            noise = self._f32(noise, (b, v.z_channels, self.h, self.w))
        z = torch.empty((b, v.z_channels, self.h, self.w), dtype=torch.float32, device=self.device)
        mom = torch.empty((b, 2 * v.z_channels, self.h, self.w), dtype=torch.float32, device=self.device) if want_moments else None
        check(self.lib.sdeo_vae_encode(self.handle, ptr(images), ptr(images_u8), b, ptr(noise), ptr(z), ptr(mom),
                                       cur_stream()), "vae_encode")
        return (z, mom) if want_moments else z


def openclip_to_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Rename the text-tower tensors of an OpenCLIP state dict (`open_clip.model.CLIP`: what `FrozenOpenCLIPEmbedder.model` holds,
    `ldm/modules/encoders/modules.py:160-162`) to the HuggingFace names the library registers.  `attn.in_proj_weight` / `_bias` are the
    fused [3W][W] / [3W] tensors: their thirds are q, k, v.  `text_projection`, `logit_scale`, `attn_mask` and the visual tower have no
    counterpart and are dropped; a dict without OpenCLIP names is returned as it is."""
    if not any("transformer.resblocks." in k and "visual." not in k for k in sd):
        return sd
    out = {}
    blk = {"ln_1.": "layer_norm1.", "ln_2.": "layer_norm2.", "attn.out_proj.": "self_attn.out_proj.", "mlp.c_fc.": "mlp.fc1.",
           "mlp.c_proj.": "mlp.fc2."}
    for k, v in sd.items():
        n = k[len("cond_stage_model."):] if k.startswith("cond_stage_model.") else k
        n = n[len("model."):] if n.startswith("model.") else n
        if n == "token_embedding.weight":
            out["embeddings.token_embedding.weight"] = v
        elif n == "positional_embedding":
            out["embeddings.position_embedding.weight"] = v
        elif n.startswith("ln_final."):
            out["final_layer_norm." + n[len("ln_final."):]] = v
        elif n.startswith("transformer.resblocks."):
            i, rest = n[len("transformer.resblocks."):].split(".", 1)
            p = f"encoder.layers.{i}."
            if rest in ("attn.in_proj_weight", "attn.in_proj_bias"):
                leaf = rest.rsplit("_", 1)[1]
                for name, part in zip(("q_proj", "k_proj", "v_proj"), torch.chunk(v, 3, dim=0)):
                    out[f"{p}self_attn.{name}.{leaf}"] = part
            else:
                for a, b in blk.items():
                    if rest.startswith(a):
                        out[p + b + rest[len(a):]] = v
    return out


class ClipRuntime(_HandleRuntime):
    """CLIP text transformer on the HIP path: create -> load_state_dict -> configure(batch) ->
    encode(tokens).  Mirrors what `FrozenCLIPEmbedder.forward` does after tokenisation
    (`ldm/modules/encoders/modules.py:126-131`: `self.transformer(input_ids=tokens).last_hidden_state`)."""

    _prefix = "sdeo_clip_"
    _ndims = 2

    def __init__(self, cfg: S.ClipConfig = S.CLIP_SD15, device: Optional[torch.device] = None, variant: Optional[tuple] = None):
        """variant = (hidden_act, skip_last_layers) of `sdeo_clip_set_variant`: (1, k) is the OpenCLIP text tower of
        `FrozenOpenCLIPEmbedder` (erf GELU; layer "last" k = 0, "penultimate" k = 1).  None: the call is not made."""
        super().__init__(device)
        self.cfg = cfg
        self._cfg = _lib.SdeoClipConfig(cfg.vocab, cfg.positions, cfg.width, cfg.layers, cfg.heads, cfg.ffn)
        check(self.lib.sdeo_clip_create(C.byref(self._cfg), C.byref(self.handle)), "sdeo_clip_create")
        self.variant = None if variant is None else (int(variant[0]), int(variant[1]))
        if self.variant is not None:
            self._call("set_variant", self.variant[0], self.variant[1])
        self.batch = 0
        self.generation = 0          # bumped by every re-plan of the activation buffers (see SdeoRuntime.generation)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """Accepts HuggingFace names (`text_model.*`, or bare), or the SD checkpoint's `cond_stage_model.transformer.text_model.*`,
        or OpenCLIP's names (bare, or below `model.` / `cond_stage_model.model.` as an SD-2.x checkpoint stores them; see
        `openclip_to_hf`); anything else (e.g. `position_ids`, the UNet tensors of a full checkpoint) is ignored unless strict."""
        return super().load_state_dict(openclip_to_hf(sd), strict)

    def load_synthetic(self, seed: int = 0):
        for name, shape in self.expected_weights().items():
            self.load_tensor(name, S.synth_tensor(S.NS_CLIP + name, shape, seed))
        self._finalize()
        return self

    def configure(self, batch: int):
        if batch != self.batch:
            self.generation += 1
            self.batch = 0
            check(self.lib.sdeo_clip_configure(self.handle, batch), "sdeo_clip_configure")
            self.batch = batch
        return self

    def encode(self, tokens: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens: integer [batch, positions] -> fp32 [batch, positions, width] on the device (into `out` when given)."""
        if tokens.dim() != 2 or tokens.shape[1] != self.cfg.positions:
            raise ValueError(f"tokens must be [batch, {self.cfg.positions}], got {tuple(tokens.shape)}")
        if tokens.shape[0] != self.batch:
            self.configure(int(tokens.shape[0]))
        tok = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        shape = (self.batch, self.cfg.positions, self.cfg.width)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise _lib.SdeoError(f"encode: out must be a contiguous fp32 tensor of shape {shape}")
        check(self.lib.sdeo_clip_encode(self.handle, ptr(tok), self.batch, ptr(out), cur_stream()), "sdeo_clip_encode")
        return out


class ClipVisionRuntime(_HandleRuntime):
    """CLIP vision tower with projection on the HIP path (csrc/clip_vision.hip; HuggingFace `CLIPVisionModelWithProjection`):
    create -> load_state_dict -> configure(batch) -> encode_images(pictures) / encode_pixels(pixel_values).  The preprocessing
    (`CLIPImageProcessor`: PIL bicubic resize, centre crop, normalise) runs on the device too (`preprocess`)."""

    _prefix = "sdeo_clip_vision_"
    _ndims = 4

    def __init__(self, cfg: S.ClipVisionConfig = S.CLIP_VISION_H14, device: Optional[torch.device] = None, want_hidden: bool = False):
        """want_hidden: the encodes also return hidden_states[-2] (batch, tokens, width), the input of a Resampler projection"""
        super().__init__(device)
        self.cfg = cfg
        self._cfg = _lib.SdeoClipVisionConfig(cfg.image, cfg.patch, cfg.width, cfg.layers, cfg.heads, cfg.ffn, cfg.proj)
        check(self.lib.sdeo_clip_vision_create(C.byref(self._cfg), C.byref(self.handle)), "sdeo_clip_vision_create")
        self.want_hidden = bool(want_hidden)
        self.batch = 0
        self.generation = 0
        self._work = None            # the preprocess workspace, grown on demand

    @property
    def kp(self) -> int:
        """columns of a patch row: 3 patch^2 rounded up to a multiple of 8"""
        return (3 * self.cfg.patch ** 2 + 7) // 8 * 8

    def load_weight(self, name: str, t: torch.Tensor, strict: bool = True):
        self.load_tensor(name, t, strict)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """HuggingFace keys of `CLIPVisionModelWithProjection` (`vision_model.*`, `visual_projection.weight`; bare names below
        `vision_model.` are accepted); anything else (`position_ids`, a text tower) is ignored unless strict."""
        return super().load_state_dict(sd, strict)

    def load_synthetic(self, seed: int = 0):
        return self.load_state_dict(S.synth_clip_vision_state_dict(self.cfg, seed), strict=True)

    def configure(self, batch: int):
        if batch != self.batch:
            self.generation += 1
            self.batch = 0
            check(self.lib.sdeo_clip_vision_configure(self.handle, int(batch), int(self.want_hidden)), "sdeo_clip_vision_configure")
            self.batch = batch
        return self

    # ---------------------------------------------------------------- preprocessing
    def _image(self, image) -> torch.Tensor:
        t = torch.from_numpy(image) if not torch.is_tensor(image) else image
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"an image prompt is a uint8 (H, W, 3) RGB image, got {tuple(t.shape)} {t.dtype}")
        return t.to(self.device).contiguous()

    def _tables(self, ih: int, iw: int):
        """(device int32 tensor holding all six tables, the op's table arguments in order) for an ih x iw image"""
        from .annotator.util import clip_preprocess_tables
        import numpy as np
        tb = clip_preprocess_tables(ih, iw, self.cfg.image)
        parts = [tb[k].reshape(-1) for k in ("x_first", "x_count", "x_coeffs", "y_first", "y_count", "y_coeffs")]
        dev = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(self.device)
        offs = [0]
        for p in parts:
            offs.append(offs[-1] + p.size)
        at = lambda i: C.c_void_p(dev.data_ptr() + 4 * offs[i])
        need = int(self.lib.sdeo_clip_image_preprocess_workspace_bytes(ih, iw, self.cfg.image))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        args = (at(0), at(1), at(2), tb["x_taps"], at(3), at(4), at(5), tb["y_taps"], tb["src_row0"], tb["src_rows"], ptr(self._work),
                C.c_size_t(self._work.numel()), cur_stream())
        return dev, args

    def preprocess(self, image, want_crop: bool = False):
        """`sdeo_clip_image_preprocess_u8` on one (H, W, 3) uint8 image (host array or tensor): the fp16 patch rows (patches, Kp), and
        with want_crop the resized-and-cropped uint8 image (S, S, 3), on the device."""
        img = self._image(image)
        c = self.cfg
        rows = torch.empty(((c.image // c.patch) ** 2, self.kp), dtype=torch.float16, device=self.device)
        crop = torch.empty((c.image, c.image, 3), dtype=torch.uint8, device=self.device) if want_crop else None
        keep, args = self._tables(int(img.shape[0]), int(img.shape[1]))
        check(self.lib.sdeo_clip_image_preprocess_u8(ptr(rows), ptr(crop), ptr(img), int(img.shape[0]), int(img.shape[1]), c.image, c.patch, *args),
              "sdeo_clip_image_preprocess_u8")
        return (rows, crop) if want_crop else rows

    def unpatchify(self, rows: torch.Tensor) -> torch.Tensor:
        """patch rows (patches, Kp) -> pixel values (3, S, S), the pad columns dropped (column (py * p + px) * 3 + c)"""
        c = self.cfg
        g, p = c.image // c.patch, c.patch
        return rows[:, :3 * p * p].reshape(g, g, p, p, 3).permute(4, 0, 2, 1, 3).reshape(3, c.image, c.image)

    # ---------------------------------------------------------------- encodes
    def _encode(self):
        c = self.cfg
        out = torch.empty((self.batch, c.proj), dtype=torch.float32, device=self.device)
        hid = torch.empty((self.batch, c.tokens, c.width), dtype=torch.float32, device=self.device) if self.want_hidden else None
        check(self.lib.sdeo_clip_vision_encode(self.handle, self.batch, ptr(out), ptr(hid), cur_stream()), "sdeo_clip_vision_encode")
        return (out, hid) if self.want_hidden else out

    def encode_pixels(self, pixel_values: torch.Tensor):
        """pixel_values (batch, 3, S, S) as `CLIPImageProcessor` returns them -> image_embeds (batch, proj) fp32 on the device, or
        (image_embeds, hidden_states[-2]) with want_hidden"""
        s = self.cfg.image
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, s, s):
            raise ValueError(f"pixel_values must be (batch, 3, {s}, {s}), got {tuple(pixel_values.shape)}")
        self.configure(int(pixel_values.shape[0]))
        pix = pixel_values.to(device=self.device, dtype=torch.float32).contiguous()
        check(self.lib.sdeo_clip_vision_set_pixels(self.handle, ptr(pix), self.batch, cur_stream()), "sdeo_clip_vision_set_pixels")
        return self._encode()

    def encode_images(self, images):
        """images: a list of (H, W, 3) uint8 RGB pictures of any sizes (host arrays or tensors) -> as `encode_pixels`; resize, crop,
        normalisation and patchify run on the device, one picture per slot"""
        images = [self._image(im) for im in images]
        if not images:
            raise ValueError("encode_images: no image")
        self.configure(len(images))
        for slot, img in enumerate(images):
            keep, args = self._tables(int(img.shape[0]), int(img.shape[1]))
            check(self.lib.sdeo_clip_vision_set_image_u8(self.handle, slot, ptr(img), int(img.shape[0]), int(img.shape[1]), *args),
                  "sdeo_clip_vision_set_image_u8")
        return self._encode()


class ResamplerRuntime(_HandleRuntime):
    """The Resampler image projection of the IP-Adapter "plus" files on the HIP path (csrc/resampler.hip): create -> load_state_dict ->
    configure(batch) -> project(hidden).  `hidden` is the vision tower's hidden_states[-2] (`ClipVisionRuntime(want_hidden=True)`), the
    result what `SdeoRuntime.set_ip_tokens` takes; both stay on the device."""

    _prefix = "sdeo_resampler_"
    _ndims = 4

    def __init__(self, cfg: S.ResamplerConfig = S.RESAMPLER_PLUS_SD15, device: Optional[torch.device] = None):
        super().__init__(device)
        self.cfg = cfg
        self._cfg = _lib.SdeoResamplerConfig(cfg.tokens, cfg.embed_dim, cfg.dim, cfg.depth, cfg.dim_head, cfg.heads, cfg.num_queries, cfg.ffn,
                                             cfg.out_dim)
        check(self.lib.sdeo_resampler_create(C.byref(self._cfg), C.byref(self.handle)), "sdeo_resampler_create")
        self.batch = 0
        self.generation = 0

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """the adapter file's `image_proj` group (bare keys, or `image_proj.<key>`); anything else is ignored unless strict"""
        return super().load_state_dict(sd, strict)

    def load_synthetic(self, seed: int = 0):
        return self.load_state_dict(S.synth_resampler_state_dict(self.cfg, seed), strict=True)

    def configure(self, batch: int):
        if batch != self.batch:
            self.generation += 1
            self.batch = 0
            check(self.lib.sdeo_resampler_configure(self.handle, int(batch)), "sdeo_resampler_configure")
            self.batch = batch
        return self

    def num_launches(self) -> int:
        """launches of one `project` at the configured batch"""
        return int(self.lib.sdeo_resampler_num_launches(self.handle))

    def project(self, hidden: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """hidden (batch, tokens, embed_dim) -> image tokens (batch, num_queries, out_dim) fp32 on the device (into `out` when given)"""
        c = self.cfg
        if hidden.dim() != 3 or tuple(hidden.shape[1:]) != (c.tokens, c.embed_dim):
            raise ValueError(f"hidden states of shape {tuple(hidden.shape)}, the Resampler takes (b, {c.tokens}, {c.embed_dim})")
        self.configure(int(hidden.shape[0]))
        hid = hidden.detach().to(device=self.device, dtype=torch.float32).contiguous()
        shape = (self.batch, c.num_queries, c.out_dim)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise _lib.SdeoError(f"project: out must be a contiguous fp32 tensor of shape {shape} on {self.device}")
        check(self.lib.sdeo_resampler_project(self.handle, ptr(hid), self.batch, ptr(out), cur_stream()), "sdeo_resampler_project")
        return out


class HedRuntime(_HandleRuntime):
    """HED soft-edge annotator on the HIP path (`annotator/hed/__init__.py`: ControlNetHED_Apache2 + HEDdetector.__call__):
    create -> load_state_dict -> configure(H, W) -> detect(image).  One image per call; csrc/hed.hip."""

    _prefix = "sdeo_hed_"

    def __init__(self, device: Optional[torch.device] = None):
        super().__init__(device)
        check(self.lib.sdeo_hed_create(C.byref(self.handle)), "sdeo_hed_create")
        self.size = (0, 0)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """The reference state dict / ControlNetHED.pth names (`norm`, `block{1..5}.convs.{i}.*`, `block{1..5}.projection.*`);
        other floating-point tensors are ignored unless strict."""
        super().load_state_dict(sd, strict)
        self.size = (0, 0)
        return self

    def load_synthetic(self, seed: int = 0):
        return self.load_state_dict(S.synth_hed_state_dict(seed), strict=True)

    def configure(self, height: int, width: int):
        if (height, width) != self.size:
            self.size = (0, 0)
            check(self.lib.sdeo_hed_configure(self.handle, height, width), "sdeo_hed_configure")
            self.size = (height, width)
        return self

    def side_shapes(self):
        h, w = self.size
        out = []
        for _ in range(5):
            out.append((h, w))
            h, w = h // 2, w // 2
        return out

    def detect(self, image: torch.Tensor, edges: bool = True, control: bool = False, side: bool = False):
        """image: uint8 (H, W, 3) RGB (host or device) -> dict with "edges" (H, W) uint8, "control" (3, H, W) fp32 = edges / 255,
        "side" [five fp32 (h_k, w_k) maps], each on the device and only when asked for."""
        if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
            raise ValueError(f"HED expects a uint8 (H, W, 3) image, got {tuple(image.shape)} {image.dtype}")
        H, W = int(image.shape[0]), int(image.shape[1])
        self.configure(H, W)
        img = image.to(self.device).contiguous()
        out = {}
        if edges:
            out["edges"] = torch.empty((H, W), dtype=torch.uint8, device=self.device)
        if control:
            out["control"] = torch.empty((3, H, W), dtype=torch.float32, device=self.device)
        sp = (C.c_void_p * 5)()
        if side:
            out["side"] = [torch.empty(s, dtype=torch.float32, device=self.device) for s in self.side_shapes()]
            for k, t in enumerate(out["side"]):
                sp[k] = t.data_ptr()
        check(self.lib.sdeo_hed_detect_u8(self.handle, ptr(img), ptr(out.get("edges")), ptr(out.get("control")), sp if side else None,
                                          cur_stream()), "sdeo_hed_detect_u8")
        return out
