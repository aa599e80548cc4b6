"""`ldm/modules/encoders/modules.py` mirror: FrozenCLIPEmbedder and FrozenOpenCLIPEmbedder on the HIP path.

The reference class (`ldm/modules/encoders/modules.py:90-141`) owns a HuggingFace tokenizer and `CLIPTextModel`, both
fetched by name from the hub.  Here the transformer runs through libsdeo.so (`sdeo_clip_*`); the tokenizer stays on the
host and is loaded from LOCAL files only (`version` = a directory holding vocab.json / merges.txt) -- there is no network
access at run time.  Without such files construction FAILS unless the caller opts in to `HashTokenizer`
(`allow_hash_tokenizer=True`: deterministic, NOT CLIP's BPE -- plumbing for synthetic weights only; loading real weights
next to it warns, because crc32 ids index the real embedding table at meaningless rows)."""
from __future__ import annotations

import os
import re
import warnings
import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from .... import spec as S
from ....runtime import ClipRuntime


class AbstractEncoder:
    def encode(self, *args, **kwargs):
        raise NotImplementedError


class HashTokenizer:
    """BOS + one id per lower-cased word / punctuation mark (crc32 mod vocab) + EOS, padded with EOS to max_length --
    the shape and padding convention of `CLIPTokenizer(..., padding="max_length", truncation=True)`
    (`ldm/modules/encoders/modules.py:124-125`), not its byte-pair vocabulary."""

    def __init__(self, vocab: int = 49408, max_length: int = 77, pad: Optional[int] = None):
        """pad: id of the padding tail (None = EOS, CLIPTokenizer's; 0 = `open_clip.tokenize`'s)"""
        self.vocab, self.max_length = vocab, max_length
        self.bos, self.eos = vocab - 2, vocab - 1
        self.pad = self.eos if pad is None else int(pad)

    def __call__(self, texts: Sequence[str]) -> np.ndarray:
        out = np.full((len(texts), self.max_length), self.pad, dtype=np.int32)
        for i, t in enumerate(texts):
            words = re.findall(r"[a-z0-9]+|[^\sa-z0-9]", t.lower())
            ids = [self.bos] + [zlib.crc32(w.encode()) % (self.vocab - 2) for w in words][: self.max_length - 2] + [self.eos]
            out[i, : len(ids)] = ids
        return out


class FrozenCLIPEmbedder(AbstractEncoder):
    """Uses the CLIP transformer encoder for text; `forward(text)` returns `last_hidden_state` [B, 77, 768] (fp32, device)."""
    LAYERS = ["last"]      # the reference also lists "pooled" / "hidden"; cldm_v15 uses the default "last"

    def __init__(self, version: Optional[str] = None, device="cuda", max_length=77, freeze=True, layer="last", layer_idx=None,
                 config: S.ClipConfig = S.CLIP_SD15, runtime: Optional[ClipRuntime] = None, allow_hash_tokenizer: bool = False):
        if layer not in self.LAYERS:
            raise NotImplementedError(f"layer={layer!r}: only 'last' is built (what cldm_v15.yaml uses)")
        self.device = device
        self.max_length = max_length
        self.layer, self.layer_idx = layer, layer_idx
        self.config = config
        self.tokenizer = None
        if version is not None and os.path.isdir(version):
            from transformers import CLIPTokenizer
            self.tokenizer = CLIPTokenizer.from_pretrained(version, local_files_only=True)
        if self.tokenizer is None:
            if not allow_hash_tokenizer:
                raise RuntimeError(
                    f"FrozenCLIPEmbedder: no local CLIP tokenizer at version={version!r} (a directory with vocab.json + merges.txt is "
                    f"needed; the reference's default 'openai/clip-vit-large-patch14' is a hub name and there is no network). "
                    f"Pass allow_hash_tokenizer=True to use the crc32 stand-in -- token ids are then NOT CLIP's BPE ids, which is only "
                    f"meaningful with synthetic weights.")
            self.tokenizer = HashTokenizer(config.vocab, max_length)
        self.transformer = runtime if runtime is not None else ClipRuntime(config)

    def freeze(self):
        return self

    def load_state_dict(self, sd, strict=False):
        if isinstance(self.tokenizer, HashTokenizer) and len(sd):
            warnings.warn("FrozenCLIPEmbedder: checkpoint weights loaded next to the HashTokenizer stand-in: prompts are hashed, not "
                          "BPE-tokenised, so the conditioning is meaningless for real weights (supply version=<tokenizer dir>)",
                          RuntimeWarning, stacklevel=2)
        self.transformer.load_state_dict(sd, strict=strict)
        return self

    def tokenize(self, text: List[str]) -> torch.Tensor:
        if isinstance(self.tokenizer, HashTokenizer):
            ids = self.tokenizer(text)
        else:
            ids = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                 return_overflowing_tokens=False, padding="max_length", return_tensors="np")["input_ids"]
        return torch.from_numpy(np.asarray(ids, dtype=np.int64))

    def forward(self, text):
        if isinstance(text, str):
            text = [text]
        return self.transformer.encode(self.tokenize(list(text)))

    __call__ = forward

    def encode(self, text):
        return self(text)


class FrozenOpenCLIPEmbedder(AbstractEncoder):
    """Uses the OpenCLIP transformer encoder for text (`ldm/modules/encoders/modules.py:147-206`, the SD-2.x cond_stage_model):
    `forward(text)` returns ln_final of the last (layer="last") or last-but-one (layer="penultimate", what cldm_v21.yaml asks for)
    residual block, [B, 77, width] fp32 on the device.  The tower runs through libsdeo.so as `ClipRuntime` with erf GELU and
    `layer_idx` skipped blocks.  `arch` / `version` name a hub model in the reference; here `version` is a LOCAL directory with CLIP's
    vocab.json / merges.txt (OpenCLIP tokenises with the same byte-pair vocabulary, then pads with 0 instead of EOS), and the width /
    depth come from `config`.  The `open_clip` package is not used: its own text clean-up (ftfy, html unescape) is not restated, so
    prompts with markup or mis-encoded characters may tokenise differently."""
    LAYERS = ["last", "penultimate"]

    def __init__(self, arch="ViT-H-14", version: Optional[str] = None, device="cuda", max_length=77, freeze=True, layer="last",
                 config: S.ClipConfig = S.CLIP_SD21, runtime: Optional[ClipRuntime] = None, allow_hash_tokenizer: bool = False):
        assert layer in self.LAYERS
        self.arch = arch
        self.device = device
        self.max_length = max_length
        self.layer = layer
        self.layer_idx = {"last": 0, "penultimate": 1}[layer]
        self.config = config
        self.tokenizer = None
        if version is not None and os.path.isdir(version):
            from transformers import CLIPTokenizer
            self.tokenizer = CLIPTokenizer.from_pretrained(version, local_files_only=True)
        if self.tokenizer is None:
            if not allow_hash_tokenizer:
                raise RuntimeError(
                    f"FrozenOpenCLIPEmbedder: no local CLIP tokenizer at version={version!r} (a directory with vocab.json + merges.txt is "
                    f"needed; the reference's default {arch!r} / 'laion2b_s32b_b79k' are hub names and there is no network).  Pass "
                    f"allow_hash_tokenizer=True to use the crc32 stand-in -- token ids are then NOT byte-pair ids, which is only "
                    f"meaningful with synthetic weights.")
            self.tokenizer = HashTokenizer(config.vocab, max_length, pad=0)
        if runtime is not None and runtime.variant != (1, self.layer_idx):
            raise ValueError(f"FrozenOpenCLIPEmbedder(layer={layer!r}) needs a ClipRuntime of variant {(1, self.layer_idx)}, got {runtime.variant}")
        self.transformer = runtime if runtime is not None else ClipRuntime(config, variant=(1, self.layer_idx))
        self.model = self.transformer          # the reference keeps its tower in `.model`

    def freeze(self):
        return self

    def load_state_dict(self, sd, strict=False):
        if isinstance(self.tokenizer, HashTokenizer) and len(sd):
            warnings.warn("FrozenOpenCLIPEmbedder: checkpoint weights loaded next to the HashTokenizer stand-in: prompts are hashed, not "
                          "BPE-tokenised, so the conditioning is meaningless for real weights (supply version=<tokenizer dir>)",
                          RuntimeWarning, stacklevel=2)
        self.transformer.load_state_dict(sd, strict=strict)
        return self

    def tokenize(self, text: List[str]) -> torch.Tensor:
        """`open_clip.tokenize`: SOT + byte-pair ids + EOT, cut to max_length with EOT last, the tail padded with 0"""
        if isinstance(self.tokenizer, HashTokenizer):
            return torch.from_numpy(np.asarray(self.tokenizer(text), dtype=np.int64))
        rows = self.tokenizer(text, truncation=True, max_length=self.max_length, padding=False)["input_ids"]
        ids = np.zeros((len(rows), self.max_length), dtype=np.int64)
        for i, r in enumerate(rows):
            ids[i, : len(r)] = r
        return torch.from_numpy(ids)

    def forward(self, text):
        if isinstance(text, str):
            text = [text]
        return self.encode_with_transformer(self.tokenize(list(text)))

    __call__ = forward

    def encode_with_transformer(self, tokens):
        return self.transformer.encode(tokens)

    def encode(self, text):
        return self(text)


class FrozenCLIPImageEmbedder(AbstractEncoder):
    """The CLIP image encoder of an image prompt (IP-Adapter's `image_encoder`: HuggingFace `CLIPVisionModelWithProjection`, OpenCLIP
    ViT-H/14) on the HIP path: `forward(images)` takes one (H, W, 3) uint8 RGB picture or a list of them, of any sizes, and returns
    `image_embeds` [B, proj] fp32 on the device.  `CLIPImageProcessor` (PIL bicubic resize, centre crop, normalisation) and the tower
    both run through libsdeo.so (`ClipVisionRuntime`).  `version` names a hub model in upstream code and is ignored here: the weights
    come from `load_state_dict` (a state dict, or the path of a local `model.safetensors`); there is no network access."""

    def __init__(self, version: Optional[str] = None, device="cuda", freeze=True, config: S.ClipVisionConfig = S.CLIP_VISION_H14,
                 runtime=None, want_hidden: bool = False):
        from ....runtime import ClipVisionRuntime
        self.device = device
        self.config = config
        self.transformer = runtime if runtime is not None else ClipVisionRuntime(config, device if device != "cuda" else None, want_hidden=want_hidden)

    def freeze(self):
        return self

    @staticmethod
    def read_state_dict(sd):
        """`sd` itself when it is a dict, else the tensors of the file at that path (.safetensors or a torch checkpoint)"""
        if isinstance(sd, dict):
            return sd
        from ....cldm.model import load_state_dict
        return load_state_dict(os.fspath(sd))

    def load_state_dict(self, sd, strict=False):
        """a `CLIPVisionModelWithProjection` state dict (`vision_model.*`, `visual_projection.weight`) or the path of IP-Adapter's
        `image_encoder/model.safetensors`"""
        self.transformer.load_state_dict(self.read_state_dict(sd), strict=strict)
        return self

    def forward(self, images):
        if not isinstance(images, (list, tuple)):
            images = [images]
        return self.transformer.encode_images(list(images))

    __call__ = forward

    def encode(self, images):
        return self(images)

    def _need_hidden(self):
        if not self.transformer.want_hidden:
            raise RuntimeError("hidden_states[-2] needs a tower configured with want_hidden: FrozenCLIPImageEmbedder(..., want_hidden=True)")

    def hidden(self, images):
        """hidden_states[-2] [B, tokens, width] fp32 on the device of one picture or a list of them: what the Resampler projection of
        the IP-Adapter "plus" files reads (the tower must have been built with want_hidden)"""
        self._need_hidden()
        if not isinstance(images, (list, tuple)):
            images = [images]
        return self.transformer.encode_images(list(images))[1]

    def hidden_of_zero_pixels(self):
        """hidden_states[-2] [1, tokens, width] of an all-zero `pixel_values`: the "plus" adapters' unconditional image prompt.  It
        depends on the weights only."""
        self._need_hidden()
        s = self.config.image
        return self.transformer.encode_pixels(torch.zeros((1, 3, s, s), dtype=torch.float32, device=self.transformer.device))[1]
