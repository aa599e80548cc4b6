"""VAE encoder, host side: the expected tensors (stablediffusioneo_amd.spec.param_spec_vae_encoder) against the reference Encoder's
state_dict shapes stored in tests/golden/vae_encoder.npz (tests/golden/make_golden_vae_encoder.py), and the encode path leaves the
default specification alone."""
import json
import os

import numpy as np
import pytest

from stablediffusioneo_amd import spec as S
from tests.common import GOLDEN

PATH = os.path.join(GOLDEN, "vae_encoder.npz")


@pytest.fixture(scope="module")
def gold():
    assert os.path.exists(PATH), "tests/golden/vae_encoder.npz is missing (tests/golden/make_golden_vae_encoder.py)"
    return np.load(PATH)


@pytest.mark.parametrize("tag,cfg", [("sd15", S.VAE_SD15), ("tiny", S.VAE_TINY)])
def test_encoder_spec_matches_reference_encoder(gold, tag, cfg):
    ref = [(k, tuple(v)) for k, v in json.loads(str(gold[f"spec.{tag}"]))]
    mine = [(k, tuple(v)) for k, v in S.param_spec_vae_encoder(cfg).items()]
    assert mine == ref           # names, shapes and state_dict order


def test_encoder_spec_sd15_counts(gold):
    spec = S.param_spec_vae_encoder(S.VAE_SD15)
    assert spec["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert spec["encoder.down.0.downsample.conv.weight"] == (128, 128, 3, 3)
    assert "encoder.down.3.downsample.conv.weight" not in spec
    assert spec["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert spec["quant_conv.weight"] == (8, 8, 1, 1)
    ref = json.loads(str(gold["spec.sd15"]))
    assert S.count_params(spec) == sum(int(np.prod(v)) for _, v in ref) == 34163664


def test_default_specs_do_not_include_the_encoder():
    full = S.param_spec_full()
    assert not any(k.startswith(S.NS_VAE + "encoder.") or k.startswith(S.NS_VAE + "quant_conv") for k in full)
    assert not any(k.startswith("encoder.") or k.startswith("quant_conv") for k in S.param_spec_vae())
    assert len(full) == len(S.param_spec_unet()) + len(S.param_spec_controlnet()) + len(S.param_spec_vae()) == 1166


def test_synthetic_encoder_weights_use_checkpoint_names():
    sd = S.synth_vae_encoder_state_dict(S.VAE_TINY, 0)
    spec = S.param_spec_vae_encoder(S.VAE_TINY)
    assert list(sd) == [S.NS_VAE + k for k in spec]
    k = S.NS_VAE + "encoder.mid.attn_1.q.weight"
    assert np.array_equal(sd[k].numpy(), S.synth_tensor(k, spec["encoder.mid.attn_1.q.weight"], 0).numpy())
