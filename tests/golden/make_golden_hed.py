"""Generate tests/golden/hed.npz by running the REFERENCE's HED network (`annotator/hed/__init__.py`: ControlNetHED_Apache2) on CPU.

Needs the reference tree (build container only).  `annotator.hed` imports cv2, which it uses only in HEDdetector.__call__ and nms();
a stub module stands in for it, and HEDdetector's post-process is restated (tests/hed_oracle.py: fuse).  Weights:
stablediffusioneo_amd.spec.synth_hed_state_dict(0), loaded through the reference module's load_state_dict, whose own [name, shape]
list is stored (it pins spec.param_spec_hed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hed.py

Cases (image source, stored side maps):
    bird     tests/golden/canny.npz "image" (256x384, stored BGR) flipped to RGB     side maps + edges
    odd      tests/encoder_inputs.make_image_u8(1, 104, 168, seed=104)              side maps + edges (not a multiple of 16)
    sq512    tests/encoder_inputs.make_image_u8(1, 512, 512, seed=512)              edges only
Side maps are the reference network's fp32 outputs (pinned); the edge maps are the restated post-process of them (parity unpinned:
cv2 is absent)."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from stablediffusioneo_amd import spec as S      # noqa: E402
from tests import hed_oracle                     # noqa: E402
from tests.encoder_inputs import make_image_u8   # noqa: E402

CASES = {"bird": None, "odd": (104, 168, 104), "sq512": (512, 512, 512)}
SIDE_CASES = ("bird", "odd")


def case_image(name):
    if name == "bird":
        return np.load(os.path.join(HERE, "canny.npz"))["image"][:, :, ::-1].copy()
    h, w, seed = CASES[name]
    return make_image_u8(1, h, w, seed=seed)[0].numpy()


def main():
    sys.modules["cv2"] = types.ModuleType("cv2")
    from annotator.hed import ControlNetHED_Apache2
    torch.manual_seed(0)
    net = ControlNetHED_Apache2().float().eval()
    spec = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    net.load_state_dict(S.synth_hed_state_dict(0))
    out = {"spec": json.dumps(spec)}
    for name in CASES:
        img = case_image(name)
        H, W = img.shape[:2]
        x = torch.from_numpy(img.copy()).float().permute(2, 0, 1)[None]      # HEDdetector: rearrange 'h w c -> 1 c h w'
        with torch.no_grad():
            maps = [e.detach().cpu().numpy().astype(np.float32)[0, 0] for e in net(x)]
        if name in SIDE_CASES:
            for k, m in enumerate(maps):
                out[f"{name}.side{k + 1}"] = m
        out[f"{name}.edges"] = hed_oracle.fuse(maps, H, W)
        print(name, (H, W), [m.shape for m in maps], "edge mean", float(out[f"{name}.edges"].mean()))
    path = os.path.join(HERE, "hed.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
