"""Generate tests/golden/dataprep.npz by IMPORTING THE REFERENCE's data path
(model/marginalnet_full_dataset/dataloader.py: FullDataset.__getitem__, _load_attention_map_from_artifact,
GQA_CATEGORY_TO_TRANSFORM).

    ATTWARP_REFERENCE=<checkout of the reference> python tests/golden/make_golden_dataprep.py

The reference imports ``torchvision.transforms``; this script installs a stub with the published behaviour of the three
transforms the data path uses -- ``Resize((h, w), interpolation)`` on a PIL image is ``img.resize((w, h), BILINEAR or
NEAREST)``, ``ToTensor`` is uint8 -> float32 -> ``.div(255)`` channels first, ``Compose`` chains -- so the torchvision
boundary is "published behaviour, unpinned" (DESIGN 4), while Pillow, numpy and torch are the installed ones (versions
recorded in the file).  A handful of tiny samples are written to temporary .png / .npy files and read back through the
reference's ``__getitem__``; the file holds their decoded inputs, what ``_load_attention_map_from_artifact`` returned,
the ``image`` / ``attention_map`` tensors, and the reference's category -> transform table as two arrays of names.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
S = 32


def _stub_torchvision():
    import torch
    from PIL import Image

    class InterpolationMode:
        NEAREST, BILINEAR = "nearest", "bilinear"

    class Resize:
        def __init__(self, size, interpolation=InterpolationMode.BILINEAR):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            h, w = self.size
            return img.resize((w, h), Image.NEAREST if self.interpolation == InterpolationMode.NEAREST else Image.BILINEAR)

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img)
            a = a[:, :, None] if a.ndim == 2 else a
            return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.InterpolationMode, tr.Resize, tr.ToTensor, tr.Compose = InterpolationMode, Resize, ToTensor, Compose
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    return tr


def _load_reference():
    ref = os.environ.get("ATTWARP_REFERENCE")
    if not ref:
        sys.exit("set ATTWARP_REFERENCE to a checkout of the reference")
    path = os.path.join(ref, "model", "marginalnet_full_dataset", "dataloader.py")
    spec = importlib.util.spec_from_file_location("ref_mn_dataloader", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def samples():
    """(dataset, bucket, image uint8 [H,W,3], attention array, kind): kind "npy" = float32 array, "overlay" = uint8 gray image."""
    rng = np.random.default_rng(3100)
    def img(h, w):
        yy, xx = np.mgrid[0:h, 0:w]
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[..., 1] = (127 + 120 * np.sin(xx / 5.0) * np.cos(yy / 7.0)).astype(np.uint8)
        return a
    a0 = rng.random((24, 24), dtype=np.float32)                               # max <= 1: not divided
    a1 = (rng.random((16, 32), dtype=np.float32) * np.float32(7.5))           # max > 1
    a2 = rng.random((10, 13), dtype=np.float32) * np.float32(3.0)             # NaN: nothing is divided; +-inf -> 0
    a2[2, 3], a2[4, 5], a2[6, 7] = np.nan, np.inf, -np.inf
    a3 = rng.integers(0, 256, (16, 16), dtype=np.uint8)                       # overlay: gray / 255
    a3[0, :8] = [0, 1, 2, 127, 128, 254, 255, 85]
    a4 = -rng.random((5, 9), dtype=np.float32)                                # negative and zero
    a4[1] = 0
    return [("gqa", "query_rel", img(37, 91), a0, "npy"), ("textvqa", None, img(64, 48), a1, "npy"),
            ("docvqa", None, img(7, 5), a2, "npy"), ("gqa", "no_such_bucket", img(50, 70), a3, "overlay"),
            ("GQA_val", None, img(33, 20), a4, "npy")]


def main():
    import PIL
    import torch
    from PIL import Image
    tr = _stub_torchvision()
    mod = _load_reference()
    out = {"S": np.array(S), "versions": np.array([f"pillow {PIL.__version__}", f"numpy {np.__version__}", f"torch {torch.__version__}"]),
           "category_names": np.array(list(mod.GQA_CATEGORY_TO_TRANSFORM.keys())),
           "category_transforms": np.array(list(mod.GQA_CATEGORY_TO_TRANSFORM.values()))}
    ds = object.__new__(mod.FullDataset)
    ds.artifact_type, ds.artifact_layer, ds.image_size = "relative", 16, S
    ds.img_transform = tr.Compose([tr.Resize((S, S)), tr.ToTensor()])
    ds.attn_transform = tr.Compose([tr.Resize((S, S), interpolation=tr.InterpolationMode.NEAREST), tr.ToTensor()])
    ds.samples = []
    smp = samples()
    with tempfile.TemporaryDirectory() as tmp:
        for i, (dset, bucket, image, att, kind) in enumerate(smp):
            ip = os.path.join(tmp, f"img{i}.png")
            Image.fromarray(image).save(ip)
            if kind == "npy":
                ap = os.path.join(tmp, f"att{i}.npy")
                np.save(ap, att)
                art = {"type": "relative", "layer": 16, "npy_path": ap}
            else:
                ap = os.path.join(tmp, f"att{i}.png")
                Image.fromarray(att).save(ap)
                art = {"type": "relative", "layer": 16, "overlay_path": ap}
            meta = {"question": f"question {i}?", "answer": f"answer {i}", "image_path": ip, "artifacts": [art]}
            if bucket is not None:
                meta["bucket"] = bucket
            ds.samples.append((meta, dset))
        for i, (dset, bucket, image, att, kind) in enumerate(smp):
            item = ds[i]
            loaded = mod.FullDataset._load_attention_map_from_artifact(ds.samples[i][0]["artifacts"][0])
            out[f"image_in_{i}"] = image
            out[f"attention_in_{i}"] = att
            out[f"attention_loaded_{i}"] = np.asarray(loaded, dtype=np.float32)
            out[f"image_{i}"] = item["image"].numpy()
            out[f"attention_map_{i}"] = item["attention_map"].numpy()
            out[f"dataset_{i}"] = np.array(item["dataset"])
            out[f"bucket_{i}"] = np.array("" if item["bucket"] is None else item["bucket"])
            out[f"kind_{i}"] = np.array(kind)
    out["n"] = np.array(len(smp))
    np.savez_compressed(os.path.join(OUT, "dataprep.npz"), **out)
    print("wrote dataprep.npz:", {k: v.shape for k, v in out.items() if k.startswith(("image_", "attention_map_"))})


if __name__ == "__main__":
    main()
