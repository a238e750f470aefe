"""Writes tests/golden/sd_warp.npz from the reference checkout: what Ablations/Stable_diffusion_based_warp.py itself computes
on small planted inputs (torch CPU tensors, float32 and float16).

    python tests/golden/make_golden_sdwarp.py /path/to/reference [out.npz]

The reference file is imported by path with stub modules for cv2, torchvision(.transforms), diffusers and
attention_map_diffusers (none of them is needed by what is recorded, except cv2.remap, whose arguments are the record).

Recorded: the inputs; compute_token_importance in its three modes; aggregate_attention_map_for_tokens on equal-sized maps;
the (tx, ty) maps warp_image_by_attention hands to cv2.remap for every transform with apply_inverse on and off; the
exp_scale every pass of run's loop passes to save_warped_image for iterations 1 and 3; numpy's and torch's versions.

The inputs are softmax rows with a planted per-token bias so that the importance of rank k and rank k + 1 (k = TOP_K) differ
by far more than 1 %: the float16 and float32 top-k lists of unplanted rows differ, and no test may depend on a tie.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

TOP_K = 5
STEPS = (981, 801, 621)
LAYERS = ((0, 4, 4), (1, 8, 8), (2, 6, 6))          # (key, H, W); the last layer of every step has one size
B, HEADS, TOKENS = 2, 3, 11
TRANSFORMS = ("identity", "square", "sqrt", "exp", "log")


def load_reference(root):
    remap_calls = []
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.INTER_CUBIC, cv2.BORDER_REPLICATE = 1, 2, 1

    def remap(image, mx, my, interpolation=None, borderMode=None):
        remap_calls.append((np.array(mx), np.array(my)))
        return np.zeros(mx.shape + image.shape[2:], image.dtype)
    cv2.remap = remap
    cv2.imread = lambda path: np.zeros((9, 7, 3), np.uint8)
    stubs = {"cv2": cv2}
    for name in ("torchvision", "torchvision.transforms", "diffusers", "attention_map_diffusers"):
        stubs[name] = types.ModuleType(name)
    for n in ("Compose", "Resize", "ToTensor", "Normalize"):
        setattr(stubs["torchvision.transforms"], n, object)
    stubs["torchvision"].transforms = stubs["torchvision.transforms"]
    stubs["diffusers"].DiffusionPipeline = stubs["diffusers"].DDIMScheduler = object
    stubs["attention_map_diffusers"].init_pipeline = lambda p: p
    stubs["attention_map_diffusers"].attn_maps = {}
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("sd_warp_reference",
                                                      os.path.join(root, "Ablations", "Stable_diffusion_based_warp.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod, remap_calls


def planted_inputs():
    rng = np.random.default_rng(20261017)
    bias = np.zeros(TOKENS)
    bias[[7, 2, 9, 0, 4, 5]] = [3.0, 2.5, 2.0, 1.5, 1.0, 0.4]
    out = {}
    for s in STEPS:
        for (k, H, W) in LAYERS:
            z = rng.standard_normal((B, HEADS, H, W, TOKENS)) + bias
            e = np.exp(z - z.max(axis=-1, keepdims=True))
            out[f"in_{s}_{k}"] = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    return out


def captured(inputs, dtype):
    return {s: {k: torch.from_numpy(inputs[f"in_{s}_{k}"]).to(dtype) for (k, _, _) in LAYERS} for s in STEPS}


def step_scales(ref, iterations, exp_scale):
    """run's loop with everything before it replaced: the exp_scale of every save_warped_image call."""
    seen = []
    names = ("load_pipeline", "encode_image", "get_text_embeddings", "truncated_ddim_inversion", "forward_and_capture",
             "compute_token_importance", "aggregate_attention_map_for_tokens", "upsample_attention_map", "save_warped_image")
    saved = {n: getattr(ref, n) for n in names}
    tok = types.SimpleNamespace(convert_ids_to_tokens=lambda ids: ["x"] * 16)
    try:
        ref.load_pipeline = lambda device=None: types.SimpleNamespace(tokenizer=tok)
        ref.encode_image = lambda pipe, path: None
        ref.get_text_embeddings = lambda pipe, prompt: (None, [list(range(16))])
        ref.truncated_ddim_inversion = lambda pipe, z, emb, ts: {}
        ref.forward_and_capture = lambda pipe, inv, prompt: None
        ref.compute_token_importance = lambda maps, inference_step_selection=None: np.arange(16.0)
        ref.aggregate_attention_map_for_tokens = lambda maps, idx, inference_step_selection=None, num_last_layers=1: np.zeros((2, 2), np.float32)
        ref.upsample_attention_map = lambda a, size: np.zeros(size, np.float32)
        ref.save_warped_image = lambda *a, **kw: seen.append(float(a[6]))
        ref.run("in.png", "prompt", "out.png", 17, 13, "exp", exp_scale, 1.0, False, iterations, 3)
    finally:
        for n, f in saved.items():
            setattr(ref, n, f)
    return np.array(seen, dtype=np.float64)


def main():
    root = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "sd_warp.npz")
    ref, remap_calls = load_reference(root)
    rec = planted_inputs()
    for name, dt in (("f32", torch.float32), ("f16", torch.float16)):
        cap = captured(rec, dt)
        rec[f"imp_all_{name}"] = ref.compute_token_importance(cap)
        rec[f"imp_sel_{name}"] = ref.compute_token_importance(cap, inference_step_selection=[STEPS[1], STEPS[2]], num_layers=2)
        rec[f"imp_last_{name}"] = ref.compute_token_importance(cap, last_timestep=True)
        top = list(np.argsort(rec[f"imp_all_{name}"])[-TOP_K:][::-1])
        rec[f"top_{name}"] = np.array(top, dtype=np.int64)
        imp = np.sort(rec[f"imp_all_{name}"].astype(np.float64))[::-1]
        assert (imp[TOP_K - 1] - imp[TOP_K]) > 0.01 * imp[TOP_K - 1], "planted gap too small"
        rec[f"agg_{name}"] = ref.aggregate_attention_map_for_tokens(cap, top, inference_step_selection=None, num_last_layers=1)
    assert list(rec["top_f32"]) == list(rec["top_f16"])

    rng = np.random.default_rng(7)
    att = rng.random((12, 10)).astype(np.float32)
    rec["warp_att"] = att
    image = np.zeros((12, 10, 3), np.uint8)
    for t in TRANSFORMS:
        for inv in (False, True):
            ref.set_transform_function(t, 1.5, 2.0, inv)
            del remap_calls[:]
            ref.warp_image_by_attention(image, att, 17, 13)
            mx, my = remap_calls[0]
            rec[f"warp_tx_{t}_{int(inv)}"] = mx[0].astype(np.float32)
            rec[f"warp_ty_{t}_{int(inv)}"] = my[:, 0].astype(np.float32)
    rec["step_scale_1"] = step_scales(ref, 1, 2.0)
    rec["step_scale_3"] = step_scales(ref, 3, 2.0)
    rec["versions"] = np.array([np.__version__, torch.__version__])
    np.savez_compressed(out_path, **rec)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
