"""Measure the PNG encoder's two token routes, match="rle" and match="lz" (attwarp_amd.png), in one process.

    python tools/pnglz_bench.py [--out profiles/pnglz_bench.json]

Cases: 500 x 500 x 3 photo-like images at B = 32 and B = 256, pages of glyphs (tests/pnglz_cases.py) and, where Pillow has
FreeType, pages of rendered text, 850 x 1100 grey, 24 x 24 masks up-sampled with LANCZOS to 500 x 500 grey, and 256 images of
1024 x 1024 x 3.  Per case and route: PngBatch.run on a planned batch (HIP events around the launches, as tools/png_bench.py),
the files' bytes, the share of segments written as LZ blocks, and encode_png's wall clock (plan, launches, download of the
compressed bytes).  Per case: the host route -- download of the raw pixels + Pillow ``save`` per image on 16 threads -- at
Pillow's default and at compress_level = 1, with their sizes.  None of these numbers is a pass mark."""
import argparse
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from png_bench import photo_like, timed, wall  # noqa: E402


def text_pages(n, H, W):
    """Pages of rendered words, or None where Pillow was built without FreeType."""
    from PIL import Image, ImageDraw, ImageFont, features
    if not features.check("freetype2"):
        return None
    rng = np.random.default_rng(3)
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 10)))) for _ in range(400)]
    font = ImageFont.load_default(14)
    pages = []
    for _ in range(n):
        im = Image.new("L", (W, H), 255)
        dr = ImageDraw.Draw(im)
        for y in range(20, H - 20, 20):
            dr.text((20, y), " ".join(words[int(i)] for i in rng.integers(0, 400, 14)), fill=0, font=font)
        pages.append(np.asarray(im)[:, :, None])
    return np.stack(pages)


def masks(n, S):
    from PIL import Image
    rng = np.random.default_rng(4)
    out = []
    for _ in range(n):
        m = (rng.random((24, 24)) ** 3 * 255).astype(np.uint8)
        out.append(np.asarray(Image.fromarray(m).resize((S, S), Image.LANCZOS))[:, :, None])
    return np.stack(out)


def case(name, images):
    from PIL import Image
    from attwarp_amd import png
    B = int(images.shape[0])
    res = {"case": name, "B": B, "image": list(images.shape[1:]), "filter": "sub"}
    for match in ("rle", "lz"):
        batch = png.PngBatch(images, match=match)
        entry = timed(batch.run)
        files = png.download(*batch.run())
        routes = batch.routes()
        entry["file_bytes"] = sum(len(f) for f in files)
        entry["segments"] = len(routes)
        entry["share_of_lz_segments"] = routes.count(1) / len(routes)
        entry["share_of_stored_segments"] = routes.count(2) / len(routes)
        first = np.asarray(Image.open(io.BytesIO(files[0])))
        entry["pillow_decodes_to_source"] = bool(np.array_equal(first.reshape(images.shape[1:]), images[0].cpu().numpy()))
        png.encode_png(images, match=match)                 # untimed: the first call of a shape pays for the allocator's growth
        torch.cuda.synchronize()
        w = wall(lambda: png.encode_png(images, match=match), n=5)
        w["wide_spread"] = bool(w["us_max"] > 1.5 * w["us_min"])        # (a ratio derived from such an entry means little)
        entry["encode_png_incl_plan_and_download"] = w
        res[match] = entry
        del batch
    res["lz_over_rle_time"] = res["lz"]["us_median"] / res["rle"]["us_median"]
    res["lz_over_rle_bytes"] = res["lz"]["file_bytes"] / res["rle"]["file_bytes"]
    res["lz_over_rle_encode_png_wall"] = (res["lz"]["encode_png_incl_plan_and_download"]["us_median"] /
                                          res["rle"]["encode_png_incl_plan_and_download"]["us_median"])

    def save(a, **kw):
        bio = io.BytesIO()
        Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(bio, "PNG", **kw)
        return bio.tell()

    with ThreadPoolExecutor(16) as pool:
        for key, kw in (("host_download_pillow_default_16_threads", {}), ("host_download_pillow_level1_16_threads", {"compress_level": 1})):
            size = []

            def host_path():
                size[:] = [sum(pool.map(lambda a: save(a, **kw), images.cpu().numpy()))]
            res[key] = wall(host_path)
            res[key]["file_bytes"] = size[0]
    for key in ("default", "level1"):
        host = res[f"host_download_pillow_{key}_16_threads"]
        res[f"host_{key}_over_encode_png_lz"] = host["us_median"] / res["lz"]["encode_png_incl_plan_and_download"]["us_median"]
        res[f"lz_bytes_over_pillow_{key}"] = res["lz"]["file_bytes"] / host["file_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnglz_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pnglz_bench needs a GPU"
    import pnglz_cases as C
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    gen = torch.Generator(device=dev).manual_seed(7)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "cases": []}

    def add(name, images):
        res["cases"].append(case(name, images))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()

    for B in (32, 256):
        add(f"photo_like_500x500_B{B}", torch.stack([photo_like(500, 500, dev, gen, b) for b in range(B)]))
    add("glyph_pages_1100x850_grey_B32", torch.from_numpy(np.stack([C.glyph_page(50 + b, 1100, 850, 1) for b in range(32)])).to(dev))
    pages = text_pages(32, 1100, 850)
    if pages is None:
        res["rendered_text"] = "skipped: Pillow without FreeType"
    else:
        add("rendered_text_1100x850_grey_B32", torch.from_numpy(pages).to(dev))
    add("lanczos_masks_500x500_grey_B64", torch.from_numpy(masks(64, 500)).to(dev))
    proto = photo_like(1024, 1024, dev, gen, 2)
    add("photo_like_1024x1024_B256", torch.stack([torch.roll(proto, shifts=(17 * b, 29 * b), dims=(0, 1)) for b in range(256)]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
