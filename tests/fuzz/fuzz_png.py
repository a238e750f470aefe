"""Test infrastructure: randomised differential run of the PNG encoder against tests/png_ref.py and Pillow -- random batch
sizes, image sizes (1 x 1 up to a few segments, narrow and wide), channels, filters, channel orders, run structure (noise,
flat, long runs of random lengths, smooth), row pitches and byte offsets.  Bounded: at most `iterations` batches.
usage: fuzz_png.py [iterations] [seed]"""
import io, os, sys
import numpy as np, torch
from PIL import Image
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from attwarp_amd import png
import png_ref as R
dev = torch.device("cuda:0")
iterations = min(int(sys.argv[1]) if len(sys.argv) > 1 else 20, 1000)
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
def dim():
    r = rng.random()
    if r < 0.4: return int(rng.integers(1, 9))
    if r < 0.9: return int(rng.integers(9, 200))
    return int(rng.integers(200, 900))
def content(h, w, c):
    kind = rng.choice(["noise", "flat", "runs", "smooth", "few"])
    if kind == "noise": return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "flat": return np.full((h, w, c), int(rng.integers(0, 256)), np.uint8)
    if kind == "few": return rng.integers(0, 3, (h, w, c), dtype=np.uint8) * 90
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(xx * (k + 1) + yy * 2 + rng.integers(0, 2, (h, w))) & 255 for k in range(c)], -1).astype(np.uint8)
    flat = np.empty(h * w * c, np.uint8); i = 0
    while i < flat.size:                                     # runs of random lengths around deflate's 258
        n = int(rng.choice([1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517, int(rng.integers(1, 2000))]))
        flat[i:i + n] = rng.integers(0, 256); i += n
    return flat.reshape(h, w, c)
n = bad = 0
for it in range(iterations):
    B = int(rng.integers(1, 9))
    imgs, tens, filts, orders = [], [], [], []
    for b in range(B):
        h, w, c = dim(), dim(), int(rng.choice([1, 3]))
        if h * w * c > 400_000: h = max(1, 400_000 // (w * c))
        a = content(h, w, c)
        pitch, off = w * c + int(rng.integers(0, 9)) * int(rng.random() < 0.5), int(rng.integers(0, 4))
        flat = torch.zeros(off + h * pitch, dtype=torch.uint8, device=dev)
        t = flat[off:].as_strided((h, w, c), (pitch, c, 1)); t.copy_(torch.from_numpy(a))
        imgs.append(a); tens.append(t if c == 3 or rng.random() < 0.5 else t[:, :, 0])
        filts.append(str(rng.choice(png.FILTERS))); orders.append(str(rng.choice(["rgb", "bgr"])))
    files = png.encode_png(tens, filts, orders)
    for a, f, ft, o in zip(imgs, files, filts, orders):
        n += 1
        pix = a[:, :, ::-1] if o == "bgr" and a.shape[2] == 3 else a
        ok = f == R.encode(a, ft, o) and np.array_equal(np.asarray(Image.open(io.BytesIO(f))).reshape(pix.shape), pix)
        if not ok:
            bad += 1
            print("MISMATCH", a.shape, ft, o, flush=True)
print(f"fuzz_png: {n} images in {iterations} batches, {bad} mismatches")
sys.exit(1 if bad else 0)
