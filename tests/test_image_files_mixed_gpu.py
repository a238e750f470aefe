"""One list of PNG, baseline JPEG and progressive JPEG files in scrambled order through ``pipeline.upload_image_files``: the
shared file-batch base (attwarp_amd/_batch.py), the splitter for PNG / JPEG and the one for baseline / progressive at once,
at the smallest size where a mix-up of indices shows.  Every pixel equals Pillow's; no tolerance."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _file(seed, side, fmt, **kw):
    a = np.random.default_rng(seed).integers(0, 256, (side, side, 3), dtype=np.uint8)
    a[side // 4:side // 2] //= 4                              # (every image its own content, so a swapped pair cannot pass)
    b = io.BytesIO()
    Image.fromarray(a).save(b, fmt, **kw)
    return b.getvalue()


def test_six_tiny_files_of_three_kinds_come_back_in_input_order():
    from attwarp_amd import jpeg, pipeline
    png = [_file(1, 8, "PNG"), _file(2, 8, "PNG")]
    base = [_file(3, 16, "JPEG", quality=90), _file(4, 16, "JPEG", quality=90, subsampling=0, restart_marker_blocks=1)]
    prog = [_file(5, 16, "JPEG", quality=90, progressive=True), _file(6, 16, "JPEG", quality=85, subsampling=0, progressive=True)]
    files = [prog[0], png[0], base[1], prog[1], base[0], png[1]]
    assert [jpeg.parse_jpeg(f, 0, True).get("progressive", False) for f in (base + prog)] == [False, False, True, True]
    assert jpeg.parse_jpeg(base[1])["ri"] == 1 and jpeg.parse_jpeg(base[1])["units"] == 4
    want = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    assert len({w.tobytes() for w in want}) == 6
    got = pipeline.upload_image_files(files, device=DEV, progressive=True)
    assert len(got) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.uint8 and tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), i
    # the JPEG files alone: two plans behind one object, views and statuses in input order
    jf = jpeg.JpegFiles([files[i] for i in (0, 2, 3, 4)], device=DEV, progressive=True)
    views, status = jf.run()
    assert [idx for idx, _ in jf.parts] == [[1, 3], [0, 2]] and status.cpu().tolist() == [0] * 4
    assert jf.units() == [10, 4, 10, 1] and jf.levels() == [3, 0, 3, 0] and jf.out_bytes == 4 * 16 * 16 * 3 == sum(part.out_bytes for _, part in jf.parts)
    for v, i in zip(views, (0, 2, 3, 4)):
        assert np.array_equal(v.cpu().numpy(), want[i]), i
