"""CPU-only checks of the ragged CLIP preprocess (csrc/clip_ragged.hip, pipeline.ClipBatch): the plan's table layout and
header through ctypes with fake device pointers, the entry points' validation, the documented limits, and the reference of
tests/test_clip_ragged_gpu.py standing on its own (Pillow-built canvas + clip_ref == the oracle's restatement), so that a
failure of the GPU test points at the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import clip_ref as R
import clip_ragged_ref as G
from oracle import warp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from attwarp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def records(shapes, size, pad, fake):
    """attwarp_clip_image records as ClipBatch fills them, every pointer the same fake device address."""
    from attwarp_amd import pipeline as P
    rec = np.zeros(len(shapes), dtype=P._CLIP_IMAGE_DTYPE)
    for i, (H, W) in enumerate(shapes):
        g = P.clip_geometry(H, W, size, pad)
        for k, v in g.items():
            rec[k][i] = v
        rec["H"][i], rec["W"][i] = H, W
        rec["ksize_x"][i], rec["ksize_y"][i] = G.taps(g["canvas_w"], g["nw"]), G.taps(g["canvas_h"], g["nh"])
        for f in ("image", "bounds_x", "kk_x", "bounds_y", "kk_y"):
            rec[f][i] = fake + 1000 * i
    return rec


def plan(lib, rec, C, size):
    from attwarp_amd import _lib, pipeline as P
    rp = ctypes.c_void_p(rec.ctypes.data)
    n = lib.attwarp_clip_images_table_bytes(rp, len(rec), C, size)
    assert n > 0, lib.attwarp_last_error()
    table = np.full(n, 0xAB, dtype=np.uint8)
    assert lib.attwarp_clip_images_plan(rp, len(rec), C, size, table.ctypes.data, n) == 0
    h = _lib.ClipHeader.from_address(table.ctypes.data)
    recs = table[h.off_images:h.off_images + len(rec) * P._CLIP_RECORD_DTYPE.itemsize].view(P._CLIP_RECORD_DTYPE)
    nitems = h.n_fused_items + h.n_h_items + h.n_v_items
    items = table[h.off_items:h.off_items + 16 * nitems].view(np.int32).reshape(nitems, 4)
    return table, h, recs, items


def test_structs_follow_the_header():
    from attwarp_amd import _lib, pipeline as P
    hdr = open(os.path.join(ROOT, "include", "attwarp.h")).read()
    for S, cname, size in ((_lib.ClipImage, "attwarp_clip_image", 96), (_lib.ClipHeader, "attwarp_clip_header", 88)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert [n for n, _ in S._fields_] == names, cname
        assert ctypes.sizeof(S) == size, cname
    assert P._CLIP_IMAGE_DTYPE.itemsize == 96 and list(P._CLIP_IMAGE_DTYPE.names) == [n for n, _ in _lib.ClipImage._fields_]
    assert P._CLIP_RECORD_DTYPE.itemsize == 128 and P._CLIP_RECORD_DTYPE.names[:len(P._CLIP_IMAGE_DTYPE.names)] == P._CLIP_IMAGE_DTYPE.names


def test_plan_table_layout_without_gpu(lib):
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 12), ctypes.c_void_p).value
    #          8 taps      16 taps     17 taps      identity     15 taps      31 taps
    shapes = [(48, 61), (40, 505), (40, 1177), (336, 200), (683, 1024), (2400, 40)]
    rec = records(shapes, 336, True, fake)
    table, h, recs, items = plan(lib, rec, 3, 336)
    assert (h.magic, h.B, h.C, h.size) == (0x52504C43, 6, 3, 336)
    assert (h.n_fused_images, h.n_split_images, h.ks) == (4, 2, 16)
    assert h.off_images == 96 and h.off_items == 96 + 6 * 128 and h.table_bytes == len(table) and h.table_bytes % 16 == 0
    assert h.table_bytes == (h.off_items + 16 * len(items) + 15) // 16 * 16
    # the caller's record comes back unchanged, then the launcher's choices
    for name in rec.dtype.names:
        assert np.array_equal(recs[name], rec[name]), name
    assert [int(v) for v in recs["fused"]] == [1, 1, 0, 1, 1, 0]
    assert [int(v) for v in recs["window"]] == [8, 16, 0, 8, 16, 0]
    assert [int(v) for v in recs["canvas_w"]] == [61, 505, 1177, 336, 1024, 2400]
    assert [(int(r["pad_x"]), int(r["pad_y"])) for r in recs] == [(0, 6), (0, 232), (0, 568), (68, 0), (0, 170), (1180, 0)]
    # LDS: table + the band's vertical coefficients + band rows of 1008 bytes + staged canvas rows + slack, the largest over
    # the batch, within a CU's 160 KB
    need = [3072 + 4 * int(r["ny"]) * int(r["ksize_y"]) + int(r["nr_cap"]) * 1008 + int(r["rb"]) * ((3 * int(r["canvas_w"]) + 3) & ~3) + 128 for r in recs if r["fused"]]
    assert h.lds_bytes == max(need) <= 160 * 1024
    for r in recs[recs["fused"] == 1]:
        ny = min(int(r["ny"]), 336)
        assert int(r["nr_cap"]) == min((ny - 1) * int(r["canvas_h"]) // 336 + 2 + int(r["ksize_y"]), int(r["canvas_h"]))
        assert int(r["rb"]) in (4, 8) and int(r["ny"]) in (8, 16, 32, 64)
    # work items: (image, y0, ny, 0); 8-tap bands first, then the wide ones, then the two passes of the two-launch route
    n8 = h.n_fused_items - h.n_wide_items
    assert set(items[:n8, 0]) == {0, 3} and set(items[n8:h.n_fused_items, 0]) == {1, 4}
    for b in range(6):
        mine = items[:h.n_fused_items][items[:h.n_fused_items, 0] == b]
        if recs["fused"][b]:
            assert np.array_equal(mine[:, 1], np.arange(0, 336, int(recs["ny"][b]))) and int(mine[:, 2].sum()) == 336
        else:
            assert len(mine) == 0
    hit = items[h.n_fused_items:h.n_fused_items + h.n_h_items]
    vit = items[h.n_fused_items + h.n_h_items:]
    assert h.n_h_items == -(-1177 // 16) + 2400 // 16 and h.n_v_items == 2 * 42 and not items[:, 3].any()
    assert set(hit[:, 0]) == set(vit[:, 0]) == {2, 5}
    assert int(hit[hit[:, 0] == 2][:, 2].sum()) == 1177 and int(vit[vit[:, 0] == 5][:, 2].sum()) == 336
    # the intermediate: every canvas row x the 336 cropped columns, packed, 4-byte aligned
    assert [int(recs["tmp_off"][2]), int(recs["tmp_off"][5])] == [0, 1177 * 1008] and h.tmp_bytes == (1177 + 2400) * 1008
    # planning is deterministic and the size query agrees with a too-small buffer being refused
    table2 = plan(lib, rec, 3, 336)[0]
    assert np.array_equal(table, table2)
    rp = ctypes.c_void_p(rec.ctypes.data)
    assert lib.attwarp_clip_images_plan(rp, 6, 3, 336, table.ctypes.data, len(table) - 1) == -1
    assert b"needs" in lib.attwarp_last_error()


def test_plan_without_padding_and_vertical_first(lib):
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p).value
    shapes = [(4100, 40), (48, 61), (3000, 40)]
    rec = records(shapes, 32, False, fake)
    assert [int(v) for v in rec["vertical_first"]] == [1, 0, 0] and [int(v) for v in rec["nh"]] == [3280, 32, 2400]
    assert [int(v) for v in rec["top"]] == [1624, 0, 1184] and [int(v) for v in rec["left"]] == [0, 4, 0]
    table, h, recs, items = plan(lib, rec, 3, 32)
    assert [int(v) for v in recs["fused"]] == [0, 1, 1] and (h.n_h_items, h.n_v_items) == (2, 4)
    assert h.tmp_bytes == 32 * 40 * 3                       # vertical pass first: [size, W * C] in between
    rec["pad_x"][0] = 1                                      # a vertical-first image cannot sit on a canvas
    rec["canvas_w"][0] = 41
    assert lib.attwarp_clip_images_table_bytes(ctypes.c_void_p(rec.ctypes.data), 3, 3, 32) == 0
    assert b"vertical-first" in lib.attwarp_last_error()


def test_entry_point_validation_without_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fake = p.value
    rec = records([(48, 61)], 336, True, fake)
    table, h, _, _ = plan(lib, rec, 3, 336)
    t = ctypes.c_void_p(table.ctypes.data)
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    bg = (ctypes.c_uint8 * 3)(1, 2, 3)
    mp, bp = ctypes.cast(m, ctypes.c_void_p), ctypes.cast(bg, ctypes.c_void_p)
    F32, F16, BF16 = 0, 1, 2
    assert lib.attwarp_clip_images_u8(None, p, mp, mp, bp, None, p, F32, None) == -1 and b"null" in lib.attwarp_last_error()
    assert lib.attwarp_clip_images_u8(t, None, mp, mp, bp, None, p, F32, None) == -1
    assert lib.attwarp_clip_images_u8(t, p, None, mp, bp, None, p, F32, None) == -1
    assert lib.attwarp_clip_images_u8(t, p, mp, mp, None, None, p, F32, None) == -1
    assert lib.attwarp_clip_images_u8(t, p, mp, mp, bp, None, None, F16, None) == -1
    assert lib.attwarp_clip_images_u8(p, p, mp, mp, bp, None, p, F32, None) == -1              # zeros: not a planned table
    assert b"attwarp_clip_images_plan" in lib.attwarp_last_error()
    assert lib.attwarp_clip_images_u8(t, p, mp, mp, bp, None, p, BF16, None) == -1 and b"dtype" in lib.attwarp_last_error()
    assert lib.attwarp_clip_images_u8(t, p, mp, mp, bp, None, p, 7, None) == -1
    assert lib.attwarp_clip_images_u8(t, ctypes.c_void_p(fake + 4), mp, mp, bp, None, p, F32, None) == -1
    assert b"8-byte" in lib.attwarp_last_error()
    assert lib.attwarp_clip_images_u8(t, p, mp, mp, bp, None, ctypes.c_void_p(fake + 8), F32, None) == -1
    assert b"16-byte" in lib.attwarp_last_error()
    wide, _, _, _ = plan(lib, records([(40, 1177)], 336, True, fake), 3, 336)                  # needs tmp
    assert lib.attwarp_clip_images_u8(ctypes.c_void_p(wide.ctypes.data), p, mp, mp, bp, None, p, F32, None) == -1
    assert b"bytes of tmp" in lib.attwarp_last_error()
    # the planner's own argument checks
    rp = ctypes.c_void_p(rec.ctypes.data)
    assert lib.attwarp_clip_images_table_bytes(None, 1, 3, 336) == 0
    assert lib.attwarp_clip_images_table_bytes(rp, 0, 3, 336) == 0 and lib.attwarp_clip_images_table_bytes(rp, 1, 3, 0) == 0
    assert lib.attwarp_clip_images_table_bytes(rp, 1, 2, 336) == 0 and b"C must be 1 or 3" in lib.attwarp_last_error()
    assert lib.attwarp_clip_images_plan(rp, 1, 3, 336, None, 1 << 20) == -1
    for field, value, text in (("image", 0, b"null pointer"), ("kk_y", 0, b"null pointer"), ("H", 0, b"non-positive"),
                               ("ksize_x", 0, b"non-positive"), ("pad_y", 14, b"does not lie on its"),
                               ("pad_x", -1, b"does not lie on its"), ("left", 1, b"crop"), ("nh", 335, b"crop")):
        bad = rec.copy()
        bad[field] = value
        assert lib.attwarp_clip_images_table_bytes(ctypes.c_void_p(bad.ctypes.data), 1, 3, 336) == 0, field
        assert text in lib.attwarp_last_error(), (field, lib.attwarp_last_error())
        table = np.zeros(1 << 12, np.uint8)
        assert lib.attwarp_clip_images_plan(ctypes.c_void_p(bad.ctypes.data), 1, 3, 336, table.ctypes.data, table.size) == -1


def test_limits_are_unsupported_with_a_message(lib):
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p).value
    table = np.zeros(1 << 16, np.uint8)

    def rc(rec, C, size):
        return lib.attwarp_clip_images_plan(ctypes.c_void_p(rec.ctypes.data), len(rec), C, size, table.ctypes.data, table.size)

    assert rc(records([(8192, 40)], 336, True, fake), 3, 336) == 0
    assert rc(records([(8193, 40)], 336, True, fake), 3, 336) == -2
    assert b"canvas 8193 x 8193 exceeds 8192" in lib.attwarp_last_error()
    assert rc(records([(40, 9000)], 336, False, fake), 3, 336) == -2 and b"exceeds 8192" in lib.attwarp_last_error()
    assert rc(records([(40, 40)], 4096, True, fake), 3, 4096) == 0
    assert rc(records([(40, 40)], 4097, True, fake), 3, 4097) == -2 and b"size > 4096" in lib.attwarp_last_error()
    assert rc(records([(1, 8000)], 336, False, fake), 3, 336) == -2 and b"beyond 2^20" in lib.attwarp_last_error()
    # C = 1 is served; a band that does not fit the LDS goes to the two-launch route instead of being refused
    assert rc(records([(48, 61)], 336, True, fake), 1, 336) == 0
    _, h, recs, _ = plan(lib, records([(8192, 8192)], 4096, True, fake), 3, 4096)
    assert (h.n_fused_images, h.n_split_images, h.lds_bytes) == (0, 1, 0) and int(recs["ksize_x"][0]) == 9


PAD_REF_SHAPES = [(1, 1), (2, 3), (5, 8), (48, 61), (61, 48), (40, 505), (336, 200), (337, 300)]


@pytest.mark.parametrize("hw", PAD_REF_SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_stands_on_its_own(hw):
    """Pillow's Image.new + paste + per-channel resize against the oracle's restatement of expand2square and of the HF
    processor, every pattern."""
    H, W = hw
    size = 336 if max(hw) > 61 else 32                      # (the oracle's restatement is a Python loop over the taps)
    for name in R.PATTERNS:
        img = R.pattern(name, H, W, 3, size, seed=9)
        canvas = G.pad_canvas(img, G.background_of(R.OPENAI_CLIP_MEAN))
        assert canvas.shape == (max(hw), max(hw), 3) and np.array_equal(canvas, O.expand2square(img))
        assert np.array_equal(G.reference(img, size), O.clip_preprocess(O.expand2square(img), size)), (hw, name)
    assert G.background_of(R.OPENAI_CLIP_MEAN) == (122, 116, 104)


def test_reference_background_and_channels():
    img = R.pattern("noise", 5, 8, 3, 336, seed=1)
    c = G.pad_canvas(img, (0, 255, 7))
    assert c.shape == (8, 8, 3) and np.array_equal(c[1:6], img) and (c[0] == (0, 255, 7)).all() and (c[6:] == (0, 255, 7)).all()
    t = G.pad_canvas(img.transpose(1, 0, 2).copy(), (0, 255, 7))
    assert np.array_equal(t[:, 1:6], img.transpose(1, 0, 2)) and (t[:, 0] == (0, 255, 7)).all() and (t[:, 6:] == (0, 255, 7)).all()
    g = G.pad_canvas(img[:, :, :1], (9,))
    assert g.shape == (8, 8, 1) and (g[0] == 9).all() and np.array_equal(g[1:6], img[:, :, :1])
    # a constant canvas of the background resizes to that constant: rows wholly outside the image need no horizontal pass
    from PIL import Image
    for n in (337, 505, 1024, 1177, 2400):
        out = np.asarray(Image.new("RGB", (n, n), (122, 116, 104)).resize((336, 336), Image.BICUBIC))
        assert (out == (122, 116, 104)).all(), n
    assert (np.asarray(Image.new("RGB", (1024, 8), (0, 255, 7)).resize((336, 8), Image.BICUBIC)) == (0, 255, 7)).all()


def test_process_images_reads_its_arguments_without_gpu():
    import types
    from attwarp_amd import pipeline as P
    proc = types.SimpleNamespace(image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5], size={"shortest_edge": 336},
                                 crop_size={"height": 336, "width": 336})
    with pytest.raises(NotImplementedError):
        P.process_images([], proc, types.SimpleNamespace(image_aspect_ratio="anyres"))
    with pytest.raises(NotImplementedError):
        P.process_images([], types.SimpleNamespace(**{**vars(proc), "crop_size": {"height": 224, "width": 224}}),
                         types.SimpleNamespace(image_aspect_ratio="pad"))
    with pytest.raises(NotImplementedError):
        P.process_images([], types.SimpleNamespace(**{**vars(proc), "resample": 2}), types.SimpleNamespace())
    with pytest.raises(ValueError):                          # read through to the batch: empty
        P.process_images([], proc, types.SimpleNamespace(image_aspect_ratio="pad"))
    assert P.clip_geometry(683, 1024, 336, True) == dict(canvas_w=1024, canvas_h=1024, pad_x=0, pad_y=170, nw=336, nh=336,
                                                         left=0, top=0, vertical_first=0)
    assert P.clip_geometry(5, 8, 336, True)["pad_y"] == 1 and P.clip_geometry(8, 5, 336, True)["pad_x"] == 1
