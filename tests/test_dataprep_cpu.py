"""CPU-only checks of the trainer's data preparation (attwarp_amd.dataloader, csrc/dataprep.hip): the library's host
helpers (Pillow's BILINEAR coefficient tables, the NEAREST index recurrence) against the numpy restatement
tests/dataprep_ref.py, the restatement against Pillow itself and against tests/golden/dataprep.npz (recorded from the
reference's own dataloader), and the per-sample transform rule.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest
from PIL import Image

import dataprep_ref as R


@pytest.fixture(scope="module")
def lib():
    from attwarp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("dataprep")


def _lib_tables(lib, n_in, n_out):
    cols = 1 if n_in == n_out else int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
    bounds = np.full((n_out, 2), -7, dtype=np.int32)
    kk = np.full((n_out, cols), -7, dtype=np.int32)
    ksize = lib.attwarp_pil_coeffs_8bpc(n_in, n_out, 2, bounds.ctypes.data, kk.ctypes.data, cols)
    return bounds, kk, ksize


def test_bilinear_filter_id_tables_equal_the_restatement(lib):
    """attwarp_pil_coeffs_8bpc(..., ATTWARP_PIL_BILINEAR = 2) for sizes 1..64 x {1, 5, 24, 64, 512} and 683, 1024, 1025 -> 512."""
    from attwarp_amd import _lib, _tables
    assert _lib.PIL_BILINEAR == 2 and _tables._FILTER_IDS["bilinear"] == 2
    pairs = [(n_in, n_out) for n_in in range(1, 65) for n_out in (1, 5, 24, 64, 512)] + [(683, 512), (1024, 512), (1025, 512)]
    for n_in, n_out in pairs:
        bounds, kk, ksize = _lib_tables(lib, n_in, n_out)
        rb, rk, rks = R.bilinear_coeffs(n_in, n_out)
        assert ksize == rks, (n_in, n_out, ksize, rks)
        assert np.array_equal(bounds, rb), (n_in, n_out)
        assert np.array_equal(kk[:, :ksize], rk), (n_in, n_out)
        assert not kk[:, ksize:].any()                       # zero padded
    # the earlier ids keep their tables: the python table helper sizes its columns per filter
    b0, k0, ks0 = _tables._lanczos_tables_host(24, 100, "lanczos")
    b1, k1, ks1 = _tables._lanczos_tables_host(24, 100, "bicubic")
    b2, k2, ks2 = _tables._lanczos_tables_host(24, 100, "bilinear")
    assert (ks0, ks1, ks2) == (7, 5, 3) and k0.shape[1] == 7 and k2.shape[1] == 3
    assert lib.attwarp_pil_coeffs_8bpc(24, 100, 3, b0.ctypes.data, k0.ctypes.data, 7) == -1          # unknown filter


NEAREST_IN = list(range(1, 41)) + [96, 100, 199, 255, 256, 257, 336, 500, 511, 512, 513, 683, 700, 1000, 1024, 1025, 4096]
NEAREST_OUT = [1, 2, 5, 24, 100, 336, 512, 513]
NAMED_PAIRS = [(16, 24), (40, 100), (96, 336), (18, 513)]


def test_nearest_index_equals_the_recurrence_and_pillow(lib):
    """attwarp_pil_nearest_index == the accumulated recurrence == Image.resize(NEAREST) on an index ramp (a 16-bit ramp
    image in mode "I;16" would not take the 8-bit path, so the ramp is split into a low and a high byte image)."""
    pairs = [(a, b) for a in NEAREST_IN for b in NEAREST_OUT]
    assert all(p in pairs for p in NAMED_PAIRS)
    closed_form_differs = 0
    for n_in, n_out in pairs:
        idx = np.full(n_out, -1, dtype=np.int32)
        assert lib.attwarp_pil_nearest_index(n_in, n_out, idx.ctypes.data) == 0
        assert np.array_equal(idx, R.nearest_index(n_in, n_out)), (n_in, n_out)
        ramp = np.arange(n_in, dtype=np.int64)
        lo = np.asarray(Image.fromarray((ramp & 255).astype(np.uint8)[None, :].repeat(2, 0)).resize((n_out, 2), Image.NEAREST))[0]
        hi = np.asarray(Image.fromarray((ramp >> 8).astype(np.uint8)[None, :].repeat(2, 0)).resize((n_out, 2), Image.NEAREST))[0]
        pil = lo.astype(np.int32) + 256 * hi.astype(np.int32) if n_in != n_out else np.arange(n_out, dtype=np.int32)
        assert np.array_equal(idx, pil), (n_in, n_out)
        closed = np.floor((np.arange(n_out) + 0.5) * (n_in / n_out)).astype(np.int32)
        closed_form_differs += int(not np.array_equal(closed, idx))
        if (n_in, n_out) in NAMED_PAIRS:
            assert not np.array_equal(closed, idx), (n_in, n_out)          # the pairs on which the closed form is wrong
    assert closed_form_differs > 0
    assert lib.attwarp_pil_nearest_index(0, 4, idx.ctypes.data) == -1 and lib.attwarp_pil_nearest_index(4, 4, None) == -1


RESIZE_SOURCES = [(1, 1), (2, 3), (7, 5), (37, 91), (64, 48), (375, 500), (1024, 683), (512, 512), (512, 300), (300, 512),
                  (130, 130), (2000, 8), (3, 2000), (2000, 3), (700, 1025)]                    # H x W
RESIZE_TARGETS = [(512, 512), (24, 40), (1, 1), (8, 8)]


def test_restatement_equals_pillow_bilinear():
    rng = np.random.default_rng(41)
    for h, w in RESIZE_SOURCES:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for sh, sw in RESIZE_TARGETS:
            pil = np.asarray(Image.fromarray(im).resize((sw, sh), Image.BILINEAR))
            assert np.array_equal(R.resize_bilinear_u8(im, sh, sw), pil), (h, w, sh, sw)
    g = rng.integers(0, 256, (37, 91), dtype=np.uint8)                               # mode "L"
    assert np.array_equal(R.resize_bilinear_u8(g, 24, 40), np.asarray(Image.fromarray(g).resize((40, 24), Image.BILINEAR)))
    # the pass order shows in the bytes: Pillow takes the vertical pass first exactly where vertical_first() says so
    assert R.vertical_first(2000, 8, 512) and not R.vertical_first(2000, 8, 2000) and not R.vertical_first(800, 8, 512)


def test_restatement_equals_pillow_nearest_and_to_tensor():
    import torch
    rng = np.random.default_rng(42)
    for h, w in [(24, 24), (700, 1000), (16, 32), (1, 1), (18, 40), (96, 16)]:
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for sh, sw in [(512, 512), (24, 100), (513, 336), (1, 1), (h, w)]:
            pil = np.asarray(Image.fromarray(a).resize((sw, sh), Image.NEAREST))
            assert np.array_equal(R.resize_nearest(a, sh, sw), pil), (h, w, sh, sw)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = torch.from_numpy(ramp[:, :, None].copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255).numpy()
    assert np.array_equal(R.to_tensor_u8(ramp), want)
    table = (np.arange(256, dtype=np.float64) * (1.0 / 255.0)).astype(np.float32)          # what the kernels look up
    assert np.array_equal(table, want.reshape(-1))
    assert int((np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0) != table).sum()) == 126   # not a float32 reciprocal


def test_restatement_reproduces_the_reference_fixture(fixture):
    S = int(fixture["S"])
    n = int(fixture["n"])
    assert n >= 5
    for i in range(n):
        image, att, kind = fixture[f"image_in_{i}"], fixture[f"attention_in_{i}"], str(fixture[f"kind_{i}"])
        assert np.array_equal(R.prepare_images([image], S)[0], fixture[f"image_{i}"]), i
        loaded = fixture[f"attention_loaded_{i}"]
        if kind == "npy":
            assert np.array_equal(R.attention_values(att), loaded), i
            got = R.prepare_attention_maps([att], S, normalize=True)[0]
        else:                                                   # overlay: the loader returns gray / 255 as it is
            assert np.array_equal(att.astype(np.float32) / 255.0, loaded), i
            got = R.prepare_attention_maps([loaded], S, normalize=False)[0]
        assert got.dtype == np.float32 and np.array_equal(got, fixture[f"attention_map_{i}"]), i
    with pytest.raises(ValueError):
        R.prepare_images([fixture["image_in_0"]], None)


def test_transform_for_sample_on_the_fixture_table(fixture):
    from attwarp_amd import dataloader as D
    mapping = dict(zip([str(s) for s in fixture["category_names"]], [str(s) for s in fixture["category_transforms"]]))
    assert len(mapping) == 15 and set(mapping.values()) == {"sqrt", "none", "iden"}
    for name, want in mapping.items():
        assert D.transform_for_sample("gqa", name, mapping) == want == R.transform_for_sample("gqa", name, mapping)
        assert D.transform_for_sample("GQA_val", name, mapping) == want
        assert D.transform_for_sample("textvqa", name, mapping) == "iden"
    assert D.transform_for_sample("gqa", "no_such_bucket", mapping) == "sqrt"          # missing bucket
    assert D.transform_for_sample("gqa", None, mapping) == "sqrt"
    assert D.transform_for_sample(None, "query_rel", mapping) == "iden"                # no dataset name
    assert D.transform_for_sample("docvqa", None, mapping) == "iden"
    n = int(fixture["n"])
    datasets = [str(fixture[f"dataset_{i}"]) for i in range(n)]
    buckets = [str(fixture[f"bucket_{i}"]) or None for i in range(n)]
    assert D.transforms_for_batch(datasets, buckets, mapping) == [R.transform_for_sample(d, b, mapping) for d, b in zip(datasets, buckets)]
    assert D.transforms_for_batch(datasets, buckets, mapping) == ["sqrt", "iden", "iden", "sqrt", "sqrt"]
    with pytest.raises(ValueError):
        D.transforms_for_batch(datasets, buckets[:-1], mapping)
    import inspect
    assert "query_rel" not in inspect.getsource(D)              # the package embeds no category table


def test_host_side_refusals_without_gpu(lib):
    """Argument validation of the new entry points runs before anything is enqueued."""
    import ctypes
    from attwarp_amd import dataloader as D
    p = ctypes.cast(ctypes.create_string_buffer(1 << 12), ctypes.c_void_p)
    assert lib.attwarp_prep_images_u8(None, p, p, p, None) == -1
    assert lib.attwarp_prep_images_u8(p, p, p, p, None) == -1 and b"attwarp_prep_images_plan" in lib.attwarp_last_error()
    assert lib.attwarp_prep_attention_f32(None, 1, 8, 8, p, p, None) == -1
    assert lib.attwarp_prep_attention_f32(p, 0, 8, 8, p, p, None) == -1
    assert lib.attwarp_prep_attention_workspace_bytes(3) == 3 * 16 * 4
    rec = np.zeros(1, dtype=D._PREP_IMAGE_DTYPE)
    assert rec.itemsize == 64 and np.zeros(1, dtype=D._PREP_ATTENTION_DTYPE).itemsize == 40
    for f in ("image", "bounds_x", "kk_x", "bounds_y", "kk_y"):
        rec[f] = p.value
    rec["H"], rec["W"], rec["ksize_x"], rec["ksize_y"] = 100, 80, 5, 5
    rp = ctypes.c_void_p(rec.ctypes.data)
    assert lib.attwarp_prep_images_table_bytes(rp, 1, 2, 32, 32) == 0 and b"C must be 1 or 3" in lib.attwarp_last_error()
    n = lib.attwarp_prep_images_table_bytes(rp, 1, 3, 32, 32)
    assert n > 0
    table = np.zeros(n, dtype=np.uint8)
    assert lib.attwarp_prep_images_plan(rp, 1, 3, 32, 32, table.ctypes.data, n - 1) == -1
    assert lib.attwarp_prep_images_plan(rp, 1, 3, 32, 32, table.ctypes.data, n) == 0
    from attwarp_amd import _lib
    h = _lib.PrepHeader.from_address(table.ctypes.data)
    assert (h.B, h.C, h.S_h, h.S_w, h.n_fused_images, h.n_split_images, h.tmp_bytes) == (1, 3, 32, 32, 1, 0, 0)
    assert h.n_fused_items == 2 and h.table_bytes == n and 0 < h.lds_bytes <= 64 * 1024           # bands of 16 rows
    rec["ksize_x"] = 35                                          # past the register window: the two-launch route
    n2 = lib.attwarp_prep_images_table_bytes(rp, 1, 3, 32, 32)
    table2 = np.zeros(n2, dtype=np.uint8)
    assert lib.attwarp_prep_images_plan(rp, 1, 3, 32, 32, table2.ctypes.data, n2) == 0
    h2 = _lib.PrepHeader.from_address(table2.ctypes.data)
    assert (h2.n_fused_images, h2.n_split_images, h2.n_h_items, h2.n_v_items, h2.tmp_bytes) == (0, 1, 7, 4, 100 * 96)
    with pytest.raises(ValueError):
        D.prepare_images([np.zeros((4, 4, 3), np.uint8)], image_size=None)
    with pytest.raises(ValueError):
        D.prepare_attention_maps([np.zeros((4, 4), np.float32)], image_size=None)
    with pytest.raises(ValueError):
        D.collate([np.zeros((4, 4, 3), np.uint8)], [], ["q"], ["a"], ["gqa"], [None], 8)
