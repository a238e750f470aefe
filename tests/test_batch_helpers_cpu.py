"""Host-only tests of what the planned batch classes share (attwarp_amd/_batch.py): the split-and-scatter helper keeps the
input order, the planned-table helper raises every site's own class and prefix when the library refuses the batch size
(through the real library; no GPU is touched), and the staging pool is reachable under its old names."""
import ctypes

import numpy as np
import pytest

from attwarp_amd import _batch, _lib

PATTERNS = {"all_one_kind": "aaaaa", "all_the_other": "bbb", "alternating": "ababab", "alternating_odd": "babab",
            "one_at_the_start": "baaaa", "one_at_the_end": "aaaab", "one_at_either_end": "baaab", "single": "a"}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_split_and_scatter_returns_input_order(name):
    keys = list(PATTERNS[name])
    items = [f"{k}{i}" for i, k in enumerate(keys)]
    calls = []

    def run(kind, group):
        calls.append((kind, list(group)))
        return [(kind, g.upper()) for g in group]

    got = _batch.per_kind(items, keys, ("a", "b"), run)
    assert got == [(k, it.upper()) for k, it in zip(keys, items)]
    assert [k for k, _ in calls] == [k for k in ("a", "b") if k in keys]              # one call per kind that occurs, in order
    assert all(group == [it for it, k in zip(items, keys) if k == kind] for kind, group in calls)
    assert _batch.split_indices(keys, ("a", "b")) == [(k, [i for i, x in enumerate(keys) if x == k]) for k in ("a", "b") if k in keys]


def test_scattered_puts_each_value_at_its_index():
    assert _batch.scattered(5, [([4, 0], "xy"), ([2], "z")]) == ["y", None, "z", None, "x"]


# (the *_table_bytes call of every site with B = 0 and with a B above every limit, the class and the prefix the site raises)
SITES = [("RaggedBatch", lambda B: ("attwarp_ragged_table_bytes", None, B, 3, 24, 500, 500), _lib.AttWarpError, "attwarp_ragged_table_bytes: "),
         ("ClipBatch", lambda B: ("attwarp_clip_images_table_bytes", None, B, 3, 336), _lib.AttWarpError, "attwarp_clip_images_table_bytes: "),
         ("PreparedImages", lambda B: ("attwarp_prep_images_table_bytes", None, B, 3, 512, 512), _lib.AttWarpError, "attwarp_prep_images_table_bytes: "),
         ("PngBatch", lambda B: ("attwarp_png_table_bytes", None, B), ValueError, "PngBatch: "),
         ("PngFiles", lambda B: ("attwarp_pngdec_table_bytes", None, B, 1), ValueError, "PngFiles: "),
         ("jpeg.plan", lambda B: ("attwarp_jpegdec_table_bytes", None, B), ValueError, "jpeg: "),
         ("jpeg.plan_scans", lambda B: ("attwarp_jpegdec_scans_table_bytes", None, B, max(B, 1)), ValueError, "jpeg: ")]


@pytest.mark.parametrize("site,size,exc,prefix", SITES, ids=[s[0] for s in SITES])
@pytest.mark.parametrize("B", [0, 1 << 30])
def test_planned_table_raises_the_sites_own_class_and_prefix(site, size, exc, prefix, B):
    with pytest.raises(exc) as e:                             # (the planner named here never runs: the size comes first)
        _batch.planned_table(size(B), ("attwarp_version",), ctypes.c_int, exc, prefix)
    assert str(e.value).startswith(prefix) and len(str(e.value)) > len(prefix) + 8, str(e.value)       # the library's own words follow
    assert (exc is ValueError) != isinstance(e.value, _lib.AttWarpError)


def test_the_sites_pass_those_classes_and_prefixes():
    """The two sites that plan without a device, through their own code: an empty list reaches the library with B = 0."""
    from attwarp_amd import jpeg
    with pytest.raises(ValueError, match=r"^jpeg: jpegdec_table_bytes: B=0"):
        jpeg.plan([])
    import inspect
    from attwarp_amd import dataloader, pipeline, png
    for mod, cls, prefix in ((pipeline, "RaggedBatch", "attwarp_ragged_table_bytes: "), (pipeline, "ClipBatch", "attwarp_clip_images_table_bytes: "),
                             (dataloader, "PreparedImages", "attwarp_prep_images_table_bytes: "), (png, "PngBatch", "PngBatch: "),
                             (png, "PngFiles", "PngFiles: ")):
        src = inspect.getsource(getattr(mod, cls).__init__)
        assert src.count("planned_table(") == 1 and f'"{prefix}"' in src and "attwarp_last_error" not in src, cls


def test_planned_table_plans_and_wraps_the_planners_error():
    rec = np.zeros(1, dtype=np.dtype(_lib.PngImage))
    rec["src"], rec["H"], rec["W"], rec["C"], rec["pitch"] = 256, 3, 5, 3, 15
    rec["order"], rec["filter"] = _lib.RGB, _lib.PNG_FILTER_IDS["sub"]
    rp = ctypes.c_void_p(rec.ctypes.data)
    table, header = _batch.planned_table(("attwarp_png_table_bytes", rp, 1), ("attwarp_png_plan", rp, 1, _batch.TABLE), _lib.PngHeader, ValueError, "PngBatch: ")
    assert table.dtype == np.uint8 and table.size == _lib.load().attwarp_png_table_bytes(rp, 1) and header.out_bytes >= 3 * 16 + 57
    assert ctypes.addressof(header) == table.ctypes.data
    bad = np.zeros(1, dtype=np.dtype(_lib.JpegDecImage))        # the size depends on B alone; the planner refuses a 0 x 0 image
    bp = ctypes.c_void_p(bad.ctypes.data)
    for wrap, exc in ((True, ValueError), (False, _lib.AttWarpError)):
        with pytest.raises(exc) as e:
            _batch.planned_table(("attwarp_jpegdec_table_bytes", bp, 1), ("attwarp_jpegdec_plan_ex", bp, 1, _batch.TABLE, 0, 0),
                                 _lib.JpegDecHeader, ValueError, "jpeg: ", wrap_plan=wrap)
        assert str(e.value).startswith("jpeg: attwarp_jpegdec_plan_ex failed") == wrap and "attwarp_jpegdec_plan_ex failed" in str(e.value)


def test_the_staging_pool_keeps_its_old_names():
    from attwarp_amd import dataloader, grounding, jpeg, pipeline, png
    assert pipeline._upload is _batch._upload and pipeline._upload_filled is _batch._upload_filled
    assert grounding._upload_records is _batch.uploaded and png.file_bytes is jpeg.file_bytes is _batch.file_bytes
    assert not hasattr(pipeline, "_STAGING") and not hasattr(dataloader, "_pinned_upload")
    assert issubclass(png.PngFiles, _batch.FileBatch) and issubclass(jpeg.JpegFiles, _batch.FileBatch) and not issubclass(png.PngBatch, _batch.FileBatch)
