"""The JPEG encoder's planner and the Python side of the two file encoders against a recording
(tests/golden/jpegenc_plan.json.gz) made with the code as it stood BEFORE the planner became one plan of an image and
``PngBatch`` / ``JpegBatch`` one batch core: the planned tables (SHA-256 and every header field) of every record list that
test_jpegenc_host_cpu.py, test_jpegopt_host_cpu.py, test_jpegprogenc_host_cpu.py and jpegenc_limit_cases.py plan, each with
no flags, with ``optimize`` on some images, with ``progressive`` on some, with both mixed and with every image progressive
(``nunits == 0``); the three bounds of every image; the text of every planner refusal; the class and message of everything
the Python side raises before it needs a device.  Fake source pointers and CPU tensors: nothing is launched.  No tolerance.

The recording is made by running this file on a checkout of the older code (built there with its own Makefile), never
with the code under test: ``python tests/test_jpegenc_recording_cpu.py <root of that checkout>`` writes the fixture."""
import ctypes
import gzip
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

import jpegenc_limit_cases as L
import jpegenc_ref as R
import jpegprogenc_ref as P
import test_jpegenc_host_cpu as HE
import test_jpegopt_host_cpu as HO
import test_jpegprogenc_host_cpu as HP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpegenc_plan.json.gz")
PLAN_CAP = 64 << 20                                          # tables above it are counted (table_bytes), not planned
WAYS = ("plain", "optimize", "progressive", "mixed", "all_progressive")


def tallest(bound, C=1, q=75, sub="4:2:0"):
    """The tallest image of full width whose ``bound`` stays below 2 GiB (the bisection of the host tests)."""
    H, hi = 1, R.MAX_DIM + 1
    if bound(R.MAX_DIM, R.MAX_DIM, C, q, sub) < 1 << 31:
        return R.MAX_DIM
    while hi - H > 1:
        mid = (H + hi) // 2
        H, hi = (mid, hi) if bound(mid, R.MAX_DIM, C, q, sub) < 1 << 31 else (H, mid)
    return H


def case_records(cases):
    """The records of (name, image, keywords of R.encode, expect) cases, as JpegBatch would fill them for dense images."""
    from attwarp_amd import _lib
    shapes = [(a.shape[0], a.shape[1], 3 if a.ndim == 3 else 1) for a in (np.asarray(c[1]) for c in cases)]
    kws = [c[2] for c in cases]
    rec = HE.records(shapes, quality=[k.get("quality", 75) for k in kws], restart_rows=[k.get("restart_rows", 0) for k in kws],
                     subsampling=[R.SUBSAMPLING_IDS[k.get("subsampling", "4:2:0")] for k in kws])
    rec["order"] = [_lib.BGR if k.get("order") == "bgr" else _lib.RGB for k in kws]
    return rec


def record_lists():
    """[(label, records)]: every list the four files plan or have refused."""
    rec = HE.records
    out = [("enc_five", rec([(1, 1, 1), (33, 47, 3), (40, 25, 3), (500, 500, 3), (17, 9, 1)], quality=[1, 30, 75, 95, 100],
                            subsampling=[0, 1, 2, 0, 1], restart_rows=[0, 1, 2, 0, 1])),
           ("opt_five", HO.records(HO.SHAPES, **HO.KW)), ("prog_five", HP.records_of(HP.SHAPES, **HP.KW)),
           ("opt_pair", HO.records([(8, 8, 3), (8, 8, 1)]))]
    out += [(f"refused_{n}", r) for n, r in enumerate([
        rec([(8, 8, 3)], quality=0), rec([(8, 8, 3)], quality=101), rec([(8, 8, 3)], subsampling=3), rec([(8, 8, 2)]), rec([(0, 8, 3)]),
        rec([(8, 65501, 1)]), rec([(65501, 8, 1)]), rec([(8, 8, 3)], pitch=23), rec([(8, 8, 3), (8, 8, 3)], pitch=[24, 23]),
        rec([(8, 8, 3)], restart_rows=-1), rec([(1, 65500, 1)], restart_rows=9), rec([(8, 65500, 3)], restart_rows=17), rec([(1, 1, 1)])[:0]])]
    out += [("interval_grey_8", rec([(1, 65500, 1)], restart_rows=8)), ("interval_420_16", rec([(8, 65500, 3)], restart_rows=16)),
            ("wide_9", rec([(256, 65500, 3)], restart_rows=9)), ("wide_8", rec([(256, 65500, 3)], restart_rows=8))]
    for C, q, sub in ((1, 75, "4:2:0"), (3, 75, "4:2:0"), (3, 100, "4:4:4")):
        H = tallest(R.bound, C, q, sub)
        for dh in (0, 1):
            if H + dh <= R.MAX_DIM:
                out.append((f"two_gib_{C}_{q}_{sub}_{dh}", rec([(H + dh, R.MAX_DIM, C)], quality=q, subsampling=R.SUBSAMPLING_IDS[sub])))
    H = tallest(lambda h, w, c, q, sub: P.bound(h, w, c, q))
    out += [(f"two_gib_prog_{dh}", rec([(H + dh, R.MAX_DIM, 1)])) for dh in (0, 1)]
    out += [("batch_4096", rec([(1, 1, 1)] * 4096)), ("batch_2_20", rec([(1, 1, 1)] * (1 << 20))), ("batch_2_20_1", rec([(1, 1, 1)] * ((1 << 20) + 1))),
            ("units_42", rec([(20000, 20000, 1)] * 42, quality=1)), ("units_43", rec([(20000, 20000, 1)] * 43, quality=1))]
    for c in L.cases():
        r = case_records([c])
        if c in L.group("far_rows"):
            r["pitch"] = L.FAR_PITCH
        out.append((f"limit_{c[0]}", r))
    big = {255: (0,), 256: (255,), 257: (128,), 600: (0, 300, 599)}                 # (jpegenc_limit_cases.batch, without its plans)
    out += [(f"limit_batch_{n}", case_records([L.case(L.MANY_UNITS) if i in big[n] else L.tiny(i) for i in range(n)])) for n in L.BATCH_SIZES]
    return out


def flags_of(way, B):
    i = np.arange(B)
    opt, prog = (i % 2 == 0).astype(np.int32), (i % 3 == 0).astype(np.int32)
    return {"plain": (None, None), "optimize": (opt, None), "progressive": (None, prog), "mixed": (opt, prog),
            "all_progressive": (None, np.ones(B, np.int32))}[way]


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def planned(lib_mod, rec, opt, prog):
    """What the planner makes of one list: the bytes of the table, its digest and header, or the refusal's text; and what
    attwarp_jpegenc_plan_prog says to a table of 64 bytes."""
    lib, rp, B = lib_mod.load(), ctypes.c_void_p(rec.ctypes.data), len(rec)
    out = {}
    sizes = {"prog": lib.attwarp_jpegenc_table_bytes_prog(rp, B, _p(opt), _p(prog))}
    err = lib.attwarp_last_error().decode() if sizes["prog"] == 0 else None
    if prog is None:
        sizes["ex"] = lib.attwarp_jpegenc_table_bytes_ex(rp, B, _p(opt))
    if prog is None and opt is None:
        sizes["plain"] = lib.attwarp_jpegenc_table_bytes(rp, B)
    out["table_bytes"] = {k: int(v) for k, v in sizes.items()}
    n = int(sizes["prog"])
    if n == 0:
        out["refused"] = err
    try:
        lib_mod.call("attwarp_jpegenc_plan_prog", rp, B, _p(opt), _p(prog), np.zeros(64, np.uint8).ctypes.data, 64)
        out["small_table"] = None
    except lib_mod.AttWarpError as e:
        out["small_table"] = str(e)
    if 0 < n <= PLAN_CAP:
        table = np.full(n, 0xEE, np.uint8)
        lib_mod.call("attwarp_jpegenc_plan_prog", rp, B, _p(opt), _p(prog), table.ctypes.data, n)
        h = lib_mod.JpegEncHeader.from_buffer_copy(table[:ctypes.sizeof(lib_mod.JpegEncHeader)].tobytes())
        out["sha256"] = hashlib.sha256(table.tobytes()).hexdigest()
        out["header"] = {name: int(getattr(h, name)) for name, _ in lib_mod.JpegEncHeader._fields_}
        if prog is None:                                     # the older entries forward: the same bytes
            other = np.full(n, 0xEE, np.uint8)
            lib_mod.call("attwarp_jpegenc_plan_ex", rp, B, _p(opt), other.ctypes.data, n)
            out["ex_same"] = bool((other == table).all())
        if prog is None and opt is None:
            other = np.full(n, 0xEE, np.uint8)
            lib_mod.call("attwarp_jpegenc_plan", rp, B, other.ctypes.data, n)
            out["plain_same"] = bool((other == table).all())
    return out


def plan_outcomes(lib_mod):
    out = {}
    for label, rec in record_lists():
        for way in WAYS:
            out[f"{label}|{way}"] = planned(lib_mod, rec, *flags_of(way, len(rec)))
    pair = HO.records([(8, 8, 3), (8, 8, 1)])
    for name, flags in (("1_2", [1, 2]), ("-1_0", [-1, 0])):          # a flag outside 0 / 1
        f = np.asarray(flags, np.int32)
        out[f"flag_optimize_{name}"] = planned(lib_mod, pair, f, None)
        out[f"flag_progressive_{name}"] = planned(lib_mod, pair, None, f)
        out[f"flag_both_{name}"] = planned(lib_mod, pair, f, f)
    return out


def bound_outcomes(lib_mod):
    """attwarp_jpegenc_bound, _bound_ex and _bound_prog of every distinct image of the lists."""
    lib, out = lib_mod.load(), {}
    for _, rec in record_lists():
        if len(rec) == 0:
            continue
        keys = np.unique(np.stack([rec[k] for k in ("H", "W", "C", "quality", "subsampling", "restart_rows")], 1), axis=0)
        for H, W, C, q, sub, rr in keys.tolist():
            key = f"{H}x{W}x{C} q{q} s{sub} r{rr}"
            if key not in out:
                out[key] = [int(lib.attwarp_jpegenc_bound(H, W, C, q, sub, rr))] + [int(lib.attwarp_jpegenc_bound_ex(H, W, C, q, sub, rr, o)) for o in (0, 1, 2)] + \
                           [int(lib.attwarp_jpegenc_bound_prog(H, W, C, q, sub, rr, o, p)) for o in (0, 1) for p in (0, 1, 2)]
    return out


def raised(fn):
    try:
        fn()
        return {"raises": None}
    except Exception as e:                                   # the class and the message are what is recorded
        return {"raises": type(e).__name__, "message": str(e)}


def python_outcomes(pkg):
    """Everything PngBatch, JpegBatch, write_*, save_*_ragged raise for CPU tensors: a refusal of the arguments, or (the
    arguments being fine) the refusal of a tensor that is not on a GPU."""
    png, jpeg, pipeline = pkg.png, pkg.jpeg, pkg.pipeline
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    ok = u8(8, 8, 3)
    images = {"fine": [ok], "fine_grey": [u8(8, 8)], "fine_batch": u8(2, 8, 8, 3), "float": [torch.zeros(8, 8, 3)], "one_dim": [u8(8)], "four_dim": [u8(1, 8, 8, 3)],
              "four_channels": [u8(8, 8, 4)], "two_channels": [u8(8, 8, 2)], "empty_image": [u8(0, 8, 3)], "empty_width": [ok, u8(8, 0)], "empty_batch": [],
              "empty_tensor_batch": u8(0, 8, 8, 3), "three_dim_batch": u8(8, 8, 3), "five_dim_batch": u8(1, 1, 8, 8, 3),
              "strided_columns": [u8(8, 16, 3)[:, ::2]], "strided_channels": [u8(8, 8, 6)[:, :, ::2]], "strided_grey": [u8(8, 16)[:, ::2]],
              "transposed": [u8(8, 8, 3).permute(1, 0, 2)], "row_slices": [u8(8, 16, 3)[:, :8]], "reversed_rows": [u8(8, 16, 3)[:, :8][::2]],
              "wide_rgb": [u8(1, (png.PNG_MAX_ROW_BYTES - 1) // 3 + 1, 3)], "wide_grey": [u8(1, png.PNG_MAX_ROW_BYTES)], "widest_grey": [u8(1, png.PNG_MAX_ROW_BYTES - 1)],
              "above_max_dim_w": [u8(1, jpeg.JPEGENC_MAX_DIM + 1)], "above_max_dim_h": [u8(jpeg.JPEGENC_MAX_DIM + 1, 1)], "at_max_dim": [u8(1, jpeg.JPEGENC_MAX_DIM)],
              "second_bad": [ok, torch.zeros(8, 8, 3, dtype=torch.int8)]}
    out = {}
    for name, im in images.items():
        out[f"PngBatch|{name}"] = raised(lambda: png.PngBatch(im))
        out[f"JpegBatch|{name}"] = raised(lambda: jpeg.JpegBatch(im))
        out[f"encode_png|{name}"] = raised(lambda: png.encode_png(im))
        out[f"encode_jpeg|{name}"] = raised(lambda: jpeg.encode_jpeg(im))
    two = [ok, ok]
    png_kw = dict(filter=["bad", 3, None, ["sub"], ["sub", "up", "none"], ["sub", "bad"], ("sub", "up"), "adaptive"],
                  order=["xyz", 1, ["rgb"], ["rgb", "bgr", "rgb"], ["rgb", "bad"], "bgr"],
                  match=["bad", 0, ["lz"], ["lz", "rle", "lz"], ["lz", "bad"], ["lz", "rle"]])
    jpeg_kw = dict(quality=[0, 101, 75.0, True, "75", None, [75], [75, 80, 85], [75, 0], (50, 100), np.int64(30)],
                   subsampling=["4:1:1", 3, -1, 1.0, None, ["4:4:4"], ["4:4:4", "4:2:2", "4:2:0"], ["4:4:4", 5], (0, "4:2:0")],
                   restart_rows=[-1, 1 << 16, 1.0, False, [1], [1, 2, 3], [1, -1], (0, 65535)],
                   order=["xyz", 1, ["rgb"], ["rgb", "bgr", "rgb"], ["rgb", "bad"], ("rgb", "bgr")],
                   optimize=[1, 0, "yes", None, [True], [True, False, True], [True, 1], (True, np.bool_(False))],
                   progressive=[1, 0, "yes", None, [True], [True, False, True], [True, 1], (True, np.bool_(False))])
    for key, values in png_kw.items():
        for n, v in enumerate(values):
            out[f"PngBatch|{key}|{n}"] = raised(lambda: png.PngBatch(two, **{key: v}))
    for key, values in jpeg_kw.items():
        for n, v in enumerate(values):
            out[f"JpegBatch|{key}|{n}"] = raised(lambda: jpeg.JpegBatch(two, **{key: v}))
    out["PngBatch|out_ignored_on_cpu"] = raised(lambda: png.PngBatch(two, out=u8(4)))
    out["JpegBatch|out_ignored_on_cpu"] = raised(lambda: jpeg.JpegBatch(two, out=u8(4)))
    for name, (paths, im) in {"one_for_two": (["a"], two), "three_for_two": (["a", "b", "c"], two), "none_for_tensor": ([], u8(2, 8, 8, 3)),
                              "one_for_tensor": (["a"], u8(2, 8, 8, 3)), "two_for_three_dim": (["a", "b"], u8(8, 8, 3)), "eight_for_three_dim": (["a"] * 8, u8(8, 8, 3)),
                              "matching_list": (["a", "b"], two), "matching_tensor": (("a", "b"), u8(2, 8, 8, 3)), "none_for_none": ([], [])}.items():
        out[f"write_png|{name}"] = raised(lambda: png.write_png(paths, im))
        paths = list(paths)
        out[f"write_jpeg|{name}"] = raised(lambda: jpeg.write_jpeg(paths, im))
    for name, (rb, paths, what) in {"paths": (types.SimpleNamespace(B=2, C=3), ["a"], "warped"), "no_paths": (types.SimpleNamespace(B=2, C=3), [], "mota"),
                                    "what": (types.SimpleNamespace(B=1, C=3), ["a"], "masks"), "what_none": (types.SimpleNamespace(B=1, C=3), ["a"], None),
                                    "channels": (types.SimpleNamespace(B=1, C=4), ["a"], "warped"), "channels_2": (types.SimpleNamespace(B=1, C=2), ["a"], "warped"),
                                    "what_before_channels": (types.SimpleNamespace(B=1, C=4), ["a"], "both"),
                                    "warped_on_cpu": (types.SimpleNamespace(B=2, C=3, out=u8(2, 8, 8, 3)), ["a", "b"], "warped"),
                                    "mota_on_cpu": (types.SimpleNamespace(B=2, C=4, mota_of=lambda b: u8(8, 8)), ["a", "b"], "mota")}.items():
        out[f"save_png_ragged|{name}"] = raised(lambda: pipeline.save_png_ragged(rb, paths, what))
        out[f"save_jpeg_ragged|{name}"] = raised(lambda: pipeline.save_jpeg_ragged(rb, paths, what))
    return out


def outcomes(pkg):
    return dict(plans=plan_outcomes(pkg._lib), bounds=bound_outcomes(pkg._lib), python=python_outcomes(pkg))


_CACHE = {}


def recorded_and_found():
    if not _CACHE:
        import attwarp_amd
        from attwarp_amd import _lib, jpeg, pipeline, png    # noqa: F401 (the sub-modules the outcomes reach into)
        with gzip.open(GOLDEN, "rt") as fh:
            _CACHE["want"] = json.load(fh)
        _CACHE["got"] = json.loads(json.dumps(outcomes(attwarp_amd)))
    return _CACHE["want"], _CACHE["got"]


def _compare(part):
    want, got = recorded_and_found()
    assert sorted(got[part]) == sorted(want[part])
    for key in got[part]:
        assert got[part][key] == want[part][key], key
    return got[part]


def test_planned_tables_and_refusals_equal_the_recording_byte_for_byte():
    got = _compare("plans")
    tables = [v for v in got.values() if "sha256" in v]
    assert len(tables) >= 5 * 35 and sum("refused" in v for v in got.values()) >= 5 * 13 + 6      # (the recording: 178 and 121 of 306)
    assert any(v["header"]["nunits"] == 0 and v["header"]["reserved"] for v in tables)                    # every image progressive
    assert any(v["header"]["off_optimize"] and v["header"]["reserved"] for v in tables)                   # both records in one table
    assert all(v.get("ex_same", True) and v.get("plain_same", True) for v in tables)
    text = " ".join(str(v.get("refused")) + str(v["small_table"]) for v in got.values())
    for word in ("progressive must be 0 or 1", "optimize must be 0 or 1", "restart interval above 65535", "clamps it to 65535", "2 GiB or more",
                 "progressive bound", "quality (1 .. 100)", "unknown subsampling", "non-positive size", "size above 65500", "pitch", "2^20",
                 "channels (1 or 3)", "negative restart_rows", "units in one call", "non-positive batch size", "bytes, "):
        assert word in text, word


def test_bounds_equal_the_recording():
    got = _compare("bounds")
    assert len(got) >= 60 and any(v[0] and not v[2] for v in got.values()) and any(v[0] and not v[5] for v in got.values())


def test_python_refusals_equal_the_recording_class_and_message():
    got = _compare("python")
    assert all(v["raises"] for v in got.values())             # (a CPU tensor that passes every check is refused for its device)
    classes = {v["raises"] for v in got.values()}
    assert {"ValueError", "TypeError", "RuntimeError"} <= classes
    assert got["PngBatch|float"]["raises"] == "TypeError" and got["JpegBatch|float"]["raises"] == "ValueError"
    for who, word in (("PngBatch|wide_rgb", "PNG_MAX_ROW_BYTES"), ("JpegBatch|above_max_dim_w", "JPEGENC_MAX_DIM"), ("write_png|one_for_two", "write_png: 1 paths"),
                      ("write_jpeg|one_for_two", "write_jpeg: 1 paths"), ("save_png_ragged|what", "save_png_ragged: what is"),
                      ("save_jpeg_ragged|what", "save_jpeg_ragged: what is"), ("PngBatch|three_dim_batch", "png: a tensor batch"),
                      ("JpegBatch|three_dim_batch", "JpegBatch: a tensor batch"), ("PngBatch|empty_batch", "PngBatch: empty batch"),
                      ("JpegBatch|empty_batch", "JpegBatch: empty batch")):
        assert word in got[who]["message"], who


if __name__ == "__main__":                                    # the recorder: run on a checkout of the code to record
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    import attwarp_amd
    from attwarp_amd import _lib, jpeg, pipeline, png         # noqa: F401
    assert os.path.abspath(attwarp_amd.__file__).startswith(root) and os.path.abspath(_lib.LIB_PATH).startswith(root)
    text = json.dumps(outcomes(attwarp_amd), separators=(",", ":"), sort_keys=True)
    with open(GOLDEN, "wb") as fh, gzip.GzipFile("", "wb", 9, fh, mtime=0) as z:
        z.write(text.encode())
    print(GOLDEN, len(text), "bytes of JSON")
