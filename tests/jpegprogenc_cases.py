"""The corpus of the progressive tests of the JPEG encoder: named images at the smallest shape that can go
wrong, with their parameters and an ``expect`` that tests/test_jpegprogenc_ref_cpu.py proves from the restatement
(tests/jpegprogenc_ref.py) and Pillow before the GPU test encodes the same cases.  A case is ``(name, image, keywords of
jpegprogenc_ref.encode, expect)``.  ``expect`` keys (``measure`` computes them from the restatement): ``file_bytes``, ``dri``
(the DRI values along the file), ``rst_max`` (most RSTn markers in one scan), ``flush_7fff`` / ``flush_be`` (forced flushes of
the end-of-band run), ``zrl_refine`` / ``zrl_skipped`` (ZRL symbols of refinements; runs above 15 behind EOB that get none),
``neg_odd_dc``, ``c63`` (classes of |coefficient 63| present: 1, 2 for 2 .. 3, 4 for more), ``max_depth`` (deepest table before
limiting), ``lone_eobrun`` (scans whose only symbol is one EOBRUN), ``noticed_by`` (defects that change this case's file);
values with ``min_`` in front are lower bounds.  ``big``: the GPU test runs the case in a batch of its own."""
import functools

import numpy as np

import jpegenc_cases as K
import jpegenc_ref as R
import jpegopt_cases as OC
import jpegprogenc_ref as P


def from_coefficients(coefs, quality=50):
    """An 8 x 8 grey block whose quantised zigzag coefficients are ``coefs`` (position -> value) at ``quality``: the inverse
    DCT of the de-quantised values, rounded.  ``measure`` states what the encoder's own transform makes of it."""
    q = R.quant_tables(quality)[0]
    F = np.zeros((8, 8))
    for k, v in coefs.items():
        n = int(R.ZIGZAG[k])
        F[n // 8, n % 8] = v * int(q[n])
    c = np.array([[np.cos((2 * x + 1) * u * np.pi / 16) * (np.sqrt(0.5) if u == 0 else 1.0) for x in range(8)] for u in range(8)])
    b = 128 + 0.25 * c.T @ F @ c
    return np.clip(np.rint(b), 0, 255).astype(np.uint8)


def be_image():
    """200 copies of a block with 20 coefficients of magnitude 4 and more and nothing else: in the refinement 2 -> 1 every block
    adds 20 correction bits to the run and no symbol, so the pending bits pass 937 and the run is flushed early."""
    b = from_coefficients({k: (6 if k % 2 else -5) for k in range(1, 21)}, 75)
    return np.tile(b, (1, 200))


def runs_image():
    """Refinement runs above 15: zeros 1 .. 19 in front of a coefficient +-1 at 20 (a ZRL), zeros 21 .. 59 in front of a
    coefficient of magnitude 2 and more at 60 (behind EOB: no ZRL); and 2 -> 1 likewise with 2 and 5."""
    blocks = [from_coefficients({20: 1, 60: 2}), from_coefficients({20: -1, 60: -3}), from_coefficients({20: 2, 60: 5}),
              from_coefficients({20: -3, 60: -4}), from_coefficients({40: 1}), from_coefficients({1: 9, 63: 1})]
    return np.concatenate(blocks, 1)


def c63_image():
    """Coefficient 63 at magnitude 1, 2 .. 3 and 4 and more, each sign: the last coefficient of every band that ends at 63 is
    newly non-zero, a correction bit, or coded in the first pass."""
    return np.concatenate([from_coefficients({63: v}) for v in (1, -1, 2, -3, 4, -7, 12)] + [from_coefficients({6: 4, 63: -5})], 1)


def limiter_image(n=17):
    """jpegopt_cases' sequence a(k) for the first pass 6 - 63 at Al = 2: one coefficient per block, symbol (k - 6) << 4 | size,
    the n symbols in a(k) copies each; every block also ends its band, so EOBRUN 1 (symbol 0) is the most frequent symbol."""
    kinds = [(k, v) for v in (4, 8, 16) for k in range(6, 22)][:n]
    blocks = []
    for (k, v), copies in zip(kinds, OC.limiter_copies(n)):
        blocks += [from_coefficients({k: v})] * copies
    blocks += [np.full((8, 8), 128, np.uint8)] * (-len(blocks) % 64)
    return np.concatenate([np.concatenate(blocks[i:i + 64], 1) for i in range(0, len(blocks), 64)], 0)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    out.append(("grey_1x1", np.full((1, 1), 128, np.uint8), dict(), dict(lone_eobrun=4, dri=[])))
    out.append(("rgb_1x1", np.full((1, 1, 3), 200, np.uint8), dict(), dict(lone_eobrun=8)))
    # dummy blocks right / below / both, H % 16 == 8, per sampling and grey
    seed = 0
    for sub, c in (("4:2:0", 3), ("4:2:2", 3), ("4:4:4", 3), ("grey", 1)):
        for tag, (h, w) in (("right", (16, 24)), ("below", (24, 16)), ("both", (24, 24)), ("h40", (40, 25))):
            seed += 1
            kw = dict(quality=(75, 90, 60, 85)[seed % 4], restart_rows=seed % 3)
            if c == 3:
                kw["subsampling"] = sub
            e = dict()
            if sub == "4:2:0" and tag == "both":
                e["noticed_by"] = ["ac_dummy_blocks"]
            out.append((f"dummy_{tag}_{sub.replace(':', '')}", (K.photo if seed % 2 else K.noise)(h, w, c, 300 + seed), kw, e))
    # scans with different MCUs per row: DRI alternates
    for r, dri in ((0, []), (1, [4, 7, 4, 7, 4, 7]), (2, [8, 14, 8, 14, 8, 14])):
        e = dict(dri=dri)
        if r == 1:
            e["noticed_by"] = ["dri_repeated", "dri_omitted", "cb_before_cr", "eobrun_across_restart", "dc_shift_magnitude", "corr_before_sign"]
            e["min_neg_odd_dc"] = 1
        out.append((f"restart_{r}", K.noise(40, 56, 3, 11), dict(restart_rows=r), e))
    out.append(("rstn_wraps", K.photo(88, 16, 1, 12), dict(restart_rows=1, quality=80), dict(rst_max=10, dri=[2])))
    out.append(("smooth_restart", K.photo(64, 48, 3, 13), dict(restart_rows=1, quality=40), dict(noticed_by=["eobrun_across_restart"])))
    # forced flushes of the run
    out.append(("flat_7fff", np.full((1024, 2056), 77, np.uint8), dict(), dict(flush_7fff=4, flush_be=0, noticed_by=["no_7fff_split"], big=True)))
    out.append(("be_flush", be_image(), dict(quality=75), dict(min_flush_be=1, flush_7fff=0, noticed_by=["no_be_flush"], big=True)))
    out.append(("c63", c63_image(), dict(quality=50), dict(c63=[1, 2, 4])))
    out.append(("refine_runs", runs_image(), dict(quality=50), dict(min_zrl_refine=2, min_zrl_skipped=2, noticed_by=["zrl_past_eob"])))
    out.append(("limiter", limiter_image(), dict(quality=50), dict(min_max_depth=17, max_length=16, big=True)))
    # quality 1 and 100, both channel orders
    out.append(("q1", K.photo(33, 47, 3, 2), dict(quality=1, subsampling="4:2:2"), dict()))
    out.append(("q100", K.noise(24, 40, 3, 3), dict(quality=100, subsampling="4:4:4", restart_rows=2), dict()))
    out.append(("bgr", K.photo(33, 47, 3, 1), dict(order="bgr"), dict()))
    out.append(("rgb", K.photo(33, 47, 3, 1), dict(), dict()))
    # a full unit of near-worst content per sampling: the length stays within attwarp_jpegenc_bound_prog
    out.append(("worst_grey", OC.worst(8, 128, 1, 21), dict(quality=100), dict()))
    out.append(("worst_444", OC.worst(8, 128, 3, 22), dict(quality=100, subsampling="4:4:4"), dict()))
    out.append(("worst_422", OC.worst(8, 256, 3, 23), dict(quality=100, subsampling="4:2:2"), dict()))
    out.append(("worst_420", OC.worst(16, 256, 3, 24), dict(quality=100, subsampling="4:2:0"), dict()))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


def small_names():
    return [n for n, _, _, e in cases() if not e.get("big")]


@functools.lru_cache(maxsize=None)
def _encoded(name):
    _, img, kw, _ = case(name)
    info = {}
    return P.encode(img, info=info, **kw), info


def reference(name) -> bytes:
    """The restatement's file of a case, computed once."""
    return _encoded(name)[0]


def info(name) -> dict:
    return _encoded(name)[1]


def defect_file(name, defect):
    """The case's file under a defect of jpegprogenc_ref.DEFECTS; None where the defective coder needs a symbol beyond a table."""
    _, img, kw, _ = case(name)
    try:
        return P.encode(img, defect=defect, **kw)
    except (KeyError, ValueError):
        return None


def args_of(name):
    """(H, W, components, quality, subsampling, restart_rows) of a case."""
    _, img, kw, _ = case(name)
    a = np.asarray(img)
    return (a.shape[0], a.shape[1], 1 if a.ndim == 2 else 3, kw.get("quality", 75), kw.get("subsampling", "4:2:0"), kw.get("restart_rows", 0))


def bound_use(name):
    """The largest share of its bound (jpegprogenc_ref.interval_bound_bits) an interval of the case takes, and the file's
    share of jpegprogenc_ref.bound: from the restatement."""
    i = info(name)
    worst = 0.0
    for (nblk, step, nint, bpb, _, _), lens in zip(P.scan_geometry(*args_of(name)[:3], *args_of(name)[4:]), i["interval_bits"]):
        for k, n in enumerate(lens):
            worst = max(worst, n / P.interval_bound_bits(min(step, nblk - k * step), bpb))
    H, W, nc, q, sub, rr = args_of(name)
    return worst, len(reference(name)) / P.bound(H, W, nc, q, sub, rr)


def measure(name) -> dict:
    """What a case's ``expect`` is compared with, from the restatement."""
    data, i = _encoded(name)
    per_scan = []
    body = data
    for k in range(len(body) - 1):
        if body[k] == 0xff and body[k + 1] == 0xda:
            per_scan.append(0)
        elif body[k] == 0xff and 0xd0 <= body[k + 1] <= 0xd7 and per_scan:
            per_scan[-1] += 1
    luma = i["comps"][0].reshape(-1, 64)
    c63 = sorted({1 if v == 1 else (2 if v < 4 else 4) for v in np.abs(luma[:, 63]) if v})
    dcs = np.concatenate([c.reshape(-1, 64)[:, 0] for c in i["comps"]])
    syms = [[x[2] for x in t if x[0] == "s"] for t in i["tokens"]]
    lone = sum(1 for sc, y in zip(P.script(i["ncomp"]), syms) if sc[1] > 0 and y == [0])
    lengths = [n for bits, _ in i["tables"].values() for n in range(1, 17) if bits[n - 1]]
    return dict(file_bytes=len(data), dri=i["dri"], rst_max=max(per_scan), flush_7fff=i["flush_7fff"], flush_be=i["flush_be"],
                zrl_refine=i["zrl_refine"], zrl_skipped=i["zrl_skipped"], neg_odd_dc=int(((dcs < 0) & (dcs % 2 == 1)).sum()), c63=c63,
                max_depth=max(i["depths"].values()), max_length=max(lengths),
                lone_eobrun=lone,
                noticed_by=[d for d in case(name)[3].get("noticed_by", []) if defect_file(name, d) != data])


def pillow_keywords(kw):
    """Image.save's keywords for a case's (the order is applied to the pixels by the caller)."""
    out = {k: v for k, v in kw.items() if k in ("quality", "subsampling")}
    out["restart_marker_rows"] = kw.get("restart_rows", 0)
    out["progressive"] = True
    return out
