"""The restatement of the PNG encoder's match="lz" route (tests/pnglz_ref.py) and its corpus (tests/pnglz_cases.py) without
a GPU: every file inflates with zlib to the filtered bytes and decodes with Pillow to the source pixels, every `expect` of
every case holds, an LZ file is never longer than png_ref's and equals it byte for byte when no segment chose LZ, and the
glyph pages shrink to 0.80 of the RLE file or less.  The ratios to zlib and Pillow are printed (DESIGN.md 3.24 quotes them)."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_limit_cases as L
import png_ref as R
import pnglz_cases as C
import pnglz_ref as Z

NAMES = [c.name for c in C.cases()]


def far_tokens(info):
    return [(t[1], t[2]) for seg in info for t in seg["tokens"] if t[0] == "match" and t[2] > 1]


def first_segment(c):
    fs = R.filtered_stream(c.image, c.filter, c.order)
    r0, nr = R.segments(*fs.shape)[0]
    return fs[r0:r0 + nr].tobytes()


def starts(tokens):
    out, i = {}, 0
    for t in tokens:
        out[i] = t
        i += t[1] if t[0] == "match" else 1
    return out, i


@pytest.mark.parametrize("name", NAMES)
def test_case_decodes_and_reaches_its_limit(name):
    c = C.case(name)
    f, routes, info = C.reference(name)
    fs = R.filtered_stream(c.image, c.filter, c.order)
    assert zlib.decompress(R.idat_payload(f)) == fs.tobytes()
    pix = c.image[:, :, ::-1] if c.order == "bgr" and c.image.shape[2] == 3 else c.image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))).reshape(pix.shape), pix)
    rle = R.encode(c.image, c.filter, c.order)
    assert len(f) <= len(rle) <= R.bound(*c.image.shape)
    if Z.ROUTE_LZ not in routes:
        assert f == rle
    e = c.expect
    if c.match == "rle":
        assert f == rle and not e
        return
    d = first_segment(c)
    cand = Z.candidates(d)
    at, end = starts(info[0]["tokens"])
    assert end == len(d) == info[0]["n"]
    far = far_tokens(info)
    assert all(2 <= dist <= R.SEG_BYTES - 4 and Z.FAR_MIN <= n <= 258 for n, dist in far)
    for m in e.get("matches", []):
        assert m in far, (m, far[:20])
    for dist in e.get("distances", []):
        assert dist in {d_ for _, d_ in far}, dist
    if "no_far_length" in e:
        assert all(n != e["no_far_length"] for n, _ in far)
    if "no_match" in e:
        assert e["no_match"] not in far
    if "route" in e:
        assert routes[0] == e["route"], info[0]["sizes"]
    if "routes" in e:
        assert set(routes) == e["routes"]
    if e.get("has_lz"):
        assert Z.ROUTE_LZ in routes
    if e.get("no_lz"):
        assert Z.ROUTE_LZ not in routes
    if "ratio" in e:
        assert len(f) <= e["ratio"] * len(rle), (len(f), len(rle))
    if e.get("last_token_ends_at_n"):
        last = max(at)
        assert at[last] == ("match",) + e["matches"][-1] and last + at[last][1] == len(d)
    if "max_dist_symbol" in e:
        s, eb, _ = Z.dist_symbol(max(dist for _, dist in far))
        assert (s, eb) == (e["max_dist_symbol"], 13) and max(dist for _, dist in far) == len(d) - 4
    hl, hd = Z.histograms(info[0]["tokens"])
    if "dist_symbols" in e:
        assert [s for s in range(30) if hd[s]] == e["dist_symbols"]
    if "dist_used" in e:
        assert sum(1 for h in hd if h) == e["dist_used"] and (e["dist_used"] != 1 or hd[0] == 0)
        assert e["dist_used"] > 2 or sum(Z.dist_lengths(hd)) == (1 if e["dist_used"] < 2 else 2)
    if "dist_depth" in e:                                                          # the distance code at the limiter's limit
        assert max(R.huffman_depths(hd)) == e["dist_depth"]
        assert (L.limiter_rounds(hd) > 0) == e["dist_limited"] and max(Z.dist_lengths(hd)) <= 15
        assert {t[1] for t in info[0]["tokens"] if t[0] == "match"} <= {4, 7}
    if "max_dist_code" in e:
        assert max(Z.dist_lengths(hd)) == e["max_dist_code"]
    if "candidate" in e:
        assert int(cand[e["candidate"][0]]) == e["candidate"][1]
    if "token_at" in e:
        i, tok = e["token_at"]
        assert at.get(i) == tok and Z.common_prefix(d, i, int(cand[i]), 258) == tok[1]       # (the far match is as long: a tie)
    if "literal_at" in e:
        assert at.get(e["literal_at"]) == ("lit", d[e["literal_at"]])
    if "size_diff" in e:
        assert info[0]["sizes"][0] - info[0]["sizes"][1] == e["size_diff"]
    if "segments_equal" in e:
        a, b = e["segments_equal"]
        segs = [Z.encode_segment(fs[r0:r0 + nr].tobytes())[0] for r0, nr in R.segments(*fs.shape)]
        assert segs[a] == segs[b] and b"".join(segs) == R.idat_payload(f)[2:-9]


def test_short_segments_have_no_key():
    assert Z.hashes(b"\0\1\2").size == 0 and Z.hashes(b"\0\1\2\3").size == 1
    assert (Z.candidates(bytes(range(200)) * 3)[:256] == -1).all()             # the first block has no candidate


def test_batch_positions_share_one_reference():
    assert C.reference("small_first")[0] == C.reference("small_middle")[0] == C.reference("small_last")[0]


def test_sizes_against_zlib_and_pillow(capsys):
    """Printed, not asserted: what the rule leaves on the table."""
    with capsys.disabled():
        for name in ("glyph_grey", "glyph_rgb"):
            c = C.case(name)
            f = C.reference(name)[0]
            filt = R.filtered_stream(c.image, c.filter, c.order).tobytes()
            buf = io.BytesIO()
            Image.fromarray(c.image[:, :, 0] if c.image.shape[2] == 1 else c.image).save(buf, "PNG")
            z1, z6 = len(zlib.compress(filt, 1)), len(zlib.compress(filt, 6))
            z = len(R.idat_payload(f))
            print(f"\n{name}: lz file {len(f)}, rle file {len(R.encode(c.image, c.filter, c.order))}; stream / zlib level 1 = {z / z1:.2f}, "
                  f"/ level 6 = {z / z6:.2f}; file / Pillow's default = {len(f) / len(buf.getvalue()):.2f}")
