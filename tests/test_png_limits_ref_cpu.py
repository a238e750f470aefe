"""The PNG encoder's limit corpus (tests/png_limit_cases.py) proved without a GPU: Pillow decodes the restatement's file of
every case to the source pixels, zlib inflates its stream to an independently written filter's output, the file stays within
the bound, and EVERY entry of the case's `expect` -- the limit the image is built to hit -- holds, computed from the
restatement (tests/png_ref.py).  These are conditions on the inputs: a builder that stops reaching its limit fails here."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_limit_cases as L
import png_ref as R

CASES = L.cases()
IDS = [c.name for c in CASES]
# built to defeat the Huffman code (a 153-byte block header around a handful of tokens, or frequencies the limiter flattens):
# their size against zlib's Z_RLE is reported, not asserted
REPORTED = {"code15_exact", "limiter_2_rounds", "limiter_3_rounds", "limiter_deepest", "tie_dynamic", "tie_stored_by_one"}


def spec_filters(a):
    """The specification's formulas on the whole image: a [H,W,C] uint8 -> [5, H, W C] filtered bytes, one plane per filter."""
    H, W, C = a.shape
    x = np.zeros((H + 1, W * C + C), np.int16)
    x[1:, C:] = a.reshape(H, W * C)
    cur, left, up, ul = x[1:, C:], x[1:, :-C], x[:-1, C:], x[:-1, :-C]
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    return np.stack([((cur - pred) % 256).astype(np.uint8) for pred in (np.zeros_like(cur), left, up, (left + up) // 2, paeth)])


def costs(planes, as_128=128):
    """[5, H] sums of |int8| of the filtered bytes; a byte of 128 counts `as_128`."""
    v = planes.astype(np.int64)
    return np.where(v == 128, as_128, np.where(v < 128, v, 256 - v)).sum(2)


def file_order(c):
    return c.image[:, :, ::-1] if c.order == "bgr" and c.image.shape[2] == 3 else c.image


# ---- one checker per key of `expect`: (case, facts, value) ---------------------------------------------------------------------
def _hist(f):
    return f["hist"]


def check_len15(c, F, syms):
    assert all(F[0]["lens"][s] == 15 for s in syms) and max(F[0]["lens"]) == 15
    assert any(281 <= s <= 284 for s in syms) and 256 in syms                  # five extra bits behind a 15-bit code; end of block


def check_equal_after_halving(c, F, k):
    rounds = L.halvings(_hist(F[0]))[1:]
    assert any(max(np.bincount([f for f in fr if f])) >= k for fr in rounds)


def check_split_runs(c, F, runs):
    seen = {n for f in F for n in f["run_lengths"]}
    assert set(runs) <= seen
    for n in runs:
        r = n - 1
        assert [v for k, v in R.tokens(bytes([9]) * n) if k == "len"] == [258] * (r // 258) + ([r % 258] if r % 258 >= 3 else [])
    assert {(n - 1) % 258 for n in runs} == {0, 1, 2, 3, 257}


def check_ties_through_128(c, F, _):
    planes = spec_filters(file_order(c))
    cost = costs(planes)
    best = cost.min(0)
    tied_128 = [r for r in range(cost.shape[1]) if (cost[:, r] == best[r]).sum() >= 2 and
                any((planes[t, r] == 128).any() for t in range(5) if cost[t, r] == best[r])]
    assert len(tied_128) >= 3
    winners = [r for r in tied_128 if (planes[int(np.argmin(cost[:, r])), r] == 128).any()]
    assert winners and len(winners) < len(tied_128)                            # the 128 on the winner's side, and on a loser's
    for wrong in (127, 129):                                                   # the choice depends on 128 counting 128
        assert (np.argmin(costs(planes, wrong), 0) != np.argmin(cost, 0)).any()


CHECK = {
    "nseg": lambda c, F, v: len(F) == v and len(R.segments(c.image.shape[0], 1 + c.image.shape[1] * c.image.shape[2])) == v,
    "depth": lambda c, F, v: [f["depth"] for f in F] == [v] * len(F),
    "rounds": lambda c, F, v: [f["rounds"] for f in F] == [v] * len(F),
    "stored": lambda c, F, v: [f["stored"] for f in F] == v,
    "len15": check_len15,
    "equal_after_halving": check_equal_after_halving,
    "run_lengths": lambda c, F, v: all(f["run_lengths"] == v for f in F),
    "ntokens": lambda c, F, v: all(f["ntokens"] == v for f in F),
    "match_lengths": lambda c, F, v: all(f["match_lengths"] == v for f in F),
    "all_match_lengths": lambda c, F, v: {n for f in F for n in f["match_lengths"]} == set(range(3, 259)),
    "split_runs": check_split_runs,
    "used_symbols": lambda c, F, v: sum(1 for h in _hist(F[0]) if h) == v == len(_hist(F[0])),
    "dyn_minus_n": lambda c, F, v: F[0]["dyn_bytes"] - F[0]["n"] == v,
    "out_len": lambda c, F, v: all(f["out_len"] == v for f in F),
    "min_out_len": lambda c, F, v: all(f["out_len"] >= v for f in F),
    "stored_count": lambda c, F, v: sum(f["stored"] for f in F) == v,
    "stored_out_len": lambda c, F, v: all(f["out_len"] == v for f in F if f["stored"]),
    "max_dynamic_out_len": lambda c, F, v: all(f["out_len"] <= v for f in F if not f["stored"]),
    "seg_rows": lambda c, F, v: [len(f["ftypes"]) for f in F] == v,
    "ftypes_used": lambda c, F, v: sorted({t for f in F for t in f["ftypes"]}) == v,
    "ftypes": lambda c, F, v: [t for f in F for t in f["ftypes"]] == v,
    "ties_through_128": check_ties_through_128,
    "tail": lambda c, F, v: (c.image.shape[1] * c.image.shape[2]) % 12 == v,
    "groups": lambda c, F, v: (c.image.shape[1] * c.image.shape[2]) // 12 == v,
    "odd_placement": lambda c, F, v: isinstance(v, bool),
}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_decodes_inflates_and_reaches_its_limit(c):
    png = L.reference(c.name)
    want = file_order(c)
    H, W, C = c.image.shape
    assert c.image.dtype == np.uint8 and c.image.nbytes <= 8 << 20
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert np.array_equal(got.reshape(want.shape), want)
    assert len(png) <= R.bound(H, W, C)
    z = R.idat_payload(png)
    raw = zlib.decompress(z)
    stream = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * C)
    ftypes = stream[:, 0]
    planes = spec_filters(want)
    assert np.array_equal(stream[:, 1:], planes[ftypes, np.arange(H)])
    if c.filter == "adaptive":                               # each row took the cheapest filter, ties to the lower number
        assert np.array_equal(ftypes, np.argmin(costs(planes), 0))
    else:
        assert (ftypes == R.FILTERS[c.filter]).all()
    F = L.facts(c.name)
    assert c.expect and set(c.expect) <= set(CHECK)
    for key, value in c.expect.items():                      # the limit the case is built to hit
        ok = CHECK[key](c, F, value)
        assert ok is None or ok, (c.name, key, value, [{k: v for k, v in f.items() if k not in ("hist", "lens", "ftypes")} for f in F[:4]])
    comp = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    rle = comp.compress(raw) + comp.flush()
    print(f"{c.name}: {len(z)} bytes, zlib Z_RLE level 1 {len(rle)}, ratio {len(z) / len(rle):.4f}, {len(F)} segment(s), "
          f"depth {max(f['depth'] for f in F)}, rounds {max(f['rounds'] for f in F)}")
    if c.name not in REPORTED:
        assert len(z) <= 1.02 * len(rle) + 192 * len(F) + 16


def test_the_corpus_is_the_one_the_limits_ask_for():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for n in ("code15_exact", "limiter_2_rounds", "limiter_3_rounds", "limiter_deepest", "single_run_segment", "every_match_length",
              "all_286_symbols", "tie_dynamic", "tie_stored_by_one", "full_segment_stored", "full_segment_dynamic", "rgb_full_row",
              "many_segments", "many_rows_adaptive", "adaptive_constant", "adaptive_128"):
        assert n in names
    # all but the many-segment case and the full rows are a few KB
    small = [c for c in CASES if c.name not in ("many_segments", "single_run_segment", "full_segment_stored", "full_segment_dynamic",
                                                "rgb_full_row", "every_match_length", "limiter_3_rounds", "limiter_deepest")]
    assert all(c.image.nbytes <= 9000 for c in small)
    assert L.case("code15_exact").image.shape[0] == 1 and L.case("single_run_segment").image.shape == (2, 24575, 1)
    assert L.case("tie_dynamic").image.shape == (1, 153, 1) and L.case("tie_stored_by_one").image.shape == (1, 152, 1)
    assert not L.case("tie_dynamic").image.any() and not L.case("single_run_segment").image.any()
    assert L.case("many_segments").image.shape == (600, 12288, 1) and L.case("many_rows_adaptive").image.shape == (2049, 1, 1)
    assert L.case("rgb_full_row").image.shape == (2, 8191, 3) and (L.case("rgb_full_row").filter, L.case("rgb_full_row").order) == ("paeth", "bgr")
    stored = [f["stored"] for f in L.facts("many_segments")]
    assert [i for i, s in enumerate(stored) if s] == list(range(0, 600, 37))       # stored blocks among the small ones


def test_tails_cover_every_residue_filter_and_order():
    tails = [c for c in CASES if c.name.startswith("tail_")]
    assert 150 <= len(tails) <= 400 and all(c.image.shape[0] == 5 for c in tails)
    for C, order, reach in ((1, "rgb", range(12)), (3, "rgb", (0, 3, 6, 9)), (3, "bgr", (0, 3, 6, 9))):
        for filt in R.FILTERS:
            mine = [c for c in tails if (c.image.shape[2], c.order, c.filter) == (C, order, filt)]
            wc = {c.image.shape[1] * C for c in mine}
            assert {n % 12 for n in wc} == set(reach) and {12, 24, 36} <= wc, (C, order, filt)
            assert all(c.expect["tail"] == (c.image.shape[1] * C) % 12 for c in mine)
            assert 3 * sum(c.expect["odd_placement"] for c in mine) >= len(mine)   # a third at odd addresses, in every sweep
    assert 3 * sum(c.expect["odd_placement"] for c in tails) >= len(tails)


def test_limiter_round_counter_agrees_with_the_restatement():
    """halvings / limiter_rounds repeat R.code_lengths' loop: the last frequencies' tree IS the restatement's code."""
    for name in ("code15_exact", "limiter_2_rounds", "limiter_3_rounds", "limiter_deepest", "all_286_symbols"):
        hist = L.facts(name)[0]["hist"]
        hv = L.halvings(hist)
        assert R.huffman_depths(hv[-1]) == R.code_lengths(hist) and L.limiter_rounds(hist) == len(hv) - 1
        assert all(max(R.huffman_depths(fr)) > 15 for fr in hv[:-1])
        lens = R.code_lengths(hist)
        assert max(lens) <= 15 and sum(2.0 ** -l for l in lens if l) == 1.0


def test_guard_batch_reaches_every_destination_residue():
    """The sub-batch of the guard-byte test: from the restatement's lengths alone, the segments' destinations offset + 43 +
    pre cover all four residues mod 4 at each of the four buffer alignments; many_segments stands between small images."""
    names = L.guard_batch()
    assert {"tie_dynamic", "tie_stored_by_one", "code15_exact", "full_segment_stored", "many_segments"} <= set(names)
    assert sum(n.startswith("tail_") for n in names) == L.GUARD_TAILS and len(set(names)) == len(names)
    i = names.index("many_segments")
    assert 0 < i < len(names) - 1 and sum(len(L.facts(n)) for n in names[:i]) >= 1
    addr = np.array(L.segment_addresses(names))
    assert addr.size == sum(len(L.facts(n)) for n in names)
    for k in range(4):
        assert set(((addr + k) % 4).tolist()) == {0, 1, 2, 3}
        assert set(((addr[:i] + k) % 4).tolist()) | set(((addr[i + 600:] + k) % 4).tolist()) == {0, 1, 2, 3}
