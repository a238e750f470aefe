"""The JPEG encoder's limit cases (tests/jpegenc_limit_cases.py) proved without a GPU: for every case the file put together
unit by unit (R.assemble_by_units, the restatement of launches 3 .. 7) equals R.encode's and Pillow's, whole file; its length
is within the bound; every ``expect`` holds.  Then the proof that the cases close a gap: every seeded defect of the assembly
(R.DEFECTS) changes the bytes of a named case of the class meant for it, and the 69-case corpus of tests/jpegenc_cases.py
notices only two of them."""
import numpy as np
import pytest

import jpegenc_cases as K
import jpegenc_limit_cases as L
import jpegenc_ref as R
from test_jpegenc_ref_cpu import pillow_file

NAMES = [c[0] for c in L.cases()]

# defect -> (class, the named case that notices it)
COVERAGE = {
    "bits_carry_dropped": ("scan_chunks", "chunk_257_420"),
    "bytes_carry_dropped": ("scan_chunks", "chunk_257_420"),
    "files_carry_dropped": ("batch", 257),
    "interval_in_chunk": ("scan_chunks", "chunks_grey_520"),
    "straddle_one_unit": ("sub_byte", "shared_straddle_8x136"),
    "empty_unit_no_marker": ("sub_byte", "flat129_8x136"),
    "empty_unit_marker_late": ("sub_byte", "flat129_8x136"),
    "upos0_without_interval": ("scan_chunks", "chunks_grey_520"),
    "rst_not_modulo": ("scan_chunks", "chunks_grey_520"),
    "row_address_32bit": ("far_rows", "far_grey"),
}
# what the corpus of tests/jpegenc_cases.py alone notices (measured by test_the_old_corpus_alone_misses_the_assembly_defects)
OLD_CORPUS_NOTICES = {"upos0_without_interval", "rst_not_modulo"}


def differs(plans, defect, want):
    """'' when the defective assembly still gives the files ``want``, else how it shows."""
    try:
        files, _ = R.assemble_batch(plans, defect)
    except R.AssemblyError:
        return "leaves its buffers"
    return "" if files == want else "other bytes"


@pytest.mark.parametrize("name", NAMES)
def test_assembly_equals_restatement_equals_pillow(name):
    _, img, kw, expect = L.case(name)
    want, got = pillow_file(img, **kw), L.reference(name)
    assert got == want, (len(got), len(want), next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), -1))
    assert L.assembled(name)[0] == got
    assert len(got) <= L.plan(name)["bound"]
    m = L.measure(name)
    for k, v in expect.items():
        assert m[k] == v, (k, m[k], v)


def test_single_image_entry_and_its_info():
    _, img, kw, _ = L.case("flat129_8x136")
    info = {}
    assert R.assemble_by_units(img, info=info, **kw) == L.reference("flat129_8x136") == R.encode(img, **kw)
    assert info["owned"] == [13, 0] and info["owning_none"] == 1 and info["fpos"] == [0, 13] and info["upos"] == [0, 13]
    with pytest.raises(ValueError):
        R.assemble_by_units(img, defect="no such defect")


def test_classes_reach_what_they_claim():
    m = {n: L.measure(n) for n in NAMES}
    sub = [m[c[0]] for c in L.group("sub_byte")]
    assert min(min(x["unit_bits"]) for x in sub) == 6 and {14} <= {b for x in sub for b in x["unit_bits"]}
    assert sum(x["owning_none"] for x in sub) == 8 and not any(any(x["ff_ends"]) for x in sub)
    assert {(x["unit_bits"][0] % 8) for x in sub if x["unit_bits"][1] == 6} == {1, 2, 3, 6}
    assert sorted(m[c[0]]["units"] for c in L.group("scan_chunks")) == [256, 257, 270, 514]
    assert max(m[c[0]]["chunks"] for c in L.group("extreme")) == 32 and m["column_grey_rst"]["rst_wraps"] == 1023
    assert m["row_grey_rst8"]["units"] * R.UNIT_MCUS >= 8188 and R.MAX_DIM == 65500
    # a full unit of every sampling takes 0.45 .. 0.46 of its slot (recorded, from the restatement)
    assert [m[c[0]]["slot_share"] for c in L.group("near_worst")] == [0.4509, 0.4627, 0.4508]
    # the corpus of jpegenc_cases.py has no unit below a byte and no image of more than eleven units
    old = [K._encoded(n)[1]["unit_bits"] for n, *_ in K.cases()]
    assert min(min(u) for u in old) == 8 and max(len(u) for u in old) == 11


@pytest.mark.parametrize("n", L.BATCH_SIZES)
def test_batches_assemble_to_their_files(n):
    batch = L.batch(n)
    plans = [p for _, p in batch]
    files, offsets = R.assemble_batch(plans)
    want = [p["file"] for p in plans]
    assert files == want and offsets == np.r_[0, np.cumsum([len(f) for f in want])].tolist()
    assert len({len(f) for f in want}) >= 100 and [i for i, (c, _) in enumerate(batch) if c[0] == L.MANY_UNITS] == \
        {255: [0], 256: [255], 257: [128], 600: [0, 300, 599]}[n]
    for (name, img, kw, _), p in batch[:: 1 if n == 600 else 37]:              # every tiny image is one of the 600
        assert p["file"] == pillow_file(img, **kw), name


def test_every_defect_is_noticed_by_a_named_case_of_its_class():
    assert set(COVERAGE) == set(R.DEFECTS)
    shown = {}
    for defect, (cls, name) in COVERAGE.items():
        if cls == "batch":
            plans = [p for _, p in L.batch(name)]
            shown[defect] = differs(plans, defect, [p["file"] for p in plans])
            assert not differs([p for _, p in L.batch(256)], defect, [p["file"] for _, p in L.batch(256)])     # 256 files are one chunk
        elif cls == "far_rows":
            _, img, kw, _ = L.case(name)
            assert name in [c[0] for c in L.group(cls)]
            fetched = R.source_rows(img, L.FAR_PITCH, defect)
            assert R.source_rows(img, L.FAR_PITCH) is img
            wrong = np.flatnonzero((fetched != img).reshape(L.FAR_H, -1).any(1))
            assert wrong.size and int(wrong[0]) * L.FAR_PITCH >= 1 << 31 > int(wrong[0] - 1) * L.FAR_PITCH     # the first row behind 2^31
            shown[defect] = "other bytes" if R.encode(fetched, **kw) != L.reference(name) else ""
        else:
            assert name in [c[0] for c in L.group(cls)]
            shown[defect] = differs([L.plan(name)], defect, [L.reference(name)])
    print({d: (COVERAGE[d][1], how) for d, how in shown.items()})
    assert all(shown.values()), shown
    # the chunk boundary from both sides: 256 units are one chunk, no carry is needed yet
    for defect in ("bits_carry_dropped", "bytes_carry_dropped", "interval_in_chunk"):
        assert not differs([L.plan("chunk_256_420")], defect, [L.reference("chunk_256_420")])
    # [99, 6] owns a byte, [98, 6] does not: only the second notices a marker that an empty unit loses
    assert not differs([L.plan("flat130_8x136")], "empty_unit_no_marker", [L.reference("flat130_8x136")])


def test_the_old_corpus_alone_misses_the_assembly_defects():
    """The 69 cases of jpegenc_cases.py, each alone and all in one batch as test_jpegenc_gpu.py encodes them, against every
    seeded defect: they notice an interval that starts a byte early and an RSTn that is not taken modulo 8, and nothing else:
    neither scan carry, nor the straddle walk (c), nor the marker of a unit that owns no byte (d)."""
    old = [R.unit_plan(img, **kw) for _, img, kw, _ in K.cases()]
    want = [p["file"] for p in old]
    assert want == [K.reference(c[0]) for c in K.cases()]
    noticed = set()
    for defect in R.DEFECTS:
        if defect == "row_address_32bit":                                      # the old pitch test: 19 rows, 87 bytes apart
            img = K.photo(19, 27, 3, 2)
            if not np.array_equal(R.source_rows(img, 87, defect), img):
                noticed.add(defect)
        elif differs(old, defect, want) or any(differs([p], defect, [f]) for p, f in zip(old, want)):
            noticed.add(defect)
    assert noticed == OLD_CORPUS_NOTICES
    assert not {"straddle_one_unit", "empty_unit_no_marker", "empty_unit_marker_late"} & noticed
