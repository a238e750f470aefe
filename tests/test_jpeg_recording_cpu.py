"""``jpeg.parse_jpeg`` and ``jpeg.plan`` against a recording (tests/golden/jpeg_parse_*.json.gz, jpeg_plan.json.gz) made with the
parser as it stood BEFORE its baseline and progressive tails became one walk: every file of the four JPEG corpora, good,
malformed and refused, with ``progressive`` False and True, gives the same dict or raises the same class with the same
message; the planned tables of the lists the other tests plan have the same SHA-256.  No tolerance anywhere.

The recording is made by running this file on a checkout of the older code, never with the code under test:
``python tests/test_jpeg_recording_cpu.py <root of that checkout>`` writes the fixtures (gzipped JSON: class and message per
case, dicts with byte strings as hex) into golden/.

The fixtures of the layout, scan and scan-sub-stream families (jpeg_parse_jpegfmt / jpegscan / jpegprog_sync, jpeg_plan_families)
were recorded the same way (``python tests/test_jpeg_recording_cpu.py <root> families``) from commit c528f74, the last one
before the planners and decode entry points of csrc/jpegdec.hip were written once over the record family: every file of tests/jpegfmt_cases.py, jpegscan_cases.py and jpegprog_sync_cases.py
under ``all_layouts`` and ``all_scans``, with and without ``progressive``, and the tables of attwarp_jpegdec_plan_layouts,
_plan_layout_scans and _plan_scans_ex for the lists their tests plan."""
import gzip
import hashlib
import json
import os
import sys

import jpegdec_cases as A
import jpegdec_limit_cases as L
import jpegdec_sync_cases as S
import jpegfmt_cases as F
import jpegprog_cases as P
import jpegprog_sync_cases as Y
import jpegscan_cases as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORPORA = {"jpegdec": (A, "good malformed refused"), "jpegdec_sync": (S, "good all_one_unit_good"),
           "jpegdec_limit": (L, "narrow extreme long_files long_cuts restart_files restart_damaged data_ends behind_end "
                                "smallest_plans cap_files"),
           "jpegprog": (P, "good malformed refused")}
FAMILIES = {"jpegfmt": (F, "good long_plain malformed refused"), "jpegscan": (N, "good malformed refused"),
            "jpegprog_sync": (Y, "limits larger")}
KEYWORDS = [dict(all_layouts=True), dict(all_layouts=True, progressive=True), dict(all_scans=True), dict(all_scans=True, progressive=True)]
INTERN = 24                                                  # characters of JSON above which a value is stored once


def files_of(corpus):
    mod, makers = CORPORA[corpus] if corpus in CORPORA else FAMILIES[corpus]
    return [(f"{m}/{i}:{c[0]}", c[1]) for m in makers.split() for i, c in enumerate(getattr(mod, m)())]


def plans():
    """(label, files, keywords of plan()) of every list the CPU tests of the four corpora plan."""
    base = [f for _, f in A.good()] + [f for _, f, _ in A.malformed()]
    sync = [A.good_file(n) for n in ("ri_wrap", "big_200x136", "noise_64x48_s1", "grey_17x15", "noise_1x1_s0")] + [f for _, f in S.good()]
    prog = [f for _, f in P.good() + P.malformed()]
    out = [("jpegdec", base, dict(mode="keep", order="rgb")), ("jpegdec_bgr_L", base, dict(mode="L", order="bgr"))]
    out += [(f"sync_{s}", sync, dict(substreams="auto", segment_bytes=s)) for s in (32, 128, 512)]
    out += [("sync_off", sync, dict(substreams=False)), ("sync_default", sync, {})]
    out += [(f"smallest_{name}", [f], dict(segment_bytes=s)) for name, f, s, _ in L.smallest_plans()]
    out += [("cap", [f for _, f in L.cap_files()], dict(segment_bytes=32, max_rounds=256))]
    out += [(f"prog_levels_{lv}", prog, dict(progressive=True, levels=lv)) for lv in (True, False)]
    out += [("prog_mixed", [prog[0], P._colour_source()], dict(progressive=True)), ("prog_without_keyword", prog[:1], {})]
    return out


def plain(v):
    """A result as JSON holds it: byte strings as hex, tuples told from lists."""
    if isinstance(v, (bytes, bytearray, memoryview)):
        return {"hex": bytes(v).hex()}
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return {"tuple": [plain(x) for x in v]} if isinstance(v, tuple) else [plain(x) for x in v]
    return int(v) if not isinstance(v, (bool, str)) and v is not None else v


def outcome(fn):
    try:
        return {"result": plain(fn())}
    except Exception as e:                                   # the class and the message are what is recorded
        return {"raises": type(e).__name__, "message": str(e)}


def parse_outcomes(jpeg, corpus):
    return {f"{name}|progressive={p}": outcome(lambda: jpeg.parse_jpeg(f, 3, progressive=p)) for name, f in files_of(corpus) for p in (False, True)}


def plan_outcomes(jpeg):
    def one(files, kw):
        parsed, table, header = jpeg.plan(files, **kw)
        return dict(sha256=hashlib.sha256(table.tobytes()).hexdigest(), bytes=int(table.size), segments=[p["segments"] for p in parsed],
                    units=[p["units"] for p in parsed], out_bytes=int(header.out_bytes), scratch_bytes=int(header.scratch_bytes))
    return {label: outcome(lambda: one(files, kw)) for label, files, kw in plans()}


def family_files():
    extra = [("eob_run_textured", Y.eob_run_textured()), ("most_segments", Y.most_segments(0)), ("one_segment_more", Y.most_segments(1))]
    return {c: files_of(c) + (extra if c == "jpegprog_sync" else []) for c in FAMILIES}


def family_parse_outcomes(jpeg, corpus):
    return {f"{name}|{','.join(sorted(kw))}": outcome(lambda: jpeg.parse_jpeg(f, 3, **kw)) for name, f in family_files()[corpus] for kw in KEYWORDS}


def family_plans(jpeg):
    """(label, files, keywords of plan()) of the lists the tests of the three families plan, CPU and GPU: a list holds the
    files of one kind only, as plan() demands."""
    def kind(f, key, **kw):
        try:
            return bool(jpeg.parse_jpeg(f, 0, **kw).get(key))
        except (ValueError, OSError):
            return False
    lay = [f for _, f in F.good() + F.long_plain() + F.malformed() if kind(f, "layout", all_layouts=True)]
    scanned = [f for _, f in N.good() + N.malformed() if kind(f, "scanned", all_scans=True)]
    prog = [f for _, f in P.good() + Y.limits() + Y.larger() + P.malformed()] + [P.eob_run_case()[0]] + [f for _, f in family_files()["jpegprog_sync"][-3:]]
    out = [(f"layouts_{m}", lay, dict(all_layouts=True, mode=m, order="bgr")) for m in ("keep", "RGB", "L")]
    out += [(f"layouts_sub_{s}", lay, dict(all_layouts=True, substreams=True, segment_bytes=s)) for s in (32, 512)]
    out += [(f"scans_levels_{lv}", scanned, dict(all_scans=True, mode="keep", levels=lv)) for lv in (True, False)]
    out += [(f"prog_sub_{w}_{s}", prog, dict(progressive=True, scan_substreams=w, segment_bytes=s)) for w in (True, "auto") for s in (32, 512)]
    return out


def family_plan_outcomes(jpeg):
    def one(files, kw):
        parsed, table, header = jpeg.plan(files, **kw)
        return dict(sha256=hashlib.sha256(table.tobytes()).hexdigest(), bytes=int(table.size), segments=[p["segments"] for p in parsed],
                    units=[p["units"] for p in parsed], scan_segments=[p.get("scan_segments") for p in parsed], out_bytes=int(header.out_bytes),
                    scratch_bytes=int(header.scratch_bytes))
    return {label: outcome(lambda: one(files, kw)) for label, files, kw in family_plans(jpeg)}


def intern(v, pool):
    """Tables that many files share (Pillow's quantisation and Huffman tables) are stored once: {"ref": index in pool}."""
    if isinstance(v, dict) and "hex" not in v:
        v = {k: intern(x, pool) for k, x in v.items()}
    elif isinstance(v, list):
        v = [intern(x, pool) for x in v]
    if isinstance(v, (dict, list)):
        text = json.dumps(v, sort_keys=True)
        if len(text) > INTERN:
            return {"ref": pool.setdefault(text, len(pool))}
    return v


def expand(v, pool):
    if isinstance(v, dict) and "ref" in v:
        return expand(pool[v["ref"]], pool)
    if isinstance(v, dict):
        return {k: expand(x, pool) for k, x in v.items()}
    return [expand(x, pool) for x in v] if isinstance(v, list) else v


def load(name):
    with gzip.open(os.path.join(GOLDEN, name + ".gz"), "rt") as fh:
        doc = json.load(fh)
    pool = [json.loads(t) for t in doc["pool"]]
    return {k: expand(v, pool) for k, v in doc["cases"].items()}


def test_parse_jpeg_equals_the_recording_on_every_file_of_the_four_corpora():
    from attwarp_amd import jpeg
    seen = raised = 0
    for corpus in CORPORA:
        want, got = load(f"jpeg_parse_{corpus}.json"), parse_outcomes(jpeg, corpus)
        assert sorted(got) == sorted(want), corpus
        for key in got:
            assert got[key] == want[key], (corpus, key)
        seen += len(got)
        raised += sum("raises" in v for v in got.values())
    assert seen >= 2 * (66 + 23 + 28 + 115 + 14 + 13) and 2 * (28 + 13) <= raised < seen // 2


def test_plan_tables_equal_the_recording_byte_for_byte():
    from attwarp_amd import jpeg
    want, got = load("jpeg_plan.json"), plan_outcomes(jpeg)
    assert sorted(got) == sorted(want)
    for key in got:
        assert got[key] == want[key], key
    assert sum("raises" in v for v in got.values()) == 2 and "JpegFiles splits" in got["prog_mixed"]["message"]


def test_parse_jpeg_equals_the_recording_on_every_file_of_the_layout_scan_and_sub_stream_corpora():
    from attwarp_amd import jpeg
    for corpus in FAMILIES:
        want, got = load(f"jpeg_parse_{corpus}.json"), family_parse_outcomes(jpeg, corpus)
        assert sorted(got) == sorted(want) and len(got) == len(KEYWORDS) * len(family_files()[corpus]), corpus
        for key in got:
            assert got[key] == want[key], (corpus, key)
        assert any("result" in v for v in got.values()), corpus
    assert sum("raises" in v for v in family_parse_outcomes(jpeg, "jpegfmt").values()) >= len(F.refused())


def test_plan_tables_of_the_layout_scan_and_sub_stream_families_equal_the_recording_byte_for_byte():
    from attwarp_amd import jpeg
    want, got = load("jpeg_plan_families.json"), family_plan_outcomes(jpeg)
    assert sorted(got) == sorted(want) and len(got) == 11
    for key in got:
        assert got[key] == want[key], key
    assert all("result" in v for v in got.values())             # every list plans: the tables are what is compared


if __name__ == "__main__":                                    # the recorder: run on a checkout of the code to record
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from attwarp_amd import jpeg
    assert os.path.abspath(jpeg.__file__).startswith(os.path.abspath(sys.argv[1]))
    what = sys.argv[2] if len(sys.argv) > 2 else "four"        # "families": the fixtures of the three later families alone
    todo = ([(f"jpeg_parse_{c}.json", family_parse_outcomes(jpeg, c)) for c in FAMILIES] + [("jpeg_plan_families.json", family_plan_outcomes(jpeg))]
            if what == "families" else [(f"jpeg_parse_{c}.json", parse_outcomes(jpeg, c)) for c in CORPORA] + [("jpeg_plan.json", plan_outcomes(jpeg))])
    for name, cases in todo:
        pool = {}
        cases = {k: intern(v, pool) for k, v in cases.items()}
        text = json.dumps({"pool": list(pool), "cases": cases}, separators=(",", ":"), sort_keys=True)
        with open(os.path.join(GOLDEN, name + ".gz"), "wb") as fh, gzip.GzipFile("", "wb", 9, fh, mtime=0) as z:
            z.write(text.encode())
        print(name, len(text), "bytes of JSON,", len(cases), "cases")
