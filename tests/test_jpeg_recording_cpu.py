"""``jpeg.parse_jpeg`` and ``jpeg.plan`` against a recording (tests/golden/jpeg_parse_*.json.gz, jpeg_plan.json.gz) made with the
parser as it stood BEFORE its baseline and progressive tails became one walk: every file of the four JPEG corpora, good,
malformed and refused, with ``progressive`` False and True, gives the same dict or raises the same class with the same
message; the planned tables of the lists the other tests plan have the same SHA-256.  No tolerance anywhere.

The recording is made by running this file on a checkout of the older code, never with the code under test:
``python tests/test_jpeg_recording_cpu.py <root of that checkout>`` writes the fixtures (gzipped JSON: class and message per
case, dicts with byte strings as hex) into golden/."""
import gzip
import hashlib
import json
import os
import sys

import jpegdec_cases as A
import jpegdec_limit_cases as L
import jpegdec_sync_cases as S
import jpegprog_cases as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORPORA = {"jpegdec": (A, "good malformed refused"), "jpegdec_sync": (S, "good all_one_unit_good"),
           "jpegdec_limit": (L, "narrow extreme long_files long_cuts restart_files restart_damaged data_ends behind_end "
                                "smallest_plans cap_files"),
           "jpegprog": (P, "good malformed refused")}
INTERN = 24                                                  # characters of JSON above which a value is stored once


def files_of(corpus):
    mod, makers = CORPORA[corpus]
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


if __name__ == "__main__":                                    # the recorder: run on a checkout of the code to record
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from attwarp_amd import jpeg
    assert os.path.abspath(jpeg.__file__).startswith(os.path.abspath(sys.argv[1]))
    for name, cases in [(f"jpeg_parse_{c}.json", parse_outcomes(jpeg, c)) for c in CORPORA] + [("jpeg_plan.json", plan_outcomes(jpeg))]:
        pool = {}
        cases = {k: intern(v, pool) for k, v in cases.items()}
        text = json.dumps({"pool": list(pool), "cases": cases}, separators=(",", ":"), sort_keys=True)
        with open(os.path.join(GOLDEN, name + ".gz"), "wb") as fh, gzip.GzipFile("", "wb", 9, fh, mtime=0) as z:
            z.write(text.encode())
        print(name, len(text), "bytes of JSON,", len(cases), "cases")
