"""Images that put the PNG encoder (attwarp_amd/csrc/png.hip) at its code, run, segment, carry and tie
limits (test_png_limits_ref_cpu.py proves every case from the restatement of tests/png_ref.py, test_png_limits_gpu.py runs
them through the kernels).  A case is (name, image [H,W,C] uint8, filter, order, expect); `expect` names the limit the image
is built to hit and test_png_limits_ref_cpu.py asserts every entry of it, so a builder that stops reaching its limit fails
there.  Token histograms are made to order: under filter "none" a grey row's filtered bytes are a zero and the pixels, a
byte between two different neighbours is one literal, and a run of n + 1 equal bytes is one literal and one match of n.
Everything is deterministic, numpy only and cached."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import png_cases as K
import png_ref as R

SEG = R.SEG_BYTES
SPLIT_RUNS = [259, 260, 261, 262, 516, 517, 775]           # runs of more than one match: 258s and a remainder of 0, 1, 2, 3, 257
TAIL_SHAPES = ((1, "rgb", list(range(12, 25)) + [36]),     # W C = 12 .. 24, 36: every W C % 12 and one, two, three whole groups
               (3, "rgb", list(range(1, 9)) + [12]),       # W C = 3 .. 24, 36: the four residues three channels reach
               (3, "bgr", list(range(1, 9)) + [12]))
GUARD_TAILS = 20


class Case(NamedTuple):
    name: str
    image: np.ndarray
    filter: str
    order: str
    expect: dict


def _rng(seed):
    return np.random.default_rng(8800 + seed)


def fib(n):
    """F1 .. Fn = 1, 1, 2, 3, ..."""
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


# ---- what the restatement makes of a histogram / a segment ------------------------------------------------------------------
def halvings(hist, limit=15):
    """The frequencies at every round of R.code_lengths: [hist, halved once, ...]; the last one's tree fits `limit`."""
    freq = list(hist)
    out = [freq]
    while max(R.huffman_depths(freq)) > limit:
        freq = [(f + 1) >> 1 if f else 0 for f in freq]
        out.append(freq)
        assert len(out) <= 17
    return out


def limiter_rounds(hist, limit=15):
    """How often R.code_lengths halves the frequencies of `hist` before the tree is at most `limit` deep."""
    return len(halvings(hist, limit)) - 1


def segment_facts(image, filt, order):
    """Per segment of the image, from the restatement: filtered bytes n, token histogram, match lengths, unlimited depth,
    limiter rounds, code lengths, dyn_bytes (the size decision's left side, restated from R.encode_segment), whether the
    block is stored, its deflate length and the rows' filter types."""
    fs = R.filtered_stream(image, filt, order)
    out = []
    for r0, nr in R.segments(*fs.shape):
        d = fs[r0:r0 + nr].tobytes()
        toks = R.tokens(d)
        hist = R.histogram(toks)
        lens = R.code_lengths(hist)
        extra = sum(hist[257 + k] * (R.LEN_EXTRA[k] + 1) for k in range(29))
        dyn_bits = R.HEADER_BITS + sum(h * l for h, l in zip(hist, lens)) + extra
        enc = R.encode_segment(d)
        out.append(dict(n=len(d), hist=hist, lens=lens, depth=max(R.huffman_depths(hist)), rounds=limiter_rounds(hist),
                        dyn_bytes=(dyn_bits + 3 + 7) // 8 + 4, stored=enc[0] == 0, out_len=len(enc), ntokens=len(toks),
                        match_lengths=sorted({v for k, v in toks if k == "len"}), run_lengths=sorted({n for _, n in R.runs(d)}),
                        ftypes=fs[r0:r0 + nr, 0].tolist()))
    return out


# ---- rows with a chosen token histogram ----------------------------------------------------------------------------------------
def isolated(counts):
    """{value: count} -> uint8 array with every value `count` times and no two equal neighbours: the most frequent value
    first, dealt to the even places, then to the odd ones."""
    items = sorted(((v, n) for v, n in counts.items() if n), key=lambda vn: (-vn[1], vn[0]))
    vals = np.concatenate([np.full(n, v, np.uint8) for v, n in items])
    n = vals.size
    arr = np.empty(n, np.uint8)
    arr[0::2] = vals[:(n + 1) // 2]
    arr[1::2] = vals[(n + 1) // 2:]
    assert (arr[1:] != arr[:-1]).all()
    return arr


def expand(arr, runs):
    """{value: [n, ...]}: the first occurrences of `value` become runs of n equal bytes (its neighbours differ from it)."""
    rep = np.ones(arr.size, np.int64)
    for v, lengths in runs.items():
        idx = np.flatnonzero(arr == v)[:len(lengths)]
        assert idx.size == len(lengths)
        rep[idx] = lengths
    return np.repeat(arr, rep)


def grey_row(literals, runs=None):
    """One grey row [1, W, 1] for filter "none" whose segment has exactly `literals` {value: literal tokens} (the filter-type
    byte is one of the zeros) and one match of n - 1 per run of `runs`."""
    counts = dict(literals)
    counts[0] -= 1
    px = expand(isolated(counts), runs or {})
    assert px[0] != 0 and px.size + 1 <= R.MAX_ROW_BYTES
    return px.reshape(1, -1, 1)


def scaled_fibonacci(mult, lo, hi):
    """Literal v has mult * F(lo + v) tokens, up to F(hi); the end of block's 1 comes on top."""
    return {v: mult * f for v, f in enumerate(fib(hi)[lo - 1:])}


def code15_image():
    """F1 .. F16 exactly: end of block 1, length symbol 284 once (a run of 229 bytes of the most frequent value), literal v
    F(v+3) times for v = 0 .. 13."""
    f = fib(16)
    return grey_row({v: f[v + 2] for v in range(14)}, {13: [229]})


def deepest_image():
    """F1 .. F20 (sum 17,710, the last Fibonacci histogram a segment holds): end of block 1, literal v F(v+2) times."""
    f = fib(20)
    return grey_row({v: f[v + 1] for v in range(19)})


def every_match_length_image():
    """Grey rows of 6144 filtered bytes (four to a segment): runs of 4 .. 259 bytes, one per match length 3 .. 258, then
    SPLIT_RUNS, neighbours different, each row filled up with alternating bytes."""
    W = 6143
    rows, cur, used = [], [], 0

    def flush():
        nonlocal cur, used
        pad = np.where(np.arange(W - used) % 2 == 0, 250, 251).astype(np.uint8)
        rows.append(np.concatenate(cur + [pad]))
        cur, used = [], 0

    for k, n in enumerate([L + 1 for L in range(3, 259)] + SPLIT_RUNS):
        if used + n > W:
            flush()
        cur.append(np.full(n, 1 + k % 200, np.uint8))
        used += n
    flush()
    return np.stack(rows)[:, :, None]


def all_symbols_image():
    """One grey row: every byte value as a literal, and a run of LEN_BASE[k] + 1 bytes for each of the 29 length symbols."""
    px = np.concatenate([np.arange(1, 256), [0]]).astype(np.uint8)
    return expand(px, {10 + k: [R.LEN_BASE[k] + 1] for k in range(29)}).reshape(1, -1, 1)


def many_segments_image():
    """600 grey rows of 12,289 filtered bytes, one segment each: a ramp ("sub" leaves one long run: about 160 bytes), every
    37th row noise (a stored block of 12,294 bytes)."""
    img = K.ramp(600, 12288, 1).copy()
    rows = np.arange(0, 600, 37)
    img[rows] = _rng(1).integers(0, 256, (rows.size, 12288, 1), dtype=np.uint8)
    return img


def many_rows_image():
    """2049 x 1 grey for "adaptive": stretches of small values (none), of a slow walk (up), of a walk around twice the row
    above's half (average) and of noise."""
    rng = _rng(2)
    H = 2049
    walk = np.cumsum(rng.integers(-2, 3, H)) + 120
    small = rng.integers(0, 4, H)
    kind = (np.arange(H) // 61) % 4
    v = np.where(kind == 0, small, np.where(kind == 1, walk, np.where(kind == 2, walk // 2 + (np.arange(H) % 2) * 60, rng.integers(0, 256, H))))
    return (v & 255).astype(np.uint8).reshape(H, 1, 1)


# Rows between rows of zeros filter as a first row does (none = up, sub = paeth).  Found by enumeration over the values
# 0, 1, 2, 63 .. 65, 127 .. 129, 191 .. 193, 255.  Costs (none, sub, average):
#   255   1 128: 130 = 130 < 255, the 128 is the winner's (none);    1 129 192: 192 = 192 < 256, the 128 is the loser's (sub);
#     2   1 128: 131 > 130 = 130, sub ties with average's 2 0 128;  128 127   0: 255, 256, 254: average wins by one, 128 in all.
# Counting a 128 as 127 turns the second and third choice, as 129 the first.
ADAPTIVE_128_ROWS = [[255, 1, 128], [1, 129, 192], [2, 1, 128], [128, 127, 0]]
ADAPTIVE_128_TYPES = [0, 0, 1, 3]
LIMITER_2 = (2, 2, 17)                                      # 2 F2 .. 2 F17 and the end of block: 8,359 tokens, 16 deep
LIMITER_3 = (4, 2, 17)                                      # 4 F2 .. 4 F17 and the end of block: 16,717 tokens, 16 deep
DEEPEST_ROUNDS = 1


def adaptive_128_image():
    z = [0] * len(ADAPTIVE_128_ROWS[0])
    rows = []
    for r in ADAPTIVE_128_ROWS:
        rows += [z, r]
    return np.array(rows + [z], np.uint8)[:, :, None]


def tail_image(W, C, seed):
    return (K.ramp(5, W, C) + (_rng(100 + seed).integers(0, 256, (5, W, C), dtype=np.uint8) >> 5)).astype(np.uint8)


def tails():
    out, i = [], 0
    for C, order, widths in TAIL_SHAPES:
        for filt in R.FILTERS:
            for W in widths:
                out.append(Case(f"tail_c{C}{order}_{filt}_w{W}", tail_image(W, C, i), filt, order,
                                dict(tail=(W * C) % 12, groups=(W * C) // 12, odd_placement=i % 2 == 0)))
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[Case(name, image, filter, order, expect)]"""
    z = np.zeros
    c = [Case("code15_exact", code15_image(), "none", "rgb", dict(nseg=1, depth=15, rounds=0, stored=[False], len15=[256, 284])),
         Case("limiter_2_rounds", grey_row(scaled_fibonacci(*LIMITER_2)), "none", "rgb",
              dict(nseg=1, depth=16, rounds=2, stored=[False], equal_after_halving=3)),
         Case("limiter_3_rounds", grey_row(scaled_fibonacci(*LIMITER_3)), "none", "rgb",
              dict(nseg=1, depth=16, rounds=3, stored=[False], equal_after_halving=3)),
         Case("limiter_deepest", deepest_image(), "none", "rgb", dict(nseg=1, depth=19, rounds=DEEPEST_ROUNDS, stored=[False])),
         Case("single_run_segment", z((2, SEG - 1, 1), np.uint8), "none", "rgb",
              dict(nseg=2, stored=[False, False], run_lengths=[SEG], ntokens=1 + 95 + 1, match_lengths=[65, 258])),
         Case("every_match_length", every_match_length_image(), "none", "rgb",
              dict(nseg=2, stored=[False, False], all_match_lengths=True, split_runs=SPLIT_RUNS)),
         Case("all_286_symbols", all_symbols_image(), "none", "rgb", dict(nseg=1, stored=[False], used_symbols=286)),
         Case("tie_dynamic", z((1, 153, 1), np.uint8), "none", "rgb", dict(nseg=1, dyn_minus_n=5, stored=[False])),
         Case("tie_stored_by_one", z((1, 152, 1), np.uint8), "none", "rgb", dict(nseg=1, dyn_minus_n=6, stored=[True])),
         Case("full_segment_stored", K.noise(2, SEG - 1, 1, 21), "none", "rgb", dict(nseg=2, stored=[True, True], out_len=SEG + 5)),
         Case("full_segment_dynamic", _rng(3).integers(0, 128, (1, SEG - 1, 1), dtype=np.uint8), "none", "rgb",
              dict(nseg=1, stored=[False], min_out_len=20001)),
         Case("rgb_full_row", np.concatenate([K.noise(1, 8191, 3, 22), K.ramp(2, 8191, 3)[1:]]), "paeth", "bgr", dict(nseg=2, stored=[True, False])),
         Case("many_segments", many_segments_image(), "sub", "rgb", dict(nseg=600, stored_count=17, stored_out_len=12294, max_dynamic_out_len=200)),
         Case("many_rows_adaptive", many_rows_image(), "adaptive", "rgb", dict(nseg=3, seg_rows=[1024, 1024, 1], ftypes_used=[0, 2, 3])),
         Case("adaptive_constant", np.full((9, 40, 3), 77, np.uint8), "adaptive", "rgb", dict(nseg=1, ftypes=[1] + [2] * 8)),
         Case("adaptive_128", adaptive_128_image(), "adaptive", "rgb", dict(nseg=1, ftypes=[t for k in ADAPTIVE_128_TYPES for t in (0, k)] + [0], ties_through_128=True))]
    return c + tails()


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's file for a case, computed once per process."""
    c = case(name)
    return R.encode(c.image, c.filter, c.order)


@functools.lru_cache(maxsize=None)
def facts(name):
    c = case(name)
    return segment_facts(c.image, c.filter, c.order)


def guard_batch():
    """The sub-batch of the guard-byte and alignment test: many_segments stands between small images."""
    t = [c.name for c in cases() if c.name.startswith("tail_")]
    picked = [t[(37 * i) % len(t)] for i in range(GUARD_TAILS)]               # (37 and the 192 tails are coprime)
    assert len(set(picked)) == GUARD_TAILS
    return ["tie_dynamic", "tie_stored_by_one", "code15_exact"] + picked[:10] + ["many_segments", "full_segment_stored"] + picked[10:]


def segment_addresses(names):
    """offset + 43 + pre of every segment of a batch of cases, from the restatement's lengths alone (the buffer's own
    address comes on top)."""
    out, off = [], 0
    for n in names:
        pre = 0
        for f in facts(n):
            out.append(off + 43 + pre)
            pre += f["out_len"]
        assert R.FILE_OVERHEAD + pre == len(reference(n))
        off += R.FILE_OVERHEAD + pre
    return out
