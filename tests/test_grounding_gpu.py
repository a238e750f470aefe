"""GPU tests of the layer-selection study (attwarp_amd.grounding): the LANCZOS4 resize, the dense and fused box metrics and
the raw head-mean probe bit for bit against tests/grounding_ref.py, the metrics against the reference's own outputs
(tests/golden/grounding_metrics.npz), LayerSweepProbe against the study's eager expression on random-weight Llama / LLaVA
models, and layer_sweep end to end."""
import os

import numpy as np
import pytest
import torch

import grounding_ref as R

pytestmark = pytest.mark.gpu

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from attwarp_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "HIP library missing -- the product has no fallback"
    _lib.load()
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def grids_of(rng, M, g=24):
    a = rng.random((M, g, g), dtype=np.float32) ** 4
    return (a / a.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_resize_bit_exact(dev):
    from attwarp_amd import grounding as G
    rng = np.random.default_rng(1)
    sizes = TEXTVQA_LIKE_WH + [(18, 27), (24, 24), (1, 1), (7, 333), (24, 1), (1, 24), (25, 23), (97, 24), (2, 3000)]
    g = grids_of(rng, len(sizes))
    g[3] -= np.float32(0.002)                                        # negative values
    views = G.resize_lanczos4(T(g, dev), sizes)
    for i, (W, H) in enumerate(sizes):
        got = N(views[i])
        assert got.shape == (H, W)
        want = R.resize_lanczos4(g[i], W, H)
        assert np.array_equal(bits(got), bits(want)), (W, H, int((bits(got) != bits(want)).sum()))
    assert np.array_equal(N(views[sizes.index((24, 24))]), g[sizes.index((24, 24))])   # dsize == ssize: a copy
    # one size for all: a dense batch; non-square grids
    dense = G.resize_lanczos4(T(g[:4], dev), (18, 27))
    assert tuple(dense.shape) == (4, 27, 18)
    for i in range(4):
        assert np.array_equal(bits(N(dense[i])), bits(R.resize_lanczos4(g[i], 18, 27)))
    ns = rng.random((3, 13, 31), dtype=np.float32)
    out = G.resize_lanczos4(T(ns, dev), (100, 41))
    for i in range(3):
        assert np.array_equal(bits(N(out[i])), bits(R.resize_lanczos4(ns[i], 100, 41)))
    with pytest.raises(ValueError):
        G.resize_lanczos4(T(np.zeros((2, 65, 24), np.float32), dev), (10, 10))
    with pytest.raises(ValueError):
        G.resize_lanczos4(T(g[:2], dev), [(10, 10)] * 3)
    with pytest.raises(ValueError):
        G.resize_lanczos4(T(g[:2], dev), (0, 10))


def test_dense_metrics_against_reference_fixture(dev, golden):
    from attwarp_amd import grounding as G
    d = golden("grounding_metrics")
    maps = d["maps"]
    nm, nb = len(maps), len(d["raw_boxes"])
    tm = T(maps, dev)
    mlist = [tm[i] for i in range(nm) for _ in range(nb * 2)]
    boxes = [tuple(int(v) for v in d["boxes"][j, k]) for _ in range(nm) for j in range(nb) for k in range(2)]
    res = G.box_metrics(mlist, boxes)
    arg, top1, am = N(res.argmax).reshape(nm, nb, 2), N(res.top1).reshape(nm, nb, 2), N(res.am).reshape(nm, nb, 2)
    assert np.array_equal(top1, d["top1"])
    assert np.array_equal(arg, np.broadcast_to(d["argmax"][:, None, None], arg.shape))
    np.testing.assert_allclose(am, d["am"], rtol=1e-5, atol=1e-12)
    want = np.array([[[R.box_metrics(maps[i], d["boxes"][j, k])[2] for k in range(2)] for j in range(nb)] for i in range(nm)])
    np.testing.assert_allclose(am, want, rtol=1e-9, atol=1e-15)
    # the name-for-name functions
    assert G.top1(tm[1], tuple(d["boxes"][11, 0])) == int(d["top1"][1, 11, 0])
    assert abs(G.am_all(tm[0], tuple(d["boxes"][0, 0])) - float(d["am"][0, 0, 0])) <= 1e-5 * abs(float(d["am"][0, 0, 0]))


def test_dense_metrics_ties_signed_zero_and_nan_order(dev):
    from attwarp_amd import grounding as G
    H, W = 300, 700                                                 # several tiles and bands
    m = np.zeros((5, H, W), np.float32)
    m[0, 250, 600] = m[0, 10, 650] = m[0, 10, 651] = 2.0          # ties: the first in row-major order wins
    m[1] = -1.0
    m[1, 5, 5] = -0.0
    m[1, 3, 600] = 0.0                                              # -0.0 == 0.0: the earlier index
    m[2, 280, 1] = np.nan
    m[2, 290, 0] = np.nan
    m[2, 0, 0] = np.inf
    m[3] = -np.inf
    m[4] = np.float32(1 / 576)
    box = (600, 0, 60, 260)
    res = G.box_metrics(T(m, dev), [box] * 5)
    for i in range(5):
        want = R.box_metrics(m[i], box)
        assert int(res.argmax[i]) == want[0] and int(res.top1[i]) == want[1], i
        got_am = float(res.am[i])
        assert (np.isnan(got_am) and np.isnan(want[2])) or abs(got_am - want[2]) <= 1e-9 * abs(want[2]), (i, got_am, want[2])


def test_fused_equals_materialised_bits(dev):
    from attwarp_amd import grounding as G
    rng = np.random.default_rng(5)
    B, nL = 32, 9
    sizes = [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(B)]
    M = 2 * nL * B
    g = grids_of(rng, M)
    g[:B] = np.float32(1 / 576)                                     # constant grids: ties everywhere
    g[B:B + 4, 3, 7] = np.nan                                       # NaN grids
    gen = grids_of(rng, M)
    g[-B:] = g[-B:] / (gen[-B:] * np.float32(1e-3) + np.float32(1e-8))   # relative maps with large values
    msizes = sizes * (2 * nL)
    boxes = []
    for b in range(M):
        W, H = msizes[b]
        x0, y0 = (int(v) for v in rng.integers(-50, max(W, H), 2))
        boxes.append((x0, y0, int(rng.integers(0, W)), int(rng.integers(0, H))))
    tg = T(g, dev)
    fused = G.grid_box_metrics(tg, msizes, boxes)
    full = G.resize_lanczos4(tg, msizes)
    dense = G.box_metrics(full, boxes)
    assert torch.equal(fused.argmax, dense.argmax) and torch.equal(fused.top1, dense.top1)
    assert np.array_equal(N(fused.am).view(np.uint64), N(dense.am).view(np.uint64))
    again = G.grid_box_metrics(tg, msizes, boxes)                   # run to run: the same bits
    assert np.array_equal(N(again.am).view(np.uint64), N(fused.am).view(np.uint64))
    for i in (0, B, B + 1, M - 1, M // 2 + 3):                      # spot checks against the restatement
        W, H = msizes[i]
        want = R.box_metrics(R.resize_lanczos4(g[i], W, H), boxes[i])
        assert int(fused.argmax[i]) == want[0] and int(fused.top1[i]) == want[1]
        a = float(fused.am[i])
        assert (np.isnan(a) and np.isnan(want[2])) or abs(a - want[2]) <= 1e-9 * abs(want[2]) + 1e-300


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_head_mean_probe_bit_exact(dev, dt):
    from attwarp_amd import attention_extraction as ae
    rng = np.random.default_rng(11)
    B, H, Hkv, kv, D, ntok = 3, 8, 2, 700, 128, 576
    q32 = rng.standard_normal((B, H, D)).astype(np.float32)
    k32 = rng.standard_normal((B, Hkv, kv, D)).astype(np.float32)
    k32[0, :, 40:80] *= 3                                           # a peaked region
    q, k = T(q32, dev).to(dt), T(k32, dev).to(dt)
    starts = [35, 60, 80]
    pads = [0, 9, 20]
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    kb = torch.tensor(pads, dtype=torch.int32, device=dev)
    sc = D ** -0.5
    bf = dt == torch.bfloat16
    qn, kn = N(q.float() if bf else q), N(k.float() if bf else k)
    for kbeg in (None, kb):
        got = ae.probe_head_mean(q, k, st, ntok, kbeg, sc)
        assert got.dtype == dt and tuple(got.shape) == (B, ntok)
        want = R.head_mean_rows(qn, kn, starts, ntok, sc, None if kbeg is None else pads, bf16=bf)
        g = N(got.float())
        assert np.array_equal(g, want.astype(np.float32)), int((g != want).sum())
    # strided inputs: a query with q > 1 (the last one is probed) and a key view inside a larger cache
    qq = torch.zeros(B, H, 3, D, device=dev, dtype=dt)
    qq[:, :, -1] = q
    big = torch.zeros(B, Hkv, kv + 64, D, device=dev, dtype=dt)
    big[:, :, 16:16 + kv] = k
    got = ae.probe_head_mean(qq, big[:, :, 16:16 + kv], st, ntok, kb, sc)
    assert torch.equal(got, ae.probe_head_mean(q, k, st, ntok, kb, sc))
    # not renormalised: differs from the hook's per-head renormalised mean
    assert not torch.equal(got, ae.probe_last_query(q, k, st, ntok, kb, sc))


def _eager_rows(model, ids, am, layers, span, pos=None):
    """The study's expression on eager attention: attentions[L][b, :, -1, span].mean(0)."""
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=am, position_ids=pos, output_attentions=True)
    return torch.stack([torch.stack([out.attentions[L][b, :, -1, span[b]:span[b] + 576].mean(0) for b in range(ids.shape[0])])
                        for L in layers])


def test_sweep_probe_against_eager_llama(dev):
    transformers = pytest.importorskip("transformers")
    from attwarp_amd import grounding as G
    cfg = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=4,
                                   num_key_value_heads=2, vocab_size=1000, head_dim=128, max_position_embeddings=2048)
    torch.manual_seed(3)
    model = transformers.LlamaForCausalLM(cfg).to(dev).half().eval()
    layers = [0, 1, 2]
    B, L = 3, 640
    pads = [0, 5, 11]
    ids = torch.randint(0, 1000, (B, L), device=dev)
    am = torch.ones(B, L, dtype=torch.long, device=dev)
    for b, p_ in enumerate(pads):
        am[b, :p_] = 0
    pos = (am.cumsum(-1) - 1).clamp_min(0)
    starts = [30 + p_ for p_ in pads]
    model.config._attn_implementation = "sdpa"
    with G.LayerSweepProbe(model, layers) as probe:
        probe.set_image_token_starts(starts)
        with torch.no_grad():
            model(input_ids=ids, attention_mask=am, position_ids=pos)
        got = probe.rows()
    assert got.shape == (3, B, 576) and got.dtype == torch.float16
    model.config._attn_implementation = "eager"
    tol = {0: 1e-2, 1: 5e-2, 2: 1e-1}                   # (batch 1 vs 3: the projections may round differently)
    for b, p_ in enumerate(pads):                       # each padded sample against its own unpadded batch-1 eager run
        want = _eager_rows(model, ids[b:b + 1, p_:], None, layers, [30])
        for li in range(3):
            np.testing.assert_allclose(N(got[li, b].float()), N(want[li, 0].float()), rtol=tol[li], atol=2e-6)
    # the unpadded batch against the batched eager expression: the same positions
    model.config._attn_implementation = "sdpa"
    with G.LayerSweepProbe(model, [0]) as probe:
        probe.set_image_token_starts([30] * B)
        with torch.no_grad():
            model(input_ids=ids)
        r0 = probe.rows()
    model.config._attn_implementation = "eager"
    want = _eager_rows(model, ids, None, [0], [30] * B)
    np.testing.assert_allclose(N(r0.float()), N(want.float()), rtol=4e-3, atol=2e-6)


def test_sweep_probe_against_eager_llava(dev):
    transformers = pytest.importorskip("transformers")
    from attwarp_amd import grounding as G
    text = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                                    num_key_value_heads=2, head_dim=128, vocab_size=600, max_position_embeddings=2048)
    vision = transformers.CLIPVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=2,
                                           image_size=336, patch_size=14)
    cfg = transformers.LlavaConfig(vision_config=vision, text_config=text, image_token_index=599, projector_hidden_act="gelu",
                                   vision_feature_layer=-2, vision_feature_select_strategy="default")
    torch.manual_seed(4)
    model = transformers.LlavaForConditionalGeneration(cfg).to(dev).half().eval()
    pre, post = torch.randint(0, 500, (1, 7)), torch.randint(0, 500, (1, 40))
    ids = torch.cat([pre, torch.full((1, 576), 599), post], dim=1).to(dev)
    pix = torch.randn(1, 3, 336, 336, device=dev).half()
    pos = ids[0].tolist().index(599)                    # the study's span (uncertainty_attn_maps_llava.py:47-49)
    layers = [0, 2]
    text_cfg = model.get_decoder().config                # the language model's config (the vision tower keeps its own)
    text_cfg._attn_implementation = "sdpa"
    with G.LayerSweepProbe(model, layers) as probe:
        probe.set_image_token_starts([pos])
        with torch.no_grad():
            model(input_ids=ids, pixel_values=pix)
        got = probe.rows()
    text_cfg._attn_implementation = "eager"
    with torch.no_grad():
        out = model(input_ids=ids, pixel_values=pix, output_attentions=True)
    for i, L in enumerate(layers):
        want = out.attentions[L][0, :, -1, pos:pos + 576].mean(0)
        np.testing.assert_allclose(N(got[i, 0].float()), N(want.float()), rtol=4e-3 if L == 0 else 5e-2, atol=2e-6)


def test_layer_sweep_end_to_end(dev):
    from attwarp_amd import grounding as G
    rng = np.random.default_rng(9)
    nL, B = 3, 7
    sizes = [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(B)]
    a = torch.from_numpy(grids_of(rng, nL * B).reshape(nL, B, 576)).to(dev).bfloat16()
    gen = torch.from_numpy(grids_of(rng, nL * B).reshape(nL, B, 576)).to(dev).bfloat16()
    boxes = [G.select_box([int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2)), int(rng.integers(1, W // 2)),
                           int(rng.integers(1, H // 2))]) for (W, H) in sizes]
    res = G.layer_sweep(a, gen, sizes, boxes, return_maps=True, layers=[3, 7, 19])
    an, gn = N(a.float()), N(gen.float())
    top1, am, arg, small = R.layer_sweep(an, gn, sizes, boxes)
    assert np.array_equal(N(res.top1), top1) and np.array_equal(N(res.argmax), arg)
    np.testing.assert_allclose(N(res.am), am, rtol=1e-9, atol=1e-15)
    assert np.array_equal(bits(N(res.small)), bits(small))
    rel = N(a.float() / (gen.float() + 1e-8))
    assert np.array_equal(bits(rel), bits(an / (gn + 1e-8)))         # numpy's float32 expression, bit for bit
    W, H = sizes[2]
    assert np.array_equal(bits(N(res.maps[1][1][2])), bits(R.resize_lanczos4(rel[1, 2].reshape(24, 24), W, H)))
    rows = res.summary()
    assert [(r[0], r[1]) for r in rows[:2]] == [(3, "absolute"), (3, "relative")] and len(rows) == 2 * nL
    assert abs(rows[1][2] - top1[0, 1].mean()) < 1e-12 and abs(rows[1][3] - am[0, 1].mean()) < 1e-9
    with pytest.raises(ValueError):
        G.layer_sweep(a, gen[:, :3], sizes, boxes)
    with pytest.raises(ValueError):
        G.layer_sweep(a, gen, sizes, boxes[:-1] + [None])
