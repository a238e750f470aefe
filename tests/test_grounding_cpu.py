"""CPU tests of the layer-selection study's pieces (attwarp_amd.grounding): the numpy restatement against the reference's own
metrics (tests/golden/grounding_metrics.npz), the library's host LANCZOS4 tables against the restatement, numpy's slice
rules, argument validation of the new entry points, and LayerSweepProbe's plumbing on CPU models built from configs."""
import ctypes

import numpy as np
import pytest
import torch

import grounding_ref as R


@pytest.fixture(scope="module")
def lib():
    from attwarp_amd import _lib
    return _lib.load()


def test_restatement_matches_reference_metrics(golden):
    from attwarp_amd import grounding as G
    d = golden("grounding_metrics")
    assert list(d["methods"]) == G.BBOX_METHODS
    for j, raw in enumerate(d["raw_boxes"]):
        for k, meth in enumerate(G.BBOX_METHODS):
            assert G.interpret_bbox(list(raw), meth) == tuple(int(v) for v in d["boxes"][j, k])
        want = next((tuple(int(v) for v in d["boxes"][j, k]) for k in range(2) if d["boxes"][j, k, 2] > 0 and d["boxes"][j, k, 3] > 0),
                    None)
        assert G.select_box(list(raw)) == want
    for i, m in enumerate(d["maps"]):
        for j in range(len(d["raw_boxes"])):
            for k in range(2):
                arg, t, am = R.box_metrics(m, d["boxes"][j, k])
                assert arg == d["argmax"][i]
                assert t == d["top1"][i, j, k], (d["names"][i], j, k)
                np.testing.assert_allclose(am, d["am"][i, j, k], rtol=1e-5, atol=1e-12)


def test_select_box_none_and_xyxy_fallback():
    from attwarp_amd import grounding as G
    assert G.select_box([5, 5, 0, 3]) is None                      # xywh zero width, xyxy negative height
    assert G.select_box([30.0, 4.0, 45.0, 12.0]) == (30, 4, 45, 12)
    assert G.select_box([10, 10, -2, 20]) is None                  # negative width either way
    assert G.select_box([10.9, 2.2, 30.5, 8.1]) == (10, 2, 30, 8)


@pytest.mark.parametrize("n_out", [1, 18, 24, 27, 333, 683, 1024, 4096])
def test_lanczos4_coeffs_bit_exact(lib, n_out):
    from attwarp_amd import _tables
    ofs, co = _tables.lanczos4_tables_host(24, n_out)
    rofs, rco = R.lanczos4_coeffs(24, n_out)
    assert np.array_equal(ofs, rofs)
    assert np.array_equal(co.view(np.uint32), rco.view(np.uint32))
    assert np.all(np.abs(co.sum(axis=1, dtype=np.float64) - 1.0) < 1e-5)


@pytest.mark.parametrize("n_out", [1, 2, 7, 500])
def test_lanczos4_coeffs_from_one_pixel(lib, n_out):
    from attwarp_amd import _tables
    ofs, co = _tables.lanczos4_tables_host(1, n_out)
    rofs, rco = R.lanczos4_coeffs(1, n_out)
    assert np.array_equal(ofs, rofs) and np.array_equal(co.view(np.uint32), rco.view(np.uint32))


LIMIT_N_OUT = [1, 2, 3, 5, 17, 18, 27, 63, 64, 65, 255, 256, 257, 500, 1000]


@pytest.mark.parametrize("n_in", range(1, 65))
def test_lanczos4_coeffs_bit_exact_for_every_grid_side(lib, n_in):
    """Every grid side the kernels take (1 .. 64) against output sides around the grid's own, a 256-pixel tile and beyond,
    down-sampling included; the longest tables (4096 and the limit, 32768) for the largest grid."""
    from attwarp_amd import _tables
    for n_out in LIMIT_N_OUT + ([4096, 32768] if n_in == 64 else []):
        ofs, co = _tables.lanczos4_tables_host(n_in, n_out)
        rofs, rco = R.lanczos4_coeffs(n_in, n_out)
        assert ofs.dtype == np.int32 and co.dtype == np.float32 and co.shape == (n_out, 8)
        assert np.array_equal(ofs, rofs), (n_in, n_out)
        assert np.array_equal(co.view(np.uint32), rco.view(np.uint32)), (n_in, n_out)
        assert np.isfinite(co).all() and -1 <= int(ofs.min()) and int(ofs.max()) <= n_in - 1, (n_in, n_out)


def test_box_slice_follows_numpy_slicing():
    from attwarp_amd import grounding as G
    rng = np.random.default_rng(7)
    for _ in range(3000):
        H, W = (int(v) for v in rng.integers(1, 40, 2))
        box = tuple(int(v) for v in rng.integers(-60, 60, 4))
        a = np.arange(H * W).reshape(H, W)
        x0, y0, w, h = box
        want = a[y0:y0 + h, x0:x0 + w]
        for r0, r1, c0, c1 in (G.box_slice(box, H, W), R.box_slice(box, H, W)):
            assert 0 <= r0 <= r1 <= H and 0 <= c0 <= c1 <= W
            assert np.array_equal(a[r0:r1, c0:c1], want) and (r1 - r0) * (c1 - c0) == want.size


def _rec(n, **kw):
    from attwarp_amd import grounding as G
    rec = np.zeros(n, dtype=G._GRID_MAP_DTYPE)
    rec["src"], rec["out"] = 4096, 8192
    rec["ofs_x"] = rec["coef_x"] = rec["ofs_y"] = rec["coef_y"] = 4096
    rec["H"], rec["W"] = 100, 80
    rec["r1"], rec["c1"] = 10, 10
    for k, v in kw.items():
        rec[k] = v
    return rec


def test_new_entry_points_reject_bad_arguments_without_a_gpu(lib):
    """Every call below fails host-side validation: nothing is enqueued."""
    E_ARG, E_UNS = -1, -2
    ofs = np.zeros(4, np.int32)
    co = np.zeros((4, 8), np.float32)
    assert lib.attwarp_lanczos4_coeffs(0, 4, ofs.ctypes.data, co.ctypes.data) == E_ARG
    assert lib.attwarp_lanczos4_coeffs(4, 4, None, co.ctypes.data) == E_ARG
    rec = _rec(2)
    dev_copy = ctypes.c_void_p(1 << 20)
    assert lib.attwarp_resize_lanczos4(rec.ctypes.data, dev_copy, 0, 24, 24, None) == E_ARG
    assert lib.attwarp_resize_lanczos4(None, dev_copy, 2, 24, 24, None) == E_ARG
    assert lib.attwarp_resize_lanczos4(rec.ctypes.data, ctypes.c_void_p((1 << 20) + 4), 2, 24, 24, None) == E_ARG
    assert lib.attwarp_resize_lanczos4(rec.ctypes.data, dev_copy, 2, 65, 24, None) == E_UNS
    assert lib.attwarp_resize_lanczos4(_rec(2, out=0).ctypes.data, dev_copy, 2, 24, 24, None) == E_ARG
    assert lib.attwarp_resize_lanczos4(_rec(2, H=0).ctypes.data, dev_copy, 2, 24, 24, None) == E_ARG
    assert lib.attwarp_resize_lanczos4(_rec(2, W=40000).ctypes.data, dev_copy, 2, 24, 24, None) == E_UNS
    assert lib.attwarp_resize_lanczos4(_rec(2, coef_y=0).ctypes.data, dev_copy, 2, 24, 24, None) == E_ARG
    assert lib.attwarp_box_metrics_workspace_bytes(rec.ctypes.data, 0) == 0
    assert lib.attwarp_box_metrics_workspace_bytes(rec.ctypes.data, 2) == 2 * 1 * 32
    assert lib.attwarp_box_metrics_workspace_bytes(_rec(1, H=600, W=300).ctypes.data, 1) == 3 * 2 * 32
    ws = ctypes.c_void_p(1 << 21)
    outs = [ctypes.c_void_p(1 << 22)] * 3

    def bm(r, fused=1, h=24, w=24, wsp=ws):
        return lib.attwarp_box_metrics(r.ctypes.data, dev_copy, len(r), fused, h, w, *outs, wsp, None)
    assert bm(_rec(2, r1=101)) == E_ARG                  # slice beyond the map
    assert bm(_rec(2, r0=5, r1=4)) == E_ARG              # reversed slice
    assert bm(_rec(2, c0=-1)) == E_ARG
    assert bm(_rec(2, box_w=1 << 41)) == E_ARG
    assert bm(_rec(2), wsp=ctypes.c_void_p((1 << 21) + 8)) == E_ARG
    assert bm(_rec(2), h=0) == E_ARG
    assert bm(_rec(2, src=0), fused=0) == E_ARG
    assert lib.attwarp_box_metrics(rec.ctypes.data, dev_copy, 2, 1, 24, 24, None, outs[1], outs[2], ws, None) == E_ARG
    # the head-mean probe shares the probe's validation
    q = ctypes.c_void_p(1 << 20)
    st = ctypes.c_void_p(1 << 21)
    assert lib.attwarp_attn_probe_head_mean(q, q, 0, 2, 6, 4, 64, 100, 0, 0, 0, 0, 0, None, st, 50, 0.125, q, q, None) == E_ARG
    assert lib.attwarp_attn_probe_head_mean(q, q, 0, 2, 8, 4, 64, 100, 0, 0, 0, 0, 0, None, None, 50, 0.125, q, q, None) == E_ARG
    assert lib.attwarp_attn_probe_head_mean(q, q, 0, 2, 8, 4, 64, 100, 0, 0, 0, 0, 0, None, st, 101, 0.125, q, q, None) == E_ARG
    assert lib.attwarp_attn_probe_head_mean(q, q, 7, 2, 8, 4, 64, 100, 0, 0, 0, 0, 0, None, st, 50, 0.125, q, q, None) == E_ARG
    assert "attn_probe_head_mean" in lib.attwarp_last_error().decode()


def test_python_surface_has_no_cpu_path():
    from attwarp_amd import grounding as G
    rows = torch.rand(2, 3, 576)
    with pytest.raises(ValueError, match="GPU"):
        G.layer_sweep(rows, rows, [(100, 80)] * 3, [(1, 1, 5, 5)] * 3)
    with pytest.raises(ValueError, match="GPU"):
        G.resize_lanczos4(torch.rand(3, 24, 24), (18, 27))
    with pytest.raises(ValueError, match="GPU"):
        G.box_metrics([torch.rand(10, 10)], [(0, 0, 3, 3)])
    with pytest.raises(ValueError, match="GPU"):
        G.grid_box_metrics(torch.rand(3, 24, 24), (50, 40), [(0, 0, 3, 3)] * 3)


# ---- LayerSweepProbe plumbing on CPU models ---------------------------------------------------------------------------
def _tiny_llama(layers=4):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4,
                                   num_key_value_heads=2, vocab_size=100, max_position_embeddings=256)
    cfg._attn_implementation = "eager"
    torch.manual_seed(0)
    return transformers.LlamaForCausalLM(cfg).eval()


def _tiny_llava():
    transformers = pytest.importorskip("transformers")
    text = transformers.LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                                    num_key_value_heads=4, vocab_size=120, max_position_embeddings=256)
    vision = transformers.CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=5, num_attention_heads=2,
                                           image_size=32, patch_size=8)
    cfg = transformers.LlavaConfig(vision_config=vision, text_config=text, image_token_index=110, projector_hidden_act="gelu",
                                   vision_feature_layer=-2, vision_feature_select_strategy="default")
    torch.manual_seed(0)
    return transformers.LlavaForConditionalGeneration(cfg).eval()


def test_sweep_probe_resolves_and_restores_llama():
    from attwarp_amd import grounding as G
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
    model = _tiny_llama()
    dec = G.decoder_layers(model)
    assert dec is model.model.layers
    before = [l.self_attn.config for l in dec]
    ids = torch.randint(0, 100, (2, 12))
    with torch.no_grad():
        ref = model(input_ids=ids).logits
    with G.LayerSweepProbe(model, [0, 2]) as probe:
        after = [l.self_attn.config for l in dec]
        assert after[1] is before[1] and after[3] is before[3]
        assert after[0] is not before[0] and after[2] is not before[2]
        assert after[0]._attn_implementation.startswith("attwarp_sweep_")
        names = [n for (_, _, n) in probe._saved]
        assert all(n in ALL_ATTENTION_FUNCTIONS._global_mapping for n in names)
        with torch.no_grad():                             # no starts set: the wrapper only delegates
            assert torch.equal(model(input_ids=ids).logits, ref)
        probe.set_image_token_starts([2, 2])
        probe.ntok = 4
        with pytest.raises(RuntimeError, match="GPU"):    # the probe itself has no CPU path
            with torch.no_grad():
                model(input_ids=ids)
    assert [l.self_attn.config for l in dec] == before and all(a is b for a, b in zip((l.self_attn.config for l in dec), before))
    assert not any(n in ALL_ATTENTION_FUNCTIONS._global_mapping for n in names)
    with pytest.raises(ValueError):
        G.LayerSweepProbe(model, [4])
    with pytest.raises(ValueError):
        G.LayerSweepProbe(model, [1, 1])


def test_study_layer_L_is_decoder_index_L_minus_1():
    """uncertainty_attn_maps_llava.py:55 reads out.attentions[L-1] for the study's L: that tensor is what decoder layer L-1's
    attention returns, i.e. LayerSweepProbe(model, [L - 1 for L in LAYERS])."""
    from attwarp_amd import grounding as G
    model = _tiny_llama(layers=4)
    dec = G.decoder_layers(model)
    seen = {}
    hooks = [dec[i].self_attn.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__(i, o[1])) for i in range(4)]
    ids = torch.randint(0, 100, (1, 10))
    with torch.no_grad():
        out = model(input_ids=ids, output_attentions=True)
    for h in hooks:
        h.remove()
    for L in (1, 2, 4):
        assert torch.equal(out.attentions[L - 1], seen[L - 1])


def test_sweep_probe_resolves_llava_text_layers_not_the_vision_tower():
    from attwarp_amd import grounding as G
    model = _tiny_llava()
    dec = G.decoder_layers(model)
    assert len(dec) == 3 and dec is model.get_decoder().layers
    assert all(type(l).__name__ == "LlamaDecoderLayer" for l in dec)
    before = [l.self_attn.config for l in dec]
    vision = [m for m in model.modules() if type(m).__name__ == "CLIPAttention"]
    vbefore = [m.config for m in vision]
    p = G.LayerSweepProbe(model, [1, 2])
    assert dec[0].self_attn.config is before[0] and dec[1].self_attn.config is not before[1]
    assert all(m.config is c for m, c in zip(vision, vbefore))
    p.remove()
    assert all(l.self_attn.config is c for l, c in zip(dec, before))


def test_sweep_probe_fails_loudly_without_attention_interface(monkeypatch):
    from attwarp_amd import grounding as G
    import transformers.modeling_utils as mu
    model = _tiny_llama(layers=2)
    monkeypatch.delattr(mu, "AttentionInterface")
    with pytest.raises(RuntimeError, match="AttentionInterface"):
        G.LayerSweepProbe(model, [0])
