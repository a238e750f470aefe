"""The gate of the float32 resample's streaming cache policy, read through the tuning flavour's plan query (no launch, no
GPU): only a launch of the 1024 x 3 class whose source plus destination bytes exceed the 256 MiB Infinity Cache streams;
every other class, and the same class below the cache size, is planned exactly as before."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE = 256 << 20
SHIP = 1                 # "stream" of a launch that takes the streaming variant (nontemporal stores)


@pytest.fixture(scope="module")
def plan():
    from attwarp_amd import _lib
    if not os.path.exists(_lib.TUNING_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.remap_plan


def test_gate_at_the_cache_size(plan):
    per_image = 2 * 1024 * 1024 * 3 * 4                  # source + destination bytes of one 1024 x 1024 x 3 float32 image
    below = CACHE // per_image                           # the largest batch that still fits
    assert below * per_image <= CACHE < (below + 1) * per_image and below == 10
    for mode, cpw, group in (("cv2", 2, 8), ("exact", 1, 3)):
        big = plan(256, 3, 1024, 1024, 1024, 1024, mode)
        assert big == {"rows": 3, "cpw": cpw, "group": group, "stream": SHIP}, (mode, big)
        fits, over = plan(below, 3, 1024, 1024, 1024, 1024, mode), plan(below + 1, 3, 1024, 1024, 1024, 1024, mode)
        assert fits["stream"] == 0 and over["stream"] == SHIP, (mode, fits, over)
        # the policy is all the gate changes: block shape and order are those of the cached launch
        from attwarp_amd import _lib
        with _lib.debug_override(remap_stream=0):
            assert plan(below + 1, 3, 1024, 1024, 1024, 1024, mode) == dict(over, stream=0)
        # bytes, not images, decide: the same batch with half the output rows fits again
        assert plan(below + 1, 3, 1024, 1024, 256, 1024, mode)["stream"] == 0
        assert plan(below + 1, 3, 2048, 1024, 1024, 1024, mode)["stream"] == SHIP


@pytest.mark.parametrize("mode", ["cv2", "exact"])
def test_other_classes_never_stream(plan, mode):
    from attwarp_amd import _lib
    others = [
        dict(B=256, C=3, H=336, W=336, H_out=336, W_out=336),                          # the 336 x 3 class, 690 MB
        dict(B=256, C=3, H=1024, W=1024, H_out=1024, W_out=1024, channels_last=False),  # planar: plane by plane, 4 KB rows
        dict(B=256, C=4, H=1024, W=1024, H_out=1024, W_out=1024),                      # 16 KB rows (KI = 4)
        dict(B=256, C=3, H=1024, W=1024, H_out=1024, W_out=1000),                      # per-element store offsets
        dict(B=256, C=3, H=1024, W=1024, H_out=1024, W_out=500),                       # KO = 8
        dict(B=256, C=3, H=768, W=768, H_out=768, W_out=768),                          # 9 KB rows
        dict(B=64, C=3, H=2048, W=2048, H_out=2048, W_out=2048),                       # column tiles
        dict(B=256, C=1, H=1024, W=1024, H_out=1024, W_out=1024),                      # 4 KB rows
    ]
    for kw in others:
        p = plan(mode=mode, **kw)
        assert p is not None and p["stream"] == 0, (kw, p)
        with _lib.debug_override(remap_stream=1):         # not even when forced: the variant does not exist for them
            assert plan(mode=mode, **kw)["stream"] == 0, kw


def test_the_key_forces_the_policy_either_way(plan):
    from attwarp_amd import _lib
    small, big = (3, 3, 24, 1024, 7, 1024), (256, 3, 1024, 1024, 1024, 1024)
    assert plan(*small)["stream"] == 0 and plan(*big)["stream"] == SHIP
    for v in (0, 1):
        with _lib.debug_override(remap_stream=v):
            assert plan(*small)["stream"] == v and plan(*big)["stream"] == v
    assert plan(*small)["stream"] == 0 and plan(*big)["stream"] == SHIP
    with _lib.debug_override(remap_variant=1):            # the generic gather kernel: no plan
        assert plan(*big) is None
    with pytest.raises(_lib.AttWarpError):                # a malformed query is an error, not a plan
        plan(0, 3, 1024, 1024, 1024, 1024)
