"""Host-side checks of the MarginalNet training losses: the Python surface matches the reference's signatures (from the
fixture tests/golden/losses.npz), and every new C entry point rejects bad sizes and null pointers with ATTWARP_E_ARG
before touching a GPU."""
import inspect
import json

import pytest

ATTWARP_E_ARG = -1
ATTWARP_E_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def lib():
    from attwarp_amd import _lib
    return _lib.load()


def test_losses_module_matches_reference_signatures(golden):
    from attwarp_amd import losses, model
    meta = json.loads(str(golden("losses")["meta"]))
    assert set(meta["signatures"]) == {"l1_cdf_loss", "sym_kl", "separable_recon_loss", "recon_l1", "build_axis_cdf_targets",
                                       "cdf_from_density_downsample", "mix_with_uniform", "entropy"}
    for name, ref in meta["signatures"].items():
        fn = getattr(model if name in ("mix_with_uniform", "entropy") else losses, name)
        params = list(inspect.signature(fn).parameters.values())
        assert len(params) >= len(ref), name
        for p, (ref_name, ref_default) in zip(params, ref):
            assert p.name == ref_name, (name, p.name, ref_name)
            got = None if p.default is inspect.Parameter.empty else p.default
            assert got == ref_default, (name, p.name, got, ref_default)
        for p in params[len(ref):]:                       # extra trailing parameters are keywords with defaults
            assert p.default is not inspect.Parameter.empty, (name, p.name)


def test_trainer_entry_points_exist():
    from attwarp_amd import losses, pipeline
    assert list(inspect.signature(losses.pdf_l1_loss).parameters) == ["px_s", "py_s", "px_gt_vis", "py_gt_vis", "W", "H", "eps"]
    assert inspect.signature(losses.pdf_l1_loss).parameters["eps"].default == 1e-8
    assert list(inspect.signature(pipeline.trainer_attention_targets).parameters) == ["A_full", "transforms", "grid"]


def test_cpu_tensors_raise():
    import torch
    from attwarp_amd import losses, model
    p = torch.full((2, 24), 1.0 / 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.l1_cdf_loss(p, p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.entropy(p)
    assert model.mix_with_uniform(p, 0.0) is p           # alpha <= 0 returns p itself, as the reference


def test_new_entry_points_reject_bad_arguments(lib):
    P = 1 << 20
    calls = {
        "attwarp_cdf_downsample": [(None, 2, 24, 128, P, None), (P, 0, 24, 128, P, None), (P, 2, 24, 0, P, None)],
        "attwarp_build_axis_cdf_targets": [(None, 2, 24, 24, 128, P, P, P, None), (P, 2, 0, 24, 128, P, P, P, None),
                                           (P, 2, 24, 24, 128, P, None, P, None)],
        "attwarp_l1_cdf_loss": [(P, None, 2, 24, P, P, P, None), (P, P, 2, 0, P, P, P, None), (P, P, 2, 24, P, None, P, None)],
        "attwarp_l1_cdf_loss_backward": [(P, P, 2, 24, None, P, P, None), (P, P, -1, 24, P, P, P, None)],
        "attwarp_sym_kl": [(None, P, 2, 24, 1e-6, P, P, P, None), (P, P, 2, 0, 1e-6, P, P, P, None)],
        "attwarp_sym_kl_backward": [(P, P, 2, 24, 1e-6, P, None, P, None), (P, P, 0, 24, 1e-6, P, P, P, None)],
        "attwarp_recon_loss": [(P, P, None, 2, 24, 24, 0, P, P, P, None), (P, P, P, 2, 0, 24, 1, P, P, P, None),
                               (P, P, P, 2, 24, 24, 7, P, P, P, None)],
        "attwarp_recon_loss_backward": [(P, P, P, 2, 24, 24, 0, None, P, P, None), (P, P, P, 2, 24, -3, 1, P, P, P, None),
                                        (P, P, P, 2, 24, 24, 2, P, P, P, None)],
        "attwarp_scale_shift": [(None, 48, 0.5, 0.1, P, None), (P, 0, 0.5, 0.1, P, None)],
        "attwarp_entropy": [(None, 2, 24, 1e-8, P, P, P, None), (P, 2, 0, 1e-8, P, P, P, None)],
        "attwarp_entropy_backward": [(P, 2, 24, 1e-8, None, P, None), (P, 0, 24, 1e-8, P, P, None)],
        "attwarp_pdf_l1_loss": [(P, P, P, None, 2, 24, 24, 512, 512, P, P, P, P, P, None),
                                (P, P, P, P, 2, 24, 24, 0, 512, P, P, P, P, P, None),
                                (P, P, P, P, 2, 24, 24, 512, 512, P, P, P, None, P, None)],
        "attwarp_pdf_l1_loss_backward": [(P, P, P, P, 2, 24, 24, 512, 512, P, None, P, P, P, None),
                                         (P, P, P, P, 2, 0, 24, 512, 512, P, P, P, P, P, None)],
        "attwarp_trainer_attention_targets": [(P, None, 2, 96, 96, 24, 24, P, P, P, None),
                                              (P, P, 2, 96, 96, 0, 24, P, P, P, None),
                                              (P, P, 0, 96, 96, 24, 24, P, P, P, None)],
    }
    for name, cases in calls.items():
        for args in cases:
            assert getattr(lib, name)(*args) == ATTWARP_E_ARG, (name, args)
    # size limits: a valid request the build cannot serve, refused before anything is enqueued
    too_big = {
        "attwarp_cdf_downsample": [(P, 2, 4097, 24, P, None), (P, 2, 24, 4097, P, None), (P, 65536, 24, 24, P, None)],
        "attwarp_l1_cdf_loss": [(P, P, 2, 4097, P, P, P, None)],
        "attwarp_l1_cdf_loss_backward": [(P, P, 2, 4097, P, P, P, None)],
        "attwarp_sym_kl": [(P, P, 2, 4097, 1e-6, P, P, P, None)],
        "attwarp_entropy": [(P, 2, 4097, 1e-8, P, P, P, None)],
        "attwarp_entropy_backward": [(P, 2, 4097, 1e-8, P, P, None)],
        "attwarp_recon_loss": [(P, P, P, 2, 4097, 24, 0, P, P, P, None), (P, P, P, 2, 24, 4097, 1, P, P, P, None)],
        "attwarp_recon_loss_backward": [(P, P, P, 2, 4097, 24, 0, P, P, P, None)],
        "attwarp_pdf_l1_loss": [(P, P, P, P, 2, 24, 24, 8193, 512, P, P, P, P, P, None),
                                (P, P, P, P, 2, 65, 24, 512, 512, P, P, P, P, P, None)],
        "attwarp_pdf_l1_loss_backward": [(P, P, P, P, 2, 24, 24, 512, 8193, P, P, P, P, P, None)],
        # 16384 + 4096 doubles are a compute unit's whole LDS; with the kernel's own 32 bytes the launch cannot fit
        "attwarp_build_axis_cdf_targets": [(P, 2, 24, 16384, 4096, P, P, P, None), (P, 2, 16384, 24, 4096, P, P, P, None),
                                           (P, 2, 24, 16385, 24, P, P, P, None), (P, 2, 24, 24, 4097, P, P, P, None)],
        "attwarp_trainer_attention_targets": [(P, P, 2, 96, 16385, 24, 24, P, P, P, None)],
    }
    for name, cases in too_big.items():
        for args in cases:
            assert getattr(lib, name)(*args) == ATTWARP_E_UNSUPPORTED, (name, args)
