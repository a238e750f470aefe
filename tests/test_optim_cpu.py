"""CPU-only checks of the optimiser step: tests/optim_ref.py (the float64 restatement the GPU tests compare against) is
pinned against the real torch.optim.AdamW + clip_grad_norm_ + torch.amp.GradScaler("cpu") on float64 parameters, and the
parts of attwarp_amd.optim that need no GPU (rejections, the workspace size of the library, the state-dict keys)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from optim_ref import AdamWRef, Scale, inv_scale32

SHAPES = [(1,), (3,), (4097,), (256, 256, 3, 3), (512, 256)]


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_restatement_matches_torch_float64():
    """Six steps, an inf gradient at step 3, growth_interval=2: p, m, v, step counts, scale and norm agree to 1e-12."""
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    hyper = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.AdamW(params, **hyper)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=2)
    scaler.scale(torch.zeros(()))                      # creates the scale tensor, as scaler.scale(loss) does in a trainer
    ref = AdamWRef(p0, [dict(idx=list(range(len(p0))), **hyper)], max_grad_norm=1.0)
    sched = Scale(init_scale=1024.0, growth_interval=2)
    worst = 0.0
    for step in range(1, 7):
        scale = float(sched.scale)
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.05 * scale for s in SHAPES]
        if step == 3:
            grads[-1].view(-1)[-1] = float("inf")
        for p, g in zip(params, grads):
            p.grad = g.clone()
        scaler.unscale_(opt)
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
        scaler.step(opt)
        scaler.update()
        taken = ref.step(grads, scale=scale)
        sched.update(not taken)
        assert taken == (step != 3)
        assert float(scaler.get_scale()) == float(sched.scale)
        assert int(scaler._growth_tracker.item()) == sched.tracker
        if taken:
            worst = max(worst, abs(float(norm) - ref.grad_norm) / ref.grad_norm)
        else:
            assert math.isinf(float(norm)) and math.isinf(ref.grad_norm)
        for i, p in enumerate(params):
            st = opt.state[p]
            assert int(st["step"]) == ref.t[i]
            worst = max(worst, _rel(p.detach(), ref.p[i]), _rel(st["exp_avg"], ref.m[i]), _rel(st["exp_avg_sq"], ref.v[i]))
    assert [float(x) for x in (sched.scale,)] == [2048.0] and ref.t == [5] * len(SHAPES)
    print(f"restatement vs torch float64: worst relative distance {worst:.3e}")
    assert worst <= 1e-12, worst


def test_inv_scale_is_the_float64_reciprocal_rounded_once():
    for s in (1024.0, 3.0, 65536.0, 0.1):
        want = float(torch.tensor(s, dtype=torch.float32).double().reciprocal().float())
        assert inv_scale32(s) == want


def test_rejections_without_a_gpu():
    from attwarp_amd import optim
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="tensor lr"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], maximize=True)
    with pytest.raises(ValueError, match="global"):
        optim.AdamW([dict(params=[torch.nn.Parameter(torch.zeros(4))], max_grad_norm=1.0),
                     dict(params=[torch.nn.Parameter(torch.zeros(4))], max_grad_norm=2.0)])
    assert optim.AdamW._step_supports_amp_scaling is True


def test_workspace_bytes_follow_the_chunk():
    """The Python CHUNK is the library's: one more chunk costs one more float64 partial, one more tensor a partial and a
    64-byte record."""
    from attwarp_amd import _lib, optim
    lib = _lib.load()
    wb = lib.attwarp_adamw_workspace_bytes
    assert wb(optim.CHUNK, 1) - wb(optim.CHUNK - 1, 1) == 8
    assert wb(2 * optim.CHUNK - 1, 1) == wb(optim.CHUNK, 1)
    assert wb(optim.CHUNK, 2) - wb(optim.CHUNK, 1) == 8 + 64
    assert wb(0, 0) == 32 and wb(-1, 1) == 0
    assert ctypes.sizeof(_lib.AdamWTensor) == 88


def test_step_call_rejects_bad_arguments_on_the_host():
    """attwarp_adamw_step validates before it launches: no GPU is touched by these calls."""
    from attwarp_amd import _lib
    lib = _lib.load()
    desc = (_lib.AdamWTensor * 1)()
    one = ctypes.c_void_p(64)
    args = lambda ws_bytes: (ctypes.cast(desc, ctypes.c_void_p), 1, 1.0, 1e-6, None, None, one, one, one, ws_bytes, None)
    assert lib.attwarp_adamw_step(*args(4096)) == -1 and b"null pointer" in lib.attwarp_last_error()
    desc[0].p = desc[0].g = desc[0].m = desc[0].v = 64
    desc[0].numel, desc[0].beta1, desc[0].beta2 = 5000, 0.9, 0.999
    assert lib.attwarp_adamw_step(*args(32 + 8 + 64)) == -1 and b"workspace" in lib.attwarp_last_error()
    desc[0].g = 66
    assert lib.attwarp_adamw_step(*args(4096)) == -1 and b"4-byte aligned" in lib.attwarp_last_error()
    desc[0].g, desc[0].beta1 = 64, 1.0
    assert lib.attwarp_adamw_step(*args(4096)) == -1 and b"betas" in lib.attwarp_last_error()
