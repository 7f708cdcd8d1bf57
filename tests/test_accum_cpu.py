"""Gradient accumulation / non-finite skip / EMA of the flat AdamW step, host side: the restatement of u3d_adamw_step_accum
(tests/accum_ref.py) against torch.optim.AdamW fed the window's mean gradient, what a held call and a dropped window leave alone,
the argument checks of TrainStep and the bindings."""
import types

import pytest
import torch

import accum_ref as R


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("max_norm", [0.0, 0.5])
def test_restatement_equals_torch_adamw_fed_the_window_mean(max_norm, dtype):
    """k micro-gradients through the restatement == clip_grad_norm_ + AdamW on their mean, at the tolerance of
    test_flat_adamw_with_clipping_matches_torch (tests/test_trainer_gpu.py)."""
    n, k = 4099, 3
    torch.manual_seed(n)
    p0 = torch.randn(n)
    pr = torch.nn.Parameter(p0.clone().to(dtype))
    opt = torch.optim.AdamW([pr], lr=3e-3, weight_decay=0.01)
    ref = R.AccumRef(p0, k=k, dtype=dtype, max_norm=max_norm)
    for it in range(4):
        gs = [torch.randn(n) * (10.0 if it % 2 else 0.01) for _ in range(k)]
        before = [t.clone() for t in ref.tensors()[:3]]
        for j, g in enumerate(gs):
            out = ref.call(g)
            if j < k - 1:
                assert out == R.ACCUMULATED and ref.fill == j + 1
                assert all(torch.equal(a, b) for a, b in zip(before, ref.tensors()[:3]))
        assert out == R.APPLIED and ref.fill == 0 and ref.step == it + 1 and ref.applied == it + 1
        assert not ref.acc.any()
        mean = (gs[0].to(dtype) + gs[1].to(dtype) + gs[2].to(dtype)) / k
        pr.grad = mean.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pr], max_norm)
        opt.step()
        gn = float(mean.double().norm())
        assert abs(ref.norm - gn) <= 1e-5 * gn
        assert (ref.p - pr.detach()).abs().max().item() <= 2e-6 * max(1.0, pr.detach().abs().max().item()), it


def test_held_call_and_dropped_window_leave_the_state_alone():
    n, k = 301, 3
    torch.manual_seed(0)
    skip = torch.zeros((n + 63) // 64, dtype=torch.uint8)
    skip[1] = 1
    ref = R.AccumRef(torch.randn(n), k=k, max_norm=0.5, ema_decay=0.9, skip=skip)
    for _ in range(k):
        ref.call(torch.randn(n))                                   # one applied update: moments and EMA are not trivial
    assert ref.applied == 1 and not torch.equal(ref.ema, ref.p)
    ref.call(torch.randn(n))
    before = [t.clone() for t in ref.tensors()]
    counters = (ref.step, ref.fill, ref.applied, ref.dropped)
    assert ref.call(torch.full((n,), float("nan")), hold=True) == R.HELD
    assert all(torch.equal(a, b) for a, b in zip(before, ref.tensors()))        # the accumulator included
    assert (ref.step, ref.fill, ref.applied, ref.dropped) == counters and ref.held == 1
    for bad in (float("inf"), float("nan")):
        before = [t.clone() for t in ref.tensors()]
        drops, step, applied = ref.dropped, ref.step, ref.applied
        while True:
            g = torch.randn(n)
            g[7] = bad
            if ref.call(g) != R.ACCUMULATED:
                break
        assert ref.outcome == R.DROPPED and ref.dropped == drops + 1 and ref.fill == 0 and (ref.step, ref.applied) == (step, applied)
        p, m, v, acc, ema = ref.tensors()
        assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2]) and torch.equal(ema, before[4])
        assert not acc.any()
    # a skipped chunk never moves, in any buffer
    sl = slice(64, 128)
    p0 = ref.p[sl].clone()
    for _ in range(k):
        ref.call(torch.randn(n))
    assert ref.outcome == R.APPLIED and torch.equal(ref.p[sl], p0) and not ref.acc[sl].any() and not ref.m[sl].any()


def test_train_step_refuses_bad_accumulation_arguments_before_any_device_work():
    from uni3detr_amd.trainer import TrainStep
    pts = [torch.zeros((40, 4)), torch.zeros((70, 4))]
    model = types.SimpleNamespace(dynamic_voxelization=False)       # no parameters(): anything past the checks would fail on it
    with pytest.raises(ValueError, match="accum_steps"):
        TrainStep(model, pts, [], [], accum_steps=0)
    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(model, pts, [], [], ema_decay=1.0)
    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(model, pts, [], [], ema_decay=0.0)
    with pytest.raises(NotImplementedError, match="flat_update"):
        TrainStep(model, pts, [], [], accum_steps=2, flat_update=False)
    with pytest.raises(NotImplementedError, match="flat_update"):
        TrainStep(model, pts, [], [], skip_nonfinite=True, flat_update=False)


def test_bindings_and_header_declare_the_new_entries():
    """(their parameter counts are pinned in tests/test_abi_cpu.py)"""
    from uni3detr_amd import native as nv
    for name in ("u3d_adamw_step_accum", "u3d_adamw_set_accum"):
        assert name in nv.exported_symbols()
    assert callable(nv.adamw_step_accum) and callable(nv.adamw_set_accum)
