"""static_batch without a GPU: the capacity arithmetic, the host-side validation of a packed batch against CPU-resident buffers (no
refusal reaches u3d_batch_ingest) and the rule for when the several-workgroup FPS can time out."""
from types import SimpleNamespace

import pytest
import torch

from uni3detr_amd import native as nv
from uni3detr_amd import static_batch as sb

B, P, F, G = 2, 8, 4, 3


@pytest.mark.parametrize("margin, want", [(1.0, [0, 256, 256, 256, 512]), (1.25, [0, 256, 512, 512, 512])])
def test_level_capacity_rounds_the_margin_up_to_256(margin, want):
    # int(count * margin), then up to a multiple of 256: 255 * 1.25 = 318 -> 512, 256 * 1.25 = 320 -> 512, 257 * 1.25 = 321 -> 512
    assert [sb.level_capacity(c, margin) for c in (0, 1, 255, 256, 257)] == want


def test_max_level_counts_folds_per_level():
    assert sb.max_level_counts([[900, 40, 7, 3], [700, 55, 7, 9]]) == [900, 55, 7, 9]
    assert sb.max_level_counts([[5, 4, 3]]) == [5, 4, 3]


def _batch(gt=False):
    b = dict(points=torch.zeros(10, F), scene_off=torch.tensor([0, 6, 10], dtype=torch.int32), count=torch.tensor([6, 4], dtype=torch.int32))
    if gt:
        b.update(gt_bboxes_3d=torch.zeros(3, 7), gt_labels_3d=torch.zeros(3, dtype=torch.int32), gt_off=torch.tensor([0, 1, 3], dtype=torch.int32))
    return b


@pytest.mark.parametrize("prefix", ["set_packed_batch:", "InferenceStep:"])
def test_bind_packed_refusals_carry_the_prefix_and_never_reach_the_ingest(prefix, monkeypatch):
    def no_ingest(*a, **k):
        raise AssertionError("a refusal reached u3d_batch_ingest")
    monkeypatch.setattr(nv, "batch_ingest", no_ingest)
    plain, with_gt = sb.StaticBatch(B, P, F, "cpu"), sb.StaticBatch(B, P, F, "cpu", G, 7)
    assert plain.gts is None and plain.pts["cat"].shape == (B * P, F) and plain.pts["lens"] == [P] * B
    assert with_gt.gts["gt"].shape == (B * G, 7) and with_gt.gts["labels"].dtype == torch.int32 and with_gt.gts["gmax"] == G
    ok = _batch()
    wide = torch.zeros(10, 2 * F)
    cases = [(plain, dict(ok, sweeps={}), "sweeps"),
             (plain, dict(ok, points=ok["points"].double()), "float32"),
             (plain, dict(ok, points=wide[:, ::2]), "contiguous"),
             (plain, dict(ok, points=torch.zeros(10, F + 1)), f"\\[n, {F}\\]"),
             (plain, dict(ok, scene_off=torch.zeros(B + 2, dtype=torch.int32)), f"{B + 1} scenes, the step was built for {B}"),
             (plain, dict(ok, count=ok["count"].long()), "count must be a contiguous int32 tensor of 2 elements"),
             (with_gt, dict(_batch(gt=True), gt_labels_3d=None), "needs gt_labels_3d and gt_off"),
             (with_gt, {k: v for k, v in _batch(gt=True).items() if k != "gt_off"}, "needs gt_labels_3d and gt_off")]
    for buf, batch, what in cases:
        with pytest.raises(ValueError, match=f"^{prefix} .*{what}"):
            buf.bind_packed(batch, prefix)
    # the well-formed batches are what does reach it: once each, with GT exactly when the buffers have GT
    calls = []
    monkeypatch.setattr(nv, "batch_ingest", lambda *a, **k: calls.append(k))
    plain.bind_packed(_batch(gt=True), prefix)
    with_gt.bind_packed(_batch(gt=True), prefix)
    assert len(calls) == 2 and calls[0]["gt"] is None and calls[0]["gt_out"] is None
    assert calls[1]["gt"] is not None and calls[1]["gt_out"] is with_gt.gts["gt"] and calls[1]["gt_cap"] == G


def test_fps_can_time_out_above_the_register_limit_unless_single_workgroup():
    assert not sb.fps_can_time_out(SimpleNamespace(), nv.FPS_REG_MAX)
    assert sb.fps_can_time_out(SimpleNamespace(), nv.FPS_REG_MAX + 1)
    assert sb.fps_can_time_out(SimpleNamespace(fps_max_wg=0), nv.FPS_REG_MAX + 1)
    for n in (1, nv.FPS_REG_MAX, nv.FPS_REG_MAX + 1, 10 * nv.FPS_REG_MAX):
        assert not sb.fps_can_time_out(SimpleNamespace(fps_max_wg=1), n)
