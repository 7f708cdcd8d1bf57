"""The batched inference tail without a GPU: the two entry points are part of the build (their signatures are pinned in
tests/test_abi_cpu.py), and native.DetBatch's host-side views on hand-made CPU tensors."""
import os

import torch

from uni3detr_amd import native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_and_bound():
    for name in ("u3d_det_tail_workspace", "u3d_det_tail"):
        assert name in nv.exported_symbols()
    assert os.path.exists(os.path.join(ROOT, "uni3detr_amd", "csrc", "det_tail.hip"))
    assert (nv.DET_TAIL_NONE, nv.DET_TAIL_NMS, nv.DET_TAIL_DECODE) == (0, 1, 2)


def _batch(count, K=4, D=7):
    B = len(count)
    boxes = torch.arange(B * K * D, dtype=torch.float32).reshape(B, K, D) + 1
    scores = torch.arange(B * K, dtype=torch.float32).reshape(B, K) + 1
    labels = torch.arange(B * K, dtype=torch.int32).reshape(B, K) + 1
    cnt = torch.tensor(count, dtype=torch.int32)
    off = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(cnt, 0).int()])
    return nv.DetBatch(boxes, scores, labels, cnt, off)


def test_det_batch_empty_scene_in_the_middle():
    d = _batch([2, 0, 3])
    lst = d.to_list()
    assert len(d) == 3 and [r[1].tolist() for r in lst] == [[1.0, 2.0], [], [9.0, 10.0, 11.0]]
    assert [r[2].tolist() for r in lst] == [[1, 2], [], [9, 10, 11]] and all(r[2].dtype == torch.long for r in lst)
    assert lst[1][0].shape == (0, 7) and torch.equal(lst[2][0], d.boxes[2, :3])
    bx, sc, lb, off = d.packed()
    assert sc.tolist() == [1.0, 2.0, 9.0, 10.0, 11.0] and lb.tolist() == [1, 2, 9, 10, 11] and lb.dtype == torch.int32
    assert torch.equal(bx, torch.cat([d.boxes[0, :2], d.boxes[2, :3]])) and off.tolist() == [0, 2, 2, 5]
    h = d.cpu()
    assert torch.equal(h.boxes, d.boxes) and torch.equal(h.off, d.off)


def test_det_batch_all_scenes_empty():
    d = _batch([0, 0, 0], D=9)
    assert [tuple(r[0].shape) for r in d.to_list()] == [(0, 9)] * 3 and all(r[1].numel() == 0 and r[2].numel() == 0 for r in d.to_list())
    bx, sc, lb, off = d.packed()
    assert bx.shape == (0, 9) and sc.shape == (0,) and lb.shape == (0,) and off.tolist() == [0, 0, 0, 0]


def test_det_batch_from_list_round_trip():
    dets = [[torch.ones(2, 7), torch.tensor([0.5, 0.25]), torch.tensor([1, 0])], [torch.zeros(0, 7), torch.zeros(0), torch.zeros(0, dtype=torch.long)]]
    d = nv.DetBatch.from_list(dets, 3, 7, torch.device("cpu"))
    assert d.boxes.shape == (2, 3, 7) and d.count.tolist() == [2, 0] and d.off.tolist() == [0, 2, 2] and d.labels.dtype == torch.int32
    assert not d.boxes[0, 2:].any() and not d.scores[1].any()
    for got, want in zip(d.to_list(), dets):
        assert all(torch.equal(g, w) for g, w in zip(got, want))
