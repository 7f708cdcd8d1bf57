"""The batched inference tail (csrc/det_tail.hip: u3d_det_tail behind NMSFreeCoder.decode_batched, Uni3DETRHead.get_bboxes_batched,
Uni3DETR.simple_test_batched and aug_test(batched_tail=True)) against the per-scene path it replaces (NMSFreeCoder.decode,
Uni3DETRHead.get_bboxes), which tests/golden/coder_decode.npz pins to the reference.  Every comparison is per scene and bit for bit:
torch.equal on boxes, scores and labels, and the count."""
import ast
import copy
import os

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import native as nv
from uni3detr_amd.plugin.bbox import NMSFreeCoder

pytestmark = pytest.mark.gpu

RANGE = [-4.0, -4.0, -2.0, 4.0, 4.0, 2.0]


@pytest.fixture(scope="module")
def head():
    """get_bboxes / get_bboxes_batched read only bbox_coder, post_processing and num_classes: one head, re-dressed per test."""
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    return build_model(copy.deepcopy(MODEL_CFG)).pts_bbox_head.eval()


def _dress(head, C, pp, max_num=50, score_threshold=None, post_range=RANGE, alpha=0.5):
    head.num_classes = C
    head.post_processing = pp
    head.bbox_coder = NMSFreeCoder(pc_range=RANGE, post_center_range=post_range, max_num=max_num, score_threshold=score_threshold,
                                   alpha=alpha, num_classes=C)
    return head


def _preds(dev, B, Q, C, dim, seed, spread=3.0, L=3):
    """Random head outputs: centres N(0, spread) (some beyond RANGE), sizes around 1, any yaw."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    code = [r(L, B, Q, 2) * spread, r(L, B, Q, 2) * 0.3, r(L, B, Q, 1) * 0.8, r(L, B, Q, 1) * 0.3, r(L, B, Q, 2)]
    if dim == 9:
        code.append(r(L, B, Q, 2))
    return dict(all_cls_scores=(r(L, B, Q, C) - 0.5).to(dev), all_bbox_preds=torch.cat(code, -1).to(dev),
                all_iou_preds=r(L, B, Q, 1).to(dev))


def _reference(head, preds):
    """The per-scene path.  Under num_thr its torch.argsort(-scores) leaves equal scores in an open order, so the scores that enter
    that sort must be pairwise distinct for the comparison to say anything: asserted here."""
    pp = head.post_processing
    if pp is not None and "num_thr" in pp:
        head.post_processing = {k: v for k, v in pp.items() if k != "num_thr"}
        for _, s, _ in head.get_bboxes(preds, None):
            assert torch.unique(s).numel() == s.numel(), "tied scores under num_thr: the per-scene order is unpinned"
        head.post_processing = pp
    return head.get_bboxes(preds, None)


def _assert_same(det, ref):
    got = det.to_list()
    cnt = det.count.cpu().tolist()
    assert len(got) == len(ref) == len(det)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert cnt[b] == r[0].shape[0], (b, cnt[b], r[0].shape[0])
        assert g[2].dtype == torch.long and det.labels.dtype == torch.int32
        assert torch.equal(g[0], r[0]), (b, "boxes")
        assert torch.equal(g[1], r[1]), (b, "scores")
        assert torch.equal(g[2], r[2].long()), (b, "labels")
    off = det.off.cpu().tolist()
    assert off == [0] + np.cumsum(cnt).tolist()
    K = det.scores.shape[1]
    past = torch.arange(K, device=det.count.device)[None, :] >= det.count[:, None]
    assert not det.boxes[past].any() and not det.scores[past].any() and not det.labels[past].any()     # rows past the count are zero
    return cnt


PPS = [None, dict(type="nms", nms_thr=0.2), dict(type="nms", nms_thr=0.2, score_thr=0.12),
       dict(type="nms", nms_thr=0.2, score_thr=[0.05, 0.2, 0.12]), dict(type="nms", nms_thr=0.2, num_thr=10),
       dict(type="nms", nms_thr=0.2, score_thr=[0.05, 0.2, 0.12], num_thr=10)]


def test_decode_batched_equals_decode_on_the_reference_golden(cuda):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "coder_decode.npz"))
    preds = dict(all_cls_scores=torch.from_numpy(z["cls"]).to(cuda), all_bbox_preds=torch.from_numpy(z["box"]).to(cuda),
                 all_iou_preds=torch.from_numpy(z["iou"]).to(cuda))
    si = 0
    while f"s{si}_cfg" in z:
        c = z[f"s{si}_cfg"]
        coder = NMSFreeCoder(pc_range=list(z["pc_range"]), voxel_size=[0.02] * 3, post_center_range=[float(v) for v in c[3:9]],
                             max_num=int(c[2]), score_threshold=None if c[1] < 0 else float(c[1]), alpha=float(c[0]), num_classes=10)
        ref = coder.decode(preds)
        det = coder.decode_batched(preds)
        _assert_same(det, [[r["bboxes"], r["scores"], r["labels"]] for r in ref])
        for b, (bx, sc, lb) in enumerate(det.to_list()):                  # ... and hence the reference file's own output
            assert lb.cpu().numpy().tolist() == z[f"s{si}_b{b}_labels"].tolist(), (si, b)
            for k, got in (("bboxes", bx), ("scores", sc)):
                want = z[f"s{si}_b{b}_{k}"]
                assert got.shape == want.shape and np.abs(got.cpu().numpy() - want).max(initial=0.0) <= 1e-6 * max(1.0, np.abs(want).max(initial=0.0))
        si += 1
    assert si == 3


@pytest.mark.parametrize("dim", [7, 9])
@pytest.mark.parametrize("pp", PPS, ids=lambda p: "none" if p is None else "-".join(k for k in p if k != "type"))
def test_small_random_heads(cuda, head, dim, pp):
    """B=3, Q=40, C=3, max_num=50: some candidates beyond post_center_range, the last scene entirely outside it (count 0)."""
    preds = _preds(cuda, 3, 40, 3, dim, seed=dim)
    preds["all_bbox_preds"][:, 2, :, 0] += 1000.0
    _dress(head, 3, pp)
    ref = _reference(head, preds)
    cnt = _assert_same(head.get_bboxes_batched(preds, None), ref)
    assert cnt[2] == 0 and min(cnt[:2]) > 0
    if pp is None:
        assert max(cnt) < 50                                              # the centre range did drop candidates
        dec = head.bbox_coder.decode_batched(preds)
        _assert_same(dec, [[r["bboxes"], r["scores"], r["labels"]] for r in head.bbox_coder.decode(preds)])


@pytest.mark.parametrize("pp", [None, dict(type="nms", nms_thr=0.2)], ids=["none", "nms"])
def test_raw_score_ties_follow_the_pinned_order(cuda, head, pp):
    """Logit rows (class and IoU) repeated over the queries: many (query, class) entries tie, across the k-th place too, and so do
    the fused scores the NMS sorts by; boxes stay distinct, so the order is visible.  No num_thr: its ties are unpinned upstream."""
    B, Q, C = 2, 40, 3
    preds = _preds(cuda, B, Q, C, 7, seed=11, spread=1.0)
    pick = torch.randint(0, 5, (Q,), generator=torch.Generator().manual_seed(3)).to(cuda)
    preds["all_cls_scores"] = preds["all_cls_scores"][:, :, :5][:, :, pick].contiguous()
    preds["all_iou_preds"] = preds["all_iou_preds"][:, :, :5][:, :, pick].contiguous()
    _dress(head, C, pp)
    prob = preds["all_cls_scores"][1:].mean(0).sigmoid()[0].reshape(-1)
    kth = prob.topk(50).values[-1]
    assert int((prob >= kth).sum()) > 50 and torch.unique(prob).numel() <= 15         # the cut runs through a group of equal scores
    _assert_same(head.get_bboxes_batched(preds, None), head.get_bboxes(preds, None))


def test_num_thr_with_distinct_scores(cuda, head):
    preds = _preds(cuda, 2, 60, 4, 7, seed=5, spread=1.5)
    _dress(head, 4, dict(type="nms", nms_thr=0.5, num_thr=10), max_num=80)
    ref = _reference(head, preds)                                         # asserts the pairwise distinct scores
    cnt = _assert_same(head.get_bboxes_batched(preds, None), ref)
    assert cnt == [10, 10]


@pytest.mark.parametrize("pp", [None, dict(type="nms", nms_thr=0.2, score_thr=0.1)], ids=["none", "nms"])
def test_edge_shapes_one_scene_k_is_all_entries_and_coder_threshold(cuda, head, pp):
    """B=1; Q*C = 30 < max_num = 50, so K = 30; score_threshold set on the coder."""
    preds = _preds(cuda, 1, 10, 3, 7, seed=2, spread=1.0)
    _dress(head, 3, pp, max_num=50, score_threshold=0.3)
    det = head.get_bboxes_batched(preds, None)
    assert det.scores.shape == (1, 30)
    cnt = _assert_same(det, _reference(head, preds))
    assert 0 < cnt[0] < 30


@pytest.mark.parametrize("n", [63, 64, 65, 129, 600, 2100])
def test_one_crowded_class(cuda, head, n):
    """C=2: n candidates of label 0 in a tight cluster (long suppression chains), 5 of label 1.  n = 2100 is a segment above the
    2048 rows whose BEV boxes the NMS workgroup keeps in LDS; the small sizes sit around the 64-lane wave."""
    Q = n + 5
    preds = _preds(cuda, 1, Q, 2, 7, seed=n, spread=1.0)
    cls = preds["all_cls_scores"]
    cls[..., 0] = cls[..., 0] * 0.5 + 2.0
    cls[..., 1] = cls[..., 1] * 0.5 - 6.0
    cls[:, :, n:, 0] -= 8.0
    cls[:, :, n:, 1] += 8.0
    _dress(head, 2, dict(type="nms", nms_thr=0.2), max_num=Q, post_range=[-100.0] * 3 + [100.0] * 3)
    ref = head.get_bboxes(preds, None)
    dec = head.bbox_coder.decode(preds)[0]["labels"]
    assert int((dec == 0).sum()) == n and int((dec == 1).sum()) == 5
    cnt = _assert_same(head.get_bboxes_batched(preds, None), ref)
    assert 1 < cnt[0] < n                                                 # the cluster is thinned out


def test_k_5000_the_largest_lds_sort(cuda, head):
    preds = _preds(cuda, 2, 300, 18, 7, seed=9, spread=1.5)
    _dress(head, 18, None, max_num=5000)
    det = head.get_bboxes_batched(preds, None)
    assert det.scores.shape == (2, 5000)
    _assert_same(det, head.get_bboxes(preds, None))
    with pytest.raises(nv.U3DError):                                     # above 8192: an error, not a silent cut
        _dress(head, 18, None, max_num=8193).get_bboxes_batched(_preds(cuda, 1, 500, 18, 7, seed=1), None)


@pytest.mark.parametrize("pp", [dict(type="soft_nms", gaussian_sigma=0.3, prune_threshold=1e-3),
                                dict(type="box_merging", score_thr=[0.1, 0.05, 0.05], num_thr=500)], ids=["soft_nms", "box_merging"])
def test_per_scene_modes_through_get_bboxes_batched(cuda, head, pp):
    preds = _preds(cuda, 2, 60, 3, 7, seed=4, spread=1.0)
    _dress(head, 3, pp, max_num=100)
    cnt = _assert_same(head.get_bboxes_batched(preds, None), _reference(head, preds))
    assert min(cnt) > 0


def test_rows_past_count_are_zero_and_two_calls_give_the_same_bytes(cuda, head):
    preds = _preds(cuda, 3, 40, 3, 9, seed=6)
    _dress(head, 3, dict(type="nms", nms_thr=0.2, score_thr=0.1, num_thr=10))
    a = head.get_bboxes_batched(preds, None)
    junk = torch.full((1 << 16,), float("nan"), device=cuda)              # whatever the allocator hands out next is not zero
    del junk
    b = head.get_bboxes_batched(preds, None)
    for k in ("boxes", "scores", "labels", "count", "off"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    _assert_same(a, _reference(head, preds))                              # includes the zero rows
    bx, sc, lb, off = a.packed()
    cat = [torch.cat([r[i] for r in a.to_list()]) for i in range(3)]
    assert torch.equal(bx, cat[0]) and torch.equal(sc, cat[1]) and torch.equal(lb.long(), cat[2]) and off is a.off


@pytest.mark.parametrize("mode", ["none", "nms"])
def test_non_contiguous_inputs(cuda, head, mode):
    """native.det_tail takes views: prob and fused transposed (two copies of one size, made one after the other), boxes a column
    slice, center_range and score_thr strided.  Every copy it makes must live until the launch."""
    pp = None if mode == "none" else dict(type="nms", nms_thr=0.2, score_thr=[0.05, 0.2, 0.12], num_thr=10)
    preds = _preds(cuda, 3, 40, 3, 9, seed=21)
    _dress(head, 3, pp)
    ref = _reference(head, preds)
    coder = head.bbox_coder
    prob, fused, boxes, rng = coder.batched_prelude(preds)
    prob_v = prob.transpose(1, 2).contiguous().transpose(1, 2)
    fused_v = fused.transpose(1, 2).contiguous().transpose(1, 2)
    boxes_v = torch.cat([boxes, boxes.new_full((3, 40, 2), 7.0)], -1)[..., :9]
    rng_v = torch.stack([rng, rng + 1.0], 1)[:, 0]
    thr_v = None if pp is None else torch.tensor([[0.05, 9.0], [0.2, 9.0], [0.12, 9.0]], device=cuda)[:, 0]
    for t in (prob_v, fused_v, boxes_v, rng_v) + (() if thr_v is None else (thr_v,)):
        assert not t.is_contiguous()
    assert torch.equal(prob_v, prob) and torch.equal(fused_v, fused) and torch.equal(boxes_v, boxes)
    if pp is None:
        det = nv.det_tail(prob_v, fused_v, boxes_v, coder.max_num, rng_v, coder.score_threshold, mode=nv.DET_TAIL_NONE)
    else:
        det = nv.det_tail(prob_v, fused_v, boxes_v, coder.max_num, rng_v, coder.score_threshold, mode=nv.DET_TAIL_NMS, nms_thr=0.2,
                          score_thr=thr_v, num_thr=10)
    cnt = _assert_same(det, ref)
    assert min(cnt[:2]) > 0


def test_library_refuses_large_k_and_a_short_workspace(cuda):
    """The C side of the limits, behind the guard of native.det_tail: K = 8193 is U3D_ERR_UNSUPPORTED, a workspace one byte short is
    U3D_ERR_WORKSPACE.  Both return before any launch; every buffer has its full size all the same."""
    UNSUPPORTED, WORKSPACE = -2, -4

    def call(B, Q, C, max_num, short):
        K = min(max_num, Q * C)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=cuda)
        rng = torch.tensor([-1.0] * 3 + [1.0] * 3, device=cuda)
        wsb = int(nv.lib().u3d_det_tail_workspace(B, Q, C, max_num, 7))
        assert wsb > 0
        ws = torch.zeros((wsb,), dtype=torch.uint8, device=cuda)
        t = [f32(B, Q, C), f32(B, Q, C), f32(B, Q, 7), rng, f32(B, K, 7), f32(B, K), i32(B, K), i32(B), i32(B + 1), ws]
        p = [nv._ptr(x) for x in t]
        rc = nv.lib().u3d_det_tail(p[0], p[1], p[2], B, Q, C, 7, max_num, p[3], 0.0, nv.DET_TAIL_NMS, 0.2, None, 0, p[4], p[5], p[6],
                                   p[7], p[8], p[9], wsb - short, nv._stream())
        torch.cuda.synchronize()
        return rc

    assert call(1, 500, 18, 8193, 0) == UNSUPPORTED
    assert call(1, 500, 18, 8192, 0) == 0                                 # the largest K is served
    assert call(3, 40, 3, 50, 1) == WORKSPACE
    assert call(3, 40, 3, 50, 0) == 0


def _replay_head(model, monkeypatch):
    """The forward is not bitwise reproducible from run to run, and these tests are about the tail: the head's outputs of the first
    call are kept and served again to the second."""
    kept = []
    orig = model.pts_bbox_head.forward
    monkeypatch.setattr(model.pts_bbox_head, "forward", lambda *a, **k: kept.append(orig(*a, **k)) or kept[-1])

    def replay():
        it = iter(kept)
        monkeypatch.setattr(model.pts_bbox_head, "forward", lambda *a, **k: next(it))
    return replay


def test_simple_test_batched_equals_simple_test(cuda, monkeypatch):
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    from uni3detr_amd.registry import build_model
    from uni3detr_amd.synth import room_scene
    torch.manual_seed(1)
    model = build_model(copy.deepcopy(MODEL_CFG)).to(cuda).eval()
    pts = [torch.from_numpy(room_scene(i, 12000 - 1000 * i)[0]).to(cuda) for i in range(2)]
    replay = _replay_head(model, monkeypatch)
    ref = model.simple_test(None, pts)
    replay()
    got = model.simple_test_batched(None, pts)
    assert len(got) == len(ref) == 2
    for g, r in zip(got, ref):
        assert set(g) == set(r) == {"boxes_3d", "scores_3d", "labels_3d"} and r["scores_3d"].numel() > 0
        for k in r:
            assert not g[k].is_cuda and g[k].dtype == r[k].dtype and torch.equal(g[k], r[k]), k
    replay()
    det = model.simple_test_batched(None, pts, on_device=True)
    assert det.boxes.is_cuda and det.count.cpu().tolist() == [r["scores_3d"].numel() for r in ref]
    assert det.off.cpu().tolist() == [0] + np.cumsum(det.count.cpu().numpy()).tolist()


SHIPPED = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")


@pytest.mark.parametrize("name,npts", [("kitti_3classes", 16000), ("nuscenes", 30000)])
def test_aug_test_batched_tail_equals_aug_test(cuda, name, npts, monkeypatch):
    """The input of tests/test_tta_gpu.py::test_aug_test_end_to_end: two samples, double-flip views (A = 4)."""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.registry import build_model, to_config
    from uni3detr_amd.synth import room_scene
    cfg = to_config(ast.literal_eval(open(SHIPPED).read())[name]["config"]["model"])
    model = build_model(cfg).to(cuda).eval()
    pc = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    nfeat = cfg["pts_middle_encoder"]["in_channels"]
    raw = []
    for i in range(2):
        p = room_scene(i, npts - 1000 * i, pc_range=pc)[0]
        if nfeat > 4:
            p = np.concatenate([p, np.zeros((p.shape[0], nfeat - 4), np.float32)], 1)
        raw.append(torch.from_numpy(p).to(cuda))
    inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=list(pc))]
    pipe = dp.DevicePipeline([dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True,
                                   pcd_vertical_flip=True, transforms=inner)])
    points, metas = dp.tta_forward_inputs(pipe(dp.pack_batch(raw, box_type_3d="LiDAR")))
    assert len(points) == 4
    replay = _replay_head(model, monkeypatch)
    ref = model.aug_test(points, metas)
    replay()
    got = model.aug_test(points, metas, batched_tail=True)
    assert len(got) == len(ref) == 2 and sum(r["scores_3d"].numel() for r in ref) > 0
    for g, r in zip(got, ref):
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert g[k].dtype == r[k].dtype and torch.equal(g[k], r[k]), k
