"""The soft-NMS and box-merging modes of the batched inference tail (csrc/det_tail.hip: u3d_det_tail_pp, modes U3D_DET_TAIL_SOFT_NMS /
_MERGE behind Uni3DETRHead.get_bboxes_batched) against the per-scene path they replace: Uni3DETRHead.get_bboxes with u3d_soft_nms /
u3d_box_merge.  Every comparison is per scene and bit for bit - torch.equal on boxes, scores and labels, and the count -: both sides
run the same arithmetic on the same device, so there is no tolerance."""
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
WIDE = [-100.0] * 3 + [100.0] * 3
SOFT = dict(type="soft_nms", gaussian_sigma=0.3, prune_threshold=1e-3)
MERGE = dict(type="box_merging")
KITTI_THR = [0.0, 0.3, 0.65]


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


def _plain(head, preds, pp):
    """The per-scene result of the bare post-processing type (no score_thr / num_thr) and the coder's output it started from."""
    keep = head.post_processing
    head.post_processing = {k: v for k, v in pp.items() if k not in ("score_thr", "num_thr")}
    ref = head.get_bboxes(preds, None)
    head.post_processing = keep
    return ref, head.bbox_coder.decode(preds)


def _shows_its_effect(head, preds, pp):
    """An input on which nothing merges or decays proves nothing."""
    ref, dec = _plain(head, preds, pp)
    if pp["type"] == "box_merging":     # fewer boxes than the coder emitted, in at least one scene
        return any(r[0].shape[0] < d["scores"].numel() for r, d in zip(ref, dec))
    # soft_nms: a reported score that is not one of the scene's fused scores
    return any(bool((~torch.isin(r[1], d["scores"])).any()) for r, d in zip(ref, dec))


# ---- 1 ----
@pytest.mark.parametrize("pp", [dict(MERGE, score_thr=[0.1, 0.05, 0.05]), dict(SOFT, score_thr=0.05)], ids=["box_merging", "soft_nms"])
def test_no_per_scene_work_and_no_sync(cuda, head, pp, monkeypatch):
    """_post_process_scene must not run and nothing may synchronise.  The first call fills the two value-keyed device caches
    (centre range, score_thr: one host-to-device copy per setting); the second runs under the sync debug mode."""
    preds = _preds(cuda, 2, 60, 3, 7, seed=4, spread=1.0)
    _dress(head, 3, pp, max_num=100)
    ref = _reference(head, preds)
    assert _shows_its_effect(head, preds, pp)

    def boom(*a, **k):
        raise AssertionError("the per-scene routine ran")
    monkeypatch.setattr(head, "_post_process_scene", boom)
    head.get_bboxes_batched(preds, None)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        det = head.get_bboxes_batched(preds, None)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    cnt = _assert_same(det, ref)
    assert min(cnt) > 0


# ---- 2 ----
VARIANTS = {"none": {}, "score_thr": dict(score_thr=0.12), "per_class": dict(score_thr=[0.05, 0.2, 0.12]), "num_thr": dict(num_thr=10),
            "kitti": dict(score_thr=KITTI_THR)}
SMALL = [(t, v) for t in ("box_merging", "soft_nms") for v in ("none", "score_thr", "per_class", "num_thr")] + [("box_merging", "kitti")]


@pytest.mark.parametrize("dim,Q", [(7, 40), (9, 57)])
@pytest.mark.parametrize("kind,variant", SMALL, ids=[f"{t}-{v}" for t, v in SMALL])
def test_small_random_heads(cuda, head, dim, Q, kind, variant):
    """B=3, C=3, max_num=50; some candidates beyond post_center_range."""
    pp = dict(MERGE if kind == "box_merging" else SOFT, **VARIANTS[variant])
    preds = _preds(cuda, 3, Q, 3, dim, seed=30 + dim, spread=1.5)
    _dress(head, 3, pp)
    assert _shows_its_effect(head, preds, pp)
    cnt = _assert_same(head.get_bboxes_batched(preds, None), _reference(head, preds))
    assert min(cnt) > 0
    if variant == "num_thr":
        assert max(cnt) == 10


# ---- 3 ----
CROWD = [1, 2, 63, 64, 65, 129, 600, 2100]


def _crowd(dev, n):
    """C=2: n candidates of label 0 in a tight cluster, 5 of label 1 (the construction of the NMS test of the same name)."""
    Q = n + 5
    preds = _preds(dev, 1, Q, 2, 7, seed=n, spread=1.0)
    cls = preds["all_cls_scores"]
    cls[..., 0] = cls[..., 0] * 0.5 + 2.0
    cls[..., 1] = cls[..., 1] * 0.5 - 6.0
    cls[:, :, n:, 0] -= 8.0
    cls[:, :, n:, 1] += 8.0
    return preds, Q


@pytest.fixture(scope="module")
def crowd_merge(cuda, head):
    """The per-scene box_merging result of every crowd size, computed once, with what it shows about the medians: `changed` - a kept
    box whose first 7 columns are not its own; `odd` - one whose merged x is an input x other than its own (an odd count: the middle
    value); `even` - one whose merged x is no input x (an even count: the mean of two different middle values)."""
    out = {}
    for n in CROWD:
        preds, Q = _crowd(cuda, n)
        _dress(head, 2, dict(MERGE), max_num=Q, post_range=WIDE)
        ref = head.get_bboxes(preds, None)
        dec = head.bbox_coder.decode(preds)[0]
        assert int((dec["labels"] == 0).sum()) == n and int((dec["labels"] == 1).sum()) == 5
        own = dec["bboxes"].clone()
        own[:, 2] = own[:, 2] - own[:, 5] * 0.5
        order = torch.argsort(-dec["scores"], stable=True)
        ssort = dec["scores"][order]
        assert torch.unique(ssort).numel() == ssort.numel()              # distinct fused scores: a kept box is known by its score
        b = ref[0][0]
        src = own[order][torch.isin(ssort, ref[0][1])]                   # the kept boxes before merging, in the output's order
        assert src.shape == b.shape
        moved = (b[:, :7] != src[:, :7]).any(1)
        is_input = torch.isin(b[:, 0], own[:, 0])
        flags = dict(changed=bool(moved.any()), odd=bool((moved & is_input & (b[:, 0] != src[:, 0])).any()),
                     even=bool((moved & ~is_input).any()))
        out[n] = (preds, Q, ref, flags)
    return out


@pytest.mark.parametrize("n", CROWD)
def test_one_crowded_class_merge(cuda, head, crowd_merge, n):
    """n = 2100 is a segment above the 2048 rows (U3D_DET_TAIL_LDS_CAP) whose boxes the merge workgroup keeps in LDS; the small sizes
    sit around the 64-lane wave and the 256-thread tile of the sweep."""
    preds, Q, ref, _ = crowd_merge[n]
    _dress(head, 2, dict(MERGE), max_num=Q, post_range=WIDE)
    cnt = _assert_same(head.get_bboxes_batched(preds, None), ref)
    if n >= 63:
        assert 1 < cnt[0] < Q                                             # the cluster is thinned out


def test_crowded_merges_run_both_median_branches(crowd_merge):
    flags = [f for _, _, _, f in crowd_merge.values()]
    assert any(f["changed"] for f in flags) and any(f["odd"] for f in flags) and any(f["even"] for f in flags)


@pytest.mark.parametrize("n", CROWD)
def test_one_crowded_class_soft_nms(cuda, head, n):
    """n = 2100: above the 2048 rows a soft-NMS workgroup keeps in LDS, below u3d_soft_nms' own limit of 7680 candidates."""
    preds, Q = _crowd(cuda, n)
    _dress(head, 2, dict(SOFT), max_num=Q, post_range=WIDE)
    ref = head.get_bboxes(preds, None)
    cnt = _assert_same(head.get_bboxes_batched(preds, None), ref)
    assert cnt[0] >= 6
    if n >= 63:
        assert _shows_its_effect(head, preds, dict(SOFT))


# ---- 4 ----
def _hand_preds(dev, codes, logits, iou_logit, L=3):
    """One scene from explicit box codes [Q, 8|10] and class logits [Q, C]; every layer alike, so the layer mean is the value."""
    codes = torch.tensor(codes, dtype=torch.float32)
    logits = torch.tensor(logits, dtype=torch.float32)
    Q = codes.shape[0]
    iou = torch.tensor(iou_logit, dtype=torch.float32).reshape(Q, 1)
    rep = lambda t: t[None, None].repeat(L, 1, 1, 1).to(dev)
    return dict(all_cls_scores=rep(logits), all_bbox_preds=rep(codes), all_iou_preds=rep(iou))


@pytest.mark.parametrize("nbox", [4, 5, 6])
def test_median_ties_rank_by_position(cuda, head, nbox):
    """Same-label boxes that share a centre and a yaw and differ in z, dz and the sign of a zero x: the best one absorbs the rest
    (an even and an odd count), whole columns hold equal values - among them +0 and -0, which only the rank by position tells
    apart - and columns 7-8 come from the kept box."""
    cx = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    cz = [0.0, 0.1, 0.1, 0.0, 0.2, 0.1]
    lh = [0.0, 0.1, 0.0, 0.1, 0.1, 0.0]
    codes = [[cx[i], 0.25, 0.0, 0.0, cz[i], lh[i], 0.0, 1.0, 1.0 + i, -2.0 - i] for i in range(nbox)]
    logits = [[2.0 - 0.25 * i, -9.0] for i in range(nbox)]
    preds = _hand_preds(cuda, codes, logits, [0.5] * nbox)         # one IoU logit: box 0, the best class score, is kept
    _dress(head, 2, dict(MERGE), max_num=nbox, post_range=WIDE)
    ref = head.get_bboxes(preds, None)
    dec = head.bbox_coder.decode(preds)[0]
    assert dec["labels"].tolist() == [0] * nbox
    top = dec["bboxes"][torch.argmax(dec["scores"])]
    assert ref[0][0].shape == (1, 9) and torch.equal(ref[0][0][0, 7:], top[7:])      # one box, its own columns 7-8
    assert ref[0][0][0, 2] != top[2] - top[5] * 0.5                                     # ... and a median that is not its own z
    _assert_same(head.get_bboxes_batched(preds, None), ref)


# ---- 5 ----
@pytest.mark.parametrize("pp", [dict(MERGE), dict(SOFT)], ids=["box_merging", "soft_nms"])
def test_empty_and_single_candidate_segments(cuda, head, pp):
    """B=3, C=4: the middle scene lies outside post_center_range (count 0); label 3 has no candidate anywhere, label 1 exactly one."""
    B, Q, C = 3, 40, 4
    preds = _preds(cuda, B, Q, C, 9, seed=8, spread=1.5)
    cls = preds["all_cls_scores"]
    cls[..., 3] = -20.0
    cls[..., 1] = -20.0
    cls[:, :, 7, 1] = 5.0
    preds["all_bbox_preds"][:, :, 7, :2] = 0.0
    preds["all_bbox_preds"][:, :, 7, 4] = 0.0
    preds["all_bbox_preds"][:, 1, :, 0] += 1000.0
    _dress(head, C, pp)
    for b, d in enumerate(head.bbox_coder.decode(preds)):
        lab = d["labels"]
        assert lab.numel() == 0 if b == 1 else (int((lab == 1).sum()) == 1 and int((lab == 3).sum()) == 0 and int((lab == 0).sum()) > 1)
    cnt = _assert_same(head.get_bboxes_batched(preds, None), head.get_bboxes(preds, None))
    assert cnt[1] == 0 and cnt[0] > 0 and cnt[2] > 0


# ---- 6 ----
@pytest.mark.parametrize("pp", [dict(MERGE, score_thr=KITTI_THR, num_thr=10), dict(SOFT, score_thr=0.1, num_thr=10)],
                         ids=["box_merging", "soft_nms"])
def test_rows_past_count_are_zero_and_two_calls_give_the_same_bytes(cuda, head, pp):
    preds = _preds(cuda, 3, 40, 3, 9, seed=6, spread=1.5)
    _dress(head, 3, pp)
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


# ---- 7 ----
@pytest.mark.parametrize("kind", ["box_merging", "soft_nms"])
def test_non_contiguous_inputs(cuda, head, kind):
    """native.det_tail takes views: prob and fused transposed (two copies of one size, made one after the other), boxes a column
    slice, center_range and score_thr strided.  Every copy it makes must live until the launch."""
    pp = dict(MERGE if kind == "box_merging" else SOFT, score_thr=[0.05, 0.2, 0.12], num_thr=10)
    preds = _preds(cuda, 3, 40, 3, 9, seed=21, spread=1.5)
    _dress(head, 3, pp)
    ref = _reference(head, preds)
    coder = head.bbox_coder
    prob, fused, boxes, rng = coder.batched_prelude(preds)
    prob_v = prob.transpose(1, 2).contiguous().transpose(1, 2)
    fused_v = fused.transpose(1, 2).contiguous().transpose(1, 2)
    boxes_v = torch.cat([boxes, boxes.new_full((3, 40, 2), 7.0)], -1)[..., :9]
    rng_v = torch.stack([rng, rng + 1.0], 1)[:, 0]
    thr_v = torch.tensor([[0.05, 9.0], [0.2, 9.0], [0.12, 9.0]], device=cuda)[:, 0]
    for t in (prob_v, fused_v, boxes_v, rng_v, thr_v):
        assert not t.is_contiguous()
    assert torch.equal(prob_v, prob) and torch.equal(fused_v, fused) and torch.equal(boxes_v, boxes)
    if kind == "box_merging":
        det = nv.det_tail(prob_v, fused_v, boxes_v, coder.max_num, rng_v, coder.score_threshold, mode=nv.DET_TAIL_MERGE, nms_thr=0.1,
                          score_thr=thr_v, num_thr=10)
    else:
        det = nv.det_tail(prob_v, fused_v, boxes_v, coder.max_num, rng_v, coder.score_threshold, mode=nv.DET_TAIL_SOFT_NMS,
                          score_thr=thr_v, num_thr=10, soft_sigma=0.3, soft_prune=1e-3)
    cnt = _assert_same(det, ref)
    assert min(cnt) > 0


# ---- 8 ----
@pytest.mark.parametrize("mode", [3, 4], ids=["soft_nms", "box_merging"])
def test_library_refuses_large_k_and_a_short_workspace(cuda, mode):
    """The C side of the limits for the new modes: K = 8193 is U3D_ERR_UNSUPPORTED, a workspace one byte short of
    u3d_det_tail_pp_workspace(..., mode) is U3D_ERR_WORKSPACE.  Both return before any launch; every buffer has its full size all
    the same.  K = 8192 is served."""
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
    assert (nv.DET_TAIL_SOFT_NMS, nv.DET_TAIL_MERGE) == (3, 4)

    def call(B, Q, C, max_num, short, sigma=0.3):
        K = min(max_num, Q * C)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=cuda)
        rng = torch.tensor([-1.0] * 3 + [1.0] * 3, device=cuda)
        wsb = int(nv.lib().u3d_det_tail_pp_workspace(B, Q, C, max_num, 7, mode))
        assert wsb >= int(nv.lib().u3d_det_tail_workspace(B, Q, C, max_num, 7)) > 0
        ws = torch.zeros((wsb,), dtype=torch.uint8, device=cuda)
        t = [f32(B, Q, C), f32(B, Q, C), f32(B, Q, 7), rng, f32(B, K, 7), f32(B, K), i32(B, K), i32(B), i32(B + 1), ws]
        p = [nv._ptr(x) for x in t]
        rc = nv.lib().u3d_det_tail_pp(p[0], p[1], p[2], B, Q, C, 7, max_num, p[3], 0.0, mode, 0.1, None, 0, sigma, 1e-3, p[4], p[5],
                                      p[6], p[7], p[8], p[9], wsb - short, nv._stream())
        torch.cuda.synchronize()
        return rc

    assert call(1, 500, 18, 8193, 0) == UNSUPPORTED
    assert call(1, 500, 18, 8192, 0) == 0                                 # the largest K is served
    assert call(3, 40, 3, 50, 1) == WORKSPACE
    assert call(3, 40, 3, 50, 0) == 0
    if mode == nv.DET_TAIL_SOFT_NMS:
        assert call(3, 40, 3, 50, 0, sigma=0.0) == ARG


# ---- 9 ----
def _replay_head(model, monkeypatch):
    """The forward is not bitwise reproducible from run to run, and these tests are about the tail: the head's outputs of the first
    call are kept and served again to the later ones."""
    kept = []
    orig = model.pts_bbox_head.forward
    monkeypatch.setattr(model.pts_bbox_head, "forward", lambda *a, **k: kept.append(orig(*a, **k)) or kept[-1])

    def replay():
        it = iter(kept)
        monkeypatch.setattr(model.pts_bbox_head, "forward", lambda *a, **k: next(it))
    return replay


SHIPPED = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")


def test_kitti_simple_test_batched_equals_simple_test(cuda, monkeypatch):
    """The shipped kitti_3classes model (box_merging, max_num=150, per-class score_thr) on two small synthetic scenes."""
    from uni3detr_amd.registry import build_model, to_config
    from uni3detr_amd.synth import room_scene
    cfg = to_config(ast.literal_eval(open(SHIPPED).read())["kitti_3classes"]["config"]["model"])
    torch.manual_seed(1)
    model = build_model(cfg).to(cuda).eval()
    assert model.pts_bbox_head.post_processing["type"] == "box_merging"
    pc = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    nfeat = cfg["pts_middle_encoder"]["in_channels"]
    pts = []
    for i in range(2):
        p = room_scene(i, 16000 - 1000 * i, pc_range=pc)[0]
        if nfeat > 4:
            p = np.concatenate([p, np.zeros((p.shape[0], nfeat - 4), np.float32)], 1)
        pts.append(torch.from_numpy(p).to(cuda))
    replay = _replay_head(model, monkeypatch)
    ref = model.simple_test(None, pts)
    replay()
    got = model.simple_test_batched(None, pts)
    assert len(got) == len(ref) == 2 and sum(r["scores_3d"].numel() for r in ref) > 0
    for g, r in zip(got, ref):
        assert set(g) == set(r) == {"boxes_3d", "scores_3d", "labels_3d"}
        for k in r:
            assert not g[k].is_cuda and g[k].dtype == r[k].dtype and torch.equal(g[k], r[k]), k
    replay()
    det = model.simple_test_batched(None, pts, on_device=True)
    bx, sc, lb, off = det.packed()
    assert bx.is_cuda and off.cpu().tolist() == [0] + np.cumsum([r["scores_3d"].numel() for r in ref]).tolist()
    assert torch.equal(bx.cpu(), torch.cat([r["boxes_3d"] for r in ref]))
    assert torch.equal(sc.cpu(), torch.cat([r["scores_3d"] for r in ref]))
    assert torch.equal(lb.cpu().long(), torch.cat([r["labels_3d"] for r in ref]).long())
