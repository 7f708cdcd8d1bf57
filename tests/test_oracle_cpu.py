"""CPU: the oracle restatement (oracle/model.py, oracle/boxes.py, oracle/geometry.py) against
(1) golden vectors generated from the reference's own files (tests/golden/*.npz, oracle/make_golden.py) and
(2) self-checking properties for the un-vendored upstream ops (parity unpinned there)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import boxes as ob
from oracle import geometry as og
from oracle import model as om
from oracle.weights import seeded_input, seeded_tensor

G = os.path.join(os.path.dirname(__file__), "golden")


def load_head_fixture(name="head_train_b2.npz"):
    z = np.load(os.path.join(G, name), allow_pickle=False)
    return z


def head_state(z_train, seed):
    sd = {}
    for k, shp in zip(z_train["sd_names"], z_train["sd_shapes"]):
        shape = tuple(int(s) for s in str(shp).split(",")) if str(shp) else ()
        sd["pts_bbox_head." + str(k)] = seeded_tensor(str(k), shape, seed)
    return sd


def head_inputs(B, seed):
    feats = seeded_input("pts_feats", (B, 256, 15, 40, 40), seed, -0.5, 1.0).clamp_min(0)
    fps = seeded_input("fpsbpts", (B, 600, 3), seed, 0.0, 1.0)
    return feats, fps


def split_gts(z):
    gts, labels, o = [], [], 0
    for n in z["gt_lens"]:
        gts.append(torch.from_numpy(z["gts"][o:o + n]))
        labels.append(torch.from_numpy(z["labels"][o:o + n]))
        o += n
    return gts, labels


def test_small_ops_match_reference():
    z = np.load(os.path.join(G, "small_ops.npz"))
    tb = torch.from_numpy(z["boxes"])
    norm = om.normalize_bbox(tb)
    np.testing.assert_allclose(norm.numpy(), z["norm"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(om.denormalize_bbox(norm).numpy(), z["denorm"], rtol=1e-5, atol=1e-5)
    pred = torch.from_numpy(z["pred"])
    l1 = torch.cdist(pred, norm[:12, :8], p=1) * 0.25
    np.testing.assert_allclose(l1.numpy(), z["l1cost"], rtol=1e-5, atol=1e-5)
    iouc = (1 - ob.bbox_overlaps_nearest_3d(om.denormalize_bbox(pred), tb[:12])) * 1.2
    np.testing.assert_allclose(iouc.numpy(), z["ioucost"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(om.sine_embed(torch.from_numpy(z["pos"])).numpy(), z["sine"], rtol=1e-5, atol=1e-6)
    il = 1 - ob.bbox_overlaps_nearest_3d(tb[:32], tb[32:], is_aligned=True)
    np.testing.assert_allclose(il.numpy(), z["iou3d_loss"], rtol=1e-5, atol=1e-6)


def test_head_forward_and_loss_match_reference():
    z = load_head_fixture()
    cfg = om.sunrgbd_cfg()
    seed = int(z["seed"])
    sd = head_state(z, seed)
    feats, fps = head_inputs(2, seed)
    feats.requires_grad_(True)
    cls, box, iou = om.head_forward(sd, "pts_bbox_head.", feats, fps, cfg)
    for a, k in ((cls, "cls"), (box, "box"), (iou, "iou")):
        ref = torch.from_numpy(z[k])
        assert a.shape == ref.shape
        err = (a.detach() - ref).abs().max().item()
        assert err <= 1e-3 * max(1.0, ref.abs().max().item()) * 0.1, (k, err)
    gts, labels = split_gts(z)
    losses, assigned = om.head_loss(cls, box, iou, gts, labels, cfg)
    assert np.array_equal(assigned.numpy().astype(np.int16), z["assigned"])
    for name, val in zip(z["loss_names"], z["loss_values"]):
        assert abs(float(losses[str(name)]) - val) <= 1e-4 * max(1.0, abs(val)), name
    # the checker-only `assigned=` override (tests/test_grad_parity_gpu.py): fed the reference's own matching it is the identity
    with torch.no_grad():
        l2, a2 = om.head_loss(cls, box, iou, gts, labels, cfg, assigned=torch.from_numpy(z["assigned"].astype(np.int64)))
    assert torch.equal(a2, assigned) and all(float(l2[k]) == float(losses[k]) for k in losses)
    sum(losses.values()).backward()
    np.testing.assert_allclose(feats.grad.reshape(-1)[::997].numpy(), z["feats_grad_sub"], rtol=2e-3, atol=2e-5)
    assert abs(float(feats.grad.abs().sum()) - float(z["feats_grad_abs_sum"])) <= 1e-3 * float(z["feats_grad_abs_sum"])


def test_head_eval_layout_matches_reference():
    zt = load_head_fixture()
    z = np.load(os.path.join(G, "head_eval_b1.npz"))
    cfg = om.sunrgbd_cfg()
    sd = head_state(zt, int(z["seed"]))
    feats, fps = head_inputs(1, int(z["seed"]))
    with torch.no_grad():
        cls, box, iou = om.head_forward(sd, "pts_bbox_head.", feats, fps, cfg, rand_points=torch.from_numpy(z["rand_points"]))
    assert cls.shape == (3, 1, 1200, 10)
    for a, k in ((cls, "cls"), (box, "box"), (iou, "iou")):
        assert (a - torch.from_numpy(z[k])).abs().max().item() <= 1e-4 * max(1.0, float(np.abs(z[k]).max()))


# ---------------------------------------------------------------------------------------------------
# properties of the un-vendored ops (no reference vectors exist: SURVEY.md §4)
# ---------------------------------------------------------------------------------------------------
def test_rotated_iou_axis_aligned_closed_form_and_monte_carlo():
    rng = np.random.default_rng(0)
    b1 = torch.tensor([[0.0, 0, 0, 2, 1, 1, 0.0], [0, 0, 0, 2, 1, 1, math.pi / 2], [1, 1, 0.5, 2, 2, 2, 0.3]])
    b2 = torch.tensor([[0.5, 0.25, 0.5, 2, 1, 1, 0.0], [0, 0, 0, 1, 2, 1, 0.0], [1.2, 0.8, 0.0, 1.5, 2.5, 2, -0.9]])
    got = ob.bbox_overlaps_3d_aligned(b1, b2)
    inter0 = 1.5 * 0.75 * 0.5
    assert abs(got[0].item() - inter0 / (2 + 2 - inter0)) < 1e-6
    assert abs(got[1].item() - 1.0) < 1e-6        # (2x1 @ 90deg) == (1x2 @ 0deg)
    # Monte-Carlo for the generic pair
    pts = rng.uniform(-2, 4, (400000, 3))
    def inside(b, p):
        c, s = math.cos(b[6]), math.sin(b[6])
        dx, dy = p[:, 0] - b[0], p[:, 1] - b[1]
        lx, ly = dx * c + dy * s, -dx * s + dy * c
        return (np.abs(lx) <= b[3] / 2) & (np.abs(ly) <= b[4] / 2) & (p[:, 2] >= b[2]) & (p[:, 2] <= b[2] + b[5])
    i1, i2 = inside(b1[2].numpy(), pts), inside(b2[2].numpy(), pts)
    mc = (i1 & i2).sum() / max((i1 | i2).sum(), 1)
    assert abs(got[2].item() - mc) < 0.01


def test_sparse_conv_equals_masked_dense_conv():
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    dims = (8, 12, 12)
    cells = rng.choice(2 * 8 * 12 * 12, 300, replace=False)
    co = np.stack([cells // (8 * 144), cells // 144 % 8, cells // 12 % 12, cells % 12], 1).astype(np.int32)
    x = torch.randn(300, 5)
    w = torch.randn(27, 5, 7)
    # SubM: out set == in set
    y = og.sparse_conv(x, w, og.nbr_table(co, co, dims, (3, 3, 3), (1, 1, 1), (1, 1, 1), 0))
    dense = og.dense_conv_reference(x, co, dims, w, (3, 3, 3), (1, 1, 1), (1, 1, 1), 2)
    c = torch.from_numpy(co).long()
    assert (y - dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]).abs().max() < 1e-4
    # strided with asymmetric padding: active set = support of the dense conv of the indicator
    for pad in [(1, 1, 1), (0, 1, 1)]:
        oc, od = og.strided_out_coords(co, dims, (3, 3, 3), (2, 2, 2), pad)
        ys = og.sparse_conv(x, w, og.nbr_table(oc, co, dims, (3, 3, 3), (2, 2, 2), pad, 0))
        ds = og.dense_conv_reference(x, co, dims, w, (3, 3, 3), (2, 2, 2), pad, 2)
        assert tuple(ds.shape[2:]) == od
        o = torch.from_numpy(oc).long()
        assert (ys - ds[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]]).abs().max() < 1e-4
        ind = og.dense_conv_reference(torch.ones(300, 1), co, dims, torch.ones(27, 1, 1), (3, 3, 3), (2, 2, 2), pad, 2)[:, 0] > 0
        mask = torch.zeros_like(ind)
        mask[o[:, 0], o[:, 1], o[:, 2], o[:, 3]] = True
        assert torch.equal(mask, ind)


def test_voxelize_semantics_small():
    pts = np.array([[0.011, 0.0, -1.99, 1], [0.012, 0.001, -1.99, 2], [5.0, 0, 0, 3], [0.03, 0.0, -1.99, 4],
                    [0.013, 0.002, -1.985, 5]], np.float32)
    v, c, n = og.voxelize_hard(pts, (0.02,) * 3, (-3.2, -0.2, -2.0, 3.2, 6.2, 0.56), 2, 10)
    assert c.tolist() == [[0, 10, 160], [0, 10, 161]]
    assert n.tolist() == [2, 1]                     # third point of voxel 0 dropped (max_points=2), OOR point skipped
    assert v[0, 1, 3] == 2 and v[1, 0, 3] == 4
    v, c, n = og.voxelize_hard(pts, (0.02,) * 3, (-3.2, -0.2, -2.0, 3.2, 6.2, 0.56), 2, 1)
    assert c.shape[0] == 1 and n.tolist() == [2]    # voxel cap: later voxel never created, its point dropped


def test_fps_tie_rule_and_coverage():
    p = np.zeros((10, 3), np.float32)
    p[:, 0] = [0, 1, 1, 5, 5, 2, 2, 3, 3, 4]
    idx = om.fps_packed(p.reshape(-1), 10, 3)
    assert idx[0] == 0 and idx[1] == 3             # two maxima (3 and 4): T = 8, (3%8,3) < (4%8,4)
    q = np.random.default_rng(0).random((500, 3)).astype(np.float32)
    idx = om.fps_packed(q.reshape(-1), 500, 50)
    assert len(set(idx.tolist())) == 50


def test_merge_oracle_overlap_closed_forms():
    """oracle/postproc.py (restatement of core/bbox/bbox_merging.py; the file itself needs cv2 / shapely / numba and cannot be imported):
    the overlap of axis-aligned boxes has a closed form, a 90-degree yaw swaps the footprint extents, and the polygon clip is checked
    against a Monte-Carlo area on rotated pairs."""
    import numpy as np
    from oracle import postproc as pp
    # boxes are (x, y, z, l, h, w, yaw): footprint in (x, z) with extents (l, w), "height" interval [y - h, y]
    a = np.array([[0.0, 0.0, 0.0, 2.0, 1.0, 4.0, 0.0]])
    b = np.array([[1.0, -0.5, 1.0, 2.0, 1.0, 4.0, 0.0]])
    ca, cb = pp._corners(a), pp._corners(b)
    shared = (2.0 - 1.0) * (4.0 - 1.0)            # x overlap 1, z overlap 3
    inter = 0.5 * shared                           # shared height 0.5
    union = 1.0 * 8.0 + 1.0 * 8.0
    assert abs(pp._overlap(ca[0], cb)[0] - inter / (union - inter)) < 1e-6
    # yaw = pi/2: the footprint of b becomes 4 (x) by 2 (z)
    b2 = b.copy(); b2[0, 6] = np.pi / 2
    cb2 = pp._corners(b2)
    sx = min(1.0, 1.0 + 2.0) - max(-1.0, 1.0 - 2.0)      # a: x in [-1,1]; b2: x in [-1,3]
    sz = min(2.0, 1.0 + 1.0) - max(-2.0, 1.0 - 1.0)      # a: z in [-2,2]; b2: z in [0,2]
    inter = 0.5 * sx * sz
    assert abs(pp._overlap(ca[0], cb2)[0] - inter / (16.0 - inter)) < 1e-6
    # disjoint in height -> 0
    b3 = b.copy(); b3[0, 1] = 5.0
    assert pp._overlap(ca[0], pp._corners(b3))[0] == 0.0
    # rotated pair: polygon clip vs Monte-Carlo
    rng = np.random.default_rng(3)
    p = np.array([[0.2, 0, -0.1, 3.0, 1, 1.5, 0.7]]); q = np.array([[0.9, 0, 0.4, 2.0, 1, 2.5, -0.4]])
    P, Q = pp._corners(p)[0][:4][:, [0, 2]], pp._corners(q)[0][:4][:, [0, 2]]
    pts = rng.uniform(-4, 4, (400000, 2))
    def inside(poly, x):
        s = None
        for i in range(4):
            e, v = poly[(i + 1) % 4] - poly[i], x - poly[i]
            c = e[0] * v[:, 1] - e[1] * v[:, 0]
            s = (c >= 0) if s is None else (s & (c >= 0))
        return s
    def ccw(poly):
        return poly if _area2(poly) > 0 else poly[::-1]
    def _area2(poly):
        x, y = poly[:, 0], poly[:, 1]
        return np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))
    mc = (inside(ccw(P), pts) & inside(ccw(Q), pts)).mean() * 64.0
    assert abs(pp._convex_intersection_area(P, Q) - mc) < 0.03


def test_merge_oracle_median_and_sweep_order():
    """three overlapping same-class boxes + one of another class + a far one: the best-scored box absorbs the two overlapping ones and
    becomes their per-coordinate median; the other class and the far box survive untouched."""
    import numpy as np
    from oracle import postproc as pp
    boxes = np.array([[0.0, 0, 0, 2, 1, 4, 0.00], [0.1, 0, 0.1, 2.2, 1, 4.2, 0.02], [-0.1, 0, 0.2, 1.8, 1, 3.8, -0.02],
                      [0.0, 0, 0, 2, 1, 4, 0.0], [30.0, 0, 0, 2, 1, 4, 0.0]], np.float32)
    labels = np.array([1, 1, 1, 2, 1])
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    lab, bx, sc, idx, order = pp.merge_boxes(labels, boxes, scores, 0.1)
    assert idx.tolist() == [0, 3, 4] and lab.tolist() == [1, 2, 1]
    assert np.allclose(bx[0], np.median(boxes[:3], axis=0)) and np.allclose(bx[1], boxes[3]) and np.allclose(bx[2], boxes[4])


@pytest.mark.parametrize("name", ["kitti_3classes", "nuscenes"])
def test_oracle_head_matches_reference_golden_for_other_head_shapes(name):
    """oracle/model.py head_forward (+ head_loss) with the KITTI (9 decoder layers, 3 classes) and nuScenes (900 queries, code size 10)
    numbers against the reference head's own outputs (tests/golden/head_variants.npz, oracle/make_golden.py gen_head_variants)."""
    z = np.load(os.path.join(G, "head_variants.npz"))
    seed = int(z["seed"])
    cfg = om.kitti_cfg() if name == "kitti_3classes" else om.nuscenes_cfg()
    B, C, D, H, W, nq = (int(v) for v in z[name + "_shape"])
    L = z[name + "_cls"].shape[0]
    assert L == cfg["dec_layers"] and nq == cfg["num_query"] and z[name + "_box"].shape[-1] == cfg["code_size"]
    # state dict of the reference head: names / shapes follow from the layer count, class count and code size
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd.configs import variants
    from uni3detr_amd.registry import build_model
    head = build_model(getattr(variants, name)).pts_bbox_head
    sd = {"pts_bbox_head." + k: seeded_tensor(k, tuple(v.shape), seed) for k, v in head.state_dict().items()}
    feats = seeded_input(name + ".pts_feats", (B, C, D, H, W), seed, -0.5, 1.0).clamp_min(0)
    fps = seeded_input(name + ".fpsbpts", (B, 2 * nq, 3), seed, 0.0, 1.0)
    with torch.no_grad():
        cls, box, iou = om.head_forward(sd, "pts_bbox_head.", feats, fps, cfg)
    for got, key in ((cls, "_cls"), (box, "_box"), (iou, "_iou")):
        ref = z[name + key]
        assert got.shape == ref.shape and np.abs(got.numpy() - ref).max() <= 2e-4 * max(1.0, np.abs(ref).max()), key
    if name + "_loss_values" in z:
        gts, labels, o = [], [], 0
        for n in z[name + "_gt_lens"]:
            gts.append(torch.from_numpy(z[name + "_gts"][o:o + n])); labels.append(torch.from_numpy(z[name + "_labels"][o:o + n])); o += n
        with torch.no_grad():
            losses, _ = om.head_loss(cls, box, iou, gts, labels, cfg)
        for k, v in zip(z[name + "_loss_names"], z[name + "_loss_values"]):
            assert abs(float(losses[str(k)]) - v) <= 1e-4 * max(1.0, abs(v)), (k, float(losses[str(k)]), v)


# ---------------------------------------------------------------------------------------------------------------------------
# data-path oracle: pinned to what transform_3d.py writes out itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_datapath_oracle_matches_the_matrices_the_reference_writes():
    """ref transform_3d.py:380-383 (rot_mat_T, mmdet3d >= 1.0 branch), :429-431 (uni_scale_mat), :571-580 (flip_mat), :461-464 and
    :564-567 (composition): for LiDAR coordinates the augmented xyz is xyz @ uni_rot_aug."""
    from oracle import datapath as od
    rng = np.random.default_rng(0)
    p = rng.normal(size=(200, 4)).astype(np.float32)
    a = 0.3
    assert np.allclose(od.rot_mat_T(a), [[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]], atol=1e-7)
    assert np.array_equal(od.flip_mat(True, False), np.diag([1, -1, 1]).astype(np.float32))
    assert np.array_equal(od.flip_mat(False, True), np.diag([-1, 1, 1]).astype(np.float32))
    for fh, fv, ang, sc in [(0, 0, 0.3, 1.1), (1, 0, -0.4, 0.9), (0, 1, 0.2, 1.0), (1, 1, 0.5236, 1.15)]:
        got = od.augment_points(p, fh, fv, ang, sc, od.LIDAR, 3)
        assert np.allclose(got[:, :3], p[:, :3] @ od.uni_rot_aug(fh, fv, ang, sc), atol=2e-6)
        assert np.allclose(got[:, 3], p[:, 3] * np.float32(sc))            # shift_height: the height attribute scales


def _bev_corners(b):
    c, s = np.cos(b[6]), np.sin(b[6])
    out = []
    for sx, sy in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        x, y = sx * b[3], sy * b[4]
        out.append((b[0] + x * c - y * s, b[1] + x * s + y * c))
    return np.array(sorted(out))


def test_datapath_oracle_boxes_move_with_their_corner_points():
    """Self-consistency that fixes the yaw conventions: the BEV corners of the augmented box are the augmented corners of the box
    (as a set: a mirror reverses their order), in both coordinate systems, for every flip combination."""
    from oracle import datapath as od
    rng = np.random.default_rng(1)
    for coord in (od.DEPTH, od.LIDAR):
        for fh in (0, 1):
            for fv in (0, 1):
                b = np.array([[1.0, -2.0, 0.3, 2.0, 0.8, 1.1, 0.7]], np.float32)
                ang, sc = float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.85, 1.15))
                nb = od.augment_boxes(b, fh, fv, ang, sc, coord)[0]
                corners = _bev_corners(b[0])
                pts = np.concatenate([corners, np.zeros((4, 1))], 1).astype(np.float32)
                moved = od.augment_points(pts, fh, fv, ang, sc, coord)[:, :2]
                assert np.allclose(_bev_corners(nb), np.array(sorted(map(tuple, moved))), atol=1e-5), (coord, fh, fv)
                assert np.allclose(nb[3:6], b[0, 3:6] * np.float32(sc)) and np.isclose(nb[2], b[0, 2] * np.float32(sc))


def test_datapath_oracle_filter_and_sample():
    from oracle import datapath as od
    p = np.array([[0, 0, 0, 1], [-3.2, 0, 0, 2], [1, 1, 0.56, 3], [1, 1, 0.5, 4], [np.nan, 0, 0, 5]], np.float32)
    kept = od.range_filter(p, [-3.2, -0.2, -2.0, 3.2, 6.2, 0.56])
    assert kept[:, 3].tolist() == [1.0, 4.0]                                # strict bounds, NaN dropped, order kept
    rng = np.random.default_rng(0)
    s, idx = od.point_sample(kept, 5, rng)
    assert s.shape == (5, 4) and set(idx) <= {0, 1}                         # n < num_points: with replacement
    s, idx = od.point_sample(np.arange(40, dtype=np.float32).reshape(10, 4), 6, rng)
    assert len(set(idx)) == 6                                               # n >= num_points: without replacement


# ==================================================================================================
# round 6: the reference-held math that was restated but not pinned (SECOND3D / SECOND3DFPN, SparseEncoderHD wiring,
# shift_scale_points) against goldens produced by the reference's own files (oracle/make_golden.py gen_dense_stack /
# gen_encoder_wiring / gen_detector_glue)
# ==================================================================================================
ORACLE_CFG = {"sunrgbd": om.sunrgbd_cfg, "kitti_3classes": om.kitti_cfg, "scannet_large": om.scannet_large_cfg, "nuscenes": om.nuscenes_cfg}


def _seeded_sd(prefix, keys, shapes, seed):
    """The generator seeds each reference module's tensors by its OWN (unprefixed) key."""
    return {prefix + str(k): seeded_tensor(str(k), eval(str(s)), seed) for k, s in zip(keys, shapes)}     # noqa: S307 (repr of an int tuple)


def dense_stack_fixture(name):
    z = np.load(os.path.join(G, "dense_stack.npz"), allow_pickle=False)
    seed = int(z["seed"])
    sd = _seeded_sd("pts_backbone.", z[f"{name}.backbone_keys"], z[f"{name}.backbone_shapes"], seed)
    sd.update(_seeded_sd("pts_neck.", z[f"{name}.neck_keys"], z[f"{name}.neck_shapes"], seed))
    return z, sd


@pytest.fixture
def four_cpu_threads():
    """torch's CPU kernels pick their summation order by thread count: oneDNN's single-thread FPN deconvolutions round the neck output
    differently from the multi-thread ones the fixture was generated with (2-8 threads reproduce it bit for bit).  Pinned for the test."""
    old = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(old)


@pytest.mark.parametrize("name", ["sunrgbd", "scannet_large"])
def test_dense_stack_oracle_matches_reference_golden(name, four_cpu_threads):
    """ref models/backbones/second_3d.py:52-76,89-114 + models/necks/second3d_fpn.py:48-104,112-143, training-mode BatchNorm."""
    z, sd = dense_stack_fixture(name)
    cfg = ORACLE_CFG[name]()
    leaf = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    x = torch.from_numpy(z[f"{name}.x"]).requires_grad_(True)
    outs = om.second3d(leaf, "pts_backbone.", x, cfg)
    y = om.second3dfpn(leaf, "pts_neck.", outs, cfg)
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().numpy(), z[f"{name}.backbone{i}"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(y.detach().numpy(), z[f"{name}.neck"], rtol=1e-5, atol=1e-6)
    (y * torch.from_numpy(z[f"{name}.cot"])).sum().backward()
    scale = float(np.abs(z[f"{name}.dx"]).max())
    np.testing.assert_allclose(x.grad.numpy(), z[f"{name}.dx"], rtol=1e-4, atol=1e-5 * scale)
    got = np.concatenate([leaf[str(k)].grad.numpy().reshape(-1) for k in z[f"{name}.bn_grad_keys"]])
    np.testing.assert_allclose(got, z[f"{name}.bn_grads"], rtol=1e-4, atol=1e-5 * float(np.abs(z[f"{name}.bn_grads"]).max()))
    w0 = leaf["pts_backbone.blocks.0.0.weight"].grad[:8].numpy()
    np.testing.assert_allclose(w0, z[f"{name}.wgrad_first_8"], rtol=1e-4, atol=1e-5 * float(np.abs(w0).max()))
    wd = leaf["pts_neck.deblocks.2.0.weight"].grad[:, :4].numpy()
    np.testing.assert_allclose(wd, z[f"{name}.wgrad_deconv2_4"], rtol=1e-4, atol=1e-5 * float(np.abs(wd).max()))


def test_dense_stack_aliases_and_state_dict_names():
    """KITTI / nuScenes ship the SAME pts_backbone / pts_neck dicts as SUN RGB-D (recorded by the generator, mirrored by the oracle's
    configs); the product's modules carry the reference's parameter names and shapes."""
    z = np.load(os.path.join(G, "dense_stack.npz"), allow_pickle=False)
    keys = ("bb_in", "bb_out", "bb_layers", "bb_strides", "bb_kernel", "fpn_in", "fpn_out", "fpn_strides", "fpn_extra", "bn_eps")
    for alias in ("kitti_3classes", "nuscenes"):
        assert str(z[f"{alias}.same_as"]) == "sunrgbd"
        assert all(ORACLE_CFG[alias]()[k] == om.sunrgbd_cfg()[k] for k in keys)
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd.configs.sunrgbd import model as mine
    from uni3detr_amd.registry import build_model
    m = build_model(mine)
    for mod, pre in ((m.pts_backbone, "backbone"), (m.pts_neck, "neck")):
        ref = {str(k): eval(str(s)) for k, s in zip(z[f"sunrgbd.{pre}_keys"], z[f"sunrgbd.{pre}_shapes"])}     # noqa: S307
        assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == ref


def _expected_trace(cfg, shape):
    """The sparse-conv call sequence oracle.model.sparse_encoder performs, from its config numbers (the restatement's wiring)."""
    k3 = (3, 3, 3)
    rows = [("SubMConv3d", cfg["enc_in"], cfg["enc_base"], k3, (1, 1, 1))]
    c = cfg["enc_base"]
    last = len(cfg["encoder_channels"]) - 1
    for i, blocks in enumerate(cfg["encoder_channels"]):
        for j, oc in enumerate(blocks):
            if j == len(blocks) - 1 and i != last:
                s = (cfg["encoder_strides"][i],) * 3
                rows.append(("SparseConv3d", c, oc, k3, s))
            else:
                rows += [("SubMConv3d", oc, oc, k3, (1, 1, 1))] * 2
            c = oc
    rows.append(("SparseConv3d", c, cfg["enc_out"], (1, 1, 1), (1, 1, 1)))
    return rows


@pytest.mark.parametrize("name", ["sunrgbd", "kitti_3classes", "scannet_large", "nuscenes"])
def test_encoder_wiring_oracle_matches_reference_golden(name):
    """ref models/pts_encoder/sparse_encoder_hd.py:36-138 (constructor + forward) and :140-214 (make_encoder_layers), built from the
    shipped config over stand-in sparse layers that evaluate conv3d on the densified tensor: the oracle performs the same sequence of
    sparse convolutions (kind, channels, kernel, stride, padding), meets the same active-set sizes at every level (its rulebook code
    against the dense-mask definition) and produces the same dense volume."""
    z = np.load(os.path.join(G, "encoder_wiring.npz"), allow_pickle=False)
    seed, shape = int(z["seed"]), tuple(int(v) for v in z["sparse_shape"])
    cfg = dict(ORACLE_CFG[name](), sparse_shape=shape)
    sd = _seeded_sd("pts_middle_encoder.", z[f"{name}.keys"], z[f"{name}.shapes"], seed)
    feats, coors = torch.from_numpy(z[f"{name}.feats"]), z[f"{name}.coors"]
    B = int(coors[:, 0].max()) + 1
    y = om.sparse_encoder(sd, "pts_middle_encoder.", feats, coors, B, cfg)
    ref = z[f"{name}.dense"]
    assert tuple(y.shape) == ref.shape
    np.testing.assert_allclose(y.numpy(), ref, rtol=2e-4, atol=2e-5 * float(np.abs(ref).max()))
    assert np.array_equal(y.numpy() != 0, ref != 0) or float(np.mean((y.numpy() != 0) != (ref != 0))) < 1e-3     # same active cells (ReLU zeros aside)
    # the call sequence
    num = z[f"{name}.trace_num"]
    exp = _expected_trace(cfg, shape)
    assert len(exp) == num.shape[0] == 21
    for row, kind, (ek, ecin, ecout, ekern, estride) in zip(num, z[f"{name}.trace_kind"], exp):
        assert (str(kind), int(row[0]), int(row[1]), tuple(row[2:5]), tuple(row[5:8])) == (ek, ecin, ecout, ekern, estride)
    # active-set sizes level by level: oracle/geometry.py's strided rule against the dense-mask definition the stand-ins evaluate
    c, dims, pads = coors, shape, []
    strided = [r for r, k in zip(num, z[f"{name}.trace_kind"]) if str(k) == "SparseConv3d" and tuple(r[2:5]) == (3, 3, 3)]
    for r in strided:
        pad = tuple(int(v) for v in r[8:11])
        oc, odims = og.strided_out_coords(c, dims, (3, 3, 3), tuple(int(v) for v in r[5:8]), pad)
        assert (int(r[11]), int(r[12])) == (c.shape[0], oc.shape[0]) and tuple(int(v) for v in r[16:19]) == tuple(odims)
        c, dims = oc, odims
        pads.append(pad)
    assert pads == [(1, 1, 1), (1, 1, 1), (0, 1, 1)]                # encoder_paddings' last entries (cfg :39), as make_encoder_layers reads them
    # indice keys as the reference assigns them (:79,:88,:103,:189): SparseBasicBlock convs carry none (=> rulebooks rebuilt per conv upstream)
    keys = [str(k) for k in z[f"{name}.trace_key"]]
    assert keys[0] == "subm1" and keys[-1] == "spconv_down2" and [k for k in keys if k.startswith("spconv") and k != "spconv_down2"] == ["spconv1", "spconv2", "spconv3"]
    assert sum(k == "" for k in keys) == 16


def test_encoder_state_dict_names_match_reference():
    z = np.load(os.path.join(G, "encoder_wiring.npz"), allow_pickle=False)
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd.configs.sunrgbd import model as mine
    from uni3detr_amd.registry import build_model
    m = build_model(mine)
    ref = {str(k): eval(str(s)) for k, s in zip(z["sunrgbd.keys"], z["sunrgbd.shapes"])}     # noqa: S307
    assert {k: tuple(v.shape) for k, v in m.pts_middle_encoder.state_dict().items()} == ref


def test_shift_scale_points_matches_reference_golden():
    """ref models/detectors/uni3detr.py:18-46."""
    z = np.load(os.path.join(G, "detector_glue.npz"), allow_pickle=False)
    x3 = torch.from_numpy(z["x3"])
    lo, hi = x3.min(dim=1)[0], x3.max(dim=1)[0]
    assert np.array_equal(om.shift_scale_unit(x3).numpy(), z["y_unit"])
    assert np.array_equal(om.shift_scale_points(x3, lo, hi, torch.from_numpy(z["dst_lo"]), torch.from_numpy(z["dst_hi"])).numpy(), z["y_dst"])
    ints = torch.from_numpy(z["ints"])
    assert np.array_equal(om.shift_scale_unit(ints).numpy(), z["y_int"])
    x4 = torch.from_numpy(z["x4"])
    f = x4.reshape(x4.shape[0], -1, 3)
    assert np.array_equal(om.shift_scale_points(x4, f.min(dim=1)[0], f.max(dim=1)[0]).numpy(), z["y4"])
    # the product's host-side form of the same function (plugin/detector.py) on the same vectors
    from uni3detr_amd.plugin.detector import shift_scale_points as prod
    assert np.array_equal(prod(x3, [lo, hi]).numpy(), z["y_unit"])
    assert np.array_equal(prod(ints, [ints.min(dim=1)[0], ints.max(dim=1)[0]]).numpy(), z["y_int"])


def test_dense_stack_gradient_conditioning():
    """The yardstick for every gradient tolerance over the dense stack (tests/test_reference_golden_gpu.py): in
    float64, perturb every convolution output of the restated SECOND3D + SECOND3DFPN by a relative 3e-6 (gaussian).  The forward
    moves by ~2e-5 - and the gradients by ~1.5e-2, three orders of magnitude more: ReLU decisions next to zero flip, each flip moves
    a whole row of the gradient in front of it and the BatchNorm means behind it.  A correct backward whose FORWARD deviates by 2e-5
    (the `parity` mode's split-bf16 products) therefore shows gradient deviations of 1-2e-2 on this network."""
    import torch.nn.functional as F
    name = "sunrgbd"
    z, sd = dense_stack_fixture(name)
    cfg = om.sunrgbd_cfg()

    def run(noise):
        g = torch.Generator().manual_seed(1)
        leaf = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
        x = torch.from_numpy(z[f"{name}.x"]).double().requires_grad_(True)
        orig = F.conv3d

        def noisy(*a, **k):
            y = orig(*a, **k)
            return y * (1 + noise * torch.randn(y.shape, generator=g, dtype=y.dtype)) if noise else y
        F.conv3d = noisy
        try:
            y = om.second3dfpn(leaf, "pts_neck.", om.second3d(leaf, "pts_backbone.", x, cfg), cfg)
        finally:
            F.conv3d = orig
        (y * torch.from_numpy(z[f"{name}.cot"]).double()).sum().backward()
        return y.detach(), x.grad, leaf["pts_backbone.blocks.0.1.bias"].grad

    rel = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    clean, pert = run(0.0), run(3e-6)
    fwd, dx, db = (rel(a, b) for a, b in zip(pert, clean))
    assert 5e-6 < fwd < 1e-4, fwd
    assert 3e-3 < dx < 5e-2 and 3e-3 < db < 6e-2, (dx, db)
    assert dx > 100 * fwd                                       # the amplification itself
