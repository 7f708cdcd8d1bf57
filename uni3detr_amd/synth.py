"""Seeded synthetic SUN-RGB-D-shaped scenes: points on room surfaces + 8 boxes, GT boxes/labels.

Host-side numpy only; the bench uploads the result once and keeps it resident in HBM.
"""
import numpy as np

SUNRGBD_RANGE = (-3.2, -0.2, -2.0, 3.2, 6.2, 0.56)
SUNRGBD_VOXEL = (0.02, 0.02, 0.02)


def room_scene(scene_id, n_points=20000, n_boxes=8, num_classes=10, pc_range=SUNRGBD_RANGE, seed_base=1234):
    """Returns points f32 [n_points,4] (x,y,z,height), gt f32 [n_boxes,7] (cx,cy,cz_gravity,dx,dy,dz,yaw), labels i64."""
    rng = np.random.default_rng(seed_base + scene_id)
    x0, y0, z0, x1, y1, z1 = pc_range
    sx, sy = (x1 - x0), (y1 - y0)
    # scale the canonical 6x6 m room to the configured range (identity for SUN RGB-D)
    fx, fy = sx / 6.4, sy / 6.4
    floor_z = z0 + 0.1
    surfaces = []  # (origin, u, v, area)
    rx0, rx1, ry0, ry1 = x0 + 0.2 * fx, x0 + 6.2 * fx, y0 + 0.2 * fy, y0 + 6.2 * fy
    surfaces.append((np.array([rx0, ry0, floor_z]), np.array([rx1 - rx0, 0, 0]), np.array([0, ry1 - ry0, 0])))
    wall_h = (z1 - z0) * 0.9
    surfaces.append((np.array([rx0, ry1, floor_z]), np.array([rx1 - rx0, 0, 0]), np.array([0, 0, wall_h])))
    surfaces.append((np.array([rx0, ry0, floor_z]), np.array([0, ry1 - ry0, 0]), np.array([0, 0, wall_h])))
    gt = np.zeros((n_boxes, 7), np.float32)
    for b in range(n_boxes):
        cx = rng.uniform(rx0 + 0.7 * fx, rx1 - 0.7 * fx)
        cy = rng.uniform(ry0 + 0.7 * fy, ry1 - 0.7 * fy)
        dx = rng.uniform(0.4, 2.0) * min(fx, 1.0)
        dy = rng.uniform(0.4, 1.2) * min(fy, 1.0)
        dz = min(rng.uniform(0.4, 1.2), wall_h * 0.8)
        yaw = rng.uniform(-np.pi, np.pi)
        cz = floor_z + dz / 2
        gt[b] = (cx, cy, cz, dx, dy, dz, yaw)
        c, s = np.cos(yaw), np.sin(yaw)
        ux, uy = np.array([c, s, 0.0]) * dx, np.array([-s, c, 0.0]) * dy
        uz = np.array([0, 0, dz])
        o = np.array([cx, cy, cz]) - ux / 2 - uy / 2 - uz / 2
        surfaces += [(o + uz, ux, uy), (o, ux, uz), (o + uy, ux, uz), (o, uy, uz), (o + ux, uy, uz)]
    areas = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in surfaces])
    counts = rng.multinomial(n_points, areas / areas.sum())
    pts = []
    for (o, u, v), k in zip(surfaces, counts):
        a, b = rng.random(k), rng.random(k)
        pts.append(o[None] + a[:, None] * u[None] + b[:, None] * v[None])
    p = np.concatenate(pts) + rng.normal(0, 0.005, (n_points, 3))
    p = p[rng.permutation(n_points)]
    h = p[:, 2:3] - p[:, 2].min()
    points = np.concatenate([p, h], 1).astype(np.float32)
    labels = rng.integers(0, num_classes, n_boxes).astype(np.int64)
    return points, gt, labels


def uniform_scene(scene_id, n_points=20000, pc_range=SUNRGBD_RANGE, seed_base=4321):
    """Uniform-in-volume cloud: the hash / active-set worst case."""
    rng = np.random.default_rng(seed_base + scene_id)
    lo, hi = np.array(pc_range[:3]), np.array(pc_range[3:])
    p = lo + rng.random((n_points, 3)) * (hi - lo)
    h = p[:, 2:3] - p[:, 2].min()
    return np.concatenate([p, h], 1).astype(np.float32)


def eval_scenes(n_scenes, n_det, num_classes, seed=0, max_gt=12, pc_range=SUNRGBD_RANGE, tp_frac=0.3, dup=3):
    """Seeded detection-evaluation sets: per scene (gt f32 [m,7] gravity-centre, gt labels i64 [m], det boxes f32 [n,7] bottom-centre,
    det scores f32 [n], det labels i64 [n]).  GT are room_scene-like boxes; detections are jittered copies of the GT (up to `dup` per GT,
    some with a wrong class) filling tp_frac of the list, the rest random boxes with random classes; n_det per scene (an int, or a
    [n_scenes] array)."""
    rng = np.random.default_rng(seed)
    x0, y0, z0, x1, y1, z1 = pc_range
    out = []
    for s in range(n_scenes):
        nd = int(n_det[s]) if np.ndim(n_det) else int(n_det)
        m = int(rng.integers(0, max_gt + 1))
        dims = rng.uniform(0.3, 2.0, (m, 3))
        ctr = np.stack([rng.uniform(x0 + 0.5, x1 - 0.5, m), rng.uniform(y0 + 0.5, y1 - 0.5, m), z0 + dims[:, 2] / 2 + rng.uniform(0, 0.3, m)], 1)
        gt = np.concatenate([ctr, dims, rng.uniform(-np.pi, np.pi, (m, 1))], 1).astype(np.float32)
        gl = rng.integers(0, num_classes, m)
        k = min(nd, int(round(tp_frac * nd)), m * dup) if m else 0
        src = rng.integers(0, m, k) if m else np.zeros(0, np.int64)
        near = gt[src].astype(np.float64)
        near[:, 2] -= near[:, 5] / 2
        near[:, :3] += rng.normal(0, 0.12, (k, 3)) * near[:, 3:6]
        near[:, 3:6] *= rng.uniform(0.75, 1.25, (k, 3))
        near[:, 6] += rng.normal(0, 0.15, k)
        nl = np.where(rng.uniform(size=k) < 0.9, gl[src], rng.integers(0, num_classes, k))
        r = nd - k
        rd = rng.uniform(0.2, 2.0, (r, 3))
        rand = np.concatenate([rng.uniform((x0, y0, z0), (x1, y1, z1 - 0.5), (r, 3)), rd, rng.uniform(-np.pi, np.pi, (r, 1))], 1)
        db = np.concatenate([near, rand]).astype(np.float32)
        dl = np.concatenate([nl, rng.integers(0, num_classes, r)]).astype(np.int64)
        ds = np.concatenate([rng.uniform(0.3, 1.0, k), rng.uniform(0.0, 0.7, r)]).astype(np.float32)
        p = rng.permutation(nd)
        out.append((gt, gl.astype(np.int64), db[p], ds[p], dl[p]))
    return out


# KITTI-like camera calibration (public KITTI object-benchmark values, rounded)
_KITTI_P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                      [0.0, 0.0, 0.0, 1.0]])
_KITTI_TR = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                      [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01], [0.0, 0.0, 0.0, 1.0]])
# (name, l, h, w, weight)
_KITTI_OBJECTS = (("Car", 3.9, 1.55, 1.65, 0.45), ("Van", 5.0, 2.1, 1.9, 0.08), ("Pedestrian", 0.85, 1.75, 0.65, 0.2),
                  ("Person_sitting", 0.8, 1.25, 0.6, 0.05), ("Cyclist", 1.75, 1.72, 0.6, 0.12), ("DontCare", 0, 0, 0, 0.1))


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def kitti_scenes(n, max_objects=16, det_per_scene=40, class_names=("Pedestrian", "Cyclist", "Car"), seed=0, image_shape=(375, 1242),
                 miss=0.15, dup=0.2):
    """Seeded KITTI-shaped evaluation sets -> (infos, results).

    infos: mmdet3d KITTI info dicts (image.image_idx / image_shape, calib.P2 / R0_rect / Tr_velo_to_cam as 4x4, annos in the camera frame
    with name / truncated / occluded / alpha / bbox / dimensions (l, h, w) / location (bottom centre) / rotation_y; DontCare rows have
    location -1000, dimensions -1, rotation_y and alpha -10).  Objects are Car / Van / Pedestrian / Person_sitting / Cyclist / DontCare at
    5-65 m, so 2-D heights spread around the 25 / 40 px limits; occlusion 0-3, truncation 0-0.6.
    results: `simple_test`-style dicts of LiDAR bottom-centre boxes f32 [m,7] (counter-clockwise yaw), scores f32 [m], labels i64 [m] in
    `class_names` order: perturbed copies of the GT (Van detected as Car, Person_sitting as Pedestrian; some missed, some duplicated)
    plus false positives, `det_per_scene` rows at most (an int, or a [n] array)."""
    from .kitti_eval import project_bbox
    rng = np.random.default_rng(seed)
    H, W = image_shape
    names = [o[0] for o in _KITTI_OBJECTS]
    prob = np.array([o[4] for o in _KITTI_OBJECTS])
    prob = prob / prob.sum()
    as_det = {"Car": "Car", "Van": "Car", "Pedestrian": "Pedestrian", "Person_sitting": "Pedestrian", "Cyclist": "Cyclist"}
    infos, results = [], []
    for s in range(n):
        R0 = np.eye(4)
        R0[:3, :3] = _rot_x(rng.normal(0, 0.004))
        Tr = _KITTI_TR.copy()
        Tr[:3, 3] += rng.normal(0, 0.01, 3)
        P2 = _KITTI_P2.copy()
        m = int(rng.integers(0, max_objects + 1))
        kinds = rng.choice(len(names), m, p=prob)
        rows = []
        placed = []
        for k in kinds:
            name, l, h, w, _ = _KITTI_OBJECTS[k]
            if name == "DontCare":
                x1, y1 = rng.uniform(0, W - 40), rng.uniform(100, H - 20)
                bw, bh = rng.uniform(15, 120), rng.uniform(10, 60)
                rows.append((name, -1.0, -1, -10.0, [x1, y1, min(x1 + bw, W), min(y1 + bh, H)], [-1.0, -1.0, -1.0], [-1000.0, -1000.0, -1000.0], -10.0))
                continue
            dims = np.array([l, h, w]) * rng.uniform(0.9, 1.1, 3)
            for _ in range(20):
                z = rng.uniform(5, 65)
                x = rng.uniform(-0.45, 0.45) * z
                if all(abs(x - px) > 2.5 or abs(z - pz) > 5.5 for px, pz in placed):
                    break
            placed.append((x, z))
            loc = np.array([x, 1.65 + rng.normal(0, 0.05), z])
            ry = rng.uniform(-np.pi, np.pi)
            bb = project_bbox(loc, dims, ry, P2)[0]
            bb[:2] = np.maximum(bb[:2], 0)
            bb[2:] = np.minimum(bb[2:], [W, H])
            if not (bb[2] > bb[0] + 1 and bb[3] > bb[1] + 1):
                continue
            trunc = float(rng.choice([0.0, 0.0, 0.0, 0.1, 0.2, 0.4, 0.6]))
            occ = int(rng.choice([0, 0, 1, 2, 3], p=[0.4, 0.2, 0.2, 0.15, 0.05]))
            rows.append((name, trunc, occ, float(ry - np.arctan2(x, z)), bb.tolist(), dims.tolist(), loc.tolist(), float(ry)))
        annos = dict(name=np.array([r[0] for r in rows], dtype="<U14"), truncated=np.array([r[1] for r in rows], np.float64),
                     occluded=np.array([r[2] for r in rows], np.int64), alpha=np.array([r[3] for r in rows], np.float64),
                     bbox=np.array([r[4] for r in rows], np.float64).reshape(-1, 4),
                     dimensions=np.array([r[5] for r in rows], np.float64).reshape(-1, 3),
                     location=np.array([r[6] for r in rows], np.float64).reshape(-1, 3),
                     rotation_y=np.array([r[7] for r in rows], np.float64))
        infos.append(dict(image=dict(image_idx=s, image_shape=np.array([H, W], np.int32)),
                          calib=dict(P2=P2, R0_rect=R0, Tr_velo_to_cam=Tr), annos=annos))
        # detections: camera -> LiDAR with inv(R0_rect @ Tr_velo_to_cam), yaw = -ry - pi/2, (dx, dy, dz) = (l, w, h)
        Tinv = np.linalg.inv(R0 @ Tr)
        nd = int(det_per_scene[s]) if np.ndim(det_per_scene) else int(det_per_scene)
        boxes, labels, scores = [], [], []
        for r in rows:
            if r[0] not in as_det or as_det[r[0]] not in class_names or rng.uniform() < miss:
                continue
            for _ in range(2 if rng.uniform() < dup else 1):
                loc = np.array(r[6]) + rng.normal(0, 0.15, 3) * np.array([1.0, 0.3, 1.0])
                dims = np.array(r[5]) * rng.uniform(0.9, 1.1, 3)
                ry = r[7] + rng.normal(0, 0.1)
                p = Tinv @ np.append(loc, 1.0)
                boxes.append([p[0], p[1], p[2], dims[0], dims[2], dims[1], -ry - np.pi / 2])
                labels.append(class_names.index(as_det[r[0]]))
                scores.append(rng.uniform(0.3, 1.0))
        boxes, labels, scores = boxes[:nd], labels[:nd], scores[:nd]
        nfp = nd - len(boxes)
        for _ in range(nfp):
            c = int(rng.integers(0, len(class_names)))
            _, l, h, w, _ = _KITTI_OBJECTS[names.index(class_names[c])]
            boxes.append([rng.uniform(0, 70), rng.uniform(-40, 40), rng.uniform(-2.5, -1.0), l, w, h, rng.uniform(-np.pi, np.pi)])
            labels.append(c)
            scores.append(rng.uniform(0.0, 0.7))
        perm = rng.permutation(len(boxes))
        results.append(dict(boxes_3d=np.asarray(boxes, np.float32).reshape(-1, 7)[perm], scores_3d=np.asarray(scores, np.float32)[perm],
                            labels_3d=np.asarray(labels, np.int64)[perm]))
    return infos, results


# nuScenes-like object sizes (l, w, h) and how often each class appears
_NUSC_OBJECTS = (("car", 4.6, 1.9, 1.7, 0.3), ("truck", 6.9, 2.5, 2.8, 0.08), ("trailer", 12.0, 2.9, 3.9, 0.04), ("bus", 11.0, 2.9, 3.5, 0.03),
                 ("construction_vehicle", 6.4, 2.8, 3.2, 0.03), ("bicycle", 1.7, 0.6, 1.3, 0.06), ("motorcycle", 2.1, 0.8, 1.5, 0.06),
                 ("pedestrian", 0.7, 0.7, 1.8, 0.2), ("traffic_cone", 0.4, 0.4, 1.1, 0.1), ("barrier", 2.5, 0.5, 1.0, 0.1))


def _quat(roll, pitch, yaw):
    """(w, x, y, z) of R = Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = (np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2))
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


def nusc_samples(n, preds_per_sample=60, seed=0, class_names=None, max_gt=30, miss=0.15, dup=0.2):
    """Seeded nuScenes-shaped evaluation sets -> (infos, results).

    infos: mmdet3d v1.0 nuScenes info dicts (token, lidar2ego / ego2global rotation (w, x, y, z) with small pitch / roll and translation,
    global translations of 300-2000 m; gt_boxes [g, 7] gravity centre (x, y, z, l, w, h, yaw), gt_names, gt_velocity [g, 2] (some NaN),
    num_lidar_pts (some 0), num_radar_pts, gt_attr_names).  Every sample holds all 10 classes at 0-60 m, so the class ranges cut; every
    third sample has a `static_object.bicycle_rack` row with a bicycle inside, and some rows have a non-evaluated name.  GT attributes
    follow the prediction heuristic of the GT's own global velocity.
    results: `simple_test`-style dicts of LiDAR bottom-centre boxes f32 [m, 9] (x, y, z, l, w, h, yaw, vx, vy), scores f32 [m] (some on a
    0.05 grid, so equal scores occur), labels i64 [m] in `class_names` order: perturbed copies of the GT (some missed, some duplicated,
    a few turned by pi) plus false positives, `preds_per_sample` rows at most (an int, or a [n] array)."""
    from .nuscenes_eval import CLASSES, _attr_code, _calib, _pred_attribute, _Tables, to_global
    class_names = tuple(CLASSES if class_names is None else class_names)
    tab = _Tables(CLASSES)
    rng = np.random.default_rng(seed)
    names = [o[0] for o in _NUSC_OBJECTS]
    prob = np.array([o[4] for o in _NUSC_OBJECTS])
    prob = prob / prob.sum()
    infos, results = [], []
    for s in range(n):
        info = dict(token=f"nusc_{seed}_{s}", lidar2ego_rotation=_quat(rng.normal(0, 0.01), rng.normal(0, 0.01), rng.uniform(-np.pi, np.pi)),
                    lidar2ego_translation=[0.94 + rng.normal(0, 0.02), rng.normal(0, 0.02), 1.84 + rng.normal(0, 0.02)],
                    ego2global_rotation=_quat(rng.normal(0, 0.02), rng.normal(0, 0.02), rng.uniform(-np.pi, np.pi)),
                    ego2global_translation=[rng.uniform(300, 2000), rng.uniform(300, 2000), rng.normal(0, 1)])
        m = int(rng.integers(len(names), max_gt + 1))
        kinds = np.concatenate([np.arange(len(names)), rng.choice(len(names), m - len(names), p=prob)])
        rows, gnames, vel, lid, rad = [], [], [], [], []
        for k in kinds:
            name, l, w, h, _ = _NUSC_OBJECTS[k]
            r, a = rng.uniform(2, 60), rng.uniform(-np.pi, np.pi)
            dims = np.array([l, w, h]) * rng.uniform(0.85, 1.15, 3)
            rows.append([r * np.cos(a), r * np.sin(a), rng.normal(-1.0, 0.3), *dims, rng.uniform(-np.pi, np.pi)])
            gnames.append(name)
            if name in ("barrier", "traffic_cone"):
                v = [0.0, 0.0]
            else:
                sp, d = (rng.uniform(0.15, 0.25) if rng.uniform() < 0.2 else rng.uniform(0, 8)), rng.uniform(-np.pi, np.pi)
                v = [sp * np.cos(d), sp * np.sin(d)] if rng.uniform() > 0.1 else [np.nan, np.nan]
            vel.append(v)
            lid.append(0 if rng.uniform() < 0.08 else int(rng.integers(1, 200)))
            rad.append(int(rng.integers(0, 4)))
        if s % 3 == 0:                                     # a rack with a parked bicycle in it
            c = rows[0][:2]
            rows.append([c[0] + 4.0, c[1] + 4.0, -1.0, 3.0, 1.5, 1.2, rng.uniform(-np.pi, np.pi)])
            gnames.append("static_object.bicycle_rack")
            vel.append([0.0, 0.0]); lid.append(30); rad.append(0)                        # noqa: E702
            rows.append([c[0] + 4.2, c[1] + 3.9, -1.1, 1.7, 0.6, 1.0, rng.uniform(-np.pi, np.pi)])
            gnames.append("bicycle")
            vel.append([0.0, 0.0]); lid.append(20); rad.append(0)                        # noqa: E702
        if s % 4 == 1:                                     # a class outside the evaluation
            rows.append([5.0, -3.0, -1.0, 1.0, 0.6, 0.5, 0.3])
            gnames.append("animal")
            vel.append([np.nan, np.nan]); lid.append(5); rad.append(0)                   # noqa: E702
        rows = np.asarray(rows, np.float64).reshape(-1, 7)
        vel = np.asarray(vel, np.float64).reshape(-1, 2)
        g = rows.shape[0]
        # GT attributes: the heuristic of the GT's global velocity
        grows = np.concatenate([rows, vel], 1)
        cls = np.asarray([tab.index.get(nm, -1) for nm in gnames], np.int32)
        rec, _ = to_global(grows, np.maximum(cls, 0), np.zeros(g), None, [g], _calib(info)[None], True, tab)
        speed = np.sqrt(rec[:, 7] * rec[:, 7] + rec[:, 8] * rec[:, 8])
        attrs = [_pred_attribute(nm, bool(sp > 0.2)) if nm in tab.index else "" for nm, sp in zip(gnames, speed)]
        assert all(_attr_code(a) >= -1 for a in attrs)
        info.update(gt_boxes=rows, gt_names=np.array(gnames), gt_velocity=vel, num_lidar_pts=np.asarray(lid, np.int64),
                    num_radar_pts=np.asarray(rad, np.int64), gt_attr_names=np.array(attrs), valid_flag=np.ones(g, bool))
        infos.append(info)
        # predictions
        nd = int(preds_per_sample[s]) if np.ndim(preds_per_sample) else int(preds_per_sample)
        boxes, labels, scores = [], [], []
        for i in range(g):
            if gnames[i] not in class_names or rng.uniform() < miss:
                continue
            for _ in range(2 if rng.uniform() < dup else 1):
                sig = rng.choice([0.05, 0.3, 0.8, 1.5])
                x, y, z, l, w, h, yaw = rows[i]
                yaw = yaw + (np.pi if rng.uniform() < 0.05 else rng.normal(0, 0.15))
                v = np.nan_to_num(vel[i]) + rng.normal(0, 0.3, 2)
                boxes.append([x + rng.normal(0, sig), y + rng.normal(0, sig), z - h / 2 + rng.normal(0, 0.1), *(rows[i, 3:6] * rng.uniform(0.9, 1.1, 3)),
                              yaw, v[0], v[1]])
                labels.append(class_names.index(gnames[i]))
                scores.append(rng.uniform(0.3, 1.0))
        boxes, labels, scores = boxes[:nd], labels[:nd], scores[:nd]
        for _ in range(nd - len(boxes)):
            c = int(rng.integers(0, len(class_names)))
            _, l, w, h, _ = _NUSC_OBJECTS[names.index(class_names[c])]
            r, a = rng.uniform(0, 60), rng.uniform(-np.pi, np.pi)
            boxes.append([r * np.cos(a), r * np.sin(a), rng.normal(-1.8, 0.3), l, w, h, rng.uniform(-np.pi, np.pi), *rng.normal(0, 2, 2)])
            labels.append(c)
            scores.append(rng.uniform(0.0, 0.6))
        scores = np.asarray(scores, np.float64)
        grid = rng.uniform(size=scores.shape) < 0.15
        scores[grid] = np.round(scores[grid] * 20) / 20
        perm = rng.permutation(len(boxes))
        results.append(dict(boxes_3d=np.asarray(boxes, np.float32).reshape(-1, 9)[perm], scores_3d=scores.astype(np.float32)[perm],
                            labels_3d=np.asarray(labels, np.int64)[perm]))
    return infos, results


def gtdb_scenes(kind, n, seed=0):
    """Seeded scenes shaped like what the GT-paste database builder crops, as the dicts gtdb.create_groundtruth_database takes.
    kind 'nuscenes': a 10-sweep cloud already merged (250-300 k points, 5 columns: x, y, z, intensity, time lag), about 35 boxes of 9
    columns over the ten classes, a valid flag; kind 'kitti': about 120 k points of 4 columns, about 10 boxes of 7 columns, difficulty.
    Ground points on a ring pattern plus a cluster of points on every box, so that objects hold from a handful to a few thousand."""
    rng = np.random.default_rng(seed)
    nusc = kind == "nuscenes"
    if kind not in ("nuscenes", "kitti"):
        raise ValueError(f"kind {kind!r} (nuscenes or kitti)")
    objects = _NUSC_OBJECTS if nusc else tuple(o for o in _KITTI_OBJECTS if o[0] != "DontCare")
    prob = np.array([o[4] for o in objects])
    out = []
    for s in range(n):
        g = int(rng.integers(25, 46)) if nusc else int(rng.integers(5, 16))
        kinds = rng.choice(len(objects), g, p=prob / prob.sum())
        boxes = np.zeros((g, 9 if nusc else 7), np.float32)
        r, a = rng.uniform(4, 50 if nusc else 60, g), rng.uniform(-np.pi, np.pi, g) if nusc else rng.uniform(-0.6, 0.6, g)
        boxes[:, 0], boxes[:, 1], boxes[:, 2] = r * np.cos(a), r * np.sin(a), rng.normal(-1.8, 0.15, g)
        for j, k in enumerate(kinds):
            o = objects[k]
            boxes[j, 3:6] = np.array((o[1], o[2], o[3]) if nusc else (o[1], o[3], o[2])) * rng.uniform(0.9, 1.1, 3)
        boxes[:, 6] = rng.uniform(-np.pi, np.pi, g)
        if nusc:
            boxes[:, 7:] = rng.normal(0, 2, (g, 2))
        npts = int(rng.integers(250_000, 300_001)) if nusc else int(rng.integers(110_000, 130_001))
        feat = 5 if nusc else 4
        rr = rng.gamma(2.0, 9.0, npts) + 1.5
        aa = rng.uniform(-np.pi, np.pi, npts) if nusc else rng.uniform(-0.8, 0.8, npts)
        pts = np.zeros((npts, feat), np.float32)
        pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3] = rr * np.cos(aa), rr * np.sin(aa), rng.normal(-1.8, 0.1, npts), rng.uniform(0, 1, npts)
        if nusc:
            pts[:, 4] = rng.integers(0, 11, npts) * np.float32(0.05)
        on = rng.integers(0, g, npts // 20)                       # a twentieth of the cloud sits on the objects, fewer far away
        on = on[rng.uniform(0, 1, len(on)) < np.minimum(1.0, 12.0 / r[on])]
        q = rng.uniform(-0.5, 0.5, (len(on), 3)) * boxes[on, 3:6] + np.array([0, 0, 0.5]) * boxes[on, 3:6]
        c, sn = np.cos(boxes[on, 6]), np.sin(boxes[on, 6])
        pts[:len(on), 0] = q[:, 0] * c - q[:, 1] * sn + boxes[on, 0]
        pts[:len(on), 1] = q[:, 0] * sn + q[:, 1] * c + boxes[on, 1]
        pts[:len(on), 2] = q[:, 2] + boxes[on, 2]
        pts = pts[rng.permutation(npts)]
        sc = dict(sample_idx=f"{s:06d}" if nusc else s, points=pts, gt_bboxes_3d=boxes, gt_names=np.array([objects[k][0] for k in kinds]))
        if nusc:
            sc["valid_flag"] = rng.uniform(0, 1, g) < 0.9
        else:
            sc["difficulty"] = rng.integers(-1, 3, g).astype(np.int32)
        out.append(sc)
    return out
