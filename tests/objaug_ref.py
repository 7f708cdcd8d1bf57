"""NumPy restatement of the upstream mmdet3d helpers behind GT-paste and ObjectNoise (v1.0.0rc5, recalled): box_np_ops
(center_to_corner_box2d, points_in_rbbox), data_augment_utils (box_collision_test, noise_per_box, the noise_per_object_v3_ transform
steps) and dbsampler.BatchSampler, plus the per-scene GT-paste of UnifiedDataBaseSampler.sample_all / sample_class_v2 on candidates
that are already drawn.  float64 throughout; yaw counter-clockwise, as the project's boxes and rotated IoU.  Used by
test_objaug_cpu.py (also injected, as stub modules, under the reference's own sampler) and test_objaug_gpu.py."""
import numpy as np


class BatchSampler:
    def __init__(self, sampled_list, name=None, epoch=None, shuffle=True, drop_reminder=False):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx, self._example_num, self._name, self._shuffle = 0, len(sampled_list), name, shuffle

    def _sample(self, num):
        if self._idx + num >= self._example_num:
            ret = self._indices[self._idx:].copy()
            self._reset()
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def _reset(self):
        if self._shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0

    def sample(self, num):
        return [self._sampled_list[i] for i in self._sample(num)]


def center_to_corner_box2d(centers, dims, angles):
    """[N, 4, 2]: corners (-.5,-.5), (-.5,.5), (.5,.5), (.5,-.5) times dims, rotated counter-clockwise by the angle, plus the centre."""
    centers, dims, angles = (np.asarray(a, np.float64) for a in (centers, dims, angles))
    norm = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]])
    c = dims[:, None, :] * norm[None]
    cs, sn = np.cos(angles)[:, None], np.sin(angles)[:, None]
    return np.stack([c[..., 0] * cs - c[..., 1] * sn, c[..., 0] * sn + c[..., 1] * cs], -1) + centers[:, None, :]


def box_collision_test(boxes, qboxes, clockwise=True):
    """[N, K] bool for corner lists [N, 4, 2] / [K, 4, 2]: standup overlap, then an edge crossing or full containment."""
    N, K = boxes.shape[0], qboxes.shape[0]
    ret = np.zeros((N, K), dtype=np.bool_)
    for i in range(N):
        for j in range(K):
            ret[i, j] = _collide(boxes[i], qboxes[j], clockwise)
    return ret


def _collide(a, b, clockwise=True):
    if not (min(a[:, 0].max(), b[:, 0].max()) - max(a[:, 0].min(), b[:, 0].min()) > 0):
        return False
    if not (min(a[:, 1].max(), b[:, 1].max()) - max(a[:, 1].min(), b[:, 1].min()) > 0):
        return False
    for k in range(4):
        A, B = a[k], a[(k + 1) % 4]
        for l in range(4):
            C, D = b[l], b[(l + 1) % 4]
            acd = (D[1] - A[1]) * (C[0] - A[0]) > (C[1] - A[1]) * (D[0] - A[0])
            bcd = (D[1] - B[1]) * (C[0] - B[0]) > (C[1] - B[1]) * (D[0] - B[0])
            if acd != bcd:
                abc = (C[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (C[0] - A[0])
                abd = (D[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (D[0] - A[0])
                if abc != abd:
                    return True
    for o, q in ((a, b), (b, a)):
        holds = True
        for l in range(4):
            for k in range(4):
                vec = o[k] - o[(k + 1) % 4]
                if clockwise:
                    vec = -vec
                if vec[1] * (o[k, 0] - q[l, 0]) - vec[0] * (o[k, 1] - q[l, 1]) >= 0:
                    holds = False
                    break
            if not holds:
                break
        if holds:
            return True
    return False


def points_in_rbbox(points, rbbox, z_axis=2, origin=(0.5, 0.5, 0)):
    """[N, M] bool: point strictly inside all six faces of the bottom-centre box (x, y, z, dx, dy, dz, yaw)."""
    assert z_axis == 2 and tuple(origin) == (0.5, 0.5, 0)
    p = np.asarray(points, np.float64)[:, None, :3]
    b = np.asarray(rbbox, np.float64)[None]
    dx, dy = p[..., 0] - b[..., 0], p[..., 1] - b[..., 1]
    c, s = np.cos(b[..., 6]), np.sin(b[..., 6])
    lx, ly = dx * c + dy * s, -dx * s + dy * c
    return (np.abs(lx) < b[..., 3] / 2) & (np.abs(ly) < b[..., 4] / 2) & (p[..., 2] > b[..., 2]) & (p[..., 2] < b[..., 2] + b[..., 5])


def greedy_accept(gt_boxes, cand_boxes, cand_grp):
    """sample_class_v2 class by class (classes contiguous in cand_grp): -> accepted bool [K]."""
    acc = np.zeros(len(cand_boxes), bool)
    avoid = np.asarray(gt_boxes, np.float64).reshape(-1, cand_boxes.shape[1] if len(cand_boxes) else 7)
    k = 0
    while k < len(cand_boxes):
        e = k
        while e < len(cand_boxes) and cand_grp[e] == cand_grp[k]:
            e += 1
        sp = cand_boxes[k:e]
        total = np.concatenate([avoid, sp], 0)
        bv = center_to_corner_box2d(total[:, 0:2], total[:, 3:5], total[:, 6])
        coll = box_collision_test(bv, bv)
        coll[np.arange(len(total)), np.arange(len(total))] = False
        ng = avoid.shape[0]
        for i in range(ng, len(total)):
            if coll[i].any():
                coll[i] = False
                coll[:, i] = False
            else:
                acc[k + i - ng] = True
        avoid = np.concatenate([avoid, sp[acc[k:e]]], 0)
        k = e
    return acc


def paste_scene(points, gt_boxes, gt_labels, cand_boxes, cand_labels, cand_points, cand_grp, sampled_first):
    """one scene's GT-paste with drawn candidates (cand_points: list of points relative to the box's (x, y, z_bottom)) ->
    dict(points, boxes, labels, points_idx, accepted)."""
    cand_boxes = np.asarray(cand_boxes, np.float64).reshape(-1, gt_boxes.shape[1])
    acc = greedy_accept(gt_boxes, cand_boxes, np.asarray(cand_grp))
    if not acc.any():
        return dict(points=points, boxes=gt_boxes, labels=gt_labels, points_idx=-np.ones(len(points), int), accepted=acc)
    sb = cand_boxes[acc]
    sp, si = [], []
    for n, k in enumerate(np.nonzero(acc)[0]):
        p = np.array(cand_points[k], np.float64)
        p[:, :3] += cand_boxes[k, :3]
        sp.append(p)
        si.append(np.full(len(p), n))
    sp, si = np.concatenate(sp), np.concatenate(si)
    keep = points[~points_in_rbbox(points, sb).any(-1)]
    if sampled_first:
        pts, idx = np.concatenate([sp, keep]), np.concatenate([si, -np.ones(len(keep), int)])
    else:
        pts, idx = np.concatenate([keep, sp]), np.concatenate([-np.ones(len(keep), int), si])
    return dict(points=pts, boxes=np.concatenate([gt_boxes, sb]), labels=np.concatenate([gt_labels, np.asarray(cand_labels)[acc]]),
                points_idx=idx, accepted=acc)


def noise_per_box(boxes, valid_mask, loc_noises, rot_noises):
    """boxes [N, 5] = (x, y, dx, dy, yaw) -> chosen try per box (-1 = none)."""
    corners = center_to_corner_box2d(boxes[:, :2], boxes[:, 2:4], boxes[:, 4])
    success = -np.ones(len(boxes), np.int64)
    for i in range(len(boxes)):
        if not valid_mask[i]:
            continue
        for j in range(loc_noises.shape[1]):
            c, s = np.cos(rot_noises[i, j]), np.sin(rot_noises[i, j])
            cur = corners[i] - boxes[i, :2]
            cur = np.stack([cur[:, 0] * c - cur[:, 1] * s, cur[:, 0] * s + cur[:, 1] * c], -1) + boxes[i, :2] + loc_noises[i, j, :2]
            hit = [k for k in range(len(boxes)) if k != i and _collide(cur, corners[k])]
            if not hit:
                success[i] = j
                corners[i] = cur
                break
    return success


def object_noise(boxes, points, loc, rot):
    """noise_per_object_v3_ (global_rot_range = 0) with given draws -> (boxes, points, chosen); inputs are not modified."""
    boxes, points = np.array(boxes, np.float64), np.array(points, np.float64)
    chosen = noise_per_box(boxes[:, [0, 1, 3, 4, 6]], np.ones(len(boxes), bool), loc, rot)
    if len(points) and len(boxes):
        mask = points_in_rbbox(points, boxes)
        first = mask.argmax(1)                             # points_transform_: the first box holding the point, then break
        sel = mask.any(1) & (chosen[first] >= 0)
        j = first[sel]
        a, l = rot[j, chosen[j]], loc[j, chosen[j]]
        c, s = np.cos(a), np.sin(a)
        x, y, z = (points[sel, :3] - boxes[j, :3]).T
        points[sel, 0] = x * c - y * s + boxes[j, 0] + l[:, 0]
        points[sel, 1] = x * s + y * c + boxes[j, 1] + l[:, 1]
        points[sel, 2] = z + boxes[j, 2] + l[:, 2]
    for j in range(len(boxes)):
        if chosen[j] >= 0:
            boxes[j, :3] += loc[j, chosen[j]]
            boxes[j, 6] += rot[j, chosen[j]]
    return boxes, points, chosen
