"""KITTI 3-D detection evaluation: AP11 / AP40 of the 2-D, BEV and 3-D boxes and AOS, per class, difficulty and overlap setting (the
`evaluation` of the shipped KITTI configs, upstream `KittiDataset.evaluate` -> `kitti_eval`).

Provenance: parity unpinned.  The upstream metric is mmdet3d v1.0.0rc5's `core/evaluation/kitti_utils/eval.py` (the numba port of the
KITTI devkit); it is neither in the reference tree nor installed, so nothing here is pinned against its source.  The semantics below
are the contract, restated from the upstream algorithm; the `ret_dict` key names are recalled and kept in `_KEYS` so a correction is
one edit.

  * annos are KITTI camera-frame dicts: name, truncated, occluded, alpha, bbox [n,4], dimensions [n,3] (l, h, w), location [n,3]
    (bottom centre), rotation_y, and score for detections; current_classes are Car / Pedestrian / Cyclist (names or ids 0 / 1 / 2);
  * overlaps are [dt, gt] per scene: 2-D IoU without +1; BEV rotated IoU of (x, z, l, w, ry); 3-D = BEV intersection x height overlap
    (camera y points down, the top is y - h).  A box with a non-positive l, h or w (KITTI's DontCare rows) has BEV / 3-D overlap 0;
  * clean_data: MIN_HEIGHT 40 / 25 / 25, MAX_OCCLUSION 0 / 1 / 2, MAX_TRUNCATION 0.15 / 0.3 / 0.5; Van counts as an ignored Car,
    Person_sitting as an ignored Pedestrian; a detection lower than MIN_HEIGHT (strict '<') is ignored; DontCare boxes are collected;
  * compute_statistics: pass 1 (thresh 0) takes, per GT in index order, the highest-scoring eligible detection (lowest index on ties);
    get_thresholds picks <= 41 scores from the sorted TP scores; pass 2 takes the best-overlap detection at each threshold, counts
    tp / fp / fn, removes bbox false positives inside a DontCare box (intersection over the detection's area) and sums (1 + cos d) / 2;
  * precision = tp / (tp + fp) and aos = sim / (tp + fp) in float64, each replaced by its maximum over the later thresholds;
    AP11 = sum prec[0:41:4] / 11 * 100, AP40 = sum prec[1:41] / 40 * 100; AOS (with the bbox metric) is on when some detection has
    alpha != -10 and the first GT of some scene with GT has alpha != -10.

Two implementations of the same result: the device path (csrc/kitti_eval.hip through `native.kitti_eval_core`; ATen only sorts the TP
scores and scans the validity flags of the LiDAR conversion) and a float64 NumPy restatement for `device="cpu"`, which is the test
yardstick.  Everything is deterministic: any batching of the same scenes gives bit-identical results.
"""
import numpy as np
import torch

from .eval_common import DetBuffer, default_device, invalid_device, invalid_host, offsets, print_log, raise_invalid
from .evaluation import rect_corners, rect_inter_area

# the messages of the detection checks: a non-finite score, a label that does not index class_names
ERRORS = ("kitti_eval: detection scores must be finite", "KittiEvaluator: labels must index class_names")
_SHORT = "kitti_eval: boxes_3d must have 7 columns (x, y, z, dx, dy, dz, yaw)"
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist"}
_NAME_TO_ID = {v.lower(): k for k, v in CLASS_TO_NAME.items()}
# class codes of the device records: Car, Pedestrian, Cyclist, Van, Person_sitting, DontCare, anything else
_CODES = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}
_OTHER, _DONTCARE = 6, 5
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
DIFFICULTY = ("easy", "moderate", "hard")
SETTINGS = ("strict", "loose")
METRICS = ("bbox", "bev", "3d")
NO_DETECTION = -10000000.0
N_SAMPLE_PTS = 41
# min overlap [setting][metric][class id]
MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5], [0.7, 0.5, 0.5], [0.7, 0.5, 0.5]],
                         [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])
# ret_dict naming (mmdet3d v1.0, recalled): metric tags and the two key patterns
_KEYS = dict(metric={"3d": "3D", "bev": "BEV", "bbox": "2D", "aos": "AOS"},
             cls="KITTI/{cls}_{metric}_{ap}_{difficulty}_{setting}", overall="KITTI/Overall_{metric}_{ap}_{difficulty}")


# --------------------------------------------------------------------------------------------------
# input encoding: records [n, 16] = camera box (x, y, z, l, h, w, ry), bbox (4), alpha, score | GT ignore bits, class code, 2 unused
# --------------------------------------------------------------------------------------------------
def _class_ids(current_classes):
    out = []
    for c in current_classes:
        if isinstance(c, str):
            if c.lower() not in _NAME_TO_ID:
                raise ValueError(f"kitti_eval: unsupported class {c!r} (Car, Pedestrian, Cyclist)")
            out.append(_NAME_TO_ID[c.lower()])
        else:
            if int(c) not in CLASS_TO_NAME:
                raise ValueError(f"kitti_eval: unsupported class id {c!r} (0 Car, 1 Pedestrian, 2 Cyclist)")
            out.append(int(c))
    if not out:
        raise ValueError("kitti_eval: no classes to evaluate")
    return out


def _codes(names):
    return np.asarray([_CODES.get(str(n).lower(), _OTHER) for n in names], np.int64)


def _rows(a, n, k):
    a = np.asarray(a, np.float64)
    return a.reshape(n, k) if n else np.zeros((0, k))


def _encode(anno, is_gt):
    """one anno dict -> float64 records [n, 16]"""
    n = len(anno["name"])
    r = np.zeros((n, 16))
    if n == 0:
        return r
    r[:, 0:3] = _rows(anno["location"], n, 3)
    r[:, 3:6] = _rows(anno["dimensions"], n, 3)
    r[:, 6] = np.asarray(anno["rotation_y"], np.float64).reshape(n)
    r[:, 7:11] = _rows(anno["bbox"], n, 4)
    r[:, 11] = np.asarray(anno["alpha"], np.float64).reshape(n)
    if is_gt:
        height = r[:, 10] - r[:, 8]
        occ = np.asarray(anno["occluded"], np.float64).reshape(n)
        trunc = np.asarray(anno["truncated"], np.float64).reshape(n)
        bits = np.zeros(n, np.int64)
        for d in range(3):
            ign = (occ > MAX_OCCLUSION[d]) | (trunc > MAX_TRUNCATION[d]) | (height <= MIN_HEIGHT[d])
            bits |= ign.astype(np.int64) << d
        r[:, 12] = bits
    else:
        sc = np.asarray(anno["score"], np.float64).reshape(n)
        raise_invalid(invalid_host(sc, np.zeros(0)), ERRORS)
        r[:, 12] = sc
    r[:, 13] = _codes(anno["name"])
    return r


def _encode_all(annos, is_gt):
    recs = [_encode(a, is_gt) for a in annos]
    counts = [r.shape[0] for r in recs]
    return (np.concatenate(recs) if recs else np.zeros((0, 16))), counts


def _compute_aos(gt_annos, dt_annos):
    pred_alpha = any(np.any(np.asarray(a["alpha"]) != -10) for a in dt_annos)
    valid_alpha_gt = any(len(a["alpha"]) and np.asarray(a["alpha"]).reshape(-1)[0] != -10 for a in gt_annos)
    return bool(pred_alpha and valid_alpha_gt)


def _groups(class_ids, metrics):
    """group g -> (flag index = class slot * 3 + difficulty, metric id, min overlap); order (class, difficulty, metric, setting)."""
    gfid, gmet, gmin = [], [], []
    for ci, c in enumerate(class_ids):
        for d in range(3):
            for m in metrics:
                for o in range(2):
                    gfid.append(ci * 3 + d)
                    gmet.append(m)
                    gmin.append(MIN_OVERLAPS[o, m, c])
    return np.asarray(gfid, np.int64), np.asarray(gmet, np.int64), np.asarray(gmin, np.float64)


# --------------------------------------------------------------------------------------------------
# host path (float64 NumPy)
# --------------------------------------------------------------------------------------------------
def image_box_iou(a, b, criterion=-1):
    """[N, K] 2-D overlap of boxes (x1, y1, x2, y2) without +1: IoU (criterion -1) or intersection over a's area (criterion 0)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    inter = iw * ih
    aa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    ab = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    ua = aa + ab - inter if criterion == -1 else np.broadcast_to(aa, inter.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((iw > 0) & (ih > 0), inter / ua, 0.0)


def box_overlaps(dt, gt):
    """camera boxes (x, y, z, l, h, w, ry) [N,>=7] x [K,>=7] -> (bev IoU, 3-D IoU) float64 [N, K]."""
    a, b = np.asarray(dt, np.float64).reshape(-1, dt.shape[-1])[:, :7], np.asarray(gt, np.float64).reshape(-1, gt.shape[-1])[:, :7]
    n, k = a.shape[0], b.shape[0]
    if n * k == 0:
        return np.zeros((n, k)), np.zeros((n, k))
    p, q = np.repeat(a, k, 0), np.tile(b, (n, 1))
    z = np.zeros(p.shape[0])
    inter = rect_inter_area(rect_corners(z, z, p[:, 3], p[:, 5], -p[:, 6]),
                            rect_corners(q[:, 0] - p[:, 0], q[:, 2] - p[:, 2], q[:, 3], q[:, 5], -q[:, 6]))
    ok = (p[:, 3:6] > 0).all(1) & (q[:, 3:6] > 0).all(1)
    inter = np.where(ok, inter, 0.0)
    dy = np.minimum(p[:, 1], q[:, 1]) - np.maximum(p[:, 1] - p[:, 4], q[:, 1] - q[:, 4])
    inter3 = inter * np.maximum(dy, 0.0)
    den_bev = p[:, 3] * p[:, 5] + q[:, 3] * q[:, 5] - inter
    den3 = p[:, 3] * p[:, 4] * p[:, 5] + q[:, 3] * q[:, 4] * q[:, 5] - inter3
    with np.errstate(divide="ignore", invalid="ignore"):
        bev = np.where(ok & (den_bev > 0), inter / den_bev, 0.0)
        d3 = np.where(ok & (den3 > 0), inter3 / den3, 0.0)
    return bev.reshape(n, k), d3.reshape(n, k)


def scene_overlaps(dt, gt):
    """[3, nd, ng] = bbox / bev / 3d overlaps of one scene's records."""
    bev, d3 = box_overlaps(dt, gt)
    return np.stack([image_box_iou(dt[:, 7:11], gt[:, 7:11]), bev, d3])


def gt_flags(gt, cls_code, difficulty):
    code, ign = gt[:, 13].astype(np.int64), (gt[:, 12].astype(np.int64) >> difficulty) & 1
    vc = np.where(code == cls_code, 1, np.where(((cls_code == 1) & (code == 4)) | ((cls_code == 0) & (code == 3)), 0, -1))
    return np.where((vc == 1) & (ign == 0), 0, np.where((vc == 0) | ((ign == 1) & (vc == 1)), 1, -1)).astype(np.int64)


def dt_flags(dt, cls_code, difficulty):
    height = np.abs(dt[:, 10] - dt[:, 8])
    return np.where(height < MIN_HEIGHT[difficulty], 1, np.where(dt[:, 13].astype(np.int64) == cls_code, 0, -1)).astype(np.int64)


def dc_iof(dt, gt):
    """max intersection over the detection's area with the scene's DontCare boxes (0 without one), [nd]."""
    dc = gt[gt[:, 13] == _DONTCARE]
    if dt.shape[0] == 0 or dc.shape[0] == 0:
        return np.zeros(dt.shape[0])
    return np.maximum(image_box_iou(dt[:, 7:11], dc[:, 7:11], criterion=0).max(1), 0.0)


def pass1(ov, gf, df, scores, min_overlap):
    """compute_statistics(compute_fp=False) of one scene: the TP scores in GT order."""
    nd = ov.shape[0]
    assigned = np.zeros(nd, bool)
    out = []
    for i in range(ov.shape[1]):
        if gf[i] == -1:
            continue
        cand = np.nonzero((ov[:, i] > min_overlap) & (df != -1) & ~assigned & (scores > NO_DETECTION))[0]
        if cand.size == 0:
            continue
        j = cand[np.argmax(scores[cand])]                        # the first maximum: the lowest index on ties
        if not (gf[i] == 1 or df[j] == 1):
            out.append(scores[j])
        assigned[j] = True
    return out


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    scores = np.sort(np.asarray(scores, np.float64))[::-1]
    current_recall = 0.0
    thresholds = []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < len(scores) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def pass2(ov, gf, df, scores, dcf, thr, min_overlap, is_bbox, do_aos, gt_alpha, dt_alpha):
    """compute_statistics(compute_fp=True) of one scene at every threshold of `thr` at once -> tp, fp, fn int64 [T], sim float64 [T]."""
    T, nd = len(thr), ov.shape[0]
    thr = np.asarray(thr, np.float64)
    assigned = np.zeros((T, nd), bool)
    ign_thr = scores[None, :] < thr[:, None]
    tp, fn = np.zeros(T, np.int64), np.zeros(T, np.int64)
    sim = np.zeros(T)
    for i in range(ov.shape[1]):
        if gf[i] == -1:
            continue
        det, maxov, aig = np.full(T, -1), np.zeros(T), np.zeros(T, bool)
        for j in np.nonzero((ov[:, i] > min_overlap) & (df != -1))[0]:
            ok = ~assigned[:, j] & ~ign_thr[:, j]
            o = ov[j, i]
            if df[j] == 0:
                take = ok & ((o > maxov) | aig)
                maxov = np.where(take, o, maxov)
                aig = np.where(take, False, aig)
            else:
                take = ok & (det < 0)
                aig = np.where(take, True, aig)
            det = np.where(take, j, det)
        has = np.nonzero(det >= 0)[0]
        if gf[i] == 0:
            fn += det < 0
        dj = det[has]
        is_tp = ~((gf[i] == 1) | (df[dj] == 1))
        tp[has[is_tp]] += 1
        if do_aos:
            sim[has[is_tp]] += (1.0 + np.cos(gt_alpha[i] - dt_alpha[dj[is_tp]])) / 2.0
        assigned[has, dj] = True
    elig = (df == 0)[None, :] & ~ign_thr & ~assigned
    fp = elig.sum(1).astype(np.int64)
    if is_bbox:
        fp -= (elig & dcf[None, :]).sum(1)
    if do_aos:
        sim = np.where((tp > 0) | (fp > 0), sim, -1.0)
    else:
        sim = np.zeros(T)
    return tp, fp, fn, sim


def ap_from_counts(tp, fp, sim, nt):
    """precision / aos with the suffix max, -> (AP11, AP40, AOS AP11, AOS AP40) (float64, summed in index order)."""
    prec, aos = np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(nt):
            prec[t] = np.float64(tp[t]) / np.float64(tp[t] + fp[t])
            aos[t] = sim[t] / np.float64(tp[t] + fp[t])
    for t in range(nt):
        prec[t] = np.max(prec[t:])
        aos[t] = np.max(aos[t:])
    out = []
    for v in (prec, aos):
        s11, s40 = 0.0, 0.0
        for i in range(0, N_SAMPLE_PTS, 4):
            s11 = s11 + v[i]
        for i in range(1, N_SAMPLE_PTS):
            s40 = s40 + v[i]
        out += [s11 / 11 * 100, s40 / 40 * 100]
    return out[0], out[1], out[2], out[3]


def host_core(dt, dt_counts, gt, gt_counts, class_ids, metrics, aos, ov=None, dcf=None):
    """float64 restatement of the device path over records (see _encode).  ov / dcf: optional per-scene overlaps [3, nd, ng] and DontCare
    IoF [nd] to use instead of computing them.  -> dict with the same fields as the device path (numpy)."""
    S = len(dt_counts)
    doff, goff = offsets(dt_counts), offsets(gt_counts)
    dts = [dt[doff[s]:doff[s + 1]] for s in range(S)]
    gts = [gt[goff[s]:goff[s + 1]] for s in range(S)]
    if ov is None:
        ov = [scene_overlaps(dts[s], gts[s]) for s in range(S)]
    if dcf is None:
        dcf = [dc_iof(dts[s], gts[s]) for s in range(S)]
    K = len(class_ids)
    gfl = np.zeros((3 * K, gt.shape[0]), np.int64)
    dfl = np.zeros((3 * K, dt.shape[0]), np.int64)
    for ci, c in enumerate(class_ids):
        for d in range(3):
            gfl[ci * 3 + d] = gt_flags(gt, c, d)
            dfl[ci * 3 + d] = dt_flags(dt, c, d)
    nvalid = (gfl == 0).sum(1)
    gfid, gmet, gmin = _groups(class_ids, metrics)
    NG = len(gfid)
    thr = np.zeros((NG, N_SAMPLE_PTS))
    nthr = np.zeros(NG, np.int64)
    tot = np.zeros((NG, 3, N_SAMPLE_PTS), np.int64)
    sim_tot = np.zeros((NG, N_SAMPLE_PTS))
    ap = np.zeros((NG, 4))
    for g in range(NG):
        f, m, mino = gfid[g], gmet[g], gmin[g]
        scores = []
        for s in range(S):
            scores += pass1(ov[s][m], gfl[f, goff[s]:goff[s + 1]], dfl[f, doff[s]:doff[s + 1]], dts[s][:, 12], mino)
        th = get_thresholds(scores, nvalid[f]) if nvalid[f] > 0 else []
        nt = len(th)
        assert nt <= N_SAMPLE_PTS
        nthr[g], thr[g, :nt] = nt, th
        if nt == 0:
            continue
        do_aos = bool(aos) and m == 0
        for s in range(S):
            tp, fp, fn, sm = pass2(ov[s][m], gfl[f, goff[s]:goff[s + 1]], dfl[f, doff[s]:doff[s + 1]], dts[s][:, 12], dcf[s] > mino,
                                   thr[g, :nt], mino, m == 0, do_aos, gts[s][:, 11], dts[s][:, 11])
            tot[g, 0, :nt] += tp
            tot[g, 1, :nt] += fp
            tot[g, 2, :nt] += fn
            for t in range(nt):
                if sm[t] != -1:
                    sim_tot[g, t] += sm[t]
        ap[g] = ap_from_counts(tot[g, 0], tot[g, 1], sim_tot[g], nt)
    return dict(ov=ov, dc_iof=dcf, gt_flag=gfl, dt_flag=dfl, nvalid=nvalid, thr=thr, nthr=nthr, tot=tot, sim=sim_tot, ap=ap)


# --------------------------------------------------------------------------------------------------
# device path
# --------------------------------------------------------------------------------------------------
def _device_core(dt, dt_off, gt, gt_off, dt_counts, gt_counts, class_ids, metrics, aos):
    """dt / gt: float32 records on the device, offsets int32 [S+1] on the device, counts as host lists."""
    from . import native as nv
    dev = dt_off.device
    if dt_counts and max(dt_counts) > 4096:
        raise ValueError("kitti_eval: the device path takes at most 4096 detections per scene")
    lds = max([int(nv.lib().u3d_kitti_pass2_lds(int(a), int(b))) for a, b in zip(dt_counts, gt_counts)] + [0])
    if lds > 160 * 1024:
        raise ValueError(f"kitti_eval: a scene needs {lds} B of LDS in pass 2 (detections x GT too large for the device path)")
    gfid, gmet, gmin = _groups(class_ids, metrics)
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32), device=dev)     # noqa: E731
    r = nv.kitti_eval_core(dt, dt_off, gt, gt_off, i32(class_ids), i32(gfid), i32(gmet), torch.as_tensor(gmin, dtype=torch.float32, device=dev),
                           aos, dt_counts, gt_counts)
    r["ap"] = r["ap"].cpu().numpy()
    return r


def _upload(rec, counts, dev):
    return torch.as_tensor(rec.astype(np.float32), device=dev).reshape(-1, 16), offsets(counts, dev)


# --------------------------------------------------------------------------------------------------
# results
# --------------------------------------------------------------------------------------------------
def _results(ap, class_ids, metrics, aos, logger=None):
    """ap [NG, 4] in _groups order -> (result_str, ret_dict)."""
    K, M = len(class_ids), len(metrics)
    ap = np.asarray(ap, np.float64).reshape(K, 3, M, 2, 4)             # class, difficulty, metric, setting, (AP11, AP40, AOS11, AOS40)
    tables = {}                                                         # (metric name, AP kind) -> [K, 3 difficulties, 2 settings]
    for mi, m in enumerate(metrics):
        for k, kind in enumerate(("AP11", "AP40")):
            tables[(METRICS[m], kind)] = ap[:, :, mi, :, k]
            if METRICS[m] == "bbox" and aos:
                tables[("aos", kind)] = ap[:, :, mi, :, 2 + k]
    order = [x for x in ("bbox", "bev", "3d", "aos") if (x, "AP11") in tables]
    label = {"bbox": "bbox", "bev": "bev ", "3d": "3d  ", "aos": "aos "}
    ret, result = {}, ""
    for kind in ("AP11", "AP40"):
        result += f"\n----------- {kind} Results ------------\n\n"
        for j, c in enumerate(class_ids):
            name = CLASS_TO_NAME[c]
            for i in range(2):
                ov = [MIN_OVERLAPS[i, m, c] for m in range(3)]
                result += "{} {}@{:.2f}, {:.2f}, {:.2f}:\n".format(name, kind, *ov)
                for x in order:
                    v = tables[(x, kind)][j, :, i]
                    fmt = "{:.2f}" if x == "aos" else "{:.4f}"
                    result += f"{label[x]} {kind}:" + ", ".join(fmt.format(float(a)) for a in v) + "\n"
                    for d in range(3):
                        ret[_KEYS["cls"].format(cls=name, metric=_KEYS["metric"][x], ap=kind, difficulty=DIFFICULTY[d],
                                                setting=SETTINGS[i])] = float(v[d])
        if K > 1:
            result += "\nOverall {}@{}, {}, {}:\n".format(kind, *DIFFICULTY)
            for x in order:
                mean = tables[(x, kind)].mean(axis=0)[:, 0]
                fmt = "{:.2f}" if x == "aos" else "{:.4f}"
                result += f"{label[x]} {kind}:" + ", ".join(fmt.format(float(a)) for a in mean) + "\n"
                for d in range(3):
                    ret[_KEYS["overall"].format(metric=_KEYS["metric"][x], ap=kind, difficulty=DIFFICULTY[d])] = float(mean[d])
    if logger is not None:
        print_log(result, logger)
    return result, ret


def _metric_ids(eval_types):
    ids = [METRICS.index(t) for t in ("bbox", "bev", "3d") if t in eval_types]
    unknown = set(eval_types) - set(METRICS) - {"aos"}
    if unknown or not ids:
        raise ValueError(f"kitti_eval: eval_types must be drawn from {METRICS}, got {tuple(eval_types)}")
    return ids


def evaluate_records(dt, dt_counts, gt, gt_counts, class_ids, metrics, aos, device="cpu"):
    """Array-level entry over float64 records (see _encode) -> dict with ap [NG, 4], thr / nthr, tot [NG, 3, 41], flags, overlaps."""
    dev = torch.device(device)
    if dev.type == "cpu":
        return host_core(dt, list(dt_counts), gt, list(gt_counts), class_ids, metrics, aos)
    d, doff = _upload(dt, dt_counts, dev)
    g, goff = _upload(gt, gt_counts, dev)
    return _device_core(d, doff, g, goff, list(dt_counts), list(gt_counts), class_ids, metrics, aos)


def kitti_eval(gt_annos, dt_annos, current_classes, eval_types=("bbox", "bev", "3d"), device=None):
    """mmdet3d's kitti_eval: -> (result_str, ret_dict).  device: None = the GPU when there is one, "cpu" = the float64 host path."""
    assert len(gt_annos) == len(dt_annos), "kitti_eval: one dt anno per GT anno"
    class_ids = _class_ids(current_classes)
    metrics = _metric_ids(eval_types)
    gt, gc = _encode_all(gt_annos, True)
    dt, dc = _encode_all(dt_annos, False)
    aos = _compute_aos(gt_annos, dt_annos) and 0 in metrics
    r = evaluate_records(dt, dc, gt, gc, class_ids, metrics, aos, default_device(device))
    return _results(r["ap"], class_ids, metrics, aos)


# --------------------------------------------------------------------------------------------------
# LiDAR results -> KITTI annos
# --------------------------------------------------------------------------------------------------
def _calib(info):
    c = info["calib"]
    T = np.asarray(c["R0_rect"], np.float64).reshape(4, 4) @ np.asarray(c["Tr_velo_to_cam"], np.float64).reshape(4, 4)
    return T, np.asarray(c["P2"], np.float64).reshape(4, 4), np.asarray(info["image"]["image_shape"], np.float64).reshape(-1)[:2]


def camera_corners(loc, dims, ry):
    """[n, 8, 3] corners of camera boxes: local x in +-l/2, y in {-h, 0}, z in +-w/2, turned by R_y = [[c,0,s],[0,1,0],[-s,0,c]]."""
    loc, dims, ry = np.asarray(loc, np.float64).reshape(-1, 3), np.asarray(dims, np.float64).reshape(-1, 3), np.asarray(ry, np.float64).reshape(-1)
    k = np.arange(8)
    lx = np.where(k & 1, 0.5, -0.5)[None] * dims[:, :1]
    ly = np.where(k & 2, -1.0, 0.0)[None] * dims[:, 1:2]
    lz = np.where(k & 4, 0.5, -0.5)[None] * dims[:, 2:3]
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    return np.stack([c * lx + s * lz, ly, -s * lx + c * lz], -1) + loc[:, None, :]


def project_bbox(loc, dims, ry, P2):
    """2-D box (min / max of the 8 projected corners) [n, 4]."""
    cr = camera_corners(loc, dims, ry)
    h = np.concatenate([cr, np.ones(cr.shape[:2] + (1,))], -1) @ np.asarray(P2, np.float64).reshape(4, 4).T
    uv = h[..., :2] / h[..., 2:3]
    return np.concatenate([uv.min(1), uv.max(1)], -1) if cr.shape[0] else np.zeros((0, 4))


def _empty_anno(sample_idx):
    return dict(name=np.array([]), truncated=np.array([]), occluded=np.array([]), alpha=np.array([]), bbox=np.zeros([0, 4]),
                dimensions=np.zeros([0, 3]), location=np.zeros([0, 3]), rotation_y=np.array([]), score=np.array([]),
                sample_idx=np.array([], np.int64) if sample_idx is None else np.full(0, sample_idx, np.int64))


def _scene(info):
    """what the conversion needs of one info: (T, P2, image (H, W), image_idx or None, the device path's calibration row T | P2)"""
    T, P2, hw = _calib(info)
    return T, P2, hw, info.get("image", {}).get("image_idx"), np.concatenate([T.reshape(-1), P2.reshape(-1)])


def _host_buffer():
    return DetBuffer(7, torch.float64, "cpu", short=_SHORT)


def lidar_results_to_kitti(results, infos, class_names, pcd_limit_range=(0, -40, -3, 70.4, 40, 0.0)):
    """`Uni3DETR.simple_test` results (LiDAR bottom-centre boxes, counter-clockwise yaw) -> KITTI dt annos, the float64 counterpart of
    KittiDataset.bbox2result_kitti + convert_valid_bboxes (infos: mmdet3d KITTI info dicts with calib / image)."""
    assert len(results) == len(infos)
    buf = _host_buffer()
    for res in results:
        buf.add(res)
    return _buffer_to_kitti(buf, [_scene(i) for i in infos], class_names, pcd_limit_range)


def _buffer_to_kitti(buf, scenes, class_names, pcd_limit_range):
    """lidar_results_to_kitti over a host DetBuffer (float64) and the scenes' _scene() tuples"""
    boxes, scores, labels, off = (t.numpy() for t in buf.cat())
    raise_invalid(invalid_host(scores, labels, len(class_names)), ERRORS)
    lim = np.asarray(pcd_limit_range, np.float64)
    out = []
    for s, (T, P2, hw, sample_idx, _) in enumerate(scenes):
        b, sc, lab = boxes[off[s]:off[s + 1]], scores[off[s]:off[s + 1]], labels[off[s]:off[s + 1]]
        loc = np.concatenate([b[:, :3], np.ones((b.shape[0], 1))], 1) @ T.T
        loc = loc[:, :3]
        dims = b[:, [3, 5, 4]]
        ry = -b[:, 6] - np.pi / 2
        bbox = project_bbox(loc, dims, ry, P2)
        H, W = hw
        keep = (bbox[:, 0] < W) & (bbox[:, 1] < H) & (bbox[:, 2] > 0) & (bbox[:, 3] > 0)
        keep &= ((b[:, :3] > lim[:3]) & (b[:, :3] < lim[3:])).all(1)
        if not keep.any():
            out.append(_empty_anno(sample_idx))
            continue
        bbox = bbox[keep]
        bbox[:, :2] = np.maximum(bbox[:, :2], 0)
        bbox[:, 2:] = np.minimum(bbox[:, 2:], [W, H])
        bl = b[keep]
        anno = dict(name=np.array([class_names[int(l)] for l in lab[keep]]), truncated=np.zeros(int(keep.sum())),
                    occluded=np.zeros(int(keep.sum()), np.int64), alpha=-np.arctan2(-bl[:, 1], bl[:, 0]) + ry[keep], bbox=bbox,
                    dimensions=dims[keep], location=loc[keep], rotation_y=ry[keep], score=sc[keep])
        anno["sample_idx"] = np.full(int(keep.sum()), -1 if sample_idx is None else sample_idx, np.int64)
        out.append(anno)
    return out


class KittiEvaluator:
    """Streaming KITTI evaluation over `simple_test` batches.

    add(results, infos) keeps the detections on `device` (LiDAR boxes, scores, labels) and encodes the GT annos of `infos` once on the
    host (records with class codes, difficulty ignore bits and the DontCare rows), with the scenes' calibration rows.  compute() converts
    every detection to KITTI format on the device and runs the evaluation once over everything added, so any batching of the same scenes
    gives bit-identical results."""

    def __init__(self, class_names, eval_types=("bbox", "bev", "3d"), device="cuda", pcd_limit_range=(0, -40, -3, 70.4, 40, 0.0)):
        self.class_names = list(class_names)
        self.class_ids = _class_ids(self.class_names)
        self.metrics = _metric_ids(eval_types)
        self.device = torch.device(device)
        self.pcd_limit_range = tuple(float(v) for v in pcd_limit_range)
        self.reset()

    def reset(self):
        on_host = self.device.type == "cpu"                                # the host path is the float64 restatement
        self._det = DetBuffer(7, torch.float64 if on_host else torch.float32, self.device, short=_SHORT)
        self._gt, self._gt_counts, self._gt_alpha0, self._scenes = [], [], [], []

    def __len__(self):
        return len(self._gt_counts)

    def add(self, results, infos):
        assert len(results) == len(infos)
        for res in results:
            self._det.add(res)
        self._add_infos(infos)

    def _add_infos(self, infos):
        """per scene: what the conversion needs of its calibration, and the encoded GT"""
        for info in infos:
            self._scenes.append(_scene(info))
            g = _encode(info["annos"], True)
            self._gt.append(g)
            self._gt_counts.append(g.shape[0])
            self._gt_alpha0.append(g[0, 11] if g.shape[0] else None)

    def add_store(self, store, infos):
        """add() for every scene of a det_store.DetStore at once, in the store's scene order: the detections are store.packed() (they
        never leave the device), the per-scene counts come from one read of its det_off; infos: one per scene of the store.
        Bit-identical to add() over the same scenes in the same order."""
        self._det.add_store(store, len(infos), f"KittiEvaluator.add_store: the store holds {{n}} scenes, {len(infos)} infos were given",
                            len(self.class_names), ERRORS)
        self._add_infos(infos)

    def compute(self, logger="silent"):
        """-> ret_dict of `kitti_eval` over everything added (the result string goes to `logger`)."""
        if not len(self):
            raise ValueError("KittiEvaluator.compute: nothing was added")
        gt = np.concatenate(self._gt)
        valid_alpha_gt = any(a is not None and a != -10 for a in self._gt_alpha0)
        if self.device.type == "cpu":
            dt_annos = _buffer_to_kitti(self._det, self._scenes, self.class_names, self.pcd_limit_range)
            dt, dc = _encode_all(dt_annos, False)
            aos = valid_alpha_gt and any(np.any(a["alpha"] != -10) for a in dt_annos) and 0 in self.metrics
            r = host_core(dt, dc, gt, self._gt_counts, self.class_ids, self.metrics, aos)
            return _results(r["ap"], self.class_ids, self.metrics, aos, logger)[1]
        from . import native as nv
        dev = self.device
        boxes, scores, labels, off = self._det.cat()
        raise_invalid(invalid_device(scores, labels, len(self.class_names)), ERRORS)
        calib = torch.as_tensor(np.asarray([s[4] for s in self._scenes], np.float32).reshape(-1, 32), device=dev)
        img = torch.as_tensor(np.asarray([s[2] for s in self._scenes], np.float32).reshape(-1, 2), device=dev)
        codes = torch.as_tensor(_codes(self.class_names).astype(np.int32), device=dev)
        lim = torch.as_tensor(np.asarray(self.pcd_limit_range, np.float32), device=dev)
        dt, dt_off = nv.kitti_convert(boxes, scores, labels, off, calib, img, codes, lim)
        dt_counts = np.diff(dt_off.cpu().numpy()).tolist()
        aos = valid_alpha_gt and bool((dt[:, 11] != -10).any()) and 0 in self.metrics
        g, goff = _upload(gt, self._gt_counts, dev)
        r = _device_core(dt, dt_off, g, goff, dt_counts, list(self._gt_counts), self.class_ids, self.metrics, aos)
        return _results(r["ap"], self.class_ids, self.metrics, aos, logger)[1]
