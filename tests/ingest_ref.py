"""NumPy restatement of the batch ingest (u3d_batch_ingest, uni3detr_amd/csrc/ingest.hip), loop by loop and independent of the
binding: a packed pipeline batch -> the capacity-sized static buffers of a training step."""
import numpy as np


def _live(off, cnt, b):
    seg = int(off[b + 1]) - int(off[b])
    live = seg if cnt is None else int(cnt[b])
    return max(0, min(live, seg))


def batch_ingest(points, scene_off, count, P, cat, gt=None, gt_labels=None, gt_off=None, gt_count=None, G=0, gt_out=None, labels_out=None,
                 flag=0.0):
    """points f32 [n, F], scene_off [B+1], count [B] | None, per-scene capacity P; `cat` f32 [rows >= B*P, F] is written in place (rows
    that receive no point keep what they hold).  With gt_out f32 [rows >= B*G, 7 | 9] / labels_out int32: gt f32 [g, 7 | 9]
    bottom-centre, gt_labels, gt_off, gt_count | None.  -> dict(dst_off int32 [B+1], gt_off int32 [B+1] | None, flag float32 (the
    input flag + 1 when a scene was cut), overflow int32 [2] (points cut, boxes cut; 0 / 1 for this call))."""
    B = len(scene_off) - 1
    dst_off = np.zeros(B + 1, np.int32)
    over = np.zeros(2, np.int32)
    row = 0
    for b in range(B):
        live = _live(scene_off, count, b)
        if live > P:
            over[0] = 1
            live = P
        dst_off[b] = row
        src = int(scene_off[b])
        for k in range(live):
            cat[row] = points[src + k]
            row += 1
    dst_off[B] = row
    assert row <= B * P
    gt_off_out = None
    if gt_out is not None:
        gd = gt_out.shape[1]
        gt_off_out = np.zeros(B + 1, np.int32)
        row = 0
        has = gt is not None and len(gt) > 0
        for b in range(B):
            gt_off_out[b] = row
            if not has:
                continue
            live = _live(gt_off, gt_count, b)
            if live > G:
                over[1] = 1
                live = G
            src = int(gt_off[b])
            for k in range(live):
                r = gt[src + k]
                o = np.zeros(gd, np.float32)
                o[0], o[1] = r[0], r[1]
                o[2] = np.float32(r[2]) + np.float32(r[5]) * np.float32(0.5)        # bottom centre -> gravity centre
                o[3:7] = r[3:7]
                if gd == 9 and len(r) == 9:
                    o[7:9] = r[7:9]
                gt_out[row] = o
                labels_out[row] = gt_labels[src + k]
                row += 1
        gt_off_out[B] = row
        assert row <= B * G
    return dict(dst_off=dst_off, gt_off=gt_off_out, flag=np.float32(flag) + np.float32(1.0 if over.any() else 0.0), overflow=over)
