"""A NumPy restatement of u3d_det_store_merge, written from the header's text (include/u3d_hip.h is the contract), on the RefStore of
tests/det_store_ref.py; and the wire form of a list of RefStores, as an all-gather of their packs leaves it."""
import numpy as np

from det_store_ref import RefStore


def wire(stores, Nmax=None, Smax=None, pad_f=0.0, pad_i=0):
    """[RefStore, ...] -> sh_boxes [W, Nmax, D], sh_scores, sh_labels [W, Nmax], sh_off [W, Smax + 1], sh_head [W, 2]: every store's
    pack() padded (with pad_f / pad_i) to common sizes - the largest of them unless given"""
    packs = [s.pack() for s in stores]
    W, D = len(stores), stores[0].D
    Nmax = max(1, max(p[0].shape[0] for p in packs)) if Nmax is None else Nmax
    Smax = max(p[3].shape[0] - 1 for p in packs) if Smax is None else Smax
    sh_boxes = np.full((W, Nmax, D), pad_f, np.float32)
    sh_scores = np.full((W, Nmax), pad_f, np.float32)
    sh_labels = np.full((W, Nmax), pad_i, np.int32)
    sh_off = np.full((W, Smax + 1), pad_i, np.int32)
    sh_head = np.zeros((W, 2), np.int32)
    for w, (b, s, l, off, _) in enumerate(packs):
        n = b.shape[0]
        sh_boxes[w, :n], sh_scores[w, :n], sh_labels[w, :n], sh_off[w, :off.shape[0]] = b, s, l, off
        sh_head[w] = (off.shape[0] - 1, n)
    return sh_boxes, sh_scores, sh_labels, sh_off, sh_head


def merge(dst, sh_boxes, sh_scores, sh_labels, sh_off, sh_head, scene_map):
    """u3d_det_store_merge into the RefStore `dst`; -> False when the call is refused (then only dst.cursor[3] moved)"""
    W, Nmax, _ = sh_boxes.shape
    Smax = sh_off.shape[1] - 1
    n = scene_map.shape[0]
    scenes, rows = int(dst.cursor[0]), int(dst.cursor[1])
    refuse = not (0 <= scenes <= dst.S) or rows < 0
    refuse |= any(not (0 <= int(hs) <= Smax and 0 <= int(hr) <= Nmax) for hs, hr in sh_head)
    runs = []
    for w, l in scene_map.tolist():
        if not 0 <= w < W or not 0 <= l < int(sh_head[w, 0]):
            refuse = True
            continue
        hr = int(sh_head[w, 1])
        a, b = (min(max(int(v), 0), hr) for v in sh_off[w, l:l + 2])        # the shard's offsets, clamped into [0, its rows]
        runs.append((w, a, max(b - a, 0)))
    refuse |= scenes + n > dst.S or rows + sum(c for _, _, c in runs) > dst.R
    if refuse:
        dst.cursor[3] += 1
        return False
    for i, (w, a, c) in enumerate(runs):
        dst.boxes[rows:rows + c], dst.scores[rows:rows + c] = sh_boxes[w, a:a + c], sh_scores[w, a:a + c]
        dst.labels[rows:rows + c] = sh_labels[w, a:a + c]
        dst.table[scenes + i] = (rows, c)
        rows += c
    dst.cursor[0], dst.cursor[1] = scenes + n, rows
    return True


def merged(stores, scene_map, S=None, R=None):
    """a fresh RefStore holding the merge of `stores` (S / R default to exactly what it needs, at least 1)"""
    w = wire(stores)
    S = max(scene_map.shape[0], 1) if S is None else S
    R = max(int(w[4][:, 1].sum()), 1) if R is None else R
    dst = RefStore(S, R, stores[0].D, 0)
    assert merge(dst, *w, scene_map)
    return dst
