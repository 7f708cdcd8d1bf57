"""The detection store on the GPU (uni3detr_amd.det_store.DetStore, u3d_det_store_append / u3d_det_store_pack): appends, refusals and
repairs bit for bit against the NumPy restatement of tests/det_store_ref.py on a store pre-filled with poison, no host synchronisation
and graph capture of append (its graph: two nodes, one edge), shapes past one step of every scan loop, the argument checks, the three evaluators' add_store against add(), and testing.test_dataset end to end
against the per-batch loop step.results() + IndoorEvaluator.add() under the same seeds, once with an invalid batch in the middle.

Every comparison here is equality: the store moves bytes, it computes nothing."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import det_store_ref as ref
import projects.mmdet3d_plugin  # noqa: F401
from test_bn_fold_cpu import tiny_cfg
from test_varlen_gpu import _no_host_sync
from uni3detr_amd import evaluation as ev
from uni3detr_amd import kitti_eval as ke
from uni3detr_amd import native as nv
from uni3detr_amd import nuscenes_eval as ne
from uni3detr_amd import testing
from uni3detr_amd.det_store import DetStore
from uni3detr_amd.inference import InferenceModel, InferenceStep
from uni3detr_amd.synth import eval_scenes, kitti_scenes, nusc_samples, room_scene

pytestmark = pytest.mark.gpu
NB, K = 3, 5
SEED = 77


def _poisoned(cuda, S, D, R=None, M=4, max_num=K):
    st = DetStore(S, max_num, D, cuda, row_capacity=R, invalid_capacity=M)
    st.boxes.fill_(float("nan"))
    st.scores.fill_(float("nan"))
    for t in (st.labels, st.table, st.invalid):
        t.fill_(ref.POISON_I)
    return st, ref.RefStore(S, st.row_capacity, D, M)


def _det(arrays, cuda):
    b, s, l, c = (torch.from_numpy(a).to(cuda) for a in arrays)
    return nv.DetBatch(b, s, l, c, None)


def _i32(v, cuda):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=cuda)


def _buffers(st):
    return {k: getattr(st, k).cpu().numpy() for k in ("boxes", "scores", "labels", "table", "invalid", "cursor")}


def _assert_store(st, want):
    """every byte of the store - poison past the used rows, untouched table and invalid entries included"""
    got = _buffers(st)
    for k, w in want.arrays().items():
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w, equal_nan=True), k


def _assert_packed(st, want, num_classes=0):
    got = st.packed(num_classes)
    for name, g, w in zip(("boxes", "scores", "labels", "off"), got, want.pack(num_classes=num_classes)[:4]):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


# ---- 1: append against the restatement ----------------------------------------------------------------------------------------------
def _assert_raw_pack(st, want):
    """u3d_det_store_pack on the buffers as they are - unrepaired invalid scenes are empty scenes - against the restatement's pack"""
    scenes, rows = int(want.cursor[0]), int(want.cursor[1])
    got = [t.cpu().numpy() for t in nv.det_store_pack(st.boxes, st.scores, st.labels, st.table, scenes, rows)]
    n = int(got[3][-1])                                                    # the outputs are sized by the rows in use; orphaned rows leave a tail
    assert n <= rows
    for name, g, w in zip(("boxes", "scores", "labels", "off", "bad"), [g[:n] for g in got[:3]] + got[3:], want.pack()):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


@pytest.mark.parametrize("D", [7, 9])
def test_append_matches_restatement(cuda, D):
    rng = np.random.default_rng(D)
    cases = [(n, v) for n in range(4) for v in (1, 0)]
    repaired = 0
    for seq in range(6):
        st, want = _poisoned(cuda, 4 * NB, D)
        calls = [cases[i] for i in rng.choice(len(cases), 4, replace=False)]
        if seq == 0:
            calls = [(3, 1), (2, 0), (None, None), (1, 1)]                 # the null forms of n_live and valid
        if seq == 1:
            calls = [(2, 1), (0, 1), (3, 1), (1, 1)]                       # all valid: padding scenes and a call without live scenes
        for n_live, valid in calls:
            arrays = ref.random_det(rng, NB, K, D)
            want.append(*arrays, n_live=n_live, valid=valid)
            st.append(_det(arrays, cuda), n_live=_i32(n_live, cuda), valid=_i32(valid, cuda))
        _assert_store(st, want)
        _assert_raw_pack(st, want)                                         # every sequence: the pack as the buffers stand
        assert len(st) == int(want.cursor[0])
        invalid = [tuple(r) for r in want.invalid[:want.cursor[2]].tolist()]
        assert st.invalid_batches() == invalid
        if invalid:
            with pytest.raises(RuntimeError, match="still empty"):
                st.packed()
        for first, n in invalid:                                           # the same repair on both sides, then packed() itself
            arrays = ref.random_det(rng, n, K, D, counts=rng.integers(0, K + 1, n))
            st.put(first, _det(arrays, cuda))
            want.append(*arrays, scene_ids=np.arange(first, first + n, dtype=np.int32))
            repaired += 1
        _assert_store(st, want)
        _assert_packed(st, want)
    assert repaired >= 3                                                   # the draws do contain invalid calls with live scenes


def test_counts_are_read_clamped(cuda):
    st, want = _poisoned(cuda, 4, 7)
    b, s, l, _ = ref.random_det(np.random.default_rng(1), NB, K, 7, counts=[K, K, K])
    arrays = (b, s, l, np.array([-2, K + 4, 3], np.int32))
    want.append(*arrays)
    st.append(_det(arrays, cuda))
    _assert_store(st, want)
    assert want.table[:3].tolist() == [[0, 0], [0, K], [K, 3]]


# ---- 2: refusal ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["scenes", "rows"])
def test_a_call_that_does_not_fit_writes_nothing(cuda, what):
    rng = np.random.default_rng(2)
    if what == "scenes":
        st, want = _poisoned(cuda, 4, 7)
        first, second = ref.random_det(rng, NB, K, 7), ref.random_det(rng, NB, K, 7)
    else:
        st, want = _poisoned(cuda, 8, 7, R=9)
        first, second = ref.random_det(rng, NB, K, 7, counts=[K, 0, 2]), ref.random_det(rng, NB, K, 7, counts=[1, 0, 2])
    assert want.append(*first) and not want.append(*second)
    st.append(_det(first, cuda))
    before = _buffers(st)
    st.append(_det(second, cuda))
    after = _buffers(st)
    for k in ("boxes", "scores", "labels", "table", "invalid"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    assert after["cursor"].tolist() == before["cursor"][:3].tolist() + [1]
    _assert_store(st, want)
    with pytest.raises(RuntimeError, match="scene_capacity = %d, row_capacity = %d" % (st.scene_capacity, st.row_capacity)):
        st.packed()
    with pytest.raises(RuntimeError, match="refused"):
        st.results()


# ---- 3: repair -------------------------------------------------------------------------------------------------------------------------
def test_put_repairs_an_invalid_call(cuda):
    rng = np.random.default_rng(3)
    a, b, c = (ref.random_det(rng, NB, K, 9) for _ in range(3))
    st, want = _poisoned(cuda, 3 * NB, 9)
    clean, all_valid = _poisoned(cuda, 3 * NB, 9)
    for arrays, valid in ((a, 1), (b, 0), (c, 1)):
        gated = arrays if valid else tuple(np.zeros_like(x) for x in arrays)          # what the gate leaves of an invalid replay
        st.append(_det(gated, cuda), valid=_i32(valid, cuda))
        want.append(*gated, valid=valid)
        clean.append(_det(arrays, cuda))
        all_valid.append(*arrays)
    with pytest.raises(RuntimeError, match="still empty"):
        st.packed()
    with pytest.raises(ValueError, match="not reported"):
        st.put(0, _det(a, cuda))                                                       # a valid range
    with pytest.raises(ValueError, match="not reported"):
        st.put(NB, _det(b, cuda).to_list()[:2])                                        # part of the invalid range
    assert st.invalid_batches() == [(NB, NB)]
    per_scene = [(bx, sc, lb) for bx, sc, lb in _det(b, cuda).to_list()]               # the list form; labels come as int64
    st.put(NB, per_scene)
    want.append(*b, scene_ids=np.arange(NB, 2 * NB, dtype=np.int32))
    _assert_store(st, want)
    with pytest.raises(ValueError, match="put already"):
        st.put(NB, per_scene)
    got, ref_clean = st.packed(), clean.packed()
    for name, g, w, r in zip(("boxes", "scores", "labels", "off"), got, ref_clean, all_valid.pack()[:4]):
        assert torch.equal(g, w) and np.array_equal(g.cpu().numpy(), r), name           # = the all-valid sequence
    res = st.results()
    assert len(res) == 3 * NB and [r["scores_3d"].shape[0] for r in res] == np.diff(all_valid.pack()[3]).tolist()
    assert res[0]["labels_3d"].dtype == torch.int64 and not res[0]["boxes_3d"].is_cuda
    # the DetBatch form of put, on a second invalid call
    st.reset()
    want = ref.RefStore(3 * NB, st.row_capacity, 9, 4)
    st.append(_det(tuple(np.zeros_like(x) for x in a), cuda), n_live=_i32(2, cuda), valid=_i32(0, cuda))
    assert st.invalid_batches() == [(0, 2)]
    two = tuple(x[:2] for x in a)
    st.put(0, _det(two, cuda))
    want.append(*tuple(np.zeros_like(x) for x in a), n_live=2, valid=0)
    want.append(*two, scene_ids=np.array([0, 1], np.int32))
    _assert_packed(st, want)
    # rows orphaned by a direct call on the buffers do not come back from packed(): N is det_off[-1], not the cursor's row count
    nv.det_store_append(_det(two, cuda), None, None, torch.tensor([1, 0], dtype=torch.int32, device=cuda), st.boxes, st.scores, st.labels,
                        st.table, st.cursor, st.invalid)
    want.append(*two, scene_ids=np.array([1, 0], np.int32))
    _assert_packed(st, want)
    assert int(st.cursor[1]) == 2 * int(two[3].sum()) and st.packed()[0].shape[0] == int(two[3].sum())


def test_scene_id_past_the_cursor_refuses_at_the_abi(cuda):
    rng = np.random.default_rng(4)
    st, want = _poisoned(cuda, 2 * NB, 7)
    a, b = ref.random_det(rng, NB, K, 7), ref.random_det(rng, NB, K, 7)
    st.append(_det(a, cuda))
    want.append(*a)
    for ids in ([0, NB, 1], [0, -1, 1]):
        ids_t = torch.tensor(ids, dtype=torch.int32, device=cuda)
        nv.det_store_append(_det(b, cuda), None, None, ids_t, st.boxes, st.scores, st.labels, st.table, st.cursor, st.invalid)
        assert not want.append(*b, scene_ids=np.array(ids, np.int32))
    _assert_store(st, want)
    assert want.cursor.tolist()[2:] == [0, 2]
    # an id named twice: the last one wins; the rows of both are appended
    ids = [1, 2, 1]
    nv.det_store_append(_det(b, cuda), None, None, torch.tensor(ids, dtype=torch.int32, device=cuda), st.boxes, st.scores, st.labels,
                        st.table, st.cursor, st.invalid)
    assert want.append(*b, scene_ids=np.array(ids, np.int32))
    _assert_store(st, want)


# ---- 4: no host synchronisation, graph capture -----------------------------------------------------------------------------------
def test_append_runs_without_host_sync_and_in_a_graph(cuda):
    rng = np.random.default_rng(5)
    arrays = ref.random_det(rng, NB, K, 7)
    det, n_live, valid = _det(arrays, cuda), _i32(2, cuda), _i32(1, cuda)
    st, want = _poisoned(cuda, 4 * NB, 7)
    st.append(det, n_live=n_live, valid=valid)                              # (first use: the code object loads)
    torch.cuda.synchronize()
    with _no_host_sync():
        st.append(det, n_live=n_live, valid=valid)
    torch.cuda.synchronize()
    for _ in range(2):
        want.append(*arrays, n_live=2, valid=1)
    _assert_store(st, want)
    # captured alone: a straight line of two kernels; every replay appends, and reads n_live / valid / count as they are then
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        st.append(det, n_live=n_live, valid=valid)
    torch.cuda.synchronize()
    _assert_store(st, want)                                                 # the capture itself appended nothing
    for live, ok in ((3, 1), (1, 0), (2, 1)):
        n_live.fill_(live)
        valid.fill_(ok)
        g.replay()
        want.append(*arrays, n_live=live, valid=ok)
    torch.cuda.synchronize()
    _assert_store(st, want)
    assert want.cursor.tolist()[0] == 2 + 2 + 3 + 1 + 2 and st.invalid_batches() == [(7, 1)]


def _graph_nodes_and_edges(g):
    """(number of nodes, [(from, to), ...]) of a captured graph kept with keep_graph=True, asked of the HIP runtime torch has loaded
    (RTLD_NOLOAD: the library already in the process, never a second copy of it)"""
    hip = C.CDLL("libamdhip64.so", mode=os.RTLD_NOLOAD | os.RTLD_NOW)
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    graph = C.c_void_p(g.raw_cuda_graph())
    n, ne = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and hip.hipGraphGetEdges(graph, None, None, C.byref(ne)) == 0
    frm, to = (C.c_void_p * max(ne.value, 1))(), (C.c_void_p * max(ne.value, 1))()
    assert hip.hipGraphGetEdges(graph, frm, to, C.byref(ne)) == 0
    return n.value, [(frm[i], to[i]) for i in range(ne.value)]


def test_captured_append_is_a_straight_line(cuda):
    """the graph of one captured append: two kernel nodes and the one edge between them - no parallel branches"""
    det, n_live, valid = _det(ref.random_det(np.random.default_rng(8), NB, K, 7), cuda), _i32(2, cuda), _i32(1, cuda)
    st, _ = _poisoned(cuda, 4 * NB, 7)
    st.append(det, n_live=n_live, valid=valid)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        st.append(det, n_live=n_live, valid=valid)
    torch.cuda.synchronize()
    nodes, edges = _graph_nodes_and_edges(g)
    print("captured append:", nodes, "nodes,", len(edges), "edges")
    assert nodes == 2 and len(edges) == 1 and edges[0][0] != edges[0][1], (nodes, edges)


def test_more_than_one_step_of_every_loop(cuda):
    """Shapes past one 64-lane step of k_ds_commit and k_ds_offsets and past one 256-thread stride of the plan: calls of 70 and of 300
    scenes (290 live), an invalid one among them, a repair of 70 scenes with an id named in two different steps, 430 scenes packed."""
    rng = np.random.default_rng(9)
    k = 3
    st, want = _poisoned(cuda, 440, 7, max_num=k)

    def both(B, n_live=None, valid=None, ids=None, full=False):
        arrays = ref.random_det(rng, B, k, 7, counts=np.full(B, k) if full else rng.integers(0, k + 1, B))
        ids_t = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=cuda)
        nv.det_store_append(_det(arrays, cuda), _i32(n_live, cuda), _i32(valid, cuda), ids_t, st.boxes, st.scores, st.labels, st.table,
                            st.cursor, st.invalid)
        return want.append(*arrays, n_live=n_live, valid=valid, scene_ids=None if ids is None else np.array(ids, np.int32))

    assert both(70) and both(300, n_live=290) and both(70, valid=0)
    _assert_store(st, want)
    assert want.cursor.tolist() == [430, int(want.table[:430, 1].sum()), 1, 0] and want.invalid[0].tolist() == [360, 70]
    _assert_raw_pack(st, want)
    ids = list(range(360, 430))
    ids[69] = 361                                                          # scene 361 named in the first and in the second step: the last wins
    assert both(70, ids=ids, full=True)
    assert not both(300, ids=list(range(299)) + [430])                     # a bad id in the plan's second stride refuses the call
    assert not both(70)                                                    # 430 + 70 scenes do not go into 440
    _assert_store(st, want)
    _assert_raw_pack(st, want)
    assert want.cursor.tolist()[2:] == [1, 2] and int(want.pack()[3][-1]) == int(want.cursor[1]) - k        # scene 361's first rows are orphaned


# ---- 5: bad arguments at the ABI ------------------------------------------------------------------------------------------------------
def test_append_refuses_bad_arguments(cuda):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=cuda)                 # noqa: E731
    i32 = torch.int32
    p = nv._ptr
    st = dict(boxes=z(16, 9), scores=z(16), labels=z(16, dt=i32), table=z(4, 2, dt=i32), cursor=z(4, dt=i32), invalid=z(2, 2, dt=i32))

    def call(batch, k, dim, boxes=True, R=16):
        bx, sc, lb, ct = z(2, 5, 9), z(2, 5), z(2, 5, dt=i32), z(2, dt=i32)
        return nv.lib().u3d_det_store_append(p(bx) if boxes else None, p(sc), p(lb), p(ct), batch, k, dim, None, None, None, p(st["boxes"]),
                                             p(st["scores"]), p(st["labels"]), p(st["table"]), p(st["cursor"]), p(st["invalid"]), R, 4, 2,
                                             nv._stream())

    assert call(2, 5, 8) == -1 and call(0, 5, 7) == -1 and call(2, 0, 7) == -1 and call(2, 5, 7, boxes=False) == -1
    assert call(65536, 5, 7) == nv.U3D_ERR_UNSUPPORTED and call(2, nv.DET_TAIL_MAX_K + 1, 7) == nv.U3D_ERR_UNSUPPORTED
    assert call(2, 5, 7, R=2 ** 31 // 7 + 1) == nv.U3D_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for t in st.values())                                     # nothing was launched
    bad = nv.DetBatch(z(2, 5, 8), z(2, 5), z(2, 5, dt=i32), z(2, dt=i32), None)
    with pytest.raises(ValueError, match="box_dim"):
        DetStore(4, 5, 7, cuda).append(bad)
    with pytest.raises(ValueError, match="box_dim"):
        DetStore(4, 5, 8, cuda)
    with pytest.raises(ValueError, match="2\\^31"):
        DetStore(2 ** 20, 512, 7, cuda)


def test_pack_flags_and_capacity_messages(cuda):
    st, want = _poisoned(cuda, NB, 7, M=1)
    b, s, l, c = ref.random_det(np.random.default_rng(6), NB, K, 7, counts=[2, 0, 3])
    l[2, 1] = 7
    st.append(_det((b, s, l, c), cuda))
    want.append(b, s, l, c)
    _assert_packed(st, want, num_classes=8)
    with pytest.raises(ValueError, match="labels must lie in \\[0, 7\\)"):
        st.packed(7)
    with pytest.raises(ValueError, match="their own words"):
        st.packed(7, errors=("", "their own words"))
    st.reset()
    s[0, 1] = np.inf
    st.append(_det((b, s, l, c), cuda))
    with pytest.raises(ValueError, match="scores must be finite"):
        st.packed()
    # more invalid calls than the list holds
    st, _ = _poisoned(cuda, 2 * NB, 7, M=1)
    zero = tuple(np.zeros_like(x) for x in (b, s, l, c))
    for _ in range(2):
        st.append(_det(zero, cuda), valid=_i32(0, cuda))
    with pytest.raises(RuntimeError, match="invalid_capacity = 1"):
        st.invalid_batches()


# ---- 6: the evaluators --------------------------------------------------------------------------------------------------------------
S6, K6, C6 = 6, 8, 3


def _store_of(cuda, per_scene, D, batch=4):
    """per-scene (boxes [n, D], scores [n], labels [n]) NumPy -> a DetStore filled in batches of `batch` scenes, the last one partial"""
    st = DetStore(len(per_scene), K6, D, cuda)
    for i in range(0, len(per_scene), batch):
        chunk = per_scene[i:i + batch]
        pad = chunk + [chunk[0]] * (batch - len(chunk))
        det = nv.DetBatch.from_list([tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in d) for d in pad], K6, D, cuda)
        live = torch.arange(K6, device=cuda)[None, :] < det.count[:, None]
        assert bool((det.scores[~live] == 0).all())
        if len(chunk) < batch:                                               # what the gate does to padding scenes
            det.boxes[len(chunk):], det.scores[len(chunk):], det.labels[len(chunk):], det.count[len(chunk):] = 0, 0, 0, 0
        st.append(det, n_live=_i32(len(chunk), cuda))
    return st


def _quantised(scores):
    return np.maximum(np.round(np.asarray(scores, np.float32) * 4) / 4, 0.25).astype(np.float32)      # ties across scenes


def _same_dict(got, want):
    assert set(got) == set(want)
    for k in want:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])


def test_indoor_add_store_equals_add(cuda):
    data = eval_scenes(S6, K6, C6, seed=21)
    data = [(gt, gl, db[:0], ds[:0], dl[:0]) if s == 2 else (gt, gl, db, _quantised(ds), dl) for s, (gt, gl, db, ds, dl) in enumerate(data)]
    scores = np.concatenate([d[3] for d in data])
    assert len(np.unique(scores)) < scores.size / 2                         # ties do occur
    gts, labs = [torch.from_numpy(d[0]).to(cuda) for d in data], [torch.from_numpy(d[1]).to(cuda) for d in data]
    a = ev.IndoorEvaluator(C6, device=cuda)
    for s in range(0, S6, 4):
        a.add([[torch.from_numpy(d[2]).to(cuda), torch.from_numpy(d[3]).to(cuda), torch.from_numpy(d[4]).to(cuda)] for d in data[s:s + 4]],
              gts[s:s + 4], labs[s:s + 4])
    b = ev.IndoorEvaluator(C6, device=cuda)
    b.add_store(_store_of(cuda, [(d[2], d[3], d[4].astype(np.int32)) for d in data], 7), gts, labs)
    assert len(a) == len(b) == S6
    want = a.compute()
    _same_dict(b.compute(), want)
    assert 0.0 < want["mAP_0.25"] <= 1.0
    with pytest.raises(ValueError, match="holds 6 scenes"):
        b.add_store(_store_of(cuda, [(d[2], d[3], d[4].astype(np.int32)) for d in data], 7), gts[:5], labs[:5])


def test_kitti_add_store_equals_add(cuda):
    classes = ["Pedestrian", "Cyclist", "Car"]
    infos, results = kitti_scenes(S6, det_per_scene=K6, seed=22)
    results = [dict(boxes_3d=r["boxes_3d"][:K6], scores_3d=_quantised(r["scores_3d"][:K6]), labels_3d=r["labels_3d"][:K6]) for r in results]
    results[3] = dict(boxes_3d=np.zeros((0, 7), np.float32), scores_3d=np.zeros(0, np.float32), labels_3d=np.zeros(0, np.int64))
    a = ke.KittiEvaluator(classes, device=cuda)
    for s in range(0, S6, 4):
        a.add(results[s:s + 4], infos[s:s + 4])
    b = ke.KittiEvaluator(classes, device=cuda)
    b.add_store(_store_of(cuda, [(np.asarray(r["boxes_3d"], np.float32).reshape(-1, 7), np.asarray(r["scores_3d"], np.float32),
                                  np.asarray(r["labels_3d"]).astype(np.int32)) for r in results], 7), infos)
    assert len(a) == len(b) == S6
    want = a.compute()
    _same_dict(b.compute(), want)
    assert any(v > 0 for v in want.values())


def test_nuscenes_add_store_equals_add(cuda):
    infos, results = nusc_samples(S6, preds_per_sample=K6, seed=23, class_names=ne.CLASSES[:C6])
    results = [dict(boxes_3d=np.asarray(r["boxes_3d"], np.float32)[:K6], scores_3d=_quantised(r["scores_3d"][:K6]),
                    labels_3d=np.asarray(r["labels_3d"])[:K6]) for r in results]
    results[1] = dict(boxes_3d=np.zeros((0, 9), np.float32), scores_3d=np.zeros(0, np.float32), labels_3d=np.zeros(0, np.int64))
    a = ne.NuScenesEvaluator(ne.CLASSES[:C6], device=cuda)
    for s in range(0, S6, 4):
        a.add(results[s:s + 4], infos[s:s + 4])
    b = ne.NuScenesEvaluator(ne.CLASSES[:C6], device=cuda)
    b.add_store(_store_of(cuda, [(r["boxes_3d"].reshape(-1, 9), r["scores_3d"], r["labels_3d"].astype(np.int32)) for r in results], 9), infos)
    assert len(a) == len(b) == S6
    want = a.compute()
    got = b.compute()
    assert set(got) == set(want)
    for k in want:                                                          # NaN entries (classes without GT) compare by their bytes too
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])


S3 = 3


def _indoor3(cuda):
    data = eval_scenes(S3, K6, C6, seed=31)
    dets = [(np.asarray(d[2], np.float32), np.asarray(d[3], np.float32), np.asarray(d[4]).astype(np.int32)) for d in data]
    rest = ([torch.from_numpy(d[0]).to(cuda) for d in data], [torch.from_numpy(d[1]).to(cuda) for d in data])
    return dets, rest, lambda: ev.IndoorEvaluator(C6, device=cuda), (ev.ERRORS[0], ev.ERRORS[2].format(C6)), 7


def _kitti3(cuda):
    infos, results = kitti_scenes(S3, det_per_scene=K6, seed=32)
    dets = [(np.asarray(r["boxes_3d"], np.float32).reshape(-1, 7)[:K6], np.asarray(r["scores_3d"], np.float32)[:K6],
             np.asarray(r["labels_3d"]).astype(np.int32)[:K6]) for r in results]
    return dets, (infos,), lambda: ke.KittiEvaluator(["Pedestrian", "Cyclist", "Car"], device=cuda), ke.ERRORS, 7


def _nusc3(cuda):
    infos, results = nusc_samples(S3, preds_per_sample=K6, seed=33, class_names=ne.CLASSES[:C6])
    dets = [(np.asarray(r["boxes_3d"], np.float32).reshape(-1, 9)[:K6], np.asarray(r["scores_3d"], np.float32)[:K6],
             np.asarray(r["labels_3d"]).astype(np.int32)[:K6]) for r in results]
    return dets, (infos,), lambda: ne.NuScenesEvaluator(ne.CLASSES[:C6], device=cuda), ne.ERRORS, 9


@pytest.mark.parametrize("family", [_indoor3, _kitti3, _nusc3], ids=["indoor", "kitti", "nuscenes"])
@pytest.mark.parametrize("what", ["score", "label"])
def test_the_evaluators_messages_on_the_device(cuda, family, what):
    """a NaN score and a label one past the classes give the evaluator's one message, the module constant, from the device compute()
    after add() and from add_store() (the store's own check, or compute() where the store is not given the classes)"""
    dets, rest, make, errors, D = family(cuda)
    want = errors[0] if what == "score" else errors[1]
    bad = [tuple(np.copy(x) for x in d) for d in dets]
    assert len(bad[1][1]) >= 2
    if what == "score":
        bad[1][1][1] = np.nan
    else:
        bad[1][2][0] = C6
    with pytest.raises(ValueError) as e:
        a = make()
        a.add([dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in bad], *rest)
        a.compute()
    assert str(e.value) == want
    with pytest.raises(ValueError) as e:
        b = make()
        b.add_store(_store_of(cuda, bad, D, batch=2), *rest)
        b.compute()
    assert str(e.value) == want


def test_nuscenes_add_store_scene_count_mismatch(cuda):
    dets, (infos,), make, _, D = _nusc3(cuda)
    e = make()
    with pytest.raises(ValueError) as err:
        e.add_store(_store_of(cuda, dets, D, batch=2), infos[:2])
    assert str(err.value) == "nuscenes_eval: one result per info" and len(e) == 0
    e.add_store(_store_of(cuda, dets, D, batch=2), infos)
    assert len(e) == S3 and e.compute()


# ---- 7: end to end --------------------------------------------------------------------------------------------------------------------
B7, P7 = 2, 10240


class _World:
    """Model, scenes, GT and one captured step sized to the small scenes at margin 1.0: built once, shared, left unchanged."""

    def __init__(self, cuda):
        from oracle.weights import seeded_tensor
        from uni3detr_amd.registry import build_model
        model = build_model(tiny_cfg())
        model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
        self.model = model.to(cuda).eval().set_precision("bf16")
        self.inf = InferenceModel(self.model)

        def scenes(ids_sizes):
            out = [room_scene(i, n) for i, n in ids_sizes]
            return ([torch.from_numpy(o[0]).to(cuda) for o in out], [torch.from_numpy(o[1]).to(cuda) for o in out],
                    [torch.from_numpy(o[2]).to(cuda) for o in out])

        self.small = scenes([(7, 1200), (8, 1000), (9, 1100), (10, 900), (11, 1300)])       # five scenes of differing size
        self.dense = scenes([(0, 9000), (1, 6500)])
        self.step = InferenceStep(self.inf, batch_size=B7, point_capacity=P7)
        pts = self.small[0]
        self.step.capture(batches=[pts[0:2], pts[2:4], pts[4:5]], margin=1.0, warmup=1)
        self.max_num = int(self.step.det.boxes.shape[1])
        self.num_classes = int(self.model.pts_bbox_head.num_classes)


@pytest.fixture(scope="module")
def world(cuda):
    return _World(cuda)


def _per_batch_loop(world, batches, gts, labs):
    """what a user does today: step.results() and IndoorEvaluator.add() per batch; every forward, the fallback's too, starts from
    torch.manual_seed(SEED + i)"""
    step, inf = world.step, world.inf
    e = ev.IndoorEvaluator(world.num_classes, device=batches[0][0].device)
    orig = inf.simple_test_batched
    inf.simple_test_batched = orig                                          # an instance attribute from here on: `del` restores the method
    k = 0
    try:
        for i, pts in enumerate(batches):
            inf.simple_test_batched = lambda *a, _i=i, **kw: torch.manual_seed(SEED + _i) and orig(*a, **kw)
            torch.manual_seed(SEED + i)
            e.add(step.results(pts), gts[k:k + len(pts)], labs[k:k + len(pts)])
            k += len(pts)
    finally:
        del inf.simple_test_batched
    return e.compute()


def _store_loop(world, batches, gts, labs, reload):
    """the same batches as the packed dicts a feeder yields (the last one partial: the loop itself sends it through run's list form)"""
    from uni3detr_amd import datapath as dp
    cuda = batches[0][0].device
    store = DetStore(sum(len(b) for b in batches), world.max_num, 7, cuda)
    testing.test_dataset(world.step, (dp.pack_batch(b) for b in batches), store, reload=reload, on_batch=lambda i: torch.manual_seed(SEED + i))
    e = ev.IndoorEvaluator(world.num_classes, device=cuda)
    e.add_store(store, gts, labs)
    return store, e.compute()


def test_dataset_loop_equals_the_per_batch_loop(world):
    pts, gts, labs = world.small
    batches = [pts[0:2], pts[2:4], pts[4:5]]                                # two full batches and a partial one
    before = world.step.fallbacks
    want = _per_batch_loop(world, batches, gts, labs)
    store, got = _store_loop(world, batches, gts, labs, None)
    assert world.step.fallbacks == before and store.invalid_batches() == [] and len(store) == 5
    assert sum(r["scores_3d"].shape[0] for r in store.results()) > 0
    _same_dict(got, want)


def test_dataset_loop_repairs_an_invalid_batch(world):
    pts, gts, labs = world.small
    dpts, dgts, dlabs = world.dense
    batches = [pts[0:2], dpts, pts[4:5]]                                    # the middle batch exceeds the captured level capacities
    gts, labs = gts[0:2] + dgts + gts[4:5], labs[0:2] + dlabs + labs[4:5]
    before = world.step.fallbacks
    want = _per_batch_loop(world, batches, gts, labs)
    assert world.step.fallbacks == before + 1                               # ... so the per-batch loop fell back once
    with pytest.raises(RuntimeError, match="batch 1 .*no reload"):
        _store_loop(world, batches, gts, labs, None)
    store, got = _store_loop(world, batches, gts, labs, lambda i: batches[i])
    assert world.step.fallbacks == before + 2 and store.invalid_batches() == [(2, 2)] and len(store) == 5
    _same_dict(got, want)
