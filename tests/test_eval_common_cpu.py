"""The evaluators' shared input handling (uni3detr_amd.eval_common): the detection buffer gives the same tensors for any batching of the
same scenes, empty scenes included; every accepted form of one result unwraps to the same triple; a float64 input survives a float64
host buffer bit for bit; the per-scene cap and each evaluator's two messages come out the same from add(), add_store() and compute().
No GPU: the device halves of the message checks are in tests/test_det_store_gpu.py."""
import numpy as np
import pytest
import torch

from uni3detr_amd import eval_common as ec
from uni3detr_amd import evaluation as ev
from uni3detr_amd import kitti_eval as ke
from uni3detr_amd import nuscenes_eval as ne
from uni3detr_amd.synth import eval_scenes, kitti_scenes, nusc_samples

COUNTS = [0, 3, 0, 5, 2, 0]                     # an empty first, middle and last scene
CAP_MSG = "a scene has {n} detections, more than {cap}"


def _scenes(box_dim, dtype, counts=COUNTS, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=(n, box_dim)).astype(dtype), rng.random(n).astype(dtype), rng.integers(0, 3, n)) for n in counts]


def _packed(scenes, box_dim):
    """what DetStore.packed() hands over: float32 rows, int32 labels and offsets"""
    t = lambda xs, shape, dt: torch.from_numpy(np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt))      # noqa: E731
    return (t([s[0] for s in scenes], (0, box_dim), np.float32), t([s[1] for s in scenes], (0,), np.float32),
            t([s[2] for s in scenes], (0,), np.int32), torch.from_numpy(ec.offsets([len(s[1]) for s in scenes])))


def _same(a, b):
    assert a.counts == b.counts and len(a) == len(b)
    for x, y in zip(a.cat(), b.cat()):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


def _unwrap(*a, **k):
    """unwrap() answers in NumPy on the host; as tensors, the comparisons below read the same for both"""
    return tuple(torch.as_tensor(x) for x in ec.unwrap(*a, **k))


class _Box:
    def __init__(self, t):
        self.tensor = t


class StubStore:
    """results() with DetStore's contract: the two checks with the caller's messages, then one dict per scene"""

    def __init__(self, scenes):
        self.scenes = scenes

    def results(self, num_classes=0, errors=None):
        for _, s, l in self.scenes:
            if not np.all(np.isfinite(s)):
                raise ValueError(errors[0])
            if num_classes > 0 and np.any((np.asarray(l) < 0) | (np.asarray(l) >= num_classes)):
                raise ValueError(errors[1])
        return [dict(boxes_3d=torch.as_tensor(b), scores_3d=torch.as_tensor(s), labels_3d=torch.as_tensor(l).long()) for b, s, l in self.scenes]


# ---- the buffer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_dim,dtype", [(7, torch.float32), (9, torch.float64)])
def test_any_batching_gives_the_same_cat(box_dim, dtype):
    scenes = _scenes(box_dim, np.float32)                                   # float32 values: what a store holds
    one = ec.DetBuffer(box_dim, dtype, "cpu")
    for s in scenes:
        one.add(s)
    whole = ec.DetBuffer(box_dim, dtype, "cpu")
    whole.add_packed(*_packed(scenes, box_dim))
    mix = ec.DetBuffer(box_dim, dtype, "cpu")
    mix.add(dict(boxes_3d=scenes[0][0], scores_3d=scenes[0][1], labels_3d=scenes[0][2]))
    mix.add_packed(*_packed(scenes[1:4], box_dim))
    mix.add_packed(*_packed([], box_dim))                                   # a store without scenes adds nothing
    for s in scenes[4:]:
        mix.add(s)
    _same(whole, one)
    _same(mix, one)
    boxes, scores, labels, off = one.cat()
    assert boxes.dtype == dtype and scores.dtype == dtype and labels.dtype == torch.int64 and off.dtype == torch.int32
    assert boxes.shape == (sum(COUNTS), box_dim) and off.tolist() == np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
    assert np.array_equal(boxes.numpy(), np.concatenate([s[0] for s in scenes]).astype(boxes.numpy().dtype))
    assert one.counts == COUNTS and len(one) == len(COUNTS)


def test_a_buffer_of_empty_scenes_and_an_empty_buffer():
    buf = ec.DetBuffer(9, torch.float64, "cpu")
    boxes, scores, labels, off = buf.cat()
    assert len(buf) == 0 and boxes.shape == (0, 9) and scores.shape == (0,) and labels.shape == (0,) and off.tolist() == [0]
    buf.add((np.zeros((0, 9)), [], []))
    buf.add_packed(*_packed(_scenes(9, np.float32, [0, 0]), 9))
    boxes, scores, labels, off = buf.cat()
    assert len(buf) == 3 and buf.counts == [0, 0, 0] and off.tolist() == [0, 0, 0, 0]
    assert boxes.shape == (0, 9) and boxes.dtype == torch.float64 and scores.shape == (0,) and labels.dtype == torch.int64


def test_every_result_form_unwraps_to_the_same_triple():
    b, s, l = _scenes(9, np.float32, [4])[0]
    want = _unwrap((b, s, l), 7, torch.float32, "cpu")
    assert want[0].shape == (4, 7) and np.array_equal(want[0].numpy(), b[:, :7])          # more columns than box_dim are cut
    assert want[1].dtype == torch.float32 and want[2].dtype == torch.int32
    d = dict(boxes_3d=b, scores_3d=s, labels_3d=l)
    tb, ts, tl = torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(l)
    forms = [d, dict(pts_bbox=d), [b, s, l], dict(boxes_3d=tb, scores_3d=ts, labels_3d=tl), dict(boxes_3d=_Box(tb), scores_3d=ts, labels_3d=tl),
             dict(pts_bbox=dict(boxes_3d=_Box(tb), scores_3d=s.tolist(), labels_3d=l.tolist())), (b, s[:, None], l[None])]
    for f in forms:
        for x, y in zip(_unwrap(f, 7, torch.float32, "cpu"), want):
            assert x.dtype == y.dtype and torch.equal(x, y)
    got = _unwrap(dict(img_bbox=d), 7, torch.float32, "cpu", result_name="img_bbox")
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # a scene without detections, in whatever shape it comes
    for empty in (np.zeros((0, 7)), np.zeros(0), torch.zeros((0, 9)), []):
        e = _unwrap((empty, [], []), 7, torch.float32, "cpu")
        assert e[0].shape == (0, 7) and e[0].dtype == torch.float32 and e[1].shape == (0,) and e[2].shape == (0,)
    # fewer columns: zero-filled for the indoor setting, nuScenes' message for the nuScenes setting
    six = _unwrap((b[:, :6], s, l), 7, torch.float32, "cpu")[0]
    assert np.array_equal(six.numpy()[:, :6], b[:, :6]) and not six.numpy()[:, 6].any()
    with pytest.raises(ValueError) as e:
        ec.unwrap((b[:, :8], s, l), 9, torch.float64, "cpu", short=ne._SHORT)
    assert str(e.value) == ne._SHORT == "nuscenes_eval: boxes_3d must have 9 columns (x, y, z, l, w, h, yaw, vx, vy)"
    with pytest.raises(ValueError) as e:
        ne._pred_buffer("cpu").add_packed(*_packed(_scenes(7, np.float32, [2]), 7))
    assert str(e.value) == ne._SHORT


def test_a_float64_input_survives_a_float64_host_buffer():
    x = np.array([[0.1, 1.0 / 3.0, np.pi, 1e-300, 1.0 + 2.0 ** -40, -2.0 / 3.0, 7.7, 123456789.123456789, 5e-324]])
    assert not np.array_equal(x.astype(np.float32).astype(np.float64), x)
    sc = np.array([1.0 / 7.0])
    for boxes, scores in ((x, sc), (torch.from_numpy(x), torch.from_numpy(sc)), (x.tolist(), sc.tolist()), (_Box(torch.from_numpy(x)), sc)):
        buf = ne._pred_buffer("cpu")
        buf.add(dict(boxes_3d=boxes, scores_3d=scores, labels_3d=[0]))
        b, s, _, _ = buf.cat()
        assert b.dtype == torch.float64 and b.numpy().tobytes() == x.tobytes() and s.numpy().tobytes() == sc.tobytes()
    # the evaluators' own buffers: float64 on the host for KITTI and nuScenes, float32 for the indoor paths and on the devices' side
    assert ke.KittiEvaluator(["Car"], device="cpu")._det.dtype == torch.float64
    assert ne.NuScenesEvaluator(device="cpu")._enc.pred.dtype == torch.float64
    assert ev.IndoorEvaluator(3, device="cpu")._det.dtype == torch.float32


def test_the_cap_raises_from_add_and_from_add_packed_alike():
    scenes = _scenes(7, np.float32, [2, 4, 1])
    a = ec.DetBuffer(7, torch.float32, "cpu", cap=3, cap_message=CAP_MSG)
    a.add(scenes[0])
    with pytest.raises(ValueError) as e1:
        a.add(scenes[1])
    b = ec.DetBuffer(7, torch.float32, "cpu", cap=3, cap_message=CAP_MSG)
    with pytest.raises(ValueError) as e2:
        b.add_packed(*_packed(scenes, 7))
    assert str(e1.value) == str(e2.value) == "a scene has 4 detections, more than 3"
    assert len(a) == 1 and len(b) == 0                                     # the refused scene / store left nothing behind
    b.add_packed(*_packed([scenes[0], scenes[2]], 7))                       # at the cap and below it
    assert b.counts == [2, 1]
    many = dict(boxes_3d=np.zeros((ne.MAX_BOXES_PER_SAMPLE + 1, 9)), scores_3d=np.zeros(ne.MAX_BOXES_PER_SAMPLE + 1),
                labels_3d=np.zeros(ne.MAX_BOXES_PER_SAMPLE + 1, np.int64))
    with pytest.raises(ValueError, match="a sample has 501 predictions, more than 500"):
        ne._pred_buffer("cpu").add(many)


def test_offsets_and_the_validity_flags():
    off = ec.offsets([2, 0, 3])
    assert off.dtype == np.int32 and off.tolist() == [0, 2, 2, 5] and ec.offsets([]).tolist() == [0]
    t = ec.offsets(np.array([2, 0, 3]), "cpu")
    assert t.dtype == torch.int32 and t.tolist() == [0, 2, 2, 5]
    ok, lab = np.array([0.5, 1.0]), np.array([0, 2])
    assert ec.invalid_host(ok, lab, 3) == (False, False, False)
    assert ec.invalid_host(np.array([0.5, np.inf]), lab, 3) == (True, False, False)
    assert ec.invalid_host(ok, (lab, np.array([-1])), 3) == (False, True, False)
    assert ec.invalid_host(ok, lab, 2) == (False, False, True) and ec.invalid_host(ok, lab) == (False, False, False)
    assert ec.invalid_host(np.zeros(0), np.zeros(0, np.int64), 1) == (False, False, False)
    for flags, msg in (((True, True, True), "s"), ((False, True, False), "l"), ((False, False, True), "l")):
        with pytest.raises(ValueError, match=msg):
            ec.raise_invalid(flags, ("s", "l"))
    ec.raise_invalid((False, False, False), ("s", "l"))


# ---- each evaluator's messages, from add() + compute() and from add_store() of a store ------------------------------------------------
S, K, C = 3, 5, 3


def _indoor():
    data = eval_scenes(S, K, C, seed=3)
    dets = [(np.asarray(d[2], np.float32), np.asarray(d[3], np.float32), np.asarray(d[4]).astype(np.int64)) for d in data]
    gt = ([torch.from_numpy(d[0]) for d in data], [torch.from_numpy(d[1]) for d in data])
    return dets, gt, lambda: ev.IndoorEvaluator(C, device="cpu"), (ev.ERRORS[0], ev.ERRORS[2].format(C))


def _kitti():
    infos, results = kitti_scenes(S, det_per_scene=K, seed=4)
    dets = [(np.asarray(r["boxes_3d"], np.float32).reshape(-1, 7)[:K], np.asarray(r["scores_3d"], np.float32)[:K],
             np.asarray(r["labels_3d"]).astype(np.int64)[:K]) for r in results]
    return dets, (infos,), lambda: ke.KittiEvaluator(["Pedestrian", "Cyclist", "Car"], device="cpu"), ke.ERRORS


def _nusc():
    infos, results = nusc_samples(S, preds_per_sample=K, seed=5, class_names=ne.CLASSES[:C])
    dets = [(np.asarray(r["boxes_3d"], np.float32).reshape(-1, 9)[:K], np.asarray(r["scores_3d"], np.float32)[:K],
             np.asarray(r["labels_3d"]).astype(np.int64)[:K]) for r in results]
    return dets, (infos,), lambda: ne.NuScenesEvaluator(ne.CLASSES[:C], device="cpu"), ne.ERRORS


def _spoil(dets, what):
    """scene 1 gets a NaN score or a label one past the classes"""
    out = [tuple(np.copy(x) for x in d) for d in dets]
    assert len(out[1][1]) >= 2
    if what == "score":
        out[1][1][1] = np.nan
    else:
        out[1][2][0] = C
    return out


@pytest.fixture(scope="module", params=[_indoor, _kitti, _nusc], ids=["indoor", "kitti", "nuscenes"])
def family(request):
    return request.param()


@pytest.mark.parametrize("what", ["score", "label"])
def test_the_evaluators_messages_on_the_host(family, what):
    dets, rest, make, errors = family
    want = errors[0] if what == "score" else errors[1]
    assert isinstance(want, str) and want
    bad = _spoil(dets, what)
    good = make()
    good.add(dets, *rest)
    assert len(good) == S and good.compute()                                # the unspoilt scenes do evaluate
    with pytest.raises(ValueError) as e:
        a = make()
        a.add(bad, *rest)
        a.compute()
    assert str(e.value) == want
    with pytest.raises(ValueError) as e:
        b = make()
        b.add_store(StubStore(bad), *rest)
        b.compute()
    assert str(e.value) == want
    via_store = make()
    via_store.add_store(StubStore(dets), *rest)
    assert via_store.compute() == good.compute() or str(via_store.compute()) == str(good.compute())       # NaN entries compare by text


def test_a_scene_count_mismatch_keeps_each_class_its_wording(family):
    dets, rest, make, _ = family
    e = make()
    short = tuple(r[:S - 1] for r in rest)
    with pytest.raises(ValueError) as err:
        e.add_store(StubStore(dets), *short)
    want = {ev.IndoorEvaluator: "IndoorEvaluator.add_store: the store holds 3 scenes, GT was given for 2",
            ke.KittiEvaluator: "KittiEvaluator.add_store: the store holds 3 scenes, 2 infos were given",
            ne.NuScenesEvaluator: "nuscenes_eval: one result per info"}[type(e)]
    assert str(err.value) == want and len(e) == 0
