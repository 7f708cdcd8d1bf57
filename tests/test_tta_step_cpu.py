"""Test-time augmentation behind the captured step, without a GPU: the padded merge's entry points as the header-derived binding sees
them and their argument checks (answered before any launch), InferenceStep's `views` argument, and test_dataset's sample arithmetic
for views > 1 on stub step / store objects (the pattern of tests/test_det_store_cpu.py)."""
import copy
import ctypes as C

import pytest
import torch

from test_bn_fold_cpu import tiny_cfg
from uni3detr_amd import abi
from uni3detr_amd import native as nv
from uni3detr_amd import testing
from uni3detr_amd.inference import InferenceModel, InferenceStep

P, I, L, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float


def test_padded_merge_is_declared_and_bound():
    p = abi.load().prototypes
    # boxes, scores, labels, count | batch, views, max_det, box_dim | params | coord, num_classes | nms_thr | max_num | workspace, bytes |
    # out_boxes, out_scores, out_labels, out_count, out_off | stream
    assert p["u3d_tta_merge_padded"] == (I, [P] * 4 + [I] * 4 + [P, I, I, F, I, P, L] + [P] * 5 + [P])
    assert len(p["u3d_tta_merge_padded"][1]) == 21
    assert p["u3d_tta_merge_padded_workspace"] == (L, [I] * 5)
    assert p["u3d_tta_merge"][0] is I and len(p["u3d_tta_merge"][1]) == 21 and p["u3d_tta_merge_workspace"] == (L, [I] * 6)     # untouched
    for name in ("u3d_tta_merge_padded", "u3d_tta_merge_padded_workspace"):
        assert name in nv.exported_symbols() and hasattr(C.CDLL(nv.LIB_PATH), name)
    assert callable(nv.tta_merge_padded)


def test_padded_merge_workspace_and_argument_checks_need_no_device():
    ws = nv.lib().u3d_tta_merge_padded_workspace
    small, large = int(ws(2, 4, 150, 7, 3)), int(ws(2, 4, 1000, 7, 3))
    assert 0 < small < large
    # above U3D_TTA_LDS_CAP candidates per sample the suppression masks come on top: [batch][views*K][ceil(views*K / 64)] words
    assert large - int(ws(2, 4, 512, 7, 3)) > 2 * 4000 * 63 * 8
    assert int(ws(2, 4, 512, 7, 3)) < 2 * 4 * 512 * 4 * 32                     # linear in the rows up to the cap
    for bad in ((0, 4, 8, 7, 3), (2, 0, 8, 7, 3), (2, 4, 0, 7, 3), (2, 4, 8, 8, 3), (2, 4, 8, 7, 0), (65536, 4, 8, 7, 3),
                (2, 4, nv.DET_TAIL_MAX_K + 1, 7, 3), (1, 65, nv.DET_TAIL_MAX_K, 7, 3)):
        assert int(ws(*bad)) == -1, bad
    # a null pointer is answered before anything else
    rc = nv.lib().u3d_tta_merge_padded(None, None, None, None, 2, 4, 8, 7, None, 0, 3, 0.1, 500, None, 0, None, None, None, None, None, None)
    assert rc == -1


@pytest.fixture(scope="module")
def inf():
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    return InferenceModel(copy.deepcopy(build_model(tiny_cfg())).set_precision("bf16").eval())


def test_step_checks_views(inf):
    for bad in (0, -1):
        with pytest.raises(ValueError, match="views"):
            InferenceStep(inf, batch_size=2, point_capacity=1024, views=bad)
    with pytest.raises(ValueError, match="tta_max_num"):
        InferenceStep(inf, batch_size=2, point_capacity=1024, views=2, tta_max_num=nv.DET_TAIL_MAX_K + 1)
    step = InferenceStep(inf, batch_size=2, point_capacity=1024, views=4, tta_nms_thr=0.2, tta_max_num=300, box_type_3d="LiDAR")
    assert (step.views, step.tta_nms_thr, step.tta_max_num, step.coord, step.batch_size) == (4, 0.2, 300, 1, 2)
    one = InferenceStep(inf, batch_size=2, point_capacity=1024)
    assert one.views == 1 and one.view_det is None and one.tta_params is None and one.coord is None
    with pytest.raises(RuntimeError, match="capture"):
        step.run([])


# ---- test_dataset on stubs ------------------------------------------------------------------------------------------------------------
class _Scalar:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


class _Inf:
    def __init__(self, log):
        self.log = log

    def aug_test_batched(self, scenes, tta_params=None, views=None, box_type_3d=None, on_device=False, nms_thr=None, max_num=None):
        assert on_device is True and (views, box_type_3d, nms_thr, max_num) == (2, "Depth", 0.1, 500)
        self.log.append(("eager", list(scenes), tta_params))
        return ("eager-det", list(scenes))


class _Step:
    batch_size, views, box_type_3d, tta_nms_thr, tta_max_num = 2, 2, "Depth", 0.1, 500

    def __init__(self, log):
        self.log, self.inf, self.fallbacks = log, _Inf(log), 0
        self.det = self.valid = self.n_live = None

    def run(self, batch, tta_params=None):
        self.log.append(("run", batch, tta_params))
        self.det, self.valid, self.n_live = ("det", len(self.log)), "valid", "n_live"
        return self.det


class _Store:
    def __init__(self, log, invalid=()):
        self.log, self._invalid = log, list(invalid)

    def __len__(self):
        return 0

    def append(self, det, n_live=None, valid=None):
        self.log.append(("append", det))

    def invalid_batches(self):
        return list(self._invalid)

    def put(self, first, dets):
        self.log.append(("put", first, dets))


def _dict_batch(scenes, tag):
    return dict(points=tag, scene_off=_Scalar(scenes + 1), tta_params="tab-" + tag, tta_views=2)


@pytest.fixture()
def stub_scenes(monkeypatch):
    monkeypatch.setattr(testing, "_scenes", lambda b: [b["points"] + str(k) for k in range(b["scene_off"].numel() - 1)] if isinstance(b, dict) else list(b))


def test_loop_counts_samples_not_views(stub_scenes):
    log = []
    step = _Step(log)
    full, part = _dict_batch(4, "a"), _dict_batch(2, "b")                  # B * A = 4 scenes = 2 samples; 2 scenes = 1 sample: partial
    store = _Store(log, invalid=[(0, 2), (2, 1)])
    reloaded = {0: _dict_batch(4, "r"), 1: (["x0", "x1"], "tab-x")}         # the expanded dict, or the views with their table rows
    testing.test_dataset(step, [full, part], store, reload=lambda i: reloaded[i])
    runs = [e for e in log if e[0] == "run"]
    assert runs[0][1] is full and runs[0][2] is None                       # a full dict goes through as it is
    assert runs[1][1:] == (["b0", "b1"], "tab-b")                          # the partial one: its views as a list, with its table rows
    assert [e for e in log if e[0] == "put"] == [("put", 0, ("eager-det", ["r0", "r1", "r2", "r3"])), ("put", 2, ("eager-det", ["x0", "x1"]))]
    assert [e[2] for e in log if e[0] == "eager"] == ["tab-r", "tab-x"] and step.fallbacks == 2
    # a list batch is the pair (views, tta_params)
    log.clear()
    testing.test_dataset(step, [(["p0", "p1", "q0", "q1"], "tab-pq"), (["r0", "r1"], "tab-r")], _Store(log, invalid=[(2, 1)]),
                         reload=lambda i: (["y0", "y1"], "tab-y"))
    assert [e[1:] for e in log if e[0] == "run"] == [(["p0", "p1", "q0", "q1"], "tab-pq"), (["r0", "r1"], "tab-r")]
    assert [e for e in log if e[0] == "put"] == [("put", 2, ("eager-det", ["y0", "y1"]))]
    with pytest.raises(ValueError, match="pair"):
        testing.test_dataset(step, [["p0", "p1"]], _Store(log))


def test_loop_refuses_a_reload_of_the_wrong_sample_count(stub_scenes):
    log = []
    with pytest.raises(RuntimeError, match="returned 2 views = 1 samples of 2 views, batch 0 had 2 samples"):
        testing.test_dataset(_Step(log), [_dict_batch(4, "a")], _Store(log, invalid=[(0, 2)]), reload=lambda i: _dict_batch(2, "r"))
    with pytest.raises(RuntimeError, match="returned 3 views"):
        testing.test_dataset(_Step(log), [_dict_batch(4, "a")], _Store(log, invalid=[(0, 2)]), reload=lambda i: (["a", "b", "c"], "t"))
    with pytest.raises(RuntimeError, match="no reload"):
        testing.test_dataset(_Step(log), [_dict_batch(4, "a")], _Store(log, invalid=[(0, 2)]))
    assert not [e for e in log if e[0] == "put"]


def test_loop_refuses_a_store_narrower_than_the_merged_batch(stub_scenes):
    log = []
    step, store = _Step(log), _Store(log)
    run = step.run

    def wide(batch, tta_params=None):
        run(batch, tta_params)
        step.det = type("Det", (), dict(boxes=torch.zeros(2, 500, 7)))()
        return step.det
    step.run = wide
    store.max_num = 300
    with pytest.raises(ValueError, match="500 rows wide.*max_num = 300.*tta_max_num"):
        testing.test_dataset(step, [_dict_batch(4, "a")], store)
    assert not [e for e in log if e[0] == "append"]
    store.max_num = 500
    testing.test_dataset(step, [_dict_batch(4, "a")], store)
    assert len([e for e in log if e[0] == "append"]) == 1
