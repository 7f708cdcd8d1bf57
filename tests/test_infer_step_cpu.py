"""The captured inference step without a GPU: the header / export / binding triple of u3d_det_gate, its argument checks (answered
before any launch) and InferenceStep's refusals, none of which touches a device."""
import copy
import ctypes as C

import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from test_bn_fold_cpu import tiny_cfg
from uni3detr_amd import abi
from uni3detr_amd import native as nv
from uni3detr_amd.inference import InferenceModel, InferenceStep

P, I = C.c_void_p, C.c_int32
OK, ARG, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def model():
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    return build_model(tiny_cfg()).set_precision("bf16").eval()


def test_det_gate_is_declared_exported_and_bound():
    assert "u3d_det_gate" in nv.exported_symbols()                # = declared in include/u3d_hip.h (tests/test_abi_cpu.py)
    assert hasattr(C.CDLL(nv.LIB_PATH), "u3d_det_gate")
    # flag n_live boxes scores labels count off | batch max_num box_dim | valid stream
    want = (I, [P] * 7 + [I] * 3 + [P, P])
    assert abi.load().prototypes["u3d_det_gate"] == want and len(want[1]) == 12
    fn = nv.lib().u3d_det_gate
    assert fn.restype is want[0] and list(fn.argtypes) == want[1]
    assert callable(nv.det_gate)


def test_det_gate_return_codes():
    buf = (C.c_char * (64 * 9))()
    base = (C.addressof(buf) + 63) & ~63
    h = [C.c_void_p(base + 64 * i) for i in range(8)]             # aligned host addresses the calls never dereference

    def call(batch=2, max_num=5, box_dim=7, null=None):
        a = [None if i == null else p for i, p in enumerate(h)]
        return nv.lib().u3d_det_gate(*a[:7], batch, max_num, box_dim, a[7], None)

    for i in range(8):
        assert call(null=i) == ARG, i
    assert call(batch=0) == ARG and call(max_num=0) == ARG and call(batch=-1) == ARG
    assert call(box_dim=8) == ARG and call(box_dim=0) == ARG
    assert call(batch=65536) == UNSUPPORTED and call(max_num=nv.DET_TAIL_MAX_K + 1) == UNSUPPORTED
    assert call(batch=65536, box_dim=8) == ARG                    # argument checks come before shape checks


def test_inference_step_refusals_touch_no_device(model, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal reached the device")
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    inf = InferenceModel(model)
    with pytest.raises(TypeError, match="InferenceModel"):
        InferenceStep(model, batch_size=2, point_capacity=1000)               # a bare model
    with pytest.raises(ValueError, match="batch_size"):
        InferenceStep(inf, batch_size=0, point_capacity=1000)
    with pytest.raises(ValueError, match="point_capacity"):
        InferenceStep(inf, batch_size=2, point_capacity=0)
    dyn = copy.deepcopy(model)
    dyn.dynamic_voxelization = True
    with pytest.raises(NotImplementedError, match="dynamic_voxelization"):
        InferenceStep(InferenceModel(dyn), batch_size=2, point_capacity=1000)
    # a well-formed request allocates nothing until it is used, and cannot run before capture()
    step = InferenceStep(inf, batch_size=2, point_capacity=1000)
    assert (step.batch_size, step.point_capacity, step.feat, step.fallbacks) == (2, 1000, 4, 0)
    assert step.pts is None and step.valid is None and step.overflows() == 0
    with pytest.raises(RuntimeError, match="capture"):
        step.run([torch.zeros(10, 4)])
