"""CPU: the training step's schedule (uni3detr_amd.trainer.step_plan) - the one list that TrainStep's eager step, its capture and its
replay walk: the three schedules name for name, which records are captured stages, every name a TrainStep method, and the walkers
looking a name up on the instance when they run (tests/test_dist_gpu.py replaces the reductions on the instance)."""
from types import SimpleNamespace

import pytest

from uni3detr_amd.trainer import TrainStep, step_plan

SINGLE = ["_stage1", "_reduce_num_pos", "_stage2", "_reduce_grads", "_stage3"]
TWO = ["_stage1", "_reduce_num_pos", "_stage2a", "_reduce_grads_a", "_stage2b", "_reduce_grads_b", "_stage3"]
THREE = ["_stage1", "_reduce_num_pos", "_stage2a", "_reduce_grads_a", "_stage2m", "_reduce_grads_m", "_stage2b", "_reduce_grads_b", "_stage3"]
PLANS = {(False, False): SINGLE, (True, False): TWO, (True, True): THREE}


@pytest.mark.parametrize("key", sorted(PLANS))
def test_the_three_schedules(key):
    plan = step_plan(*key)
    assert [ph.name for ph in plan] == PLANS[key]
    assert isinstance(plan, tuple) and plan == step_plan(*key)                  # immutable, and a pure function of its arguments
    assert [ph.name for ph in plan if ph.captured] == [n for n in PLANS[key] if n.startswith("_stage")]
    assert [ph.name for ph in plan if not ph.captured] == [n for n in PLANS[key] if n.startswith("_reduce_")]
    assert all(callable(getattr(TrainStep, ph.name)) for ph in plan)
    with pytest.raises(AttributeError):
        plan[0].name = "_stage2"


def test_three_phase_without_overlap_is_refused():
    with pytest.raises(ValueError):
        step_plan(False, True)


def _stub(plan, log):
    class _Stub(SimpleNamespace):
        pass
    for name in {ph.name for ph in plan}:
        setattr(_Stub, name, lambda self, name=name: log.append(name))
    return _Stub(plan=plan, loss="the loss")


@pytest.mark.parametrize("key", sorted(PLANS))
def test_eager_step_walks_the_plan_and_resolves_names_late(key):
    log = []
    st = _stub(step_plan(*key), log)
    assert TrainStep.eager_step(st) == "the loss" and log == PLANS[key]
    del log[:]
    st._reduce_num_pos = lambda: log.append("replaced")                       # on the instance, after construction
    TrainStep.eager_step(st)
    assert log == ["replaced" if n == "_reduce_num_pos" else n for n in PLANS[key]]
    del log[:]
    TrainStep.eager_step(st, stage1_done=True)                                 # the caller ran stage 1: everything but the first record
    assert log == ["replaced" if n == "_reduce_num_pos" else n for n in PLANS[key][1:]]
