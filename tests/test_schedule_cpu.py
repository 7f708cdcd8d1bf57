"""lr / momentum schedules (uni3detr_amd/schedule.py) against the closed forms of the mmcv hooks the shipped configs name."""
import ast
import math
import os

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import schedule as S
from uni3detr_amd.registry import Config, to_config

# the shipped configs as Config.fromfile resolves them (oracle/make_golden.py gen_shipped_configs)
SHIPPED = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")


def shipped(name):
    return Config(to_config(ast.literal_eval(open(SHIPPED).read())[name]["config"]))


def test_step_policy_of_the_sunrgbd_config():
    cfg = shipped("sunrgbd")
    sch = S.build_schedule(cfg, iters_per_epoch=100)
    base = cfg["optimizer"]["lr"]
    assert sch.lr(0) == base and sch.lr(31 * 100 + 99) == base
    assert math.isclose(sch.lr(32 * 100), base * 0.1) and math.isclose(sch.lr(37 * 100 + 5), base * 0.1)
    assert math.isclose(sch.lr(38 * 100), base * 0.01)


def test_step_policy_warmup_forms():
    s = S.StepSchedule(1.0, [2], iters_per_epoch=10, warmup="linear", warmup_iters=4, warmup_ratio=0.25)
    assert math.isclose(s.lr(0), 0.25) and math.isclose(s.lr(2), 1 - 0.5 * 0.75) and s.lr(4) == 1.0
    assert math.isclose(S.StepSchedule(1.0, [], warmup="exp", warmup_iters=4, warmup_ratio=0.01).lr(2), 0.1)
    assert S.StepSchedule(1.0, [], warmup="constant", warmup_iters=4, warmup_ratio=0.5).lr(3) == 0.5


def test_cyclic_policy_of_the_nuscenes_config():
    cfg = shipped("nuscenes")
    ipe = 50
    sch = S.build_schedule(cfg, iters_per_epoch=ipe)
    T = cfg["runner"]["max_epochs"] * ipe
    base = cfg["optimizer"]["lr"]
    up = int(0.4 * T)
    assert math.isclose(sch.lr(0), base)
    assert math.isclose(sch.lr(up), base * 10)
    assert math.isclose(sch.lr(up // 2), base * (10 + 0.5 * (1 - 10) * (math.cos(math.pi * (up // 2) / up) + 1)))
    assert sch.lr(T - 1) < base * 1e-3 and sch.lr(T - 1) > base * 1e-4
    h0, hup = sch.hyper(0), sch.hyper(up)
    b1, b2 = cfg["optimizer"].get("betas", (0.9, 0.999))        # the config inherits betas (0.95, 0.99) from the cyclic_20e schedule
    assert math.isclose(h0["betas"][0], b1) and math.isclose(hup["betas"][0], b1 * 0.85 / 0.95) and hup["betas"][1] == b2
    lrs = [sch.lr(i) for i in range(T)]
    assert all(b >= a for a, b in zip(lrs[:up], lrs[1:up + 1])) and all(b <= a for a, b in zip(lrs[up:-1], lrs[up + 1:]))
