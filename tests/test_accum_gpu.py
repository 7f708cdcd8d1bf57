"""GPU: u3d_adamw_step_accum (gradient accumulation, non-finite skip, EMA weights in the flat AdamW step) against
u3d_adamw_step_hold, bit for bit where the two must agree, and against its restatement (tests/accum_ref.py); then TrainStep with
accum_steps / ema_decay: captured replay versus eager, ema_scope, and the optimizer state round trip with an open window."""
import copy

import pytest
import torch

import accum_ref as R
import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
from uni3detr_amd.plugin.structures import Boxes3D
from uni3detr_amd.registry import build_model
from uni3detr_amd.synth import room_scene
from uni3detr_amd.trainer import TrainStep

pytestmark = pytest.mark.gpu

SIZES = [5, 4099, 300001]        # scalar tail only | one odd size over a single block | odd, many blocks
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _skip_mask(n, dev, seed=1):
    """uint8 per 64-element chunk, about a quarter set - None where the size has a single chunk."""
    chunks = (n + 63) // 64
    if chunks < 2:
        return None
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(chunks, generator=g) < 0.25).to(torch.uint8)
    m[0], m[-1] = 0, 1                                      # the chunk that holds the scalar tail is a skipped one
    return m.to(dev)


class _Bufs:
    """The flat buffers and the two state vectors of one optimizer, on the device."""

    def __init__(self, p0, k, max_norm, ema_decay=None, skip=None):
        from uni3detr_amd import native as nv
        self.nv = nv
        dev = p0.device
        self.p = p0.clone()
        self.m, self.v, self.acc = torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0)
        self.ema = p0.clone() if ema_decay is not None else None
        self.st, self.ast = torch.zeros(16, device=dev), torch.zeros(8, device=dev)
        self.skip = skip
        nv.adamw_set_hyper(self.st, HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], max_norm)
        nv.adamw_set_accum(self.ast, k, ema_decay)

    def call(self, g, hold=None):
        self.nv.adamw_step_accum(self.p, g, self.acc, self.m, self.v, self.st, self.ast, ema=self.ema, skip=self.skip, hold=hold)

    def tensors(self):
        return [self.p, self.m, self.v, self.acc] + ([self.ema] if self.ema is not None else [])

    def clones(self):
        return [t.clone() for t in self.tensors()] + [self.st[:5].clone()]

    def same_as(self, snap):
        return all(torch.equal(a, b) for a, b in zip(self.tensors() + [self.st[:5]], snap))


def _close(got, want, what):
    """The bound of test_flat_adamw_with_clipping_matches_torch (tests/test_trainer_gpu.py)."""
    want = want.to(got.device)
    err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
    print(f"{what}: max abs error {err:.3e} (bound {2e-6 * scale:.3e})")
    assert err <= 2e-6 * scale, what


# (a mask where the size allows one: 5 elements are a single chunk)
@pytest.mark.parametrize("n,max_norm,use_skip", [(n, mn, sk) for n in SIZES for mn in (0.0, 0.5) for sk in (False, True) if n > 64 or not sk])
def test_one_micro_step_per_update_is_todays_step_bit_for_bit(cuda, n, max_norm, use_skip):
    from uni3detr_amd import native as nv
    skip = _skip_mask(n, cuda) if use_skip else None
    torch.manual_seed(n)
    p0 = torch.randn(n, device=cuda)
    a = _Bufs(p0, 1, max_norm, skip=skip)
    p, m, v, st = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(16, device=cuda)
    nv.adamw_set_hyper(st, HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], max_norm)
    for it in range(3):
        g = torch.randn(n, device=cuda) * (10.0 if it % 2 else 0.01)
        a.call(g)
        nv.adamw_step_state(p, g, m, v, st, skip=skip)
        assert torch.equal(a.p, p) and torch.equal(a.m, m) and torch.equal(a.v, v), it
        assert torch.equal(a.st[:5], st[:5]), (it, a.st[:5].tolist(), st[:5].tolist())
        assert not a.acc.any() and a.ast[1:7].tolist()[:5] == [0.0, it + 1.0, 0.0, 0.0, 1.0]
    assert not torch.equal(p, p0)


@pytest.mark.parametrize("n", SIZES)
def test_windows_of_three_apply_every_third_call(cuda, n):
    k, max_norm = 3, 0.5
    skip = _skip_mask(n, cuda)
    torch.manual_seed(n + 1)
    p0 = torch.randn(n, device=cuda)
    a = _Bufs(p0, k, max_norm, skip=skip)
    ref = R.AccumRef(p0, k=k, max_norm=max_norm, skip=skip, **HYPER)
    for call in range(1, 7):
        g = torch.randn(n, device=cuda) * (10.0 if call > 3 else 0.01)
        before = [a.p.clone(), a.m.clone(), a.v.clone(), float(a.st[0])]
        a.call(g)
        ref.call(g)
        if call % k:
            assert torch.equal(a.p, before[0]) and torch.equal(a.m, before[1]) and torch.equal(a.v, before[2])
            assert float(a.st[0]) == before[3] and float(a.ast[5]) == R.ACCUMULATED and float(a.ast[1]) == call % k
        else:
            assert float(a.ast[5]) == R.APPLIED and float(a.st[0]) == call // k
            _close(a.p, ref.p, f"param after call {call}")
            _close(a.m, ref.m, f"exp_avg after call {call}")
            _close(a.v, ref.v, f"exp_avg_sq after call {call}")
            assert abs(float(a.st[4]) - ref.norm) <= 1e-5 * ref.norm and float(a.ast[6]) == float(a.st[4])
    assert float(a.st[0]) == 2 and not a.acc.any() and float(a.ast[2]) == 2 and float(a.ast[1]) == 0 and float(a.ast[3]) == 0
    if skip is not None:
        dead = skip.bool().repeat_interleave(64)[:n]
        assert torch.equal(a.p[dead], p0[dead]) and not a.m[dead].any() and not a.v[dead].any()


@pytest.mark.parametrize("n", SIZES)
def test_held_call_inside_a_window_is_as_if_it_never_came(cuda, n):
    k = 3
    skip = _skip_mask(n, cuda)
    torch.manual_seed(n + 2)
    p0 = torch.randn(n, device=cuda)
    gs = [torch.randn(n, device=cuda) for _ in range(3)]
    a, b = _Bufs(p0, k, 0.5, ema_decay=0.9, skip=skip), _Bufs(p0, k, 0.5, ema_decay=0.9, skip=skip)
    hold = torch.ones(1, device=cuda)
    a.call(gs[0])
    snap = a.clones()
    a.call(torch.full((n,), float("nan"), device=cuda), hold=hold)
    assert float(a.ast[5]) == R.HELD and float(a.st[11]) == 1 and float(a.st[12]) == 1 and float(a.ast[1]) == 1
    assert a.same_as(snap)                                 # the accumulator included: the held gradient is discarded
    a.call(gs[1], hold=torch.zeros(1, device=cuda))
    a.call(gs[2])
    for g in gs:
        b.call(g)
    assert all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors())) and torch.equal(a.st[:5], b.st[:5])
    assert float(a.st[12]) == 1 and float(a.st[11]) == 0 and float(a.ast[5]) == R.APPLIED and float(a.ast[2]) == 1
    assert not torch.equal(a.p, p0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", SIZES)
def test_non_finite_window_is_dropped_and_leaves_no_trace(cuda, n, bad):
    k = 3
    skip = _skip_mask(n, cuda)
    torch.manual_seed(n + 3)
    p0 = torch.randn(n, device=cuda)
    a, b = _Bufs(p0, k, 0.5, ema_decay=0.9, skip=skip), _Bufs(p0, k, 0.5, ema_decay=0.9, skip=skip)
    first = [torch.randn(n, device=cuda) for _ in range(k)]
    last = [torch.randn(n, device=cuda) for _ in range(k)]
    for g in first:                                         # one clean window first: moments and EMA are not trivial
        a.call(g); b.call(g)
    snap = a.clones()
    for j in range(k):
        g = torch.randn(n, device=cuda)
        if j == 1:
            g[n // 2 if skip is None else 3] = bad          # (element 3 lies in chunk 0, which the mask keeps live)
        a.call(g)
    assert float(a.ast[5]) == R.DROPPED and float(a.ast[3]) == 1 and float(a.ast[1]) == 0 and float(a.ast[2]) == 1
    assert not a.acc.any()
    assert a.same_as(snap[:3] + [torch.zeros_like(a.acc)] + snap[4:])          # param, moments, ema, state[0:5]: the same bits
    for g in last:
        a.call(g); b.call(g)
    assert all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors())) and torch.equal(a.st[:5], b.st[:5])
    assert float(a.ast[2]) == 2 and float(b.ast[3]) == 0 and float(a.ast[5]) == R.APPLIED


@pytest.mark.parametrize("n", SIZES)
def test_ema_follows_the_float64_restatement_and_moves_only_on_applied_updates(cuda, n):
    """d = 0.9 over three applied updates from ema0 = param0, end to end against the float64 restatement.  rtol 1e-6; the absolute
    term is for elements near zero: an AdamW update is at most ~lr = 3e-3 and float32 carries it to ~1e-6 relative (a handful of
    roundings of 6e-8 each: mean, lerp, sqrt, two divisions), i.e. ~3e-9 per update, 1e-8 over the three."""
    k, d = 2, 0.9
    skip = _skip_mask(n, cuda)
    torch.manual_seed(n + 4)
    p0 = torch.randn(n, device=cuda)
    a = _Bufs(p0, k, 0.0, ema_decay=d, skip=skip)
    ref = R.AccumRef(p0, k=k, dtype=torch.float64, max_norm=0.0, ema_decay=d, skip=skip, **HYPER)
    one, nan = torch.ones(1, device=cuda), torch.full((n,), float("nan"), device=cuda)
    # accumulate, apply | held | accumulate, apply | accumulate(inf), drop | accumulate, apply
    plan = ["g", "g", "held", "g", "g", "inf", "g", "g", "g"]
    for what in plan:
        g = torch.randn(n, device=cuda)
        if what == "inf":
            g[0] = float("inf")
        before = a.ema.clone()
        if what == "held":
            a.call(nan, hold=one); ref.call(nan, hold=True)
        else:
            a.call(g); ref.call(g)
        out = float(a.ast[5])
        assert out == ref.outcome
        if out != R.APPLIED:
            assert torch.equal(a.ema, before), what
        else:
            assert not torch.equal(a.ema, before)
    assert float(a.ast[2]) == 3 and ref.applied == 3 and float(a.ast[3]) == 1 and float(a.st[12]) == 1
    want = ref.ema.to(cuda)
    err = (a.ema.double() - want).abs()
    print(f"ema: max abs error {err.max().item():.3e}, max error / (1e-6 |ref| + 1e-8) = {(err / (1e-6 * want.abs() + 1e-8)).max().item():.3f}")
    torch.testing.assert_close(a.ema.double(), want, rtol=1e-6, atol=1e-8)
    assert not torch.equal(a.ema, a.p)
    if skip is not None:
        dead = skip.bool().repeat_interleave(64)[:n]
        assert torch.equal(a.ema[dead], p0[dead]) and torch.equal(a.p[dead], p0[dead])
    # decay <= 0: the buffer is given but not written
    b = _Bufs(p0, 1, 0.0, ema_decay=0.0, skip=skip)
    b.call(torch.randn(n, device=cuda))
    assert float(b.ast[5]) == R.APPLIED and torch.equal(b.ema, p0) and not torch.equal(b.p, p0)


# ---- trainer level: the smallest model and scenes of tests/test_trainer_gpu.py, built the same way ------------------------------------
def _data(dev, B=2, n=12000, seed0=0):
    pts, gts, labels = [], [], []
    for i in range(B):
        p, g, l = room_scene(seed0 + i, n)
        gb = torch.from_numpy(g).clone()
        gb[:, 2] -= gb[:, 5] / 2
        pts.append(torch.from_numpy(p).to(dev)); gts.append(Boxes3D(gb).to(dev)); labels.append(torch.from_numpy(l).to(dev))
    return pts, gts, labels


def _model(dev, sd=None):
    torch.manual_seed(5)
    m = build_model(copy.deepcopy(MODEL_CFG))
    if sd is not None:
        m.load_state_dict(sd)
    for mod in m.modules():                       # dropout off: the two runs must be comparable
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "attn_drop"):
            mod.attn_drop = 0.0
    return m.to(dev).train().set_precision("bf16")


def test_captured_accumulating_step_matches_eager(cuda):
    """accum_steps=2, ema_decay=0.99, four batches: both steps move the parameters on steps 2 and 4 only; losses, final parameters
    and EMA weights agree at the relative 2e-2 at which test_graph_step_matches_eager_step compares its captured and eager steps
    (losses per step; the buffers by their largest difference over their largest magnitude)."""
    batches = [_data(cuda, seed0=2 * j) for j in range(4)]
    ref = _model(cuda)
    sd = copy.deepcopy(ref.state_dict())
    eager = TrainStep(ref, *batches[0], graph=False, accum_steps=2, ema_decay=0.99)
    m2 = _model(cuda, sd)
    ts = TrainStep(m2, *batches[0], graph=True, accum_steps=2, ema_decay=0.99)
    snap = ts.snapshot()
    ts.capture(batches=batches)
    ts.restore(snap)
    assert ts.window_fill() == 0 and ts.applied_updates() == 0 and torch.equal(ts.ema, ts.flat_param) and not ts.acc.any()
    assert torch.equal(ts.flat_param, eager.flat_param)
    le, lg = [], []
    for j, b in enumerate(batches):
        for step, out in ((eager, le), (ts, lg)):
            before = step.flat_param.clone()
            step.set_batch(*b)
            out.append(float(step.step()))
            assert torch.equal(step.flat_param, before) == (j % 2 == 0), j
    for step in (eager, ts):
        assert step.applied_updates() == 2 and step.window_fill() == 0 and step.nonfinite_skips() == 0 and step.held_steps() == 0
        assert float(step.opt_state[0]) == 2 and not step.acc.any() and not torch.equal(step.ema, step.flat_param)
    print("losses eager", le, "captured", lg)
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-2 * abs(a), (le, lg)
    for name in ("flat_param", "ema"):
        a, b = getattr(eager, name), getattr(ts, name)
        err, scale = (a - b).abs().max().item(), a.abs().max().item()
        print(f"{name}: largest difference {err:.3e}, largest magnitude {scale:.3e}")
        assert err <= 2e-2 * scale, name


def test_ema_scope_exchanges_contents_in_place_and_ema_state_dict_has_the_models_layout(cuda):
    pts, gts, labels = _data(cuda)
    m = _model(cuda)
    ts = TrainStep(m, pts, gts, labels, graph=False, ema_decay=0.5)
    assert ts.accum and ts.accum_steps == 1
    for _ in range(2):
        ts.step()
    assert ts.applied_updates() == 2 and not torch.equal(ts.ema, ts.flat_param)
    p0, e0, ptr = ts.flat_param.clone(), ts.ema.clone(), (ts.flat_param.data_ptr(), ts.ema.data_ptr())
    w = next(iter(ts.params))
    with ts.ema_scope():
        assert torch.equal(ts.flat_param, e0) and torch.equal(ts.ema, p0)
        assert torch.equal(w.detach().reshape(-1), e0[:w.numel()])             # the model's own parameter sees the EMA weights
    assert torch.equal(ts.flat_param, p0) and torch.equal(ts.ema, e0)
    assert (ts.flat_param.data_ptr(), ts.ema.data_ptr()) == ptr
    sd, live = ts.ema_state_dict(), m.state_dict()
    assert list(sd.keys()) == list(live.keys()) and all(sd[k].shape == live[k].shape for k in live)
    names = {k for k, _ in m.named_parameters()}
    moved = [k for k in live if k in names and not torch.equal(sd[k], live[k])]
    assert moved and all(torch.equal(sd[k], live[k]) for k in live if k not in names)      # buffers are the live ones
    o = ts.offsets[0]
    first = next(k for k, p in m.named_parameters() if p is ts.params[0])
    assert torch.equal(sd[first].reshape(-1), ts.ema[o:o + ts.params[0].numel()])


def test_optimizer_state_round_trip_with_an_open_window(cuda):
    """The state is saved after the first of two micro-steps.  The second one is then given as a fixed gradient to the update stage
    of both the uninterrupted step and a fresh one that loaded the state: the same input, so the same bits are owed."""
    pts, gts, labels = _data(cuda)
    m = _model(cuda)
    a = TrainStep(m, pts, gts, labels, graph=False, accum_steps=2, ema_decay=0.9)
    a.step()
    assert a.window_fill() == 1 and a.applied_updates() == 0
    osd, msd = a.optimizer_state_dict(), copy.deepcopy(m.state_dict())
    assert osd["accum_steps"] == 2 and osd["acc"].any()
    g = torch.Generator(device=cuda).manual_seed(11)
    g2 = torch.randn(a.flat_grad.numel(), device=cuda, generator=g) * 1e-3
    a.flat_grad.copy_(g2)
    a._stage3()
    assert a.applied_updates() == 1 and a.window_fill() == 0
    b = TrainStep(_model(cuda, msd), pts, gts, labels, graph=False, accum_steps=2, ema_decay=0.9)
    b.load_optimizer_state_dict(osd)
    assert b.window_fill() == 1 and torch.equal(b.acc.cpu(), osd["acc"])
    b.flat_grad.copy_(g2)
    b._stage3()
    assert b.applied_updates() == 1 and b.window_fill() == 0
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "ema", "acc"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.opt_state[:5], b.opt_state[:5]) and not torch.equal(b.ema, b.flat_param)
    with pytest.raises(ValueError, match="accum_steps"):
        b.load_optimizer_state_dict(dict(osd, accum_steps=3))
    # a dict saved by a step without a window: fresh window, EMA = parameters
    plain = {k: v for k, v in osd.items() if k not in ("accum_steps", "acc", "acc_state", "ema")}
    b.load_optimizer_state_dict(plain)
    assert b.window_fill() == 0 and b.applied_updates() == 0 and not b.acc.any() and torch.equal(b.ema, b.flat_param)
    assert float(b.acc_state[0]) == 2 and abs(float(b.acc_state[4]) - 0.9) < 1e-6
