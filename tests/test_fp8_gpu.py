"""FP8 (OCP e4m3fn) inference of the wide dense convolutions on the GPU: the quantiser on every bf16 bit pattern, the absmax slot, the
weight fold against a float64 restatement, the convolution - exact on integer data (which also pins the operand lane map of the
block-scaled MFMA), within the stated bound on random data against float64 and against the bf16 kernel this feature does not touch -
and InferenceModel(dense_fp8=True) on the small two-scene SUN RGB-D model.  The reference side is tests/fp8_ref.py."""
import copy
import functools
import os

import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
import fp8_ref as R
from uni3detr_amd import native as nv
from uni3detr_amd import sparse as sp
from uni3detr_amd.inference import InferenceModel, fp8_exponent

pytestmark = pytest.mark.gpu
EPS = 1e-3


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


# ---- 1. the quantiser, exhaustively ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-3, 0, 5])
def test_quantiser_on_every_bf16_bit_pattern(cuda, e):
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).view(512, 128)
    ref, nan = R.quant_ref(x, e)
    got = nv.quant_rows_e4m3(x.to(cuda), _i32(e, cuda), _i32(512, cuda)).cpu()
    assert torch.equal(got[~nan], ref[~nan])
    assert bool(((got[nan] & 0x7f) == 0x7f).all()) and int(nan.sum()) == 254
    # only the first *n_dev rows are written
    out = torch.full((512, 128), 0x55, dtype=torch.uint8, device=cuda)
    assert nv.quant_rows_e4m3(x.to(cuda), _i32(e, cuda), _i32(300, cuda), out=out) is out
    out = out.cpu()
    assert bool((out[300:] == 0x55).all()) and torch.equal(out[:300], got[:300])


# ---- 2. absmax ------------------------------------------------------------------------------------------------------------------------
def test_absmax_is_exact_honours_n_dev_and_accumulates(cuda):
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(1000, 128, generator=gen).bfloat16()
    x[777, 5] = -39.5                                                    # a negative extreme past the live rows of the first call
    x[123, 77] = -17.25                                                  # and one inside them
    xd = x.to(cuda)
    slot = torch.zeros(3, device=cuda)
    nv.absmax_rows(xd, _i32(500, cuda), slot[1:2])
    assert slot.tolist() == [0.0, x[:500].abs().max().item(), 0.0] and slot[1].item() == 17.25
    nv.absmax_rows(xd, _i32(1000, cuda), slot[1:2])                      # a second call accumulates
    assert slot[1].item() == x.abs().max().item() == 39.5
    nv.absmax_rows(xd[:300], _i32(300, cuda), slot[1:2])                 # a smaller maximum leaves it
    assert slot[1].item() == 39.5
    for bad in (float("inf"), float("-inf"), float("nan")):
        y = xd.clone()
        y[10, 3] = bad
        s = torch.zeros(1, device=cuda)
        nv.absmax_rows(y, _i32(1000, cuda), s)
        assert s.item() == float("inf")


# ---- 3. the weight fold ---------------------------------------------------------------------------------------------------------------
def _bn_params(cout, gen, dev):
    u = lambda lo, hi: (torch.rand(cout, generator=gen) * (hi - lo) + lo).to(dev)      # noqa: E731
    return (u(0.5, 1.5), (torch.randn(cout, generator=gen) * 0.5).to(dev), (torch.randn(cout, generator=gen) * 0.5).to(dev), u(0.5, 2.0))


def _fp8_pair(w, layout, bn, dev):
    k, cout, cin = nv.conv_weight_strides(tuple(w.shape), layout)[:3]
    return (w, layout, *bn, EPS, torch.full((k, cout, cin), 0x7f, dtype=torch.uint8, device=dev),
            torch.full((cout,), -99, dtype=torch.int32, device=dev), torch.full((cout,), float("nan"), device=dev))


def test_weight_fold_three_pairs_one_launch(cuda):
    gen = torch.Generator().manual_seed(31)
    specs = [("dhwio", (3, 3, 3, 128, 128)), ("oidhw", (256, 128, 1, 3, 3)), ("dhwio", (1, 1, 1, 128, 128))]
    pairs = []
    for layout, shape in specs:
        w = (torch.randn(shape, generator=gen) * 0.05).to(cuda)
        pairs.append(_fp8_pair(w, layout, _bn_params(nv.conv_weight_strides(shape, layout)[1], gen, cuda), cuda))
    pairs[2][0][..., 5] = 0.0                                            # an all-zero output channel
    table = nv.BnFoldFp8Table(pairs)
    assert table.njobs == 3 and table.total_blocks == 128 + 256 + 128
    table.run()
    lut = R.lut(cuda).double()
    for w, layout, gamma, beta, mean, var, eps, qw, e_w, shift in pairs:
        wf, sh64 = R.fold64(w, layout, gamma, beta, mean, var, eps)
        # shift: today's bn_fold shift within 1e-6 relative
        k, cout, cin = wf.shape
        wb, sb = torch.empty((k, cout, cin), dtype=torch.bfloat16, device=cuda), torch.empty(cout, device=cuda)
        nv.bn_fold([(w, layout, gamma, beta, mean, var, eps, wb, sb)])
        assert bool(((shift - sb).abs() <= 1e-6 * sb.abs()).all())
        assert bool(((shift.double() - sh64).abs() <= 1e-6 * (beta.double().abs() + (mean.double() * gamma.double() / torch.sqrt(var.double() + eps)).abs())).all())
        # e_w: the smallest exponent that keeps the channel's max at or below 448 (or one more where the f32 product rounds across a
        # power of two); 0 for the all-zero channel
        want = torch.tensor([R.exponent_ref(v) for v in wf.abs().amax(dim=(0, 2)).tolist()], dtype=torch.int32)
        d = e_w.cpu() - want
        assert bool(((d == 0) | (d == 1)).all()), d.unique().tolist()
        if layout == "dhwio" and k == 1:
            assert e_w[5].item() == 0 and not bool(qw[:, 5].any())
        # the codes: within half an e4m3 step (normal: 2^-4 relative, subnormal: 2^(e_w - 10)) of the f32 product, no NaN code
        assert not bool(((qw & 0x7f) == 0x7f).any())
        deq = lut[qw.long()] * torch.ldexp(torch.ones(cout, dtype=torch.float64, device=cuda), e_w)[None, :, None]
        bound = 2.0 ** -4 * wf.abs() + torch.ldexp(torch.ones(cout, dtype=torch.float64, device=cuda), e_w - 10)[None, :, None]
        ratio = ((deq - wf).abs() / bound).max().item()
        print(f"fold fp8 {layout} {tuple(w.shape)}: max |qw * 2^e_w - w_folded| / bound = {ratio:.6f}")
        assert ratio <= 1.0
        # the scale is used: every channel's maximum lies in (224, 448] x 2^e_w, so its largest code is at least 224 (the value just
        # above 224 rounds down to it) unless the channel is zero
        top = lut[qw.long()].abs().amax(dim=(0, 2))
        live = wf.abs().amax(dim=(0, 2)) > 0
        assert bool((top[live] >= 224.0).all()) and bool((top <= 448.0).all())


# ---- 4. - 6. the convolution ----------------------------------------------------------------------------------------------------------
def _table(kvol, n, gen, dev):
    t = torch.randint(0, n, (kvol, n), generator=gen, dtype=torch.int32)
    t[torch.rand(kvol, n, generator=gen) < 0.4] = -1                     # absent neighbours
    return t.to(dev).contiguous()


@pytest.mark.parametrize("kvol", [27, 9, 1])
@pytest.mark.parametrize("cin,cout", [(128, 128), (256, 128), (128, 256), (256, 256)])
@pytest.mark.parametrize("n", [300, 700])
def test_convolution_is_exact_on_integer_data(cuda, n, cin, cout, kvol):
    # (few row tiles: the plan takes the 192-row kernel for every table launch here; the 256-row one has its own case below)
    _exact_case(cuda, n, cin, cout, kvol, "fp8_glds8_256x256_rows" if kvol == 1 else "fp8_glds8_192x256")


def test_convolution_is_exact_on_the_256_row_table_kernel(cuda):
    """k_igemm_fp8_glds8_256x256, the instantiation that serves the dominant layer: 50 000 rows are 196 tiles of 256 rows (one round
    of 256 CUs) against 261 of 192 (two), so the plan keeps 256-row tiles.  The last tile is partial (80 rows)."""
    _exact_case(cuda, 50000, 256, 256, 9, "fp8_glds8_256x256")


def _exact_case(cuda, n, cin, cout, kvol, kernel):
    """Inputs in [-4, 4], weights in [-2, 2], integer shift, column scales in {1/4, 1, 2}: every product and sum is exact in f32
    (K * 8 < 2^24), so the kernel must give the float64 result rounded once to bf16 - whatever the order of its sums.  Random
    (asymmetric) weights: a transposed or permuted fragment map cannot pass."""
    gen = torch.Generator().manual_seed(n + cin + 3 * cout + kvol)
    a = torch.randint(-4, 5, (n, cin), generator=gen).float()
    w = torch.randint(-2, 3, (kvol, cout, cin), generator=gen).float()
    qa, qw = R.quant_ref(a, 0)[0].to(cuda), R.quant_ref(w, 0)[0].to(cuda)
    lut = R.lut(cuda)
    assert torch.equal(lut[qa.long()].cpu(), a) and torch.equal(lut[qw.long()].cpu(), w)
    nbr = _table(kvol, n, gen, cuda) if kvol > 1 else None
    colscale = torch.tensor([0.25, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=gen)].to(cuda)
    shift = torch.randint(-50, 51, (cout,), generator=gen).float().to(cuda)
    live, SENT = n - 13, -77.0
    n_dev = _i32(live, cuda)
    assert nv.fwd_fp8_plan(n, cin, cout, kvol, kvol > 1).kernel == kernel
    for relu in (False, True):
        ref, _ = R.conv_fp8_ref64(qa, qw, nbr, colscale, shift, relu, lut)
        out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
        got = nv.igemm_fwd_affine_fp8(qa, qw, nbr, colscale, shift, relu, n_dev, n, out=out)
        assert got is out and bool((got[live:] == SENT).all())
        assert torch.equal(got[:live], ref[:live].float().bfloat16()), (relu, float((got[:live].double() - ref[:live]).abs().max()))
    assert float(ref[:live].abs().max()) > 20.0                          # (the data is not degenerate)


class _RandomCase:
    """A random layer quantised by the code under test (tests 1 and 3 hold it to the reference), its float64 yardstick on the
    dequantised operands and the bound: |y - ref| <= 2^-8 |ref| + 1e-5 s_c sum |qa| |qw| - one bf16 rounding plus the f32 accumulation
    over K <= 6912."""

    def __init__(self, n, cin, cout, kvol, dev, seed):
        gen = torch.Generator().manual_seed(seed)
        self.n, self.live = n, n - 13
        self.kernel = nv.fwd_fp8_plan(n, cin, cout, kvol, kvol > 1).kernel
        self.n_dev = _i32(self.live, dev)
        x = (torch.randn(n, cin, generator=gen) * 1.7).to(dev).bfloat16()
        e_a = fp8_exponent(float(x.abs().max()) * 2.0)
        self.qa = nv.quant_rows_e4m3(x, _i32(e_a, dev), _i32(n, dev))
        shape = (cout, cin, 1, 1, kvol)
        w = (torch.randn(shape, generator=gen) / (kvol * cin) ** 0.5).to(dev)
        pair = _fp8_pair(w, "oidhw", _bn_params(cout, gen, dev), dev)
        nv.BnFoldFp8Table([pair]).run()
        self.qw, e_w, self.shift = pair[7], pair[8], pair[9]
        self.colscale = torch.ldexp(torch.ones(cout, device=dev), e_w + e_a)
        self.nbr = _table(kvol, n, gen, dev) if kvol > 1 else None
        self.lut = R.lut(dev)
        self.ref, self.mag = {}, None
        for relu in (False, True):
            self.ref[relu], self.mag = R.conv_fp8_ref64(self.qa, self.qw, self.nbr, self.colscale, self.shift, relu, self.lut)

    def check(self, y, relu, what):
        ref = self.ref[relu][:self.live]
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * self.mag[:self.live]
        diff = (y[:self.live].double() - ref).abs()
        assert bool((diff <= bound).all())                               # (a row with no neighbour and relu(shift) = 0: 0 <= 0)
        ratio = torch.where(bound > 0, diff / bound, torch.zeros_like(diff)).max().item()
        print(f"{what} relu={relu}: max |y - ref| / bound = {ratio:.4f}; |ref| max {float(ref.abs().max()):.3f}")
        assert ratio <= 1.0, (what, relu, ratio)
        assert float(ref.abs().max()) > 0.5


# (shape, the kernel the plan must give it: 50 000 rows keep the 256-row table kernel, see the exact case above)
RANDOM_SHAPES = [(700, 256, 256, 27), (300, 128, 128, 9), (300, 256, 128, 1), (50000, 128, 128, 9)]
RANDOM_KERNELS = dict(zip(RANDOM_SHAPES, ("fp8_glds8_192x256", "fp8_glds8_192x256", "fp8_glds8_256x256_rows", "fp8_glds8_256x256")))


@functools.lru_cache(maxsize=None)
def _random_case(shape, dev):
    return _RandomCase(*shape, dev, seed=sum(shape))


@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_convolution_random_against_float64(cuda, shape):
    c = _random_case(shape, cuda)
    assert c.kernel == RANDOM_KERNELS[shape]
    for relu in (False, True):
        out = torch.full((c.n, shape[2]), -77.0, dtype=torch.bfloat16, device=cuda)
        y = nv.igemm_fwd_affine_fp8(c.qa, c.qw, c.nbr, c.colscale, c.shift, relu, c.n_dev, c.n, out=out)
        assert bool((y[c.live:] == -77.0).all())
        c.check(y, relu, f"fp8 {shape}")


@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_convolution_against_the_bf16_kernel(cuda, shape):
    """The same layer through u3d_igemm_fwd_affine_bf16 with the codes as bf16 rows and qw * 2^(e_a + e_w) as bf16 weights (both exact):
    the same real arithmetic in another summation order, held to the same bound - and then the two kernels to twice that bound of
    each other."""
    c = _random_case(shape, cuda)
    for relu in (False, True):
        emu = R.emulate_on_bf16(nv, c.qa, c.qw, c.nbr, c.colscale, c.shift, relu, c.n_dev, c.n, table=c.lut)
        c.check(emu, relu, f"bf16 emulation {shape}")
        y = nv.igemm_fwd_affine_fp8(c.qa, c.qw, c.nbr, c.colscale, c.shift, relu, c.n_dev, c.n)
        ref = c.ref[relu][:c.live]
        bound = 2 * (2.0 ** -8 * ref.abs() + 1e-5 * c.mag[:c.live])
        assert bool(((y[:c.live].double() - emu[:c.live].double()).abs() <= bound).all())


def test_entry_refuses_what_the_plan_does_not_serve(cuda):
    qa = torch.zeros(256, 64, dtype=torch.uint8, device=cuda)
    qw = torch.zeros(1, 128, 64, dtype=torch.uint8, device=cuda)
    with pytest.raises(nv.U3DError, match="igemm_fwd_affine_fp8"):
        nv.igemm_fwd_affine_fp8(qa, qw, None, torch.ones(128, device=cuda), torch.zeros(128, device=cuda), 1, _i32(256, cuda), 256)


# ---- 7. the model ---------------------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    """The SUN RGB-D model with two layers per SECOND3D block and one extra FPN conv (the model of tests/test_bn_fold_gpu.py)."""
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["pts_backbone"]["layer_nums"] = [2, 2, 2]
    cfg["pts_neck"]["extra_conv"]["num_conv"] = 1
    return cfg


@pytest.fixture(scope="module")
def scene(cuda):
    from oracle.weights import seeded_tensor
    from uni3detr_amd.registry import build_model
    from uni3detr_amd.synth import room_scene
    model = build_model(_tiny_cfg())
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval().set_precision("bf16")
    pts = [torch.from_numpy(room_scene(i, 9000 - 2500 * i)[0]).to(cuda) for i in range(2)]       # B = 2, different point counts
    inf = InferenceModel(model, dense_fp8=True)
    with pytest.raises(RuntimeError, match="calibrate"):
        inf.extract_pts_feat(pts)
    cal = inf.calibrate([pts])
    return model, pts, inf, cal


def _emulated(lut):
    def conv(feats, ent, geom, relu=True):
        qin = nv.quant_rows_e4m3(feats.contiguous(), ent.e_a, geom.n_in_dev)
        nbr = geom.nbr_fwd if ent.qw.shape[0] > 1 else None
        return R.emulate_on_bf16(nv, qin, ent.qw, nbr, ent.colscale, ent.shift, relu, geom.n_out_dev, geom.n_out, table=lut)
    return conv


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_model_fp8_layers_take_the_fp8_entry(scene, monkeypatch):
    model, pts, inf, cal = scene
    # what measured faster than bf16: the 256 -> 128 first conv, the 256- and 512-channel stride-1 convs, the FPN's 3 x 3 x 3 conv
    assert inf.fp8_layers == (["pts_backbone.blocks.0.0"] + [f"pts_backbone.blocks.{b}.{j}" for b in (1, 2) for j in (3, 6)]
                              + ["pts_neck.extra_blocks.0"])
    why = dict(inf.fp8_skipped)
    assert "strided" in why["pts_backbone.blocks.1.0"] and "1 x 1 x 1" in why["pts_neck.deblocks.0.0"] and "128 -> 128" in why["pts_backbone.blocks.0.3"]
    assert sorted(cal) == sorted(inf.fp8_layers)
    for name, (amax, e_a) in cal.items():
        assert amax > 0 and e_a == fp8_exponent(amax * 2.0) and amax * 2.0 <= 448.0 * 2.0 ** e_a
    calls, quants, affine = [], [], []
    o1, o2, o3 = nv.igemm_fwd_affine_fp8, nv.quant_rows_e4m3, nv.igemm_fwd_affine
    monkeypatch.setattr(nv, "igemm_fwd_affine_fp8", lambda *a, **k: calls.append(tuple(a[1].shape)) or o1(*a, **k))
    monkeypatch.setattr(nv, "quant_rows_e4m3", lambda *a, **k: quants.append(1) or o2(*a, **k))
    monkeypatch.setattr(nv, "igemm_fwd_affine", lambda *a, **k: affine.append(1) or o3(*a, **k))
    inf.extract_pts_feat(pts)
    assert len(calls) == len(quants) == len(inf.fp8_layers) and len(affine) == len(inf.folded) - len(inf.fp8_layers)
    assert sorted(calls) == sorted(tuple(e.qw.shape) for e in inf._fp8) and sp._FOLD[0] is None      # (the branches run in their own order)


def test_model_feature_volume_matches_the_emulation_on_the_bf16_kernel(scene, monkeypatch):
    model, pts, inf, cal = scene
    got = inf.extract_pts_feat(pts)[0]
    monkeypatch.setattr(sp, "conv_affine_fp8", _emulated(R.lut(got.device)))
    emu = inf.extract_pts_feat(pts)[0]
    monkeypatch.undo()
    rel = _rel(got, emu)
    print(f"feature volume, fp8 kernels vs their emulation on the bf16 kernel: relative L2 {rel:.3e}")
    assert bool(torch.isfinite(got).all()) and float(emu.double().norm()) > 0
    assert rel <= 1e-2


def test_model_state_roundtrip_refresh_and_batched_tail(scene):
    model, pts, inf, cal = scene
    state = inf.fp8_state()
    assert state["headroom"] == 2.0 and state["e_a"] == {n: e for n, (_, e) in cal.items()}
    other = InferenceModel(model, dense_fp8=True)
    with pytest.raises(RuntimeError, match="calibrate"):
        other.extract_pts_feat(pts)
    other.load_fp8_state(state)                                          # no second calibration
    for a, b in zip(inf._fp8, other._fp8):
        assert torch.equal(a.e_a, b.e_a) and torch.equal(a.colscale, b.colscale) and torch.equal(a.qw, b.qw) and b.calibrated
        assert torch.equal(a.colscale, torch.ldexp(torch.ones_like(a.colscale), a.e_w + a.e_a))
    assert _rel(other.extract_pts_feat(pts)[0], inf.extract_pts_feat(pts)[0]) <= 1e-2
    # refresh(): weights folded and quantised again, column scales rebuilt
    ent = other._fp8[-1]
    bn = dict(model.named_modules())[ent.name[:-1] + "1"]
    q0, s0, c0 = ent.qw.clone(), ent.shift.clone(), ent.colscale.clone()
    bn.weight.data.mul_(4.0)
    other.refresh()
    assert torch.equal(ent.colscale, c0 * 4.0) and torch.equal(ent.qw, q0) and not torch.equal(ent.shift, s0)      # gamma x 4: e_w + 2, same codes
    bn.weight.data.div_(4.0)
    other.refresh()
    assert torch.equal(ent.colscale, c0) and torch.equal(ent.qw, q0)
    det = inf.simple_test_batched(None, pts, on_device=True)
    K = det.boxes.shape[1]
    cnt = det.count.cpu().tolist()
    assert det.boxes.is_cuda and len(cnt) == 2 and all(0 <= c <= K for c in cnt)
    for b, c in enumerate(cnt):
        assert not bool(det.boxes[b, c:].any()) and not bool(det.scores[b, c:].any()) and not bool(det.labels[b, c:].any())
    assert bool(torch.isfinite(det.boxes).all()) and bool(torch.isfinite(det.scores).all())


def test_model_logit_parity_is_reported(scene, monkeypatch):
    """Not a gate: the relative L2 of the class and box logits from the fp32 model, for the bf16 folded, the fp8 and the emulated-fp8
    forward.  (No trained checkpoint: the effect on AP is unmeasured.)  Written to $U3D_FP8_PARITY_FILE when that is set."""
    model, pts, inf, cal = scene

    def logits(which):
        with torch.no_grad():
            if which is None:
                feat, fps = model.extract_pts_feat(pts)
                outs = model.pts_bbox_head(feat, None, fps)
            else:
                outs = which.head_outputs(pts)
        return outs["all_cls_scores"].double(), outs["all_bbox_preds"].double()

    try:
        model.set_precision("fp32")
        ref = logits(None)
    finally:
        model.set_precision("bf16")
    rows = {"bf16 folded": logits(InferenceModel(model)), "fp8": logits(inf)}
    monkeypatch.setattr(sp, "conv_affine_fp8", _emulated(R.lut(pts[0].device)))
    rows["fp8 emulated on the bf16 kernel"] = logits(inf)
    monkeypatch.undo()
    lines = ["relative L2 of the head's logits from set_precision('fp32'), two SUN RGB-D scenes, seeded weights (no trained checkpoint)",
             f"{'forward':34s} {'cls':>10s} {'box':>10s}"]
    for name, (cls, box) in rows.items():
        lines.append(f"{name:34s} {_rel(cls, ref[0]):10.3e} {_rel(box, ref[1]):10.3e}")
        assert bool(torch.isfinite(cls).all()) and bool(torch.isfinite(box).all())
    lines.append("calibration (max |input|, e_a): " + ", ".join(f"{n.split('.', 1)[1]} ({a:.3g}, {e})" for n, (a, e) in cal.items()))
    print("\n".join(lines))
    path = os.environ.get("U3D_FP8_PARITY_FILE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
