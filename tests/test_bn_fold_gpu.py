"""Eval-mode BatchNorm folded into the convolutions, on the GPU: the fold kernel (u3d_bn_fold_batched) and the affine convolution
(u3d_igemm_fwd_affine_bf16) against float64 restatements written here, the bit-exact identities with u3d_igemm_fwd_bf16, and
InferenceModel against model.eval() and the fp32 model.

E(path) = max |path - f64| / max |f64| over live rows; the folded path is held to E(folded) <= 2 * E(unfolded), with E(unfolded)
measured in the same test on the same inputs through the existing entries (u3d_igemm_fwd_bf16 + u3d_bn_apply).  Both are a few bf16
roundings of the same real number; a wrong scale, shift or channel mapping misses by orders of magnitude."""

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from test_bn_fold_cpu import AFFINE_PLAN, bf16_bits_from_f64, tiny_cfg
from uni3detr_amd import native as nv
from uni3detr_amd import sparse as sp
from uni3detr_amd.inference import InferenceModel

pytestmark = pytest.mark.gpu
EPS = 1e-3


def _bn_params(cout, gen, dev):
    u = lambda lo, hi: (torch.rand(cout, generator=gen) * (hi - lo) + lo).to(dev)      # noqa: E731
    return dict(gamma=u(0.5, 1.5), beta=torch.randn(cout, generator=gen).to(dev) * 0.5, mean=torch.randn(cout, generator=gen).to(dev) * 0.5,
                var=u(0.5, 2.0))


def _koi64(w, layout):
    """f64 [kvol, Cout, Cin] view of a master weight."""
    if layout == "dhwio":
        kd, kh, kw, cin, cout = w.shape
        return w.double().reshape(kd * kh * kw, cin, cout).permute(0, 2, 1).contiguous()
    cout, cin = w.shape[:2]
    return w.double().reshape(cout, cin, -1).permute(2, 0, 1).contiguous()


def _fold_pairs(shapes, gen, dev):
    pairs = []
    for layout, shape in shapes:
        w = torch.randn(shape, generator=gen).to(dev)
        k, cout, cin = nv.conv_weight_strides(shape, layout)[:3]
        bn = _bn_params(cout, gen, dev)
        pairs.append((w, layout, bn["gamma"], bn["beta"], bn["mean"], bn["var"], EPS,
                      torch.full((k, cout, cin), float("nan"), dtype=torch.bfloat16, device=dev),
                      torch.full((cout,), float("nan"), device=dev)))
    return pairs


def _check_fold(pair):
    w, layout, gamma, beta, mean, var, eps, wf, shift = pair
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    ref_shift = beta.double() - mean.double() * scale
    bound = 8 * 2.0 ** -24 * (beta.double().abs() + (mean.double() * scale).abs())
    assert bool(((shift.double() - ref_shift).abs() <= bound).all()), float(((shift.double() - ref_shift).abs() / bound).max())
    ref = bf16_bits_from_f64((_koi64(w, layout) * scale[None, :, None]).cpu().numpy())
    got = wf.cpu().view(torch.int16).numpy().view(np.uint16)
    assert got.shape == ref.shape
    # sign-magnitude patterns of the same sign: one ulp apart = patterns one apart
    d = got.astype(np.int32) - ref.astype(np.int32)
    assert np.abs(d).max() <= 1, int(np.abs(d).max())
    share = float((d != 0).mean())
    print(f"fold {layout} {tuple(w.shape)}: {share:.2e} of the elements one ulp from the directly rounded value")
    assert share <= 0.01
    return share


def test_fold_kernel_three_jobs_both_layouts_one_launch(cuda):
    gen = torch.Generator().manual_seed(11)
    # (kvol, Cin, Cout) = (9, 128, 128) [kD,kH,kW,Cin,Cout]; (27, 64, 64) and (1, 128, 256) [Cout,Cin,kD,kH,kW] (the last: contiguous
    # input channels, the 16-byte loads)
    pairs = _fold_pairs([("dhwio", (1, 3, 3, 128, 128)), ("oidhw", (64, 64, 3, 3, 3)), ("oidhw", (256, 128, 1, 1, 1))], gen, cuda)
    table = nv.bn_fold(pairs)
    assert table.njobs == 3 and table.total_blocks == 72 + 54 + 16
    for p in pairs:
        _check_fold(p)
    # refresh: new running_var in place, the same table, one more launch -> other weights and another shift
    before_w, before_s = pairs[1][7].clone(), pairs[1][8].clone()
    others = [(p[7].clone(), p[8].clone()) for p in (pairs[0], pairs[2])]
    pairs[1][5].mul_(1.7)
    table.run()
    assert not torch.equal(pairs[1][7], before_w) and not torch.equal(pairs[1][8], before_s)
    _check_fold(pairs[1])
    for p, (w0, s0) in zip((pairs[0], pairs[2]), others):                  # the untouched jobs give the same bytes again
        assert torch.equal(p[7].view(torch.int16), w0.view(torch.int16)) and torch.equal(p[8], s0)


def test_fold_kernel_ragged_job_and_scale_only(cuda):
    gen = torch.Generator().manual_seed(12)
    # 5 * 20 * 36 = 3600 elements: one full 2048-element chunk and a ragged one; the job behind it must start on its own block
    pairs = _fold_pairs([("dhwio", (1, 1, 5, 36, 20)), ("oidhw", (12, 8, 1, 1, 3)), ("dhwio", (1, 1, 1, 64, 64))], gen, cuda)
    guard = torch.full((4096 + 64,), 7.0, dtype=torch.bfloat16, device=cuda)            # the last job writes the front of a guarded buffer
    last = list(pairs[2])
    last[7], last[8] = guard[:4096].view(1, 64, 64), None                               # scale_only: no shift written
    pairs[2] = tuple(last)
    table = nv.bn_fold(pairs)
    assert table.njobs == 3 and table.total_blocks == 2 + 1 + 2
    for p in pairs[:2]:
        _check_fold(p)
    full = list(pairs[2])
    full[8] = torch.empty(64, device=cuda)
    nv.bn_fold([tuple(full[:7]) + (torch.empty_like(guard[:4096].view(1, 64, 64)), full[8])])
    _check_fold((*pairs[2][:7], pairs[2][7], full[8]))                                 # same weights as a job that also writes the shift
    assert bool((guard[4096:] == 7.0).all())                                            # nothing past the job's last element


# ---- the affine convolution -------------------------------------------------------------------------------------------------------
class _Case:
    """Inputs, the f64 yardstick and the unfolded result of one shape; built once per shape and shared."""

    def __init__(self, n, cin, cout, kvol, table, dev, seed):
        gen = torch.Generator().manual_seed(seed)
        self.n, self.cin, self.cout, self.kvol = n, cin, cout, kvol
        self.live = n - 13                                                              # *n_out_dev < n_out_cap
        self.n_dev = torch.tensor([self.live], dtype=torch.int32, device=dev)
        self.x = torch.randn(n, cin, generator=gen).to(dev).bfloat16()
        self.w = (torch.randn(kvol, cout, cin, generator=gen) / (kvol * cin) ** 0.5).to(dev)          # f32 master, n-major
        self.nbr = None
        if table:
            t = torch.randint(0, n, (kvol, n), generator=gen, dtype=torch.int32)
            t[torch.rand(kvol, n, generator=gen) < 0.3] = -1                                          # absent neighbours
            self.nbr = t.to(dev).contiguous()
        self.bn = _bn_params(cout, gen, dev)
        self.scale = self.bn["gamma"].double() / torch.sqrt(self.bn["var"].double() + EPS)
        self.shift64 = self.bn["beta"].double() - self.bn["mean"].double() * self.scale
        self.conv64 = self._conv64()

    def _conv64(self):
        x, w = self.x.double(), self.w.double()
        if self.nbr is None:
            return x @ w[0].t()
        out = torch.zeros(self.n, self.cout, dtype=torch.float64, device=x.device)
        for k in range(self.kvol):
            idx = self.nbr[k].long()
            g = x[idx.clamp(min=0)] * (idx >= 0).unsqueeze(1)
            out += g @ w[k].t()
        return out

    def plain(self, w_bf16, sentinel=None):
        out = torch.full((self.n, self.cout), sentinel, dtype=torch.bfloat16, device=self.x.device) if sentinel is not None else None
        y = torch.empty((self.n, self.cout), dtype=torch.bfloat16, device=self.x.device) if out is None else out
        ld = self.nbr.shape[1] if self.nbr is not None else 0
        nv._check(nv.lib().u3d_igemm_fwd_bf16(nv._ptr(self.x), nv._ptr(w_bf16), nv._ptr(self.nbr), ld, nv._ptr(y), nv._ptr(self.n_dev),
                                              self.n, self.cin, self.cout, self.kvol, 1, None, None, nv._stream()), "igemm_fwd_bf16")
        return y


def _E(path, ref, live):
    return float((path[:live].double() - ref[:live]).abs().max() / ref[:live].abs().max())


@pytest.mark.parametrize("shape,family", AFFINE_PLAN)
def test_affine_conv_identities_padding_and_error_bound(cuda, shape, family):
    n, cin, cout, kvol, table = shape
    assert nv.igemm_fwd_affine_plan(*shape)[0] in family
    c = _Case(n, cin, cout, kvol, table, cuda, seed=n % 1000 + cout)
    live, SENT = c.live, -77.0
    wb = c.w.bfloat16()
    zero = torch.zeros(cout, device=cuda)
    base = c.plain(wb, SENT)
    assert bool((base[live:] == SENT).all()) and bool((base[:live] != SENT).any())
    # shift = 0: bit for bit u3d_igemm_fwd_bf16 on the same weights; relu = 1: relu() of it; rows past *n_out_dev as that entry leaves them
    for relu in (0, 1):
        out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
        got = nv.igemm_fwd_affine(c.x, wb, c.nbr, zero, relu, c.n_dev, n, out=out)
        want = base.clone()
        if relu:
            want[:live] = torch.relu(base[:live])
        assert got is out and torch.equal(got.view(torch.int16), want.view(torch.int16)), relu
    # the folded path: one fold launch, one conv launch
    wf, sh = torch.empty((kvol, cout, cin), dtype=torch.bfloat16, device=cuda), torch.empty(cout, device=cuda)
    master = c.w.permute(1, 2, 0).contiguous().view(cout, cin, 1, 1, kvol)              # [Cout,Cin,kD,kH,kW]
    nv.bn_fold([(master, "oidhw", c.bn["gamma"], c.bn["beta"], c.bn["mean"], c.bn["var"], EPS, wf, sh)])
    for relu in (True, False):
        ref = c.conv64 * c.scale[None] + c.shift64[None]
        if relu:
            ref = torch.relu(ref)
        out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
        folded = nv.igemm_fwd_affine(c.x, wf, c.nbr, sh, relu, c.n_dev, n, out=out)
        assert bool((folded[live:] == SENT).all())
        # the unfolded path as sparse._BNRows runs it in eval mode
        y0 = nv.spconv_fwd(c.x, wb, c.nbr, c.n_dev, n, cout, transpose_w=True, tag="spconv_fwd")
        unfolded = nv.bn_apply(y0, c.bn["mean"], torch.rsqrt(c.bn["var"] + EPS), c.bn["gamma"], c.bn["beta"], None, relu, c.n_dev)
        ef, eu = _E(folded, ref, live), _E(unfolded, ref, live)
        print(f"affine {shape} relu={relu}: E(folded) = {ef:.3e}  E(unfolded) = {eu:.3e}")
        assert eu < 2e-2                                                                 # the yardstick itself is bf16-grade
        assert ef <= 2 * eu, (ef, eu)


def test_affine_entry_refuses_what_it_does_not_serve(cuda):
    x = torch.zeros(256, 32, dtype=torch.bfloat16, device=cuda)
    w = torch.zeros(1, 64, 32, dtype=torch.bfloat16, device=cuda)
    n_dev = torch.tensor([256], dtype=torch.int32, device=cuda)
    with pytest.raises(nv.U3DError, match="igemm_fwd_affine_bf16"):
        nv.igemm_fwd_affine(x, w, None, torch.zeros(64, device=cuda), 1, n_dev, 256)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(cuda):
    from oracle.weights import seeded_tensor
    from uni3detr_amd.registry import build_model
    from uni3detr_amd.synth import room_scene
    model = build_model(tiny_cfg())
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval()
    pts = [torch.from_numpy(room_scene(i, 9000 - 2500 * i)[0]).to(cuda) for i in range(2)]       # B = 2, different point counts
    return model, pts


def _logits(model, pts, inf=None):
    with torch.no_grad():
        if inf is not None:
            outs = inf.head_outputs(pts)
        else:           # model.eval() as it stands; in bf16 mode the head runs under autocast (as forward_pts_train runs it)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=model.amp_dtype is not None):
                feat, fps = model.extract_pts_feat(pts)
                outs = model.pts_bbox_head(feat, None, fps)
    return outs["all_cls_scores"].double(), outs["all_bbox_preds"].double()


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_model_logits_folded_vs_unfolded_against_fp32(scene):
    """Deviation = relative L2 of the head's class / box logits from the same model under set_precision('fp32') (the measure of
    tests/test_bf16_parity_gpu.py); folded <= 2 x unfolded."""
    model, pts = scene
    ref = _logits(model.set_precision("fp32"), pts)
    model.set_precision("bf16")
    unf = _logits(model, pts)
    inf = InferenceModel(model)
    fol = _logits(model, pts, inf)
    for name, r, u, f in zip(("cls", "box"), ref, unf, fol):
        du, df = _rel(u, r), _rel(f, r)
        print(f"{name} logits: folded {df:.3e}  unfolded {du:.3e}")
        assert df <= 2 * du, (name, df, du)


def test_model_structure_batched_tail_and_refresh(scene, monkeypatch):
    model, pts = scene
    model.set_precision("bf16")
    inf = InferenceModel(model)
    assert len(inf.folded) == 13 and len(inf.unfolded) == 21
    # every BatchNorm apply pass of a folded forward belongs to an unfolded layer; the unfolded forward runs one per BatchNorm
    calls = []
    orig = nv.bn_apply
    monkeypatch.setattr(nv, "bn_apply", lambda *a, **k: calls.append(1) or orig(*a, **k))
    inf.extract_pts_feat(pts)
    assert len(calls) == len(inf.unfolded)
    calls.clear()
    with torch.no_grad():
        model.extract_pts_feat(pts)
    assert len(calls) == len(inf.unfolded) + len(inf.folded) and sp._FOLD[0] is None
    monkeypatch.setattr(nv, "bn_apply", orig)
    # the batched tail on the folded forward: a well-formed DetBatch
    det = inf.simple_test_batched(None, pts, on_device=True)
    K = det.boxes.shape[1]
    cnt = det.count.cpu().tolist()
    assert det.boxes.is_cuda and len(cnt) == 2 and all(0 <= c <= K for c in cnt)
    for b, c in enumerate(cnt):
        assert not bool(det.boxes[b, c:].any()) and not bool(det.scores[b, c:].any()) and not bool(det.labels[b, c:].any())
    out = inf.simple_test(None, pts)
    assert len(out) == 2 and set(out[0]) == {"boxes_3d", "scores_3d", "labels_3d"}
    # running statistics changed in place: the folded buffers, and so the output, move only at refresh().  The forward in front of the
    # dense stack is not bitwise reproducible from run to run (f32 sums in another order: ~1e-3 after the bf16 roundings), while half
    # a standard deviation on every channel of the last BatchNorm moves the O(1) feature volume by tens of percent
    bn = dict(model.named_modules())["pts_neck.extra_blocks.1"]
    shift = inf._by_bn[id(bn)].shift
    a, s0 = inf.extract_pts_feat(pts)[0].double(), shift.clone()
    bn.running_mean.add_(0.5)
    b, s1 = inf.extract_pts_feat(pts)[0].double(), shift.clone()
    inf.refresh()
    c, s2 = inf.extract_pts_feat(pts)[0].double(), shift.clone()
    bn.running_mean.sub_(0.5)
    inf.refresh()
    print(f"refresh: without {_rel(b, a):.3e}, with {_rel(c, a):.3e}")
    assert torch.equal(s0, s1) and not torch.equal(s1, s2)
    assert torch.allclose(shift, s0, atol=1e-6)                        # ((m + 0.5) - 0.5 is m up to an f32 rounding)
    assert _rel(b, a) <= 1e-2 and _rel(c, a) >= 5e-2
