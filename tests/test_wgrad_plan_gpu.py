"""Every route of the weight-gradient launch plan (wgrad_plan / wgrad_plan_batched in csrc/igemm_wgrad.hip) on the device, at the
smallest shape that takes it, against an exact reference.  tests/test_wgrad_plan_cpu.py pins which kernel the plan names; this file
pins what the named kernel computes.

The kernels accumulate exact bf16 products in f32 and write f32.  With integer operands in [-3, 3] every product and partial sum is
an integer far below 2^24, so the f32 result does not depend on summation order, split count or reduction tree: it must equal the
float64 reference bit for bit (torch.equal, no tolerance).  One missing, doubled or misplaced row, an unwritten partial, a wrong
tile decode or a transposed layout fails it (tests/test_wgrad_exact_cpu.py runs those mistakes against the same yardstick).  The
inputs and the yardstick are tests/wgrad_ref.py: `in` with more rows than `dout`, a table whose leading dimension exceeds the
capacity and whose columns past the live count name NaN rows, NaN past both live counts.  The entry is called directly
(u3d_igemm_wgrad_bf16 / u3d_wgrad_batched_bf16), into a NaN-prefilled output and a NaN-prefilled workspace: native.spconv_wgrad
hands the kernels torch.empty, so a row split left without a single stage still has to write its zeros.

The rounding pass runs Gaussian operands once per cell and requires |dw - P| <= (n_dev + nsplit) * 2^-23 * A elementwise, A = the
same sums over absolute values: the worst-case bound of n_dev + nsplit f32 additions of exact products in any order, with twice the
f32 unit roundoff because the matrix unit's internal accumulation is not documented to round to nearest.  The measured ratios are
profiles/wgrad_routes_exact.txt."""
import pytest
import torch

import wgrad_ref as R
from uni3detr_amd import native as nv

pytestmark = pytest.mark.gpu

# name -> ((cap, cin, cout, kvol, table), (family, tile, nsplit) of the plan).  Tile and nsplit by hand from the rules in
# tests/test_wgrad_plan_cpu.py's docstring; stages = ceil(cap / 64), per = kvol * ci_blocks * co_blocks:
#   4700 x 256 x 256 x 27: 74 stages, per 27, target 256 // 27 = 9, 74 // 9 = 8 stages each -> 9; 243 workgroups keep the 256 tile
#   2100 x 256 x 512 x 27: 33 stages, per 54, target 4, 33 // 4 = 8 -> 4; 216 workgroups
#   6200 x 1024^2 x 1: 97 stages, per 16, target 16, lowered until 97 // ns >= 8 -> 12; 192 workgroups: just keeps the 256 tile
#   12300 x 1024 x 512 x 1: 193 stages, per 8, target 32 -> 24 (193 // 24 = 8); 192 workgroups
#   4700 x 128 x 128 x 27: per 27, target 512 // 27 = 18 -> 9 (74 // 9 = 8)
#   1600 x 256 x 512 x 9: 25 stages; tile 256: per 18, ns 3 (25 // 3 = 8), 54 < 192 -> tile 128: per 72, target 7 -> 3, 216 >= 192
#   4700 x 64 x 64 x 27: as the 128 one;  1000 x 64 x 128 x 9: 16 stages, per 18, target 28 -> 2
#   1000 x 128 x 128 x 1: tile 128: per 1, ns 2, 2 < 192 -> tile 64: per 4, target 128 -> 2 (16 // 2 = 8)
#   700 x 64 x 64 x 54: 11 stages, per 54, target 9 -> 1
#   1000 x 64 x 32 x 27 (tile 32): per 54, target 2048 // 54 = 37 -> 2;  1000 x 32 x 96 x 9: per 27, target 75 -> 2
#   1000 x 64 x 16 x 27 (tile 16): per 108, target 18 -> 2;  1000 x 48 x 80 x 9: per 135, target 15 -> 2
#   narrow: min(ceil(cap / 64), 256) rounded up to 8 workgroup partials;  conv_in: one partial per 128 rows
CELLS = {
    "glds8_256_remap_remainder": ((4700, 256, 256, 27, True), ("glds8_256", 256, 9)),     # one channel tile, 8 XCD-aligned splits + 1
    "glds8_256_wide_out": ((2100, 256, 512, 27, True), ("glds8_256", 256, 4)),            # gridDim.z = 2, no remap
    "glds8_256_wide_in": ((2100, 512, 256, 27, True), ("glds8_256", 256, 4)),             # the transposed rectangle
    "glds8_256_single_offset": ((6200, 1024, 1024, 1, True), ("glds8_256", 256, 12)),     # single offset through the table
    "glds_256_two_phase": ((6200, 1024, 1024, 1, False), ("glds_256", 256, 12)),          # the FPN's 1x1 convolutions
    "glds_256_two_phase_rect": ((12300, 1024, 512, 1, False), ("glds_256", 256, 24)),
    "glds_128_remap_remainder": ((4700, 128, 128, 27, True), ("glds_128", 128, 9)),
    "glds_128_halved_rect": ((1600, 256, 512, 9, True), ("glds_128", 128, 3)),            # halved from 256; kvol <= 9: one z slice
    "glds_64_remap": ((4700, 64, 64, 27, True), ("glds_64", 64, 9)),
    "glds_64_rect": ((1000, 64, 128, 9, True), ("glds_64", 64, 2)),
    "glds_64_halved_twice": ((1000, 128, 128, 1, False), ("glds_64", 64, 2)),
    "glds_64_kvol54": ((700, 64, 64, 54, True), ("glds_64", 64, 1)),                      # layouts 1 / 2 turn at most 27 offsets
    "reg_32": ((1000, 64, 32, 27, True), ("reg_32", 32, 2)),
    "reg_32_cout96": ((1000, 32, 96, 9, True), ("reg_32", 32, 2)),                        # cout no multiple of 64 in the oik / abk sums
    "reg_16": ((1000, 64, 16, 27, True), ("reg_16", 16, 2)),
    "reg_16_48_80": ((1000, 48, 80, 9, True), ("reg_16", 16, 2)),                         # channel counts on the 16 grid only
    "narrow_16_32": ((2500, 16, 32, 27, True), ("narrow", 0, 40)),
    "narrow_32_64": ((1000, 32, 64, 27, True), ("narrow", 0, 16)),
    "conv_in": ((300, 8, 16, 27, True), ("conv_in", 0, 3)),
}
# (count, rows, cin, cout) -> (tile, nsplit, workspace bytes = count * nsplit * cin * cout * 4) of wgrad_plan_batched: the largest
# tile of 256 / 128 / 64 that divides both; per = count * ci_blocks * co_blocks, nsplit = min(ceil(768 / per), max(stages // 8, 1));
# below 192 workgroups half the tile, down to 64.  The bytes give nsplit; the tile follows from the rule:
#   12 x 2050 x 512 x 512: 33 stages, tile 256: per 48, min(16, 4) = 4, 192 workgroups: stays
#   48 x 2050 x 256 x 256: per 48, 4, 192: stays
#   5 x 7200 x 256 x 256: 113 stages, tile 256: per 5, min(154, 14) = 14, 70 < 192 -> tile 128: per 20, 14, 280
#   3 x 1000 x 64 x 128: tile 64: per 6, min(128, 2) = 2
BATCH_CELLS = [((12, 2050, 512, 512), (256, 4, 50331648)),
               ((48, 2050, 256, 256), (256, 4, 50331648)),
               ((5, 7200, 256, 256), (128, 14, 18350080)),
               ((3, 1000, 64, 128), (64, 2, 196608))]
SERVED = {"narrow": (0, 1), "conv_in": (0,)}                    # every other family: all three layouts, up to 27 offsets


def _layouts(name):
    (cap, cin, cout, kvol, table), (family, _, _) = CELLS[name]
    return (0,) if kvol > 27 else SERVED.get(family, (0, 1, 2))


def _sweep(name):
    cap, cin = CELLS[name][0][:2]
    return (65, cap - 13) if cin >= 1024 else (0, 1, 63, 64, 65, cap - 13, cap)


def _seed(name, n_dev):
    cap, cin, cout, kvol, table = CELLS[name][0]
    return (cap * 31 + cin) * 1009 + cout * 57 + kvol * 2 + int(table) + 7919 * n_dev


def _launch(shape, x, dy, nbr, n_t, layout, workspace_bytes):
    """u3d_igemm_wgrad_bf16 into a NaN-prefilled output with a NaN-prefilled workspace -> (return code, dw flat)."""
    cap, cin, cout, kvol, table = shape
    dw = torch.full((kvol * cin * cout,), R.NAN, dtype=torch.float32, device=x.device)
    ws = torch.full((max(workspace_bytes // 4, 4),), R.NAN, dtype=torch.float32, device=x.device)
    nbr_p, ld = nv._nbr_ptr_ld(nbr)
    rc = nv.lib().u3d_igemm_wgrad_bf16(nv._ptr(x), nv._ptr(dy), nbr_p, ld, nv._ptr(dw), nv._ptr(n_t), cap, cin, cout, kvol, layout, nv._ptr(ws),
                                       workspace_bytes, nv._stream())
    return rc, dw


def _check_exact(p, n_dev):
    """The reference proves what it claims: exact in f32, and from 64 rows on too large for a bf16 intermediate to hold."""
    big = float(p.abs().max()) if p.numel() else 0.0
    assert big < 2 ** 24 and not bool(p.isnan().any())
    if n_dev >= 64:
        assert big > 256
    if n_dev == 0:
        assert not bool(p.any())


def test_every_family_and_batched_tile_is_reached():
    assert {want[0] for _, want in CELLS.values()} == set(nv.WGRAD_KERNELS) - {"none"}
    assert {want[0] for _, want in BATCH_CELLS} == {256, 128, 64}


@pytest.mark.parametrize("name", list(CELLS))
def test_exact(cuda, name):
    shape, want = CELLS[name]
    cap, cin, cout, kvol, table = shape
    wrong = []
    for n_dev in _sweep(name):
        x, dy, nbr = R.make_inputs(*shape, n_dev, cuda, True, _seed(name, n_dev))
        assert x.shape[0] != dy.shape[0] and (nbr is None or nbr.shape[1] > cap)
        p = R.reference(x, dy, nbr, n_dev, kvol)
        _check_exact(p, n_dev)
        n_t = torch.tensor([n_dev], dtype=torch.int32, device=cuda)
        for layout in (0, 1, 2):
            plan = nv.igemm_wgrad_plan(cap, cin, cout, kvol, table, out_layout=layout)
            if layout not in _layouts(name):                     # refused, and the output left as it was
                assert plan is None
                rc, dw = _launch(shape, x, dy, nbr, n_t, layout, nv.igemm_wgrad_plan(cap, cin, cout, kvol, table)[3])
                assert rc == nv.U3D_ERR_UNSUPPORTED and bool(dw.isnan().all())
                continue
            assert plan is not None and plan[:3] == want and plan[3] == want[2] * kvol * cin * cout * 4
            ref = R.in_layout(p, layout).float().reshape(-1)
            runs = []
            for _ in range(2):
                rc, dw = _launch(shape, x, dy, nbr, n_t, layout, plan[3])
                assert rc == 0
                runs.append(dw)
            if not torch.equal(runs[0], ref):
                bad = runs[0] != ref
                wrong.append(f"n_dev {n_dev} layout {layout}: {int(bad.sum())} of {ref.numel()} differ, {int(runs[0].isnan().sum())} NaN, "
                             f"first at {int(bad.nonzero()[0])}")
            if not torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)):
                wrong.append(f"n_dev {n_dev} layout {layout}: two launches differ")
    assert not wrong, f"{name} {want}: " + "; ".join(wrong)


@pytest.mark.parametrize("name", list(CELLS))
def test_rounding(cuda, name):
    shape, want = CELLS[name]
    cap, cin, cout, kvol, table = shape
    n_dev = cap - 13
    plan = nv.igemm_wgrad_plan(cap, cin, cout, kvol, table)
    assert plan is not None and plan[:3] == want
    x, dy, nbr = R.make_inputs(*shape, n_dev, cuda, False, _seed(name, n_dev) + 1)
    p, a = R.reference(x, dy, nbr, n_dev, kvol), R.reference(x, dy, nbr, n_dev, kvol, absolute=True)
    rc, dw = _launch(shape, x, dy, nbr, torch.tensor([n_dev], dtype=torch.int32, device=cuda), 0, plan[3])
    assert rc == 0
    err, bound = (dw.double().view_as(p) - p).abs(), (n_dev + plan[2]) * 2.0 ** -23 * a
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"wgrad_route {name}: cap {cap} cin {cin} cout {cout} kvol {kvol} table {int(table)} -> {plan[0]} tile {plan[1]} nsplit {plan[2]} "
          f"workspace {plan[3]}; n_dev {n_dev}: max |dw - P| {float(err.max()):.3e} of max |P| {float(p.abs().max()):.3e}, "
          f"max |dw - P| / bound {ratio:.3e}")
    assert bool((err <= bound).all())


def _batch_inputs(count, rows, cin, cout, n_dev, dev):
    gen = torch.Generator(device=dev).manual_seed(((count * 131 + rows) * 131 + cin) * 131 + cout + 7919 * n_dev)
    ins = torch.randint(-3, 4, (count, rows, cin), generator=gen, device=dev).to(torch.bfloat16)
    douts = torch.randint(-3, 4, (count, rows, cout), generator=gen, device=dev).to(torch.bfloat16)
    ins[:, :, 1], douts[:, :, cout - 2] = 3, -3                 # one sum past 256 from 64 rows on, see tests/wgrad_ref.py
    ins[:, n_dev:], douts[:, n_dev:] = R.NAN, R.NAN
    ref = torch.bmm(ins[:, :n_dev].double().transpose(1, 2), douts[:, :n_dev].double())
    _check_exact(ref, n_dev)
    return ins, douts, ref


def _launch_batched(ins, douts, outs, n_dev, workspace_bytes):
    """u3d_wgrad_batched_bf16 with a NaN-prefilled workspace; outs: one f32 [cin, cout] tensor per slot."""
    count, rows, cin = ins.shape
    ws = torch.full((workspace_bytes // 4,), R.NAN, dtype=torch.float32, device=ins.device)
    n_t = torch.tensor([n_dev], dtype=torch.int32, device=ins.device)
    nv._check(nv.lib().u3d_wgrad_batched_bf16(nv._ptr_array(list(ins)), nv._ptr_array(list(douts)), nv._ptr_array(outs), count, nv._ptr(n_t),
                                              rows, cin, douts.shape[2], nv._ptr(ws), workspace_bytes, nv._stream()), "wgrad_batched_bf16")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,want", BATCH_CELLS, ids=lambda v: "x".join(map(str, v)) if len(v) == 4 else None)
def test_batched_exact(cuda, shape, want):
    count, rows, cin, cout = shape
    tile, nsplit, nbytes = want
    assert int(nv.lib().u3d_wgrad_batched_workspace(*shape)) == nbytes == count * nsplit * cin * cout * 4
    for n_dev in (0, 65, rows - 13, rows):
        ins, douts, ref = _batch_inputs(*shape, n_dev, cuda)
        runs = []
        for _ in range(2):
            dws = torch.full((count, cin, cout), R.NAN, dtype=torch.float32, device=cuda)
            _launch_batched(ins, douts, list(dws), n_dev, nbytes)
            runs.append(dws)
        bad = runs[0] != ref.float()
        assert torch.equal(runs[0], ref.float()), f"n_dev {n_dev}: {int(bad.sum())} of {bad.numel()} differ, {int(runs[0].isnan().sum())} NaN"
        assert torch.equal(runs[0], runs[1])


def test_batched_shared_outputs(cuda):
    """Consecutive slots that name one output (a weight shared by three layers, then two single slots): the exact sum of the group's
    products lands in it, the single slots hold their own product alone, and nothing else is written."""
    shape = (5, 1000, 64, 128)
    count, rows, cin, cout = shape
    nbytes = 5 * 2 * 64 * 128 * 4                                # tile 64: per 5 * 1 * 2 = 10, min(ceil(768 / 10), 16 // 8) = 2 splits
    assert int(nv.lib().u3d_wgrad_batched_workspace(*shape)) == nbytes
    for n_dev in (0, 65, rows - 13, rows):
        ins, douts, ref = _batch_inputs(*shape, n_dev, cuda)
        want = torch.stack([ref[0] + ref[1] + ref[2], ref[3], ref[4]])
        _check_exact(want, n_dev)
        dws = torch.full((4, cin, cout), R.NAN, dtype=torch.float32, device=cuda)      # the fourth is nobody's output
        _launch_batched(ins, douts, [dws[0], dws[0], dws[0], dws[1], dws[2]], n_dev, nbytes)
        assert torch.equal(dws[:3], want.float()), f"n_dev {n_dev}"
        assert bool(dws[3].isnan().all())
