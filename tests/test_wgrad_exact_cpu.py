"""The yardstick of tests/test_wgrad_plan_gpu.py without a GPU (tests/wgrad_ref.py): a torch restatement of what the weight-gradient
kernels do - f32 partial sums per row split into a NaN-prefilled workspace, summed afterwards - equals the float64 reference bit for
bit on the integer operands, in two row orders; and each of three mistakes a kernel could make fails that comparison."""
import pytest
import torch

import wgrad_ref as R

CAP, CIN, COUT, KVOL, NSPLIT = 1000, 64, 128, 9, 2          # the rectangular glds_64 cell of the device test
N_DEV = CAP - 13


def emulate(x, dy, nbr, n_dev, kvol, nsplit, order=None, unwritten=None):
    """f32 [kvol, cin, cout] the way the kernels get there: split s sums the 64-row stages [s * per, (s + 1) * per) of the live rows
    in f32 (order: a permutation of its rows) into its slice of a NaN-prefilled workspace; the slices are then added in order."""
    ws = torch.full((nsplit, kvol, x.shape[1], dy.shape[1]), R.NAN)
    ntiles = (n_dev + 63) // 64
    per = (ntiles + nsplit - 1) // nsplit
    for s in range(nsplit):
        if s == unwritten:
            continue
        rows = torch.arange(min(n_dev, s * per * 64), min(n_dev, (s + 1) * per * 64))
        if order is not None:
            rows = rows[order(len(rows))]
        for k in range(kvol):
            idx = rows if nbr is None else nbr[k, rows].long()
            g = torch.where((idx >= 0).unsqueeze(1), x.float()[idx.clamp(min=0)], torch.zeros(()))
            ws[s, k] = g.t() @ dy.float()[rows]
    out = torch.zeros_like(ws[0])
    for s in range(nsplit):
        out += ws[s]
    return out


@pytest.fixture(scope="module")
def cell():
    x, dy, nbr = R.make_inputs(CAP, CIN, COUT, KVOL, True, N_DEV, torch.device("cpu"), True, 7)
    return x, dy, nbr, R.reference(x, dy, nbr, N_DEV, KVOL)


def test_inputs_are_what_the_device_test_relies_on(cell):
    x, dy, nbr, ref = cell
    assert x.shape == (CAP + R.IN_EXTRA, CIN) and dy.shape == (CAP, COUT) and nbr.shape == (KVOL, R.table_ld(CAP)) and nbr.shape[1] > CAP + 127
    live_in = N_DEV + R.LIVE_EXTRA
    assert not x[:live_in].isnan().any() and x[live_in:].isnan().all() and not dy[:N_DEV].isnan().any() and dy[N_DEV:].isnan().all()
    assert int(nbr[:, :N_DEV].max()) < live_in and int(nbr[:, :N_DEV].min()) == -1 and int(nbr[:, N_DEV:].min()) >= live_in
    assert int(nbr.max()) < x.shape[0]
    absent = float((nbr[:, :N_DEV] < 0).float().mean())
    assert 0.25 < absent < 0.35
    assert torch.equal(x[:live_in], x[:live_in].round()) and float(x[:live_in].abs().max()) == 3 and float(dy[:N_DEV].abs().max()) == 3
    assert 256 < float(ref.abs().max()) < 2 ** 24 and not ref.isnan().any()


def test_f32_sums_equal_the_reference_in_any_order(cell):
    x, dy, nbr, ref = cell
    gen = torch.Generator().manual_seed(3)
    for order in (None, lambda n: torch.randperm(n, generator=gen)):
        for nsplit in (1, NSPLIT, 5):
            assert torch.equal(emulate(x, dy, nbr, N_DEV, KVOL, nsplit, order), ref.float())
    x1, dy1, _ = R.make_inputs(CAP, CIN, CIN, 1, False, N_DEV, torch.device("cpu"), True, 8)
    assert torch.equal(emulate(x1, dy1, None, N_DEV, 1, NSPLIT), R.reference(x1, dy1, None, N_DEV, 1).float())
    assert not R.reference(x, dy, nbr, 0, KVOL).any()


def test_a_dropped_last_row_fails(cell):
    x, dy, nbr, ref = cell
    assert not torch.equal(emulate(x, dy, nbr, N_DEV - 1, KVOL, NSPLIT), ref.float())


def test_swapped_layout_permutes_fail(cell):
    ref = cell[3]
    sq = R.reference(*R.make_inputs(300, 32, 32, 9, True, 287, torch.device("cpu"), True, 9), 287, 9)      # square: the shapes agree
    for p in (ref, sq):
        got = {layout: R.in_layout(p, layout).float() for layout in (1, 2)}
        assert got[1].shape == (p.shape[2], p.shape[1], p.shape[0]) and got[2].shape == (p.shape[1], p.shape[2], p.shape[0])
        assert not torch.equal(got[1], R.in_layout(p, 2).float()) and not torch.equal(got[2], R.in_layout(p, 1).float())


def test_an_unwritten_partial_fails(cell):
    x, dy, nbr, ref = cell
    for s in range(NSPLIT):
        got = emulate(x, dy, nbr, N_DEV, KVOL, NSPLIT, unwritten=s)
        assert got.isnan().all() and not torch.equal(got, ref.float())
    # a split without a single stage still owes its zeros: 65 live rows are two stages, the third of three splits has none
    assert emulate(x, dy, nbr, 65, KVOL, 3, unwritten=2).isnan().all()
    assert torch.equal(emulate(x, dy, nbr, 65, KVOL, 3), R.reference(x, dy, nbr, 65, KVOL).float())
