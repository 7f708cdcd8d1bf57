"""The two pieces every sparse / dense convolution call goes through, without a GPU: sparse._conv_route (which kernels serve one
convolution, decided once in its forward) against the expressions _SparseConv.forward / backward carried piecemeal before it, and
native.census_meta / timed_begin / timed_end (the timed region and the census entry of a launch) against the block each of the eleven
wrappers carried before them."""
import itertools
import types

import pytest
import torch

from uni3detr_amd import native as nv
from uni3detr_amd import sparse as sp

FLAGS = ("SUBM_HALO", "REV_SUBM_TABLE", "HALO_128", "NMAJOR_FWD", "STRIDED_DGRAD_SPLIT", "SPLIT_BF16")
SHAPES = ((4, 16), (16, 16), (16, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 128), (256, 256))


def route_as_it_was(feats, cin, cout, kv, g):
    """(split, nmajor, halo, strided_split) the way the forward and the two backward bodies used to work them out."""
    bf16 = feats.dtype == torch.bfloat16
    nmajor = sp.NMAJOR_FWD and bf16 and ((cin % 64 == 0 and cout % 64 == 0) or nv.direct_serves(cin, cout, kv))
    # _split_serves, then the forward's "narrow and no table -> none"
    if not (sp._SPLIT[0] and feats.is_cuda and feats.dtype == torch.float32):
        split = None
    elif cin % 64 == 0 and cout % 64 == 0:
        split = "wide"
    elif nv.direct_serves(cin, cout, kv):
        split = "narrow"
    else:
        split = None
    if split == "narrow" and g.nbr_fwd is None:
        split = None
    halo = None
    if not split:
        halo = sp._halo_of(g, kv, cin, cout) if nmajor else None
    dout_dtype, n_out, kvol = feats.dtype, g.n_out, kv
    if split == "narrow":
        strided = False
    elif split == "wide":
        strided = (sp.STRIDED_DGRAD_SPLIT and g.strided and kvol > 1 and (kvol * cin) % 64 == 0
                   and n_out * (sp.STRIDED_SPLIT_SPARSE_RATIO if g.kind == "sparse" else sp.STRIDED_SPLIT_MIN_RATIO) <= g.n_in)
    else:
        strided = (sp.STRIDED_DGRAD_SPLIT and g.strided and kvol > 1 and dout_dtype == torch.bfloat16 and cout % 64 == 0
                   and (kvol * cin) % 64 == 0
                   and g.n_out * (sp.STRIDED_SPLIT_SPARSE_RATIO if g.kind == "sparse" else sp.STRIDED_SPLIT_MIN_RATIO) <= g.n_in)
    return split, bool(nmajor), halo, bool(strided)


def test_route_is_what_forward_and_backward_decided_piecemeal(monkeypatch):
    table, halo_tab = object(), object()
    level = types.SimpleNamespace(halo=lambda: halo_tab)
    seen = set()
    for flags in itertools.product((True, False), repeat=len(FLAGS)):
        for name, v in zip(FLAGS, flags):
            monkeypatch.setattr(sp, name, v)
        for scope_on in (True, False):
            with sp.split_scope(scope_on):
                assert sp._SPLIT[0] == (scope_on and sp.SPLIT_BF16)
                for dtype, (cin, cout), kv, tab, n_out, kind, rel in itertools.product(
                        (torch.bfloat16, torch.float32), SHAPES, (1, 9, 27), (table, None), (4095, 4096), ("sparse", "dense"),
                        (None, -1, 0, 1)):
                    # rel None: a SubM conv on its Level; else a strided conv with n_in just below / at / above 16 * n_out
                    g = types.SimpleNamespace(nbr_fwd=tab, nbr_bwd=tab, n_out=n_out, kind=kind, strided=rel is not None,
                                              n_in=n_out if rel is None else 16 * n_out + rel, level=level if rel is None else None)
                    feats = types.SimpleNamespace(dtype=dtype, is_cuda=True, shape=(g.n_in, cin))
                    want = route_as_it_was(feats, cin, cout, kv, g)
                    r = sp._conv_route(feats, (1, 1, kv, cin, cout), g)
                    assert (r.split, r.nmajor, r.halo, r.strided_split) == want, (flags, scope_on, dtype, cin, cout, kv, tab, n_out, rel)
                    assert (r.kvol, r.cin, r.cout) == (kv, cin, cout)
                    seen.add((want[0], want[1], want[2] is not None, want[3]))
    # the product reaches every kind of route: both split kinds, n-major or not, halo, both strided input gradients
    assert {s[0] for s in seen} == {None, "wide", "narrow"} and {s[1] for s in seen} == {True, False}
    assert (None, True, True, False) in seen and (None, True, False, True) in seen and ("wide", False, False, True) in seen
    with pytest.raises(AttributeError):
        r.split = None          # the record is immutable: the backward cannot "re-decide" into it


def test_route_needs_a_device_tensor_for_the_split_kernels():
    g = types.SimpleNamespace(nbr_fwd=object(), nbr_bwd=object(), n_out=100, n_in=100, kind="sparse", strided=False, level=None)
    with sp.split_scope(True):
        if sp.SPLIT_BF16:
            assert sp._conv_route(types.SimpleNamespace(dtype=torch.float32, is_cuda=True), (3, 3, 3, 128, 128), g).split == "wide"
        assert sp._conv_route(types.SimpleNamespace(dtype=torch.float32, is_cuda=False), (3, 3, 3, 128, 128), g).split is None


# ---- native.census_meta: each variant written out with the formula its wrapper carried ---------------------------------------------

def _table(kvol, ld, holes, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 50, (kvol, ld), dtype=torch.int32, generator=g)
    flat = t.view(-1)
    flat[torch.randperm(kvol * ld, generator=g)[:holes]] = -1
    return t


def test_census_entry_of_every_pricing_variant(monkeypatch):
    monkeypatch.setattr(nv, "CALL_KIND", "dense")
    n_in, n_out, cin, cout, kvol = 70, 50, 32, 64, 27
    t = _table(kvol, 56, 200, 0)                     # 56 columns, 50 of them rows of this call
    pairs = int((t[:, :n_out] >= 0).sum())
    assert 0 < kvol * n_out - pairs <= 200 and int((t >= 0).sum()) != pairs
    # bf16 forward (spconv_fwd with statistics, igemm_fwd_affine, igemm_direct_affine)
    assert nv.census_meta(n_in, n_out, cin, cout, kvol, t) == dict(
        kind="dense", v2=True, n_in=n_in, n_out=n_out, cin=cin, cout=cout, kvol=kvol, pairs=pairs,
        bytes=n_in * cin * 2 + n_out * cout * 2 + 8 * pairs + kvol * cin * cout * 2, flops=2 * pairs * cin * cout)
    # f32 on the first-generation kernel (spconv_fwd: element size s everywhere, v2 = whether an implicit-GEMM kernel took it)
    s = 4
    assert nv.census_meta(n_in, n_out, cin, cout, kvol, t, act_bytes=s, v2=False) == dict(
        kind="dense", v2=False, n_in=n_in, n_out=n_out, cin=cin, cout=cout, kvol=kvol, pairs=pairs,
        bytes=n_in * cin * s + n_out * cout * s + 8 * pairs + kvol * cin * cout * s, flops=2 * pairs * cin * cout)
    # weight gradient (spconv_wgrad: the gradient is written in f32)
    for s, v2 in ((2, True), (4, False)):
        assert nv.census_meta(n_in, n_out, cin, cout, kvol, t, act_bytes=s, w_bytes=4, v2=v2) == dict(
            kind="dense", v2=v2, n_in=n_in, n_out=n_out, cin=cin, cout=cout, kvol=kvol, pairs=pairs,
            bytes=n_in * cin * s + n_out * cout * s + 8 * pairs + kvol * cin * cout * 4, flops=2 * pairs * cin * cout)
    # split-wide (spconv_fwd_split): the tripled table (t, t, t + plane) and kvol3 // 3 offsets, priced as the f32 conv it stands for
    t3 = torch.cat([t, t, torch.where(t >= 0, t + n_in, t)], 0)
    kvol3 = t3.shape[0]
    k = kvol3 // 3
    assert nv.census_meta(n_in, n_out, cin, cout, kvol3 // 3, t3, split=True) == dict(
        kind="dense", v2=True, split=True, n_in=n_in, n_out=n_out, cin=cin, cout=cout, kvol=k, pairs=pairs,
        bytes=n_in * cin * 4 + n_out * cout * 4 + 8 * pairs + k * cin * cout * 4, flops=2 * pairs * cin * cout)
    # halo (subm_halo_conv / _affine; subm_halo_wgrad with f32 weights): n_in = n_out = n_cap, pairs from the level's forward table
    n, c = 50, 64
    assert nv.census_meta(n, n, c, c, kvol, t) == dict(
        kind="dense", v2=True, n_in=n, n_out=n, cin=c, cout=c, kvol=kvol, pairs=pairs,
        bytes=n * c * 2 * 2 + 8 * pairs + kvol * c * c * 2, flops=2 * pairs * c * c)
    assert nv.census_meta(n, n, 64, 64, 27, t, w_bytes=4) == dict(
        kind="dense", v2=True, n_in=n, n_out=n, cin=64, cout=64, kvol=27, pairs=pairs,
        bytes=n * 64 * 2 * 2 + 8 * pairs + 27 * 64 * 64 * 4, flops=2 * pairs * 64 * 64)
    # no table (1x1x1): every output row is one pair
    monkeypatch.setattr(nv, "CALL_KIND", "sparse")
    assert nv.census_meta(n_in, n_out, cin, cout, 1, None) == dict(
        kind="sparse", v2=True, n_in=n_in, n_out=n_out, cin=cin, cout=cout, kvol=1, pairs=n_out,
        bytes=n_in * cin * 2 + n_out * cout * 2 + 8 * n_out + 1 * cin * cout * 2, flops=2 * n_out * cin * cout)
    # RevNbr: the wrappers counted over nbr.t.flip(0) - the same count as over the table itself
    rev = nv.RevNbr(t)
    assert int((rev.t.flip(0)[:, :n_out] >= 0).sum()) == pairs
    assert nv.census_meta(n_in, n_out, cin, cout, kvol, rev) == nv.census_meta(n_in, n_out, cin, cout, kvol, t)
    assert nv.census_meta(n_in, n_out, cin, cout, kvol, rev, split=True)["pairs"] == pairs


# ---- native.timed_begin / timed_end ---------------------------------------------------------------------------------------------------

class StubTimer:
    def __init__(self, mode):
        self.mode, self.log, self.counter = mode, [], 0

    def begin(self):
        self.counter += 1
        self.log.append(("begin",))
        return ("event", self.counter)

    def end(self, tag, e0, meta=None):
        self.log.append(("end", tag, e0, meta))


class CountingTable:
    """Stands in for a neighbour table: counts how often the census reads it."""

    def __init__(self, t):
        self.t, self.reads = t, 0

    def __getitem__(self, idx):
        self.reads += 1
        return self.t[idx]


def _launch(table, fail=False):
    """A wrapper's shape: region, launch, end."""
    ran = []
    region = nv.timed_begin()
    if fail:
        raise nv.U3DError("launch failed")
    ran.append(1)
    nv.timed_end(region, "spconv_fwd", 70, 50, 32, 64, 27, table, act_bytes=4)
    return ran


def test_timed_region_without_a_timer_does_nothing(monkeypatch):
    monkeypatch.setattr(nv, "TIMER", None)
    tab = CountingTable(_table(27, 56, 100, 1))
    assert nv.timed_begin() is None
    assert _launch(tab) == [1] and tab.reads == 0


@pytest.mark.parametrize("mode", ["time", "census"])
def test_timed_region_records_one_begin_and_one_end(monkeypatch, mode):
    t = StubTimer(mode)
    monkeypatch.setattr(nv, "TIMER", t)
    monkeypatch.setattr(nv, "CALL_KIND", "sparse")
    table = _table(27, 56, 100, 1)
    tab = CountingTable(table)
    assert _launch(tab) == [1]
    meta = nv.census_meta(70, 50, 32, 64, 27, table, act_bytes=4) if mode == "census" else None
    assert t.log == [("begin",), ("end", "spconv_fwd", ("event", 1), meta)]
    assert tab.reads == (1 if mode == "census" else 0)          # the host-syncing count happens in census mode only
    # a section without shape facts (gtdb_crop's three): no meta in either mode
    nv.timed_end(nv.timed_begin(), "gtdb_scan")
    assert t.log[2:] == [("begin",), ("end", "gtdb_scan", ("event", 2), None)]


def test_timed_region_of_a_launch_that_raises_records_no_end(monkeypatch):
    t = StubTimer("census")
    monkeypatch.setattr(nv, "TIMER", t)
    with pytest.raises(nv.U3DError):
        _launch(None, fail=True)
    assert t.log == [("begin",)]


def test_timed_region_reads_the_timer_at_call_time_and_advances_mark_mode_once(monkeypatch):
    t = nv.KernelTimer("mark", targets=(), per_step=3)          # no targets: no event is ever created
    monkeypatch.setattr(nv, "TIMER", t)
    for i in range(1, 6):
        assert _launch(None) == [1]
        assert t.counter == i
    assert t.marks == {} and t.calls == [] and t.census == []
    monkeypatch.setattr(nv, "TIMER", None)
    _launch(None)
    assert t.counter == 5
