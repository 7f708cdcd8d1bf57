"""The launch plan of the forward / input-gradient implicit GEMM (fwd_plan in csrc/igemm_bf16.hip) without a GPU: the plan entry is
host only, so the library answers here.  And native.spconv_fwd on a recording stub of the library: one launch per call, to the entry
the trial-launch ladder it replaces ended on.

Where the literal cells come from.  They are derived by hand from the rules of the commit before u3d_igemm_fwd_plan existed, where
u3d_igemm_fwd_bf16 dispatched in this order (first match wins; n = n_out_cap, tiles = ceil(n / 256)):
  1. k-major weights, 8 -> 16, kvol <= 27: the input convolution (256 rows per workgroup, 16 columns).  No addend, no statistics.
  2. a table, kvol 27, (cin, cout) in {16, 32} x {16, 32, 64} or 64 -> {16, 32}: the direct-operand kernel <padded cin 32 / 64>x<cout>
     in the weights' layout, 64-row tiles per wave, addend epilogue; statistics only n-major and cout <= 32.  Waves per workgroup: 8
     for 32x64 and 64x32, else 4; grid = ceil(ceil(n / 64) / waves) rounded up to 8 (small n: the tiles bound it, not the CUs);
     statistics partials = grid * waves, one per wave (rows per partial 0).
       987 rows: 16 tiles; 4 waves -> 4 -> 8 workgroups -> 32 partials; 8 waves -> 2 -> 8 workgroups -> 64 partials.
  3. n-major weights, cin % 64 == 0, cout % 64 == 0, n > 0: the LDS-DMA kernels, all with a statistics epilogue (one partial per row
     tile), all but the two-phase 256 x 256 with an addend epilogue:
       cout % 256 == 0 and tiles * cout / 256 >= 128: no table -> two-phase 256 x 256; a table -> eight-phase 256 x 256, or 192 x 256
         where the 192-row rule applies (tests/test_plugin_cpu.py::STATS_LAYOUT pins it: 32513 and 48000 rows x 256 -> 192-row
         tiles, 49153 rows -> 256);
       else a table, cout % 128 == 0, kvol * cin / 64 >= 48, tiles * cout / 128 >= 160: eight-phase 256 x 128 (192 x 128: 40705 rows x
         128 -> 192, STATS_LAYOUT);
       else 128 x 128 if cout % 128 == 0, else 128 x 64.
     An eval-mode BatchNorm shift (AFFINE) follows rule 3 only.
  4. n > 0, cin in {16, 32}, cout in {16, 32, 64}: register-staged 256 x cout tiles in the weights' layout.  (64 -> 16 / 32 is
     excluded: measured slower than the first-generation kernel.)  No addend, no statistics.
  5. n > 0, k-major weights, cin % 64 == 0, cout % 64 == 0: register-staged wide tiles.  cout % 256 == 0: 256 x 128 if tiles * cout /
     256 < 128, else 256 x 256; else cout % 128 == 0: 256 x 128; else 128 x 64.  No addend, no statistics.
       12000 rows x 512: 47 * 2 = 94 < 128 -> 256 x 128.  48000 rows x 256: 188 >= 128 -> 256 x 256.
  6. Otherwise no second-generation kernel: native.spconv_fwd launched the first-generation u3d_spconv_fwd.
u3d_igemm_fwd_add_bf16 served exactly the kernels with an addend epilogue (rule 2, rule 3 but the two-phase 256 x 256) and the caller
added afterwards elsewhere: the query asked with "add" answers the plain plan with takes_addend False there.
u3d_igemm_fwd_stats_bf16 (n-major weights only) served rule 2's statistics kernels and rule 3: "stats" is None elsewhere."""
import ctypes

import pytest
import torch

from uni3detr_amd import native as nv

# (n_out_cap, cin, cout, kvol, has_nbr, nmajor, epi) -> (family, kernel, tile rows, tile columns, statistics partials, takes_addend)
CELLS = [
    # 1. the input convolution: k-major against n-major weights, more than 27 offsets, the epilogues it does not have
    ((128000, 8, 16, 27, 1, 0, "plain"), ("conv_in", "conv_in", 256, 16, 0, False)),
    ((300, 8, 16, 27, 1, 0, "add"), ("conv_in", "conv_in", 256, 16, 0, False)),
    ((300, 8, 16, 1, 0, 0, "plain"), ("conv_in", "conv_in", 256, 16, 0, False)),
    ((300, 8, 16, 27, 1, 1, "plain"), None),
    ((300, 8, 16, 28, 1, 0, "plain"), None),
    ((300, 8, 16, 27, 1, 0, "stats"), None),
    # 2. direct-operand kernels
    ((987, 16, 32, 27, 1, 1, "plain"), ("direct", "32x32_n", 64, 32, 32, True)),
    ((987, 16, 32, 27, 1, 1, "add"), ("direct", "32x32_n", 64, 32, 32, True)),
    ((987, 16, 32, 27, 1, 1, "stats"), ("direct", "32x32_ns", 64, 32, 32, False)),
    ((987, 16, 32, 27, 1, 0, "add"), ("direct", "32x32_k", 64, 32, 32, True)),
    ((987, 16, 32, 27, 1, 0, "stats"), None),                                  # statistics need n-major weights
    ((987, 32, 64, 27, 1, 1, "plain"), ("direct", "32x64_n", 64, 64, 64, True)),
    ((987, 32, 64, 27, 1, 1, "stats"), None),                                  # no statistics kernel for 64 columns
    ((987, 64, 32, 27, 1, 0, "plain"), ("direct", "64x32_k", 64, 32, 64, True)),
    ((987, 64, 16, 27, 1, 1, "stats"), ("direct", "64x16_ns", 64, 16, 32, False)),
    ((987, 16, 16, 27, 1, 0, "plain"), ("direct", "32x16_k", 64, 16, 32, True)),      # 16 -> 16 at 27 offsets: direct ...
    ((987, 16, 16, 9, 1, 0, "plain"), ("reg", "n16_k", 256, 16, 0, False)),           # ... at 9: register-staged
    ((987, 16, 32, 27, 1, 1, "affine"), None),
    # 3. LDS-DMA kernels
    ((300, 64, 64, 27, 1, 1, "plain"), ("glds", "glds_128x64", 128, 64, 3, True)),
    ((300, 64, 64, 27, 1, 1, "stats"), ("glds", "glds_128x64", 128, 64, 3, True)),
    ((300, 128, 128, 27, 1, 1, "add"), ("glds", "glds_128x128", 128, 128, 3, True)),
    ((300, 128, 128, 27, 1, 1, "affine"), ("glds", "glds_128x128", 128, 128, 3, True)),
    ((32513, 256, 256, 1, 0, 1, "plain"), ("glds", "glds_256x256", 256, 256, 128, False)),
    ((32513, 256, 256, 1, 0, 1, "add"), ("glds", "glds_256x256", 256, 256, 128, False)),      # ADD for a kernel without that epilogue
    ((32513, 256, 256, 1, 0, 1, "stats"), ("glds", "glds_256x256", 256, 256, 128, False)),
    ((32512, 256, 256, 1, 0, 1, "add"), ("glds", "glds_128x128", 128, 128, 254, True)),       # 127 workgroups: the 128-row tile
    ((32513, 256, 256, 27, 1, 1, "add"), ("glds", "glds8_192x256", 192, 256, 170, True)),
    ((49153, 256, 256, 27, 1, 1, "plain"), ("glds", "glds8_256x256", 256, 256, 193, True)),
    ((32512, 256, 256, 27, 1, 1, "plain"), ("glds", "glds8_256x128", 256, 128, 127, True)),
    ((40705, 128, 128, 27, 1, 1, "stats"), ("glds", "glds8_192x128", 192, 128, 213, True)),
    ((0, 64, 64, 27, 1, 1, "plain"), None),
    # 4. register-staged narrow kernels: every width in both layouts; the shapes next to them
    ((300, 16, 16, 9, 1, 1, "plain"), ("reg", "n16_n", 256, 16, 0, False)),
    ((300, 16, 32, 9, 1, 0, "add"), ("reg", "n32_k", 256, 32, 0, False)),
    ((300, 32, 32, 1, 0, 1, "plain"), ("reg", "n32_n", 256, 32, 0, False)),            # no table: not a direct-operand shape
    ((300, 32, 64, 9, 1, 0, "plain"), ("reg", "n64_k", 256, 64, 0, False)),
    ((300, 16, 64, 1, 0, 1, "plain"), ("reg", "n64_n", 256, 64, 0, False)),
    ((300, 16, 16, 9, 1, 1, "stats"), None),
    ((0, 16, 16, 9, 1, 0, "plain"), None),
    ((12240, 64, 32, 9, 1, 0, "plain"), None),                                  # 64 -> 32 k-major off the direct shapes: first-generation
    ((12240, 64, 16, 9, 1, 1, "plain"), None),
    ((300, 24, 24, 27, 1, 0, "plain"), None),
    ((300, 24, 24, 27, 1, 1, "plain"), None),
    ((300, 48, 48, 27, 1, 0, "plain"), None),
    # 5. register-staged wide kernels (k-major weights)
    ((12000, 512, 512, 27, 1, 0, "plain"), ("reg", "256x128", 256, 128, 0, False)),    # 94 workgroups at 256 columns < 128
    ((48000, 256, 256, 27, 1, 0, "plain"), ("reg", "256x256", 256, 256, 0, False)),    # 188
    ((32512, 256, 256, 1, 0, 0, "plain"), ("reg", "256x128", 256, 128, 0, False)),     # 127
    ((32513, 256, 256, 1, 0, 0, "add"), ("reg", "256x256", 256, 256, 0, False)),       # 128
    ((300, 128, 128, 27, 1, 0, "plain"), ("reg", "256x128", 256, 128, 0, False)),
    ((300, 128, 384, 27, 1, 0, "plain"), ("reg", "256x128", 256, 128, 0, False)),
    ((300, 64, 64, 27, 1, 0, "add"), ("reg", "128x64", 128, 64, 0, False)),
    ((300, 128, 64, 1, 0, 0, "plain"), ("reg", "128x64", 128, 64, 0, False)),
    ((300, 64, 64, 27, 1, 0, "stats"), None),
    ((300, 64, 64, 27, 1, 0, "affine"), None),
    ((0, 64, 64, 27, 1, 0, "plain"), None),
]


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else None


@pytest.mark.parametrize("shape,want", CELLS, ids=_id)
def test_plan_cells(shape, want):
    got = nv.fwd_plan(*shape)
    assert (got if got is None else (got.family, got.kernel, got.rows, got.cols, got.partials, got.takes_addend)) == want
    if got is not None:
        assert got.rows_per_partial == (got.rows if got.family == "glds" else 0)


def test_every_family_and_every_register_staged_slot_is_reached():
    served = [w for _, w in CELLS if w is not None]
    assert {w[0] for w in served} == set(nv.FWD_FAMILIES) - {"none"} == set(nv.FWD_KERNELS)
    assert {w[1] for w in served if w[0] == "reg"} == set(nv.FWD_KERNELS["reg"])


def test_plan_entry_rejects_bad_arguments():
    info = nv.FwdPlanInfo()
    assert nv.lib().u3d_igemm_fwd_plan(1000, 64, 64, 27, 1, 1, 0, None) == -1
    for epi in (-1, len(nv.FWD_EPI)):
        assert nv.lib().u3d_igemm_fwd_plan(1000, 64, 64, 27, 1, 1, epi, ctypes.byref(info)) == -1


# ---- native.spconv_fwd: one plan query, one launch ---------------------------------------------------------------------------------
def ladder_as_it_was(bf16, ld, addend_ok, want_stats, served):
    """Where the trial launches of the commit before ended.  served[epi]: the entry of that epilogue returned 0 for the shape
    (u3d_igemm_fwd_stats_bf16 was only tried after its layout query answered with at least one partial; u3d_igemm_fwd_add_bf16 returned
    U3D_ERR_UNSUPPORTED for a kernel without the addend epilogue).  -> (entry, addend in the epilogue, v2)."""
    UNSUPPORTED = -2
    if want_stats and bf16 and nv.USE_IGEMM_V2 and served["stats"]:               # sparse._SparseConv.forward tried this one first
        return "stats", False, True
    rc, entry, taken = UNSUPPORTED, None, False
    if addend_ok and bf16 and nv.USE_IGEMM_V2 and ld != 0:
        entry, rc = "add", 0 if served["add"] else UNSUPPORTED
        taken = rc == 0
    if rc == UNSUPPORTED and bf16 and nv.USE_IGEMM_V2:
        entry, rc = "plain", 0 if served["plain"] else UNSUPPORTED
    if rc == UNSUPPORTED:
        entry = "first_generation"
    return entry, taken, rc == 0


class _Recorder:
    """Stands in for the library: the plan query is the real one, the launch entries record their arguments, zero the output and
    return `rc`."""

    def __init__(self, rc=0):
        self.real, self.rc, self.launches, self.queries = nv.lib(), rc, [], 0
        self.u3d_strerror = self.real.u3d_strerror

    def u3d_igemm_fwd_plan(self, *a):
        self.queries += 1
        return self.real.u3d_igemm_fwd_plan(*a)

    def u3d_igemm_fwd_bf16(self, inp, w, nbr, ld, out, n_dev, n, cin, cout, kvol, tw, addend, stats, s):
        ctypes.memset(out, 0, n * cout * 2)
        self.launches.append(("igemm", dict(shape=(n, cin, cout, kvol, ld, tw), addend=addend, stats=stats)))
        return self.rc

    def u3d_spconv_fwd(self, inp, w, nbr, ld, out, n_dev, n, cin, cout, kvol, tw, dtype, s):
        ctypes.memset(out, 0, n * cout * (2 if dtype == nv.BF16 else 4))
        self.launches.append(("first_generation", dict(shape=(n, cin, cout, kvol, ld, tw), dtype=dtype)))
        return self.rc


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(nv, "lib", lambda: rec)
    monkeypatch.setattr(nv, "_ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(nv, "_stream", lambda: None)
    return rec


SHAPES = sorted({s[:6] for s, _ in CELLS if s[0] > 0})


def _call(shape, dtype, with_addend, want_stats):
    n, cin, cout, kvol, has_nbr, nmajor = shape
    inp = torch.zeros((1, cin), dtype=dtype)
    w = torch.zeros((kvol, 1, 1), dtype=dtype)
    nbr = torch.zeros((kvol, 1), dtype=torch.int32) if has_nbr else None         # (never read: ld = 1)
    addend = torch.ones((n, cout), dtype=dtype) if with_addend else None
    res = nv.spconv_fwd(inp, w, nbr, torch.zeros(1, dtype=torch.int32), n, cout, transpose_w=bool(nmajor), addend=addend,
                        want_stats=want_stats)
    return res, addend


@pytest.mark.parametrize("with_addend,want_stats", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_spconv_fwd_is_one_launch_where_the_ladder_ended(recorder, shape, with_addend, want_stats):
    n, cin, cout, kvol, has_nbr, nmajor = shape
    plans = {epi: nv.fwd_plan(*shape, epi) for epi in ("plain", "add", "stats")}
    served = dict(plain=plans["plain"] is not None, add=plans["add"] is not None and plans["add"].takes_addend,
                  stats=plans["stats"] is not None and plans["stats"].partials > 0)
    entry, taken, v2 = ladder_as_it_was(True, has_nbr, with_addend, want_stats, served)
    recorder.queries = 0                                  # (the three above)
    res, addend = _call(shape, torch.bfloat16, with_addend, want_stats)
    out, stats, rows = res if want_stats else (res, None, 0)
    assert len(recorder.launches) == 1 and recorder.queries == (2 if want_stats and entry != "stats" else 1)
    name, args = recorder.launches[0]
    assert name == ("first_generation" if entry == "first_generation" else "igemm")
    assert args["shape"] == (n, cin, cout, kvol, 1 if has_nbr else 0, nmajor)
    if name == "igemm":
        assert (args["addend"] is not None) == taken == (entry == "add") and (args["stats"] is not None) == (entry == "stats")
        assert args["addend"] in (None, addend.data_ptr() if with_addend else None)
    if entry == "stats":
        assert tuple(stats.shape) == (plans["stats"].partials, 2, cout) and stats.dtype == torch.float64
        assert args["stats"] == stats.data_ptr() and rows == plans["stats"].rows_per_partial
    else:
        assert stats is None and rows == 0
    # the stub zeroes the output: ones = added after the launch, exactly when the epilogue did not take the addend
    assert bool((out == (1 if with_addend and not taken else 0)).all())


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_census_v2_flag_is_a_found_plan(recorder, monkeypatch, shape):
    seen = []
    monkeypatch.setattr(nv, "timed_begin", lambda: "region")
    monkeypatch.setattr(nv, "timed_end", lambda region, tag, *a, **price: seen.append((tag, price["v2"])))
    _call(shape, torch.bfloat16, True, False)
    entry, _, v2 = ladder_as_it_was(True, shape[4], True, False, dict(
        plain=nv.fwd_plan(*shape) is not None, add=getattr(nv.fwd_plan(*shape, "add"), "takes_addend", False), stats=False))
    assert seen == [("spconv_dgrad" if shape[5] else "spconv_fwd", v2)]


@pytest.mark.parametrize("dtype,v2_on", [(torch.float32, True), (torch.bfloat16, False)])
def test_f32_rows_and_the_v2_switch_skip_the_query(recorder, monkeypatch, dtype, v2_on):
    monkeypatch.setattr(nv, "USE_IGEMM_V2", v2_on)
    for shape in ((300, 64, 64, 27, 1, 1), (987, 16, 32, 27, 1, 0)):
        for with_addend, want_stats in ((False, False), (True, False), (False, True)):
            recorder.launches.clear()
            recorder.queries = 0
            res, _ = _call(shape, dtype, with_addend, want_stats)
            out, stats, rows = res if want_stats else (res, None, 0)
            assert recorder.queries == 0 and [l[0] for l in recorder.launches] == ["first_generation"]
            assert ladder_as_it_was(dtype == torch.bfloat16, 1, with_addend, want_stats, dict(plain=True, add=True, stats=True)) == \
                ("first_generation", False, False)
            assert recorder.launches[0][1]["dtype"] == (nv.BF16 if dtype == torch.bfloat16 else nv.F32)
            assert stats is None and rows == 0 and bool((out == (1 if with_addend else 0)).all())


def test_an_unsupported_launch_raises(monkeypatch, recorder):
    recorder.rc = nv.U3D_ERR_UNSUPPORTED
    for shape, dtype in (((300, 64, 64, 27, 1, 1), torch.bfloat16), ((300, 24, 24, 27, 1, 0), torch.bfloat16),
                         ((300, 64, 64, 27, 1, 1), torch.float32)):
        with pytest.raises(nv.U3DError):
            _call(shape, dtype, False, False)
