"""The launch plan of the implicit-GEMM weight gradient (wgrad_plan in csrc/igemm_wgrad.hip) without a GPU: the plan entry is host
only, so the library answers here.

Where the literal numbers come from.  The WORKSPACE bytes were recorded from the library of the commit before the plan existed, by
calling its u3d_igemm_wgrad_bf16_workspace(n, cin, cout, kvol) for each cell; they are not taken from the code under test.  The
KERNEL, TILE and NSPLIT values are derived by hand from that commit's rules:
  conv-in (8 -> 16, kvol <= 27, [K][Cin][Cout] output): one partial per 128 rows;
  narrow (a table, kvol 27, 16 -> 16 / 16 -> 32 / 32 -> 32 / 32 -> 64): min(ceil(n / 64), 256) rounded up to 8 workgroup partials;
  otherwise the largest square tile T of 256 / 128 / 64 / 32 that divides both channel counts, else 16;
    per = kvol * ceil(cin / T) * ceil(cout / T), target = max(1, (256 if T == 256 else 512 if T >= 64 else 2048) // per),
    nsplit = min(ceil(n / 64), target), lowered until ceil(n / 64) // nsplit >= 8;
    while T > 64 and nsplit * per < 192: the same with T / 2.
  T 256 runs the eight-phase kernel with a neighbour table and the two-phase one without; 128 / 64 the LDS-DMA kernels; 32 / 16 the
  register-staged ones.  nsplit is always workspace / (kvol * cin * cout * 4)."""
import ctypes
import itertools

import pytest

from uni3detr_amd import native as nv

# (n_out_cap, cin, cout, kvol, has_nbr, out_oik) -> (kernel, tile, nsplit, workspace) or None
CELLS = [
    ((128000, 8, 16, 27, 1, 0), ("conv_in", 0, 1000, 13824000)),
    ((1, 8, 16, 1, 0, 0), ("conv_in", 0, 1, 512)),
    ((100000, 16, 16, 27, 1, 0), ("narrow", 0, 256, 7077888)),
    ((100000, 16, 32, 27, 1, 0), ("narrow", 0, 256, 14155776)),
    ((2500, 16, 32, 27, 1, 0), ("narrow", 0, 40, 2211840)),
    ((100000, 32, 32, 27, 1, 1), ("narrow", 0, 256, 28311552)),
    ((100000, 32, 64, 27, 1, 0), ("narrow", 0, 256, 56623104)),
    ((0, 32, 16, 27, 1, 0), ("narrow", 0, 8, 442368)),                       # no rows: the family's zero fill
    ((48000, 256, 256, 27, 1, 0), ("glds8_256", 256, 9, 63700992)),
    ((12000, 512, 512, 27, 1, 0), ("glds8_256", 256, 2, 56623104)),
    ((200000, 256, 256, 1, 0, 0), ("glds_256", 256, 256, 67108864)),         # no table, enough rows to keep the 256 tile
    ((200000, 256, 256, 1, 1, 0), ("glds8_256", 256, 256, 67108864)),
    ((48000, 256, 256, 1, 1, 0), ("glds_128", 128, 93, 24379392)),           # 93 workgroups at 256 < 192: halved once
    ((7200, 512, 512, 1, 0, 0), ("glds_128", 128, 14, 14680064)),            # few rows: 256 -> 128
    ((7200, 256, 256, 1, 0, 0), ("glds_64", 64, 14, 3670016)),               # few rows: 256 -> 128 -> 64
    ((100000, 128, 128, 27, 1, 0), ("glds_128", 128, 18, 31850496)),
    ((48000, 128, 128, 27, 1, 1), ("glds_128", 128, 18, 31850496)),
    ((48000, 128, 256, 9, 1, 0), ("glds_128", 128, 28, 33030144)),
    ((100000, 64, 64, 27, 1, 0), ("glds_64", 64, 18, 7962624)),
    ((100000, 64, 64, 54, 1, 0), ("glds_64", 64, 9, 7962624)),
    ((100000, 64, 32, 27, 1, 0), ("reg_32", 32, 37, 8183808)),
    ((2500, 64, 32, 27, 1, 0), ("reg_32", 32, 5, 1105920)),
    ((100000, 64, 16, 27, 1, 0), ("reg_16", 16, 18, 1990656)),
    ((2500, 64, 16, 27, 1, 0), ("reg_16", 16, 5, 552960)),
    ((100000, 16, 64, 27, 1, 0), ("reg_16", 16, 18, 1990656)),
    ((100000, 48, 48, 27, 1, 0), ("reg_16", 16, 8, 1990656)),
    ((100000, 32, 16, 27, 1, 0), None),                                      # claimed by the narrow family, which has no kernel for it
    ((100000, 64, 64, 54, 1, 1), None),                                      # [Cout][Cin][K] output turns at most 27 offsets
    ((100000, 8, 16, 27, 1, 1), None),                                       # conv-in writes [K][Cin][Cout] only
    ((100000, 8, 16, 28, 1, 0), None),
    ((100000, 24, 32, 27, 1, 0), None),
]


@pytest.mark.parametrize("shape,want", CELLS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else None)
def test_plan_cells(shape, want):
    n, cin, cout, kvol, has_nbr, oik = shape
    got = nv.igemm_wgrad_plan(n, cin, cout, kvol, has_nbr, bool(oik))
    assert got == want
    if want is not None:
        assert want[2] * kvol * cin * cout * 4 == want[3]


def test_every_family_is_reached():
    assert {w[0] for _, w in CELLS if w is not None} == set(nv.WGRAD_KERNELS) - {"none"}


def test_plan_and_workspace_query_agree():
    """The query has no has_nbr / out_layout argument: over a grid of shapes it returns the plan's workspace, which does not depend on
    the table (the launch refuses kvol > 1 without one)."""
    ws = nv.lib().u3d_igemm_wgrad_bf16_workspace
    checked = 0
    for n, cin, cout, kvol in itertools.product((0, 1, 2500, 7200, 48000, 200000), (8, 16, 32, 48, 64, 128, 256, 512),
                                                (16, 32, 64, 128, 256, 512), (1, 9, 27, 54)):
        plans = [nv.igemm_wgrad_plan(n, cin, cout, kvol, has_nbr) for has_nbr in (0, 1)]
        assert (plans[0] is None) == (plans[1] is None)
        if plans[0] is None:
            continue
        assert plans[0][3] == plans[1][3] == int(ws(n, cin, cout, kvol)) > 0
        assert plans[0][1:] == plans[1][1:] and (plans[0][0] == plans[1][0] or plans[1][0] == "glds8_256")
        checked += 1
    assert checked > 900


def test_plan_entry_rejects_null_outputs():
    k = ctypes.c_int32(0)
    assert nv.lib().u3d_igemm_wgrad_plan(1000, 64, 64, 27, 1, 0, ctypes.byref(k), None, None, None) == -1
