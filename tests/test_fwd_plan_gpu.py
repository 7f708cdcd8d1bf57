"""Every route of the forward launch plan (u3d_igemm_fwd_plan -> native.spconv_fwd) on the device, at the smallest shape that takes it:
bf16 rows, a random table with about 30 % absent neighbours, fewer live rows than the capacity.  Each result is compared with a
float64 gather-and-matmul of the same bf16 inputs, within the bound tests/test_sparse_gpu.py::test_spconv_fwd_bwd_bf16 applies to bf16
forward convolutions (1e-2 of the reference's largest magnitude: the output's bf16 rounding); epilogue statistics the way
test_conv_epilogue_bn_statistics_match_separate_pass compares them (the running statistics they finalise to against those of the
stand-alone pass over the same output, rtol 1e-4 / atol 1e-6); rows at or past *n_out_dev keep a sentinel."""
import pytest
import torch

from uni3detr_amd import native as nv

pytestmark = pytest.mark.gpu
SENT = -77.0

# name -> (n, cin, cout, kvol, table, n-major weights), the kernel the plain plan names (None: first-generation)
SHAPES = {
    "conv_in": ((300, 8, 16, 27, True, False), ("conv_in", "conv_in")),
    "direct_16_32": ((987, 16, 32, 27, True, True), ("direct", "32x32_n")),
    "direct_32_64": ((987, 32, 64, 27, True, True), ("direct", "32x64_n")),
    "glds_64": ((300, 64, 64, 27, True, True), ("glds", "glds_128x64")),
    "glds_128": ((300, 128, 128, 27, True, True), ("glds", "glds_128x128")),
    "glds_256_table_free": ((32513, 256, 256, 1, False, True), ("glds", "glds_256x256")),
    "reg_16_k": ((300, 16, 16, 9, True, False), ("reg", "n16_k")),
    "reg_16_n": ((300, 16, 16, 9, True, True), ("reg", "n16_n")),
    "kmajor_64": ((300, 64, 64, 27, True, False), ("reg", "128x64")),
    "kmajor_128": ((300, 128, 128, 27, True, False), ("reg", "256x128")),
    "first_generation": ((300, 24, 24, 27, True, False), None),
}
# (shape, mode, the addend / the statistics go through the kernel's epilogue)
CASES = [("conv_in", "plain", False), ("conv_in", "add", False),
         ("direct_16_32", "plain", False), ("direct_16_32", "add", True), ("direct_16_32", "stats", True),
         ("direct_32_64", "plain", False), ("direct_32_64", "stats", False),
         ("glds_64", "plain", False), ("glds_64", "add", True), ("glds_64", "stats", True),
         ("glds_128", "plain", False), ("glds_128", "add", True), ("glds_128", "stats", True),
         ("glds_256_table_free", "add", False),
         ("reg_16_k", "plain", False), ("reg_16_n", "plain", False), ("reg_16_n", "add", False),
         ("kmajor_64", "plain", False), ("kmajor_128", "plain", False), ("kmajor_128", "add", False),
         ("first_generation", "plain", False), ("first_generation", "add", False)]


@pytest.fixture(scope="module")
def inputs():
    """inputs(name, device): the inputs and the float64 yardstick of one shape, built once, shared by its cases and freed with the module."""
    cache = {}

    def get(name, dev):
        if name not in cache:
            cache[name] = _build(name, dev)
        return cache[name]
    yield get
    cache.clear()


def _build(name, dev):
    n, cin, cout, kvol, table, nmajor = SHAPES[name][0]
    gen = torch.Generator().manual_seed(1000 * cin + cout + kvol)
    x = torch.randn(n, cin, generator=gen).to(dev).bfloat16()
    w = (torch.randn(kvol, cin, cout, generator=gen) / (kvol * cin) ** 0.5).to(dev).bfloat16()          # [K][Cin][Cout]
    add = torch.randn(n, cout, generator=gen).to(dev).bfloat16()
    nbr = None
    if table:
        t = torch.randint(0, n, (kvol, n), generator=gen, dtype=torch.int32)
        t[torch.rand(kvol, n, generator=gen) < 0.3] = -1
        nbr = t.to(dev).contiguous()
    ref = torch.zeros(n, cout, dtype=torch.float64, device=dev)
    for k in range(kvol):
        idx = nbr[k].long() if table else torch.arange(n, device=dev)
        ref += (x.double()[idx.clamp(min=0)] * (idx >= 0).unsqueeze(1)) @ w[k].double()
    return dict(x=x, w=w.transpose(1, 2).contiguous() if nmajor else w, add=add, nbr=nbr, ref=ref,
                n_dev=torch.tensor([n - 13], dtype=torch.int32, device=dev))


@pytest.mark.parametrize("name,mode,in_epilogue", CASES)
def test_route(cuda, inputs, name, mode, in_epilogue):
    shape, kernel = SHAPES[name]
    n, cin, cout, kvol, table, nmajor = shape
    c = inputs(name, cuda)
    live = n - 13
    plain = nv.fwd_plan(*shape)
    assert (plain and (plain.family, plain.kernel)) == kernel
    plan = nv.fwd_plan(*shape, mode)
    if mode == "add":
        assert (plan and (plan.family, plan.kernel)) == kernel and bool(plan and plan.takes_addend) == in_epilogue
    if mode == "stats":
        assert (plan is not None) == in_epilogue
    addend = c["add"] if mode == "add" else None
    res = nv.spconv_fwd(c["x"], c["w"], c["nbr"], c["n_dev"], n, cout, transpose_w=nmajor, tag="spconv_fwd", addend=addend,
                        want_stats=mode == "stats")
    y, stats, rows = res if mode == "stats" else (res, None, 0)
    ref = c["ref"] + c["add"].double() if mode == "add" else c["ref"]
    err, scale = float((y[:live].double() - ref[:live]).abs().max()), float(ref[:live].abs().max())
    print(f"{name} {mode}: max error {err:.3e} of {scale:.3e}")
    assert err <= 1e-2 * scale
    # the launch itself, into a buffer the test owns: rows past the count stay as they were, the live ones are spconv_fwd's
    out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
    nbr_p, ld = nv._nbr_ptr_ld(c["nbr"])
    ptrs = (nv._ptr(c["x"]), nv._ptr(c["w"]), nbr_p, ld, nv._ptr(out), nv._ptr(c["n_dev"]), n, cin, cout, kvol, int(nmajor))
    st2 = torch.empty_like(stats) if stats is not None else None
    if kernel is None:
        nv._check(nv.lib().u3d_spconv_fwd(*ptrs, nv.BF16, nv._stream()), "spconv_fwd")
    else:
        nv._check(nv.lib().u3d_igemm_fwd_bf16(*ptrs, nv._ptr(addend) if in_epilogue and mode == "add" else None, nv._ptr(st2),
                                              nv._stream()), "igemm_fwd_bf16")
    assert bool((out[live:] == SENT).all())
    if addend is not None and not in_epilogue:
        out[:live] += addend[:live]                                     # added afterwards, as spconv_fwd does
    assert torch.equal(out[:live], y[:live])
    if mode != "stats":
        return
    if not in_epilogue:
        assert stats is None and rows == 0
        return
    assert tuple(stats.shape) == (plan.partials, 2, cout) and rows == plan.rows_per_partial
    run = [[torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)] for _ in range(2)]
    nv.bn_finalize_partials(stats, rows, c["n_dev"], n, 1e-3, 0.01, *run[0])
    nv.bn_forward_stats(y, c["n_dev"], 1e-3, 0.01, *run[1])
    assert torch.allclose(run[0][0], run[1][0], rtol=1e-4, atol=1e-6) and torch.allclose(run[0][1], run[1][1], rtol=1e-4, atol=1e-6)


@pytest.fixture(scope="module")
def exact_inputs():
    """exact_inputs(name, device): integer inputs of one shape and their float64 result, built once and shared like `inputs`."""
    cache = {}

    def get(name, dev):
        if name not in cache:
            cache[name] = _build_exact(name, dev)
        return cache[name]
    yield get
    cache.clear()


def _build_exact(name, dev):
    """x and the addend integers in [-3, 3], w in [-2, 2]: exact in bf16, and every sum an integer of at most 27 * 256 * 6 < 2^24, so
    the f32 accumulator holds the float64 result whatever the order of its additions."""
    n, cin, cout, kvol, table, nmajor = SHAPES[name][0]
    gen = torch.Generator().manual_seed(2000 * cin + cout + kvol)
    x = torch.randint(-3, 4, (n, cin), generator=gen).to(dev).bfloat16()
    w = torch.randint(-2, 3, (kvol, cin, cout), generator=gen).to(dev).bfloat16()                      # [K][Cin][Cout]
    add = torch.randint(-3, 4, (n, cout), generator=gen).to(dev).bfloat16()
    nbr = None
    if table:
        t = torch.randint(0, n, (kvol, n), generator=gen, dtype=torch.int32)
        t[torch.rand(kvol, n, generator=gen) < 0.3] = -1
        nbr = t.to(dev).contiguous()
    ref = torch.zeros(n, cout, dtype=torch.float64, device=dev)
    for k in range(kvol):
        idx = nbr[k].long() if table else torch.arange(n, device=dev)
        ref += (x.double()[idx.clamp(min=0)] * (idx >= 0).unsqueeze(1)) @ w[k].double()
    assert float(ref.abs().max()) < 2 ** 24
    return dict(x=x, w=w.transpose(1, 2).contiguous() if nmajor else w, add=add, nbr=nbr, ref=ref,
                n_dev=torch.tensor([n - 13], dtype=torch.int32, device=dev))


@pytest.mark.parametrize("name,mode,in_epilogue", [c for c in CASES if c[1] in ("plain", "add")])
def test_route_exact(cuda, exact_inputs, name, mode, in_epilogue):
    """Integer operands through every plain / addend route: the accumulator is exact and the kernels round once to bf16, to nearest
    even, so the live rows ARE the float64 reference rounded to bf16 - of conv + addend where the addend goes through the epilogue,
    plus the addend in bf16 where spconv_fwd adds it afterwards.  torch.equal, no tolerance."""
    shape, kernel = SHAPES[name]
    n, cin, cout, kvol, table, nmajor = shape
    c = exact_inputs(name, cuda)
    live = n - 13
    plan = nv.fwd_plan(*shape, mode)
    assert (plan and (plan.family, plan.kernel)) == kernel and (mode != "add" or bool(plan and plan.takes_addend) == in_epilogue)
    addend = c["add"] if mode == "add" else None
    if mode == "plain":
        want = c["ref"].to(torch.bfloat16)
    elif in_epilogue:
        want = (c["ref"] + c["add"].double()).to(torch.bfloat16)
    else:
        want = c["ref"].to(torch.bfloat16) + c["add"]
    y = nv.spconv_fwd(c["x"], c["w"], c["nbr"], c["n_dev"], n, cout, transpose_w=nmajor, tag="spconv_fwd", addend=addend)
    assert torch.equal(y[:live], want[:live])
    # the launch itself, into a buffer the test owns: rows past the count keep the sentinel
    out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
    nbr_p, ld = nv._nbr_ptr_ld(c["nbr"])
    ptrs = (nv._ptr(c["x"]), nv._ptr(c["w"]), nbr_p, ld, nv._ptr(out), nv._ptr(c["n_dev"]), n, cin, cout, kvol, int(nmajor))
    if kernel is None:
        nv._check(nv.lib().u3d_spconv_fwd(*ptrs, nv.BF16, nv._stream()), "spconv_fwd")
    else:
        nv._check(nv.lib().u3d_igemm_fwd_bf16(*ptrs, nv._ptr(addend) if in_epilogue else None, None, nv._stream()), "igemm_fwd_bf16")
    assert bool((out[live:] == SENT).all())
    if addend is not None and not in_epilogue:
        out[:live] += addend[:live]                                     # added afterwards, as spconv_fwd does
    assert torch.equal(out[:live], want[:live])


def test_an_epilogue_the_plan_lacks_is_refused(cuda, inputs):
    """An addend for the register-staged kernels, statistics for 32 -> 64: the entry says so instead of dropping them."""
    for name, addend, stats in (("reg_16_n", True, False), ("direct_32_64", False, True), ("first_generation", False, False)):
        shape = SHAPES[name][0]
        n, cin, cout, kvol, table, nmajor = shape
        c = inputs(name, cuda)
        out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
        st = torch.zeros((64, 2, cout), dtype=torch.float64, device=cuda) if stats else None
        nbr_p, ld = nv._nbr_ptr_ld(c["nbr"])
        rc = nv.lib().u3d_igemm_fwd_bf16(nv._ptr(c["x"]), nv._ptr(c["w"]), nbr_p, ld, nv._ptr(out), nv._ptr(c["n_dev"]), n, cin, cout, kvol,
                                         int(nmajor), nv._ptr(c["add"]) if addend else None, nv._ptr(st), nv._stream())
        assert rc == nv.U3D_ERR_UNSUPPORTED and bool((out == SENT).all())
