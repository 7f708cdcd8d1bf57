"""Inputs and the float64 yardstick of the weight-gradient route tests (tests/test_wgrad_plan_gpu.py on the device,
tests/test_wgrad_exact_cpu.py for the yardstick itself).  Plain torch, any device.

    P[k][ci][co] = sum over m < n_dev of  in[nbr[k][m]][ci] * dout[m][co]        (no table: in row m pairs with dout row m)

One cell's inputs (make_inputs):
  in    bf16 [cap + 517, cin]: more rows than dout, as in a strided convolution and in the exchanged-operand call; the first
        n_dev + 200 are live, the rest NaN;
  dout  bf16 [cap, cout]: the first n_dev rows live, the rest NaN;
  nbr   int32 [kvol, ld], ld = round_up(cap, 128) + 128 (a leading dimension above the capacity).  Columns below n_dev: uniform over
        the live input rows, repeats allowed, about 30 % absent (-1).  Columns at or past n_dev name NaN input rows only: a kernel
        that consumes one of them poisons its sum.
Exact operands are integers in [-3, 3]: exact in bf16, every product and partial sum an integer far below 2^24, so an f32 sum in any
order, split and tree IS the float64 one.  Random sums of so few terms stay small, though (64 rows: about 120 at the most), and a
sum below 256 is exact in bf16 as well; so input channel 1 is 3 and output channel cout - 2 is -3 on every live row: that one
element is -9 times the present neighbours of the offset, past 256 from 64 rows on.  Rounding operands are Gaussian."""
import torch

IN_EXTRA, LIVE_EXTRA, ABSENT = 517, 200, 0.3
NAN = float("nan")


def table_ld(cap):
    return (cap + 127) // 128 * 128 + 128


def make_inputs(cap, cin, cout, kvol, table, n_dev, dev, exact, seed):
    """-> (in, dout, nbr or None) of one cell at one live count, on dev."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    n_in, live_in = cap + IN_EXTRA, n_dev + LIVE_EXTRA

    def draw(rows, cols):
        if exact:
            return torch.randint(-3, 4, (rows, cols), generator=gen, device=dev).to(torch.bfloat16)
        return torch.randn(rows, cols, generator=gen, device=dev).to(torch.bfloat16)
    x, dy = draw(n_in, cin), draw(cap, cout)
    if exact:
        x[:, 1], dy[:, cout - 2] = 3, -3
    x[live_in:], dy[n_dev:] = NAN, NAN
    if not table:
        return x, dy, None
    nbr = torch.randint(live_in, n_in, (kvol, table_ld(cap)), generator=gen, device=dev, dtype=torch.int32)
    if n_dev > 0:
        live = torch.randint(0, live_in, (kvol, n_dev), generator=gen, device=dev, dtype=torch.int32)
        live[torch.rand(kvol, n_dev, generator=gen, device=dev) < ABSENT] = -1
        nbr[:, :n_dev] = live
    return x, dy, nbr.contiguous()


def reference(x, dy, nbr, n_dev, kvol, absolute=False):
    """P float64 [kvol, cin, cout]; absolute: the same sums over |in| and |dout| (the A of a rounding bound)."""
    xd, dd = x.double(), dy[:n_dev].double()
    if absolute:
        xd, dd = xd.abs(), dd.abs()
    out = torch.zeros(kvol, x.shape[1], dy.shape[1], dtype=torch.float64, device=x.device)
    for k in range(kvol):
        if nbr is None:
            g = xd[:n_dev]
        else:
            idx = nbr[k, :n_dev].long()
            g = torch.where((idx >= 0).unsqueeze(1), xd[idx.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=x.device))
        out[k] = g.t() @ dd
    return out


def in_layout(p, layout):
    """The reference as u3d_igemm_wgrad_bf16 lays it out: 0 [K][Cin][Cout], 1 [Cout][Cin][K], 2 [Cin][Cout][K]."""
    return (p, p.permute(2, 1, 0), p.permute(1, 2, 0))[layout].contiguous()
