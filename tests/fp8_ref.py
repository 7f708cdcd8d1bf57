"""Reference side of the fp8 (OCP e4m3fn) inference tests: the quantiser and the scale formulas restated with torch on the CPU, float64
restatements of the weight fold and of the convolution, and the emulation of the fp8 convolution on the bf16 kernel
(u3d_igemm_fwd_affine_bf16 with the codes as bf16 rows and qw * 2^(e_a + e_w) as bf16 weights: both exact, the same real arithmetic in
another summation order).  Nothing here calls the code under test."""
import torch

E4M3_MAX = 448.0


def quant_ref(x, e):
    """-> (codes uint8, nan mask): q(x, e) = e4m3_rne(clamp(x * 2^-e, -448, 448)) on the CPU.  torch rounds to nearest even and does
    not saturate (470 -> NaN), hence the clamp; NaN stays NaN through it."""
    q = x.detach().cpu().float().mul(2.0 ** -e).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), q.float().isnan()


def lut(device="cpu"):
    """f32 value of each of the 256 codes (NaN for 0x7f / 0xff)."""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().to(device)


def dequant(codes, table=None):
    table = lut(codes.device) if table is None else table
    return table[codes.long()]


def exponent_ref(x):
    """Smallest integer e with x <= 448 * 2^e (exact float comparisons; 448 * 2^e is exact in float64); 0 for x == 0."""
    x = float(x)
    if x == 0.0:
        return 0
    e = 0
    while x > E4M3_MAX * 2.0 ** e:
        e += 1
    while x <= E4M3_MAX * 2.0 ** (e - 1):
        e -= 1
    return e


def koi64(w, layout):
    """f64 [kvol, Cout, Cin] view of a master weight in its checkpoint layout."""
    if layout == "dhwio":
        kd, kh, kw, cin, cout = w.shape
        return w.double().reshape(kd * kh * kw, cin, cout).permute(0, 2, 1).contiguous()
    cout, cin = w.shape[:2]
    return w.double().reshape(cout, cin, -1).permute(2, 0, 1).contiguous()


def fold64(w, layout, gamma, beta, mean, var, eps):
    """-> (w_folded f64 [kvol, Cout, Cin], shift f64 [Cout]) of conv weight x eval-mode BatchNorm."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return koi64(w, layout) * scale[None, :, None], beta.double() - mean.double() * scale


def conv64(a, w, nbr):
    """sum_k a[nbr[k]] @ w[k]^T in float64; a [n_in, Cin], w [kvol, Cout, Cin], nbr int32 [kvol, n] (-1: absent) or None (kvol 1)."""
    a, w = a.double(), w.double()
    if nbr is None:
        return a @ w[0].t()
    out = torch.zeros(nbr.shape[1], w.shape[1], dtype=torch.float64, device=a.device)
    for k in range(w.shape[0]):
        idx = nbr[k].long()
        out += (a[idx.clamp(min=0)] * (idx >= 0).unsqueeze(1)) @ w[k].t()
    return out


def conv_fp8_ref64(qa, qw, nbr, colscale, shift, relu, table=None):
    """-> (y f64, bound term f64): act(conv(deq qa; deq qw) * colscale + shift) and colscale * sum |qa| |qw| (the accumulation term)."""
    a, w = dequant(qa, table), dequant(qw, table)
    y = conv64(a, w, nbr) * colscale.double()[None] + shift.double()[None]
    mag = conv64(a.abs(), w.abs(), nbr) * colscale.double()[None]
    return (torch.relu(y) if relu else y), mag


def emulate_on_bf16(nv, qa, qw, nbr, colscale, shift, relu, n_out_dev, n_out, out=None, table=None):
    """The fp8 convolution on the bf16 kernel: codes as bf16 rows (every e4m3 value is a bf16 number), qw * colscale as bf16 weights
    (a power-of-two scale: exact)."""
    a = dequant(qa, table).bfloat16()
    w = (dequant(qw, table) * colscale[None, :, None]).bfloat16()
    return nv.igemm_fwd_affine(a, w.contiguous(), nbr, shift, relu, n_out_dev, n_out, out=out)
