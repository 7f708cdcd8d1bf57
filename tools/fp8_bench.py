"""A/B of the fp8 inference route per dense-stack layer (GPU): u3d_igemm_fwd_affine_bf16 against the quantise pass +
u3d_igemm_fwd_affine_fp8 on the same activations, windows of the two arms alternating in one process.
usage: python tools/fp8_bench.py [--only dense256] [--iters 20] [--windows 7] [--rotate 3]
One line per layer: median [min .. max] ms of each arm over the windows, the ratio of the medians, and whether the fp8 pair is faster
by more than the spread (its slowest window against the bf16 arm's fastest)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uni3detr_amd import native as nv  # noqa: E402
from uni3detr_amd.inference import fp8_exponent  # noqa: E402

LAYERS = {
    # name: (batch, dims(z,y,x), cin, cout, ksize, stride, pad) - SUN RGB-D bench workload (B = 8, 15 x 40 x 40 = 192 000 rows)
    "dense256": (8, (15, 40, 40), 256, 256, (3, 3, 3), (1, 1, 1), (1, 1, 1)),              # the FPN's extra convs: the dominant layer
    "b0_256to128k9": (8, (15, 40, 40), 256, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "b0_128k9": (8, (15, 40, 40), 128, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "b1_stride2_256": (8, (15, 40, 40), 256, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    "b1_256k9": (8, (15, 20, 20), 256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "b2_stride4_512": (8, (15, 40, 40), 256, 512, (1, 3, 3), (1, 4, 4), (0, 1, 1)),
    "b2_512k9": (8, (15, 10, 10), 512, 512, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "fpn_128to256k1": (8, (15, 40, 40), 128, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    # KITTI (B = 4, 5 x 200 x 176 = 704 000 rows)
    "kitti_128k9": (4, (5, 200, 176), 128, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "kitti_256k9": (4, (5, 100, 88), 256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "kitti_512k9": (4, (5, 50, 44), 512, 512, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "kitti_dense256": (4, (5, 200, 176), 256, 256, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=3, help="input tensors cycled through, so the working set exceeds the Infinity Cache")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fmt = lambda v: f"{statistics.median(v):7.4f} [{min(v):7.4f} .. {max(v):7.4f}]"      # noqa: E731
    for name, (B, dims, cin, cout, ks, st, pad) in LAYERS.items():
        if a.only and a.only not in name:
            continue
        dims_out = tuple((d + 2 * p_ - k_) // s_ + 1 for d, k_, s_, p_ in zip(dims, ks, st, pad))
        n_in, n = B * dims[0] * dims[1] * dims[2], B * dims_out[0] * dims_out[1] * dims_out[2]
        kvol = ks[0] * ks[1] * ks[2]
        nbr = nv.dense_nbr_table(B, dims_out, dims, ks, st, pad, 0, dev) if kvol > 1 else None
        nd, nd_in = nv.count_tensor(n, dev), nv.count_tensor(n_in, dev)
        torch.manual_seed(0)
        xs = [torch.relu(torch.randn(n_in, cin, device=dev) * 0.7 + 0.1).bfloat16() for _ in range(a.rotate)]      # post-BatchNorm-ReLU-like rows
        w = torch.randn(kvol, cout, cin, device=dev) * 0.05
        shift = torch.randn(cout, device=dev) * 0.1
        wb = w.bfloat16()
        e_a = fp8_exponent(float(xs[0].abs().max()) * 2.0)
        e_w = [fp8_exponent(v) for v in w.abs().amax(dim=(0, 2)).tolist()]
        e_wd = torch.tensor(e_w, dtype=torch.int32, device=dev)
        qw = torch.empty((kvol, cout, cin), dtype=torch.uint8, device=dev)
        for c in sorted(set(e_w)):                                      # weights through the activation quantiser, one exponent at a time
            sel = (e_wd == c).nonzero().flatten()
            rows = w[:, sel].reshape(-1, cin).bfloat16().contiguous()
            qw[:, sel] = nv.quant_rows_e4m3(rows, nv.count_tensor(c, dev), nv.count_tensor(rows.shape[0], dev)).view(kvol, -1, cin)
        colscale = torch.ldexp(torch.ones(cout, device=dev), e_wd + e_a)
        e_ad = nv.count_tensor(e_a, dev)
        qbuf = torch.empty((n_in, cin), dtype=torch.uint8, device=dev)
        ctr = [0]

        def nxt():
            ctr[0] += 1
            return xs[ctr[0] % a.rotate]
        plan = nv.fwd_fp8_plan(n, cin, cout, kvol, nbr is not None)
        bplan = nv.igemm_fwd_affine_plan(n, cin, cout, kvol, nbr is not None)
        if plan is None:
            print(f"{name:16s} N={n} {cin}->{cout} K={kvol}: the fp8 plan does not serve the shape (bf16: {bplan and bplan[0]})", flush=True)
            continue
        arms = {
            "bf16": lambda: nv.igemm_fwd_affine(nxt(), wb, nbr, shift, True, nd, n),
            "fp8": lambda: nv.igemm_fwd_affine_fp8(nv.quant_rows_e4m3(nxt(), e_ad, nd_in, out=qbuf), qw, nbr, colscale, shift, True, nd, n),
            "fp8conv": lambda: nv.igemm_fwd_affine_fp8(qbuf, qw, nbr, colscale, shift, True, nd, n),
        }
        # same layer, same numbers up to the quantisation: relative L2 of the two outputs
        yb = nv.igemm_fwd_affine(xs[0], wb, nbr, shift, True, nd, n).float()
        yq = nv.igemm_fwd_affine_fp8(nv.quant_rows_e4m3(xs[0], e_ad, nd_in), qw, nbr, colscale, shift, True, nd, n).float()
        rel = float((yq - yb).norm() / yb.norm())
        for fn in arms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(a.windows):
            for k, fn in arms.items():
                t[k].append(window(fn, a.iters))
        mb, mq = statistics.median(t["bf16"]), statistics.median(t["fp8"])
        verdict = "faster beyond the spread" if max(t["fp8"]) < min(t["bf16"]) else ("slower beyond the spread" if min(t["fp8"]) > max(t["bf16"]) else "within the spread")
        print(f"{name:16s} N={n} {cin}->{cout} K={kvol} [{bplan[0]} | {plan.kernel}] ms: bf16 {fmt(t['bf16'])}  quant+fp8 {fmt(t['fp8'])}  "
              f"(fp8 conv alone {fmt(t['fp8conv'])})  bf16/fp8 = {mb / mq:.2f}x  {verdict}  rel L2 {rel:.2e}", flush=True)


if __name__ == "__main__":
    main()
