"""Times DGR's inlier network (gmf_amd.ResUNetBN2C, D = 6, 'ones' features) on the 6-D correspondences of the 3DMatch demo
fragments (tests/golden/fpfh_demo_clouds.npz): voxel_select at 5 cm, FPFH, find_knn_gpu, inlier_coordinates.

Reports, with device events after warm-up (median, min, max over repeats): the whole forward from image tokens (both pe
variants), the plan build (levels and kernel maps) alone, and each convolution of one forward with its rate of useful work
(2 x pairs x Cin x Cout).  Also the bytes of weight blocks the convolutions fetch, computed from the kernel maps (one Cin x Cout
block per 64 pairs of an offset per output-row group), against the blocks of the offsets present, each read once, and the full
kernels (k^D x Cin x Cout x 4 B each).

Usage: python tools/time_sparse.py [--repeats 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import sparse as SP     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)        # us
    return statistics.median(ts), min(ts), max(ts)


def demo_coords(v=0.05):
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    xyz, feat = [], []
    for c in (z["cloud0"], z["cloud1"]):
        x, f = gmf_amd.fpfh_descriptors(torch.as_tensor(c.astype(np.float32), device=DEV), v, voxelize="select")
        xyz.append(x)
        feat.append(f)
    coords = [torch.cat([torch.zeros((len(x), 1), dtype=torch.int32, device=DEV), torch.floor(x / v).int()], 1) for x in xyz]
    idx1 = gmf_amd.find_knn_gpu(feat[0], feat[1], nn_max_n=-1, knn=1).reshape(-1)
    return gmf_amd.inlier_coordinates(coords[0], coords[1], torch.arange(len(idx1), device=DEV), idx1)


# the convolutions of one forward: (layer index, map index or None, out level, name)
CONVS = [(i, m, lvl, conv) for i, (conv, _, m, lvl) in enumerate(SP.TRUNK)]


def row_groups(K, cin, cout, nsplit, cap):
    """csrc/sparse_conv_plan.hpp: sparse_conv_row_groups (the output-row groups of one convolution)."""
    if K * cin * cout * 4 > (16 << 20):
        return 1
    wgs = nsplit * -(-cout // 64)
    return max(1, min(-(-512 // wgs), -(-cap // 128), 65535))


def weight_bytes(host, m, n_out, cin, cout, K, nsplit, cap):
    """(bytes of W the convolution fetches: one Cin x Cout block per 64 pairs of an offset per output-row group; the bytes of the
    blocks of the offsets present, each once; the full kernel)."""
    full = K * cin * cout * 4
    if m is None:
        return full * ((n_out + 63) // 64), full, full
    rp, pairs = host["maps"][m]
    rp, d = rp.numpy(), pairs[:, 0].numpy()
    G = row_groups(K, cin, cout, nsplit, cap)
    tiles = 0
    for g in range(G):
        lo, hi = n_out * g // G, n_out * (g + 1) // G
        cnt = np.bincount(d[rp[lo]:rp[hi]], minlength=K)
        tiles += int(((cnt + 63) // 64).sum())
    return tiles * cin * cout * 4, len(np.unique(d)) * cin * cout * 4, full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    report = lambda s: (print(s), lines.append(s))    # noqa: E731
    coords = demo_coords()
    M = len(coords)
    feats = torch.ones((M, 1), device=DEV)
    g = torch.Generator().manual_seed(0)
    pt = torch.randn(1, 1200, 128, generator=g).to(DEV)       # a 120 x 160 image pair through the encoder: 15 x 20 tokens each
    qt = torch.randn(1, 1200, 128, generator=g).to(DEV)
    plan = SP.SparsePlan(coords, 4, SP._NET_MAPS)
    host = plan.to_host()
    report(f"demo correspondences at 5 cm: M = {M} rows; level rows {host['counts']}; "
           f"pairs per map {[int(r[-1]) for r, _ in host['maps']]}")
    for pe in (False, True):
        torch.manual_seed(1)
        model = gmf_amd.ResUNetBN2C(1, 1, D=6, pe=pe).to(DEV).eval()
        med, lo, hi = timed(lambda: model(coords, feats, p_tokens=pt, q_tokens=qt), args.repeats)
        report(f"forward pe={pe}: {med:.0f} us (min {lo:.0f}, max {hi:.0f})")
    med, lo, hi = timed(lambda: SP.SparsePlan(coords, 4, SP._NET_MAPS), args.repeats)
    report(f"plan build (4 levels, 10 maps): {med:.0f} us (min {lo:.0f}, max {hi:.0f})")
    L = model._weights(DEV)
    n = host["counts"]
    tot_t, tot_read, tot_present, tot_full = 0.0, 0, 0, 0
    x = {c: torch.randn(M, c, device=DEV) for c in (1, 32, 64, 96, 128, 256)}
    for i, m, lvl, name in CONVS:
        W, sc, sh = L[i]
        K, cin, cout = W.shape
        xa = x[cin] if cin in x else x[256]
        nsplit = SP.layer_nsplit(K, cin, cout)
        med, _, _ = timed(lambda: SP.sparse_conv(plan, m, lvl, xa, W, scale=sc, shift=sh, nsplit=nsplit), args.repeats)
        rd, present, full = weight_bytes(host, m, n[lvl], cin, cout, K, nsplit, M)
        tot_t += med
        tot_read += rd
        tot_present += present
        tot_full += full
        flops = 2 * (int(host["maps"][m][0][-1]) if m is not None else n[lvl]) * cin * cout
        report(f"  {name:16s} level {lvl} rows {n[lvl]:5d} K {K:3d} {cin:3d}->{cout:3d} nsplit {nsplit:3d}: {med:7.1f} us, "
               f"{flops / med / 1e6:6.2f} TFLOP/s of pair work, W fetched {rd / 2**20:7.2f} MiB, present blocks "
               f"{present / 2**20:7.2f} MiB, kernel {full / 2**20:6.2f} MiB")
    report(f"convolutions: {tot_t:.0f} us in all; weight blocks fetched {tot_read / 2**20:.1f} MiB, blocks of the offsets present "
           f"{tot_present / 2**20:.1f} MiB, full kernels {tot_full / 2**20:.1f} MiB")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
