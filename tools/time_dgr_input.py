"""Times the batched inlier-network input of DGR's training step against what a caller had to write without it.

1. Matching: `find_knn_gpu_batch` on B = 8 pairs with N0, N1 ~ U[3000, 5000] and d = 32 against the loop of `find_knn_gpu` calls
   (three launches against 3 B).  The loop is timed twice (arms "loop" and "loop again"), so the spread between two runs of the
   same code is on the table next to the difference.
2. `generate_inlier_input` on three pairs of the 3DMatch demo fragments (tests/golden/fpfh_demo_clouds.npz, 6.25 cm voxels,
   seeded FCGF) against its pieces by hand: FCGF per side, the loop of find_knn_gpu, inlier_coordinates per pair, and the labels on
   the host in numpy after a device-to-host copy of every pair list.

The arms run in one process and alternate window by window; every window is `--inner` calls that end in a device synchronise,
timed with the host clock; after a warm-up, medians with min and max over `--repeats` windows, in us per call.  Fails without a
GPU.

Usage: python tools/time_dgr_input.py [--repeats 15] [--inner 10] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import fcgf             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternated(arms, repeats, inner, warmup=3):
    """arms: {name: fn}.  -> {name: (median, min, max)} in us per call."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e6 / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def matching_case(dev, B=8, d=32, seed=0):
    rng = np.random.default_rng(seed)
    len_batch = [(int(rng.integers(3000, 5001)), int(rng.integers(3000, 5001))) for _ in range(B)]
    g = torch.Generator().manual_seed(seed)
    F0 = torch.nn.functional.normalize(torch.randn(sum(a for a, _ in len_batch), d, generator=g), dim=1).to(dev)
    F1 = torch.nn.functional.normalize(torch.randn(sum(b for _, b in len_batch), d, generator=g), dim=1).to(dev)
    return F0, F1, len_batch


def knn_loop(F0, F1, len_batch, nn_max_n):
    out, a, b = [], 0, 0
    for n0, n1 in len_batch:
        out.append(gmf_amd.find_knn_gpu(F0[a:a + n0], F1[b:b + n1], nn_max_n=nn_max_n))
        a, b = a + n0, b + n1
    return out


def input_case(dev, voxel=0.0625):
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    c0, c1 = z["cloud0"].astype(np.float32), z["cloud1"].astype(np.float32)
    crops = (c0[c0[:, 0] < np.median(c0[:, 0])], c1[c1[:, 1] < np.median(c1[:, 1])])
    xyz0s, xyz1s, C0, C1 = [], [], [], []

    def vox(xyz, batch):
        x = torch.as_tensor(xyz).to(dev)
        x = x[gmf_amd.voxel_select(x, voxel)].contiguous()
        c = torch.floor(x.double() / voxel).int()
        return x, torch.cat([torch.full((len(c), 1), batch, dtype=torch.int32, device=dev), c], 1)

    for b, (a, c) in enumerate([(c0, c1), (c1, c0), crops]):
        x, cc = vox(a, b)
        xyz0s.append(x), C0.append(cc)
        x, cc = vox(c, b)
        xyz1s.append(x), C1.append(cc)
    torch.manual_seed(5)
    m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3).to(dev).eval()
    return m, xyz0s, xyz1s, torch.cat(C0).contiguous(), torch.cat(C1).contiguous(), [(len(a), len(b)) for a, b in zip(xyz0s, xyz1s)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_dgr_input: no GPU found - timings are taken on the device or not at all")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    F0, F1, len_batch = matching_case(dev)
    same = all(torch.equal(a, b) for a, b in zip(gmf_amd.find_knn_gpu_batch(F0, F1, len_batch), knn_loop(F0, F1, len_batch, -1)))
    say(f"matching: B = {len(len_batch)}, d = 32, len_batch = {len_batch}; batched == loop: {same}")
    res = alternated({"loop": lambda: knn_loop(F0, F1, len_batch, -1),
                      "batched": lambda: gmf_amd.find_knn_gpu_batch(F0, F1, len_batch),
                      "loop again": lambda: knn_loop(F0, F1, len_batch, -1)}, args.repeats, args.inner)
    for k, (med, lo, hi) in res.items():
        say(f"  {k:12s} median {med:9.1f} us   min {lo:9.1f}   max {hi:9.1f}   ({args.repeats} windows of {args.inner} calls)")
    say(f"  loop / batched = {res['loop'][0] / res['batched'][0]:.2f}; loop / loop again = {res['loop'][0] / res['loop again'][0]:.3f}")

    m, xyz0s, xyz1s, iC0, iC1, lb = input_case(dev)
    off0 = np.concatenate([[0], np.cumsum([a for a, _ in lb])])
    off1 = np.concatenate([[0], np.cumsum([b for _, b in lb])])
    Ts = torch.eye(4, dtype=torch.float64).repeat(len(lb), 1, 1)
    pos = gmf_amd.matching_indices_batched(torch.cat(xyz0s), off0.tolist(), torch.cat(xyz1s), off1.tolist(), Ts, 2 * 0.0625)
    pos_off = pos[1].tolist()
    pos_host = [pos[0][pos_off[b]:pos_off[b + 1]].cpu().numpy() for b in range(len(lb))]
    one0, one1 = torch.ones((len(iC0), 1), device=dev), torch.ones((len(iC1), 1), device=dev)

    def by_hand():
        G0, G1 = m(iC0, one0), m(iC1, one1)
        coords, labels = [], []
        for b, (n0, n1) in enumerate(lb):
            nn = gmf_amd.find_knn_gpu(G0[off0[b]:off0[b + 1]], G1[off1[b]:off1[b + 1]], nn_max_n=250).reshape(-1)
            idx0 = torch.arange(n0, device=dev)
            coords.append(gmf_amd.inlier_coordinates(iC0[off0[b]:off0[b + 1]], iC1[off1[b]:off1[b + 1]], idx0, nn))
            seed = max(n0, n1)
            labels.append(np.isin(np.arange(n0) + nn.cpu().numpy() * seed, pos_host[b][:, 0] + pos_host[b][:, 1] * seed))
        return torch.cat(coords), torch.ones((off0[-1], 1), device=dev), torch.as_tensor(np.concatenate(labels)).to(dev)

    def built():
        return gmf_amd.generate_inlier_input(m, xyz0s, xyz1s, iC0, iC1, one0, one1, lb, pos, inlier_feature_type="ones", nn_max_n=250)

    a, b = by_hand(), built()
    say(f"generate_inlier_input: len_batch = {lb}, {pos[0].shape[0]} positive pairs; rows equal: {torch.equal(a[0], b[0])}, "
        f"labels equal: {torch.equal(a[2], b[3])}")
    res = alternated({"by hand": by_hand, "built": built, "by hand again": by_hand}, args.repeats, max(1, args.inner // 2))
    for k, (med, lo, hi) in res.items():
        say(f"  {k:14s} median {med:9.1f} us   min {lo:9.1f}   max {hi:9.1f}")
    say(f"  by hand / built = {res['by hand'][0] / res['built'][0]:.2f}")
    say(f"matching_indices_batched on the same three pairs ({pos[0].shape[0]} pairs out):")
    res = alternated({"matching_indices": lambda: gmf_amd.matching_indices_batched(
        torch.cat(xyz0s), off0.tolist(), torch.cat(xyz1s), off1.tolist(), Ts, 2 * 0.0625)}, args.repeats, max(1, args.inner // 2))
    med, lo, hi = res["matching_indices"]
    say(f"  median {med:9.1f} us   min {lo:9.1f}   max {hi:9.1f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
