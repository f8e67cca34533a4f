"""FCGF training, conv1's weight gradient and the whole step (fcgf_train forward + hardest-contrastive loss + backward), with
conv1 on the narrow-input kernels (--narrow 1) or on the generic ones (--narrow 0); without --narrow both run alternating in
one process, warm, and the second round is reported: median and (min, max) of repeated timed loops.  Sizes: the 3DMatch demo
pair of tests/golden at 5 cm, and a synthetic batch of 2 x 30 000 voxels (two noisy spherical shells); conv1 7^3, 32 features,
normalised.  The step's time includes the plan build and the one host read of the level counts.
GPU box:  python tools/fcgf_train_ab.py [--narrow 0|1] [--loops 7] [--reps 5] [--sizes demo,synthetic]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmf_amd                                     # noqa: E402
from gmf_amd import fcgf                           # noqa: E402
from gmf_amd import sparse as SP                   # noqa: E402
from gmf_amd import train as T                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--narrow", type=int, choices=(0, 1), default=None, help="conv1 on the narrow kernels (1) or the generic ones (0); default: both")
ap.add_argument("--loops", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="demo,synthetic")
args = ap.parse_args()
dev = torch.device("cuda:0")
VOXEL, K1 = 0.05, 7


def timed(fn):
    """Median and (min, max) in ms over `loops` timed loops of `reps` calls, after three warm-up calls."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(args.loops):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / args.reps * 1e3)
    return statistics.median(out), min(out), max(out)


def demo_pair():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    xyz = []
    for c in (z["cloud0"], z["cloud1"]):
        p = torch.as_tensor(c.astype(np.float32)).to(dev)
        xyz.append(p[gmf_amd.voxel_select(p, VOXEL)])
    n0, n1 = len(xyz[0]), len(xyz[1])
    vox = [torch.floor(x.double() / VOXEL).to(torch.int32) for x in xyz]
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None]
    pairs, _ = gmf_amd.matching_indices_batched(xyz[0], [0, n0], xyz[1], [0, n1], eye, 1.5 * VOXEL)
    return vox, pairs


def synthetic_pair(n=30000, seed=0):
    """Two clouds of n voxels each: the same spherical shell seen twice (the second shifted by one voxel in x), pairs (i, i)."""
    rng = np.random.default_rng(seed)
    r = (n / (4 * np.pi)) ** 0.5 * 1.1
    d = rng.normal(size=(8 * n, 3))
    p = d / np.linalg.norm(d, axis=1, keepdims=True) * (r + rng.uniform(-0.5, 0.5, (8 * n, 1)))
    v = np.unique(np.floor(p).astype(np.int64), axis=0)
    assert len(v) >= n, len(v)
    v = v[rng.permutation(len(v))[:n]]
    vox = [torch.as_tensor(v, dtype=torch.int32, device=dev), torch.as_tensor(v + [1, 0, 0], dtype=torch.int32, device=dev)]
    idx = torch.arange(n, device=dev)
    return vox, torch.stack([idx, idx], 1)


def report(what, res):
    cols = []
    for narrow in sorted(res, reverse=True):
        m, lo, hi = res[narrow]
        cols.append(f"{'narrow' if narrow else 'generic'} {m:.3f} ms [{lo:.3f}, {hi:.3f}]")
    if len(res) == 2:
        cols.append(f"narrow / generic {res[1][0] / res[0][0]:.2f}")
    print(f"{what}: " + "   ".join(cols), flush=True)


variants = (1, 0) if args.narrow is None else (args.narrow,)
for size in args.sizes.split(","):
    vox, pairs = demo_pair() if size == "demo" else synthetic_pair()
    n0, n1 = len(vox[0]), len(vox[1])
    coords = torch.cat([torch.cat([torch.full((len(v), 1), b, dtype=torch.int32, device=dev), v], 1) for b, v in enumerate(vox)])
    M = coords.shape[0]
    feats = torch.ones(M, 1, device=dev)
    torch.manual_seed(0)
    model = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=K1, normalize_feature=True, D=3).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(1)

    plan = SP.SparsePlan(coords, 1, [(K1, 0, 0)])
    nnz = int(plan.kernel_map(0)[0][M])
    dy = torch.randn(M, 32, device=dev)
    wgrad = {1: lambda: SP.sparse_conv_narrow_wgrad(plan, 0, 0, feats, dy), 0: lambda: SP.sparse_conv_wgrad(plan, 0, 0, feats, dy)}
    diff = float((wgrad[1]() - wgrad[0]()).abs().max())

    def step():
        model.zero_grad(set_to_none=True)
        out = T.fcgf_train(model, coords, feats)
        sel0, sel1, pos_sel = fcgf.sample_hardest_contrastive(n0, n1, pairs.shape[0], generator=gen)
        pos, neg, _ = fcgf.hardest_contrastive_loss(out[:n0], out[n0:], pairs, sel0, sel1, pos_sel)
        (pos + neg).backward()

    res_w, res_s = {}, {}
    for rnd in range(2):                           # alternate; keep the second round (both warm)
        for narrow in variants:
            res_w[narrow] = timed(wgrad[narrow])
            model.narrow_conv1 = bool(narrow)
            res_s[narrow] = timed(step)
    print(f"{size}: {n0} + {n1} voxels, conv1 {K1}^3 with {nnz} pairs, {pairs.shape[0]} positive pairs; "
          f"max |dW narrow - dW generic| = {diff:.2e}", flush=True)
    report(f"{size}: conv1 weight gradient [{M}, 1] x [{M}, 32]", res_w)
    report(f"{size}: forward + loss + backward", res_s)
gmf_amd.check_status()
