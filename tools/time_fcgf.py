"""Times FCGF (gmf_amd.fcgf.ResUNetBN2C: Cin 1, Cout 32, conv1 7^3, normalised) and DGR's register() on the 3DMatch demo
fragments (tests/golden/fpfh_demo_clouds.npz), with device events after warm-up (median, min, max over repeats, in us):

- the FCGF pair forward (both clouds in one plan) at 5 cm and 2.5 cm;
- conv1 on the narrow-input kernel against the generic sparse_conv, alternated in one run, on the same plan and weights;
- the fused head against its two-launch form (two identity-map sparse_conv calls) plus torch's norm and divide;
- each stage of register() at 5 cm (random weights; the inlier net's images as 1 200 tokens each).

Usage: python tools/time_fcgf.py [--repeats 20] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import dgr, fcgf        # noqa: E402
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
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def alternated(fa, fb, repeats, warmup=3):
    """A and B in turn, each timed on its own: (median A, median B)."""
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(repeats):
        for f, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def clouds():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    return z["cloud0"].astype(np.float32), z["cloud1"].astype(np.float32)


def pair_coords(v):
    out = []
    for b, c in enumerate(clouds()):
        x = torch.as_tensor(c, device=DEV)
        x = x[gmf_amd.voxel_select(x, v)]
        c = torch.floor(x.double() / v).int()
        out.append(torch.cat([torch.full((len(c), 1), b, dtype=torch.int32, device=DEV), c], 1))
    return torch.cat(out).contiguous(), [len(o) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    report = lambda s: (print(s, flush=True), lines.append(s))    # noqa: E731
    torch.manual_seed(0)
    model = fcgf.ResUNetBN2C(1, 32, bn_momentum=0.05, conv1_kernel_size=7, normalize_feature=True, D=3).to(DEV).eval()
    for v in (0.05, 0.025):
        coords, sizes = pair_coords(v)
        feats = torch.ones((len(coords), 1), device=DEV)
        med, lo, hi = timed(lambda: model(coords, feats), args.repeats)
        report(f"FCGF pair forward at {v * 100:g} cm ({sizes[0]} + {sizes[1]} voxels): {med:.0f} us (min {lo:.0f}, max {hi:.0f})")
        model.narrow_conv1 = False
        med, lo, hi = timed(lambda: model(coords, feats), args.repeats)
        model.narrow_conv1 = True
        report(f"  the same with conv1 on the generic kernel: {med:.0f} us (min {lo:.0f}, max {hi:.0f})")

    coords, sizes = pair_coords(0.05)
    M = len(coords)
    feats = torch.ones((M, 1), device=DEV)
    L = model._weights(DEV)
    maps = list(SP._NET_MAPS) + [(7, 0, 0)]
    plan = SP.SparsePlan(coords, 4, maps)
    host = plan.to_host()
    W, sc, sh = L[0]
    nsplit = SP.layer_nsplit(*W.shape)
    narrow = lambda: SP.sparse_conv_narrow(plan, len(maps) - 1, 0, feats, W, scale=sc, shift=sh)     # noqa: E731
    generic = lambda: SP.sparse_conv(plan, len(maps) - 1, 0, feats, W, scale=sc, shift=sh, nsplit=nsplit)   # noqa: E731
    d = (narrow() - generic()).abs().max().item()
    ta, tb = alternated(narrow, generic, args.repeats)
    pairs = int(host["maps"][-1][0][-1])
    report(f"conv1 (7^3, 1 -> 32, {M} rows, {pairs} pairs, {pairs / M:.0f} per row), alternated: narrow {ta:.1f} us, generic "
           f"(nsplit {nsplit} + split reduce) {tb:.1f} us; max |narrow - generic| = {d:.2e}")

    g = torch.Generator().manual_seed(1)
    t1, s1 = torch.randn(M, 64, generator=g).relu().to(DEV), torch.randn(M, 32, generator=g).relu().to(DEV)
    W1, W2, b = L[21][0], L[22][0], L[22][2]
    fused = lambda: SP.sparse_head_l2(plan, 0, t1, W1, W2, xb=s1, bias=b, normalize=True)     # noqa: E731

    def two_launch():
        o = SP.sparse_conv(plan, None, 0, t1, W1, xb=s1, relu=True)
        y = SP.sparse_conv(plan, None, 0, o, W2, shift=b)
        return y / (torch.norm(y, p=2, dim=1, keepdim=True) + 1e-8)
    d = (fused() - two_launch()).abs().max().item()
    ta, tb = alternated(fused, two_launch, args.repeats)
    report(f"head ({M} rows, 96 -> 64 -> 32, normalised), alternated: fused {ta:.1f} us, two sparse_conv + torch norm / divide "
           f"{tb:.1f} us; max difference {d:.2e}")

    # register() stage by stage at 5 cm
    nc = types.SimpleNamespace(feat_model="ResUNetBN2C", feat_model_n_out=32, bn_momentum=0.05, feat_conv1_kernel_size=7,
                               normalize_feature=True, inlier_model="ResUNetBN2C", inlier_conv1_kernel_size=3,
                               inlier_feature_type="ones", voxel_size=0.05, nn_max_n=500)
    torch.manual_seed(2)
    inl = gmf_amd.ResUNetBN2C(1, 1, D=6, pe=True)
    state = {"config": nc, "state_dict": model.state_dict(), "state_dict_inlier": inl.state_dict()}
    R = dgr.DeepGlobalRegistration({"clip_weight_thresh": 0.05}, device=DEV, state=state)
    pt = torch.randn(1, 1200, 128, generator=g).to(DEV)
    qt = torch.randn(1, 1200, 128, generator=g).to(DEV)
    c0, c1 = clouds()
    x0, x1 = torch.as_tensor(c0, device=DEV), torch.as_tensor(c1, device=DEV)
    p0, k0 = R.preprocess(x0)
    p1, k1 = R.preprocess(x1)
    F0, F1 = R.features(k0, k1)
    i0, i1 = R.correspondences(F0, F1)
    z = lambda c: torch.cat([torch.zeros((len(c), 1), dtype=torch.int32, device=DEV), c], 1)    # noqa: E731
    ic = gmf_amd.inlier_coordinates(z(k0), z(k1), i0, i1)
    ones = torch.ones((len(ic), 1), device=DEV)
    w = R.inlier_model(ic, ones, p_tokens=pt, q_tokens=qt).sigmoid()
    stages = [("preprocess (voxel_select + coords, both clouds)", lambda: (R.preprocess(x0), R.preprocess(x1))),
              ("FCGF pair forward", lambda: R.features(k0, k1)),
              ("find_knn_gpu", lambda: R.correspondences(F0, F1)),
              ("inlier network (+ sigmoid)", lambda: R.inlier_model(ic, ones, p_tokens=pt, q_tokens=qt).sigmoid()),
              ("GlobalRegistration", lambda: gmf_amd.GlobalRegistration(p0[i0], p1[i1], weights=w, break_threshold_ratio=1e-4,
                                                                        quantization_size=0.1)),
              ("safeguard RANSAC (80 000 hypotheses)", lambda: R.safeguard_registration(p0, p1, i0, i1)),
              ("ICP", lambda: gmf_amd.registration_icp(p0, p1, 0.1, init=torch.eye(4, device=DEV)))]
    report(f"register() stages at 5 cm ({len(p0)} + {len(p1)} voxels, {len(ic)} correspondences):")
    for name, fn in stages:
        med, lo, hi = timed(fn, max(3, args.repeats // 4), warmup=1)
        report(f"  {name:48s} {med:9.0f} us (min {lo:.0f}, max {hi:.0f})")
    t = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R.register(c0, c1, p_tokens=pt, q_tokens=qt)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    report(f"  whole register() (host clock, 5 runs): {statistics.median(t):.0f} us; branch {R.last_stats['branch']}, "
           f"wsum {R.last_stats['wsum']:.1f} / threshold {R.last_stats['wsum_threshold']:.1f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
