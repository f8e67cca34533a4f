"""Times the descriptor stages (gmf_amd/features.py) at the sizes of the reference's FPFH recipes:

  one cloud    a 3DMatch demo fragment (tests/golden/fpfh_demo_clouds.npz, 2 cm-thinned, ~30 k points) at v = 5 cm and 2.5 cm:
               voxel_down_sample, voxel_select, the radius search (5v, 100), normals (2v, 30), FPFH (5v, 100) on the
               voxelised cloud, and the whole fpfh_descriptors recipe from the raw points
  batch of 32  32 ragged clouds (rigidly moved, randomly cropped copies of both fragments) through the same stages

Device events around each call, after warm-up; median and spread over repeats.  The voxel stages include their one count
read-back.  Usage: python tools/time_features.py [--repeats 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import synthetic        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def stages(P, off, v, repeats, report, label):
    xyz, offd = gmf_amd.voxel_down_sample_batched(P, off, v)
    n = gmf_amd.estimate_normals_batched(xyz, offd, 2 * v, 30)
    M = xyz.shape[0]
    rows = [
        ("voxel_down_sample", lambda: gmf_amd.voxel_down_sample_batched(P, off, v)),
        ("voxel_select", lambda: gmf_amd.voxel_select_batched(P, off, v)),
        ("radius_knn (5v, 100)", lambda: gmf_amd.radius_knn_batched(xyz, offd, 5 * v, 100)),
        ("normals (2v, 30)", lambda: gmf_amd.estimate_normals_batched(xyz, offd, 2 * v, 30)),
        ("fpfh (5v, 100)", lambda: gmf_amd.compute_fpfh_batched(xyz, n, offd, 5 * v, 100)),
        ("fpfh_descriptors (mean)", lambda: gmf_amd.fpfh_descriptors(P, v, offsets=off)),
        ("fpfh_descriptors (select)", lambda: gmf_amd.fpfh_descriptors(P, v, offsets=off, voxelize="select")),
    ]
    report(f"{label}, v = {100 * v:g} cm: {P.shape[0]} raw points -> {M} voxels")
    for name, fn in rows:
        med, lo, hi = timed(fn, repeats)
        report(f"  {name:<27s} {med:9.1f} us [{lo:.1f}, {hi:.1f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_features.py measures on a HIP device"
    dev = "cuda:0"
    lines = []

    def report(s):
        print(s, flush=True)
        lines.append(s)

    report(f"device: {torch.cuda.get_device_name(0)}; median [min, max] over {a.repeats} repeats, device events")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    c0 = torch.as_tensor(z["cloud0"]).to(dev)
    for v in (0.05, 0.025):
        stages(c0, None, v, a.repeats, report, "one cloud")
    r = np.random.default_rng(0)
    clouds = []
    for b in range(32):
        c = z[f"cloud{b % 2}"].astype(np.float64)
        keep = r.random(len(c)) < r.uniform(0.5, 1.0)
        R = synthetic.random_rotation(r)
        clouds.append((c[keep] @ R.T + r.uniform(-1, 1, 3)).astype(np.float32))
    P = torch.as_tensor(np.concatenate(clouds)).to(dev)
    off = np.r_[0, np.cumsum([len(c) for c in clouds])].tolist()
    for v in (0.05, 0.025):
        stages(P, off, v, max(3, a.repeats // 2), report, "batch of 32")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
