"""Writes tests/golden/fpfh_demo_clouds.npz: the reference's 3DMatch demo fragments (GMF_PointDSC/demo_data/cloud_bin_{0,1}.ply,
redkitchen, 258 k / 269 k points) thinned on the host by a voxel mean (open3d's voxel_down_sample formula, in float64) so the
fixture stays small.  Arrays cloud0 / cloud1 [N,3] float32 and `thin` (the voxel edge used).  Run on a machine that has the
reference checkout; the tests read only the npz.

Usage: python tests/tools/make_fpfh_demo_clouds.py REFERENCE_ROOT [--thin 0.02]"""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_ply_xyz(path):
    with open(path, "rb") as f:
        n, props = None, []
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("format"):
                assert line.split()[1] == "binary_little_endian", line
            elif line.startswith("element vertex"):
                n = int(line.split()[2])
            elif line.startswith("property") and n is not None:
                props.append(line.split())
            elif line == "end_header":
                break
        assert [p[1:] for p in props[:3]] == [["float", "x"], ["float", "y"], ["float", "z"]], props
        assert all(p[1] == "float" for p in props), props
        data = np.frombuffer(f.read(n * 4 * len(props)), dtype="<f4").reshape(n, len(props))
    return data[:, :3].astype(np.float32)


def voxel_mean(p, v):
    p64 = p.astype(np.float64)
    lo = p64.min(0) - v / 2
    key = np.floor((p64 - lo) / v).astype(np.int64)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    s = np.zeros((len(first), 3))
    np.add.at(s, inv, p64)
    m = (s / np.bincount(inv)[:, None]).astype(np.float32)
    return m[np.argsort(first, kind="stable")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--thin", type=float, default=0.02)
    a = ap.parse_args()
    out = {"thin": np.float64(a.thin)}
    for k in (0, 1):
        raw = read_ply_xyz(os.path.join(a.reference, "GMF_PointDSC", "demo_data", f"cloud_bin_{k}.ply"))
        out[f"cloud{k}"] = voxel_mean(raw, a.thin)
        print(f"cloud_bin_{k}: {len(raw)} -> {len(out[f'cloud{k}'])} points")
    path = os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
