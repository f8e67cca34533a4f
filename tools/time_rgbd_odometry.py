"""Times the RGB-D odometry (gmf_amd/rgbd.py): rgbd_pyramids, rgbd_odometry and rgbd_fragments.

  scene    synthetic: the inside of a 4 x 2.4 x 4.8 m room with a sphere in it, ray-cast analytically to 100 frames of 480 x 640 (uint16
           millimetres; the grey value is a smooth texture of the world point, uint8; fx = fy = 525, cx = 319.5, cy = 239.5) from
           a camera that turns 0.005 rad and moves 5 mm per frame
  calls    rgbd_pyramids of the 100 frames; rgbd_odometry of their 99 consecutive pairs (make_fragments.py's options: 0.07 m,
           0.3 .. 3.0 m, 20 / 10 / 5 iterations) on those pyramids; rgbd_fragments of 1 and of 8 fragments x 100 frames (the same
           frames under 8 fragment numbers), voxel_length 0.008, sdf_trunc 0.04, with and without the pose-graph optimisation
  figures  the pairs that succeed, the rotation and translation error of the chain's last pose against the camera's true pose,
           and for rgbd_odometry the time per pair and per iteration launch triple

Device events around each call after warm-up; median, min and max over repeats, in us.  There is no open3d to compare the times
with: they are recorded, not gated.
Usage: python tools/time_rgbd_odometry.py [--repeats 5] [--warmup 1] [--fragments 1,8] [--frames 100] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                                     # noqa: E402

H, W = 480, 640
K = (525.0, 525.0, 319.5, 239.5)
VOXEL, TRUNC, STRIDE = 0.008, 0.04, 4
ROOM = torch.tensor([2.0, 1.2, 2.4])               # half extents: every wall within max_depth of the camera
SPHERE_C, SPHERE_R = torch.tensor([0.3, 0.4, 1.0]), 0.5
OPTIONS = dict(max_depth_diff=0.07, min_depth=0.3, max_depth=3.0)


def pose(k):
    a = 0.005 * k
    P = np.eye(4)
    P[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    P[:3, 3] = [0.005 * k - 0.25, 0.0, -0.5]
    return P


def render(P, dev):
    """(grey uint8, depth uint16 millimetres) of the room seen from camera-to-world pose P."""
    fx, fy, cx, cy = K
    i, j = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    d = torch.stack([(j - cx) / fx, (i - cy) / fy, torch.ones_like(i)], -1) @ torch.from_numpy(P[:3, :3].T.copy()).to(dev)
    o = torch.from_numpy(P[:3, 3].copy()).to(dev)
    room = ROOM.to(dev, torch.float64)
    s = torch.where(d > 0, (room - o) / d, (-room - o) / d).amin(-1)            # the wall the ray leaves the room through
    oc = o - SPHERE_C.to(dev, torch.float64)
    a, b, c = (d * d).sum(-1), 2 * (d * oc).sum(-1), (oc * oc).sum() - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    t = (-b - disc.clamp_min(0).sqrt()) / (2 * a)
    s = torch.where((disc > 0) & (t > 0), torch.minimum(s, t), s)
    X = o + d * s[..., None]
    tex = 0.5 + 0.2 * torch.sin(7 * X[..., 0]) * torch.cos(5 * X[..., 1]) + 0.15 * torch.sin(9 * X[..., 1] + 3 * X[..., 2]) \
        + 0.1 * torch.cos(11 * X[..., 0] + 2 * X[..., 2])
    grey = (255 * tex.clamp(0, 1)).round().to(torch.uint8)
    depth = torch.from_numpy((s * 1000.0).round().clamp(0, 65535).cpu().numpy().astype(np.uint16)).to(dev)
    return grey, depth


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts, out


def pose_error(P, gt):
    d = np.linalg.inv(gt) @ P
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(d[:3, :3]) - 1) / 2)))), float(np.linalg.norm(d[:3, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fragments", default="1,8")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rgbd_odometry.py needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ts):
        return f"{statistics.median(ts):11.1f} us ({min(ts):.1f} .. {max(ts):.1f})"

    F1 = args.frames
    poses1 = np.stack([pose(k) for k in range(F1)])
    frames = [render(P, dev) for P in poses1]
    grey1, depth1 = torch.stack([f[0] for f in frames]), torch.stack([f[1] for f in frames])
    pyramid_args = dict(min_depth=OPTIONS["min_depth"], max_depth=OPTIONS["max_depth"])
    t_pyr, pyr = timed(lambda: gmf_amd.rgbd_pyramids(grey1, depth1, **pyramid_args), args.warmup, args.repeats)
    src = list(range(F1 - 1))
    tgt = [i + 1 for i in src]
    t_odo, (ok, X, info) = timed(lambda: gmf_amd.rgbd_odometry(pyr, pair_source=src, pair_target=tgt, intrinsic=K,
                                                               max_depth_diff=OPTIONS["max_depth_diff"]), args.warmup, args.repeats)
    chain = gmf_amd.odometry_poses(X).cpu().numpy()
    rot, tr = pose_error(chain[-1], np.linalg.inv(poses1[0]) @ poses1[-1])
    med = statistics.median(t_odo)
    say(f"{F1} frames of {H} x {W}, {F1 - 1} consecutive pairs: {int(ok.sum())} succeed; the last pose of the chain is off by "
        f"{rot:.3f} deg, {1000 * tr:.1f} mm after {F1 - 1} steps")
    say(f"  rgbd_pyramids   {fmt(t_pyr)}")
    say(f"  rgbd_odometry   {fmt(t_odo)} | {med / (F1 - 1):.1f} us per pair, {med / 37:.1f} us per scatter + walk + finish of all pairs "
        f"(35 iterations, the scales, the information matrix)")
    for l, its in ((0, (0, 0, 5)), (1, (0, 10, 0)), (2, (20, 0, 0))):      # each with the two level-0 triples of scales and information
        t, _ = timed(lambda: gmf_amd.rgbd_odometry(pyr, pair_source=src, pair_target=tgt, intrinsic=K, iterations=its,
                                                   max_depth_diff=OPTIONS["max_depth_diff"]), args.warmup, args.repeats)
        if l == 0:
            level0 = statistics.median(t) / (sum(its) + 2)
        per = level0 if l == 0 else (statistics.median(t) - 2 * level0) / sum(its)
        say(f"    level {l} ({H >> l} x {W >> l}) alone, {sum(its)} iterations: {fmt(t)} | {per:.1f} us per launch triple")
    for G in (int(x) for x in args.fragments.split(",")):
        grey = grey1.repeat(G, 1, 1)
        depth = depth1.view(torch.int16).repeat(G, 1, 1).view(torch.uint16)
        off = list(range(0, G * F1 + 1, F1))
        tsdf = dict(voxel_length=VOXEL, sdf_trunc=TRUNC, depth_sampling_stride=STRIDE)
        for optimize in (False, True):
            t, out = timed(lambda: gmf_amd.rgbd_fragments(grey, depth, K, frame_offsets=off, optimize=optimize, **OPTIONS, **tsdf),
                           args.warmup, args.repeats)
            say(f"  rgbd_fragments  {fmt(t)} | {G} fragment(s) x {F1} frames, optimize={optimize}: {out[0].shape[0]} vertices")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
