"""Times the fragment builder (gmf_amd/fragments.py: tsdf_fragments, and with --color tsdf_fragments_colored), stage by stage.

  scene    synthetic: the inside of a 6 x 3 x 7 m room with a sphere in it, ray-cast analytically to 50 frames of 480 x 640 uint16
           millimetres (fx = fy = 525, cx = 319.5, cy = 239.5) from a camera that turns 0.02 rad and moves 1 cm per frame
  shapes   one fragment per call, then 8 (the same frames under 8 fragment numbers), voxel_length 0.008, sdf_trunc 0.04, stride 4
  stages   gmf_tsdf_allocate, gmf_tsdf_integrate, gmf_tsdf_extract (the counting call and the emitting call), as
           tsdf_fragments issues them; and the whole tsdf_fragments call
  --color  also gmf_tsdf_integrate_color, the emitting gmf_tsdf_extract_color and the whole tsdf_fragments_colored call, each
           beside the colour-free time of the same run; the colour frames are a pattern of the pixel and the frame (the time does
           not depend on the values); the colour form moves 12 B per voxel and 3 + 4 B per pixel on top
  --mesh   also gmf_tsdf_extract_mesh (the counting and the emitting call: vertices, normals, triangles), each beside
           gmf_tsdf_extract's time of the same run, and estimate_normals_batched (radius three voxels, max_nn 30) on the same
           vertices: the normals the mesh normals replace
  figures  units, vertices, voxel updates (the sum of the weights) and unit-frame visits; for the integration call the updates per
           second, and bytes per second over what it must move: the volume written once (8 B per voxel) and every depth frame
           converted once (2 B read, 4 B written) - the gathered reads of depth it does on top are served by the caches

Device events around each call after warm-up; median, min and max over repeats, in us.  There is no open3d to compare the times
with: they are recorded, not gated.
Usage: python tools/time_tsdf.py [--repeats 5] [--warmup 1] [--fragments 1,8] [--frames 50] [--color] [--mesh] [--out FILE]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                                     # noqa: E402
from gmf_amd._util import handle_and_stream         # noqa: E402

H, W = 480, 640
K = (525.0, 525.0, 319.5, 239.5)
VOXEL, TRUNC, STRIDE = 0.008, 0.04, 4
ROOM = torch.tensor([3.0, 1.5, 3.5])               # half extents
SPHERE_C, SPHERE_R = torch.tensor([0.3, 0.4, 1.0]), 0.5


def pose(k):
    a = 0.02 * k
    P = np.eye(4)
    P[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    P[:3, 3] = [0.01 * k - 0.25, 0.0, -0.5]
    return P


def raycast(P, dev):
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
    return torch.from_numpy((s * 1000.0).round().clamp(0, 65535).cpu().numpy().astype(np.uint16)).to(dev)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fragments", default="1,8")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--max-units", type=int, default=1 << 18)
    ap.add_argument("--color", action="store_true")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--normal-radius", type=float, default=0.024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tsdf.py needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ts):
        return f"{statistics.median(ts):11.1f} us ({min(ts):.1f} .. {max(ts):.1f})"

    F1 = args.frames
    poses1 = np.stack([pose(k) for k in range(F1)])
    depth1 = torch.stack([raycast(P, dev) for P in poses1])
    if args.color:
        i, j, k = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), torch.arange(F1, device=dev), indexing="ij")
        color1 = torch.stack([(3 * j + k) % 256, (5 * i + 2 * k) % 256, (i + j + 7 * k) % 256], -1).permute(2, 0, 1, 3).to(torch.uint8)
    for G in (int(x) for x in args.fragments.split(",")):
        depth = depth1.view(torch.int16).repeat(G, 1, 1).view(torch.uint16)
        poses = np.tile(poses1, (G, 1, 1))
        off_h = list(range(0, G * F1 + 1, F1))
        F = G * F1
        both = torch.from_numpy(np.stack([poses, np.linalg.inv(poses)])).to(dev)
        off = torch.tensor(off_h, dtype=torch.int32, device=dev)
        h, st = handle_and_stream(depth)
        camera = (G, F, H, W) + K + (VOXEL, TRUNC, 1000.0, 4.5)
        cap = args.max_units
        keys = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        birth = torch.empty(cap, dtype=torch.int32, device=dev)
        uoff = torch.empty(G + 1, dtype=torch.int32, device=dev)
        poff = torch.empty(G + 1, dtype=torch.int32, device=dev)
        n = C.c_longlong(0)

        def allocate():
            h.call("gmf_tsdf_allocate", depth.data_ptr(), 1, both[0].data_ptr(), off.data_ptr(), *camera, STRIDE, cap, keys.data_ptr(),
                   birth.data_ptr(), uoff.data_ptr(), C.byref(n), st)
            return int(n.value)

        t_alloc, U = timed(allocate, args.warmup, args.repeats)
        tsdf = torch.empty((U, 16, 16, 16), device=dev)
        weight = torch.empty((U, 16, 16, 16), device=dev)

        def integrate():
            h.call("gmf_tsdf_integrate", depth.data_ptr(), 1, both[1].data_ptr(), off.data_ptr(), *camera, keys.data_ptr(), uoff.data_ptr(),
                   birth.data_ptr(), U, tsdf.data_ptr(), weight.data_ptr(), st)

        t_int, _ = timed(integrate, args.warmup, args.repeats)
        volume = (keys.data_ptr(), uoff.data_ptr(), G, U, tsdf.data_ptr(), weight.data_ptr(), VOXEL)

        def count():
            h.call("gmf_tsdf_extract", *volume, None, 0, poff.data_ptr(), C.byref(n), st)
            return int(n.value)

        t_count, M = timed(count, args.warmup, args.repeats)
        pts = torch.empty((M, 3), device=dev)
        t_emit, _ = timed(lambda: h.call("gmf_tsdf_extract", *volume, pts.data_ptr(), M, poff.data_ptr(), None, st), args.warmup,
                          args.repeats)
        t_all, out = timed(lambda: gmf_amd.tsdf_fragments(depth, torch.from_numpy(poses), K, frame_offsets=off_h, voxel_length=VOXEL,
                                                          sdf_trunc=TRUNC, depth_sampling_stride=STRIDE, max_units=cap),
                           args.warmup, args.repeats)
        assert out[0].shape[0] == M and torch.equal(out[0], pts)
        updates = int(weight.sum(dtype=torch.float64))
        visits = int((F1 - birth[:U]).sum()) * 4096             # every fragment has F1 frames; a unit takes those from its birth on
        moved = U * 4096 * 8 + F * H * W * 6
        t = statistics.median(t_int) * 1e-6
        say(f"{G} fragment(s) x {F1} frames of {H} x {W}: {U} units, {M} vertices, {updates} voxel updates of {visits} voxel-frame visits")
        say(f"  allocate        {fmt(t_alloc)}")
        say(f"  integrate       {fmt(t_int)} | {updates / t / 1e9:.2f} G updates/s, {visits / t / 1e9:.2f} G visits/s, "
            f"{moved / t / 1e9:.1f} GB/s over {moved / 1e6:.1f} MB")
        say(f"  extract (count) {fmt(t_count)}")
        say(f"  extract (emit)  {fmt(t_emit)}")
        say(f"  tsdf_fragments  {fmt(t_all)}")
        if args.color:
            color = color1.repeat(G, 1, 1, 1).contiguous()
            cvol = torch.empty((U, 16, 16, 16, 3), device=dev)
            tsdf_c, weight_c = torch.empty_like(tsdf), torch.empty_like(weight)

            def integrate_color():
                h.call("gmf_tsdf_integrate_color", depth.data_ptr(), 1, color.data_ptr(), both[1].data_ptr(), off.data_ptr(), *camera,
                       keys.data_ptr(), uoff.data_ptr(), birth.data_ptr(), U, tsdf_c.data_ptr(), weight_c.data_ptr(), cvol.data_ptr(), st)

            t_int_c, _ = timed(integrate_color, args.warmup, args.repeats)
            assert torch.equal(tsdf_c, tsdf) and torch.equal(weight_c, weight)
            pts_c, cols = torch.empty_like(pts), torch.empty_like(pts)
            t_emit_c, _ = timed(lambda: h.call("gmf_tsdf_extract_color", keys.data_ptr(), uoff.data_ptr(), G, U, tsdf.data_ptr(),
                                               weight.data_ptr(), cvol.data_ptr(), VOXEL, pts_c.data_ptr(), cols.data_ptr(), M,
                                               poff.data_ptr(), None, st), args.warmup, args.repeats)
            assert torch.equal(pts_c, pts)
            t_all_c, out_c = timed(lambda: gmf_amd.tsdf_fragments_colored(color, depth, torch.from_numpy(poses), K, frame_offsets=off_h,
                                                                          voxel_length=VOXEL, sdf_trunc=TRUNC,
                                                                          depth_sampling_stride=STRIDE, max_units=cap),
                                   args.warmup, args.repeats)
            assert torch.equal(out_c[0], pts) and torch.equal(out_c[2], cols)
            moved_c = moved + U * 4096 * 12 + F * H * W * 7
            tc = statistics.median(t_int_c) * 1e-6
            say(f"  integrate_color        {fmt(t_int_c)} against {fmt(t_int)} | {updates / tc / 1e9:.2f} G updates/s, "
                f"{moved_c / tc / 1e9:.1f} GB/s over {moved_c / 1e6:.1f} MB")
            say(f"  extract_color (emit)   {fmt(t_emit_c)} against {fmt(t_emit)}")
            say(f"  tsdf_fragments_colored {fmt(t_all_c)} against {fmt(t_all)}")
        if args.mesh:
            toff = torch.empty(G + 1, dtype=torch.int32, device=dev)
            m = C.c_longlong(0)
            mesh_volume = volume[:6] + (None, VOXEL)

            def mesh_count():
                h.call("gmf_tsdf_extract_mesh", *mesh_volume, None, None, None, 0, None, 0, poff.data_ptr(), toff.data_ptr(), C.byref(n),
                       C.byref(m), st)
                return int(n.value), int(m.value)

            t_mcount, (Mm, Km) = timed(mesh_count, args.warmup, args.repeats)
            assert Mm == M
            pts_m, nrm = torch.empty_like(pts), torch.empty_like(pts)
            tri = torch.empty((Km, 3), dtype=torch.int32, device=dev)
            t_memit, _ = timed(lambda: h.call("gmf_tsdf_extract_mesh", *mesh_volume, pts_m.data_ptr(), nrm.data_ptr(), None, M,
                                              tri.data_ptr(), Km, poff.data_ptr(), toff.data_ptr(), None, None, st), args.warmup, args.repeats)
            assert torch.equal(pts_m, pts)
            t_knn, _ = timed(lambda: gmf_amd.estimate_normals_batched(pts, poff, args.normal_radius, 30), args.warmup, args.repeats)
            say(f"  mesh: {Km} triangles")
            say(f"  extract_mesh (count)     {fmt(t_mcount)} against {fmt(t_count)}")
            say(f"  extract_mesh (emit)      {fmt(t_memit)} against {fmt(t_emit)}")
            say(f"  estimate_normals_batched {fmt(t_knn)} (radius {args.normal_radius}, max_nn 30, the same {M} vertices)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
