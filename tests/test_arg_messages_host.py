"""Characterisation of the argument checks of the Python wrappers (gmf_amd/_args.py and the modules that use it): every check a
wrapper can raise without a device, by exception type and full message, against tests/golden/arg_messages.txt.

The table below holds one bad call per case, on small CPU tensors (B = 2, N = 16): every row of the `bad` tables of the
tests/test_*_host.py files, and two-fault cases that pin the order of the checks (the fault reported is the one that was reported
before the checks moved into one module).  The golden file has one line per case: id, exception type, message, separated by tabs.
`python tests/test_arg_messages_host.py FILE` writes such a file from the tree it runs in; the committed one was written that way
from the commit before gmf_amd/_args.py existed, and only the lines whose wording was unified on purpose were replaced:

  the offset lists (ransac-16..19, 21, icp-09, 11, 24, fm-29..31, sm-12..16, pmc-12..16, features-04, 05, 19, 37, multiway-00,
  08..10, 16, 35, 39, dgr-00..03, 14), which said "offsets must be increasing, start at 0 and end at N", "target_offsets must
  not decrease, start at 0 and end at the number of target rows", "offsets must not decrease, start at 0 and end at sum N",
  "cloud_offsets must increase strictly from 0 to the number of rows (no empty cloud)" or "`off0` must ascend from 0 to the row
  count 10 (got [...])", say "<name> must increase strictly | ascend from 0 to the row count <n> (B + 1 integers)";
  the device requirement (pyr-25..28, odo-28, 29, frag-17..19, 27..30, dgr-10..12, 19, 33), which said "`color` and `depth` must
  live on a HIP device (got cpu, cpu); ...", "xyz0 and xyz1 must live on one HIP device; there is no CPU fallback",
  "pred_pairs | feat_model must live on a HIP device; there is no CPU fallback", says "`<name>` must live on a HIP device (got
  <device>); the HIP path is mandatory, there is no CPU fallback" for the first tensor that does not (frag-30, a `color` that
  is no tensor beside zero frames, says so as it does beside any other number of frames)."""
import os
import sys
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arg_messages.txt")


def _cases():
    import gmf_amd as G
    out = []

    def add(cid, fn):
        out.append((cid, fn))

    def table(prefix, fn, base, rows, order):
        """One case per row: `base` updated by the row's dict, handed to fn in `order` (positional), the rest as keywords."""
        for i, kw in enumerate(rows):
            def call(kw=kw):
                args = dict(base)
                args.update(kw)
                pos = [args.pop(k) for k in order]
                return fn(*pos, **args)
            add(f"{prefix}-{i:02d}", call)

    p = torch.zeros(2, 16, 3)
    p[0, :, 0] = torch.arange(16.0)
    rp = p.reshape(-1, 3)
    eye2 = torch.eye(4).repeat(2, 1, 1)

    # ---- solvers.py -------------------------------------------------------------------------------------------------------------
    table("ransac", lambda src, tgt, tau, **k: G.ransac_correspondence_batched(src, tgt, tau, **k), dict(src=p, tgt=p, tau=0.1), [
        dict(src=p, tgt=p[:, :8]), dict(src=p.double(), tgt=p.double()), dict(src=p[..., :2], tgt=p[..., :2]),
        dict(src=rp, tgt=rp), dict(src=torch.zeros(0, 5, 3), tgt=torch.zeros(0, 5, 3)), dict(src=p.numpy()),
        dict(ransac_n=2), dict(ransac_n=9), dict(ransac_n=3.5), dict(num_hypotheses=0), dict(num_hypotheses=2 ** 24 + 1),
        dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(mask=torch.ones(2, 16)),
        dict(mask=torch.ones(2, 15, dtype=torch.bool)), dict(src=rp, tgt=rp, offsets=[0, 16]),
        dict(src=rp, tgt=rp, offsets=[0, 20, 30]), dict(src=rp, tgt=rp, offsets=[0, 16, 16, 32]),
        dict(src=rp, tgt=rp, offsets=[1, 16, 32]), dict(src=rp, tgt=rp, offsets=[0, "a", 32]),
        dict(src=rp, tgt=rp, offsets=np.array([0, 20, 32])[::-1].copy()), dict(first_pair=-1),
        dict(), dict(src=rp, tgt=rp, offsets=[0, 16, 32]), dict(src=rp, tgt=rp, offsets=torch.tensor([0, 16, 32])),
        # two faults: the tensor before the scalar, the scalars in their order, the offsets last of the host checks, all before the device
        dict(src=rp.double(), tgt=rp.double(), offsets=[0, 16]), dict(ransac_n=2, tau=0.0), dict(num_hypotheses=0, first_pair=-1),
        dict(src=rp, tgt=rp, offsets=[0, 16], first_pair=-1), dict(tau=0.0), dict(mask=torch.ones(2, 16), ransac_n=2),
    ], ("src", "tgt", "tau"))

    s, t = p, torch.zeros(2, 20, 3)
    rs, rt = s.reshape(-1, 3), t.reshape(-1, 3)
    table("icp", lambda a, b, c, tau, **k: G.icp_point_to_point_batched(a, b, c, tau, **k), dict(source=s, target=t, init=eye2, tau=0.1), [
        dict(target=torch.zeros(3, 20, 3)), dict(source=s.double()), dict(init=torch.eye(4)), dict(init=eye2.double()),
        dict(tau=0.0), dict(max_iteration=-1), dict(max_iteration=2.5), dict(relative_fitness=-1.0), dict(source_offsets=[0, 16, 32]),
        dict(source=rs, target=rt, source_offsets=[0, 16, 32], target_offsets=[0, 20, 41]),
        dict(source=rs, target=rt, source_offsets=[0, 16, 32], target_offsets=[0, 10, 20, 40]),
        dict(source=rs, target=rt, source_offsets=[0, 16, 32], target_offsets=[0, 20, 20, 40]),
        dict(search="kd"), dict(search=""), dict(search="GRID"), dict(search=1), dict(search=None), dict(search=b"grid"),
        dict(), dict(search="grid"), dict(source=rs, target=rt, source_offsets=[0, 16, 32], target_offsets=[0, 20, 40]),
        dict(search="kd", source=s.double()), dict(source=s.double(), tau=0.0), dict(tau=0.0, max_iteration=-1),
        dict(source=rs, target=rt, source_offsets=[0, 16, 33], target_offsets=[0, 20, 41]), dict(max_iteration=-1, search="grid"),
        dict(init=torch.eye(4).repeat(3, 1, 1)),
    ], ("source", "target", "init", "tau"))

    nn = torch.zeros(2, 16, dtype=torch.int64)
    rn = nn.reshape(-1)
    table("fm", lambda a, b, c, tau, **k: G.ransac_feature_matching_batched(a, b, c, tau, **k), dict(source=s, target=t, nn=nn, tau=0.1), [
        dict(target=torch.zeros(3, 20, 3)), dict(source=s.double()), dict(target=t.double()), dict(source=s[..., :2]),
        dict(source=rs, nn=rn), dict(source=torch.zeros(2, 0, 3), nn=torch.zeros(2, 0, dtype=torch.int64)),
        dict(nn=nn.float()), dict(nn=nn[:, :8]), dict(nn=nn.numpy()), dict(ransac_n=2), dict(ransac_n=9), dict(ransac_n=3.5),
        dict(max_iteration=0), dict(max_iteration=2 ** 24 + 1), dict(max_iteration=10.5), dict(max_validation=0),
        dict(max_validation=65537), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(checker_distance=-0.1),
        dict(checker_distance=float("inf")), dict(edge_length_threshold=0.0), dict(edge_length_threshold=1.5),
        dict(edge_length_threshold=float("nan")), dict(first_pair=-1), dict(search="kdtree"), dict(search=1),
        dict(source_offsets=[0, 16, 32]),
        dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 16, 32], target_offsets=[0, 10, 20, 40]),
        dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, 20, 41]),
        dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, 30, 20, 40]),
        dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, "a", 40]),
        dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, 10, 20, 40]),
        dict(), dict(search="brute"), dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, 40, 40]),
        dict(ransac_n=2, max_iteration=0), dict(max_validation=0, tau=0.0), dict(tau=0.0, checker_distance=-0.1),
        dict(checker_distance=-0.1, edge_length_threshold=0.0), dict(first_pair=-1, source=rs, target=rt, nn=rn,
                                                                   source_offsets=[0, 16], target_offsets=[0, 40]),
        dict(nn=nn.float(), ransac_n=2),
    ], ("source", "target", "nn", "tau"))

    W = G.registration_ransac_based_on_feature_matching
    add("fmwrap-00", lambda: W(s[0], t[0], torch.zeros(33, 16), torch.zeros(33, 20), 0.1))
    add("fmwrap-01", lambda: W(s[0].numpy(), t[0].numpy(), np.zeros((33, 16), np.float32), np.zeros((33, 20), np.float32), 0.1))
    add("fmwrap-02", lambda: W(s[0], t[0], torch.zeros(16, 33), torch.zeros(20, 32), 0.1))
    add("fmwrap-03", lambda: W(s[0], t[0], torch.zeros(16, 8), torch.zeros(20, 8), 0.1))
    add("fmwrap-04", lambda: W(s[0].numpy(), t[0].numpy(), torch.zeros(16, 8), np.zeros((20, 8), np.float32), 0.1))
    add("corrwrap-00", lambda: G.registration_ransac_based_on_correspondence(s[0], s[0], torch.arange(16).repeat(2, 1).t(), 0.1))
    add("icpwrap-00", lambda: G.registration_icp(s[0], s[1], 0.1))
    add("icpwrap-01", lambda: G.registration_icp(s[0], s[1], 0.1, search="grid"))
    add("icpwrap-02", lambda: G.registration_icp(s[0], s[1], 0.1, search="kd"))
    add("icpwrap-03", lambda: G.registration_icp(s[0], s[1], 0.1, search=None))
    add("icprefine-00", lambda: G.icp_refine(s, s, eye2))

    # ---- spectral.py, clique.py -------------------------------------------------------------------------------------------------
    c = torch.zeros(2, 16, 6)
    rc = c.reshape(-1, 6)
    ragged = dict(corr=rc, src=rp, tgt=rp)
    shared = [
        dict(corr=c.double()), dict(src=p.double()), dict(tgt=p.half()), dict(corr=c.numpy()), dict(corr=c[..., :5]),
        dict(src=p[..., :2]), dict(tgt=torch.zeros(2, 16, 6)), dict(corr=rc), dict(offsets=[0, 16, 32]), dict(src=p[:, :8]),
        dict(tgt=p[:1]), dict(corr=torch.zeros(0, 4, 6), src=torch.zeros(0, 4, 3), tgt=torch.zeros(0, 4, 3)),
        dict(ragged, offsets=[0, 16]), dict(ragged, offsets=[1, 16, 32]), dict(ragged, offsets=[0, 20, 16, 32]),
        dict(ragged, offsets=[0, 16, 33]), dict(ragged, offsets=[32]), dict(ragged, offsets=[0, "a", 32]),
        dict(thr=0.0), dict(thr=-0.1), dict(thr=float("nan")), dict(thr=float("inf")),
        dict(), dict(ragged, offsets=[0, 8, 8, 32]), dict(corr=torch.zeros(2, 0, 6), src=torch.zeros(2, 0, 3), tgt=torch.zeros(2, 0, 3)),
        # two faults
        dict(ragged, corr=rc.double(), offsets=[0, 16]), dict(ragged, thr=0.0, offsets=[0, 16]), dict(src=p[:, :8], thr=0.0),
    ]
    sm_own = [dict(top_ratio=-0.01), dict(top_ratio=1.01), dict(top_ratio=float("nan")), dict(num_iterations=0),
              dict(num_iterations=1001), dict(num_iterations=2.5), dict(_col_splits=0), dict(_col_splits=33), dict(_col_splits=1.5),
              dict(thr=0.0, top_ratio=2.0), dict(top_ratio=2.0, num_iterations=0), dict(num_iterations=0, _col_splits=0),
              dict(ragged, _col_splits=0, offsets=[0, 16])]
    pmc_own = [dict(metric="l2"), dict(metric=0), dict(max_steps=0), dict(max_steps=2.5), dict(max_steps=-3),
               dict(thr=0.0, metric="l2"), dict(metric="l2", max_steps=0), dict(ragged, max_steps=0, offsets=[0, 16])]
    order = ("corr", "src", "tgt", "thr")
    table("sm", lambda a, b, d, thr, **k: G.spectral_matching_batched(a, b, d, thr, **k), dict(corr=c, src=p, tgt=p, thr=0.1),
          shared + sm_own, order)
    table("pmc", lambda a, b, d, thr, **k: G.max_clique_batched(a, b, d, thr, **k), dict(corr=c, src=p, tgt=p, thr=0.1),
          shared + pmc_own, order)
    ns = types.SimpleNamespace(inlier_threshold=0.1)
    for name, F in (("SM", G.SM), ("PMC", G.PMC)):
        add(f"{name}-00", lambda F=F: F(c, p, p, ns))
        add(f"{name}-01", lambda F=F: F(rc, rp, rp, ns))
        add(f"{name}-02", lambda F=F: F(c[:1], p[:1], p[:1], ns))
        add(f"{name}-03", lambda F=F: F(c.numpy(), p, p, ns))
    table("graph", lambda corr, thr, **k: G.compatibility_graph(corr, thr, **k), dict(corr=rc, thr=0.1), [
        dict(corr=rc.double()), dict(corr=c), dict(thr=0.0), dict(metric="l1"), dict(), dict(corr=c, thr=0.0), dict(thr=0.0, metric="l1"),
    ], ("corr", "thr"))

    # ---- features.py ------------------------------------------------------------------------------------------------------------
    q = torch.zeros(64, 3)
    n = torch.zeros(64, 3)
    for i, f in enumerate([
        lambda: G.radius_knn_batched(q.double(), None, 0.1, 30), lambda: G.radius_knn_batched(q[:, :2], None, 0.1, 30),
        lambda: G.radius_knn_batched(torch.zeros(0, 3), None, 0.1, 30), lambda: G.radius_knn_batched(q.numpy(), None, 0.1, 30),
        lambda: G.radius_knn_batched(q, [0, 32], 0.1, 30), lambda: G.radius_knn_batched(q, [0, 40, 40, 64], 0.1, 30),
        lambda: G.radius_knn_batched(q, None, 0.0, 30), lambda: G.radius_knn_batched(q, None, float("inf"), 30),
        lambda: G.radius_knn_batched(q, None, "x", 30), lambda: G.radius_knn_batched(q, None, 0.1, 0),
        lambda: G.radius_knn_batched(q, None, 0.1, 257), lambda: G.radius_knn_batched(q, None, 0.1, 2.5),
        lambda: G.radius_knn_batched(q, None, 0.1, "x"), lambda: G.estimate_normals_batched(q, None, -1.0),
        lambda: G.estimate_normals(q, 0.1, max_nn=300), lambda: G.compute_fpfh_batched(q, n[:10], None, 0.25),
        lambda: G.compute_fpfh_batched(q, n.double(), None, 0.25), lambda: G.compute_fpfh_feature(q, n, float("nan")),
        lambda: G.voxel_down_sample(q, 0.0), lambda: G.voxel_select_batched(q, [1, 64], 0.05),
        lambda: G.fpfh_descriptors(q, 0.05, voxelize="grid"), lambda: G.fpfh_descriptors(q, -0.05),
        lambda: G.radius_knn_batched(q, [0, 32, 64], 0.1, 30), lambda: G.estimate_normals_batched(q, [0, 64], 0.1),
        lambda: G.compute_fpfh_batched(q, n, None, 0.25), lambda: G.voxel_down_sample_batched(q, [0, 64], 0.05),
        lambda: G.voxel_select_batched(q, None, 0.05), lambda: G.voxel_down_sample(q, 0.05), lambda: G.voxel_select(q, 0.05),
        lambda: G.estimate_normals(q, 0.1), lambda: G.compute_fpfh_feature(q, n, 0.25), lambda: G.fpfh_descriptors(q, 0.05),
        lambda: G.fpfh_descriptors(q, 0.05, voxelize="select"), lambda: G.fpfh_descriptors(q, 0.05, offsets=[0, 32, 64]),
        # two faults: the scalars before the cloud, the cloud before its offsets, the normals before the device
        lambda: G.radius_knn_batched(q.double(), None, 0.0, 30), lambda: G.radius_knn_batched(q.double(), None, 0.1, 0),
        lambda: G.radius_knn_batched(q.double(), [0, 32], 0.1, 30), lambda: G.compute_fpfh_batched(q, n[:10], [0, 32], 0.25),
        lambda: G.fpfh_descriptors(q.double(), 0.0, voxelize="grid"), lambda: G.fpfh_descriptors(q.double(), 0.0),
    ]):
        add(f"features-{i:02d}", f)

    # ---- multiway.py ------------------------------------------------------------------------------------------------------------
    pts = torch.zeros(10, 3)
    T1 = torch.eye(4, dtype=torch.float64)[None]
    poses3 = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    info1 = torch.eye(6, dtype=torch.float64)[None]
    unc1 = torch.zeros(1, dtype=torch.bool)
    IM, GO, LR, MW = G.information_matrix_batched, G.global_optimization, G.local_refinement_batched, G.multiway_registration
    for i, f in enumerate([
        lambda: IM(pts, [0, 4, 4, 10], [0], [1], T1, 0.1), lambda: IM(pts, [0, 4, 10], [0], [2], T1, 0.1),
        lambda: IM(pts, [0, 4, 10], [0, 1], [1, 0], T1, 0.1), lambda: IM(pts, [0, 4, 10], [0], [1], T1, 0.0),
        lambda: IM(pts.double(), [0, 4, 10], [0], [1], T1, 0.1), lambda: IM(pts[:, :2], [0, 4, 10], [0], [1], T1, 0.1),
        lambda: IM(pts.numpy(), [0, 4, 10], [0], [1], T1, 0.1), lambda: IM(pts, [0, "a", 10], [0], [1], T1, 0.1),
        lambda: IM(pts, [1, 4, 10], [0], [1], T1, 0.1), lambda: IM(pts, [0, 4, 11], [0], [1], T1, 0.1), lambda: IM(pts, [10], [0], [1], T1, 0.1),
        lambda: IM(pts, np.array([0, 4, 10]), [0], [1, 0], T1, 0.1), lambda: IM(pts, torch.tensor([0, 4, 10]), [0], [1], T1.float()[0], 0.1),
        lambda: IM(pts, [0, 4, 10], [0], [1], T1, float("nan")), lambda: IM(pts, [0, 4, 10], [0], [1], T1, 0.1),
        lambda: IM(pts.double(), [0, 4, 4, 10], [0], [2], T1, 0.0), lambda: IM(pts, [0, 4, 4, 10], [0], [2], T1, 0.0),
        lambda: IM(pts, [0, 4, 10], [0], [2], T1[0], 0.0), lambda: IM(pts, [0, 4, 10], [0], [1], T1[0], 0.0),
        lambda: GO(poses3, [1], [1], T1, info1, unc1), lambda: GO(poses3, [0], [3], T1, info1, unc1),
        lambda: GO(poses3, [0], [1], T1, info1, unc1, criteria={"max_iter": 3}), lambda: GO(poses3, [0], [1], T1, info1, unc1, node_offsets=[0, 3]),
        lambda: GO(torch.eye(4, dtype=torch.float64).repeat(257, 1, 1), [0], [1], T1, info1, unc1),
        lambda: GO(poses3, [0], [1], T1, info1, unc1, node_offsets=[0, 2, 2, 3], edge_offsets=[0, 1, 1, 1]),
        lambda: GO(poses3, [0], [1, 2], T1, info1, unc1), lambda: GO(poses3[0], [0], [1], T1, info1, unc1),
        lambda: GO(poses3, [0], [1], T1, info1[0], unc1), lambda: GO(poses3, [0], [1], T1, info1, unc1.float()),
        lambda: GO(poses3, [0], [1], T1, info1, unc1, preference_loop_closure=0.0),
        lambda: GO(poses3, [0], [1], T1, info1, unc1, criteria={"max_iteration": -1}), lambda: GO(poses3[:2], [0], [1], T1, info1, unc1),
        lambda: GO(poses3, [0], [1], T1, info1, unc1, edge_mask=unc1),
        lambda: MW(pts, [0, 3, 6, 10], [0, 0], [1, 2], T1.repeat(2, 1, 1)), lambda: MW(pts, [0, 4, 10], [0], [1], T1),
        lambda: MW(pts, [0, 4, 4, 10], [0, 0], [1, 2], T1), lambda: MW(pts, [0, 4, 10], [0, 1], [1, 1], T1.repeat(2, 1, 1)),
        lambda: LR(pts, [0, 4, 10], [0], [1], T1), lambda: LR(pts, [0, 4, 10], [0], [1], T1, voxel_size=(0.05,), max_iter=(1, 2)),
        lambda: LR(pts, [0, 4, 4, 10], [0], [1], T1, voxel_size=(), max_iter=()),
    ]):
        add(f"multiway-{i:02d}", f)

    # ---- fragments.py, rgbd.py --------------------------------------------------------------------------------------------------
    F = 3
    depth = torch.zeros(F, 8, 12, dtype=torch.float32)
    color3 = torch.zeros(F, 8, 12, 3, dtype=torch.uint8)
    poses = torch.eye(4, dtype=torch.float64).repeat(F, 1, 1)
    K = (10.0, 10.0, 5.5, 3.5)
    singular = poses.clone()
    singular[1] = 0
    nan_pose = poses.clone()
    nan_pose[2, 0, 3] = float("nan")
    table("tsdf", lambda d, P, k, **kw: G.tsdf_fragments(d, P, k, **kw), dict(depth=depth, poses=poses, intrinsic=K), [
        dict(depth=depth.numpy()), dict(depth=depth.double()), dict(depth=depth.to(torch.int32)), dict(depth=depth[0]),
        dict(depth=depth[None]), dict(depth=torch.zeros(F, 0, 12)), dict(poses=poses.numpy()), dict(poses=poses.float()),
        dict(poses=poses[:2]), dict(poses=poses[:, :3]), dict(poses=singular), dict(poses=nan_pose), dict(intrinsic=(10.0, 10.0, 5.5)),
        dict(intrinsic=5.0), dict(intrinsic=(0.0, 10.0, 5, 3)), dict(intrinsic=(10.0, -1.0, 5, 3)),
        dict(intrinsic=(10.0, 10.0, float("nan"), 3)), dict(intrinsic=("a", 1, 2, 3)), dict(frame_offsets=[0]), dict(frame_offsets=[1, 3]),
        dict(frame_offsets=[0, 2]), dict(frame_offsets=[0, 2, 1, 3]), dict(frame_offsets=[0, "a", 3]), dict(frame_offsets=[0, 1.5, 3]),
        dict(frame_offsets=7), dict(frame_offsets=[0] * 65536 + [3]), dict(voxel_length=0.0), dict(voxel_length=float("inf")),
        dict(voxel_length="x"), dict(sdf_trunc=-0.04), dict(sdf_trunc=float("nan")), dict(depth_scale=0.0), dict(depth_scale=float("inf")),
        dict(depth_trunc=0.0), dict(depth_trunc=float("nan")), dict(depth_sampling_stride=0), dict(depth_sampling_stride=2.0),
        dict(max_units=0), dict(max_units=(1 << 22) + 1), dict(max_units=10.5), dict(), dict(depth=depth.to(torch.uint16)),
        dict(frame_offsets=[0, 0, 2, 3], return_volume=True), dict(depth_trunc=float("inf")), dict(depth=depth[:0], poses=poses[:0]),
        dict(depth=torch.zeros(1, dtype=torch.float32).expand(65536, 1, 1), poses=torch.eye(4, dtype=torch.float64).expand(65536, 4, 4)),
        dict(voxel_length=0.0, sdf_trunc=0.0), dict(frame_offsets=[0, 2], voxel_length=0.0), dict(intrinsic=5.0, frame_offsets=[0, 2]),
        dict(max_units=0, poses=singular), dict(depth_scale=0.0, depth_trunc=0.0),
    ], ("depth", "poses", "intrinsic"))
    table("tsdfc", lambda c_, d, P, k, **kw: G.tsdf_fragments_colored(c_, d, P, k, **kw),
          dict(color=color3, depth=depth, poses=poses, intrinsic=K), [
        dict(color=color3.numpy()), dict(color=None), dict(color=color3.float()), dict(color=color3.to(torch.int16)),
        dict(color=color3[..., 0]), dict(color=torch.zeros(F, 8, 12, 4, dtype=torch.uint8)), dict(color=color3[:2]), dict(color=color3[:, :7]),
        dict(color=color3[:, :, :11]), dict(color=torch.zeros(F, 8, 12, 3, dtype=torch.uint8, device="meta")), dict(depth=depth.double()),
        dict(poses=poses[:2]), dict(voxel_length=0.0), dict(frame_offsets=[0, 2]), dict(max_units=0), dict(),
        dict(frame_offsets=[0, 0, 2, 3], return_volume=True), dict(color=color3[:0], depth=depth[:0], poses=poses[:0]),
        dict(color=color3.float(), poses=poses[:2]),
    ], ("color", "depth", "poses", "intrinsic"))

    grey = torch.zeros(F, 8, 12, dtype=torch.uint8)
    d16 = torch.zeros(F, 8, 12, dtype=torch.uint16)
    table("pyr", lambda c_, d, **kw: G.rgbd_pyramids(c_, d, **kw), dict(color=grey, depth=d16), [
        dict(color=grey.numpy()), dict(depth=d16.numpy()), dict(depth=d16.to(torch.int32)), dict(depth=d16.double()), dict(depth=d16[0]),
        dict(depth=d16[:0], color=grey[:0]), dict(color=grey[:2]), dict(color=grey.double()), dict(color=torch.zeros(F, 8, 12, 4, dtype=torch.uint8)),
        dict(color=torch.zeros(F, 8, 12, 3)), dict(color=grey[:, :, :11]), dict(depth_scale=0.0), dict(depth_scale=float("inf")),
        dict(depth_scale="x"), dict(depth_trunc=0.0), dict(depth_trunc=float("nan")), dict(min_depth=-0.1), dict(min_depth=float("nan")),
        dict(min_depth="x"), dict(min_depth=1.0, max_depth=1.0), dict(max_depth=float("nan")), dict(levels=0), dict(levels=9), dict(levels=2.0),
        dict(levels=5), dict(), dict(color=color3), dict(color=grey.float(), depth=d16.float()), dict(levels=4, max_depth=float("inf")),
        dict(depth_scale=0.0, levels=0), dict(color=grey[:2], depth_scale=0.0),
    ], ("color", "depth"))
    L = 3
    pyr = G.RGBDPyramids(torch.zeros(sum(F * 6 * (8 >> l) * (12 >> l) for l in range(L))), F, 8, 12, L)
    add("pyrplanes-00", lambda: pyr.planes(3))
    eye = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    pair_rows = [
        dict(pair_source=[0]), dict(pair_source=[0, 3]), dict(pair_target=[-1, 1]), dict(pair_source=[0, 1.5]), dict(pair_target="ab"),
        dict(pair_source=7), dict(intrinsic=(10.0, 10.0, 5.5)), dict(intrinsic=(0.0, 10.0, 5, 3)), dict(intrinsic=(10.0, 10.0, float("nan"), 3)),
        dict(intrinsic=None), dict(max_depth_diff=-0.01), dict(max_depth_diff=float("inf")), dict(max_depth_diff="x"),
    ]
    table("cmap", lambda **kw: G.rgbd_correspondence_map(**kw),
          dict(pyr=pyr, pair_source=[0, 1], pair_target=[1, 2], transformation=eye, intrinsic=K), pair_rows + [
        dict(pyr=None), dict(level=3), dict(level=-1), dict(level=1.0), dict(transformation=eye.float()), dict(transformation=eye[:1]),
        dict(transformation=eye.numpy()), dict(), dict(pair_source=[0], intrinsic=None), dict(intrinsic=None, level=3),
        dict(level=3, max_depth_diff=-1), dict(max_depth_diff=-1, transformation=eye[:1]),
    ], ())
    table("odo", lambda pc, **kw: G.rgbd_odometry(pc, **kw), dict(pyr_or_color=pyr, pair_source=[0, 1], pair_target=[1, 2], intrinsic=K),
          pair_rows + [
        dict(iterations=(20, 10)), dict(iterations=(20, 10, -1)), dict(iterations=(1.5, 1, 1)), dict(iterations=5), dict(iterations=()),
        dict(odo_init=eye.float()), dict(odo_init=eye[:1]), dict(odo_init=eye), dict(depth=d16), dict(levels=3), dict(pyr_or_color=grey),
        dict(pyr_or_color=grey, depth=d16, jacobian="color"), dict(pyr_or_color=grey, depth=d16.to(torch.int32)),
        dict(pyr_or_color=grey, depth=d16, levels=9), dict(pyr_or_color=grey, depth=d16, min_depth=-1.0), dict(pyr_or_color=grey, depth=d16),
        dict(pyr_or_color=grey, depth=d16, iterations=(3, 3)), dict(), dict(return_trace=True, pair_source=[], pair_target=[]),
        dict(iterations=5, intrinsic=None), dict(intrinsic=None, max_depth_diff="x"), dict(max_depth_diff="x", pair_source=[0]),
    ], ("pyr_or_color",))
    table("frag", lambda c_, d, k, **kw: G.rgbd_fragments(c_, d, k, **kw), dict(color=grey, depth=d16, intrinsic=K), [
        dict(depth=d16.numpy()), dict(depth=d16[0]), dict(frame_offsets=[0]), dict(frame_offsets=[1, 3]), dict(frame_offsets=[0, 2, 1, 3]),
        dict(frame_offsets=[0, 1.5, 3]), dict(frame_offsets=7), dict(preference_loop_closure=0.0), dict(preference_loop_closure="x"),
        dict(intrinsic=(10.0, 10.0)), dict(intrinsic=(10.0, -10.0, 1, 1)), dict(voxel_size=0.01), dict(max_depth_diff=-1.0),
        dict(min_depth=-1.0), dict(max_depth=0.2), dict(color=grey[:2]), dict(depth_scale=0.0), dict(),
        dict(frame_offsets=[0, 2, 2, 3], optimize=False, voxel_length=0.02), dict(color=grey[:0], depth=d16[:0]),
        dict(color=grey, colors=True), dict(color=grey.float(), colors=True), dict(color=grey.numpy(), colors=True), dict(color=color3, colors=1.5),
        dict(color=color3, colors=1), dict(color=color3, colors="yes"), dict(color=color3, colours=True), dict(color=color3, colors=True),
        dict(color=color3, colors=False), dict(color=color3[:0], colors=True, depth=d16[:0]), dict(color=None, depth=d16[:0]),
        dict(frame_offsets=[0], preference_loop_closure=0.0), dict(preference_loop_closure=0.0, intrinsic=(10.0, 10.0)),
    ], ("color", "depth", "intrinsic"))

    # ---- dgr.py, matching.py, correspondences.py, registration.py ---------------------------------------------------------------------
    x0, x1, Te = torch.zeros(10, 3), torch.zeros(12, 3), torch.eye(4).repeat(2, 1, 1)
    MI = G.matching_indices_batched
    feats = lambda rows, d=8: torch.zeros(rows, d)      # noqa: E731
    iC = torch.zeros(10, 4, dtype=torch.int32)
    pred = [torch.zeros(3, 2, dtype=torch.int64)] * 2
    GI = lambda *a, **k: G.generate_inlier_input(None, None, None, *a, **k)      # noqa: E731
    P6, Q5, S6, T5 = torch.zeros(6, 3), torch.zeros(5, 3), torch.zeros(6, 32), torch.zeros(5, 32)
    BC = G.build_correspondences
    for i, f in enumerate([
        lambda: MI(x0, [0, 7, 5, 10], x1, [0, 4, 8, 12], torch.eye(4).repeat(3, 1, 1), 0.1), lambda: MI(x0, [0, 4, 10], x1, [0, 13, 12], Te, 0.1),
        lambda: MI(x0, [1, 4, 10], x1, [0, 6, 12], Te, 0.1), lambda: MI(x0, [0, "a", 10], x1, [0, 6, 12], Te, 0.1),
        lambda: MI(x0, [0, 4, 10], x1, [0, 12], Te, 0.1), lambda: MI(x0, [0, 4, 10], x1, [0, 6, 12], Te[:1], 0.1),
        lambda: MI(x0, [0, 4, 10], x1, [0, 6, 12], Te, 0.0), lambda: MI(x0, [0, 4, 10], x1, [0, 6, 12], Te, float("inf")),
        lambda: MI(x0.double(), [0, 4, 10], x1, [0, 6, 12], Te, 0.1), lambda: MI(x0, [0, 4, 10], x1[:0], [0, 0, 0], Te, 0.1),
        lambda: MI(x0, [0, 4, 4, 10], x1, [0, 6, 12, 12], torch.eye(4).repeat(3, 1, 1), 0.1), lambda: MI(x0, [0, 4, 10], x1, [0, 6, 12], Te, 0.1),
        lambda: MI(x0, np.array([0, 4, 10]), x1, torch.tensor([0, 6, 12]), Te, 0.1),
        lambda: MI(x0.double(), [0, 4], x1, [0, 6, 12], Te, 0.0), lambda: MI(x0, [0, 4], x1, [0, 6], Te, 0.0), lambda: MI(x0, [0, 4, 10], x1, [0, 6, 12], Te[:1], 0.0),
        lambda: G.find_correct_correspondence(pred[:1], pred, hash_seed=10), lambda: G.find_correct_correspondence(pred, pred, len_batch=[(3, 3)]),
        lambda: G.find_correct_correspondence(pred, pred), lambda: G.find_correct_correspondence(pred, pred, hash_seed=10),
        lambda: G.find_correct_correspondence([], [], hash_seed=10), lambda: G.find_correct_correspondence(pred, [p_.float() for p_ in pred], hash_seed=10),
        lambda: GI(iC, iC, None, None, [(4, 5), (5, 5)], None, inlier_feature_type="ones"), lambda: GI(iC, iC, None, None, [(10, 10)], None, inlier_feature_type="counts"),
        lambda: GI(iC, iC, None, None, [(10, 10)], None, inlier_feature_type=None), lambda: GI(iC, iC, None, None, [(10, 10)], None, inlier_feature_type="ones", knn=2),
        lambda: GI(iC.float(), iC, None, None, [(10, 10)], None, inlier_feature_type="ones"), lambda: GI(iC, iC[:, :3], None, None, [(10, 10)], None, inlier_feature_type="ones"),
        lambda: GI(iC, iC, None, None, [(10, 10)], pred, inlier_feature_type="ones"), lambda: GI(iC, iC, None, None, [], None, inlier_feature_type="ones"),
        lambda: GI(iC, iC, None, None, 5, None, inlier_feature_type="ones"), lambda: GI(iC, iC, None, None, [(-1, 10), (11, 0)], None, inlier_feature_type="ones"),
        lambda: G.generate_inlier_input(None, x0[:9], x0, iC, iC, None, None, [(10, 10)], None, inlier_feature_type="coords"),
        lambda: G.generate_inlier_input(torch.nn.Linear(1, 1), x0, x0, iC, iC, None, None, [(10, 10)], None, inlier_feature_type="coords"),
        lambda: G.dgr.load_model("SimpleNet"), lambda: G.dgr.inlier_in_channels("counts", 32), lambda: G.dgr.parse_network_config({"feat_model": "x"}),
        lambda: G.find_knn_gpu_batch(feats(10, 8), feats(12, 9), [(10, 12)]), lambda: G.find_knn_batch(feats(10, 8), feats(12, 9), [(10, 12)]),
        lambda: G.find_pairs(feats(10, 8), feats(12, 9), [(10, 12)]), lambda: G.find_knn_gpu_batch(feats(10), feats(12), [(4, 6), (5, 6)]),
        lambda: G.find_pairs(feats(10), feats(12), [(4, 6), (5, 6)]), lambda: G.find_knn_gpu_batch(feats(10), feats(12), [(10, 12)], knn=2),
        lambda: G.find_knn_batch(feats(10), feats(12), [(10, 12)], knn=2), lambda: G.find_pairs(feats(10), feats(12), [(10, 12)], knn=2),
        lambda: G.find_knn_batch(feats(10), feats(12), [(10, 12)], search_method="cpu"), lambda: G.find_knn_batch(feats(10), feats(12), [(10, 12)], search_method="kdtree"),
        lambda: G.find_knn_gpu_batch(feats(4, 129), feats(4, 129), [(4, 4)]), lambda: G.find_knn_gpu_batch(feats(4), feats(4), [(4, 4)]),
        lambda: G.find_knn_gpu_batch(feats(4).numpy(), feats(4), [(4, 4)]), lambda: G.find_knn_gpu_batch(feats(4)[0], feats(4), [(4, 4)]),
        lambda: G.find_pairs(feats(4), feats(4), [(4, 4)]), lambda: G.find_knn_gpu_batch(feats(4).double(), feats(4).double(), [(4, 4)]),
        lambda: G.find_knn_gpu(feats(4), feats(4)), lambda: G.find_knn_gpu(feats(4), feats(4), knn=2), lambda: G.nn_match(feats(4), feats(4)),
        lambda: G.nn_match_mutual(S6, torch.zeros(5, 33)), lambda: BC(P6, Q5, S6, torch.zeros(5, 33)), lambda: G.nn_match_mutual(S6, T5, [(3, 5), (2, 0)]),
        lambda: BC(P6, Q5, S6, T5, [(6, 4)]), lambda: BC(P6, Q5, S6, T5, [(3, 5), (3, 0)]), lambda: BC(P6, Q5, S6, T5, gt_trans=torch.eye(4)[None]),
        lambda: BC(P6, Q5, S6, T5, [(3, 2), (3, 3)], gt_trans=torch.eye(4)[None], inlier_threshold=0.1), lambda: BC(P6[:5], Q5, S6, T5),
        lambda: BC(P6, Q5, S6, T5, in_dim=12), lambda: BC(P6, Q5, S6, T5, gt_trans=torch.eye(4), inlier_threshold=0.0),
        lambda: G.nn_match_mutual(S6.numpy(), T5), lambda: G.nn_match_mutual(torch.zeros(6, 129), torch.zeros(5, 129)),
        lambda: G.nn_match_mutual(S6, T5), lambda: G.nn_match_mutual(S6, T5, [(2, 1), (4, 4)]),
        lambda: BC(P6, Q5, S6, T5, gt_trans=torch.eye(4), inlier_threshold=0.1, gather_desc=True), lambda: BC(P6[:5], Q5, S6, T5, in_dim=12),
        lambda: G.weighted_procrustes_batched(x0, x0, torch.zeros(10), [0, 4, 10], 1e-6), lambda: G.weighted_procrustes(x0, x0, torch.zeros(10), 1e-6),
        lambda: G.global_registration_batched(x0, x0, None, [0, 4, 10]), lambda: G.GlobalRegistration(x0, x0, loss_fn=object()),
        lambda: G.argmin_se3_squared_dist(x0, x0),
    ]):
        add(f"dgr-{i:02d}", f)
    return out


def _outcome(fn):
    try:
        fn()
    except Exception as err:      # noqa: BLE001 - the type is what is recorded
        return type(err).__name__, str(err).replace("\\", "\\\\").replace("\n", "\\n").replace("\t", "\\t")
    return "no exception", ""


def record(path):
    with open(path, "w") as f:
        for cid, fn in _cases():
            kind, msg = _outcome(fn)
            f.write(f"{cid}\t{kind}\t{msg}\n")


def _golden():
    with open(GOLDEN) as f:
        return dict((line.split("\t", 1)[0], tuple(line.rstrip("\n").split("\t", 2)[1:])) for line in f if line.strip())


def test_every_check_raises_what_it_raised():
    golden = _golden()
    cases = _cases()
    assert [cid for cid, _ in cases] == list(golden), "the table and the golden file list the same cases in the same order"
    assert len(cases) > 400
    wrong = []
    for cid, fn in cases:
        got = _outcome(fn)
        assert got[0] != "no exception", cid
        if got != golden[cid]:
            wrong.append((cid, got, golden[cid]))
    assert not wrong, "\n".join(f"{cid}: got {g!r}, recorded {w!r}" for cid, g, w in wrong)


def test_golden_file_is_well_formed():
    golden = _golden()
    kinds = {k for k, _ in golden.values()}
    assert kinds <= {"RuntimeError", "NotImplementedError", "ValueError", "KeyError"}, kinds
    for cid, (kind, msg) in golden.items():
        if kind in ("RuntimeError", "NotImplementedError"):
            assert msg.startswith("gmf_amd"), (cid, msg)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
