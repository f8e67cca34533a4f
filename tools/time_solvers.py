"""Times the evaluation solvers (gmf_amd/solvers.py) at the sizes the reference's evaluation scripts run them:

  PointDSC RANSAC   one pair, N = 5000 correspondences (~60 % masked in), 5000 hypotheses, ransac_n = 3, tau = 0.10
  PointDSC ICP      keypoints, N = 5000 / 5000, tau = 0.10, open3d's default criteria (30 passes at most)
  DGR RANSAC        80 000 hypotheses, ransac_n = 4, N = 8000 and 30 000 correspondences, tau = 0.06
  DGR ICP           brute-force nearest neighbour, clouds of 10k / 10k and 50k / 50k points, tau = 0.05
  ICP search        search="brute" against search="grid", alternated call by call in this one process: keypoints 5000 / 5000
                    (tau = 0.10), clouds of 10k / 10k and 50k / 50k (tau = 0.05).  Per shape and search: the whole call at the
                    default criteria; then, with both relative criteria at 0 so that every pass runs, the call at
                    max_iteration = 0 (t0) and at 10 (t10).  One pass = (t10 - t0) / 10 is the search AND k_icp_step;
                    the step is the same kernel on the same data in both columns, so the difference of the columns is the
                    difference of the two searches.  The grid build = (t0 grid - t0 brute) + (pass brute - pass grid): the
                    first term is the build plus the difference of one search, the second takes that difference out again.
                    The search kernels alone (and the build's kernels one by one) are kernel times: run
                    rocprofv3 --kernel-trace --stats -- python tools/time_solvers.py --icp-shape 50k   (one shape per
                    process, so that the per-kernel averages belong to one size; shapes: keypoints, 10k, 50k).
                    tools/icp_trace_passes.py picks the working passes out of such a trace.
  ICP crossover     whole calls, brute against grid, at keypoint pairs of 125 ... 2000 rows.
  ICP point-to-plane   icp_point_to_point_batched against icp_point_to_plane_batched on the "ICP search" shapes, both with
                    search="grid", alternated call by call in this one process; the targets' normals come from
                    estimate_normals_batched (radius 2 tau, 30 neighbours) outside the timed region.  Whole calls at the default
                    criteria (the two estimators run different numbers of passes), then t0 and t10 as above: one pass is the
                    same search and k_icp_step in one column, k_icp_plane_partials + k_icp_plane_solve in the other, so the
                    difference of the columns is the difference of the steps (--plane-shape runs this block alone).
  ICP coloured      icp_point_to_plane_batched against icp_colored_batched on the "ICP search" shapes, both with search="grid",
                    alternated call by call; normals as above, intensities from a smooth field, the targets' colour gradients
                    computed outside the timed region and passed.  Whole calls, then t0 and t10 as above: one pass differs by
                    k_icp_color_partials against k_icp_plane_partials alone.  Beside them radius_knn_batched and
                    color_gradients_batched (the same search and k_color_gradient) at radius 2 tau, 30 neighbours, and the
                    10-pass call that computes its gradients itself (--colored-shape runs this block alone; under
                    rocprofv3 --kernel-trace --stats it gives the kernel times).
  feature-matching RANSAC   DGR's call: ransac_n = 4, the distance checker and tau at 2 voxels (0.10), 80 000 proposals, 1000
                    validations; clouds of 10k / 10k and 50k / 50k points (40 % of the feature matches right, the others random)
                    and keypoints 5000 / 5000.  The whole call with search="grid", and search="brute" beside it where the
                    brute-force search is affordable (not at 50k: 2.5e12 distance tests).  The evaluation kernel alone is a
                    kernel time: rocprofv3 --kernel-trace --stats -- python tools/time_solvers.py --fm-shape 50k   (one shape
                    per process; shapes: keypoints, 10k, 50k); searches per second = validated x Ns over k_fm_eval's time.

Device events around each call, after warm-up; median and spread over repeats.  For RANSAC the row tests per second and the share
of the fp32 vector peak (15 vector ops per hypothesis-row test, the issue's count, at 157.3 TFLOP/s) are printed too.
Usage: python tools/time_solvers.py [--repeats 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import synthetic        # noqa: E402

PEAK_F32_VECTOR = 157.3e12


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


def timed_alternating(fns, repeats, warmup=3):
    """Medians (us) of several callables timed in turn, one call each per round, so that drift hits all alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


ICP_SHAPES = ("keypoints", "10k", "50k")


def icp_shape(key):
    if key == "keypoints":
        p = synthetic.synthetic_pair(1, 5000)
        return ("keypoints 5000/5000 tau=0.10", torch.as_tensor(p["src_keypts"])[None], torch.as_tensor(p["tgt_keypts"])[None],
                torch.as_tensor(p["gt_trans"])[None], 0.10)
    N = {"10k": 10000, "50k": 50000}[key]
    s, q, T0 = cloud_pair(N, 5)
    return (f"cloud {key}/{key} tau=0.05", torch.as_tensor(s)[None], torch.as_tensor(q)[None], torch.as_tensor(T0)[None], 0.05)


def icp_search_rows(report, repeats, dev, keys=ICP_SHAPES):
    """search="brute" against search="grid" (the module docstring's "ICP search")."""
    report("ICP search: brute | grid, alternated; us, median")
    for name, s, q, T0, tau in (icp_shape(k) for k in keys):
        s, q, T0 = s.to(dev), q.to(dev), T0.to(dev)
        out = {k: gmf_amd.icp_point_to_point_batched(s, q, T0, tau, search=k) for k in ("brute", "grid")}
        same = all(torch.equal(x, y) for x, y in zip(out["brute"], out["grid"]))
        it = int(out["brute"][3][0])

        def call(search, **kw):
            return lambda: gmf_amd.icp_point_to_point_batched(s, q, T0, tau, search=search, **kw)

        every = dict(relative_fitness=0.0, relative_rmse=0.0)
        fns = [call(k, **kw) for kw in ({}, dict(max_iteration=0, **every), dict(max_iteration=10, **every))
               for k in ("brute", "grid")]
        (wb, wg, b0, g0, b10, g10) = timed_alternating(fns, repeats)
        pb, pg = (b10 - b0) / 10, (g10 - g0) / 10
        report(f"  {name}: outputs bit-identical: {same}; {it} passes")
        report(f"    whole call        {wb:9.1f} | {wg:9.1f}")
        report(f"    max_iteration=0   {b0:9.1f} | {g0:9.1f}   (init, for the grid its build, one search, one evaluation)")
        report(f"    one pass          {pb:9.1f} | {pg:9.1f}   (search + k_icp_step; the searches differ by {pb - pg:.1f})")
        report(f"    grid build                  | {(g0 - b0) + (pb - pg):9.1f}   ((t0 grid - t0 brute) + (pass brute - pass grid))")


def icp_plane_rows(report, repeats, dev, keys=ICP_SHAPES):
    """Point-to-point against point-to-plane (the module docstring's "ICP point-to-plane")."""
    report("ICP point-to-plane: point-to-point | point-to-plane, search=\"grid\", alternated; us, median")
    for name, s, q, T0, tau in (icp_shape(k) for k in keys):
        s, q, T0 = s.to(dev), q.to(dev), T0.to(dev)
        n = gmf_amd.estimate_normals_batched(q[0], [0, q.shape[1]], 2 * tau, 30)[None]

        def call(plane, **kw):
            if plane:
                return lambda: gmf_amd.icp_point_to_plane_batched(s, q, n, T0, tau, search="grid", **kw)
            return lambda: gmf_amd.icp_point_to_point_batched(s, q, T0, tau, search="grid", **kw)

        its = [int(call(k)()[3][0]) for k in (False, True)]
        every = dict(relative_fitness=0.0, relative_rmse=0.0)
        fns = [call(k, **kw) for kw in ({}, dict(max_iteration=0, **every), dict(max_iteration=10, **every)) for k in (False, True)]
        (wa, wb, a0, b0, a10, b10) = timed_alternating(fns, repeats)
        pa, pb = (a10 - a0) / 10, (b10 - b0) / 10
        report(f"  {name}: {its[0]} | {its[1]} passes at the default criteria")
        report(f"    whole call        {wa:9.1f} | {wb:9.1f}")
        report(f"    max_iteration=0   {a0:9.1f} | {b0:9.1f}   (init, the grid build, one search, one evaluation)")
        report(f"    one pass          {pa:9.1f} | {pb:9.1f}   (search + k_icp_step | search + k_icp_plane_partials + "
               f"k_icp_plane_solve; the steps differ by {pb - pa:.1f})")


def smooth_intensity(x):
    """A smooth intensity in 0.15 .. 0.85 at the rows of x [N,3] (a tensor)."""
    return (0.5 + 0.2 * torch.sin(3 * x[:, 0] + 0.5) * torch.cos(2 * x[:, 1]) + 0.15 * torch.sin(2.5 * x[:, 2] + 1.7 * x[:, 0] - 1.1 * x[:, 1])).float()


def icp_colored_rows(report, repeats, dev, keys=ICP_SHAPES):
    """Point-to-plane against coloured ICP, and the colour gradients beside their search (the module docstring's "ICP coloured")."""
    report("ICP coloured: point-to-plane | coloured (gradients passed), search=\"grid\", alternated; us, median")
    for name, s, q, T0, tau in (icp_shape(k) for k in keys):
        s, q, T0 = s.to(dev), q.to(dev), T0.to(dev)
        off = [0, q.shape[1]]
        n = gmf_amd.estimate_normals_batched(q[0], off, 2 * tau, 30)
        it_ = smooth_intensity(q[0])
        is_ = smooth_intensity(s[0] @ T0[0, :3, :3].T + T0[0, :3, 3])
        g = gmf_amd.color_gradients_batched(q[0], n, it_, off, 2 * tau, 30)

        def call(colored, **kw):
            if colored:
                return lambda: gmf_amd.icp_colored_batched(s, q, is_[None], it_[None], n[None], T0, tau, search="grid",
                                                           target_gradients=g[None], **kw)
            return lambda: gmf_amd.icp_point_to_plane_batched(s, q, n[None], T0, tau, search="grid", **kw)

        its = [int(call(k)()[3][0]) for k in (False, True)]
        every = dict(relative_fitness=0.0, relative_rmse=0.0)
        fns = [call(k, **kw) for kw in ({}, dict(max_iteration=0, **every), dict(max_iteration=10, **every)) for k in (False, True)]
        fns += [lambda: gmf_amd.radius_knn_batched(q[0], off, 2 * tau, 30),
                lambda: gmf_amd.color_gradients_batched(q[0], n, it_, off, 2 * tau, 30),
                lambda: gmf_amd.icp_colored_batched(s, q, is_[None], it_[None], n[None], T0, tau, search="grid",
                                                    max_iteration=10, **every)]
        (wa, wb, a0, b0, a10, b10, knn, grad, c10) = timed_alternating(fns, repeats)
        pa, pb = (a10 - a0) / 10, (b10 - b0) / 10
        report(f"  {name}: {its[0]} | {its[1]} passes at the default criteria")
        report(f"    whole call        {wa:9.1f} | {wb:9.1f}")
        report(f"    max_iteration=0   {a0:9.1f} | {b0:9.1f}   (init, the grid build, one search, one evaluation)")
        report(f"    max_iteration=10  {a10:9.1f} | {b10:9.1f}   (equal pass counts; gradients computed inside: {c10:.1f})")
        report(f"    one pass          {pa:9.1f} | {pb:9.1f}   (search + k_icp_plane_partials | k_icp_color_partials + "
               f"k_icp_plane_solve; the steps differ by {pb - pa:.1f})")
        report(f"    radius search (2 tau, 30) {knn:9.1f}; color_gradients_batched (the search and k_color_gradient) {grad:9.1f}")


def icp_crossover_rows(report, repeats, dev):
    """Whole calls at small keypoint pairs (tau = 0.10, default criteria, gt pose as init), to find the size below which the
    grid's four extra launches cost more than its search saves."""
    report("ICP search, small keypoint pairs: whole call, brute | grid, alternated; us, median")
    for N in (125, 250, 500, 1000, 2000):
        p = synthetic.synthetic_pair(1, N)
        s, q = torch.as_tensor(p["src_keypts"]).to(dev)[None], torch.as_tensor(p["tgt_keypts"]).to(dev)[None]
        T0 = torch.as_tensor(p["gt_trans"]).to(dev)[None]
        it = int(gmf_amd.icp_point_to_point_batched(s, q, T0, 0.10)[3][0])
        fns = [lambda k=k: gmf_amd.icp_point_to_point_batched(s, q, T0, 0.10, search=k) for k in ("brute", "grid")]
        wb, wg = timed_alternating(fns, repeats)
        report(f"  keypoints {N}/{N} tau=0.10 ({it} passes): {wb:9.1f} | {wg:9.1f}")


FM_SHAPES = ("keypoints", "10k", "50k")


def fm_shape(key):
    """-> (name, src [1,N,3], tgt [1,N,3], nn [1,N], tau): row i of the target is row i of the source moved; nn is i for the
    right feature matches and a random row for the others."""
    if key == "keypoints":
        p = synthetic.synthetic_pair(1, 5000)
        s, q = p["src_keypts"], p["tgt_keypts"]
        good = np.asarray(p["gt_labels"]) > 0
    else:
        N = {"10k": 10000, "50k": 50000}[key]
        s, q, _ = cloud_pair(N, 5)
        good = np.random.default_rng([7, N]).random(N) < 0.4
    n = len(good)
    nn = np.where(good, np.arange(n), np.random.default_rng([8, n]).integers(0, n, n))
    name = f"{'keypoints' if key == 'keypoints' else 'cloud'} {n}/{n} tau=0.10, {good.mean():.0%} right matches"
    return name, torch.as_tensor(s)[None], torch.as_tensor(q)[None], torch.as_tensor(nn)[None], 0.10


def fm_rows(report, repeats, dev, keys=FM_SHAPES):
    """The module docstring's "feature-matching RANSAC"."""
    report("feature-matching RANSAC: n=4, 80 000 proposals, 1000 validations, checker = tau; whole call, us, median [min, max]")
    for key in keys:
        name, s, q, nn, tau = fm_shape(key)
        s, q, nn = s.to(dev), q.to(dev), nn.to(dev)
        kw = dict(ransac_n=4, checker_distance=tau, max_iteration=80000, max_validation=1000, return_hypotheses=True)

        def call(search):
            return lambda: gmf_amd.ransac_feature_matching_batched(s, q, nn, tau, search=search, **kw)

        grid = call("grid")()
        nv, last = int(grid[6][0]), int(grid[7][0].max())
        report(f"  {name}: {nv} validated (the last is proposal {last}), fitness {float(grid[1][0]):.3f}, "
               f"{nv * s.shape[1] / 1e6:.1f} M searches")
        if key == "50k":
            med, lo, hi = timed(call("grid"), repeats)
            report(f"    grid  {med:10.1f} [{lo:.1f}, {hi:.1f}]   (brute force not run at this size)")
            continue
        same = all(torch.equal(x, y) for x, y in zip(grid, call("brute")()))
        mb, mg = timed_alternating([call("brute"), call("grid")], max(3, repeats // 2), warmup=2)
        report(f"    brute {mb:10.1f} | grid {mg:10.1f}   (alternated; outputs bit-identical: {same})")


def cloud_pair(N, seed):
    r = np.random.default_rng([seed, N])
    X = r.uniform(0, 3, (N, 3))
    R = synthetic.random_rotation(r)
    t = r.uniform(-0.5, 0.5, 3)
    tgt = (X @ R.T + t + r.normal(0, 0.005, X.shape)).astype(np.float32)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, :3], T0[:3, 3] = R, t + 0.02
    return X.astype(np.float32), tgt, T0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--icp-shape", choices=ICP_SHAPES, default=None, help="only the ICP search rows of one shape (for a kernel trace)")
    ap.add_argument("--plane-shape", choices=ICP_SHAPES + ("all",), default=None,
                    help="only the point-to-plane rows of one shape, or of all three")
    ap.add_argument("--colored-shape", choices=ICP_SHAPES + ("all",), default=None,
                    help="only the coloured ICP rows of one shape, or of all three")
    ap.add_argument("--fm-shape", choices=FM_SHAPES, default=None,
                    help="only the feature-matching RANSAC rows of one shape (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_solvers.py measures on a HIP device"
    dev = "cuda:0"
    lines = []

    def report(s):
        print(s, flush=True)
        lines.append(s)

    report(f"device: {torch.cuda.get_device_name(0)}; median [min, max] over {a.repeats} repeats, device events")
    if a.icp_shape:
        icp_search_rows(report, a.repeats, dev, (a.icp_shape,))
        return
    if a.plane_shape:
        icp_plane_rows(report, a.repeats, dev, ICP_SHAPES if a.plane_shape == "all" else (a.plane_shape,))
        return
    if a.colored_shape:
        icp_colored_rows(report, a.repeats, dev, ICP_SHAPES if a.colored_shape == "all" else (a.colored_shape,))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.fm_shape:
        fm_rows(report, a.repeats, dev, (a.fm_shape,))
        return

    # PointDSC RANSAC
    p = synthetic.synthetic_pair(1, 5000)
    src, tgt = torch.as_tensor(p["src_keypts"]).to(dev)[None], torch.as_tensor(p["tgt_keypts"]).to(dev)[None]
    r = np.random.default_rng(2)
    mask = torch.as_tensor(np.where(p["gt_labels"] > 0, r.random(5000) < 0.9, r.random(5000) < 0.55)).to(dev)[None]
    M = int(mask.sum())
    med, lo, hi = timed(lambda: gmf_amd.ransac_correspondence_batched(src, tgt, 0.10, mask=mask, ransac_n=3,
                                                                      num_hypotheses=5000), a.repeats)
    report(f"PointDSC RANSAC  N=5000 M={M} H=5000 n=3: {med:8.1f} us [{lo:.1f}, {hi:.1f}]  "
           f"{5000 * M / med * 1e-3:.1f} G row-tests/s")

    # PointDSC ICP
    T0 = torch.as_tensor(p["gt_trans"]).to(dev)[None]
    med, lo, hi = timed(lambda: gmf_amd.icp_refine(src, tgt, T0), a.repeats)
    it = int(gmf_amd.icp_point_to_point_batched(src, tgt, T0, 0.10)[3][0])
    report(f"PointDSC ICP     N=5000/5000 tau=0.10: {med:8.1f} us [{lo:.1f}, {hi:.1f}]  ({it} passes)")

    # DGR RANSAC
    for N in (8000, 30000):
        X, Y = synthetic.dgr_scene(N, 3)[:2]
        X, Y = X.to(dev)[None], Y.to(dev)[None]
        med, lo, hi = timed(lambda: gmf_amd.ransac_correspondence_batched(X, Y, 0.06, ransac_n=4, num_hypotheses=80000),
                            a.repeats)
        tests = 80000 * N
        report(f"DGR RANSAC       N={N} H=80000 n=4: {med:8.1f} us [{lo:.1f}, {hi:.1f}]  {tests / med * 1e-3:.0f} G row-tests/s, "
               f"{100 * tests * 15 / (med * 1e-6) / PEAK_F32_VECTOR:.0f} % of the fp32 vector peak at 15 ops per test")

    # DGR ICP (brute force)
    for N in (10000, 50000):
        s, q, T0 = cloud_pair(N, 5)
        s, q, T0 = torch.as_tensor(s).to(dev)[None], torch.as_tensor(q).to(dev)[None], torch.as_tensor(T0).to(dev)[None]
        res = gmf_amd.icp_point_to_point_batched(s, q, T0, 0.05)
        it = int(res[3][0])
        med, lo, hi = timed(lambda: gmf_amd.icp_point_to_point_batched(s, q, T0, 0.05), max(3, a.repeats // 4), warmup=1)
        per = med / (it + 1)
        report(f"DGR ICP          N={N}/{N} tau=0.05: {med:8.1f} us [{lo:.1f}, {hi:.1f}]  ({it} passes, {per:.1f} us per "
               f"nearest-neighbour pass, {N * N / per * 1e-3:.0f} G distance tests/s)")
    icp_search_rows(report, a.repeats, dev)
    icp_crossover_rows(report, a.repeats, dev)
    icp_plane_rows(report, a.repeats, dev)
    icp_colored_rows(report, a.repeats, dev)
    fm_rows(report, a.repeats, dev)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
