"""Times multiway registration.  There is no earlier code to compare with: the figures are absolute.

Cases (--case, one per process so that a job script can give each its own time limit):
  info_keypoints     information matrices of all 1596 pairs of 57 clouds of 20 000 rows (the reference's num_node configuration)
  info_full          the same for 400 edges over 29 clouds of 100 000 rows
  optimise_57        one global_optimization of a 57-node graph with 56 odometry edges and 300 loop closures (30 of them false),
                     and beside it the host time of the NumPy restatement (tests/posegraph_reference.py), as context
  optimise_256       the largest graph that is built: 256 nodes, 255 + 2000 edges (one run; no restatement, it would take minutes)
  multiway           multiway_registration of 12 fragments of about 6000 points cut from one surface, without and with ICP

Every window is `--inner` calls between two device events, ended by a synchronise; after a warm-up, the median with min and max
over `--repeats` windows, in us per call.  Fails without a GPU.

Usage: python tools/multiway_ab.py --case NAME [--repeats 9] [--inner 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmf_amd                          # noqa: E402
import posegraph_reference as R         # noqa: E402


def timed(fn, repeats, inner, warmup=2):
    """-> (median, min, max) in us per call, from device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def fmt(name, t):
    return f"  {name:44s} {t[0]:12.1f}  [{t[1]:12.1f}, {t[2]:12.1f}]"


def surface(rng, n, length=3.0):
    xy = rng.uniform([0, 0], [length, 3.0], (n, 2))
    z = 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(4.0 * xy[:, 1]) + 0.05 * np.sin(11.0 * xy[:, 0] + 2.0 * xy[:, 1])
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def case_info(dev, F, n, E, a):
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(np.concatenate([surface(rng, n) for _ in range(F)])).to(dev)
    off = list(range(0, F * n + 1, n))
    pairs = [(s, t) for s in range(F) for t in range(s + 1, F)][:E]
    src, tgt = [p[0] for p in pairs], [p[1] for p in pairs]
    T = torch.eye(4, dtype=torch.float64, device=dev).repeat(len(pairs), 1, 1)
    T[:, 0, 3] = 0.003                                        # (not the identity: every row is transformed)
    info, count = gmf_amd.information_matrix_batched(pts, off, src, tgt, T, 0.07)
    torch.cuda.synchronize()
    frac = float(count.double().mean()) / n
    t = timed(lambda: gmf_amd.information_matrix_batched(pts, off, src, tgt, T, 0.07), a.repeats, a.inner)
    return [f"information matrices: {len(pairs)} edges over {F} clouds of {n} rows, tau 0.07 ({frac:.2f} of the rows matched)",
            fmt("information_matrix_batched", t), f"  = {t[0] / len(pairs):.2f} us per edge"]


def big_graph(n, n_true, n_false, seed=0):
    return R.planted_graph(seed, n=n, n_true=n_true, n_false=n_false, noise=0.002, rot=0.3, trans=0.5)


def device_graph(g, dev):
    f = lambda k, dt: torch.as_tensor(np.ascontiguousarray(g[k]), dtype=dt).to(dev)      # noqa: E731
    return (f("poses0", torch.float64), g["src"], g["tgt"], f("X", torch.float64), f("info", torch.float64), f("unc", torch.bool))


def case_optimise(dev, n, n_true, n_false, a, restate):
    g = big_graph(n, n_true, n_false)
    args = device_graph(g, dev)
    P, l, kept, st = gmf_amd.global_optimization(*args, **R.REFERENCE_OPTIONS)
    torch.cuda.synchronize()
    gmf_amd.check_status()
    pruned = (~kept).cpu().numpy()
    its = st["iterations"].cpu().numpy().tolist()[0]
    lines = [f"global_optimization: {n} nodes, {n - 1} + {n_true + n_false} edges ({n_false} false closures); pruned == planted: "
             f"{bool(np.array_equal(pruned, g['planted']))}; outer iterations per pass {its}, rejected "
             f"{st['rejected'].cpu().numpy().tolist()[0]}, stop {st['stop'].cpu().numpy().tolist()[0]}"]
    t = timed(lambda: gmf_amd.global_optimization(*args, **R.REFERENCE_OPTIONS), a.repeats if restate else 1, a.inner if restate else 1,
              warmup=1 if restate else 0)
    lines.append(fmt("global_optimization (device)", t))
    if restate:
        t0 = time.perf_counter()
        rP, rl, rkept, rst = R.run(g, **R.REFERENCE_OPTIONS)
        host = (time.perf_counter() - t0) * 1e6
        lines.append(f"  {'NumPy restatement (host, one run; context)':44s} {host:12.1f}")
        lines.append(f"  device against restatement: kept equal {bool(np.array_equal(rkept, kept.cpu().numpy()))}, "
                     f"max|dP| {np.abs(rP - P.cpu().numpy()).max():.3e}")
    return lines


def fragments(rng, n_frag, width, step, n_points, noise):
    length = step * (n_frag - 1) + width
    world = surface(rng, n_points, length).astype(np.float64)
    gt = [np.eye(4)]
    for i in range(1, n_frag):
        T = R.random_pose(rng, 0.4, 0.1)
        T[:3, 3] += [step * i, 0.0, 0.0]
        gt.append(T)
    clouds = []
    for i in range(n_frag):
        w = world[(world[:, 0] >= step * i) & (world[:, 0] < step * i + width)]
        Pi = np.linalg.inv(gt[i])
        clouds.append((w @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32))
    pairs = [(i, i + 1) for i in range(n_frag - 1)] + [(i, i + 2) for i in range(n_frag - 2)] + [(0, n_frag - 2), (1, n_frag - 1)]
    X = [np.linalg.inv(gt[t]) @ gt[s] @ R.random_pose(rng, noise, noise) for s, t in pairs[:-2]] + [R.random_pose(rng, 1.0, 1.0)] * 2
    return clouds, np.stack(gt), pairs, np.stack(X).astype(np.float32)


def case_multiway(dev, a):
    rng = np.random.default_rng(1)
    clouds, gt, pairs, X = fragments(rng, 12, 1.2, 0.4, 90000, 0.01)
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(int).tolist()
    src, tgt = [p[0] for p in pairs], [p[1] for p in pairs]
    Xd, gtd = torch.from_numpy(X).to(dev), torch.from_numpy(gt).to(dev)
    lines = [f"multiway_registration: 12 fragments of {min(map(len, clouds))}..{max(map(len, clouds))} rows, {len(pairs)} pairs (2 false)"]
    for icp in (False, True):
        run = lambda: gmf_amd.multiway_registration(pts, off, src, tgt, Xd, use_icp=icp)      # noqa: E731
        out = run()
        ate = float(gmf_amd.absolute_trajectory_error(gtd, out["poses"]))
        t = timed(run, a.repeats, 1, warmup=1)
        lines.append(fmt(f"use_icp={icp} (ATE {ate:.2f} cm, {int(out['kept'].sum())} edges kept)", t))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["info_keypoints", "info_full", "optimise_57", "optimise_256", "multiway"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multiway_ab: needs a HIP device")
    dev = torch.device("cuda:0")
    if a.case == "info_keypoints":
        lines = case_info(dev, 57, 20000, 1596, a)
    elif a.case == "info_full":
        lines = case_info(dev, 29, 100000, 400, a)
    elif a.case == "optimise_57":
        lines = case_optimise(dev, 57, 270, 30, a, True)
    elif a.case == "optimise_256":
        lines = case_optimise(dev, 256, 1900, 100, a, False)
    else:
        lines = case_multiway(dev, a)
    gmf_amd.check_status()
    text = "\n".join([f"[{a.case}]  us per call: median [min, max] over {a.repeats} windows"] + lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
