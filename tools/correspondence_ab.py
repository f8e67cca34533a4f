"""Times the correspondence chain against what a caller had without it.

Per shape, arms that alternate window by window in one process:
  mutual             gmf_amd.nn_match_mutual: one two-sided sweep
  two calls          nn_match(Fs, Ft) then nn_match(Ft, Fs) per pair - the form a user has today (for the batch: a loop over the pairs)
  two batched        the same two sweeps as two batched mode-0 calls of the existing kernel (the batch only; no public name today)
  build              the whole gmf_amd.build_correspondences (mutual filter, labels, gathers, and its one device-to-host copy)
  two calls again, two batched again    the same code a second time: the spread between two runs of the same code
Shapes: one pair 5000 x 5000 x 32, and 32 ragged pairs with sizes ~ U[4000, 5500] at d = 32.

Every window is `--inner` calls between two device events, ended by a synchronise; after a warm-up, the median with min and max
over `--repeats` windows, in us per call.  Fails without a GPU.  With --trace (for a profiler run of its own) every arm runs a few
times and nothing is timed.

Usage: python tools/correspondence_ab.py [--repeats 15] [--inner 10] [--out FILE] [--trace]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import matching         # noqa: E402


def alternated(arms, repeats, inner, warmup=3):
    """arms: {name: fn} -> {name: (median, min, max)} in us per call, from device events."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def case(dev, len_batch, d, seed):
    g = torch.Generator().manual_seed(seed)
    n0, n1 = sum(a for a, _ in len_batch), sum(b for _, b in len_batch)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(dev)      # noqa: E731
    Fs, Ft = unit(n0), unit(n1)
    Ps, Pt = (torch.rand(n0, 3, generator=g) * 4).to(dev), (torch.rand(n1, 3, generator=g) * 4).to(dev)
    T = torch.eye(4).repeat(len(len_batch), 1, 1).to(dev)
    return Fs, Ft, Ps, Pt, T


def arms_of(dev, len_batch, d, seed):
    Fs, Ft, Ps, Pt, T = case(dev, len_batch, d, seed)
    swapped = [(b, a) for a, b in len_batch]
    o0 = np.r_[0, np.cumsum([a for a, _ in len_batch])]
    o1 = np.r_[0, np.cumsum([b for _, b in len_batch])]
    views = [(Fs[o0[b]:o0[b + 1]], Ft[o1[b]:o1[b + 1]]) for b in range(len(len_batch))]

    def two_calls():
        for s, t in views:
            gmf_amd.nn_match(s, t)
            gmf_amd.nn_match(t, s)

    def two_batched():
        matching._match_batched(Fs, Ft, len_batch, 0, False, "ab")
        matching._match_batched(Ft, Fs, swapped, 0, False, "ab")

    arms = {"mutual": lambda: gmf_amd.nn_match_mutual(Fs, Ft, len_batch), "two calls": two_calls}
    if len(len_batch) > 1:
        arms["two batched"] = two_batched
    arms["build"] = lambda: gmf_amd.build_correspondences(Ps, Pt, Fs, Ft, len_batch, True, T, 0.1)
    arms["two calls again"] = two_calls
    if len(len_batch) > 1:
        arms["two batched again"] = two_batched
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("correspondence_ab: needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    shapes = {"1 pair 5000 x 5000 x 32": [(5000, 5000)],
              "32 pairs ~U[4000, 5500] x 32": [(int(rng.integers(4000, 5501)), int(rng.integers(4000, 5501))) for _ in range(32)]}
    lines = []
    for name, len_batch in shapes.items():
        arms = arms_of(dev, len_batch, 32, 1)
        if a.trace:
            for fn in arms.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            continue
        res = alternated(arms, a.repeats, a.inner)
        lines.append(f"{name}  (us per call: median [min, max] over {a.repeats} windows of {a.inner} calls)")
        for k, (med, lo, hi) in res.items():
            lines.append(f"  {k:18s} {med:9.1f}  [{lo:9.1f}, {hi:9.1f}]")
    gmf_amd.check_status()
    text = "\n".join(lines)
    print(text)
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
