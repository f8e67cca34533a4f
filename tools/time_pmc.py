"""Times the maximum-clique baseline (gmf_amd/clique.py) and records how far its search went.

  shapes   1 x 1000, 1 x 5000 and 32 x 1000, 3DMatch-shape (synthetic_pair(100 + b, N, "3dmatch"), threshold 0.10), both metrics
  time     gmf_amd.max_clique_batched: one call for the whole batch
  steps    branch-and-bound nodes expanded per pair: the largest over the batch and over the repeats (the count depends on when
           the waves see each other's incumbent, so it varies from run to run; the result does not), and `exact`

Device events around each call after warm-up; median, min and max over repeats, in us.  There is nothing to compare the times
with: they are recorded, not gated.  The default budget of the library is 64 x the largest step count at N = 1000 printed here.
Usage: python tools/time_pmc.py [--repeats 10] [--warmup 2] [--max-steps K] [--shapes 1x1000,32x1000] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import synthetic        # noqa: E402

THR = 0.10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--shapes", default="1x1000,1x5000,32x1000", help="B x N, comma-separated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pmc.py needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, N in (tuple(int(x) for x in sh.split("x")) for sh in args.shapes.split(",")):
        pairs = [synthetic.synthetic_pair(100 + b, N, "3dmatch") for b in range(B)]
        corr, src, tgt = (torch.stack([torch.from_numpy(p[k]) for p in pairs]).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
        for metric in ("squared", "length"):
            def run():
                return gmf_amd.max_clique_batched(corr, src, tgt, THR, metric=metric, max_steps=args.max_steps, return_info=True)

            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            ts, steps, exact = [], 0, 1
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = run()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
                steps = max(steps, int(out[4].max()))
                exact = min(exact, int(out[3].min()))
            size, degree = out[2], out[5]
            say(f"{B} x {N} {metric:8s}: {statistics.median(ts):11.1f} us ({min(ts):.1f} .. {max(ts):.1f}) | steps <= {steps} | "
                f"exact {exact} | clique {int(size.min())} .. {int(size.max())} | edges {int(degree.sum()) // 2 // B} per pair")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
