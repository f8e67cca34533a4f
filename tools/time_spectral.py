"""Times the spectral-matching baseline (gmf_amd/spectral.py) against the reference's own form written in torch on the same GPU.

  shapes      B = 1 at N = 1000 / 5000 / 10 000 (the reference's SM takes one pair) and 32 x 5000
  matrix-free gmf_amd.spectral_matching_batched: one call for the whole batch
  dense       the reference's arithmetic in torch: the [N, N, 6] difference, the dense M, ten bmm, argsort; the pose left out (it
              is the same 3 x 3 problem either way).  At 32 x 5000 pair by pair, as the reference runs it.
  accuracy    max |eig - eig64| / max eig64 of both against the dense form in float64 on the GPU (N <= 5000)

Device events around each call after warm-up, the forms alternated call by call; median, min and max over repeats, in us.
Usage: python tools/time_spectral.py [--repeats 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                       # noqa: E402
from gmf_amd import synthetic        # noqa: E402

THR, RATIO = 0.10, 0.1


def timed_alternating(fns, repeats, warmup=3):
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
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def dense_eig(corr, dtype=torch.float32, iterations=10):
    """The dense form for one pair, corr [1,N,6] -> (eig [1,N], labels [1,N]): the reference's arithmetic, step by step."""
    c = corr[0].to(dtype)
    diff = c[:, None, :] - c[None, :, :]                                     # [N,N,6], as the reference forms it
    d = diff[..., :3].square().sum(-1).sqrt() - diff[..., 3:].square().sum(-1).sqrt()
    del diff
    sigma = THR / 3
    M = (4.5 - d.square() / 2 / sigma ** 2).clamp_min(0)
    M.fill_diagonal_(0)
    M = M[None]
    v = torch.ones((1, c.shape[0], 1), device=c.device, dtype=dtype)
    for _ in range(iterations):
        v = torch.bmm(M, v)
        v = v / (v.norm(dim=1, keepdim=True) + 1e-6)
    v = v[..., 0]
    order = torch.argsort(v, dim=1, descending=True)
    labels = torch.zeros_like(v)
    labels[0, order[0, :int(v.shape[1] * RATIO)]] = 1
    return v, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_spectral.py needs a HIP device: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, N in ((1, 1000), (1, 5000), (1, 10000), (32, 5000)):
        pairs = [synthetic.synthetic_pair(100 + b, N, "3dmatch") for b in range(B)]
        corr, src, tgt = (torch.stack([torch.from_numpy(p[k]) for p in pairs]).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
        def ours():
            return gmf_amd.spectral_matching_batched(corr, src, tgt, THR, top_ratio=RATIO, return_eigenvector=True)

        def dense():
            return [dense_eig(corr[b:b + 1]) for b in range(B)]

        res = timed_alternating([ours, dense], args.repeats)
        say(f"{B} x {N}: matrix-free {res[0][0]:9.1f} us ({res[0][1]:.1f} .. {res[0][2]:.1f}) | dense torch {res[1][0]:9.1f} us "
            f"({res[1][1]:.1f} .. {res[1][2]:.1f}) | dense / matrix-free {res[1][0] / res[0][0]:.2f}")
        if N <= 5000:
            e64 = dense_eig(corr[0:1], torch.float64)[0][0]
            errs = [float(((x.double() - e64).abs().max() / e64.max()).cpu()) for x in (ours()[2][0], dense_eig(corr[0:1])[0][0])]
            say(f"{B} x {N}: eig error against float64  matrix-free {errs[0]:.3e}  dense fp32 {errs[1]:.3e}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
