"""Times the training path of DGR's inlier network (gmf_amd.train.resunet_train, D = 6, 'ones' features, pe = True, 1 200 tokens
per image) on the 6-D correspondences of the 3DMatch demo fragments (tools/time_sparse.py: demo_coords).

Reports, with device events after warm-up (median, min, max over repeats): the eval forward, the train-mode forward, and forward +
backward of a scalar loss; then, per convolution of the network on its own plan, the forward (`sparse_conv`), the weight gradient
(`sparse_conv_wgrad`) and the data gradient (`sparse_conv_dgrad`) with the weight gradient's rate of useful work (2 x pairs x
Cin x Cout).

Usage: python tools/time_sparse_train.py [--repeats 10] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmf_amd                       # noqa: E402
from gmf_amd import sparse as SP     # noqa: E402
from gmf_amd import train as T       # noqa: E402
from time_sparse import CONVS, DEV, demo_coords, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    coords = demo_coords()
    M = coords.shape[0]
    model = gmf_amd.ResUNetBN2C(in_channels=1, out_channels=1, D=6, pe=True).to(DEV)
    feats = torch.ones(M, 1, device=DEV)
    tok = [torch.randn(1, 1200, 128, device=DEV) for _ in range(2)]
    plan = SP.SparsePlan(coords, 4, SP._NET_MAPS)
    say(f"demo pair: M = {M}, level counts {plan.counts.tolist()}")

    def eval_fwd():
        with torch.no_grad():
            model.eval()(coords, feats, p_tokens=tok[0], q_tokens=tok[1])

    def train_fwd():
        model.train()
        T.resunet_train(model, coords, feats, p_tokens=tok[0], q_tokens=tok[1])

    def train_step():
        model.train()
        model.zero_grad(set_to_none=True)
        T.resunet_train(model, coords, feats, p_tokens=tok[0], q_tokens=tok[1]).sum().backward()

    for name, fn in (("eval forward", eval_fwd), ("train forward", train_fwd), ("train forward + backward", train_step)):
        md, lo, hi = timed(fn, a.repeats)
        say(f"{name:28s} {md / 1e3:8.2f} ms  (min {lo / 1e3:.2f}, max {hi / 1e3:.2f})")

    n = plan.counts.tolist()
    params = dict(model.named_parameters())
    say("per convolution (us): forward / dW / dx, dW TFLOP/s (2 x pairs x Cin x Cout)")
    tot = [0.0, 0.0, 0.0]
    for li, m, lvl, name in CONVS:
        W = params[name + ".kernel"].detach()
        W3 = W if W.dim() == 3 else W.unsqueeze(0)
        K, cin, cout = W3.shape
        in_lvl = lvl if m is None else SP._NET_MAPS[m][2]
        x = torch.randn(M, cin, device=DEV)
        dy = torch.randn(M, cout, device=DEV)
        nsplit = SP.layer_nsplit(K, cin, cout)
        f = timed(lambda: SP.sparse_conv(plan, m, lvl, x, W3, nsplit=nsplit), a.repeats)[0]
        w = timed(lambda: SP.sparse_conv_wgrad(plan, m, lvl, x, dy), a.repeats)[0]
        d = timed(lambda: SP.sparse_conv_dgrad(plan, m, lvl, dy, W3), a.repeats)[0] if name != "conv1" else 0.0
        pairs = n[lvl] if m is None else int(plan.kernel_map(m)[0][n[lvl]])
        tf = 2.0 * pairs * cin * cout / (w * 1e-6) / 1e12
        tot = [tot[0] + f, tot[1] + w, tot[2] + d]
        say(f"  {name:16s} K {K:4d} {cin:3d}->{cout:3d} lvl {in_lvl}->{lvl} pairs {pairs:7d}  {f:8.1f} / {w:8.1f} / {d:8.1f}  "
            f"{tf:6.2f}")
    say(f"  sum              forward {tot[0] / 1e3:.2f} ms, dW {tot[1] / 1e3:.2f} ms, dx {tot[2] / 1e3:.2f} ms")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
