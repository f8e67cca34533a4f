"""Train-mode image encoder, forward + backward: the native HIP pass (ImageEncoder.native_train = True) against the stock
torch modules (MIOpen convolutions, torch autograd) alternating in one process, warm; median and spread of repeated timed
loops.  Sizes: 2 images (one pair) and 32 images (the 16-pair step) of 120 x 160, p and q as separate calls as the training
step makes them; then the whole PointDSC training step from raw images at 16 pairs x 1000 correspondences, both ways.
GPU box:  python tools/image_train_ab.py [--no-step] [--loops 7] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmf_amd                                     # noqa: E402
from gmf_amd import synthetic                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
ap.add_argument("--loops", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    """Median and (min, max) in ms over `loops` timed loops of `reps` calls, after three warm-up calls."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(args.loops):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / args.reps * 1e3)
    return statistics.median(out), min(out), max(out)


def report(what, res):
    (mn, lon, hin), (ms, los, his) = res[True], res[False]
    print(f"{what}: native {mn:.3f} ms [{lon:.3f}, {hin:.3f}]   stock {ms:.3f} ms [{los:.3f}, {his:.3f}]   native / stock {mn / ms:.2f}")


enc = gmf_amd.ImageEncoder()
enc.load_state_dict(synthetic.seeded_state_dict({k: tuple(v.shape) for k, v in enc.state_dict().items()}, seed=4242, gain=1.0))
enc = enc.to(dev).train()
for n_images in (2, 32):
    half = n_images // 2
    p, q = torch.rand(half, 3, 120, 160, device=dev), torch.rand(half, 3, 120, 160, device=dev)

    def fwd_bwd():
        enc.zero_grad(set_to_none=True)
        (enc(p).sum() + enc(q).square().sum()).backward()
    res = {}
    for rnd in range(2):                           # alternate; keep the second round (both warm)
        for native in (True, False):
            enc.native_train = native
            res[native] = timed(fwd_bwd)
    report(f"encoder forward + backward, {n_images} images of 120 x 160 (p and q apart)", res)

if not args.no_step:
    B, N = 16, 1000
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7)
    model = gmf_amd.PointDSC(num_layers=12)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).train()
    b = synthetic.synthetic_batch(list(range(400, 400 + B)), N=N, T=40)
    data = {k: b[k].to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["p_image"], data["q_image"] = torch.rand(B, 3, 120, 160, device=dev), torch.rand(B, 3, 120, 160, device=dev)
    gt = b["gt_labels"].to(dev)
    cls_loss, sm_loss = gmf_amd.ClassificationLoss(balanced=False), gmf_amd.SpectralMatchingLoss(balanced=False)

    def step():
        model.zero_grad(set_to_none=True)
        r = model(data)
        (cls_loss(r["final_labels"], gt)["loss"] + sm_loss(r["M"], gt)).backward()
    res = {}
    for rnd in range(2):
        for native in (True, False):
            model.encoder.image_encoder.native_train = native
            res[native] = timed(step)
    report(f"PointDSC training step from raw images, {B} pairs x {N}", res)
