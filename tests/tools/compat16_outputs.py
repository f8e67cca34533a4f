"""What the guarded 16-bit compat cache ("compat_16" = 1, the default) does to the results, on the GPU box:

    python tests/tools/compat16_outputs.py                 # bench.py's seeded batch (32 x 5000, T = 196): "compat_16" 1 against 0 -
                                                           # logits, poses, labels, logit signs; pair 0 against the fp32 oracle
    python tests/tools/compat16_outputs.py --fold-parent   # the constant of tests/test_gpu_compat16.py::test_fold_and_no_fold: max
                                                           # |logit(kv_fold 1) - logit(kv_fold 0)| on the fp32 cache ("compat_16" = 0: the
                                                           # parent build's code and bits) over 8 seeded pairs of each size of that file
(profiles/compat16_outputs.txt holds both.)  The timing A/B is tests/tools/kv_fold_ab.py PARENT/libgmf_hip.so live live:compat_16=0."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gmf_amd                                   # noqa: E402
from gmf_amd import _lib, synthetic              # noqa: E402
from oracle import gmf_oracle as O               # noqa: E402

dev = torch.device("cuda:0")
KEYS = ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")


def make_model(sd):
    m = gmf_amd.PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                         sigma_d=0.10, k=40, nms_radius=0.10)
    m.load_state_dict(sd, strict=False)
    return m.to(dev).eval()


def outputs():
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7, sigma_d=0.10)
    model, h = make_model(sd), _lib.handle_for(0)
    b = synthetic.synthetic_batch(list(range(32)), N=5000, T=196)
    data = {k: b[k].to(dev) for k in KEYS}
    data["testing"] = True
    out = {}
    try:
        for kv in (0, 1):
            h.call("gmf_set_tuning", b"compat_16", kv)
            h.status(clear=True)
            r = model(data)
            torch.cuda.synchronize()
            out[kv] = (model.last_logits.clone(), r["final_trans"].clone(), r["final_labels"].clone(), bool(h.status() & _lib.GMF_STATUS_PV_GUARDED))
    finally:
        h.call("gmf_set_tuning", b"compat_16", 1)
    dl = (out[0][0] - out[1][0]).abs()
    print(f"32 x 5000, compat_16 1 vs 0: max|dlogit| {float(dl.max()):.3e} mean {float(dl.mean()):.3e}, "
          f"max|dT| {float((out[0][1] - out[1][1]).abs().max()):.3e}, labels differing {int((out[0][2] != out[1][2]).sum())} of "
          f"{out[0][2].numel()}, logit signs differing {int(((out[0][0] > 0) != (out[1][0] > 0)).sum())}, guard bit {out[1][3]}")
    ref = O.pointdsc_forward(sd, {k: v[:1] for k, v in b.items()}, testing=True)
    for kv in (0, 1):
        print(f"pair 0 vs fp32 oracle, compat_16 {kv}: logits {float((out[kv][0][:1].cpu() - ref['logits']).abs().max()):.3e}, "
              f"pose {float((out[kv][1][:1].cpu() - ref['final_trans']).abs().max()):.3e}")


def fold_parent():
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7)
    model, h = make_model(sd), _lib.handle_for(0)
    force = dict(small_grid_roles=0, small_prologue_roles=0, attn_key_splits=1, ff_hidden_splits=1, compat_16=0)
    back = dict(small_grid_roles=1, small_prologue_roles=1, attn_key_splits=0, ff_hidden_splits=0, compat_16=1, kv_fold=1)
    worst = 0.0
    try:
        for k, v in force.items():
            h.call("gmf_set_tuning", k.encode(), v)
        for n in (95, 128, 333, 700):
            pairs = [synthetic.synthetic_batch([3000 + i], N=n, T=196) for i in range(8)]
            rag = {k: [p[k][0].to(dev) for p in pairs] for k in ("corr_pos", "src_keypts", "tgt_keypts")}
            rag.update(p_tokens=torch.cat([p["p_tokens"] for p in pairs]).to(dev), q_tokens=torch.cat([p["q_tokens"] for p in pairs]).to(dev),
                       testing=True)
            lg = {}
            for fold in (0, 1):
                h.call("gmf_set_tuning", b"kv_fold", fold)
                model(rag)
                torch.cuda.synchronize()
                lg[fold] = model.last_logits.clone()
            d = float((lg[0] - lg[1]).abs().max())
            worst = max(worst, d)
            print(f"fp32 cache, N = {n} x 8 pairs: max |logit(kv_fold 1) - logit(kv_fold 0)| {d:.3e}")
    finally:
        for k, v in back.items():
            h.call("gmf_set_tuning", k.encode(), v)
    print(f"PARENT_FOLD_DIFF = {worst:.3e}")


if __name__ == "__main__":
    fold_parent() if "--fold-parent" in sys.argv[1:] else outputs()
