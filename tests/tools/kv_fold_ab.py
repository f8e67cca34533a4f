"""A/B of builds / knob settings of libgmf_hip.so on bench.py's workload (32 pairs x 5000 correspondences, T = 196, the whole test-mode
forward) in ONE GPU job: every arm is a fresh child process, arms alternating, three rounds (the pool's devices differ by ~2 %, so only
numbers of one job compare).  Per arm and round one JSON line: the step time (mean of 4 x 10 forwards after 5 warm-up forwards, and the
four runs), the attention time per launch (gmf_profile_*), and a hash of the logits, poses and labels of the seeded batch - two arms
that compute the same bits print the same hash.

    python tests/tools/kv_fold_ab.py PARENT/libgmf_hip.so live live:kv_fold=0 [--rounds 3]
    python tests/tools/kv_fold_ab.py --outputs      # the folded against the unfolded results on that batch (profiles/kv_fold_outputs.txt)
ARM = LIB[:knob=value,...]; LIB is a path to another build of the library, or `live` for gmf_amd/libgmf_hip.so.
(`profiles/kv_fold_ab_rounds.txt`: the parent commit's build against the build that introduced "kv_fold".)"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(arm):
    import torch
    sys.path.insert(0, ROOT)
    import gmf_amd
    from gmf_amd import _lib, synthetic
    lib, _, knobs = arm.partition(":")
    if lib != "live":
        _lib.LIB_PATH = os.path.abspath(lib)
    dev = torch.device("cuda:0")
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7, sigma_d=0.10)
    model = gmf_amd.PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                             sigma_d=0.10, k=40, nms_radius=0.10)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    h = _lib.handle_for(0)
    for kv in [k for k in knobs.split(",") if k]:
        name, value = kv.split("=")
        h.call("gmf_set_tuning", name.encode(), int(value))
    b = synthetic.synthetic_batch(list(range(32)), N=5000, T=196)
    data = {k: b[k].to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")}
    data["testing"] = True
    for _ in range(5):
        res = model(data)
    torch.cuda.synchronize()
    steps = []
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(10):
            res = model(data)
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - t0) / 10 * 1e3)
    h.call("gmf_profile_enable", 1)
    for _ in range(5):
        model(data)
    torch.cuda.synchronize()
    ms, n = C.c_double(), C.c_int()
    h.call("gmf_profile_read", C.byref(ms), C.byref(n))
    h.call("gmf_profile_enable", 0)
    dig = hashlib.sha256(model.last_logits.cpu().numpy().tobytes() + res["final_trans"].cpu().numpy().tobytes()
                         + res["final_labels"].cpu().numpy().tobytes()).hexdigest()[:16]
    print(json.dumps({"arm": arm, "step_ms_mean": round(sum(steps) / len(steps), 4), "step_ms_runs": [round(s, 4) for s in steps],
                      "attention_ms_per_launch": round(ms.value / max(n.value, 1), 4), "launches": n.value, "outputs_sha": dig}), flush=True)


def outputs():
    """the seeded batch with "kv_fold" = 0 and 1 in one process: deviation of logits, poses and labels, and pair 0 against the fp32 oracle"""
    import torch
    sys.path.insert(0, ROOT)
    import gmf_amd
    from gmf_amd import _lib, synthetic
    from oracle import gmf_oracle as O
    dev = torch.device("cuda:0")
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7, sigma_d=0.10)
    model = gmf_amd.PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                             sigma_d=0.10, k=40, nms_radius=0.10)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    h = _lib.handle_for(0)
    b = synthetic.synthetic_batch(list(range(32)), N=5000, T=196)
    data = {k: b[k].to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")}
    data["testing"] = True
    out = {}
    for kv in (0, 1):
        h.call("gmf_set_tuning", b"kv_fold", kv)
        r = model(data)
        torch.cuda.synchronize()
        out[kv] = (model.last_logits.clone(), r["final_trans"].clone(), r["final_labels"].clone())
    h.call("gmf_set_tuning", b"kv_fold", 1)
    dl = (out[0][0] - out[1][0]).abs()
    print(f"32 x 5000, kv_fold 1 vs 0: max|dlogit| {float(dl.max()):.3e} mean {float(dl.mean()):.3e}, "
          f"max|dT| {float((out[0][1] - out[1][1]).abs().max()):.3e}, labels differing {int((out[0][2] != out[1][2]).sum())} of "
          f"{out[0][2].numel()}, logit signs differing {int(((out[0][0] > 0) != (out[1][0] > 0)).sum())}")
    ref = O.pointdsc_forward(sd, {k: v[:1] for k, v in b.items()}, testing=True)
    for kv in (0, 1):
        print(f"pair 0 vs fp32 oracle, kv_fold {kv}: logits {float((out[kv][0][:1].cpu() - ref['logits']).abs().max()):.3e}, "
              f"pose {float((out[kv][1][:1].cpu() - ref['final_trans']).abs().max()):.3e}")


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    if args and args[0] == "--outputs":
        return outputs()
    rounds = 3
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    for rnd in range(rounds):
        for arm in args:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm], capture_output=True, text=True)
            line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else "(no output) " + out.stderr[-400:]
            print(f"[round {rnd}] {line}", flush=True)
            if out.returncode != 0:          # a child that failed: nothing more is started on the device
                sys.exit(out.returncode)


if __name__ == "__main__":
    main()
