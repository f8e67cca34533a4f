"""Writes tests/golden/sm_baseline.npz: what the reference's own spectral-matching baseline `SM`
(GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:19-53) returns on the CPU for two synthetic pairs.

The module around `SM` imports open3d, tqdm and the datasets, none of which `SM` uses.  Only the function's own AST node is
compiled, in a namespace holding `torch` and the reference's `rigid_transform_3d` (models/common.py, loaded by path with its
`utils.SE3`).  Per case the file keeps `labels`, `trans`, the generator's arguments instead of the inputs, and `eig`.  The function
does not return its eigenvector, so `rigid_transform_3d` is wrapped to record the weights it is handed: `eig * labels` in the run
proper, and the eigenvector itself in a second run with top_ratio = 1, where every row is labelled.  Run on a machine that has the reference
checkout; the tests read only the .npz.

Usage: python tests/tools/make_sm_golden.py REFERENCE_ROOT"""
import argparse
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from gmf_amd import synthetic  # noqa: E402

CASES = {"3dmatch": dict(seed=1, N=257, kind="3dmatch", inlier_threshold=0.10, top_ratio=0.1),
         "kitti": dict(seed=1, N=257, kind="kitti", inlier_threshold=0.6, top_ratio=0.05)}


def load_by_path(name, path, package=None):
    if package and package not in sys.modules:
        sys.modules[package] = types.ModuleType(package)       # (the package's own __init__ is not run)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_sm(reference_root):
    dsc = os.path.join(reference_root, "GMF_PointDSC")
    load_by_path("utils.SE3", os.path.join(dsc, "utils", "SE3.py"), "utils")
    common = load_by_path("models.common", os.path.join(dsc, "models", "common.py"), "models")
    path = os.path.join(dsc, "baseline_scripts", "baseline_3DMatch.py")
    tree = ast.parse(open(path).read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "SM")
    captured = {}

    def spy(A, B, weights=None, weight_threshold=0):
        captured["weights"] = weights.clone()
        return common.rigid_transform_3d(A, B, weights, weight_threshold)
    ns = {"torch": torch, "rigid_transform_3d": spy}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["SM"], captured


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_root")
    args = ap.parse_args()
    SM, captured = reference_sm(args.reference_root)
    out = {}
    for name, c in CASES.items():
        p = synthetic.synthetic_pair(c["seed"], c["N"], c["kind"])
        corr, src, tgt = (torch.from_numpy(p[k])[None] for k in ("corr_pos", "src_keypts", "tgt_keypts"))
        before = [x.clone() for x in (corr, src, tgt)]
        a = types.SimpleNamespace(inlier_threshold=c["inlier_threshold"])
        trans, labels = SM(corr, src, tgt, a, top_ratio=c["top_ratio"])
        w = captured["weights"]                                  # leading_eig * pred_labels, as handed to rigid_transform_3d
        SM(corr, src, tgt, a, top_ratio=1.0)                     # every row labelled: the weights are the eigenvector
        eig = captured["weights"]
        assert all(torch.equal(x, y) for x, y in zip(before, (corr, src, tgt)))
        assert torch.equal(w, eig * labels)
        out[name + "_eig"] = eig[0].numpy().astype(np.float32)
        out[name + "_labels"] = labels[0].numpy().astype(np.float32)
        out[name + "_trans"] = trans[0].numpy().astype(np.float32)
        out[name + "_args"] = np.array([c["seed"], c["N"], c["inlier_threshold"], c["top_ratio"]], np.float64)
        print(name, "k =", int(labels.sum()), "max eig =", float(eig.max()))
    path = os.path.join(ROOT, "tests", "golden", "sm_baseline.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
