"""Host-side tests of the correspondence chain (no GPU): the float64 restatement on hand-made cases, the C surface (header,
ctypes signatures, exported symbols, ABI version), the argument errors of the Python entry points, and the chunk plan of
csrc/corr_plan.hpp as a program of its own under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import correspondence_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement on 4 x 3 cases worked by hand ---------------------------------------------------------------------------------

E = np.eye(3)


def test_reference_mutual_by_hand():
    # targets: the three axes.  Source 0 = e0, 1 = close to e0 (less so), 2 = e1, 3 = between e1 and e2 but nearer e2
    T = E.copy()
    S = np.array([[1, 0, 0], [0.9, 0.1, 0], [0, 1, 0], [0, 0.6, 0.8]], float)
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    si, ti = R.argmin_both(S, T)
    assert si.tolist() == [0, 0, 1, 2]
    assert ti.tolist() == [0, 2, 3]
    assert R.mutual_mask(si, ti).tolist() == [True, False, True, True]


def test_reference_ties_take_the_first_index():
    # target 2 repeats target 0; source 1 repeats source 0 (= target 0)
    T = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0]], float)
    S = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    si, ti = R.argmin_both(S, T, exact_ties=True)
    assert si.tolist() == [0, 0, 1, 0]                  # rows 0, 1: keys 0 and 2 tie -> 0; row 3: all dots 0 -> 0
    assert ti.tolist() == [0, 2, 0]                     # keys 0, 2: sources 0 and 1 tie -> 0
    assert R.mutual_mask(si, ti).tolist() == [True, False, True, False]     # nothing pairs with key 2; source 1 loses its tie


def test_reference_build_by_hand():
    T = E.copy()
    S = np.array([[1, 0, 0], [0.9, 0.1, 0], [0, 1, 0], [0, 0.6, 0.8]], float)
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    P = np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 2, 0]], np.float32)          # source keypoints
    Q = np.array([[1, 1, 1], [2, 1, 1.05], [5, 5, 5]], np.float32)                   # target keypoints
    G = np.eye(4)
    G[:3, 3] = 1.0                                                                   # x -> x + (1, 1, 1)
    r = R.build_pair(P, Q, S, T, True, G, 0.1)
    assert r["corr"].tolist() == [[0, 0], [2, 1], [3, 2]]
    assert r["src_keypts"].tolist() == P[[0, 2, 3]].tolist() and r["tgt_keypts"].tolist() == Q[[0, 1, 2]].tolist()
    # |(0,0,0)+1 - (1,1,1)| = 0; |(1,0,0)+1 - (2,1,1.05)| = 0.05; |(0,2,0)+1 - (5,5,5)| > 0.1
    assert r["gt_labels"].tolist() == [1.0, 1.0, 0.0]
    pos = np.concatenate([P[[0, 2, 3]], Q[[0, 1, 2]]], 1).astype(np.float64)
    assert np.array_equal(r["corr_pos"], pos - pos.mean(0))
    assert np.abs(r["corr_pos"].mean(0)).max() < 1e-15
    assert np.array_equal(R.build_pair(P, Q, S, T, True, None, None, in_dim=3)["corr_pos"], pos[:, :3] - pos[:, 3:])
    every = R.build_pair(P, Q, S, T, False, G, 0.1)
    assert every["corr"].tolist() == [[0, 0], [1, 0], [2, 1], [3, 2]] and every["gt_labels"].tolist() == [1.0, 0.0, 1.0, 0.0]


def test_reference_batch_offsets():
    rng = np.random.default_rng(0)
    lens = [(4, 3), (0, 2), (3, 5)]
    S, T = rng.standard_normal((7, 8)), rng.standard_normal((10, 8))
    P, Q = rng.standard_normal((7, 3)), rng.standard_normal((10, 3))
    pairs, off = R.build_batch(P, Q, S, T, lens)
    assert off.dtype == np.int32 and off[0] == 0 and len(off) == 4
    assert np.diff(off).tolist() == [len(p["corr"]) for p in pairs] and len(pairs[1]["corr"]) == 0
    one = R.build_pair(P[4:], Q[5:], S[4:], T[5:])
    assert np.array_equal(one["corr"], pairs[2]["corr"]) and np.array_equal(one["corr_pos"], pairs[2]["corr_pos"])


def test_fixture_preconditions_hold_at_the_fixed_seeds():
    """What the GPU tests assert again on the data they use: checked here too, where no GPU is needed."""
    for d in R.WIDTHS:
        gap, bound, margin = R.check_fixture(R.make_fixture(d, R.SEEDS[d]))
        assert gap > bound and margin > 1e-4, (d, gap, bound, margin)


# ---- 2. the C surface -----------------------------------------------------------------------------------------------------------------

NAMES = ("gmf_nn_match_mutual_batched", "gmf_build_correspondences")


def test_prototypes_signatures_exports_and_version():
    from gmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert re.search(r"#define\s+GMF_ABI_VERSION\s+5\b", header)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name           # one ctypes entry per C parameter
    lib = _lib.load_library()                                                              # every declared symbol resolves
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5


# ---- 3. argument errors come first, then "no CPU fallback" ---------------------------------------------------------------------------

def _cpu_inputs(ns=6, nt=5, d=32):
    return torch.zeros(ns, 3), torch.zeros(nt, 3), torch.zeros(ns, d), torch.zeros(nt, d)


def test_argument_errors_before_the_device_check():
    import gmf_amd
    P, Q, S, T = _cpu_inputs()
    with pytest.raises(RuntimeError, match="differ in width"):
        gmf_amd.nn_match_mutual(S, torch.zeros(5, 33))
    with pytest.raises(RuntimeError, match="differ in width"):
        gmf_amd.build_correspondences(P, Q, S, torch.zeros(5, 33))
    with pytest.raises(RuntimeError, match="len_batch sums to"):
        gmf_amd.nn_match_mutual(S, T, [(3, 5), (2, 0)])
    with pytest.raises(RuntimeError, match="len_batch sums to"):
        gmf_amd.build_correspondences(P, Q, S, T, [(6, 4)])
    with pytest.raises(RuntimeError, match="source rows and no target rows"):
        gmf_amd.build_correspondences(P, Q, S, T, [(3, 5), (3, 0)])
    with pytest.raises(RuntimeError, match="needs an inlier_threshold"):
        gmf_amd.build_correspondences(P, Q, S, T, gt_trans=torch.eye(4)[None])
    with pytest.raises(RuntimeError, match=r"gt_trans must be \[2, 4, 4\]"):
        gmf_amd.build_correspondences(P, Q, S, T, [(3, 2), (3, 3)], gt_trans=torch.eye(4)[None], inlier_threshold=0.1)
    with pytest.raises(RuntimeError, match=r"`src_keypts` must be \[6, 3\]"):
        gmf_amd.build_correspondences(P[:5], Q, S, T)
    with pytest.raises(NotImplementedError, match="in_dim 12"):
        gmf_amd.build_correspondences(P, Q, S, T, in_dim=12)


def test_valid_cpu_inputs_have_no_fallback():
    import gmf_amd
    P, Q, S, T = _cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.nn_match_mutual(S, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.nn_match_mutual(S, T, [(2, 1), (4, 4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.build_correspondences(P, Q, S, T, gt_trans=torch.eye(4), inlier_threshold=0.1, gather_desc=True)


# ---- 4. the chunk plan under the host sanitizers ---------------------------------------------------------------------------------------

def test_chunk_plan_under_sanitizers(tmp_path):
    """tests/abi_cpp/corr_plan_host.cpp, a program of its own built with the host compiler and -fsanitize=address,undefined: the
    chunk table of csrc/corr_plan.hpp into exactly sized malloc'ed arrays - the chunks tile every pair and never cross one."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "corr_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "corr_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "corr_plan_host: ok" in run.stdout, (run.stdout + run.stderr)[-2000:]
