"""CPU-side checks of point-to-plane ICP (gmf_amd.icp_point_to_plane_batched, gmf_icp_point_to_plane): the C surface, the
argument errors of the Python entry points, the launch plan of the split step as a program of its own under the host sanitizers,
and the float64 restatement (tests/icp_plane_reference.py) on its own scene - convergence, sign flips, the degenerate plane and
its stability under one-ulp perturbations.  tests/test_gpu_icp_plane.py compares the device against the restatement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import icp_plane_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the C surface -------------------------------------------------------------------------------------------------------------------

def test_c_abi_declares_icp_point_to_plane():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    name = "gmf_icp_point_to_plane"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.load_library(), name)
    # gmf_icp_point_to_point_ex's arguments with the normals after the targets
    old, new = _lib.SIGNATURES["gmf_icp_point_to_point_ex"], _lib.SIGNATURES[name]
    assert new[0] is old[0] and new[1] == old[1][:4] + [old[1][3]] + old[1][4:]
    assert "#define GMF_ABI_VERSION 5" in text           # an added entry point: the version stays


def test_python_rows_constant_is_the_plan_headers():
    from gmf_amd import solvers
    text = open(os.path.join(ROOT, "gmf_amd", "csrc", "icp_plane_plan.hpp")).read()
    m = re.search(r"constexpr int kIcpPlaneRows = (\d+);", text)
    assert m and int(m.group(1)) == solvers.ICP_PLANE_ROWS
    assert solvers.ICP_PLANE_ROWS % 256 == 0              # whole sweeps of the 256-thread workgroup


def test_exported():
    import gmf_amd
    assert "icp_point_to_plane_batched" in gmf_amd.__all__ and callable(gmf_amd.icp_point_to_plane_batched)


# ---- 2. argument errors -----------------------------------------------------------------------------------------------------------------

def test_batched_normals_checks():
    import gmf_amd
    s, t, T0 = torch.rand(2, 16, 3), torch.rand(2, 20, 3), torch.eye(4).repeat(2, 1, 1)
    n = torch.rand(2, 20, 3)
    bad = [n.double(), n.half(), n[:, :19], n[:1], n.reshape(40, 3), n.numpy(), None, torch.rand(2, 20, 4)]
    for x in bad:
        with pytest.raises(RuntimeError, match=r"icp_point_to_plane_batched: target_normals must be a float32 tensor of target's shape \(2, 20, 3\)"):
            gmf_amd.icp_point_to_plane_batched(s, t, x, T0, 0.1)
    with pytest.raises(RuntimeError, match="icp_point_to_plane_batched: target_normals must live on target's device"):
        gmf_amd.icp_point_to_plane_batched(s, t, n.to("meta"), T0, 0.1)
    # ragged: the packed shape
    sp, tp = s.reshape(-1, 3), t.reshape(-1, 3)
    with pytest.raises(RuntimeError, match=r"target_normals must be a float32 tensor of target's shape \(40, 3\)"):
        gmf_amd.icp_point_to_plane_batched(sp, tp, n, T0, 0.1, [0, 16, 32], [0, 20, 40])
    # the point-to-point form's checks run under the new name, in its order
    with pytest.raises(RuntimeError, match="icp_point_to_plane_batched: search must be"):
        gmf_amd.icp_point_to_plane_batched(s, t, n.double(), T0, 0.1, search="kd")
    with pytest.raises(RuntimeError, match="icp_point_to_plane_batched: `target` must be float32"):
        gmf_amd.icp_point_to_plane_batched(s, t.double(), n, T0, 0.1)
    with pytest.raises(RuntimeError, match="icp_point_to_plane_batched: init must be a float32"):
        gmf_amd.icp_point_to_plane_batched(s, t, n, T0[0], 0.1)
    with pytest.raises(RuntimeError, match="icp_point_to_plane_batched: max_iteration must be"):
        gmf_amd.icp_point_to_plane_batched(s, t, n, T0, 0.1, max_iteration=-1)
    with pytest.raises(RuntimeError, match="icp_point_to_plane_batched: max_correspondence_distance must be"):
        gmf_amd.icp_point_to_plane_batched(s, t, n, T0, 0.0)


BAD_ESTIMATION = ("plane", "", "POINT_TO_PLANE", 1, None, b"point_to_plane")


def test_registration_icp_estimation_checks():
    import gmf_amd
    s, t, n = torch.rand(16, 3), torch.rand(20, 3), torch.rand(20, 3)
    for bad in BAD_ESTIMATION:
        with pytest.raises(RuntimeError, match='registration_icp: estimation must be "point_to_point" or "point_to_plane"'):
            gmf_amd.registration_icp(s, t, 0.1, estimation=bad, target_normals=n)
    with pytest.raises(RuntimeError, match='registration_icp: estimation="point_to_plane" needs target_normals'):
        gmf_amd.registration_icp(s, t, 0.1, estimation="point_to_plane")
    with pytest.raises(RuntimeError, match="registration_icp: target_normals must be a tensor or a NumPy array"):
        gmf_amd.registration_icp(s, t, 0.1, estimation="point_to_plane", target_normals=[[0, 0, 1]] * 20)
    # `search` is still looked at first
    with pytest.raises(RuntimeError, match="registration_icp: search must be"):
        gmf_amd.registration_icp(s, t, 0.1, search="kd", estimation="plane")


def test_refinement_estimation_checks():
    import gmf_amd
    pts, off = torch.rand(40, 3), [0, 20, 40]
    T = torch.eye(4).repeat(1, 1, 1)
    for bad in BAD_ESTIMATION:
        with pytest.raises(RuntimeError, match='local_refinement_batched: estimation must be "point_to_point" or "point_to_plane"'):
            gmf_amd.local_refinement_batched(pts, off, [0], [1], T, estimation=bad)
        with pytest.raises(RuntimeError, match='multiway_registration: icp_estimation must be "point_to_point" or "point_to_plane"'):
            gmf_amd.multiway_registration(pts, off, [0], [1], T, icp_estimation=bad)
    # the checks recorded before it still come first
    with pytest.raises(RuntimeError, match="voxel_size and max_iter must have the same"):
        gmf_amd.local_refinement_batched(pts, off, [0], [1], T, voxel_size=(0.05,), max_iter=(1, 2), estimation="plane")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_cpu_tensors_fail_loudly():
    import gmf_amd
    p, n = torch.rand(2, 16, 3), torch.rand(2, 16, 3)
    for search in ("brute", "grid"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmf_amd.icp_point_to_plane_batched(p, p, n, torch.eye(4).repeat(2, 1, 1), 0.1, search=search)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmf_amd.registration_icp(p[0], p[1], 0.1, search=search, estimation="point_to_plane", target_normals=n[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.local_refinement_batched(p.reshape(-1, 3), [0, 16, 32], [0], [1], torch.eye(4)[None], estimation="point_to_plane")


# ---- 3. the launch plan under the host sanitizers ---------------------------------------------------------------------------------------

def test_plan_under_sanitizers(tmp_path):
    """tests/abi_cpp/icp_plane_plan_host.cpp, a program of its own built with the host compiler and
    -fsanitize=address,undefined: the parts of csrc/icp_plane_plan.hpp tile every pair's rows, each (pair, part) owns a slot inside
    the exactly sized scratch, and a grid that does not fit one launch is refused."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "icp_plane_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "icp_plane_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "icp_plane_plan_host: ok" in run.stdout, (run.stdout + run.stderr)[-2000:]


# ---- 4. the restatement on the corner scene ---------------------------------------------------------------------------------------------

_RUNS = {}


def reference_run(name):
    """The scene of case `name` and the restatement's result on it, computed once."""
    if name not in _RUNS:
        Nt, Ns, noise = R.CASES[name]
        src, tgt, nrm, Tg = R.corner(1, Nt, Ns, noise)
        _RUNS[name] = (src, tgt, nrm, Tg, R.icp_plane_np(src, tgt, nrm, np.eye(4), R.TAU))
    return _RUNS[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_converges_to_the_ground_truth(name):
    src, tgt, nrm, Tg, (T, fit, rm, it, nn) = reference_run(name)
    noise = R.CASES[name][2]
    assert 2 <= it <= 6, it                               # a fraction of point-to-point's passes
    assert fit > 0.99
    assert R.rotation_error_deg(T, Tg) < 0.1 and np.linalg.norm(T[:3, 3] - Tg[:3, 3]) < 0.01
    if noise == 0:
        assert rm < 1e-6 and np.abs(T - Tg).max() < 1e-5
    else:
        assert 0.5 * noise < rm < 3 * noise               # what is left is the targets' noise
    assert (nn >= 0).sum() == round(fit * len(src))


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_sign_flips_change_no_bit(name):
    src, tgt, nrm, _, (T, fit, rm, it, nn) = reference_run(name)
    flip = np.where(np.random.default_rng(3).random((len(nrm), 1)) < 0.5, np.float32(-1), np.float32(1))
    T2, fit2, rm2, it2, nn2 = R.icp_plane_np(src, tgt, nrm * flip, np.eye(4), R.TAU)
    assert np.array_equal(T, T2) and fit == fit2 and rm == rm2 and it == it2 and np.array_equal(nn, nn2)


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_degenerate_plane_returns_init(name):
    src, tgt, nrm, _, _ = reference_run(name)
    flat = np.zeros_like(nrm)
    flat[:, 2] = 1.0
    A, b = R.normal_equations(src, tgt[:len(src)], flat[:len(src)])
    assert (np.diag(A)[2:5] == 0).all() and R.ldlt_solve(A, b) is None      # three diagonal entries exactly 0
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.02, 0.005]
    T, _, _, it, _ = R.icp_plane_np(src, tgt, flat, T0, R.TAU)
    assert np.array_equal(T, T0) and it == 1


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_is_stable(name):
    """Four runs with every coordinate of the points and the normals moved one fp32 ulp at random: T moves by less than 1e-5, a
    tenth of the gate the device is held to, and the pass count stays."""
    src, tgt, nrm, _, (T, _, _, it, _) = reference_run(name)
    r = np.random.default_rng([5, len(src)])
    for _ in range(4):
        Tp, _, _, itp, _ = R.icp_plane_np(R.one_ulp(src, r), R.one_ulp(tgt, r), R.one_ulp(nrm, r), np.eye(4), R.TAU)
        assert np.abs(Tp - T).max() < 1e-5, np.abs(Tp - T).max()
        assert itp == it


def test_ldlt_solves_and_rejects():
    r = np.random.default_rng(8)
    M = r.normal(size=(40, 6))
    A, b = M.T @ M, r.normal(size=6)
    assert np.allclose(R.ldlt_solve(A, b), np.linalg.solve(A, -b), rtol=1e-10, atol=1e-12)
    A2 = A.copy()
    A2[3, :] = A2[:, 3] = 0.0                             # a zero row and column: pivot 3 is 0
    assert R.ldlt_solve(A2, b) is None
    A3 = A.copy()
    A3[0, 0] = np.nan
    assert R.ldlt_solve(A3, b) is None
    # a pivot just below and just above the threshold 2^-40 A_kk
    D = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    L = np.eye(6)
    L[5, 0] = 1.0
    for scale, ok in ((0.5, False), (2.0, True)):
        Dd = D.copy()
        Dd[5, 5] = scale * 2.0 ** -40                      # A_55 = 1 + d_5: d_5 against 2^-40 (1 + d_5)
        assert (R.ldlt_solve(L @ Dd @ L.T, b) is not None) == ok


def test_vector6_matches_open3d_order():
    x = np.array([0.3, -0.2, 0.5, 1.0, 2.0, 3.0])
    Rx, Ry, Rz = R.rotation([1, 0, 0], np.degrees(x[0])), R.rotation([0, 1, 0], np.degrees(x[1])), R.rotation([0, 0, 1], np.degrees(x[2]))
    T = R.vector6_to_matrix(x)
    assert np.allclose(T[:3, :3], Rz @ Ry @ Rx, atol=1e-15) and T[:3, 3].tolist() == [1.0, 2.0, 3.0] and T[3].tolist() == [0, 0, 0, 1]
