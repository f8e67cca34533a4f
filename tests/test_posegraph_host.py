"""Host-side tests of multiway registration (no GPU): the float64 restatement (tests/posegraph_reference.py) against closed forms,
planted false loop closures and the rejected-step case; the measured order-of-summation floor behind the device tests'
tolerances; the C surface; the argument errors of the Python entry points; and the host plans of csrc/posegraph_plan.hpp as a
program of its own under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import posegraph_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against closed forms -------------------------------------------------------------------------------------

def test_two_node_graph_stops_at_once():
    g = R.two_node_graph()
    P, l, kept, st = R.run(g, **R.REFERENCE_OPTIONS)
    for p in st["passes"]:
        assert (p["iterations"], p["rejected"], p["stop"]) == (0, 0, R.STOP_RIGHT_TERM)
    assert np.array_equal(P, g["poses0"]) and kept.tolist() == [True] and l.tolist() == [1.0]


def test_noise_free_graph_returns_the_ground_truth():
    g = R.planted_graph(0, noise=0.0, n_false=0)
    # start away from the solution: the odometry chain perturbed
    rng = np.random.default_rng(1)
    g["poses0"] = np.stack([g["gt"][0]] + [T @ R.random_pose(rng, 0.02, 0.02) for T in g["gt"][1:]])
    # (the default criteria stop at a relative 1e-6; tightened, the quadratic convergence goes to rounding)
    tight = dict(min_relative_increment=1e-13, min_relative_residual_increment=1e-13, min_right_term=1e-10, min_residual=1e-24)
    P, l, kept, st = R.run(g, criteria=tight, **R.REFERENCE_OPTIONS)
    assert kept.all()
    for k in range(len(g["src"])):
        rel = np.linalg.inv(P[g["tgt"][k]]) @ P[g["src"][k]]
        assert np.abs(rel - g["X"][k]).max() < 1e-7, k
    assert np.abs(P - g["gt"]).max() < 1e-7                  # node 0 is the reference and gt[0] = I


def test_operators_invert_each_other():
    rng = np.random.default_rng(2)
    for _ in range(20):
        v = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-2, 2, 3)])
        assert np.abs(R.vec(R.mat(v)) - v).max() < 1e-14
        T = R.mat(v)
        assert np.abs(R.rigid_mul(T, R.rigid_inv(T)) - np.eye(4)).max() < 1e-15
    # lin picks the generators' coefficients
    for i in range(6):
        e = np.zeros(6)
        e[i] = 1e-8
        assert np.abs(R.lin(R.mat(e)) - e).max() < 1e-15


def test_analytic_jacobian_equals_central_difference():
    rng = np.random.default_rng(3)
    X, Ps, Pt = (R.random_pose(rng, 1.0, 1.0) for _ in range(3))
    A, _ = R.edge_A_zeta(X, Pt, Ps)
    J = R.edge_jacobian(A, Ps)
    # J_s by the definition, column i = lin(X^-1 Pt^-1 G_i Ps), with generic 4 x 4 products
    gen = np.zeros((6, 4, 4))
    gen[0, 1, 2], gen[0, 2, 1] = -1, 1
    gen[1, 0, 2], gen[1, 2, 0] = 1, -1
    gen[2, 0, 1], gen[2, 1, 0] = -1, 1
    for i in range(3):
        gen[3 + i, i, 3] = 1
    for i in range(6):
        assert np.abs(J[:, i] - R.lin(np.linalg.inv(X) @ np.linalg.inv(Pt) @ gen[i] @ Ps)).max() < 1e-14
    # and the derivative of zeta along exp(h G_i) P_s (source) and exp(h G_i) P_t (target: J_t = -J_s at zeta = 0 only to first
    # order, so the check of J_t uses a measurement that the poses satisfy)
    h = 1e-6

    def zeta(ps, pt, x):
        return R.edge_A_zeta(x, pt, ps)[1]

    def expm(i, s):
        e = np.zeros(6)
        e[i] = s
        return R.mat(e)

    for i in range(6):
        num = (zeta(expm(i, h) @ Ps, Pt, X) - zeta(expm(i, -h) @ Ps, Pt, X)) / (2 * h)
        assert np.abs(num - J[:, i]).max() < 1e-8, i
    X0 = np.linalg.inv(Pt) @ Ps
    A0, z0 = R.edge_A_zeta(X0, Pt, Ps)
    assert np.abs(z0).max() < 1e-15
    J0 = R.edge_jacobian(A0, Ps)
    for i in range(6):
        num = (zeta(Ps, expm(i, h) @ Pt, X0) - zeta(Ps, expm(i, -h) @ Pt, X0)) / (2 * h)
        assert np.abs(num + J0[:, i]).max() < 1e-8, i


def test_ldl_solve_against_numpy():
    rng = np.random.default_rng(4)
    for n in (1, 5, 18, 72):
        B = rng.standard_normal((n, n))
        A = B @ B.T + n * np.eye(n)
        b = rng.standard_normal(n)
        assert np.abs(R.ldl_solve(A, b) - np.linalg.solve(A, b)).max() < 1e-12
    assert R.ldl_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2)) is None        # second pivot 1 - 4 < 0


# ---- 2. planted false loop closures ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,noise", R.PLANTED_SEEDS + ((3, 0.002), (4, 0.05)))
def test_planted_false_closures_are_exactly_what_is_pruned(seed, noise):
    g = R.planted_graph(seed, noise=noise)
    assert g["planted"].sum() == 4 and (g["unc"] & ~g["planted"]).sum() == 10
    P, l, kept, st = R.run(g, **R.REFERENCE_OPTIONS)
    assert np.array_equal(~kept, g["planted"])
    l1 = st["passes"][0]["line_process"]
    true = g["unc"] & ~g["planted"]
    assert l1[true].min() >= (0.98 if noise < 0.01 else 0.75) and l1[g["planted"]].max() <= 0.14
    assert st["passes"][0]["rejected"] == 0 and 2 <= st["passes"][0]["iterations"] <= 6
    # the optimised trajectory is nearer the truth than the odometry chain it started from
    assert R.absolute_trajectory_error(g["gt"], P) <= R.absolute_trajectory_error(g["gt"], g["poses0"]) + 1e-9


def test_only_loop_closure_is_pruned():
    g = R.chain_with_one_false_closure()
    P, l, kept, st = R.run(g, **R.REFERENCE_OPTIONS)
    assert np.array_equal(~kept, g["planted"]) and st["passes"][1]["edges"] == len(g["src"]) - 1


def test_masked_edge_equals_deleted_edge():
    graphs = R.test_graphs()
    g, opt, mask = graphs["masked"]
    a = R.run(g, edge_mask=mask, **opt)
    b = R.run(graphs["deleted"][0], **opt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][mask], b[1]) and np.array_equal(a[2][mask], b[2])
    assert not a[2][~mask].any() and (a[1][~mask] == 0).all()


@pytest.mark.parametrize("ref", [0, 5, -1])
def test_reference_node_keeps_its_bits(ref):
    g = R.planted_graph(0)
    P, _, _, _ = R.run(g, **dict(R.REFERENCE_OPTIONS, reference_node=ref))
    if ref >= 0:
        assert P[ref].tobytes() == g["poses0"][ref].tobytes()
    else:
        assert np.abs(P - g["poses0"]).max() > 0


# ---- 3. the rejected-step branch -------------------------------------------------------------------------------------------------

def test_rejected_steps_take_the_same_decisions_in_either_edge_order():
    g = R.hard_graph(R.HARD_SEED)
    m = len(g["src"])
    a = R.run(g, **R.REFERENCE_OPTIONS)
    b = R.run(g, order=np.arange(m)[::-1], **R.REFERENCE_OPTIONS)
    p = a[3]["passes"][0]
    assert p["rejected"] >= 5 and p["solves"] <= 40, p
    assert a[3]["decisions"] == b[3]["decisions"] and 0 in a[3]["decisions"] and 1 in a[3]["decisions"]
    assert [q["stop"] for q in a[3]["passes"]] == [q["stop"] for q in b[3]["passes"]]


# ---- 4. the measured floor behind the device tests' tolerances --------------------------------------------------------------------

# python tests/posegraph_reference.py  (the restatement on every test graph with the edges as given and reversed)
FLOOR = dict(poses=1.399e-14, line_process=1.665e-15, residual=2.075e-12)


def test_order_floor_is_what_the_device_tolerances_were_taken_from(capsys):
    f = R.order_floor()
    for k, v in f.items():
        assert v <= FLOOR[k] * 1.0005, (k, v)                # the constants are the printed figures, rounded to four digits


# ---- 5. information matrix restatement ------------------------------------------------------------------------------------------

def test_information_terms_are_G_transpose_G():
    rng = np.random.default_rng(6)
    q = rng.uniform(-2, 2, (7, 3)).astype(np.float32)
    t = R.info_terms(q, np.arange(7))
    for i in range(7):
        x, y, z = q[i].astype(np.float64)
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]])
        assert np.abs(t[i] - G.T @ G).max() < 1e-15
    info, bound = R.info_from_nn(q, np.array([0, -1, 3, 3]))
    assert np.array_equal(info[3:, 3:], 3 * np.eye(3)) and info[5, 5] == 3 and (bound >= 0).all()


def test_brute_force_search_by_hand():
    tgt = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [5, 5, 5]], np.float32)
    p = R.transform_rows_f32(np.eye(4), np.array([[0.9, 0, 0], [0.4, 0, 0], [3, 3, 3]], np.float32))
    assert R.nn_brute_f32(p, tgt, 0.5).tolist() == [1, 0, -1]                       # equal rows: the smaller index; far: none
    assert R.nn_brute_f32(p, tgt, 0.1).tolist() == [-1, -1, -1]                     # d^2 = tau^2 is outside (0.1f^2 vs 0.1f^2)


# ---- 6. the rest of the layer -----------------------------------------------------------------------------------------------------

def test_layer_restatements():
    rng = np.random.default_rng(7)
    X = np.stack([R.random_pose(rng, 0.5, 1.0) for _ in range(4)])
    P = R.odometry_poses(X)
    assert np.array_equal(P[0], np.eye(4))
    for i in range(4):
        assert np.abs(np.linalg.inv(P[i + 1]) @ P[i] - X[i]).max() < 1e-13           # X_i = P_{i+1}^-1 P_i
    gt = np.stack([R.random_pose(rng, 1.0, 2.0) for _ in range(9)])
    M = R.random_pose(rng, 1.0, 3.0)
    assert R.absolute_trajectory_error(gt, M @ gt) < 1e-10
    off = gt.copy()
    off[::2, 0, 3] += 0.02                                                           # alternate nodes 2 cm off along x
    ate = R.absolute_trajectory_error(gt, off)
    assert 0.5 < ate < 2.0 / np.sqrt(2) + 1e-9
    info = np.zeros((3, 6, 6))
    info[:, 5, 5] = [30, 29, 80]
    T = np.stack([R.random_pose(rng, 0.1, 0.1), R.random_pose(rng, 0.1, 0.1), np.eye(4)])
    assert R.loop_closure_mask(info, np.array([100, 100, 100]), np.array([200, 100, 100]), T).tolist() == [True, False, False]


# ---- 7. the C surface --------------------------------------------------------------------------------------------------------------

NAMES = ("gmf_information_matrix", "gmf_posegraph_optimize")


def test_prototypes_signatures_exports_and_version():
    from gmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert re.search(r"#define\s+GMF_ABI_VERSION\s+5\b", header)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name           # one ctypes entry per C parameter
    lib = _lib.load_library()
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5
    import ctypes
    assert ctypes.sizeof(_lib.PoseGraphOptions) == 3 * 4 + 4 + 6 * 8                      # three ints, padding, six doubles


def test_c_entries_refuse_null_and_negative_arguments_without_a_device():
    """The checks come before anything touches the device: a null handle or pointer and a negative count return the
    invalid-argument code (the library is loaded, no handle is created)."""
    import ctypes
    from gmf_amd import _lib
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    bad_arg = int(re.search(r"GMF_ERR_BAD_ARG\s*=?\s*(-?\d+)", header).group(1))
    off = (ctypes.c_int * 2)(0, 4)
    e = (ctypes.c_int * 1)(0)
    assert lib.gmf_information_matrix(None, None, off, 1, e, e, 1, None, 0.1, None, None, None, None) == bad_arg
    assert lib.gmf_posegraph_optimize(None, None, off, off, 1, e, e, None, None, None, None, None, None, None, None, None, None,
                                      None) == bad_arg


# ---- 8. argument errors come first, then "no CPU fallback" -----------------------------------------------------------------------

def test_argument_errors_before_the_device_check():
    import gmf_amd
    pts = torch.zeros(10, 3)
    T = torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match="cloud_offsets must increase strictly"):
        gmf_amd.information_matrix_batched(pts, [0, 4, 4, 10], [0], [1], T, 0.1)
    with pytest.raises(RuntimeError, match="outside 0..1"):
        gmf_amd.information_matrix_batched(pts, [0, 4, 10], [0], [2], T, 0.1)
    with pytest.raises(RuntimeError, match=r"\[2, 4, 4\]"):
        gmf_amd.information_matrix_batched(pts, [0, 4, 10], [0, 1], [1, 0], T, 0.1)
    with pytest.raises(RuntimeError, match="must be > 0"):
        gmf_amd.information_matrix_batched(pts, [0, 4, 10], [0], [1], T, 0.0)
    poses = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    info = torch.eye(6, dtype=torch.float64)[None]
    unc = torch.zeros(1, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="joins node 1 to itself"):
        gmf_amd.global_optimization(poses, [1], [1], T, info, unc)
    with pytest.raises(RuntimeError, match="outside its graph"):
        gmf_amd.global_optimization(poses, [0], [3], T, info, unc)
    with pytest.raises(RuntimeError, match="unknown criterion"):
        gmf_amd.global_optimization(poses, [0], [1], T, info, unc, criteria={"max_iter": 3})
    with pytest.raises(RuntimeError, match="both node_offsets and edge_offsets"):
        gmf_amd.global_optimization(poses, [0], [1], T, info, unc, node_offsets=[0, 3])
    with pytest.raises(NotImplementedError, match="at most 256 nodes"):
        gmf_amd.global_optimization(torch.eye(4, dtype=torch.float64).repeat(257, 1, 1), [0], [1], T, info, unc)
    with pytest.raises(RuntimeError, match="consecutive pair"):
        gmf_amd.multiway_registration(pts, [0, 3, 6, 10], [0, 0], [1, 2], T.repeat(2, 1, 1))


def test_valid_cpu_inputs_have_no_fallback():
    import gmf_amd
    pts = torch.zeros(10, 3)
    T = torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.information_matrix_batched(pts, [0, 4, 10], [0], [1], T, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.global_optimization(torch.eye(4, dtype=torch.float64).repeat(2, 1, 1), [0], [1], T, torch.eye(6, dtype=torch.float64)[None],
                                    torch.zeros(1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gmf_amd.multiway_registration(pts, [0, 4, 10], [0], [1], T)


# ---- 9. the host plans under the host sanitizers ------------------------------------------------------------------------------------

def test_host_plans_under_sanitizers(tmp_path):
    """tests/abi_cpp/posegraph_plan_host.cpp, a program of its own built with the host compiler and
    -fsanitize=address,undefined: the chunk table and the per-node edge lists of csrc/posegraph_plan.hpp into exactly sized
    malloc'ed arrays."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "posegraph_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "posegraph_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "posegraph_plan_host: ok" in run.stdout, (run.stdout + run.stderr)[-2000:]
