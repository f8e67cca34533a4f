"""CPU-side checks of ICP's grid search (`search=` of gmf_amd/solvers.py, gmf_icp_point_to_point_ex): the C ABI entry, the
keyword's argument checks, the no-device error, and the float64 kd-tree's view of the case that tests/test_gpu_icp_grid.py
compares against the tree."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_declares_icp_ex():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    name = "gmf_icp_point_to_point_ex"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.load_library(), name)
    # the brute-force entry's arguments, then total_tgt (long long), search (int) and the stream
    old, new = _lib.SIGNATURES["gmf_icp_point_to_point"], _lib.SIGNATURES[name]
    assert new[0] is old[0] and new[1][:len(old[1]) - 1] == old[1][:-1] and len(new[1]) == len(old[1]) + 2
    assert "#define GMF_ABI_VERSION 5" in text           # an added entry point: the version stays


def test_search_argument_checks():
    import gmf_amd
    s, t, T0 = torch.rand(2, 16, 3), torch.rand(2, 20, 3), torch.eye(4).repeat(2, 1, 1)
    for bad in ("kd", "", "GRID", 1, None, b"grid"):
        with pytest.raises(RuntimeError, match="icp_point_to_point_batched: search must be"):
            gmf_amd.icp_point_to_point_batched(s, t, T0, 0.1, search=bad)
        with pytest.raises(RuntimeError, match="registration_icp: search must be"):
            gmf_amd.registration_icp(s[0], t[0], 0.1, search=bad)
    # the other checks still run under either value
    for search in ("brute", "grid"):
        with pytest.raises(RuntimeError, match="max_iteration"):
            gmf_amd.icp_point_to_point_batched(s, t, T0, 0.1, max_iteration=-1, search=search)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_cpu_tensors_fail_loudly():
    import gmf_amd
    p = torch.rand(2, 16, 3)
    for search in ("brute", "grid"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmf_amd.icp_point_to_point_batched(p, p, torch.eye(4).repeat(2, 1, 1), 0.1, search=search)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmf_amd.registration_icp(p[0], p[1], 0.1, search=search)


_U64 = np.uint64


def _mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def cell_hash_np(b, c):
    """csrc/grid_hash.hpp's cell_hash for integer cells c [..., 3] of pair b."""
    x, y, z = (c[..., k].astype(np.int64).astype(np.uint64) for k in range(3))
    with np.errstate(over="ignore"):
        k = _mix64(x * _U64(0x9E3779B97F4A7C15) ^ (_U64(b) << _U64(40)))
        k = _mix64(k ^ y * _U64(0xC2B2AE3D27D4EB4F))
        return _mix64(k ^ z * _U64(0x165667B19E3779F9))


def test_three_target_scene_meets_collisions():
    """The scene of test_gpu_icp_grid.test_three_targets, seen through a restatement of the grid: 3 targets give the smallest
    table (64 slots).  Some query reaches one slot through two of its 27 cells, and some query visits a slot that lists a
    target of a cell outside its 27 - the two cases the kernel's pair test and minimum must absorb."""
    import test_gpu_icp_grid as G
    src, tgt = G.three_target_scene()
    T = 64
    while T < 2 * len(tgt):
        T *= 2
    assert T == 64
    inv_h = 1.0 / (float(np.float32(G.THREE_TAU)) * (1.0 + 1.0 / 1024))
    cell = lambda p: np.floor(p.astype(np.float64) * inv_h).astype(np.int64)        # noqa: E731  (T0 = identity: p = the source row)
    off = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(27, 3)
    qc = cell(src)[:, None, :] + off[None]                                             # [Ns, 27, 3]
    qs = (cell_hash_np(0, qc) & _U64(T - 1)).astype(np.int64)                        # [Ns, 27]
    tc = cell(tgt)
    ts = (cell_hash_np(0, tc) & _U64(T - 1)).astype(np.int64)
    twice = np.array([len(np.unique(r)) < 27 for r in qs])
    assert twice.mean() > 0.5
    far = np.zeros(len(src), bool)
    for j in range(len(tgt)):
        in_slot = (qs == ts[j]).any(1)
        in_cells = (qc == tc[j]).all(2).any(1)
        far |= in_slot & ~in_cells
    assert far.sum() >= 10


def test_kdtree_case_stays_clear_of_tau():
    """The kd-tree test skips the rows whose nearest distance lies within 1e-5 tau of tau (there fp32 and float64 may disagree
    about d < tau); it is a test of the search only while that share is small.  Checked here with the float64 tree alone."""
    import test_gpu_icp_grid as G
    *_, tau, P, Q, d, j = G.kd_case()
    band = np.abs(d - tau) <= G.KD_BAND * tau
    assert band.mean() < 0.01
    assert 0.05 < (d < tau).mean() < 0.95                # both outcomes occur
    assert len(d) == G.KD_NS and len(Q) == G.KD_NT
