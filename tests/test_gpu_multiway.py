"""GPU tests of multiway registration (gmf_amd/multiway.py, csrc/posegraph_kernels.hip): the information matrices, the pose-graph
optimiser and the Python layer, against the float64 NumPy restatement in tests/posegraph_reference.py.

Information matrices: `nn` is checked against a brute-force fp32 search and against ICP's own `nn`; the 36 numbers are checked
against an fp64 NumPy sum over the DEVICE's nn within the bound K 2^-52 sum |terms| that holds for a sum of K terms in any order,
so a search error cannot hide behind a summation tolerance.  An edge's numbers are the same bits alone, in a batch, in a permuted
batch and on a second call.

Optimiser: decisions (kept, iteration and rejection counts, stop codes) equal the restatement's; poses, line process and the
residual trace agree within 16 x the floor that the order of summation alone produces in the restatement (FLOOR below, measured
on the CPU by `python tests/posegraph_reference.py`: the restatement on every test graph with the edges as given and
reversed)."""
import functools

import numpy as np
import pytest
import torch

import gmf_amd
import posegraph_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = np.float32, np.float64

# python tests/posegraph_reference.py -> floor: poses 1.399e-14, line_process 1.665e-15, residual (relative to max(1, r)) 2.075e-12
FLOOR = dict(poses=1.399e-14, line_process=1.665e-15, residual=2.075e-12)
TOL = {k: 16 * v for k, v in FLOOR.items()}
CHUNK = 256                                                  # kInfoChunk of csrc/posegraph_plan.hpp


def _g(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# information matrices
# ---------------------------------------------------------------------------------------------------------------------------

TAU = 0.07


def _pose32(rng, rot=0.6, trans=1.0):
    """A pose whose entries are fp32 numbers (ICP takes an fp32 init; the information matrix takes the same numbers in fp64)."""
    return R.random_pose(rng, rot, trans).astype(F32).astype(F64)


def _source_for(rng, tgt, T, ns, frac=0.6):
    """ns source rows: about `frac` of them land within tau of a target row under T, the rest far away."""
    Ti = np.linalg.inv(T)
    j = rng.integers(0, len(tgt), ns)
    near = tgt[j].astype(F64) + rng.uniform(-0.02, 0.02, (ns, 3))
    far = rng.uniform(3.0, 6.0, (ns, 3))
    p = np.where((rng.random(ns) < frac)[:, None], near, far)
    return (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)


def _pack(clouds):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(int).tolist()
    return _g(np.concatenate(clouds).astype(F32)), off


def _info(pts, off, src, tgt, T, tau=TAU):
    info, count, nn = gmf_amd.information_matrix_batched(pts, off, src, tgt, _g(np.asarray(T, F64).reshape(-1, 4, 4)), tau, return_nn=True)
    torch.cuda.synchronize()
    rows = np.concatenate([[0], np.cumsum([off[s + 1] - off[s] for s in src])]).astype(int)
    nn = nn.cpu().numpy()
    return info.cpu().numpy(), count.cpu().numpy(), [nn[rows[e]:rows[e + 1]] for e in range(len(src))]


def _check_edge(clouds, s, t, T, info, count, nn, where):
    """One edge's outputs against the brute-force search, ICP's nn and the bounded fp64 sum over the device's nn."""
    src, tgt = clouds[s], clouds[t]
    want_nn = R.nn_brute_f32(R.transform_rows_f32(T, src), tgt, TAU)
    assert np.array_equal(nn, want_nn), where
    icp_nn = gmf_amd.icp_point_to_point_batched(_g(src)[None], _g(tgt)[None], _g(T.astype(F32))[None], TAU, max_iteration=0,
                                                search="grid")[4]
    assert np.array_equal(icp_nn.cpu().numpy()[0], nn), where
    want, bound = R.info_from_nn(tgt, nn)
    assert (np.abs(info - want) <= bound).all(), (where, np.abs(info - want).max(), bound.max())
    K = int((nn >= 0).sum())
    assert count == K and info[5, 5] == K and np.array_equal(info[3:, 3:], K * np.eye(3)), where
    assert np.array_equal(info, info.T), where


@functools.lru_cache(None)
def _size_cases():
    rng = np.random.default_rng(11)
    targets = [rng.uniform(-1, 1, (nt, 3)).astype(F32) for nt in (1, 200)]
    clouds, src, tgt, T = list(targets), [], [], []
    for ti in range(2):
        for ns in (1, 63, 64, 65, 257):
            Tk = _pose32(rng)
            clouds.append(_source_for(rng, targets[ti], Tk, ns))
            src.append(len(clouds) - 1); tgt.append(ti); T.append(Tk)
    return clouds, src, tgt, np.stack(T)


def test_information_matrix_sizes_alone_in_batch_permuted_and_again():
    clouds, src, tgt, T = _size_cases()
    pts, off = _pack(clouds)
    info, count, nn = _info(pts, off, src, tgt, T)
    E = len(src)
    assert sum(int(c) for c in count) > 300                  # the cases do match rows
    for e in range(E):
        _check_edge(clouds, src[e], tgt[e], T[e], info[e], count[e], nn[e], f"edge {e}")
        one = _info(pts, off, [src[e]], [tgt[e]], T[e:e + 1])
        assert one[0][0].tobytes() == info[e].tobytes() and one[1][0] == count[e] and np.array_equal(one[2][0], nn[e]), e
    perm = np.random.default_rng(12).permutation(E)
    p = _info(pts, off, [src[e] for e in perm], [tgt[e] for e in perm], T[perm])
    again = _info(pts, off, src, tgt, T)
    assert again[0].tobytes() == info.tobytes() and np.array_equal(again[1], count)
    for k, e in enumerate(perm):
        assert p[0][k].tobytes() == info[e].tobytes() and p[1][k] == count[e] and np.array_equal(p[2][k], nn[e]), e


def test_information_matrix_three_chunks():
    rng = np.random.default_rng(13)
    tgt = rng.uniform(-1, 1, (500, 3)).astype(F32)
    T = _pose32(rng)
    ns = 2 * CHUNK + 90
    src = _source_for(rng, tgt, T, ns, frac=0.7)
    pts, off = _pack([src, tgt])
    info, count, nn = _info(pts, off, [0], [1], T[None])
    hit = nn[0] >= 0
    # matched rows on both sides of both chunk edges, and in every chunk
    for edge in (CHUNK, 2 * CHUNK):
        assert hit[edge - 1] or hit[edge - 2], edge
        assert hit[edge] or hit[edge + 1], edge
    assert hit[:CHUNK].sum() > 100 and hit[CHUNK:2 * CHUNK].sum() > 100 and hit[2 * CHUNK:].sum() > 30
    _check_edge([src, tgt], 0, 1, T, info[0], count[0], nn[0], "three chunks")
    # the same edge after another edge: its chunks are counted from its own first row
    both = _info(pts, off, [1, 0], [1, 1], np.stack([np.eye(4), T]))
    assert both[0][1].tobytes() == info[0].tobytes() and np.array_equal(both[2][1], nn[0])


def test_information_matrix_shared_target_self_edge_far_edge_and_none():
    rng = np.random.default_rng(14)
    hub = rng.uniform(-1, 1, (300, 3)).astype(F32)
    Ta, Tb = _pose32(rng), _pose32(rng)
    a, b = _source_for(rng, hub, Ta, 130), _source_for(rng, hub, Tb, 77)
    clouds = [a, hub, b]
    far = np.eye(4)
    far[:3, 3] = 50.0
    # cloud 1 is the target of three edges (0, 1, 2); edge 2 is cloud 1 onto itself with T = I; edge 3 is far away; edge 4 turns
    # edge 0 round (the hub as the source)
    src, tgt = [0, 2, 1, 0, 1], [1, 1, 1, 2, 0]
    T = np.stack([Ta, Tb, np.eye(4), far, np.linalg.inv(Ta).astype(F32).astype(F64)])
    pts, off = _pack(clouds)
    info, count, nn = _info(pts, off, src, tgt, T)
    for e in range(5):
        _check_edge(clouds, src[e], tgt[e], T[e], info[e], count[e], nn[e], f"edge {e}")
    N = len(hub)
    assert count[2] == N and np.array_equal(nn[2], np.arange(N)) and np.array_equal(info[2][3:, 3:], N * np.eye(3))
    assert count[3] == 0 and not info[3].any() and (nn[3] == -1).all()
    assert count[0] > 40 and count[1] > 20 and count[4] > 40
    # a transformation that is not finite gives zeros
    bad = T.copy()
    bad[1, 0, 3] = np.nan
    i2, c2, n2 = _info(pts, off, src, tgt, bad)
    assert c2[1] == 0 and not i2[1].any() and (n2[1] == -1).all() and i2[0].tobytes() == info[0].tobytes()
    # no edges
    i0, c0 = gmf_amd.information_matrix_batched(pts, off, [], [], torch.zeros((0, 4, 4), device=DEV, dtype=torch.float64), TAU)
    assert tuple(i0.shape) == (0, 6, 6) and tuple(c0.shape) == (0,)
    gmf_amd.check_status()


# ---------------------------------------------------------------------------------------------------------------------------
# optimiser
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _reference(name):
    """The restatement's result on a test graph (computed once, shared)."""
    g, opt, mask = R.test_graphs()[name]
    return R.run(g, edge_mask=mask, **opt)


def _device(names, trace=True):
    """One call over the named test graphs (they share their options) -> per graph (poses, l, kept, stats dict of numpy)."""
    graphs = R.test_graphs()
    opt = graphs[names[0]][1]
    assert all(graphs[n][1] == opt for n in names)
    gs = [graphs[n][0] for n in names]
    masks = [graphs[n][2] if graphs[n][2] is not None else np.ones(len(graphs[n][0]["src"]), bool) for n in names]
    noff = np.concatenate([[0], np.cumsum([len(g["poses0"]) for g in gs])]).astype(int).tolist()
    eoff = np.concatenate([[0], np.cumsum([len(g["src"]) for g in gs])]).astype(int).tolist()
    cat = lambda k: np.concatenate([g[k] for g in gs])
    P, l, kept, st = gmf_amd.global_optimization(_g(cat("poses0"), torch.float64), cat("src"), cat("tgt"), _g(cat("X"), torch.float64),
                                                 _g(cat("info"), torch.float64), _g(cat("unc")), edge_mask=_g(np.concatenate(masks)),
                                                 node_offsets=noff, edge_offsets=eoff, trace=trace, **opt)
    torch.cuda.synchronize()
    P, l, kept = P.cpu().numpy(), l.cpu().numpy(), kept.cpu().numpy()
    st = {k: v.cpu().numpy() for k, v in st.items()}
    out = []
    for i in range(len(names)):
        out.append((P[noff[i]:noff[i + 1]], l[eoff[i]:eoff[i + 1]], kept[eoff[i]:eoff[i + 1]], {k: v[i] for k, v in st.items()}))
    return out


def _assert_matches_reference(name, got):
    P, l, kept, st = got
    rP, rl, rkept, rst = _reference(name)
    g, opt, _ = R.test_graphs()[name]
    assert np.array_equal(kept, rkept), name
    for p in range(2):
        want = rst["passes"][p]
        have = (int(st["iterations"][p]), int(st["rejected"][p]), int(st["stop"][p]), int(st["edges"][p]))
        assert have == (want["iterations"], want["rejected"], want["stop"], want["edges"]), (name, p, have, want)
    ref = opt["reference_node"]
    if ref >= 0:
        assert P[ref].tobytes() == g["poses0"][ref].tobytes(), name
    assert np.isfinite(P).all() and np.isfinite(l).all()
    dP, dl = np.abs(P - rP).max(), np.abs(l - rl).max()
    want_tr = R.trace_array(rst)
    tr = st["trace"]
    assert np.array_equal(np.isnan(tr), np.isnan(want_tr)), name
    ok = ~np.isnan(want_tr[:, :, 0])
    dr = (np.abs(tr[:, :, 0] - want_tr[:, :, 0])[ok] / np.maximum(1.0, np.abs(want_tr[:, :, 0][ok]))).max()
    dres = max(abs(st["residual"][p] - rst["passes"][p]["residual"]) / max(1.0, abs(rst["passes"][p]["residual"])) for p in range(2))
    print(f"{name}: max|dP| = {dP:.3e} (tol {TOL['poses']:.3e}), max|dl| = {dl:.3e} (tol {TOL['line_process']:.3e}), "
          f"max rel d(residual trace) = {dr:.3e} (tol {TOL['residual']:.3e})")
    assert dP <= TOL["poses"], (name, dP)
    assert dl <= TOL["line_process"], (name, dl)
    assert dr <= TOL["residual"] and dres <= TOL["residual"], (name, dr, dres)


@pytest.mark.parametrize("name", ["planted0", "planted1", "planted2", "ref5", "free", "two", "three", "only_closure_pruned", "hard",
                                  "masked"])
def test_optimiser_one_graph_against_the_restatement(name):
    got = _device([name])[0]
    _assert_matches_reference(name, got)
    if name == "only_closure_pruned":
        g = R.test_graphs()[name][0]
        assert np.array_equal(~got[2], g["planted"]) and got[2].sum() == len(g["src"]) - 1
    if name == "hard":
        assert got[3]["rejected"][0] >= 5
    if name.startswith("planted"):
        assert np.array_equal(~got[2], R.test_graphs()[name][0]["planted"])
    gmf_amd.check_status()


def test_optimiser_ragged_batch_masked_edge_and_bitwise_invariants():
    names = ["masked", "two", "planted2"]                    # n = 12 with two masked edges, n = 2, n = 12 with 0.05 noise
    batch = _device(names)
    for name, got in zip(names, batch):
        _assert_matches_reference(name, got)
    # a graph inside a batch equals the same graph alone, bit for bit
    for name, got in zip(names, batch):
        alone = _device([name])[0]
        assert alone[0].tobytes() == got[0].tobytes() and alone[1].tobytes() == got[1].tobytes(), name
        assert np.array_equal(alone[2], got[2]) and alone[3]["trace"].tobytes() == got[3]["trace"].tobytes(), name
    # in another place of the batch too
    again = _device(["three", "planted2", "masked"])
    assert again[2][0].tobytes() == batch[0][0].tobytes() and again[1][0].tobytes() == batch[2][0].tobytes()
    # the masked-edge graph equals the same graph with those edges deleted, bit for bit
    mask = R.test_graphs()["masked"][2]
    deleted = _device(["deleted"])[0]
    masked = batch[0]
    assert deleted[0].tobytes() == masked[0].tobytes()
    assert deleted[1].tobytes() == masked[1][mask].tobytes() and np.array_equal(deleted[2], masked[2][mask])
    assert not masked[2][~mask].any() and (masked[1][~mask] == 0).all()
    assert deleted[3]["trace"].tobytes() == masked[3]["trace"].tobytes()
    gmf_amd.check_status()


def test_optimiser_flags_a_bad_pivot():
    """An information matrix with a NaN: the first pivot of H + lambda I is not finite.  The pass stops with its own code, the
    poses stay and the handle's status word is set."""
    g = R.two_node_graph()
    P0 = g["poses0"].copy()
    P0[1] = P0[1] @ R.random_pose(np.random.default_rng(0), 0.1, 0.1)
    info = g["info"].copy()
    info[0, 0, 0] = np.nan
    P, l, kept, st = gmf_amd.global_optimization(_g(P0, torch.float64), g["src"], g["tgt"], _g(g["X"], torch.float64),
                                                 _g(info, torch.float64), _g(g["unc"]), reference_node=-1)
    torch.cuda.synchronize()
    assert st["stop"].cpu().numpy().tolist() == [[R.STOP_PIVOT, R.STOP_PIVOT]]
    assert st["iterations"].cpu().numpy().tolist() == [[1, 1]] and st["rejected"].cpu().numpy().tolist() == [[0, 0]]
    assert np.array_equal(P.cpu().numpy(), P0)
    with pytest.raises(RuntimeError, match="pivot"):
        gmf_amd.check_status()
    gmf_amd.check_status()                                   # the word was cleared


def test_c_abi_refuses_null_and_negative_arguments():
    import ctypes
    from gmf_amd._util import handle_and_stream
    h, st = handle_and_stream(torch.zeros(1, device=DEV))
    lib, bad = h.lib, -1
    off = (ctypes.c_int * 2)(0, 4)
    e = (ctypes.c_int * 1)(0)
    pts = torch.zeros((4, 3), device=DEV)
    assert lib.gmf_information_matrix(h.h, None, off, 1, e, e, 1, None, 0.1, None, None, None, st) == bad
    assert lib.gmf_information_matrix(h.h, pts.data_ptr(), off, 1, e, e, -1, None, 0.1, None, None, None, st) == bad
    assert lib.gmf_information_matrix(h.h, pts.data_ptr(), off, 0, e, e, 1, None, 0.1, None, None, None, st) == bad
    assert lib.gmf_information_matrix(h.h, pts.data_ptr(), off, 1, e, e, 1, None, -0.1, None, None, None, st) == bad
    assert lib.gmf_posegraph_optimize(h.h, None, off, off, 1, e, e, None, None, None, None, None, None, None, None, None, None, st) == bad
    poses = torch.eye(4, device=DEV, dtype=torch.float64).repeat(4, 1, 1)
    from gmf_amd import _lib
    opt = _lib.PoseGraphOptions(100, 20, -1, 1e-6, 1e-6, 1e-6, 1e-6, 0.25, 1.0)
    stats, res = torch.zeros(8, device=DEV, dtype=torch.int32), torch.zeros(2, device=DEV, dtype=torch.float64)
    assert lib.gmf_posegraph_optimize(h.h, poses.data_ptr(), off, (ctypes.c_int * 2)(0, 0), -1, e, e, None, None, None, None,
                                      ctypes.byref(opt), None, None, stats.data_ptr(), res.data_ptr(), None, st) == bad
    torch.cuda.synchronize()
    gmf_amd.check_status()


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------------

def test_layer_pieces_against_numpy():
    rng = np.random.default_rng(21)
    X = np.stack([R.random_pose(rng, 0.5, 1.0) for _ in range(5)])
    P = gmf_amd.odometry_poses(_g(X, torch.float64)).cpu().numpy()
    assert np.array_equal(P[0], np.eye(4)) and np.abs(P - R.odometry_poses(X)).max() < 1e-13
    info = np.zeros((4, 6, 6))
    info[:, 5, 5] = [30, 29, 80, 31]
    T = np.stack([R.random_pose(rng, 0.1, 0.1), R.random_pose(rng, 0.1, 0.1), np.eye(4), R.random_pose(rng, 0.1, 0.1)])
    ns, nt = [100, 100, 100, 200], [200, 100, 100, 100]
    m = gmf_amd.loop_closure_mask(_g(info, torch.float64), ns, nt, _g(T, torch.float64))
    assert m.is_cuda and m.dtype == torch.bool
    assert m.cpu().numpy().tolist() == R.loop_closure_mask(info, np.array(ns), np.array(nt), T).tolist() == [True, False, False, True]
    gt = np.stack([R.random_pose(rng, 1.0, 2.0) for _ in range(9)])
    M = R.random_pose(rng, 1.0, 3.0)
    moved = np.stack([M @ T for T in gt])
    # fp32 Kabsch over positions of size ~2: the closed form is 0, the fp32 solve leaves about 1e-6 m = 1e-4 cm
    assert float(gmf_amd.absolute_trajectory_error(_g(gt, torch.float64), _g(moved, torch.float64))) < 1e-3
    off = gt.copy()
    off[::2, 0, 3] += 0.02
    ate = float(gmf_amd.absolute_trajectory_error(_g(gt, torch.float64), _g(off, torch.float64)))
    assert abs(ate - R.absolute_trajectory_error(gt, off)) < 1e-3


def _scene(seed=31, n_frag=6, width=1.2, step=0.4, n_points=3000, noise=0.01):
    """Fragments cut with overlap from one random surface, each stored in its own frame.  -> clouds, gt poses (fragment ->
    world, pose 0 = I), pairs (source, target), their poses X = P_t^-1 P_s with small noise, and which pairs are false."""
    rng = np.random.default_rng(seed)
    length = step * (n_frag - 1) + width
    xy = rng.uniform([0, 0], [length, 1.0], (n_points, 2))
    z = 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(4.0 * xy[:, 1]) + 0.05 * np.sin(11.0 * xy[:, 0] + 2.0 * xy[:, 1])
    world = np.concatenate([xy, z[:, None]], 1)
    # a fragment's frame sits at the fragment's centre, turned at random (fragment 0: the world frame)
    gt = [np.eye(4)]
    for i in range(1, n_frag):
        T = R.random_pose(rng, 0.4, 0.1)
        T[:3, 3] += [step * i, 0.0, 0.0]
        gt.append(T)
    clouds = []
    for i in range(n_frag):
        w = world[(world[:, 0] >= step * i) & (world[:, 0] < step * i + width)]
        Pi = np.linalg.inv(gt[i])
        clouds.append((w @ Pi[:3, :3].T + Pi[:3, 3]).astype(F32))
    pairs = [(i, i + 1) for i in range(n_frag - 1)] + [(i, i + 2) for i in range(n_frag - 2)] + [(0, 4), (1, 5)]
    false = np.array([False] * (2 * n_frag - 3) + [True, True])
    X = []
    for (s, t), f in zip(pairs, false):
        X.append(R.random_pose(rng, 1.0, 1.0) if f else np.linalg.inv(gt[t]) @ gt[s] @ R.random_pose(rng, noise, noise))
    return clouds, np.stack(gt), pairs, np.stack(X).astype(F32), false


def test_multiway_registration_on_a_synthetic_scene():
    """Seed 31: with every pair pose carrying the same noise, whether the optimised trajectory beats the odometry chain is a
    matter of the draw; at this seed the restatement (with a float64 kd-tree for the information matrices) gives 0.556 cm for the
    chain and 0.507 cm after the optimisation.  With the ICP refinement the overlapping points are the same points and the
    trajectory is nearly exact whatever the draw."""
    clouds, gt, pairs, X, false = _scene()
    pts, off = _pack(clouds)
    src, tgt = [p[0] for p in pairs], [p[1] for p in pairs]
    gt_d = _g(gt, torch.float64)
    out = gmf_amd.multiway_registration(pts, off, src, tgt, _g(X), use_icp=False, refine_odometry=False)
    torch.cuda.synchronize()
    kept = out["kept"].cpu().numpy()
    assert not kept[false].any() and kept[~false].all()
    ate = float(gmf_amd.absolute_trajectory_error(gt_d, out["poses"]))
    ate_odo = float(gmf_amd.absolute_trajectory_error(gt_d, out["poses_odometry"]))
    print(f"ATE: odometry chain {ate_odo:.3f} cm, optimised {ate:.3f} cm")
    assert ate < ate_odo
    # the restatement from the same device-made information matrices, mask and start
    m = len(src)
    rP, rl, rkept, rst = R.global_optimization(out["poses_odometry"].cpu().numpy(), src, tgt, out["transformation"].cpu().numpy(),
                                               out["information"].cpu().numpy(), [t != s + 1 for s, t in pairs],
                                               out["mask"].cpu().numpy(), **R.REFERENCE_OPTIONS)
    assert np.array_equal(kept, rkept)
    dP, dl = np.abs(out["poses"].cpu().numpy() - rP).max(), np.abs(out["line_process"].cpu().numpy() - rl).max()
    print(f"scene: max|dP| = {dP:.3e} (tol {TOL['poses']:.3e}), max|dl| = {dl:.3e} (tol {TOL['line_process']:.3e})")
    assert dP <= TOL["poses"] and dl <= TOL["line_process"]
    st = out["stats"]
    assert [int(v) for v in st["iterations"][0]] == [p["iterations"] for p in rst["passes"]]
    assert [int(v) for v in st["stop"][0]] == [p["stop"] for p in rst["passes"]]
    # with the ICP refinement of every pair and the second optimisation, from pair poses with twice the noise (still inside
    # ICP's reach: about 3 cm at the fragments' rims against a correspondence distance of 7 cm).  The overlapping points are the
    # same points, so ICP comes back to the truth up to the pull of the rows just outside the overlap, whatever the start: the
    # false pairs stay out and the trajectory beats the odometry chain of the poses it was given.
    clouds, gt, pairs, X2, false = _scene(noise=0.02)
    out2 = gmf_amd.multiway_registration(pts, off, src, tgt, _g(X2), use_icp=True)
    torch.cuda.synchronize()
    kept2 = out2["kept"].cpu().numpy()
    assert not kept2[false].any() and kept2[~false].all()
    ate2 = float(gmf_amd.absolute_trajectory_error(gt_d, out2["poses"]))
    ate2_in = float(gmf_amd.absolute_trajectory_error(gt_d, gmf_amd.odometry_poses(_g(X2[:len(clouds) - 1]))))
    print(f"ATE with ICP: odometry chain of the given poses {ate2_in:.3f} cm, refined and optimised {ate2:.3f} cm")
    assert ate2 < ate2_in
    gmf_amd.check_status()
