"""GPU tests of the maximum-clique baseline (gmf_amd/clique.py: max_clique_batched, PMC, compatibility_graph; kernels k_pmc_* of
csrc/clique_kernels.hip; C ABI gmf_max_clique, gmf_pmc_graph) against the exact restatement of tests/clique_reference.py: the graph
bit for bit, the clique's size and membership in the set of all maximum cliques, the pose, ragged batching and determinism, the
step budget, the edge cases, the drop-in, graph capture and the C entry.

Bounds.  The graph and the clique are exact: equality, no margin.  The pose is held to 4 x the fp32 floor of rigid_transform_3d on
the device's own labels (spectral_reference.pose_floor), as the spectral-matching tests bound their step 5."""
import ctypes
import types

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import clique

import clique_reference as CR
import spectral_reference as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EYE = torch.eye(4)
KINDS = ("3dmatch", "kitti")
CASES = [(seed, N, kind, "squared") for seed, N in CR.TABLE for kind in KINDS] + [(3, 257, kind, "length") for kind in KINDS]


def _id(k):
    return f"{k[2]}-{k[0]}-{k[1]}-{k[3]}"


def _g(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def _clean_status():
    yield
    gmf_amd.check_status()


def _run(corr, src, tgt, thr, metric="squared", **kw):
    """One pair on the device -> (trans [4,4], labels [N], size, exact, steps, degree [N]) on the host."""
    out = gmf_amd.max_clique_batched(_g(corr)[None], _g(src)[None], _g(tgt)[None], thr, metric=metric, return_info=True, **kw)
    T, lab, size, exact, steps, degree = out
    N = len(corr)
    assert T.shape == (1, 4, 4) and lab.shape == degree.shape == (1, N) and size.shape == exact.shape == steps.shape == (1,)
    assert (lab.dtype, size.dtype, exact.dtype, steps.dtype, degree.dtype) == (torch.float32, torch.int32, torch.int32, torch.int64,
                                                                             torch.int32)
    return T[0].cpu(), lab[0].cpu(), int(size[0]), int(exact[0]), int(steps[0]), degree[0].cpu()


_DEVICE = {}


def _device(key):
    if key not in _DEVICE:
        (corr, src, tgt, thr, _), _, _, _, _ = CR.reference(*key)
        _DEVICE[key] = _run(corr, src, tgt, thr, key[3])
    return _DEVICE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the graph, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", CR.METRICS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 129, 300])
def test_graph_equals_numpy_float32(N, kind, metric):
    corr, src, tgt, thr, _ = CR.make_case(7, N, kind)
    A = CR.graph_np(corr, thr, metric)
    bits = gmf_amd.compatibility_graph(_g(corr), thr, metric)
    assert bits.shape == (N, (N + 63) // 64) and bits.dtype == torch.int64
    got = bits.cpu().numpy()
    assert np.array_equal(got, CR.bit_rows(A))
    if N % 64:                                              # the bits past column N - 1 of the last word
        assert not (got[:, -1].view(np.uint64) >> np.uint64(N % 64)).any()
    degree = _run(corr, src, tgt, thr, metric)[5]
    assert np.array_equal(degree.numpy(), A.sum(1))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exactness, pose
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", CASES, ids=_id)
def test_clique_is_a_maximum_clique(key):
    (corr, src, tgt, thr, gt), A, omega, cliques, _ = CR.reference(*key)
    T, lab, size, exact, steps, degree = _device(key)
    print(f"{_id(key)}: omega {omega}, {len(cliques)} maximum cliques; device size {size}, exact {exact}, steps {steps}")
    assert exact == 1 and size == omega
    assert set(np.unique(lab.numpy())) <= {0.0, 1.0}
    members = tuple(np.flatnonzero(lab.numpy()).tolist())
    assert len(members) == size and CR.is_clique(A, members)
    assert members in cliques
    if len(cliques) == 1:
        assert members == next(iter(cliques))
    if key[3] == "length":
        assert len(cliques) == 1 and np.array_equal(lab.numpy(), gt)


@pytest.mark.parametrize("local_rows", [0, 16])
@pytest.mark.parametrize("key", CASES, ids=_id)
def test_both_search_forms_are_exact(key, local_rows):
    """The search has two forms with one tree: a root with at most "clique_local_rows" candidates (default 384: every root of these
    cases) keeps its candidate sets in LDS, a wider one recomputes them from the bit matrix.  0 sends every root to the second
    form, 16 mixes them; each gives the default's clique."""
    from gmf_amd._util import handle_and_stream
    (corr, src, tgt, thr, gt), A, omega, cliques, _ = CR.reference(*key)
    h, _ = handle_and_stream(torch.zeros(1, device=DEV))
    cur = ctypes.c_int(0)
    h.call("gmf_get_tuning", b"clique_local_rows", ctypes.byref(cur))
    assert cur.value == 384
    h.call("gmf_set_tuning", b"clique_local_rows", local_rows)
    try:
        runs = [_run(corr, src, tgt, thr, key[3]) for _ in range(2)]
    finally:
        h.call("gmf_set_tuning", b"clique_local_rows", cur.value)
    T, lab, size, exact, steps, degree = runs[0]
    print(f"{_id(key)} local_rows {local_rows}: size {size}, exact {exact}, steps {steps}")
    assert exact == 1 and size == omega
    assert tuple(np.flatnonzero(lab.numpy()).tolist()) in cliques
    assert torch.equal(lab, runs[1][1]) and torch.equal(T, runs[1][0])
    assert torch.equal(lab, _device(key)[1]) and torch.equal(T, _device(key)[0])


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_pose_of_the_labels(key):
    (corr, src, tgt, thr, _), _, _, _, _ = CR.reference(*key)
    T, lab = _device(key)[:2]
    w = lab.double().numpy()
    err = np.abs(T.double().numpy() - SR.pose_np(src, tgt, w)).max()
    bound = 4 * SR.pose_floor(src, tgt, w)
    print(f"pose {_id(key)}: bound {bound:.3e}, device {err:.3e}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ragged batches, bits
# ---------------------------------------------------------------------------------------------------------------------------

def _ragged(sizes, seed0=20):
    pairs = [CR.make_case(seed0 + i, n, KINDS[i % 2])[:3] if n else
             (np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)) for i, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return pairs, off, tuple(_g(np.concatenate([p[k] for p in pairs])) for k in range(3))


@pytest.mark.parametrize("sizes", [(5, 64, 257, 300), (5, 64, 0, 257, 300)], ids=["ragged", "empty-pair"])
def test_ragged_batch_equals_each_pair_alone(sizes):
    pairs, off, (C, S, Q) = _ragged(sizes)
    T, lab, size, exact, steps, degree = gmf_amd.max_clique_batched(C, S, Q, 0.3, offsets=off, return_info=True)
    assert T.shape == (len(sizes), 4, 4) and lab.shape == degree.shape == (sum(sizes),) and size.shape == (len(sizes),)
    assert exact.tolist() == [1] * len(sizes)
    for b, (c, s, q) in enumerate(pairs):
        if not len(c):
            assert torch.equal(T[b].cpu(), EYE) and int(size[b]) == 0
            continue
        one = gmf_amd.max_clique_batched(_g(c)[None], _g(s)[None], _g(q)[None], 0.3, return_info=True)
        assert torch.equal(one[0][0], T[b]), b
        assert torch.equal(one[1][0], lab[off[b]:off[b + 1]]) and torch.equal(one[2][0], size[b]), b
        assert torch.equal(one[5][0], degree[off[b]:off[b + 1]]) and int(one[3][0]) == 1
        assert int(lab[off[b]:off[b + 1]].sum()) == int(size[b]) >= 1
    # device offsets: the same bits without the host knowing the sizes
    dev = gmf_amd.max_clique_batched(C, S, Q, 0.3, offsets=torch.tensor(off, dtype=torch.int32, device=DEV), return_info=True)
    for k in (0, 1, 2, 3, 5):
        assert torch.equal(dev[k], (T, lab, size, exact, steps, degree)[k]), k


def test_bits_run_to_run():
    pairs, off, (C, S, Q) = _ragged((5, 64, 257, 300))
    first = gmf_amd.max_clique_batched(C, S, Q, 0.3, offsets=off, return_info=True)
    for _ in range(4):
        again = gmf_amd.max_clique_batched(C, S, Q, 0.3, offsets=off, return_info=True)
        for k in (0, 1, 2, 3):
            assert torch.equal(first[k], again[k]), k


def test_graph_capture_equals_eager():
    pairs, off, (C, S, Q) = _ragged((5, 64, 0, 257, 300))

    def run():
        return gmf_amd.max_clique_batched(C, S, Q, 0.3, offsets=off, return_info=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                   # (also sizes the workspace and uploads the offsets before the capture)
            eager = [x.clone() for x in run()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    for k in (0, 1, 2, 3, 5):
        assert torch.equal(eager[k], captured[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the budget
# ---------------------------------------------------------------------------------------------------------------------------

def test_budget_of_one_step():
    key = (6, 300, "3dmatch", "squared")
    (corr, src, tgt, thr, _), A, omega, cliques, _ = CR.reference(*key)
    T, lab, size, exact, steps, _ = _run(corr, src, tgt, thr, max_steps=1)
    members = tuple(np.flatnonzero(lab.numpy()).tolist())
    print(f"max_steps = 1: size {size} of {omega}, exact {exact}, steps {steps}")
    assert len(members) == size >= 1 and CR.is_clique(A, members)
    assert size <= omega
    assert 0 <= steps <= 1 + clique.STEP_SLACK
    assert exact in (0, 1) and (exact == 0 or size == omega)
    assert torch.isfinite(T).all()
    T, lab, size, exact, steps, _ = _device(key)              # the default budget
    assert exact == 1 and size == omega and steps <= clique.DEFAULT_MAX_STEPS


# ---------------------------------------------------------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------------------------------------------------------

def test_edges():
    empty = gmf_amd.max_clique_batched(torch.zeros((2, 0, 6), device=DEV), torch.zeros((2, 0, 3), device=DEV),
                                       torch.zeros((2, 0, 3), device=DEV), 0.1, return_info=True)
    assert torch.equal(empty[0].cpu(), EYE.expand(2, 4, 4)) and empty[1].shape == (2, 0) and empty[2].tolist() == [0, 0]
    assert gmf_amd.compatibility_graph(torch.zeros((0, 6), device=DEV), 0.1).shape == (0, 0)
    c, s, t = CR.make_case(3, 1, "3dmatch")[:3]
    T, lab, size, exact, steps, degree = _run(c, s, t, 0.1)         # N = 1
    assert lab.tolist() == [1.0] and (size, exact, steps) == (1, 1, 0) and degree.tolist() == [0]
    assert torch.isfinite(T).all()                                  # one member: whatever rigid_transform_3d gives for it
    # no edges: the source rows on a line 1 apart, the target rows 100 apart; the smallest row alone
    a = np.zeros((8, 3), np.float32); a[:, 0] = np.arange(8)
    b = np.zeros((8, 3), np.float32); b[:, 1] = 100 * np.arange(8)
    for metric in CR.METRICS:
        assert not CR.graph_np(np.concatenate([a, b], 1), 0.1, metric).any()
        T, lab, size, exact, steps, degree = _run(np.concatenate([a, b], 1), a, b, 0.1, metric)
        assert lab.tolist() == [1.0] + [0.0] * 7 and (size, exact) == (1, 1) and not degree.any()
        assert torch.isfinite(T).all()
    # all rows identical: a complete graph
    for N in (5, 64, 200):
        c = np.tile(CR.make_case(3, 1, "kitti")[0], (N, 1))
        s, t = np.ascontiguousarray(c[:, :3]), np.ascontiguousarray(c[:, 3:])
        T, lab, size, exact, steps, degree = _run(c, s, t, 0.6)
        assert lab.tolist() == [1.0] * N and (size, exact) == (N, 1) and degree.tolist() == [N - 1] * N


def test_pair_of_8193_rows_is_refused():
    z = torch.zeros((1, 8193, 6), device=DEV)
    with pytest.raises(NotImplementedError, match="8192"):
        gmf_amd.max_clique_batched(z, z[..., :3].contiguous(), z[..., 3:].contiguous(), 0.1)
    with pytest.raises(NotImplementedError, match="8192"):
        gmf_amd.compatibility_graph(z[0], 0.1)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the drop-in, the C entry
# ---------------------------------------------------------------------------------------------------------------------------

def test_PMC_equals_the_batched_call_and_keeps_its_inputs():
    key = (3, 257, "3dmatch", "squared")
    (corr, src, tgt, thr, _), _, omega, _, _ = CR.reference(*key)
    c, s, t = _g(corr)[None], _g(src)[None], _g(tgt)[None]
    before = [x.clone() for x in (c, s, t)]
    trans, labels = gmf_amd.PMC(c, s, t, types.SimpleNamespace(inlier_threshold=thr))
    assert trans.shape == (1, 4, 4) and labels.shape == (1, 257) and int(labels.sum()) == omega
    want = _device(key)
    assert torch.equal(trans[0].cpu(), want[0]) and torch.equal(labels[0].cpu(), want[1])
    for x, y in zip(before, (c, s, t)):
        assert torch.equal(x, y)


def test_c_abi_entry():
    from gmf_amd._util import handle_and_stream
    key = (3, 257, "3dmatch", "squared")
    (corr, src, tgt, thr, _), _, _, _, _ = CR.reference(*key)
    c, s, t = _g(corr), _g(src), _g(tgt)
    off = torch.tensor([0, 257], dtype=torch.int32, device=DEV)
    lab, T = torch.zeros(257, device=DEV), torch.zeros((1, 4, 4), device=DEV)
    size, exact, degree = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (1, 1, 257))
    steps = torch.zeros(1, dtype=torch.int64, device=DEV)
    h, st = handle_and_stream(c)
    args = [c.data_ptr(), s.data_ptr(), t.data_ptr(), off.data_ptr(), 1, 257, 257, thr, 0, clique.DEFAULT_MAX_STEPS, lab.data_ptr(),
            T.data_ptr(), size.data_ptr(), exact.data_ptr(), steps.data_ptr(), degree.data_ptr()]
    h.call("gmf_max_clique", *args, st)
    want = _device(key)
    assert torch.equal(T[0].cpu(), want[0]) and torch.equal(lab.cpu(), want[1]) and torch.equal(degree.cpu(), want[5])
    assert (int(size[0]), int(exact[0])) == want[2:4]
    args[6] = 1000                                           # max_n is an upper bound: a larger one gives the same bits
    h.call("gmf_max_clique", *args, st)
    assert torch.equal(T[0].cpu(), want[0]) and torch.equal(lab.cpu(), want[1])
    args[6] = 257

    def put(k, v):
        return args[:k] + [v] + args[k + 1:]

    bad = [(put(0, None), -1, "null pointer"), (put(3, None), -1, "null pointer"), (put(10, None), -1, "null pointer"),
           (put(11, None), -1, "null pointer"), (put(12, None), -1, "null pointer"), (put(15, None), -1, "null pointer"),
           (put(4, 0), -2, "B must be"), (put(4, 65536), -2, "B must be"), (put(6, -1), -1, "max_n"), (put(5, -1), -1, "total_rows"),
           (put(6, 8193), -2, "8192"), (put(7, 0.0), -1, "inlier_threshold"), (put(7, float("nan")), -1, "inlier_threshold"),
           (put(8, 2), -1, "metric"), (put(9, 0), -1, "max_steps")]
    for a, code, msg in bad:
        with pytest.raises(RuntimeError, match=rf"status {code}\b.*max_clique.*" + msg):
            h.call("gmf_max_clique", *a, st)
    bits = torch.zeros((257, 5), dtype=torch.int64, device=DEV)
    gargs = [c.data_ptr(), off.data_ptr(), 1, 257, 257, thr, 0, bits.data_ptr(), degree.data_ptr()]
    h.call("gmf_pmc_graph", *gargs, st)
    assert torch.equal(bits, gmf_amd.compatibility_graph(c, thr))
    for k, code in ((0, -1), (1, -1), (7, -1), (8, -1)):
        with pytest.raises(RuntimeError, match=rf"status {code}\b.*pmc_graph.*null pointer"):
            h.call("gmf_pmc_graph", *(gargs[:k] + [None] + gargs[k + 1:]), st)
    gmf_amd.check_status()
