"""GPU tests of the spectral-matching baseline (gmf_amd/spectral.py: spectral_matching_batched, SM; kernels k_sm_* of
csrc/spectral_kernels.hip; C ABI gmf_spectral_matching) against the float64 restatement of tests/spectral_reference.py and the
golden fixture of the reference's own SM: the eigenvector in units of the fp32 floor, the labels, the pose alone and end to end,
ragged batching, the column splits, determinism, the edge cases, the drop-in, graph capture and the C entry.

Bounds.  The eigenvector is held to 4 x floor(case), the error of the reference's dense fp32 form against float64 on the same
case (2e-7 .. 7e-7): the factor covers another summation order, fused multiply-adds and the split columns.  The pose is held to
4 x the fp32 floor of step 5 on the same input, and to the project's 1e-4 on 3DMatch-shape cases."""
import os
import types

import numpy as np
import pytest
import torch

import gmf_amd

import spectral_reference as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(1, N, kind) for N in (64, 257, 1000) for kind in ("3dmatch", "kitti")]
EYE = torch.eye(4)


def _g(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def _clean_status():
    yield
    gmf_amd.check_status()


_DEVICE = {}


def _device(key, **kw):
    """(trans [4,4], labels [N], eig [N]) float64 numpy of one named case on the device; the default call is made once."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _DEVICE:
        (corr, src, tgt, thr, ratio), _, _ = SR.reference(*key)
        T, lab, eig = gmf_amd.spectral_matching_batched(_g(corr)[None], _g(src)[None], _g(tgt)[None], thr, top_ratio=ratio,
                                                        return_eigenvector=True, **kw)
        assert T.shape == (1, 4, 4) and lab.shape == eig.shape == (1, len(corr)) and lab.dtype == eig.dtype == torch.float32
        _DEVICE[k] = tuple(x[0].double().cpu().numpy() for x in (T, lab, eig))
    return _DEVICE[k]


def _pose_bound(src, tgt, w, kind):
    b = 4 * SR.pose_floor(src, tgt, w)
    return min(b, 1e-4) if kind == "3dmatch" else b


# ---------------------------------------------------------------------------------------------------------------------------
# 1. eigenvector, labels, pose
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", CASES, ids=lambda k: f"{k[2]}-{k[1]}")
def test_eigenvector_within_four_floors(key):
    _, r64, _ = SR.reference(*key)
    floor = SR.floor(key)
    err = SR.eig_error(_device(key)[2], r64["eig"])
    print(f"eig {key}: floor {floor:.3e}, device {err:.3e}, ratio {err / floor:.2f}")
    assert np.isfinite(err) and err <= 4 * floor


@pytest.mark.parametrize("key", CASES, ids=lambda k: f"{k[2]}-{k[1]}")
def test_labels_equal_the_restatement(key):
    _, r64, _ = SR.reference(*key)
    # the precondition, from the restatement alone: the k-th and (k+1)-th value are at least 16 floors apart
    assert 0 < r64["k"] < key[1] and r64["gap"] >= 16 * SR.floor(key), "badly chosen case"
    lab = _device(key)[1]
    assert set(np.unique(lab)) <= {0.0, 1.0} and lab.sum() == r64["k"]
    assert np.array_equal(lab, r64["labels"])


@pytest.mark.parametrize("key", CASES, ids=lambda k: f"{k[2]}-{k[1]}")
def test_pose_in_isolation(key):
    """Step 5 alone: the device's trans against the float64 step 5 on the device's own eig and labels."""
    (corr, src, tgt, thr, ratio), _, _ = SR.reference(*key)
    T, lab, eig = _device(key)
    w = eig * lab
    err = np.abs(T - SR.pose_np(src, tgt, w)).max()
    bound = _pose_bound(src, tgt, w, key[2])
    print(f"pose {key}: bound {bound:.3e}, device {err:.3e}")
    assert err <= bound


@pytest.mark.parametrize("key", CASES, ids=lambda k: f"{k[2]}-{k[1]}")
def test_pose_end_to_end(key, golden_dir):
    """Where the labels matched: trans against the restatement's, and against the reference's own where the fixture has the case."""
    (corr, src, tgt, thr, ratio), r64, _ = SR.reference(*key)
    T, lab, eig = _device(key)
    if not np.array_equal(lab, r64["labels"]):
        pytest.fail("labels differ: see test_labels_equal_the_restatement")
    bound = _pose_bound(src, tgt, r64["eig"] * r64["labels"], key[2])
    err = np.abs(T - r64["trans"]).max()
    print(f"end to end {key}: bound {bound:.3e}, device against float64 {err:.3e}")
    assert err <= bound
    if key[1] == 257:
        g = np.load(os.path.join(golden_dir, "sm_baseline.npz"))
        assert tuple(g[key[2] + "_args"][:2]) == key[:2] and np.array_equal(g[key[2] + "_labels"], lab)
        gerr = np.abs(T - g[key[2] + "_trans"]).max()
        print(f"end to end {key}: device against the fixture {gerr:.3e}")
        assert gerr <= bound
        assert SR.eig_error(eig, g[key[2] + "_eig"].astype(np.float64)) <= 4 * SR.floor(key)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. ragged batches, column splits, bits
# ---------------------------------------------------------------------------------------------------------------------------

def _ragged(sizes, seed0=20):
    pairs = [SR.make_case(seed0 + i, n, "3dmatch" if i % 2 == 0 else "kitti")[:3] if n else
             (np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)) for i, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return pairs, off, tuple(_g(np.concatenate([p[k] for p in pairs])) for k in range(3))


@pytest.mark.parametrize("sizes", [(5, 64, 257, 300), (5, 64, 0, 257, 300)], ids=["ragged", "empty-pair"])
def test_ragged_batch_equals_each_pair_alone(sizes):
    pairs, off, (C, S, Q) = _ragged(sizes)
    T, lab, eig = gmf_amd.spectral_matching_batched(C, S, Q, 0.3, top_ratio=0.2, offsets=off, return_eigenvector=True)
    assert T.shape == (len(sizes), 4, 4) and lab.shape == eig.shape == (sum(sizes),)
    for b, (c, s, q) in enumerate(pairs):
        if not len(c):
            assert torch.equal(T[b].cpu(), EYE)
            continue
        one = gmf_amd.spectral_matching_batched(_g(c)[None], _g(s)[None], _g(q)[None], 0.3, top_ratio=0.2, return_eigenvector=True)
        assert torch.equal(one[0][0], T[b]), b
        assert torch.equal(one[1][0], lab[off[b]:off[b + 1]]) and torch.equal(one[2][0], eig[off[b]:off[b + 1]]), b
        assert one[1].sum() == int(len(c) * 0.2)
    # device offsets: the same bits without the host knowing the sizes
    dev = gmf_amd.spectral_matching_batched(C, S, Q, 0.3, top_ratio=0.2, offsets=torch.tensor(off, dtype=torch.int32, device=DEV),
                                            return_eigenvector=True)
    for x, y in zip(dev, (T, lab, eig)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["3dmatch", "kitti"])
def test_forced_column_splits(kind):
    """N = 257 is three column tiles: 1, 2 and 5 (capped at 3) splits are three orders of a row's partial sums; each within the
    eigenvector bound, each the same bits on every run, and the default among them."""
    key = (1, 257, kind)
    _, r64, _ = SR.reference(*key)
    floor = SR.floor(key)
    eigs = []
    for splits in (1, 2, 5):
        T, lab, eig = _device(key, _col_splits=splits)
        err = SR.eig_error(eig, r64["eig"])
        print(f"splits {splits} {kind}: floor {floor:.3e}, device {err:.3e}")
        assert err <= 4 * floor and np.array_equal(lab, r64["labels"])
        eigs.append(eig)
        (corr, src, tgt, thr, ratio) = SR.make_case(*key)
        again = gmf_amd.spectral_matching_batched(_g(corr)[None], _g(src)[None], _g(tgt)[None], thr, top_ratio=ratio,
                                                  return_eigenvector=True, _col_splits=splits)
        assert np.array_equal(again[2][0].double().cpu().numpy(), eig) and np.array_equal(again[0][0].double().cpu().numpy(), T)
    assert not np.array_equal(eigs[0], eigs[2])                       # (the orders really differ)
    assert np.array_equal(_device(key)[2], eigs[2])                   # the rule gives three splits at N = 257


def test_bits_run_to_run():
    key = (1, 1000, "3dmatch")
    (corr, src, tgt, thr, ratio) = SR.make_case(*key)
    first = _device(key)
    for _ in range(2):
        T, lab, eig = gmf_amd.spectral_matching_batched(_g(corr)[None], _g(src)[None], _g(tgt)[None], thr, top_ratio=ratio,
                                                        return_eigenvector=True)
        for x, y in zip((T, lab, eig), first):
            assert np.array_equal(x[0].double().cpu().numpy(), y)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. edges
# ---------------------------------------------------------------------------------------------------------------------------

def _call(corr, src, tgt, thr=0.1, **kw):
    out = gmf_amd.spectral_matching_batched(_g(corr)[None], _g(src)[None], _g(tgt)[None], thr, return_eigenvector=True, **kw)
    return tuple(x[0].cpu() for x in out)


def test_edges_give_the_identity_and_no_labels():
    c, s, t = SR.make_case(3, 1, "3dmatch")[:3]
    T, lab, eig = _call(c, s, t)                                      # N = 1: M = [0]
    assert torch.equal(T, EYE) and lab.tolist() == [0.0] and eig.tolist() == [0.0]
    c, s, t = SR.make_case(3, 5, "3dmatch")[:3]
    T, lab, eig = _call(c, s, t)                                      # k = int(5 * 0.1) = 0
    assert torch.equal(T, EYE) and not lab.any() and torch.isfinite(eig).all()
    a = np.zeros((8, 3), np.float32); a[:, 0] = np.arange(8)
    b = np.zeros((8, 3), np.float32); b[:, 1] = 100 * np.arange(8)
    T, lab, eig = _call(np.concatenate([a, b], 1), a, b)              # all incompatible: M = 0, v = 0, k = 0
    assert torch.equal(T, EYE) and not lab.any() and not eig.any()
    T, lab, eig = _call(np.concatenate([a, b], 1), a, b, top_ratio=0.5)      # k = 4 rows of weight 0: the ties go to rows 0..3
    assert torch.equal(T, EYE) and lab.tolist() == [1.0] * 4 + [0.0] * 4 and not eig.any()
    empty = gmf_amd.spectral_matching_batched(torch.zeros((2, 0, 6), device=DEV), torch.zeros((2, 0, 3), device=DEV),
                                              torch.zeros((2, 0, 3), device=DEV), 0.1)
    assert torch.equal(empty[0].cpu(), EYE.expand(2, 4, 4)) and empty[1].shape == (2, 0)


def test_duplicate_rows_and_one_iteration():
    c, s, t = SR.make_case(4, 100, "3dmatch")[:3]
    c, s, t = (np.concatenate([x, x[:30], x[:30]]) for x in (c, s, t))          # every one of 30 rows three times: d = 0 off the diagonal
    T, lab, eig = _call(c, s, t)
    r64 = SR.sm_np(c, s, t, 0.1, 0.1)
    assert torch.isfinite(T).all() and torch.isfinite(eig).all() and lab.sum() == 16
    assert SR.eig_error(eig.double().numpy(), r64["eig"]) <= 4 * SR.eig_error(SR.sm_t32(c, s, t, 0.1, 0.1)["eig"], r64["eig"])
    T, lab, eig = _call(c, s, t, num_iterations=1)
    r64 = SR.sm_np(c, s, t, 0.1, 0.1, iterations=1)
    assert SR.eig_error(eig.double().numpy(), r64["eig"]) <= 4 * SR.eig_error(SR.sm_t32(c, s, t, 0.1, 0.1, iterations=1)["eig"],
                                                                              r64["eig"])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the drop-in, graph capture, the C entry
# ---------------------------------------------------------------------------------------------------------------------------

def test_SM_equals_the_batched_call_and_keeps_its_inputs():
    key = (1, 257, "kitti")
    (corr, src, tgt, thr, ratio) = SR.make_case(*key)
    c, s, t = _g(corr)[None], _g(src)[None], _g(tgt)[None]
    before = [x.clone() for x in (c, s, t)]
    trans, labels = gmf_amd.SM(c, s, t, types.SimpleNamespace(inlier_threshold=thr), top_ratio=ratio)
    assert trans.shape == (1, 4, 4) and labels.shape == (1, 257)
    want = _device(key)
    assert np.array_equal(trans[0].double().cpu().numpy(), want[0]) and np.array_equal(labels[0].double().cpu().numpy(), want[1])
    for x, y in zip(before, (c, s, t)):
        assert torch.equal(x, y)
    default = gmf_amd.SM(c, s, t, types.SimpleNamespace(inlier_threshold=thr))          # top_ratio = 0.1
    assert default[1].sum() == 25


def test_graph_capture_equals_eager():
    pairs, off, (C, S, Q) = _ragged((5, 64, 0, 257, 300))

    def run():
        return gmf_amd.spectral_matching_batched(C, S, Q, 0.3, top_ratio=0.2, offsets=off, return_eigenvector=True)

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
    for x, y in zip(eager, captured):
        assert torch.equal(x, y)


def test_c_abi_entry():
    from gmf_amd._util import handle_and_stream
    key = (1, 257, "3dmatch")
    (corr, src, tgt, thr, ratio) = SR.make_case(*key)
    c, s, t = _g(corr), _g(src), _g(tgt)
    off = torch.tensor([0, 257], dtype=torch.int32, device=DEV)
    topk = torch.tensor([int(257 * ratio)], dtype=torch.int32, device=DEV)
    eig, lab, T = torch.zeros(257, device=DEV), torch.zeros(257, device=DEV), torch.zeros((1, 4, 4), device=DEV)
    h, st = handle_and_stream(c)
    args = [c.data_ptr(), s.data_ptr(), t.data_ptr(), off.data_ptr(), 1, 257, thr, topk.data_ptr(), 10, eig.data_ptr(), lab.data_ptr(),
            T.data_ptr()]
    h.call("gmf_spectral_matching", *args, st)
    want = _device(key)
    for x, y in zip((T[0], lab, eig), want):
        assert np.array_equal(x.double().cpu().numpy(), y)
    args[5] = 1000                                           # max_n is an upper bound: a larger one gives the same bits
    h.call("gmf_spectral_matching", *args, st)
    assert np.array_equal(eig.double().cpu().numpy(), want[2]) and np.array_equal(T[0].double().cpu().numpy(), want[0])
    args[5] = 257

    def put(k, v):
        return args[:k] + [v] + args[k + 1:]

    bad = [(put(0, None), -1, "null pointer"), (put(3, None), -1, "null pointer"), (put(7, None), -1, "null pointer"),
           (put(11, None), -1, "null pointer"), (put(9, None), -1, "null pointer"),
           (put(4, 0), -2, "B must be"), (put(4, 65536), -2, "B must be"), (put(5, -1), -1, "max_n"),
           (put(6, 0.0), -1, "inlier_threshold"), (put(6, float("nan")), -1, "inlier_threshold"),
           (put(8, 0), -1, "iterations"), (put(8, 1001), -1, "iterations")]
    for a, code, msg in bad:
        with pytest.raises(RuntimeError, match=rf"status {code}\b.*spectral_matching.*" + msg):
            h.call("gmf_spectral_matching", *a, st)
    gmf_amd.check_status()


def test_c_abi_pair_beyond_max_n_is_left_out():
    """max_n is an upper bound the call cannot check without a read-back: a pair that breaks it gets the identity and zeros, the
    others their own bits."""
    from gmf_amd._util import handle_and_stream
    pairs, off, (C, S, Q) = _ragged((64, 300, 5))
    want = gmf_amd.spectral_matching_batched(C, S, Q, 0.3, top_ratio=0.2, offsets=off, return_eigenvector=True)
    o = torch.tensor(off, dtype=torch.int32, device=DEV)
    topk = torch.tensor([12, 60, 1], dtype=torch.int32, device=DEV)
    eig, lab, T = torch.ones(369, device=DEV), torch.ones(369, device=DEV), torch.ones((3, 4, 4), device=DEV)
    h, st = handle_and_stream(C)
    h.call("gmf_spectral_matching", C.data_ptr(), S.data_ptr(), Q.data_ptr(), o.data_ptr(), 3, 128, 0.3, topk.data_ptr(), 10,
           eig.data_ptr(), lab.data_ptr(), T.data_ptr(), st)
    assert torch.equal(T[1].cpu(), EYE) and not eig[64:364].any() and not lab[64:364].any()
    for b in (0, 2):
        assert torch.equal(T[b], want[0][b])
        assert torch.equal(eig[off[b]:off[b + 1]], want[2][off[b]:off[b + 1]]) and torch.equal(lab[off[b]:off[b + 1]], want[1][off[b]:off[b + 1]])
