"""GPU tests of the batched inlier-network input: find_knn_gpu_batch / find_knn_batch / find_pairs against the loop of
find_knn_gpu calls (bit for bit), and matching_indices_batched, find_correct_correspondence and generate_inlier_input against
the float64 restatement of tests/dgr_input_reference.py."""
import os

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import dgr, fcgf
from gmf_amd import train as T

import dgr_input_reference as R
import fcgf_reference as FR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(autouse=True)
def _clean_status():
    yield
    gmf_amd.check_status()


# ---- 1. batched matching equals the loop --------------------------------------------------------------------------------------------

# sizes not a multiple of 32, a one-row source, an empty source, N0 > N1, and a pair large enough for several key splits (4200 keys:
# 132 tiles, at least 33 stages) beside small ones
LEN_BATCH = [(70, 45), (1, 33), (0, 20), (300, 17), (1500, 4200), (33, 64), (0, 0)]


def _descriptors(len_batch, d, seed):
    g = torch.Generator().manual_seed(seed)
    n0 = sum(a for a, _ in len_batch)
    n1 = sum(b for _, b in len_batch)
    F0 = torch.randn(n0, d, generator=g)
    F1 = torch.randn(n1, d, generator=g)
    F0 = F0 / F0.norm(dim=1, keepdim=True)
    F1 = F1 / F1.norm(dim=1, keepdim=True)
    return F0, F1


def _loop(F0, F1, len_batch, nn_max_n):
    """What the caller had to write before: one find_knn_gpu per pair."""
    nns, dists, a, b = [], [], 0, 0
    for n0, n1 in len_batch:
        if n0:
            i, dd = gmf_amd.find_knn_gpu(F0[a:a + n0], F1[b:b + n1], nn_max_n=nn_max_n, knn=1, return_distance=True)
        else:
            i = torch.empty((0, 1) if nn_max_n > 1 else (0,), dtype=torch.int64, device=DEV)
            dd = torch.empty((0, 1), dtype=torch.float32, device=DEV)
        nns.append(i)
        dists.append(dd)
        a, b = a + n0, b + n1
    return nns, dists


def _equal_with_nan(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.parametrize("d", [5, 32, 33, 64, 128])
@pytest.mark.parametrize("nn_max_n", [250, -1])
def test_batched_matching_equals_the_loop(d, nn_max_n):
    F0, F1 = _descriptors(LEN_BATCH, d, seed=d)
    # keys duplicated inside a pair (the first index must win): pair 0's key 30 repeats key 3, pair 4's keys 4000.. repeat keys 10..
    off1 = R.offsets([b for _, b in LEN_BATCH])
    F1[off1[0] + 30] = F1[off1[0] + 3]
    F0[5] = F1[off1[0] + 3]                                       # and a query that meets both exactly
    F1[off1[4] + 4000:off1[4] + 4100] = F1[off1[4] + 10:off1[4] + 110]
    # a NaN source row: local index 0, distance NaN
    off0 = R.offsets([a for a, _ in LEN_BATCH])
    F0[off0[4] + 77, 1] = float("nan")
    F0, F1 = _g(F0), _g(F1)
    want_i, want_d = _loop(F0, F1, LEN_BATCH, nn_max_n)
    got_i, got_d = gmf_amd.find_knn_gpu_batch(F0, F1, LEN_BATCH, nn_max_n=nn_max_n, return_distance=True)
    assert len(got_i) == len(LEN_BATCH)
    for b in range(len(LEN_BATCH)):
        assert got_i[b].dtype == torch.int64 and got_i[b].shape == want_i[b].shape
        assert torch.equal(got_i[b], want_i[b]), f"pair {b}: indices differ"
        assert _equal_with_nan(got_d[b], want_d[b]), f"pair {b}: distances differ"
    assert int(got_i[0].reshape(-1)[5]) == 3
    assert int(got_i[4].reshape(-1)[77]) == 0 and bool(torch.isnan(got_d[4][77]).all())
    # without distances, through find_knn_batch
    only_i = gmf_amd.find_knn_batch(F0, F1, LEN_BATCH, nn_max_n=nn_max_n, search_method="gpu")
    assert all(torch.equal(a, b) for a, b in zip(only_i, want_i))
    # concat_results: one tensor, global key indices
    cat_i, cat_d = gmf_amd.find_knn_gpu_batch(F0, F1, LEN_BATCH, nn_max_n=nn_max_n, return_distance=True, concat_results=True)
    assert torch.equal(cat_i, torch.cat([w + int(o) for w, o in zip(want_i, off1[:-1])]))
    assert _equal_with_nan(cat_d, torch.cat(want_d))
    # find_pairs
    pairs = gmf_amd.find_pairs(F0, F1, LEN_BATCH, nn_max_n=nn_max_n)
    for b, (n0, _) in enumerate(LEN_BATCH):
        assert pairs[b].shape == (n0, 2) and pairs[b].dtype == torch.int64 and pairs[b].is_cuda
        assert torch.equal(pairs[b][:, 0], torch.arange(n0, device=DEV))
        assert torch.equal(pairs[b][:, 1], want_i[b].reshape(-1))


def test_single_pair_batch_equals_find_knn_gpu():
    F0, F1 = _descriptors([(2500, 3100)], 32, seed=1)
    F0, F1 = _g(F0), _g(F1)
    i, dd = gmf_amd.find_knn_gpu(F0, F1, nn_max_n=-1, return_distance=True)
    bi, bd = gmf_amd.find_knn_gpu_batch(F0, F1, [(2500, 3100)], return_distance=True)
    assert torch.equal(bi[0], i) and torch.equal(bd[0], dd)


# ---- 2. no leakage across pairs -----------------------------------------------------------------------------------------------------

def test_no_leakage_across_pairs():
    """Pair 1's keys hold exact copies of pair 0's queries; pair 0's own keys only perturbed copies, permuted.  A kernel that let a
    query see another pair's keys would prefer the exact copy."""
    g = torch.Generator().manual_seed(11)
    n = [200, 257, 90]
    Q = [torch.randn(k, 32, generator=g) for k in n]
    perm = [torch.randperm(k, generator=g) for k in n]
    K = []
    for b in range(3):
        keys = torch.empty(n[b], 32)
        keys[perm[b]] = Q[b] + 1e-3 * torch.randn(n[b], 32, generator=g)          # key perm[i] ~ query i
        K.append(keys)
    K[1] = torch.cat([K[1], Q[0]])                                               # exact copies of pair 0's queries
    K[2] = torch.cat([Q[1][:50], K[2]])                                          # and of pair 1's, in front
    perm[2] = perm[2] + 50
    len_batch = [(n[b], K[b].shape[0]) for b in range(3)]
    got = gmf_amd.find_knn_gpu_batch(_g(torch.cat(Q)), _g(torch.cat(K)), len_batch)
    for b in range(3):
        assert torch.equal(got[b].cpu(), perm[b]), f"pair {b}"


# ---- 3. a pair with queries and no keys ---------------------------------------------------------------------------------------------

def test_queries_without_keys_raise():
    F0, F1 = _descriptors([(10, 12), (5, 0)], 16, seed=2)
    with pytest.raises(RuntimeError, match="no key rows"):
        gmf_amd.find_knn_gpu_batch(_g(F0), _g(F1), [(10, 12), (5, 0)])
    gmf_amd.check_status()
    got = gmf_amd.find_knn_gpu_batch(_g(F0[:10]), _g(F1), [(10, 12), (0, 0)])    # the handle still works
    assert got[0].shape == (10,) and got[1].shape == (0,)


# ---- 4. ground-truth pairs ----------------------------------------------------------------------------------------------------------

GT_SEED = 4            # chosen on the CPU: no candidate pair's d^2 within a relative 1e-9 of radius^2 (asserted below)
GT_RADIUS = 0.08


def _rigid(rng, angle, shift):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    Tm = np.eye(4)
    Tm[:3, :3] = Rm
    Tm[:3, 3] = shift
    return Tm


def _gt_case():
    """Three seeded pairs: target = T source + noise (a permuted subset plus clutter); the last pair is far apart (no pairs)."""
    rng = np.random.default_rng(GT_SEED)
    sizes = [(900, 1100), (1300, 700), (257, 300)]
    x0s, x1s, Ts = [], [], []
    for b, (n0, n1) in enumerate(sizes):
        x0 = rng.uniform(-1, 1, size=(n0, 3)).astype(np.float32)
        Tm = _rigid(rng, 0.3 + 0.4 * b, rng.uniform(-0.5, 0.5, size=3))
        src = rng.integers(0, n0, n1)
        x1 = (x0[src].astype(np.float64) @ Tm[:3, :3].T + Tm[:3, 3] + rng.normal(scale=0.03, size=(n1, 3))).astype(np.float32)
        if b == 2:
            x1 = x1 + np.float32(50.0)
        x0s.append(x0), x1s.append(x1), Ts.append(Tm)
    off0 = R.offsets([a for a, _ in sizes])
    off1 = R.offsets([b for _, b in sizes])
    return np.concatenate(x0s), off0, np.concatenate(x1s), off1, np.stack(Ts), sizes


def test_matching_indices_against_the_restatement():
    x0, off0, x1, off1, Ts, _ = _gt_case()
    # a condition on the inputs, not a tolerance on the result: no candidate pair sits on the radius
    assert R.radius_margin(x0, off0, x1, off1, Ts, GT_RADIUS) > 1e-9
    want, want_off = R.matching_indices(x0, off0, x1, off1, Ts, GT_RADIUS)
    assert want_off[1] > 500 and want_off[2] - want_off[1] > 500 and want_off[3] == want_off[2]     # the far pair is empty
    pairs, pair_off = gmf_amd.matching_indices_batched(_g(x0), off0.tolist(), _g(x1), off1.tolist(), torch.as_tensor(Ts), GT_RADIUS)
    assert pairs.dtype == torch.int64 and pair_off.dtype == torch.int64 and pairs.is_cuda and pair_off.is_cuda
    assert np.array_equal(pair_off.cpu().numpy(), want_off)
    assert np.array_equal(pairs.cpu().numpy(), want)
    # device offsets give the same
    p2, o2 = gmf_amd.matching_indices_batched(_g(x0), _g(off0.astype(np.int32)), _g(x1), _g(off1.astype(np.int32)), _g(Ts), GT_RADIUS)
    assert torch.equal(p2, pairs) and torch.equal(o2, pair_off)


def test_matching_indices_nothing_in_range():
    x0 = np.zeros((5, 3), np.float32)
    x1 = np.ones((7, 3), np.float32)
    pairs, off = gmf_amd.matching_indices_batched(_g(x0), [0, 5], _g(x1), [0, 7], torch.eye(4)[None], 0.5)
    assert pairs.shape == (0, 2) and off.tolist() == [0, 0]


# ---- 5. labels --------------------------------------------------------------------------------------------------------------------

def _label_case(seed=0):
    rng = np.random.default_rng(seed)
    len_batch = [(400, 550), (300, 200), (64, 64)]
    pos, pred = [], []
    for b, (n0, n1) in enumerate(len_batch):
        p = np.stack([rng.integers(0, n0, 3000), rng.integers(0, n1, 3000)], 1).astype(np.int64)
        p = np.concatenate([p, p[:170]])                              # duplicated positive pairs
        if b == 2:
            p = p[:0]                                                 # an empty positive list
        pos.append(p)
        pred.append(np.stack([np.arange(n0), rng.integers(0, n1, n0)], 1).astype(np.int64))
    return len_batch, pos, pred


def test_find_correct_correspondence_against_the_restatement():
    len_batch, pos, pred = _label_case()
    pred_d = [_g(p) for p in pred]
    want = R.correct_by_hash(pos, pred, len_batch=len_batch)
    assert want.any() and not want.all()
    got = gmf_amd.find_correct_correspondence([_g(p) for p in pos], pred_d, len_batch=len_batch)
    assert got.dtype == torch.bool and got.is_cuda and got.shape == (sum(a for a, _ in len_batch),)
    assert np.array_equal(got.cpu().numpy(), want)
    # positives on the CPU
    got = gmf_amd.find_correct_correspondence([torch.as_tensor(p) for p in pos], pred_d, len_batch=len_batch)
    assert np.array_equal(got.cpu().numpy(), want)
    # an explicit hash_seed, large and too small (the collisions of the reference)
    for seed in (1000, 7):
        want_s = R.correct_by_hash(pos, pred, hash_seed=seed)
        got = gmf_amd.find_correct_correspondence([_g(p) for p in pos], pred_d, hash_seed=seed)
        assert np.array_equal(got.cpu().numpy(), want_s)
    assert not np.array_equal(R.correct_by_hash(pos, pred, hash_seed=7), want)
    # positives in the packed form of matching_indices_batched
    packed = (_g(np.concatenate(pos)), _g(R.offsets([len(p) for p in pos])))
    got = gmf_amd.find_correct_correspondence(packed, pred_d, len_batch=len_batch)
    assert np.array_equal(got.cpu().numpy(), want)


def test_labels_on_the_ground_truth_pairs_are_the_direct_radius_test():
    x0, off0, x1, off1, Ts, sizes = _gt_case()
    g = torch.Generator().manual_seed(3)
    # predicted pairs: half of them a true neighbour (the first positive of the row, where it has one), half random
    want_pairs, want_off = R.matching_indices(x0, off0, x1, off1, Ts, GT_RADIUS)
    pred = []
    for b, (n0, n1) in enumerate(sizes):
        j = torch.randint(0, n1, (n0,), generator=g).numpy()
        pp = want_pairs[want_off[b]:want_off[b + 1]]
        first = {}
        for i, jj in pp[::-1]:
            first[int(i)] = int(jj)
        for i in range(0, n0, 2):
            j[i] = first.get(i, j[i])
        pred.append(np.stack([np.arange(n0), j], 1).astype(np.int64))
    direct = np.concatenate([R.squared_distances(x0[off0[b]:off0[b + 1]], x1[off1[b]:off1[b + 1]], Ts[b])[p[:, 0], p[:, 1]]
                             < GT_RADIUS ** 2 for b, p in enumerate(pred)])
    assert direct.any() and not direct.all()
    pos = gmf_amd.matching_indices_batched(_g(x0), off0.tolist(), _g(x1), off1.tolist(), torch.as_tensor(Ts), GT_RADIUS)
    got = gmf_amd.find_correct_correspondence(pos, [_g(p) for p in pred], len_batch=sizes)
    assert np.array_equal(got.cpu().numpy(), direct)


# ---- 6. generate_inlier_input -------------------------------------------------------------------------------------------------------

VOXEL = 0.0625
_CASE = {}


def _voxelised(xyz, batch):
    x = _g(xyz)
    sel = gmf_amd.voxel_select(x, VOXEL)
    x = x[sel].contiguous()
    c = torch.floor(x.double() / VOXEL).int()
    return x, torch.cat([torch.full((len(c), 1), batch, dtype=torch.int32, device=DEV), c], 1).contiguous()


def _input_case():
    """B = 3 ragged pairs from the demo fragments: (cloud0, cloud1), the two reversed, and a crop of each; a seeded FCGF."""
    if "c" not in _CASE:
        z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
        c0, c1 = z["cloud0"].astype(np.float32), z["cloud1"].astype(np.float32)
        crop0 = c0[c0[:, 0] < np.median(c0[:, 0])]
        crop1 = c1[c1[:, 1] < np.median(c1[:, 1])]
        xyz0s, xyz1s, C0, C1 = [], [], [], []
        for b, (a, c) in enumerate([(c0, c1), (c1, c0), (crop0, crop1)]):
            x, cc = _voxelised(a, b)
            xyz0s.append(x), C0.append(cc)
            x, cc = _voxelised(c, b)
            xyz1s.append(x), C1.append(cc)
        iC0, iC1 = torch.cat(C0).contiguous(), torch.cat(C1).contiguous()
        len_batch = [(len(a), len(b)) for a, b in zip(xyz0s, xyz1s)]
        torch.manual_seed(5)
        m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3)
        cond = torch.cat([C0[0], C1[0]]).cpu().numpy()
        cond[len(C0[0]):, 0] = 1
        m.load_state_dict(FR.conditioned_state_dict(m, cond, torch.ones(len(cond), 1)))
        _CASE["c"] = (m.to(DEV).eval(), xyz0s, xyz1s, iC0, iC1, len_batch)
    return _CASE["c"]


def _ones(c):
    return torch.ones((len(c), 1), device=DEV)


def test_generate_inlier_input_rows_features_pairs_and_labels():
    m, xyz0s, xyz1s, iC0, iC1, len_batch = _input_case()
    assert len(set(len_batch)) == 3 and all(a != b for a, b in len_batch)
    B = len(len_batch)
    off0 = R.offsets([a for a, _ in len_batch])
    off1 = R.offsets([b for _, b in len_batch])
    # the pieces by hand: FCGF per side, the loop of find_knn_gpu calls, inlier_coordinates per pair
    F0, F1 = m(iC0, _ones(iC0)), m(iC1, _ones(iC1))
    loop_pairs, loop_coords = [], []
    for b in range(B):
        nn = gmf_amd.find_knn_gpu(F0[off0[b]:off0[b + 1]], F1[off1[b]:off1[b + 1]], nn_max_n=250).reshape(-1)
        idx0 = torch.arange(len(nn), device=DEV)
        loop_pairs.append(torch.stack([idx0, nn], 1))
        loop_coords.append(gmf_amd.inlier_coordinates(iC0[off0[b]:off0[b + 1]], iC1[off1[b]:off1[b + 1]], idx0, nn))
    loop_coords = torch.cat(loop_coords)
    assert torch.equal(loop_coords[:, 0], iC0[:, 0])                  # the batch column is iC0's
    # ground truth from an identity pose at 2 voxels (the fragments are not aligned: few pairs are correct, which is fine here)
    Ts = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    pos = gmf_amd.matching_indices_batched(torch.cat(xyz0s), off0.tolist(), torch.cat(xyz1s), off1.tolist(), Ts, 2 * VOXEL)
    pred_np = [p.cpu().numpy() for p in loop_pairs]
    want_labels = R.correct_by_hash([pos[0][int(pos[1][b]):int(pos[1][b + 1])].cpu().numpy() for b in range(B)], pred_np,
                                    len_batch=len_batch)
    x0, x1 = torch.cat(xyz0s).cpu().numpy(), torch.cat(xyz1s).cpu().numpy()
    for ftype, width in (("ones", 1), ("feats", 64), ("coords", 6)):
        coords, feats, pairs, labels = gmf_amd.generate_inlier_input(m, xyz0s, xyz1s, iC0, iC1, _ones(iC0), _ones(iC1), len_batch, pos,
                                                                     inlier_feature_type=ftype, nn_max_n=250)
        assert coords.dtype == torch.int32 and coords.shape == (off0[-1], 7) and torch.equal(coords, loop_coords)
        assert len(pairs) == B and all(torch.equal(a, b) and a.dtype == torch.int64 for a, b in zip(pairs, loop_pairs))
        assert labels.dtype == torch.bool and np.array_equal(labels.cpu().numpy(), want_labels)
        _, want_feats = R.inlier_input(iC0.cpu().numpy(), iC1.cpu().numpy(), len_batch, pred_np, ftype, F0=F0.cpu().numpy(),
                                       F1=F1.cpu().numpy(), xyz0=x0, xyz1=x1)
        assert feats.dtype == torch.float32 and feats.shape == (off0[-1], width)
        got = feats.cpu().numpy().astype(np.float64)
        if ftype == "coords":
            # cos of a float32 coordinate evaluated in float64 and rounded once: within one float32 ulp of 1 (|cos| <= 1) of the
            # float64 value, whatever the last bit of the device's float64 cos
            assert np.abs(got - want_feats).max() <= float(np.finfo(np.float32).eps)
        else:
            assert np.array_equal(got, want_feats)                    # copies
    # pos_pairs=None: no labels
    out = gmf_amd.generate_inlier_input(m, xyz0s, xyz1s, iC0, iC1, _ones(iC0), _ones(iC1), len_batch, None, inlier_feature_type="ones",
                                        nn_max_n=250)
    assert out[3] is None and torch.equal(out[0], loop_coords)


def test_generate_inlier_input_feeds_the_training_step():
    m, xyz0s, xyz1s, iC0, iC1, len_batch = _input_case()
    B = len(len_batch)
    off0 = R.offsets([a for a, _ in len_batch])
    off1 = R.offsets([b for _, b in len_batch])
    Ts = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    pos = gmf_amd.matching_indices_batched(torch.cat(xyz0s), off0.tolist(), torch.cat(xyz1s), off1.tolist(), Ts, 2 * VOXEL)
    coords, feats, pairs, labels = gmf_amd.generate_inlier_input(m, xyz0s, xyz1s, iC0, iC1, _ones(iC0), _ones(iC1), len_batch, pos,
                                                                 inlier_feature_type="ones", nn_max_n=250)
    torch.manual_seed(6)
    net = gmf_amd.ResUNetBN2C(1, 1, D=6, pe=True).to(DEV).train()
    g = torch.Generator().manual_seed(9)
    p_tok, q_tok = _g(torch.randn(1, 80, 128, generator=g)), _g(torch.randn(1, 80, 128, generator=g))
    logits = T.resunet_train(net, coords, feats, p_tokens=p_tok, q_tokens=q_tok)
    assert logits.shape[0] == coords.shape[0]
    loss, stats = dgr.inlier_training_loss(logits, xyz0s, xyz1s, pairs, labels, Ts.to(DEV), clip_weight_thresh=0.05)
    assert bool(stats["valid"].any())
    assert bool(torch.isfinite(loss))
    loss.backward()
    grad = net.final.kernel.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
