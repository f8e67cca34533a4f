"""Host tests of the batched inlier-network input (gmf_amd/matching.py: find_knn_gpu_batch, find_knn_batch, find_pairs;
gmf_amd/dgr.py: matching_indices_batched, find_correct_correspondence, generate_inlier_input): the float64 restatement against
itself, the C ABI surface, and the argument checks that raise before any device call.  No device needed."""
import os
import re

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import _lib, dgr, fcgf

import dgr_input_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("gmf_nn_match_batched", "gmf_matching_indices_count", "gmf_matching_indices_fill", "gmf_inlier_input")


# ---- the restatement checks itself ------------------------------------------------------------------------------------------------

def _label_case(seed=0):
    rng = np.random.default_rng(seed)
    len_batch = [(40, 55), (30, 20)]
    pos, pred = [], []
    for n0, n1 in len_batch:
        p = np.stack([rng.integers(0, n0, 200), rng.integers(0, n1, 200)], 1).astype(np.int64)
        pos.append(np.concatenate([p, p[:17]]))                  # with duplicates
        pred.append(np.stack([np.arange(n0), rng.integers(0, n1, n0)], 1).astype(np.int64))
    return len_batch, pos, pred


def test_hash_membership_is_set_membership_for_a_large_seed():
    len_batch, pos, pred = _label_case()
    want = R.correct_by_set(pos, pred)
    assert want.any() and not want.all()
    assert np.array_equal(R.correct_by_hash(pos, pred, len_batch=len_batch), want)
    assert np.array_equal(R.correct_by_hash(pos, pred, hash_seed=1000), want)


def test_small_hash_seed_collides_in_the_expected_rows():
    """seed 7 < N0: (i, j) and (i', j') share a key when i + 7 j = i' + 7 j'.  The rows where the hash answers differently from set
    membership are exactly those whose key is a positive key although the pair itself is not positive."""
    len_batch, pos, pred = _label_case(1)
    by_set = R.correct_by_set(pos, pred)
    by_hash = R.correct_by_hash(pos, pred, hash_seed=7)
    expected = []
    for p, q in zip(pos, pred):
        keys = {int(i) + 7 * int(j) for i, j in p}
        pairs = {(int(i), int(j)) for i, j in p}
        expected.append(np.array([(int(i) + 7 * int(j) in keys) and (int(i), int(j)) not in pairs for i, j in q]))
    expected = np.concatenate(expected)
    assert expected.any()
    assert np.array_equal(by_hash != by_set, expected)
    assert by_hash[by_set].all()                                   # a collision only ever adds a label


def test_matching_indices_restatement_order_and_radius_convention():
    xyz0 = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    xyz1 = np.array([[0.5, 0, 0], [0, 0, 0], [1, 0, 0], [3, 0, 0]], np.float32)
    T = np.eye(4)[None]
    pairs, off = R.matching_indices(xyz0, [0, 2], xyz1, [0, 4], T, 1.0)      # a point at exactly the radius is outside
    assert pairs.tolist() == [[0, 0], [0, 1], [1, 0], [1, 2]] and off.tolist() == [0, 4]
    assert R.radius_margin(xyz0, [0, 2], xyz1, [0, 4], T, 1.0) == 0.0


# ---- the C ABI surface ---------------------------------------------------------------------------------------------------------------

def _header():
    with open(os.path.join(ROOT, "include", "gmf_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_header_declares_and_lib_binds_with_matching_arity(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/gmf_hip.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert len(args) == n_args


def test_abi_version_is_still_5():
    assert re.search(r"#define\s+GMF_ABI_VERSION\s+5\b", _header())


def test_exports():
    for name in ("find_knn_gpu_batch", "find_knn_batch", "find_pairs", "matching_indices_batched", "find_correct_correspondence",
                 "generate_inlier_input"):
        assert callable(getattr(gmf_amd, name)) and name in gmf_amd.__all__


# ---- argument checks that raise before any device call ----------------------------------------------------------------------------

def _feats(n, d=8, seed=0):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


def test_offsets_that_do_not_ascend():
    x0, x1, T = torch.zeros(10, 3), torch.zeros(12, 3), torch.eye(4).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="must ascend"):
        gmf_amd.matching_indices_batched(x0, [0, 7, 5, 10], x1, [0, 4, 8, 12], torch.eye(4).repeat(3, 1, 1), 0.1)
    with pytest.raises(RuntimeError, match="must ascend"):
        gmf_amd.matching_indices_batched(x0, [0, 4, 10], x1, [0, 13, 12], T, 0.1)
    with pytest.raises(RuntimeError, match="must ascend"):
        gmf_amd.matching_indices_batched(x0, [1, 4, 10], x1, [0, 6, 12], T, 0.1)


def test_mismatched_widths():
    for fn in (gmf_amd.find_knn_gpu_batch, gmf_amd.find_knn_batch, gmf_amd.find_pairs):
        with pytest.raises(RuntimeError, match="differ in width"):
            fn(_feats(10, 8), _feats(12, 9), [(10, 12)])


def test_len_batch_must_sum_to_the_rows():
    for fn in (gmf_amd.find_knn_gpu_batch, gmf_amd.find_knn_batch, gmf_amd.find_pairs):
        with pytest.raises(RuntimeError, match="len_batch sums to"):
            fn(_feats(10), _feats(12), [(4, 6), (5, 6)])
    iC = torch.zeros(10, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="len_batch sums to"):
        gmf_amd.generate_inlier_input(None, None, None, iC, iC, None, None, [(4, 5), (5, 5)], None, inlier_feature_type="ones")


@pytest.mark.parametrize("ftype", ["counts", "nope", None])
def test_bad_inlier_feature_type(ftype):
    iC = torch.zeros(10, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="Inlier feature type not defined"):
        gmf_amd.generate_inlier_input(None, None, None, iC, iC, None, None, [(10, 10)], None, inlier_feature_type=ftype)


def test_knn_2_is_not_built():
    for fn in (gmf_amd.find_knn_gpu_batch, gmf_amd.find_knn_batch, gmf_amd.find_pairs):
        with pytest.raises(NotImplementedError, match="knn = 1"):
            fn(_feats(10), _feats(12), [(10, 12)], knn=2)
    iC = torch.zeros(10, 4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="knn = 1"):
        gmf_amd.generate_inlier_input(None, None, None, iC, iC, None, None, [(10, 10)], None, inlier_feature_type="ones", knn=2)


def test_search_methods():
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        gmf_amd.find_knn_batch(_feats(10), _feats(12), [(10, 12)], search_method="cpu")
    with pytest.raises(ValueError, match="Search method kdtree not defined"):
        gmf_amd.find_knn_batch(_feats(10), _feats(12), [(10, 12)], search_method="kdtree")


def test_wide_descriptors_and_host_tensors_are_refused():
    with pytest.raises(NotImplementedError, match="above 128"):
        gmf_amd.find_knn_gpu_batch(_feats(4, 129), _feats(4, 129), [(4, 4)])
    with pytest.raises(RuntimeError, match="HIP device"):
        gmf_amd.find_knn_gpu_batch(_feats(4), _feats(4), [(4, 4)])


def test_label_asserts_are_runtime_errors():
    pred = [torch.zeros(3, 2, dtype=torch.int64)] * 2
    with pytest.raises(RuntimeError, match="pos_pairs entries"):
        gmf_amd.find_correct_correspondence(pred[:1], pred, hash_seed=10)
    with pytest.raises(RuntimeError, match="len_batch must have one"):
        gmf_amd.find_correct_correspondence(pred, pred, len_batch=[(3, 3)])
    with pytest.raises(RuntimeError, match="len_batch must have one"):
        gmf_amd.find_correct_correspondence(pred, pred)
    with pytest.raises(RuntimeError, match="HIP device"):
        gmf_amd.find_correct_correspondence(pred, pred, hash_seed=10)
