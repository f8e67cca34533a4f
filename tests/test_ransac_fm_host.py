"""CPU-side checks of the feature-matching RANSAC (gmf_amd/solvers.py: ransac_feature_matching_batched,
registration_ransac_based_on_feature_matching; DeepGlobalRegistration.safeguard_method): the public names, every argument check,
the no-device error, the C ABI entry, and the self-test of the numpy restatement (tests/ransac_fm_reference.py) that
tests/test_gpu_ransac_fm.py holds the device to."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ransac_fm_reference as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ransac_feature_matching_batched", "registration_ransac_based_on_feature_matching"]


def test_public_names_exported():
    import gmf_amd
    for n in NAMES:
        assert hasattr(gmf_amd, n), n
        assert n in gmf_amd.__all__, n
    sig = inspect.signature(gmf_amd.ransac_feature_matching_batched)
    assert list(sig.parameters) == ["source", "target", "nn", "max_correspondence_distance", "source_offsets", "target_offsets",
                                    "ransac_n", "max_iteration", "max_validation", "checker_distance", "edge_length_threshold",
                                    "seed", "first_pair", "search", "return_hypotheses"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["ransac_n"], d["max_iteration"], d["max_validation"], d["search"]) == (4, 100000, 1000, "grid")
    sig = inspect.signature(gmf_amd.registration_ransac_based_on_feature_matching)
    assert list(sig.parameters) == ["source", "target", "source_feature", "target_feature", "max_correspondence_distance",
                                    "ransac_n", "checker_distance", "edge_length_threshold", "max_iteration", "max_validation",
                                    "seed", "search"]
    assert "[d, N]" in gmf_amd.registration_ransac_based_on_feature_matching.__doc__      # the layout that is not accepted


def test_argument_checks():
    import gmf_amd
    F = gmf_amd.ransac_feature_matching_batched
    s, t = torch.rand(2, 16, 3), torch.rand(2, 20, 3)
    nn = torch.zeros(2, 16, dtype=torch.int64)
    rs, rt, rn = s.reshape(-1, 3), t.reshape(-1, 3), nn.reshape(-1)
    bad = [
        (dict(target=torch.rand(3, 20, 3)), "same number of pairs"),
        (dict(source=s.double()), "float32"), (dict(target=t.double()), "float32"),
        (dict(source=s[..., :2]), r"\[B,N,3\]"), (dict(source=rs, nn=rn), r"\[B,N,3\]"),           # ragged without offsets
        (dict(source=torch.zeros(2, 0, 3), nn=torch.zeros(2, 0, dtype=torch.int64)), "non-empty"),
        (dict(nn=nn.float()), "nn must be"), (dict(nn=nn[:, :8]), "nn must be"), (dict(nn=nn.numpy()), "nn must be"),
        (dict(ransac_n=2), "ransac_n"), (dict(ransac_n=9), "ransac_n"), (dict(ransac_n=3.5), "ransac_n"),
        (dict(max_iteration=0), "max_iteration"), (dict(max_iteration=2 ** 24 + 1), "max_iteration"),
        (dict(max_iteration=10.5), "max_iteration"),
        (dict(max_validation=0), "max_validation"), (dict(max_validation=65537), "max_validation"),
        (dict(tau=0.0), "max_correspondence_distance"), (dict(tau=-1.0), "max_correspondence_distance"),
        (dict(tau=float("nan")), "max_correspondence_distance"),
        (dict(checker_distance=-0.1), "checker_distance"), (dict(checker_distance=float("inf")), "checker_distance"),
        (dict(edge_length_threshold=0.0), "edge_length_threshold"), (dict(edge_length_threshold=1.5), "edge_length_threshold"),
        (dict(edge_length_threshold=float("nan")), "edge_length_threshold"),
        (dict(first_pair=-1), "first_pair"),
        (dict(search="kdtree"), "search must be"), (dict(search=1), "search must be"),
        (dict(source_offsets=[0, 16, 32]), "both"),
        (dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 16, 32], target_offsets=[0, 10, 20, 40]), "offsets"),
        (dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, 20, 41]), "target_offsets"),
        (dict(source=rs, target=rt, nn=rn, source_offsets=[0, 16, 32], target_offsets=[0, 30, 20, 40]), "target_offsets"),
    ]
    for kw, msg in bad:
        args = dict(source=s, target=t, nn=nn, tau=0.1)
        args.update(kw)
        a, b, c, tau = args.pop("source"), args.pop("target"), args.pop("nn"), args.pop("tau")
        with pytest.raises(RuntimeError, match=msg):
            F(a, b, c, tau, **args)


def test_wrapper_rejects_the_d_by_n_layout():
    import gmf_amd
    W = gmf_amd.registration_ransac_based_on_feature_matching
    s, t = torch.rand(16, 3), torch.rand(20, 3)
    with pytest.raises(RuntimeError, match="one row per point"):
        W(s, t, torch.rand(33, 16), torch.rand(33, 20), 0.1)
    with pytest.raises(RuntimeError, match="one row per point"):
        W(s.numpy(), t.numpy(), np.zeros((33, 16), np.float32), np.zeros((33, 20), np.float32), 0.1)
    with pytest.raises(RuntimeError, match="differ in width"):
        W(s, t, torch.rand(16, 33), torch.rand(20, 32), 0.1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_no_device_fails_loudly():
    import gmf_amd
    s, t = torch.rand(2, 16, 3), torch.rand(2, 20, 3)
    nn = torch.zeros(2, 16, dtype=torch.int64)
    calls = [
        lambda: gmf_amd.ransac_feature_matching_batched(s, t, nn, 0.1),
        lambda: gmf_amd.ransac_feature_matching_batched(s, t, nn, 0.1, search="brute"),
        lambda: gmf_amd.registration_ransac_based_on_feature_matching(s[0], t[0], torch.rand(16, 8), torch.rand(20, 8), 0.1),
        lambda: gmf_amd.registration_ransac_based_on_feature_matching(s[0].numpy(), t[0].numpy(), torch.rand(16, 8),
                                                                      np.zeros((20, 8), np.float32), 0.1),
    ]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_c_abi_declares_the_entry():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    name = "gmf_ransac_feature_matching"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    assert "#define GMF_ABI_VERSION 5" in text
    assert name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(m.group(1).split(",")) == 30                 # the binding has the header's argument count
    lib = _lib.load_library()
    assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5


def test_dgr_has_the_safeguard_method():
    from gmf_amd import dgr
    assert dgr.DeepGlobalRegistration.SAFEGUARD_METHODS == ("correspondence", "fcgf_feature_matching")
    src = inspect.getsource(dgr.DeepGlobalRegistration.__init__)
    assert 'self.safeguard_method = "correspondence"' in src


def test_restatement_self_test():
    assert FM.self_test()


@pytest.mark.parametrize("seed,ns,nt", [(11, 300, 257), (12, 1000, 777)])
def test_restatement_scenes_meet_the_borderline_cap(seed, ns, nt):
    """The scenes tests/test_gpu_ransac_fm.py uses leave at most 1 % of the hypotheses and 0.5 % of the rows borderline, by the
    restatement alone."""
    tau = 0.1
    src, tgt, nn, _, _, _ = FM.make_scene(seed, ns, nt, tau)
    for kw in (dict(checker_distance=tau), dict(edge_length_threshold=0.9), dict(checker_distance=tau, edge_length_threshold=0.9)):
        res = FM.ransac_fm_np(src, tgt, nn, tau, H=3000, V=32, seed=5, **kw)
        assert len(res["hyp"]) == 32, kw
        assert res["prop"]["border"][:res["hyp"][-1] + 1].mean() <= 0.01, kw
        assert sum(e["border"] for e in res["ev"]) <= 0.005 * ns * len(res["ev"]), kw
