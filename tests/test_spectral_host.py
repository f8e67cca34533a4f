"""CPU-side checks of the spectral-matching baseline (gmf_amd/spectral.py: spectral_matching_batched, SM): the public names and
signatures, every argument check, the no-device error, the C ABI entry, and the float64 restatement (tests/spectral_reference.py)
that tests/test_gpu_spectral.py holds the device to - against the golden fixture written from the reference's own SM
(tests/tools/make_sm_golden.py) and on its edge cases."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import spectral_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_exported():
    import gmf_amd
    for n in ("spectral_matching_batched", "SM"):
        assert hasattr(gmf_amd, n), n
        assert n in gmf_amd.__all__, n
    sig = inspect.signature(gmf_amd.spectral_matching_batched)
    assert list(sig.parameters) == ["corr", "src_keypts", "tgt_keypts", "inlier_threshold", "top_ratio", "num_iterations", "offsets",
                                    "return_eigenvector", "_col_splits"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["top_ratio"], d["num_iterations"], d["offsets"], d["return_eigenvector"], d["_col_splits"]) == (0.1, 10, None, False, None)
    sig = inspect.signature(gmf_amd.SM)
    assert list(sig.parameters) == ["corr", "src_keypts", "tgt_keypts", "args", "top_ratio"]
    assert sig.parameters["top_ratio"].default == 0.1
    assert "argsort" in gmf_amd.spectral_matching_batched.__doc__      # the ties the reference leaves open are spelled out


def test_argument_checks():
    import gmf_amd
    F = gmf_amd.spectral_matching_batched
    c, s, t = torch.rand(2, 16, 6), torch.rand(2, 16, 3), torch.rand(2, 16, 3)
    rc, rs, rt = c.reshape(-1, 6), s.reshape(-1, 3), t.reshape(-1, 3)
    ragged = dict(corr=rc, src=rs, tgt=rt)
    bad = [
        (dict(corr=c.double()), "float32"), (dict(src=s.double()), "float32"), (dict(tgt=t.half()), "float32"),
        (dict(corr=c.numpy()), "torch tensor"),
        (dict(corr=c[..., :5]), r"\[B,N,6\]"), (dict(src=s[..., :2]), r"\[B,N,3\]"), (dict(tgt=torch.rand(2, 16, 6)), r"\[B,N,3\]"),
        (dict(corr=rc), r"\[B,N,6\]"),                                                    # packed without offsets
        (dict(offsets=[0, 16, 32]), r"\[sum N,6\]"),                                      # offsets with [B,N,.]
        (dict(src=s[:, :8]), "equal row counts"), (dict(tgt=t[:1]), "equal row counts"),
        (dict(corr=torch.zeros(0, 4, 6), src=torch.zeros(0, 4, 3), tgt=torch.zeros(0, 4, 3)), "at least one pair"),
        (dict(ragged, offsets=[0, 16]), "offsets"), (dict(ragged, offsets=[1, 16, 32]), "offsets"),
        (dict(ragged, offsets=[0, 20, 16, 32]), "offsets"), (dict(ragged, offsets=[0, 16, 33]), "offsets"),
        (dict(ragged, offsets=[32]), "offsets"), (dict(ragged, offsets=[0, "a", 32]), "offsets"),
        (dict(thr=0.0), "inlier_threshold"), (dict(thr=-0.1), "inlier_threshold"), (dict(thr=float("nan")), "inlier_threshold"),
        (dict(thr=float("inf")), "inlier_threshold"),
        (dict(top_ratio=-0.01), "top_ratio"), (dict(top_ratio=1.01), "top_ratio"), (dict(top_ratio=float("nan")), "top_ratio"),
        (dict(num_iterations=0), "num_iterations"), (dict(num_iterations=1001), "num_iterations"),
        (dict(num_iterations=2.5), "num_iterations"),
        (dict(_col_splits=0), "_col_splits"), (dict(_col_splits=33), "_col_splits"), (dict(_col_splits=1.5), "_col_splits"),
    ]
    for kw, msg in bad:
        args = dict(corr=c, src=s, tgt=t, thr=0.1)
        args.update(kw)
        a, b, d, thr = args.pop("corr"), args.pop("src"), args.pop("tgt"), args.pop("thr")
        with pytest.raises(RuntimeError, match=msg):
            F(a, b, d, thr, **args)
    with pytest.raises(RuntimeError, match=r"\[1,N,6\]"):
        gmf_amd.SM(c, s, t, types.SimpleNamespace(inlier_threshold=0.1))              # B = 1, as the reference implies
    with pytest.raises(RuntimeError, match=r"\[1,N,6\]"):
        gmf_amd.SM(rc, rs, rt, types.SimpleNamespace(inlier_threshold=0.1))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_no_device_fails_loudly():
    import gmf_amd
    c, s, t = torch.rand(1, 16, 6), torch.rand(1, 16, 3), torch.rand(1, 16, 3)
    calls = [
        lambda: gmf_amd.spectral_matching_batched(c, s, t, 0.1),
        lambda: gmf_amd.spectral_matching_batched(c[0], s[0], t[0], 0.1, offsets=[0, 8, 8, 16]),
        lambda: gmf_amd.SM(c, s, t, types.SimpleNamespace(inlier_threshold=0.1)),
    ]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_c_abi_declares_the_entry():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    name = "gmf_spectral_matching"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    assert "#define GMF_ABI_VERSION 5" in text
    params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["h", "corr", "src", "tgt", "offsets", "B", "max_n", "inlier_threshold", "topk", "iterations", "eig_out",
                      "labels_out", "T_out", "stream"]
    assert name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(params)                                      # the binding has the header's argument count
    lib = _lib.load_library()
    assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5


@pytest.mark.parametrize("kind", ["3dmatch", "kitti"])
def test_restatement_matches_the_golden_fixture(kind, golden_dir):
    """The fixture holds what the reference's SM returned in fp32.  Labels are equal; eig and trans are within 4 x the fp32 floor
    of the case as measured here (the dense fp32 form against float64): the fixture is one run of that arithmetic, and the factor
    covers another summation order of the host's matrix products and another 3 x 3 SVD."""
    g = np.load(os.path.join(golden_dir, "sm_baseline.npz"))
    seed, N, thr, ratio = g[kind + "_args"]
    assert (thr, ratio) == SR.KINDS[kind]
    key = (int(seed), int(N), kind)
    _, r64, r32 = SR.reference(*key)
    assert r64["k"] == int(g[kind + "_labels"].sum()) > 0
    assert np.array_equal(r64["labels"], g[kind + "_labels"])
    floor = SR.floor(key)
    err = SR.eig_error(g[kind + "_eig"], r64["eig"])
    print(f"{kind}: eig floor {floor:.3e}, fixture {err:.3e}")
    assert 0 < floor < 2e-6 and err <= 4 * floor
    tfloor = np.abs(r32["trans"] - r64["trans"]).max()
    terr = np.abs(g[kind + "_trans"] - r64["trans"]).max()
    print(f"{kind}: trans floor {tfloor:.3e}, fixture {terr:.3e}")
    assert terr <= 4 * tfloor
    assert np.array_equal(r64["labels"], r32["labels"])


def test_restatement_edge_cases():
    assert SR.self_test()


@pytest.mark.parametrize("kind", ["3dmatch", "kitti"])
@pytest.mark.parametrize("N", [64, 257, 1000])
def test_cases_are_far_from_a_label_tie(N, kind):
    """The cases of tests/test_gpu_spectral.py: the gap between the k-th and (k+1)-th value is at least 16 x the fp32 floor."""
    key = (1, N, kind)
    _, r64, _ = SR.reference(*key)
    assert 0 < r64["k"] < N and r64["gap"] >= 16 * SR.floor(key), (r64["gap"], SR.floor(key))
