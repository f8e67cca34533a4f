"""CPU-side checks of the maximum-clique baseline (gmf_amd/clique.py: max_clique_batched, PMC, compatibility_graph): the public
names and signatures, the argument checks (the spectral-matching baseline's, in kind), the no-device error, the C ABI entries, and
the exact restatement (tests/clique_reference.py) that tests/test_gpu_clique.py holds the device to."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import clique_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_exported():
    import gmf_amd
    for n in ("max_clique_batched", "PMC", "compatibility_graph"):
        assert hasattr(gmf_amd, n), n
        assert n in gmf_amd.__all__, n
    sig = inspect.signature(gmf_amd.max_clique_batched)
    assert list(sig.parameters) == ["corr", "src_keypts", "tgt_keypts", "inlier_threshold", "metric", "offsets", "max_steps",
                                    "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["metric"], d["offsets"], d["max_steps"], d["return_info"]) == ("squared", None, None, False)
    assert list(inspect.signature(gmf_amd.PMC).parameters) == ["corr", "src_keypts", "tgt_keypts", "args"]
    sig = inspect.signature(gmf_amd.compatibility_graph)
    assert list(sig.parameters) == ["corr", "inlier_threshold", "metric"] and sig.parameters["metric"].default == "squared"
    from gmf_amd import clique
    assert isinstance(clique.STEP_SLACK, int) and clique.STEP_SLACK >= 1
    assert isinstance(clique.DEFAULT_MAX_STEPS, int) and clique.DEFAULT_MAX_STEPS % 64 == 0      # 64 x a measured count


def test_argument_checks_match_spectral_matching_in_kind():
    import gmf_amd
    c, s, t = torch.rand(2, 16, 6), torch.rand(2, 16, 3), torch.rand(2, 16, 3)
    rc, rs, rt = c.reshape(-1, 6), s.reshape(-1, 3), t.reshape(-1, 3)
    ragged = dict(corr=rc, src=rs, tgt=rt)
    shared = [
        (dict(corr=c.double()), "float32"), (dict(src=s.double()), "float32"), (dict(tgt=t.half()), "float32"),
        (dict(corr=c.numpy()), "torch tensor"),
        (dict(corr=c[..., :5]), r"\[B,N,6\]"), (dict(src=s[..., :2]), r"\[B,N,3\]"), (dict(tgt=torch.rand(2, 16, 6)), r"\[B,N,3\]"),
        (dict(corr=rc), r"\[B,N,6\]"), (dict(offsets=[0, 16, 32]), r"\[sum N,6\]"),
        (dict(src=s[:, :8]), "equal row counts"), (dict(tgt=t[:1]), "equal row counts"),
        (dict(corr=torch.zeros(0, 4, 6), src=torch.zeros(0, 4, 3), tgt=torch.zeros(0, 4, 3)), "at least one pair"),
        (dict(ragged, offsets=[0, 16]), "offsets"), (dict(ragged, offsets=[1, 16, 32]), "offsets"),
        (dict(ragged, offsets=[0, 20, 16, 32]), "offsets"), (dict(ragged, offsets=[0, 16, 33]), "offsets"),
        (dict(ragged, offsets=[32]), "offsets"), (dict(ragged, offsets=[0, "a", 32]), "offsets"),
        (dict(thr=0.0), "inlier_threshold"), (dict(thr=-0.1), "inlier_threshold"), (dict(thr=float("nan")), "inlier_threshold"),
        (dict(thr=float("inf")), "inlier_threshold"),
    ]
    own = [(dict(metric="l2"), "metric"), (dict(metric=0), "metric"), (dict(max_steps=0), "max_steps"),
           (dict(max_steps=2.5), "max_steps"), (dict(max_steps=-3), "max_steps")]
    for F, cases in ((gmf_amd.max_clique_batched, shared + own), (gmf_amd.spectral_matching_batched, shared)):
        for kw, msg in cases:
            args = dict(corr=c, src=s, tgt=t, thr=0.1)
            args.update(kw)
            a, b, d, thr = args.pop("corr"), args.pop("src"), args.pop("tgt"), args.pop("thr")
            with pytest.raises(RuntimeError, match=msg) as e:
                F(a, b, d, thr, **args)
            assert F.__name__ in str(e.value)
    ns = types.SimpleNamespace(inlier_threshold=0.1)
    with pytest.raises(RuntimeError, match=r"\[1,N,6\]"):
        gmf_amd.PMC(c, s, t, ns)
    with pytest.raises(RuntimeError, match=r"\[1,N,6\]"):
        gmf_amd.PMC(rc, rs, rt, ns)
    for kw, msg in ((dict(corr=rc.double()), "float32"), (dict(corr=c), r"\[sum N,6\]"), (dict(thr=0.0), "inlier_threshold"),
                    (dict(metric="l1"), "metric")):
        args = dict(corr=rc, thr=0.1)
        args.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            gmf_amd.compatibility_graph(args.pop("corr"), args.pop("thr"), **args)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_no_device_fails_loudly():
    import gmf_amd
    c, s, t = torch.rand(1, 16, 6), torch.rand(1, 16, 3), torch.rand(1, 16, 3)
    calls = [
        lambda: gmf_amd.max_clique_batched(c, s, t, 0.1),
        lambda: gmf_amd.max_clique_batched(c[0], s[0], t[0], 0.1, offsets=[0, 8, 8, 16], metric="length"),
        lambda: gmf_amd.PMC(c, s, t, types.SimpleNamespace(inlier_threshold=0.1)),
        lambda: gmf_amd.compatibility_graph(c[0], 0.1),
    ]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_c_abi_declares_the_entries():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert "#define GMF_ABI_VERSION 5" in text
    want = {
        "gmf_max_clique": ["h", "corr", "src", "tgt", "offsets", "B", "total_rows", "max_n", "inlier_threshold", "metric",
                           "max_steps", "labels_out", "T_out", "size_out", "exact_out", "steps_out", "degree_out", "stream"],
        "gmf_pmc_graph": ["h", "corr", "offsets", "B", "total_rows", "max_n", "inlier_threshold", "metric", "bits_out",
                          "degree_out", "stream"],
    }
    lib = _lib.load_library()
    for name, params in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == params
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(params)                  # the binding has the header's argument count
        assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5


def test_restatement_edge_cases():
    assert CR.self_test()


def test_restatement_recomputes_the_table():
    """The cases of tests/test_gpu_clique.py: some graphs have ties (so membership is the check) and some have one answer, the
    sets of maximum cliques stay small, and under the length metric the planted inliers are the one maximum clique."""
    counts = {}
    for seed, N in CR.TABLE:
        for kind in ("3dmatch", "kitti"):
            _, A, omega, cliques, steps = CR.reference(seed, N, kind)
            assert 0 < len(cliques) < CR.MAX_TIES and all(len(c) == omega for c in cliques)
            counts[(seed, kind)] = len(cliques)
            print(f"seed {seed} N {N} {kind}: omega {omega}, {len(cliques)} maximum cliques, {steps} branch steps")
    assert min(counts.values()) == 1 < max(counts.values())             # both kinds of case are served: one answer, and ties
    for kind in ("3dmatch", "kitti"):
        case, A, omega, cliques, _ = CR.reference(3, 257, kind, "length")
        gt = tuple(np.flatnonzero(case[4]).tolist())
        assert cliques == {gt} and omega == len(gt)
