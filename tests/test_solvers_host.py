"""CPU-side checks of the evaluation solvers (gmf_amd/solvers.py): the public names, their argument checks, the no-device error,
the C ABI entries, and the numpy restatement of the RANSAC hypothesis sampler (csrc/ransac_sampler.hpp) that
tests/test_gpu_solvers.py holds the device to."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_U64 = np.uint64
_GOLD = _U64(0x9E3779B97F4A7C15)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + _GOLD
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def ransac_draw(seed, pair, hs, M, n):
    """Rows (numbered among the M participating rows) of hypotheses `hs` of pair `pair`: [len(hs), n] int64.
    key = seed ^ splitmix64(pair << 32 | h); draw c gives u = splitmix64(key ^ c * golden), row = (u >> 32) * M >> 32; one counter c
    runs over the whole sample; a slot redraws while its row repeats an earlier slot's, at most 64 times."""
    hs = np.asarray(hs, dtype=np.uint64)
    key = _U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ splitmix64((_U64(pair) << _U64(32)) | hs)
    c = np.zeros_like(hs)
    rows = np.zeros((hs.size, n), np.int64)
    with np.errstate(over="ignore"):
        for k in range(n):
            pending = np.ones(hs.size, bool)
            for r in range(65):
                u = splitmix64(key ^ (c * _GOLD))
                row = ((u >> _U64(32)) * _U64(M)) >> _U64(32)
                rows[pending, k] = row[pending].astype(np.int64)
                c = np.where(pending, c + _U64(1), c)
                rep = (rows[:, :k] == rows[:, k:k + 1]).any(1)
                pending &= rep
                if r == 64 or not pending.any():
                    break
    return rows


def kabsch_np(A, B):
    """Unweighted Umeyama without scaling in float64 over the last two axes ([..., n, 3]) -> R [..., 3, 3], t [..., 3]."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    ca, cb = A.mean(-2), B.mean(-2)
    H = np.swapaxes(A - ca[..., None, :], -1, -2) @ (B - cb[..., None, :])
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, -1, -2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, -1, -2)))
    D = np.zeros(H.shape)
    D[..., 0, 0] = 1
    D[..., 1, 1] = 1
    D[..., 2, 2] = np.where(d == 0, 1, d)
    R = V @ D @ np.swapaxes(U, -1, -2)
    t = cb - np.einsum("...ij,...j->...i", R, ca)
    return R, t


NAMES = ["ransac_correspondence_batched", "icp_point_to_point_batched", "registration_ransac_based_on_correspondence",
         "registration_icp", "icp_refine", "RegistrationResult"]


def test_public_names_exported():
    import gmf_amd
    for n in NAMES:
        assert hasattr(gmf_amd, n), n
        assert n in gmf_amd.__all__, n
    r = gmf_amd.RegistrationResult(None, None, 0.5, 0.1)
    assert r._fields == ("transformation", "correspondence_set", "fitness", "inlier_rmse")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_no_device_fails_loudly():
    import gmf_amd
    p = torch.rand(2, 16, 3)
    calls = [
        lambda: gmf_amd.ransac_correspondence_batched(p, p, 0.1),
        lambda: gmf_amd.icp_point_to_point_batched(p, p, torch.eye(4).repeat(2, 1, 1), 0.1),
        lambda: gmf_amd.registration_ransac_based_on_correspondence(p[0], p[0], torch.arange(16).repeat(2, 1).t(), 0.1),
        lambda: gmf_amd.registration_icp(p[0], p[1], 0.1),
        lambda: gmf_amd.icp_refine(p, p, torch.eye(4).repeat(2, 1, 1)),
    ]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_ransac_argument_checks():
    import gmf_amd
    R = gmf_amd.ransac_correspondence_batched
    p = torch.rand(2, 16, 3)
    bad = [
        (dict(src=p, tgt=p[:, :8]), "same shape"),
        (dict(src=p.double(), tgt=p.double()), "float32"),
        (dict(src=p[..., :2], tgt=p[..., :2]), r"\[B,N,3\]"),
        (dict(src=p.reshape(-1, 3), tgt=p.reshape(-1, 3)), r"\[B,N,3\]"),          # ragged without offsets
        (dict(src=torch.zeros(0, 5, 3), tgt=torch.zeros(0, 5, 3)), "non-empty"),
        (dict(ransac_n=2), "ransac_n"), (dict(ransac_n=9), "ransac_n"), (dict(ransac_n=3.5), "ransac_n"),
        (dict(num_hypotheses=0), "num_hypotheses"), (dict(num_hypotheses=2 ** 24 + 1), "num_hypotheses"),
        (dict(tau=0.0), "max_correspondence_distance"), (dict(tau=-1.0), "max_correspondence_distance"),
        (dict(tau=float("nan")), "max_correspondence_distance"),
        (dict(mask=torch.ones(2, 16)), "mask"), (dict(mask=torch.ones(2, 15, dtype=torch.bool)), "mask"),
        (dict(src=p.reshape(-1, 3), tgt=p.reshape(-1, 3), offsets=[0, 16]), "offsets"),
        (dict(src=p.reshape(-1, 3), tgt=p.reshape(-1, 3), offsets=[0, 20, 30]), "offsets"),
        (dict(src=p.reshape(-1, 3), tgt=p.reshape(-1, 3), offsets=[0, 16, 16, 32]), "offsets"),
        (dict(src=p.reshape(-1, 3), tgt=p.reshape(-1, 3), offsets=[1, 16, 32]), "offsets"),
        (dict(first_pair=-1), "first_pair"),
    ]
    for kw, msg in bad:
        args = dict(src=p, tgt=p, tau=0.1)
        args.update(kw)
        src, tgt, tau = args.pop("src"), args.pop("tgt"), args.pop("tau")
        with pytest.raises(RuntimeError, match=msg):
            R(src, tgt, tau, **args)


def test_icp_argument_checks():
    import gmf_amd
    I = gmf_amd.icp_point_to_point_batched
    s, t, T0 = torch.rand(2, 16, 3), torch.rand(2, 20, 3), torch.eye(4).repeat(2, 1, 1)
    bad = [
        (dict(target=torch.rand(3, 20, 3)), "same number of pairs"),
        (dict(source=s.double()), "float32"),
        (dict(init=torch.eye(4)), "init"), (dict(init=T0.double()), "init"),
        (dict(tau=0.0), "max_correspondence_distance"),
        (dict(max_iteration=-1), "max_iteration"),
        (dict(relative_fitness=-1.0), "relative_fitness"),
        (dict(source_offsets=[0, 16, 32]), "both"),
        (dict(source=s.reshape(-1, 3), target=t.reshape(-1, 3), source_offsets=[0, 16, 32], target_offsets=[0, 20, 41]),
         "offsets"),
        (dict(source=s.reshape(-1, 3), target=t.reshape(-1, 3), source_offsets=[0, 16, 32], target_offsets=[0, 10, 20, 40]),
         "same number of pairs"),
    ]
    for kw, msg in bad:
        args = dict(source=s, target=t, init=T0, tau=0.1)
        args.update(kw)
        a, b, c, tau = args.pop("source"), args.pop("target"), args.pop("init"), args.pop("tau")
        with pytest.raises(RuntimeError, match=msg):
            I(a, b, c, tau, **args)


def test_sampler_rows_distinct_and_in_range():
    for M, n in [(3, 3), (4, 4), (5, 3), (10, 8), (1000, 3), (8000, 4), (2 ** 31 - 1, 8)]:
        rows = ransac_draw(7, 3, np.arange(4000), M, n)
        assert rows.shape == (4000, n)
        assert rows.min() >= 0 and rows.max() < M
        srt = np.sort(rows, 1)
        assert (srt[:, 1:] != srt[:, :-1]).all(), (M, n)
    # spread: every row of a small pair is drawn, and the slots are not correlated with h in an obvious way
    rows = ransac_draw(0, 0, np.arange(20000), 50, 3)
    assert np.bincount(rows.ravel(), minlength=50).min() > 0.7 * rows.size / 50
    # the sampler depends on the seed and on the pair index
    assert (ransac_draw(1, 0, np.arange(100), 1000, 3) != ransac_draw(2, 0, np.arange(100), 1000, 3)).any()
    assert (ransac_draw(1, 0, np.arange(100), 1000, 3) != ransac_draw(1, 1, np.arange(100), 1000, 3)).any()


def test_sampler_fixed_values():
    """splitmix64 is the published generator (its first outputs from state 0), so the restatement is anchored to it."""
    z = [int(v) for v in splitmix64(np.array([0, 0x9E3779B97F4A7C15], np.uint64))]
    assert z == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


def test_kabsch_restatement():
    r = np.random.default_rng(5)
    A = r.uniform(0, 3, (10, 4, 3))
    q, _ = np.linalg.qr(r.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    B = A @ q.T + np.array([0.1, -0.2, 0.3])
    R, t = kabsch_np(A, B)
    assert np.allclose(R, q, atol=1e-12) and np.allclose(t, [0.1, -0.2, 0.3], atol=1e-12)


def test_c_abi_declares_solvers():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    for name in ("gmf_ransac_correspondence", "gmf_icp_point_to_point"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load_library(), name), name
    assert "#define GMF_ABI_VERSION 5" in text
