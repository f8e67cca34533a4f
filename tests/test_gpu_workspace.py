"""The workspace invariant of the C ABI, family by family: the bytes a call reserves cover the buffers it then carves
(csrc/arena_list.hpp, arena_carve in csrc/api_common.hpp).

Each family runs once normally, then again with every C call starting from a 256-byte caller-provided workspace: the call
answers GMF_ERR_WORKSPACE and says what it needs, the test hands it a torch block of need + 1 MiB announced as `need` bytes,
all of it filled with 0xA5, and the call is repeated.  A buffer carved past the reservation lands in the guard - memory the test
owns - and shows as a changed byte, not as a fault.  The outputs must equal the first run's bit for bit."""
import re

import pytest
import torch

import gmf_amd
from gmf_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 1 << 20
FILL = 0xA5
NO_WORKSPACE = ("gmf_set_tuning", "gmf_get_tuning")


def _g(x):
    return x.to(DEV)


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _flat(x, out):
    """Every tensor (and number) of a nested result, in order."""
    if torch.is_tensor(x):
        out.append(x.detach())
    elif isinstance(x, dict):
        for k in x:
            _flat(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flat(v, out)
    elif isinstance(x, (int, float)):
        out.append(torch.tensor(float(x), dtype=torch.float64))
    elif x is not None:
        raise TypeError(f"unexpected result of type {type(x)}")
    return out


class _Guarded:
    """Replaces Handle._grow_workspace (and makes every call start from a 256-byte workspace, so that each call of a family
    reports its own need) for the length of the `with` block."""

    def __enter__(self):
        self.blocks = []          # (tensor of need + GUARD bytes, need, name of the call)
        self.handles = []
        self.grow0, self.call0 = _lib.Handle._grow_workspace, _lib.Handle.call
        guarded = self

        def grow(h):
            msg = h.lib.gmf_last_error_string(h.h).decode()
            need = int(re.search(r"this call needs (\d+) B", msg).group(1))
            h.check(h.lib.gmf_set_workspace(h.h, None, 0), "gmf_set_workspace")
            ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device=torch.device("cuda", h.device))
            h._ws = ws
            h.check(h.lib.gmf_set_workspace(h.h, ws.data_ptr(), need), "gmf_set_workspace")
            guarded.blocks.append((ws, need, guarded.name))

        def call(h, name, *args):
            if name not in NO_WORKSPACE:
                if h not in guarded.handles:
                    guarded.handles.append(h)
                guarded.name = name
                h._ws = None      # Handle.call then starts from its 256-byte block; the earlier blocks stay alive in `blocks`
            return guarded.call0(h, name, *args)

        _lib.Handle._grow_workspace, _lib.Handle.call = grow, call
        return self

    def __exit__(self, *exc):
        _lib.Handle._grow_workspace, _lib.Handle.call = self.grow0, self.call0
        for h in self.handles:    # the library must not keep a pointer into a block this test frees
            h.lib.gmf_set_workspace(h.h, None, 0)
            h._ws = None


# ---------------------------------------------------------------------------------------------------------------------------
# the families: each returns its outputs (any nesting of tensors)
# ---------------------------------------------------------------------------------------------------------------------------

_MODEL = {}


def _pointdsc():
    if "m" not in _MODEL:
        sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 3, 128), seed=7)
        m = gmf_amd.PointDSC(in_dim=6, num_layers=3, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                             sigma_d=0.10, k=40, nms_radius=0.10)
        m.load_state_dict(sd, strict=False)
        _MODEL["m"] = m.to(DEV).eval()
    return _MODEL["m"]


def _batch(N, seeds=(3, 4), T=40):
    b = synthetic.synthetic_batch(list(seeds), N=N, T=T)
    return {k: _g(v) for k, v in b.items()}


def _forward_uniform():
    m, b = _pointdsc(), _batch(64)
    data = {k: b[k] for k in ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")}
    data["testing"] = True
    res = m(data)
    return res["final_trans"], res["final_labels"], m.last_logits, m.last_features


def _forward_ragged():
    m, b0, b1 = _pointdsc(), _batch(64, seeds=(3,)), _batch(96, seeds=(4,))
    data = {k: [b0[k][0], b1[k][0]] for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["p_tokens"] = torch.cat([b0["p_tokens"], b1["p_tokens"]])
    data["q_tokens"] = torch.cat([b0["q_tokens"], b1["q_tokens"]])
    res = m(data)
    return res["final_trans"], res["final_labels"], res["logits"], m.last_features


def _pick_seeds():
    b = _batch(64)
    return _pointdsc().pick_seeds(None, _g(_rand(2, 64, seed=11)), R=0.10, max_num=6, src_keypts=b["src_keypts"])


def _knn():
    x = torch.nn.functional.normalize(_rand(2, 64, 128, seed=12), dim=-1)
    return gmf_amd.knn(_g(x), 8)


def _nn_match(d):
    F0 = torch.nn.functional.normalize(_rand(70, d, seed=13), dim=-1)
    F1 = torch.nn.functional.normalize(_rand(90, d, seed=14), dim=-1)
    return gmf_amd.nn_match(_g(F0), _g(F1)), gmf_amd.find_knn_gpu(_g(F0), _g(F1), return_distance=True)


def _nn_match_batched(d):
    F0, F1 = _rand(70 + 30, d, seed=15), _rand(90 + 50, d, seed=16)
    return gmf_amd.find_knn_gpu_batch(_g(F0), _g(F1), [(70, 90), (30, 50)], return_distance=True)


def _clouds(B, Ns, Nt, seed):
    """Sources in the unit cube and targets that are a moved, noisy copy of them, padded with unrelated rows."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.rand(B, Ns, 3, generator=gen)
    c, s = 0.9553365, 0.2955202           # cos, sin of 0.3 rad
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    moved = src @ R.T + torch.tensor([0.05, -0.02, 0.03]) + 0.002 * torch.randn(B, Ns, 3, generator=gen)
    tgt = torch.cat([moved, torch.rand(B, max(Nt - Ns, 0), 3, generator=gen)], dim=1)[:, :Nt].contiguous()
    return src, tgt


def _ransac():
    src, tgt = _clouds(2, 100, 100, seed=17)
    tgt[:, 60:] = torch.rand(2, 40, 3, generator=torch.Generator().manual_seed(18))       # outliers
    return gmf_amd.ransac_correspondence_batched(_g(src), _g(tgt), 0.05, num_hypotheses=64, seed=5)


def _icp(search):
    src, tgt = _clouds(2, 80, 120, seed=19)
    init = torch.eye(4).repeat(2, 1, 1)
    return gmf_amd.icp_point_to_point_batched(_g(src), _g(tgt), _g(init), 0.4, search=search)


def _ransac_fm(search):
    src, tgt = _clouds(2, 80, 120, seed=20)
    nn = torch.arange(80).repeat(2, 1)
    nn[:, ::5] = torch.randint(0, 120, (2, 16), generator=torch.Generator().manual_seed(21))    # some wrong matches
    return gmf_amd.ransac_feature_matching_batched(_g(src), _g(tgt), _g(nn), 0.05, max_iteration=64, max_validation=8, seed=6,
                                                   search=search, return_hypotheses=search == "grid")


def _spectral():
    b = _batch(50)
    return gmf_amd.spectral_matching_batched(b["corr_pos"], b["src_keypts"], b["tgt_keypts"], 0.10, return_eigenvector=True)


def _descriptors():
    pts = _g(torch.rand(300, 3, generator=torch.Generator().manual_seed(22)))
    off = [0, 130, 300]
    knn = gmf_amd.radius_knn_batched(pts, off, 0.25, 16)
    normals = gmf_amd.estimate_normals_batched(pts, off, 0.25, max_nn=16)
    return knn, normals, gmf_amd.compute_fpfh_batched(pts, normals, off, 0.35, max_nn=24)


def _voxels():
    pts = _g(torch.rand(300, 3, generator=torch.Generator().manual_seed(23)))
    off = [0, 130, 300]
    return gmf_amd.voxel_down_sample_batched(pts, off, 0.2), gmf_amd.voxel_select_batched(pts, off, 0.2)


def _losses():
    b = _batch(64)
    fn = _g(torch.nn.functional.normalize(_rand(2, 64, 128, seed=24), dim=-1))
    gt, pred = b["gt_labels"], _g(_rand(2, 64, seed=25))
    M = gmf_amd.similarity_matrix(fn, 0.8)
    cl = gmf_amd.ClassificationLoss()(pred, gt)
    sm = gmf_amd.SpectralMatchingLoss()(M, gt)
    tl = gmf_amd.TransformationLoss()(b["gt_trans"], b["gt_trans"], b["src_keypts"], b["tgt_keypts"], torch.sigmoid(pred))
    f = fn.clone().requires_grad_(True)
    sigma = torch.tensor([0.8], device=DEV, requires_grad=True)
    loss = gmf_amd.SpectralMatchingLoss().from_features(f, sigma, gt)
    loss.backward()
    return M, cl, sm, tl, loss, f.grad, sigma.grad


def _fusion_train():
    m = gmf_amd.FusionLayer(depth=0, dim=128, latent_dim=128, cross_heads=1, latent_heads=8, cross_dim_head=64, latent_dim_head=64)
    m.load_state_dict(synthetic.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=31))
    m = m.to(DEV).train()
    x = _g(_rand(2, 64, 128, seed=26)).requires_grad_(True)
    ctx = _g(_rand(2, 8, 128, seed=27)).requires_grad_(True)
    y = m(ctx, queries_encoder=x)
    y.backward(_g(_rand(2, 64, 128, seed=28)))
    return y, x.grad, ctx.grad, [p.grad for p in m.parameters()]


FAMILIES = {
    "pointdsc_forward": _forward_uniform,
    "pointdsc_forward_ragged": _forward_ragged,
    "pick_seeds_nms": _pick_seeds,
    "knn_k8": _knn,
    "nn_match_d32": lambda: _nn_match(32),
    "nn_match_d33": lambda: _nn_match(33),
    "nn_match_batched_d32": lambda: _nn_match_batched(32),
    "nn_match_batched_d33": lambda: _nn_match_batched(33),
    "ransac_correspondence": _ransac,
    "icp_brute": lambda: _icp("brute"),
    "icp_grid": lambda: _icp("grid"),
    "ransac_feature_matching_brute": lambda: _ransac_fm("brute"),
    "ransac_feature_matching_grid": lambda: _ransac_fm("grid"),
    "spectral_matching": _spectral,
    "radius_knn_normals_fpfh": _descriptors,
    "voxel_grids": _voxels,
    "similarity_and_losses": _losses,
    "fusion_layer_train": _fusion_train,
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_reservation_covers_carving(family):
    run = FAMILIES[family]
    want = _flat(run(), [])
    torch.cuda.synchronize()
    with _Guarded() as guarded:
        got = _flat(run(), [])
        torch.cuda.synchronize()
    assert guarded.blocks, f"{family}: no call of the family asked for workspace"
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{family}: output {i} differs between the two runs"
    for ws, need, name in guarded.blocks:
        print(f"{family}: {name} needs {need} B")
        touched = int((ws[need:] != FILL).sum())
        assert touched == 0, f"{family}: {name} reserved {need} B and wrote {touched} bytes behind them"
    gmf_amd.check_status()
