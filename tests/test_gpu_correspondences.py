"""GPU tests of the correspondence chain (gmf_amd/correspondences.py, csrc/correspondence_kernels.hip): nn_match_mutual and
build_correspondences against the float64 restatement of tests/correspondence_reference.py - exactly where the result is an index,
a flag, a label or a gather, and within the worked-out fp32 bound where it is a mean - and against nn_match bit for bit."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import matching, synthetic
from gmf_amd._util import handle_and_stream

import correspondence_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
THR = R.INLIER_THRESHOLD


def _g(x):
    return torch.as_tensor(x).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def _clean_status():
    yield
    gmf_amd.check_status()


@functools.lru_cache(maxsize=None)
def _fixture(d):
    """The shared batch at width d with its two preconditions asserted, its float64 results (mutual and unfiltered), and the device
    copies.  Built once per width and never written to."""
    fx = R.make_fixture(d, R.SEEDS[d])
    gap, bound, margin = R.check_fixture(fx, THR)
    print(f"fixture d={d}: smallest top-2 gap {gap:.3e} (bound {bound:.3e}), label margin {margin:.4f}")
    assert gap > bound, (d, gap, bound)                     # twice the worst fp32 error of the two scores compared
    assert margin > 1e-4, (d, margin)
    args = (fx["src_keypts"], fx["tgt_keypts"], fx["src_desc"], fx["tgt_desc"], fx["len_batch"])
    fx["ref"], fx["ref_off"] = R.build_batch(*args, True, fx["gt_trans"], THR)
    fx["ref_all"], fx["ref_all_off"] = R.build_batch(*args, False, fx["gt_trans"], THR)
    fx["off0"] = np.r_[0, np.cumsum([a for a, _ in fx["len_batch"]])].astype(int)
    fx["off1"] = np.r_[0, np.cumsum([b for _, b in fx["len_batch"]])].astype(int)
    fx["dev"] = {k: _g(fx[k]) for k in ("src_keypts", "tgt_keypts", "src_desc", "tgt_desc", "gt_trans")}
    return fx


def _build(fx, **kw):
    v = fx["dev"]
    kw.setdefault("gt_trans", v["gt_trans"])
    if kw["gt_trans"] is not None:
        kw.setdefault("inlier_threshold", THR)
    return gmf_amd.build_correspondences(v["src_keypts"], v["tgt_keypts"], v["src_desc"], v["tgt_desc"], fx["len_batch"], **kw)


def _gaps_clear(D, bound):
    """Every row's and column's two largest entries are equal (a tie made on purpose) or further apart than bound."""
    for A in (D, D.T):
        if A.shape[1] >= 2:
            top = np.sort(A, axis=1)[:, -2:]
            g = top[:, 1] - top[:, 0]
            if ((g != 0) & (g <= bound)).any():
                return False
    return True


def _unit_rows(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- 1. nn_match_mutual ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", R.WIDTHS)
def test_mutual_matching_on_the_fixture(d):
    fx = _fixture(d)
    v = fx["dev"]
    idx, dis, mut = gmf_amd.nn_match_mutual(v["src_desc"], v["tgt_desc"], fx["len_batch"])
    assert idx.dtype == torch.int64 and dis.dtype == torch.float32 and mut.dtype == torch.bool
    assert np.array_equal(_n(idx), np.concatenate([p["source_idx"] for p in fx["ref"]]))
    assert np.array_equal(_n(mut), np.concatenate([p["mutual"] for p in fx["ref"]]))
    # the row side is the existing kernel's: bit for bit the batched mode-0 matching, and nn_match of every pair
    bidx, bdis, _, _ = matching._match_batched(v["src_desc"], v["tgt_desc"], fx["len_batch"], 0, False, "test")
    assert torch.equal(idx, bidx.long()) and torch.equal(dis.view(torch.int32), bdis.view(torch.int32))
    o0, o1 = fx["off0"], fx["off1"]
    for b, (ns, nt) in enumerate(fx["len_batch"]):
        if ns:
            i1, d1 = gmf_amd.nn_match(v["src_desc"][o0[b]:o0[b + 1]], v["tgt_desc"][o1[b]:o1[b + 1]])
            assert torch.equal(idx[o0[b]:o0[b + 1]], i1) and torch.equal(dis[o0[b]:o0[b + 1]].view(torch.int32), d1.view(torch.int32))


@pytest.mark.parametrize("d", [32, 33])
def test_mutual_matching_indices_on_the_reference_golden(golden_dir, d):
    g = np.load(os.path.join(golden_dir, "f12_descriptor_matching.npz"))
    idx, dis, mut = gmf_amd.nn_match_mutual(_g(g[f"F0_{d}"]), _g(g[f"F1_{d}"]))
    assert np.array_equal(_n(idx), g[f"pdsc_idx_{d}"])
    assert np.abs(_n(dis) - g[f"pdsc_dis_{d}"]).max() < 1e-4
    assert mut.shape == idx.shape


# ---- 2. ties, on bitwise-equal rows ----------------------------------------------------------------------------------------------------

def _tie_data(ns, nt, far_s, far_t):
    rng = np.random.default_rng(11)
    S, T = _unit_rows(rng.standard_normal((ns, 32))), _unit_rows(rng.standard_normal((nt, 32)))
    T[30] = T[3]
    S[5] = T[3]
    if far_t is not None:
        T[far_t] = T[3]
    return S, T


@pytest.mark.parametrize("ns,nt,far_s,far_t", [(40, 40, 9, None), (300, 200, 200, 150)])
def test_ties_go_to_the_smaller_index_on_both_sides(ns, nt, far_s, far_t):
    """(40, 40): one tile.  (300, 200): the tied source row sits in another workgroup (row 200: tile 6) and a third copy of the key
    in another stage (key 150), so the tie is settled by the atomics' index half, whatever order they arrive in."""
    S, T = _tie_data(ns, nt, far_s, far_t)
    bound = 4 * 32 * 2.0 ** -24
    assert _gaps_clear(R.dots(S, T, exact_ties=True), bound)
    si, ti = R.argmin_both(S, T, exact_ties=True)
    idx, _, mut = gmf_amd.nn_match_mutual(_g(S), _g(T))
    idx, mut = _n(idx), _n(mut)
    assert idx[5] == 3 and mut[5] and not (idx == 30).any()          # row 5 pairs with key 3; nothing pairs with key 30
    if far_t is not None:
        assert not (idx == far_t).any()
    assert np.array_equal(idx, si) and np.array_equal(mut, R.mutual_mask(si, ti))
    S[far_s] = S[5]                                                    # a second source row equal to row 5
    assert _gaps_clear(R.dots(S, T, exact_ties=True), bound)
    si, ti = R.argmin_both(S, T, exact_ties=True)
    idx, _, mut = gmf_amd.nn_match_mutual(_g(S), _g(T))
    idx, mut = _n(idx), _n(mut)
    assert idx[5] == 3 and idx[far_s] == 3 and mut[5] and not mut[far_s]
    assert np.array_equal(idx, si) and np.array_equal(mut, R.mutual_mask(si, ti))


# ---- 3. all dot products negative: a zero-padded source row would win every column --------------------------------------------------

def test_padding_rows_stay_out_of_the_column_fold():
    rng = np.random.default_rng(5)
    S = _unit_rows(np.abs(rng.standard_normal((33, 32))))
    T = -_unit_rows(np.abs(rng.standard_normal((40, 32))))
    D = R.dots(S, T)
    assert D.max() < 0 and _gaps_clear(D, 4 * 32 * 2.0 ** -24)
    si, ti = R.argmin_both(S, T)
    want = R.mutual_mask(si, ti)
    assert want.any()
    idx, _, mut = gmf_amd.nn_match_mutual(_g(S), _g(T))
    assert np.array_equal(_n(idx), si) and np.array_equal(_n(mut), want)


# ---- 4. a NaN source row ----------------------------------------------------------------------------------------------------------------

def test_nan_source_row_is_not_mutual_and_hurts_nobody_else():
    fx = _fixture(32)
    lens = fx["len_batch"][:5]                                        # (301, 700), (5, 3), (1, 40), (0, 20), (64, 64)
    n0, n1 = fx["off0"][5], fx["off1"][5]
    S, T = fx["src_desc"][:n0].copy(), fx["tgt_desc"][:n1]
    bad = 7                                                            # a noisy copy: mutual in the clean data
    assert fx["ref"][0]["mutual"][bad]
    idx0, dis0, mut0 = gmf_amd.nn_match_mutual(_g(S), _g(T), lens)
    S[bad] = np.nan
    idx1, dis1, mut1 = gmf_amd.nn_match_mutual(_g(S), _g(T), lens)
    idx0, dis0, mut0, idx1, dis1, mut1 = (_n(t) for t in (idx0, dis0, mut0, idx1, dis1, mut1))
    assert not mut1[bad] and np.isnan(dis1[bad])
    others = np.arange(n0) != bad
    assert np.array_equal(idx0[others], idx1[others]) and np.array_equal(dis0[others].view(np.int32), dis1[others].view(np.int32))
    # the NaN row was the winner of some columns; every other row's flag is unchanged wherever it was not
    ti = R.argmin_both(fx["src_desc"][:301], fx["tgt_desc"][:700])[1]
    touched = np.zeros(n0, bool)
    touched[:301] = ti[idx0[:301]] == bad
    keep = others & ~touched
    assert np.array_equal(mut0[keep], mut1[keep])
    # and everywhere the flags are those of the pair without that row
    rest = np.delete(fx["src_desc"][:301], bad, 0)
    assert _gaps_clear(R.dots(rest, fx["tgt_desc"][:700]), 4 * 32 * 2.0 ** -24)
    si, ti = R.argmin_both(rest, fx["tgt_desc"][:700])
    assert np.array_equal(np.delete(mut1[:301], bad), R.mutual_mask(si, ti))


# ---- 5. build_correspondences ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", R.WIDTHS)
def test_build_correspondences_on_the_fixture(d):
    fx = _fixture(d)
    v = fx["dev"]
    out = _build(fx, gather_desc=True)
    ref, off = fx["ref"], fx["ref_off"]
    M = int(off[-1])
    assert out["n_points"] == np.diff(off).tolist() and isinstance(out["n_points"], list)
    assert out["offsets"].dtype == torch.int32 and out["offsets"].is_cuda and np.array_equal(_n(out["offsets"]), off)
    assert out["corr"].dtype == torch.int64 and np.array_equal(_n(out["corr"]), np.concatenate([p["corr"] for p in ref]))
    assert np.array_equal(_n(out["gt_labels"]), np.concatenate([p["gt_labels"] for p in ref])) and out["gt_labels"].dtype == torch.float32
    for k in ("corr_pos", "src_keypts", "tgt_keypts", "src_desc", "tgt_desc", "gt_labels", "corr"):
        assert out[k].shape[0] == M
    src_rows = np.concatenate([p["corr"][:, 0] + fx["off0"][b] for b, p in enumerate(ref)])
    tgt_rows = np.concatenate([p["corr"][:, 1] + fx["off1"][b] for b, p in enumerate(ref)])
    for k, base, rows in (("src_keypts", "src_keypts", src_rows), ("tgt_keypts", "tgt_keypts", tgt_rows),
                          ("src_desc", "src_desc", src_rows), ("tgt_desc", "tgt_desc", tgt_rows)):
        assert np.array_equal(_n(out[k]).view(np.int32), fx[base][rows].view(np.int32)), k               # bit-equal gathers
    pos = _n(out["corr_pos"]).astype(np.float64)
    for b, p in enumerate(ref):
        m = len(p["corr"])
        if m:
            # an fp32 sum of m terms in any order, the division and the subtraction: (m + 2) 2^-24 max|x|
            xmax = max(np.abs(p["src_keypts"]).max(), np.abs(p["tgt_keypts"]).max())
            err = np.abs(pos[off[b]:off[b + 1]] - p["corr_pos"]).max()
            print(f"d={d} pair {b}: M={m} corr_pos error {err:.3e}, bound {(m + 2) * 2.0 ** -24 * xmax:.3e}")
            assert err <= (m + 2) * 2.0 ** -24 * xmax, (b, err)
    # in_dim 3: source minus target, not centred, bit for bit
    out3 = _build(fx, in_dim=3)
    assert out3["corr_pos"].shape == (M, 3) and torch.equal(out3["corr"], out["corr"])
    assert torch.equal(out3["corr_pos"].view(torch.int32), (out["src_keypts"] - out["tgt_keypts"]).view(torch.int32))
    # without the mutual filter: every source row, its match that of nn_match
    every = _build(fx, use_mutual=False)
    assert every["n_points"] == [a for a, _ in fx["len_batch"]]
    bidx, _, _, _ = matching._match_batched(v["src_desc"], v["tgt_desc"], fx["len_batch"], 0, False, "test")
    assert torch.equal(every["corr"][:, 1], bidx.long())
    assert np.array_equal(_n(every["corr"]), np.concatenate([p["corr"] for p in fx["ref_all"]]))
    assert np.array_equal(_n(every["gt_labels"]), np.concatenate([p["gt_labels"] for p in fx["ref_all"]]))
    # no labels without gt_trans
    assert "gt_labels" not in _build(fx, gt_trans=None) and "src_desc" not in out3


# ---- 6. batch invariance and repeatability ---------------------------------------------------------------------------------------------

KEYS = ("corr", "corr_pos", "src_keypts", "tgt_keypts", "gt_labels", "src_desc", "tgt_desc")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("d", [32, 128])
def test_a_pair_alone_gives_the_bits_it_gives_in_the_batch(d):
    fx = _fixture(d)
    v = fx["dev"]
    out = _build(fx, gather_desc=True)
    again = _build(fx, gather_desc=True)
    assert out["n_points"] == again["n_points"] and all(_same_bits(out[k], again[k]) for k in KEYS)
    off, o0, o1 = _n(out["offsets"]), fx["off0"], fx["off1"]
    for b, (ns, nt) in enumerate(fx["len_batch"]):
        one = gmf_amd.build_correspondences(v["src_keypts"][o0[b]:o0[b + 1]], v["tgt_keypts"][o1[b]:o1[b + 1]],
                                            v["src_desc"][o0[b]:o0[b + 1]], v["tgt_desc"][o1[b]:o1[b + 1]], None, True,
                                            v["gt_trans"][b], THR, 6, True)
        assert one["n_points"] == [out["n_points"][b]]
        for k in KEYS:
            assert _same_bits(one[k], out[k][off[b]:off[b + 1]]), (b, k)


# ---- 7. the dict feeds PointDSC's ragged forward ----------------------------------------------------------------------------------------

def test_pointdsc_takes_the_returned_dict():
    fx = _fixture(32)
    out = _build(fx)
    model = gmf_amd.PointDSC(in_dim=6, num_layers=2, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                             sigma_d=0.10, k=10, nms_radius=0.10)
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 2, 128), seed=7)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.image_encoder.") for k in missing)
    model = model.to(DEV).eval()
    # the caller drops what the network cannot take: empty pairs, and here the pairs with no more correspondences than the pose
    # head's k neighbours ((5, 3) and (1, 40))
    off = _n(out["offsets"])
    kept = [b for b, m in enumerate(out["n_points"]) if m > 10]
    assert [b for b, m in enumerate(out["n_points"]) if m == 0] and len(kept) >= 5
    rows = torch.cat([torch.arange(off[b], off[b + 1], device=DEV) for b in kept])
    data = {k: out[k][rows].contiguous() for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["n_points"] = [out["n_points"][b] for b in kept]
    g = torch.Generator().manual_seed(3)
    data["p_tokens"] = _g(torch.randn(len(kept), 40, 128, generator=g))
    data["q_tokens"] = _g(torch.randn(len(kept), 40, 128, generator=g))
    res = model(data)
    assert res["final_trans"].shape == (len(kept), 4, 4) and bool(torch.isfinite(res["final_trans"]).all())
    assert [int(t.shape[0]) for t in res["final_labels"]] == data["n_points"]


# ---- 8. graph capture of the C entry ------------------------------------------------------------------------------------------------------

def test_graph_capture_of_the_c_entry_replays_the_eager_bits():
    fx = _fixture(32)
    v = fx["dev"]
    B, cap, d = len(fx["len_batch"]), int(fx["off0"][-1]), 32
    off0 = (ctypes.c_int * (B + 1))(*[int(x) for x in fx["off0"]])
    off1 = (ctypes.c_int * (B + 1))(*[int(x) for x in fx["off1"]])

    def buffers():
        return {"offsets": torch.zeros(B + 1, device=DEV, dtype=torch.int32), "corr": torch.zeros((cap, 2), device=DEV, dtype=torch.int64),
                "src": torch.zeros((cap, 3), device=DEV), "tgt": torch.zeros((cap, 3), device=DEV), "pos": torch.zeros((cap, 6), device=DEV),
                "sdesc": torch.zeros((cap, d), device=DEV), "tdesc": torch.zeros((cap, d), device=DEV), "labels": torch.zeros(cap, device=DEV)}

    def run(o):
        h, st = handle_and_stream(v["src_desc"])
        h.call("gmf_build_correspondences", v["src_desc"].data_ptr(), v["tgt_desc"].data_ptr(), v["src_keypts"].data_ptr(),
               v["tgt_keypts"].data_ptr(), off0, off1, B, d, 1, 6, v["gt_trans"].data_ptr(), THR, o["offsets"].data_ptr(),
               o["corr"].data_ptr(), o["src"].data_ptr(), o["tgt"].data_ptr(), o["pos"].data_ptr(), o["sdesc"].data_ptr(),
               o["tdesc"].data_ptr(), o["labels"].data_ptr(), st)

    eager, captured = buffers(), buffers()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                   # (also sizes the workspace before the capture)
            run(eager)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(_n(eager["offsets"]), fx["ref_off"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(captured)
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert _same_bits(eager[k], captured[k]), k
    for t in captured.values():                              # a replay writes everything again
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert _same_bits(eager[k], captured[k]), k


# ---- 9. the handle's ring of pinned table slots: wrap-around and regrowth -------------------------------------------------------------

def _ring_batch(len_batch, seed):
    """A batch from the fixture recipe (no top-2 gap within the fp32 error of the scores) as the C entry takes it."""
    fx = R.make_fixture(32, seed, len_batch)
    gap, bound, _ = R.check_fixture(fx, THR)
    assert gap > bound, (gap, bound)
    B = len(len_batch)
    off0 = np.r_[0, np.cumsum([a for a, _ in len_batch])].astype(int)
    off1 = np.r_[0, np.cumsum([b for _, b in len_batch])].astype(int)
    return {"F0": _g(fx["src_desc"]), "F1": _g(fx["tgt_desc"]), "B": B, "rows": int(off0[-1]),
            "off0": (ctypes.c_int * (B + 1))(*[int(x) for x in off0]), "off1": (ctypes.c_int * (B + 1))(*[int(x) for x in off1])}


def _ring_call(h, st, bt, retry):
    """One gmf_nn_match_batched into outputs of its own.  retry False: the entry itself, so a call the library refuses for want of
    workspace (it would have taken a ring slot, and Handle.call would repeat it) fails here instead of shifting the slots."""
    idx = torch.full((bt["rows"],), -1, device=DEV, dtype=torch.int32)
    dist = torch.full((bt["rows"],), float("nan"), device=DEV)
    args = (bt["F0"].data_ptr(), bt["F1"].data_ptr(), bt["off0"], bt["off1"], bt["B"], 32, 0, 0, idx.data_ptr(), dist.data_ptr(), st)
    if retry:
        h.call("gmf_nn_match_batched", *args)
    else:
        h.check(h.lib.gmf_nn_match_batched(h.h, *args), "gmf_nn_match_batched")
    return idx, dist


def test_back_to_back_calls_wrap_the_table_ring_and_regrow_its_slots():
    """Twenty gmf_nn_match_batched calls on one handle and one stream with no synchronisation between them, over a batch whose host
    table fits a fresh 2 KiB slot (X: 4 x 48 B) and one whose table does not (Y: 101 x 48 B).  The handle is given its workspace
    beforehand, so every call succeeds at once and call i takes slot i % 8 of the ring.  The batches alternate in runs of eight (X
    for calls 0-7, Y for 8-15, X for 16-19; alternating call by call would tie each table to the slots of one parity, which then
    would never regrow and would be rewritten with the bytes they already hold).  So every slot is taken at least twice, always
    with its earlier upload's event pending and always for the other batch's table, and each of the eight slots is regrown by a Y
    call from a 2 KiB block that X filled.  Every call writes its own outputs; all X results are one set of bits, all Y results
    another, and both are those of a call alone on a fresh handle."""
    from gmf_amd import _lib
    X = _ring_batch([(20, 33), (40, 25), (31, 40)], 0)
    Y = _ring_batch([((7 * b) % 5, 1 + (3 * b) % 4) for b in range(100)], 0)      # 1-4 rows; every fifth pair has no query rows
    assert X["B"] == 3 and (X["B"] + 1) * 48 <= 2048 and Y["B"] == 100 and (Y["B"] + 1) * 48 > 2048
    kinds = [(X, Y)[(i // 8) % 2] for i in range(20)]
    for s in range(8):                                        # what the docstring says of the order, slot by slot
        held = kinds[s::8]
        assert len(held) >= 2 and all(a is not b for a, b in zip(held, held[1:])) and held[0] is X and held[1] is Y
    st = torch.cuda.current_stream().cuda_stream
    h = _lib.Handle(0)
    h._ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)           # far more than either batch needs
    h.check(h.lib.gmf_set_workspace(h.h, h._ws.data_ptr(), h._ws.numel()), "gmf_set_workspace")
    outs = [_ring_call(h, st, bt, False) for bt in kinds]
    fresh = [_lib.Handle(0), _lib.Handle(0)]                  # (alive until the synchronise)
    refs = [_ring_call(hf, st, bt, True) for hf, bt in zip(fresh, (X, Y))]
    torch.cuda.synchronize()
    first = {id(X): outs[0], id(Y): outs[8]}
    for i, (idx, dist) in enumerate(outs):
        for want_idx, want_dist in (first[id(kinds[i])], refs[kinds[i] is Y]):
            assert torch.equal(idx, want_idx) and _same_bits(dist, want_dist), i
    for (idx, dist), bt in zip(refs, (X, Y)):
        assert int(idx.min()) >= 0 and bool(torch.isfinite(dist).all()) and idx.shape[0] == bt["rows"]
