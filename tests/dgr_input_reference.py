"""Float64 numpy restatement of the step between DGR's data loader and its inlier network, written from the behaviour
gmf_amd documents (gmf_amd/matching.py, gmf_amd/dgr.py): the per-pair nearest-neighbour loop, the hashed
pair keys with their membership test, the radius pair search and the assembly of the inlier network's rows and features."""
import numpy as np


def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


# ---- nearest neighbours ----------------------------------------------------------------------------------------------------------

def nearest(F0, F1):
    """argmin_j |f0_i - f1_j|^2 in float64, the first index among equal distances -> (idx [N0], d2 [N0])."""
    F0 = np.asarray(F0, np.float64)
    F1 = np.asarray(F1, np.float64)
    d2 = ((F0[:, None, :] - F1[None, :, :]) ** 2).sum(-1)
    idx = d2.argmin(1)
    return idx, d2[np.arange(len(F0)), idx]


def find_pairs(F0, F1, len_batch):
    """Per pair the [N0, 2] rows (i, nearest j), local to the pair."""
    out, a, b = [], 0, 0
    for n0, n1 in len_batch:
        idx, _ = nearest(F0[a:a + n0], F1[b:b + n1]) if n0 else (np.zeros(0, np.int64), None)
        out.append(np.stack([np.arange(n0, dtype=np.int64), idx.astype(np.int64)], 1))
        a, b = a + n0, b + n1
    return out


# ---- labels -----------------------------------------------------------------------------------------------------------------------

def pair_keys(pairs, seed):
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return p[:, 0] + p[:, 1] * np.int64(seed)


def correct_by_hash(pos_pairs, pred_pairs, hash_seed=None, len_batch=None):
    """The key-and-isin labelling: seed = max(N0, N1) of the pair unless hash_seed is given."""
    out = []
    for b, (pos, pred) in enumerate(zip(pos_pairs, pred_pairs)):
        seed = max(len_batch[b]) if hash_seed is None else hash_seed
        out.append(np.isin(pair_keys(pred, seed), pair_keys(pos, seed)))
    return np.concatenate(out) if out else np.zeros(0, bool)


def correct_by_set(pos_pairs, pred_pairs):
    """Plain set membership of the (i, j) tuples: what the hash computes when the seed exceeds every index."""
    out = []
    for pos, pred in zip(pos_pairs, pred_pairs):
        s = {(int(i), int(j)) for i, j in np.asarray(pos).reshape(-1, 2)}
        out.append(np.array([(int(i), int(j)) in s for i, j in np.asarray(pred).reshape(-1, 2)], bool))
    return np.concatenate(out) if out else np.zeros(0, bool)


# ---- ground-truth pairs ------------------------------------------------------------------------------------------------------------

def transformed(xyz0, T):
    """p = ((T[r, 0] x + T[r, 1] y) + T[r, 2] z) + T[r, 3] in float64, in this order."""
    x = np.asarray(xyz0, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], 1)


def squared_distances(xyz0, xyz1, T):
    """d2 [N0, N1] = ((p0 - q0)^2 + (p1 - q1)^2) + (p2 - q2)^2 in float64, in this order."""
    p = transformed(xyz0, T)
    q = np.asarray(xyz1, np.float32).astype(np.float64)
    d = p[:, None, :] - q[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def matching_indices(xyz0, off0, xyz1, off1, T, radius):
    """-> (pairs [K, 2] int64, pair_offsets [B + 1]): (i, j) local to the pair with d2 < radius^2, by i then j."""
    r2 = np.float64(radius) * np.float64(radius)
    parts, counts = [], []
    for b in range(len(off0) - 1):
        d2 = squared_distances(xyz0[off0[b]:off0[b + 1]], xyz1[off1[b]:off1[b + 1]], T[b])
        ij = np.argwhere(d2 < r2).astype(np.int64)                # row-major: by i, then j
        parts.append(ij.reshape(-1, 2))
        counts.append(len(ij))
    return np.concatenate(parts), offsets(counts)


def radius_margin(xyz0, off0, xyz1, off1, T, radius):
    """The smallest |d2 - radius^2| / radius^2 over all candidate pairs of the batch: the inputs' distance from a tie."""
    r2 = float(radius) ** 2
    m = np.inf
    for b in range(len(off0) - 1):
        d2 = squared_distances(xyz0[off0[b]:off0[b + 1]], xyz1[off1[b]:off1[b + 1]], T[b])
        if d2.size:
            m = min(m, float(np.abs(d2 - r2).min()) / r2)
    return m


# ---- rows and features --------------------------------------------------------------------------------------------------------------

def inlier_input(iC0, iC1, len_batch, pred_pairs, feature_type, F0=None, F1=None, xyz0=None, xyz1=None):
    """reg_coords [M, 7] = (iC0[ind0], iC1[ind1, 1:]) and reg_feats (float64) over the predicted pairs of the batch, ind0 / ind1
    the pairs' rows in the packed tensors."""
    off0 = offsets([n for n, _ in len_batch])
    off1 = offsets([n for _, n in len_batch])
    ind0 = np.concatenate([p[:, 0] + off0[b] for b, p in enumerate(pred_pairs)])
    ind1 = np.concatenate([p[:, 1] + off1[b] for b, p in enumerate(pred_pairs)])
    coords = np.concatenate([np.asarray(iC0)[ind0], np.asarray(iC1)[ind1, 1:]], 1)
    if feature_type == "ones":
        feats = np.ones((len(ind0), 1))
    elif feature_type == "feats":
        feats = np.concatenate([np.asarray(F0, np.float64)[ind0], np.asarray(F1, np.float64)[ind1]], 1)
    elif feature_type == "coords":
        feats = np.concatenate([np.cos(np.asarray(xyz0, np.float32).astype(np.float64)[ind0]),
                                np.cos(np.asarray(xyz1, np.float32).astype(np.float64)[ind1])], 1)
    else:
        raise ValueError("Inlier feature type not defined")
    return coords, feats
