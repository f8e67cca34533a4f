"""An exact restatement of the maximum-clique baseline of gmf_amd/clique.py (`max_clique_batched`, `PMC`, `compatibility_graph`;
kernels csrc/clique_kernels.hip).  Per pair of N correspondences:

  1. the graph, in float32 with every operation rounded on its own: a = ((dx^2 + dy^2) + dz^2) on the differences of columns 0..2
     of two rows, b alike on columns 3..5; "squared": edge iff |a - b| < float32(threshold) (the reference's rule,
     baseline_3DMatch.py:56-77); "length": edge iff |sqrt(a) - sqrt(b)| < float32(threshold).  No diagonal.
  2. omega and ALL maximum cliques of that graph: a bitset branch and bound on Python integers with the greedy colour bound,
     which cuts a branch only when it cannot reach the best size so far, so ties are kept.

The device may return any one maximum clique; tests/test_gpu_clique.py checks membership in the set from here.  Nothing here is
code under test."""
import functools

import numpy as np

from gmf_amd import synthetic
from spectral_reference import KINDS

METRICS = ("squared", "length")
# (seed, N) of the cases the GPU tests use, in both kinds; the length metric is served at (3, 257)
TABLE = [(1, 64), (2, 130), (3, 257), (4, 300), (6, 300)]
MAX_TIES = 10_000


def graph_np(corr, thr, metric="squared"):
    """The [N, N] boolean adjacency in numpy's float32."""
    assert metric in METRICS
    c = np.asarray(corr, np.float32)
    d = c[:, None, :] - c[None, :, :]
    sq = d * d
    a = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    b = (sq[..., 3] + sq[..., 4]) + sq[..., 5]
    if metric == "length":
        a, b = np.sqrt(a), np.sqrt(b)
    assert a.dtype == np.float32
    A = np.abs(a - b) < np.float32(thr)
    np.fill_diagonal(A, False)
    return A


def bit_rows(A):
    """[N, ceil(N / 64)] int64: bit j % 64 of word j / 64 of row i = A[i, j]; the bits past column N - 1 are zero."""
    N = A.shape[0]
    W = (N + 63) // 64
    padded = np.zeros((N, W * 64), np.uint8)
    padded[:, :N] = A
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).view(np.int64).reshape(N, W)


def _rows_as_ints(A):
    return [int.from_bytes(np.packbits(r, bitorder="little").tobytes(), "little") for r in np.asarray(A, bool)]


def _colours(P, adj):
    """Colours the greedy sequential colouring of P uses: no clique of P is larger."""
    n, U = 0, P
    while U:
        n += 1
        Q = U
        while Q:
            v = (Q & -Q).bit_length() - 1
            U &= ~(1 << v)
            Q &= ~(adj[v] | (1 << v))
    return n


def max_cliques(A):
    """(omega, the sorted list of all maximum cliques as sorted tuples, branch steps) of the boolean adjacency A."""
    adj = _rows_as_ints(A)
    N = len(adj)
    if N == 0:
        return 0, [], 0
    state = {"best": 0, "found": [], "steps": 0}
    # a greedy clique first, so that the bound cuts from the start: from every vertex, the candidate of largest degree each time
    deg = [bin(r).count("1") for r in adj]
    for s in range(N):
        size, P = 1, adj[s]
        while P:
            u = max((v for v in range(N) if (P >> v) & 1), key=lambda v: deg[v])
            size, P = size + 1, P & adj[u]
        state["best"] = max(state["best"], size)

    def expand(R, P):
        while P:
            state["steps"] += 1
            if len(R) + _colours(P, adj) < state["best"]:
                return
            v = (P & -P).bit_length() - 1
            P &= ~(1 << v)
            Pv = P & adj[v]
            if Pv:
                expand(R + [v], Pv)
            elif len(R) + 1 > state["best"]:
                state["best"], state["found"] = len(R) + 1, [tuple(R + [v])]
            elif len(R) + 1 == state["best"]:
                state["found"].append(tuple(R + [v]))

    expand([], (1 << N) - 1)
    found = sorted(c for c in state["found"] if len(c) == state["best"])
    return state["best"], found, state["steps"]


def is_clique(A, members):
    m = np.asarray(members, np.int64)
    sub = A[np.ix_(m, m)]
    return bool((sub | np.eye(len(m), dtype=bool)).all())


def make_case(seed, N, kind):
    """(corr [N,6], src [N,3], tgt [N,3], inlier_threshold, gt_labels [N]) of synthetic_pair(seed, N, kind)."""
    p = synthetic.synthetic_pair(seed, N, kind)
    return p["corr_pos"], p["src_keypts"], p["tgt_keypts"], KINDS[kind][0], p["gt_labels"]


@functools.lru_cache(maxsize=None)
def reference(seed, N, kind, metric="squared"):
    """(case, adjacency, omega, the set of all maximum cliques) of one named case, computed once per process.  Read-only."""
    case = make_case(seed, N, kind)
    A = graph_np(case[0], case[3], metric)
    omega, cliques, steps = max_cliques(A)
    assert len(cliques) < MAX_TIES, (seed, N, kind, metric, len(cliques))
    assert all(is_clique(A, c) for c in cliques[:16])
    return case, A, omega, frozenset(cliques), steps


def self_test():
    """The restatement's own edge cases: a triangle plus a pendant, two disjoint 4-cliques, no edges, N = 1, N = 0."""
    A = np.zeros((4, 4), bool)
    for i, j in ((0, 1), (0, 2), (1, 2), (2, 3)):
        A[i, j] = A[j, i] = True
    assert max_cliques(A)[:2] == (3, [(0, 1, 2)])
    A = np.zeros((8, 8), bool)
    A[:4, :4] = A[4:, 4:] = True
    np.fill_diagonal(A, False)
    assert max_cliques(A)[:2] == (4, [(0, 1, 2, 3), (4, 5, 6, 7)])
    assert max_cliques(np.zeros((5, 5), bool))[:2] == (1, [(0,), (1,), (2,), (3,), (4,)])
    assert max_cliques(np.zeros((1, 1), bool))[:2] == (1, [(0,)])
    assert max_cliques(np.zeros((0, 0), bool))[:2] == (0, [])
    assert is_clique(A, (4, 5, 6, 7)) and not is_clique(A, (3, 4))
    # the graph: symmetric, no diagonal, float32; identical rows are all adjacent; the word layout
    c = make_case(1, 70, "3dmatch")[0]
    for metric in METRICS:
        G = graph_np(c, 0.1, metric)
        assert G.dtype == bool and np.array_equal(G, G.T) and not G.diagonal().any()
    assert graph_np(np.ones((3, 6), np.float32), 0.1).sum() == 6
    B = bit_rows(G)
    assert B.shape == (70, 2) and B.dtype == np.int64
    assert all(((int(B[i, j >> 6]) >> (j & 63)) & 1) == int(G[i, j]) for i in (0, 33, 69) for j in range(70))
    assert (B[:, 1].astype(np.uint64) >> np.uint64(6)).max() == 0
    return True
